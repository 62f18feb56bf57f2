"""The crafted clouds of tests/helpers/nn_search_cases.py on the CPU: every case is held to the property it is there for, stated on the
brute-force oracle's answer (oracle.nn_search: fp32 (dx*dx + dy*dy) + dz*dz, lowest index on ties) and without the library's cell rule,
and the fp32 oracle itself is tied to a float64 minimum.  tests/test_gpu_nn_search_crafted.py runs the same cases on the device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import nn_search_cases as nc  # noqa: E402

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def answers(oracle):
    """case name -> (case, oracle's idx, sqdist, within), computed once"""
    return {c.name: (c,) + tuple(nc.expected(oracle, c)) for c in nc.all_small_cases()}


def test_case_names_are_unique_and_arrays_are_float32(answers):
    cases = nc.all_small_cases()
    assert len({c.name for c in cases}) == len(cases) == len(answers)
    for c in cases:
        assert c.map.dtype == F and c.query.dtype == F and c.map.shape[1:] == (3,) and c.query.shape[1:] == (3,)
        assert np.isfinite(c.map).all() and np.isfinite(c.query).all()
    again = nc.all_small_cases()
    assert all(a.map.tobytes() == b.map.tobytes() and a.query.tobytes() == b.query.tobytes() for a, b in zip(cases, again))


def test_oracle_winner_is_the_float64_minimum(answers):
    """the fp32 reference against a high-precision one: the winner's float64 distance is within 1e-6 relative of the float64 minimum"""
    for name, (c, idx, sq, within) in answers.items():
        m, q = c.map.astype(np.float64), c.query.astype(np.float64)
        for lo in range(0, len(q), 256):
            d = np.sqrt(((q[lo:lo + 256, None, :] - m[None]) ** 2).sum(axis=2))
            won = d[np.arange(d.shape[0]), idx[lo:lo + 256]]
            least = d.min(axis=1)
            assert (won <= least * (1 + 1e-6)).all(), name
            # and the fp32 squared distance it reports is that distance's square (4 roundings of 2^-24 each, far below 1e-6)
            assert np.allclose(sq[lo:lo + 256], won * won, rtol=1e-6, atol=1e-30), name


@pytest.mark.parametrize("radius", nc.SLIVER_RADII)
def test_sliver_pairs_are_inside_and_at_the_rim(answers, radius):
    assert len(nc.SLIVER[radius]) >= (4 if radius in (0.3, 0.35) else 0)
    r64 = np.float64(F(radius))
    for axis in range(3):
        c, idx, sq, within = answers[f"sliver radius {radius} axis {axis}"]
        assert (c.map.min(axis=0) == nc.ORIGIN).all() and (c.map[0] == nc.ORIGIN).all()
        for qi, mi in c.meta["pairs"]:
            sep = np.float64(c.query[qi, axis]) - np.float64(c.map[mi, axis])
            assert idx[qi] == mi and within[qi] == 1 and sq[qi] < F(radius) * F(radius), (axis, qi)
            assert (1 - 3e-5) * r64 <= sep < r64 and (np.delete(c.query[qi], axis) == np.delete(c.map[mi], axis)).all(), (axis, qi)
        for qi, pi, ai in c.meta["nearer"]:
            dp, da = nc.sqdist(c.map[pi], c.query[qi]), nc.sqdist(c.map[ai], c.query[qi])
            assert dp < da < F(radius) * F(radius) and idx[qi] == pi and within[qi] == 1, (axis, qi)
            assert c.map[ai, axis] == c.query[qi, axis], "A lies on another axis"
        assert {pi < ai for _, pi, ai in c.meta["nearer"]} == ({True, False} if c.meta["nearer"] else set())
        block = c.meta["block"]
        assert len(block) == nc.SLIVER_BLOCK >= 200
        k = np.arange(1, len(block) + 1)
        sep = c.query[block, axis].astype(np.float64) - c.map[idx[block], axis].astype(np.float64)
        # the separations asked for, up to the rounding of p to fp32 (q is an fp32 value before p is derived from it)
        ulp = np.spacing(np.maximum(np.abs(c.query[block, axis]), np.abs(c.map[idx[block], axis]))).astype(np.float64)
        assert (np.abs(sep - r64 * (1 - k * 2.0 ** -22)) <= ulp).all()


def test_edges_are_bit_equal_to_the_thresholds_they_name(answers):
    for threshold, radius in nc.EDGE_CALLS:
        T = nc.f32(nc.THRESHOLDS[threshold][0])
        if threshold.startswith("r2"):
            assert _bits(T) == _bits(F(radius) * F(radius))
        else:
            cell = F(max(radius, 0.2))
            assert _bits(T) == _bits((F(0.99) * cell) * (F(0.99) * cell)) and T > 0
        want = {"below": np.nextafter(T, F(0)), "equal": T, "above": np.nextafter(T, F(np.inf))}
        for axis in range(3):
            c, idx, sq, within = answers[f"edge {threshold} axis {axis}"]
            seen = set()
            for qi, mi, which in c.meta["edges"]:
                assert idx[qi] == mi and _bits(sq[qi]) == _bits(want[which]) == _bits(c.meta["d2"][which]), (threshold, axis, qi)
                assert within[qi] == (1 if sq[qi] < F(radius) * F(radius) else 0)
                seen.add(which)
            assert seen == {"below", "equal", "above"}
            if threshold.startswith("r2"):       # strictly below is inside, equal is not
                assert [int(within[qi]) for qi, _, w in c.meta["edges"] if w != "below"] == [0] * 8
                assert [int(within[qi]) for qi, _, w in c.meta["edges"] if w == "below"] == [1] * 4


def test_ties_share_the_minimal_distance_bit_for_bit(answers):
    names = [n for n, (c, *_) in answers.items() if "tie" in c.meta]
    assert len(names) >= 11
    for name in names:
        c, idx, sq, within = answers[name]
        for reverse in (False, True):
            m = c.map[::-1] if reverse else c.map
            for qi, tied in c.meta["tie"]:
                d = nc.sqdist(m, c.query[qi][None])
                at = [len(m) - 1 - t for t in tied] if reverse else list(tied)
                assert len(at) >= 2 and len({int(b) for b in _bits(d[at])}) == 1 and _bits(d[at[0]]) == _bits(d.min()), (name, qi)
                assert sorted(np.flatnonzero(d == d.min()).tolist()) == sorted(at), (name, qi)
                if not reverse:
                    assert idx[qi] == min(tied) and _bits(sq[qi]) == _bits(d.min())
    c = answers["duplicated map points"][0]
    assert max(max(t) - min(t) for _, t in c.meta["tie"]) >= 2000            # far-apart indices, and one pair across the 2048 tile bound
    c, idx, sq, _ = answers["list tie axis 0 outside first"]
    assert sq[0] == F(0.0625) > nc.f32(nc.THRESHOLDS["h2 of cell 0.2"][0])


def test_face_values_sit_on_the_faces(answers):
    for radius in (0.15, 0.3):
        cell = F(max(radius, 0.2))
        v = nc.face_values(cell)
        assert len(v) == 22 and np.signbit(v[-1]) and v[-1] == 0
        for k in range(-3, 4):
            x = F(k) * cell
            lo, at, hi = v[3 * (k + 3):3 * (k + 3) + 3]
            assert _bits(at) == _bits(x) and lo < at < hi and np.nextafter(lo, F(np.inf)) == at == np.nextafter(hi, F(-np.inf))
        assert (v < 0).sum() >= 10 and (v > 0).sum() >= 10              # both sides of the device form's origin
        for axis in range(3):
            c = answers[f"cell faces radius {radius} axis {axis}"][0]
            assert np.array_equal(_bits(c.map[:, axis]), _bits(v)) and np.array_equal(_bits(c.query[:22, axis]), _bits(v))


def test_hash_cases_do_what_they_are_named_for(answers):
    c = answers["aliased buckets"][0]
    assert len(c.map) == 40                                                  # 1024 buckets (grid_buckets: about two per point, 1024 at least)
    b = nc.buckets27(c.query, 0.2, 1023)
    assert any(len(set(row.tolist())) < 27 for row in b), "no query probes a bucket twice"
    c, idx, sq, within = answers["one bucket"]
    cells = c.meta["cells"]
    assert len(cells) == 30 == len(np.unique(cells, axis=0)) and len(set(nc.cell_bucket(cells, 1023).tolist())) == 1
    assert np.array_equal(np.floor(c.map * F(5)).astype(np.int64), cells)
    apart = np.abs(cells[:, None] - cells[None]).max(axis=2)
    assert apart[~np.eye(30, dtype=bool)].min() >= 3                         # no two of them within each other's 27 cells
    assert idx[:30].tolist() == list(range(30)) and within[:30].all()
    c = answers["hash products wrap"][0]
    cells = np.floor(c.map * F(5)).astype(np.int64)
    assert (np.abs(cells * np.array([73856093, 19349663, 83492791])) > 2 ** 32).all() and (cells[:, 0] < 0).all() and (cells[:, 2] < 0).all()


def test_list_cases_are_far_from_the_map(answers):
    for n in nc.LIST_MAP_SIZES:
        for k in nc.LIST_LENGTHS:
            c, idx, sq, within = answers[f"list n_map {n} n_query {k}"]
            assert len(c.map) == n and len(c.query) == k and sq.min() >= 400 and not within.any()
            if n > 1:
                d = nc.sqdist(c.map, c.query[0][None])
                assert idx[0] == 0 and d[0] == d[n - 1] == d.min()                  # the repeated point ties with the first


def test_far_case_is_inside_half_the_stated_bound(answers):
    c, idx, sq, within = answers["far coordinates"]
    cell = 0.2
    reach = max(np.abs(c.map).max(), np.abs(c.query).max()) / cell
    assert 0.2 * nc.NN_MAX_CELLS < reach <= 0.5 * nc.NN_MAX_CELLS
    assert 0 < within.sum() < len(c.query) and (sq > 100).sum() == 40
