"""SSC::refineClusterByIntensity (src/ssc.cpp:571-635) on the CPU: the literal restatement and the device's convention
(tests/helpers/intensity_merge_ref.py) on hand-built scans with known answers, the two against each other on small synthetic
scenes, and the C-ABI entry points of the stage.  Not gpu."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import intensity_merge_ref as imr  # noqa: E402

YAML = dict(search_c=2, diff=2.0, cov_max=1.0)      # config/semantickitti.yaml, config/parkinglot.yaml
DEFAULTS = dict(search_c=2, diff=50.0, cov_max=20.0)  # utility.h:305-309 when the YAML omits the keys


def _scan(grid, voxels):
    """voxels: (range, sector, azimuth, av, cov, cluster tag) with one point each, in point order.  Returns the voxel table, the
    canonical names and running numbers (tag + 5) of the points."""
    R, S, Az = grid
    keys = [r * S + s + a * R * S for r, s, a, *_ in voxels]
    order = np.argsort(keys, kind="stable")
    vox = dict(vox_key=np.array(keys)[order], vox_pt_begin=np.arange(len(voxels) + 1), vox_pts=order,
               vox_av=np.array([v[3] for v in voxels], np.float32)[order], vox_cov=np.array([v[4] for v in voxels], np.float32)[order],
               idx3=np.array([v[:3] for v in voxels])[order])
    tags = np.array([v[5] for v in voxels])
    return vox, imr.canonical(tags), tags + 5


def _both(grid, voxels, iterations=1, **kw):
    vox, names, running = _scan(grid, voxels)
    p = dict(YAML)
    p.update(kw)
    conv = imr.convention(vox, names, grid, iterations, p["search_c"], p["diff"], p["cov_max"])
    lit = imr.literal(vox, running, grid, iterations, p["search_c"], p["diff"], p["cov_max"])
    assert np.array_equal(imr.canonical(lit), conv)
    return conv


G = (20, 20, 4)


def test_two_clusters_one_empty_voxel_apart_fuse():
    vs = [(5, 5, 1, 10.0, 0.0, 0), (5, 7, 1, 10.0, 0.0, 1)]
    assert len(set(_both(G, vs))) == 1
    assert len(set(_both(G, vs, search_c=1))) == 2       # the gap is beyond a radius of one


def test_cov_above_the_limit_blocks_the_fusion():
    vs = [(5, 5, 1, 10.0, 0.0, 0), (5, 7, 1, 10.0, 1.5, 1)]
    assert len(set(_both(G, vs))) == 2
    assert len(set(_both(G, vs, cov_max=1.5))) == 1      # <= (ssc.cpp:591)


def test_intensity_difference_above_the_limit_blocks_the_fusion():
    vs = [(5, 5, 1, 10.0, 0.0, 0), (5, 7, 1, 12.5, 0.0, 1)]
    assert len(set(_both(G, vs))) == 2
    assert len(set(_both(G, vs, diff=2.5))) == 1


def test_search_radius_is_one_beyond_six_tenths_of_the_range_bins():
    near = [(4, 5, 1, 10.0, 0.0, 0), (6, 5, 1, 10.0, 0.0, 1)]
    far = [(14, 5, 1, 10.0, 0.0, 0), (16, 5, 1, 10.0, 0.0, 1)]   # 14 > 0.6 * 20: radius 1 for both voxels
    assert len(set(_both(G, near))) == 1
    assert len(set(_both(G, far))) == 2
    edge = [(12, 5, 1, 10.0, 0.0, 0), (14, 5, 1, 10.0, 0.0, 1)]  # 12 is not > 12: the first voxel still looks two bins out
    assert len(set(_both(G, edge))) == 1


def test_grid_is_clipped_without_sector_wrap():
    wrap = [(5, 0, 1, 10.0, 0.0, 0), (5, 19, 1, 10.0, 0.0, 1)]
    assert len(set(_both(G, wrap))) == 2
    low = [(0, 0, 0, 10.0, 0.0, 0), (1, 2, 0, 10.0, 0.0, 1)]     # corner of the grid: clipped windows still find the neighbour
    assert len(set(_both(G, low))) == 1


def test_cluster_outside_its_own_set_stays_and_fuses_the_others():
    # C's only voxel fails the cov test: S(C) = {A, B} without C.  Visiting order (descending key): B, C, A.  C records the fusion
    # of A and B and stays a cluster of its own (ssc.cpp:600-609: c itself need not be in neighbor_name)
    vs = [(5, 2, 1, 10.0, 0.0, 0), (5, 4, 1, 10.0, 5.0, 1), (5, 6, 1, 10.0, 0.0, 2)]
    got = _both(G, vs, iterations=3)
    assert got[0] == got[2] and got[1] != got[0]


def test_three_cluster_chain_visiting_order_decides():
    # A (sector 2), B (4), C (6): the largest key is visited first, C fuses {B, C}; B is invalid; A's set {A, B} minus the
    # invalid names is {A}.  (Ascending order would have fused {A, B} instead.)
    vs = [(5, 2, 1, 10.0, 0.0, 0), (5, 4, 1, 10.0, 0.0, 1), (5, 6, 1, 10.0, 0.0, 2)]
    got = _both(G, vs, iterations=1)
    assert got[1] == got[2] and got[0] != got[1]
    got = _both(G, vs, iterations=2)                     # the second pass fuses A with {B, C}
    assert len(set(got)) == 1


def _synthetic_scenes():
    import synth
    rng = np.random.default_rng(7)
    for seed in range(6):
        kind = ("K64", "PARK")[seed % 2]
        pts, _, _ = synth.make_scan(3 + seed, 5 + 3 * seed, kind)
        x = pts.numpy()
        x = x[rng.random(len(x)) < 0.04]      # a few thousand points: the oracle's clustering loop is quadratic
        yield kind, x


@pytest.mark.parametrize("params", [YAML, DEFAULTS], ids=["yaml", "defaults"])
def test_literal_equals_convention_in_the_first_iteration(oracle, params):
    import scvod_py
    report = []
    for kind, x in _synthetic_scenes():
        P = scvod_py.make_params("semantickitti" if kind == "K64" else "parkinglot")
        grid = tuple(int(g) for g in oracle.grid_dims(P)[:3])
        apri = oracle.bin(P, x)["apri"]
        vox = oracle.voxelize(P, apri)
        running, _, _ = oracle.cluster(P, apri)
        names = imr.canonical(running)
        st = {}
        conv = imr.convention(vox, names, grid, 1, params["search_c"], params["diff"], params["cov_max"], stats=st)
        lit = imr.literal(vox, running, grid, 1, params["search_c"], params["diff"], params["cov_max"])
        assert np.array_equal(imr.canonical(lit), conv), kind
        for it in (2, 3):
            c = imr.convention(vox, names, grid, it, params["search_c"], params["diff"], params["cov_max"])
            l2 = imr.canonical(imr.literal(vox, running, grid, it, params["search_c"], params["diff"], params["cov_max"]))
            report.append((kind, it, int((c != l2).sum()), len(c)))
        report.append((kind, "fusions", st["fusions"], st["clusters_before"]))
    print("points that differ in iterations 2 / 3 (kind, iterations, differ, points):", report)


def test_capi_exports_the_intensity_merge(scvod):
    lib = scvod.load_lib()
    for name in ("scvod_set_intensity_merge", "scvod_batch_cluster_merge_stats"):
        assert hasattr(lib, name), name
    assert lib.scvod_set_intensity_merge(None, 3, 2, 2.0, 1.0) == -1      # SCVOD_ERR_INVALID without a ctx
    assert lib.scvod_batch_cluster_merge_stats(None, None) == -1
