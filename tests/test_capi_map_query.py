"""scvod_map_query / scvod_batch_map_query / scvod_map_query_stats / scvod_map_query_scratch_bytes without a GPU: the symbols and
constants, the NULL-map errors, the numpy statement (tests/helpers/map_query_ref.py) on cases worked out by hand, and -- what makes
the device's comparison against an exhaustive search meaningful -- that on the seeded clouds of tests/test_gpu_map_query.py the
27-cell answer IS the exhaustive answer.  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import map_query_ref as mq  # noqa: E402
import map_ref as mr  # noqa: E402

NEW = ("scvod_map_query", "scvod_batch_map_query", "scvod_map_query_stats", "scvod_map_query_scratch_bytes")
INVALID = -1
IDENT = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
F = np.float32


def test_symbols_declared_exported_and_listed(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("query", "query_batch", "query_stats", "query_scratch_bytes"):
        assert callable(getattr(scvod.StaticMap, m))
    for name, value in (("MISS", 0), ("CELL", 1), ("NEAR", 2), ("OUT", 3)):
        assert re.search(r"#define\s+SCVOD_MAPQ_%s\s+%d\b" % (name, value), hdr)
        assert getattr(scvod, "MAPQ_" + name) == value == getattr(mq, name)


def test_a_null_map_is_invalid(scvod):
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.scvod_map_query(None, p, p, 1, None, 0.0, None, p, p, None, None, p, None) == INVALID
    assert lib.scvod_batch_map_query(None, None, p, 0.0, None, p, p, None, None, p, None) == INVALID
    assert lib.scvod_batch_map_query(p, None, p, 0.0, None, p, p, None, None, p, None) == INVALID     # (the ctx is not looked at)
    assert lib.scvod_map_query_stats(None, p) == INVALID
    assert lib.scvod_map_query_scratch_bytes(None) == 0
    assert not buf.any()


def _one(table, pts, leaf, radius, **kw):
    pts = np.asarray(pts, F).reshape(-1, 4)
    return mq.query(table, pts, [0, len(pts)], [IDENT], leaf, radius, **kw)


def test_helper_on_a_cell_face():
    """leaf 0.25: x = 1.0 is the face between the cells 3 and 4 and belongs to cell 4 (floor)"""
    leaf = 0.25
    k3, k4 = int(mr.pack_key(3, 0, 0)), int(mr.pack_key(4, 0, 0))
    v3 = int(mr.pack_val(65535, 32767, 32767, 5))     # a representative right below the face, at the centre of its y and z
    v4 = int(mr.pack_val(0, 32767, 32767, 6))
    pt = [[1.0, 0.125, 0.125, 0.0]]
    r = _one({k3: v3, k4: v4}, pt, leaf, 0.0)
    assert r["result"].tolist() == [mq.CELL] and r["cell_val"].tolist() == [v4]
    r = _one({k3: v3}, pt, leaf, 0.0)
    assert r["result"].tolist() == [mq.MISS] and r["cell_val"].tolist() == [int(mq.PAD)]
    r = _one({k3: v3}, pt, leaf, 0.05)
    assert r["result"].tolist() == [mq.NEAR] and r["nn_key"].tolist() == [k3]
    # by hand: the representative's x is (3 + 65535.5 / 65536) * 0.25 = 1 - 0.5 / 65536 * 0.25; y and z are (0 + 32767.5 / 65536) * 0.25
    dx = 0.5 / 65536 * 0.25
    dy = 0.125 - 32767.5 / 65536 * 0.25
    assert abs(float(r["nn_sqdist"][0]) - (dx * dx + 2 * dy * dy)) < 1e-12
    assert r["scan_counts"].tolist() == [[0, 1, 0, 0]] and r["stats"].tolist() == [1, 0, 1, 0, 0]
    # an occupied own cell whose representative is farther than the radius: CELL, with an empty nn pair
    far = int(mr.pack_val(65535, 65535, 65535, 1))
    r = _one({k4: far}, pt, leaf, 0.05)
    assert r["result"].tolist() == [mq.CELL] and r["cell_val"].tolist() == [far]
    assert r["nn_key"].tolist() == [int(mq.PAD)] and np.isposinf(r["nn_sqdist"]).all()
    # the distance test is strict: a representative at exactly the radius does not count
    k0 = int(mr.pack_key(0, 0, 0))
    rep = mq.decode32(np.array([k0], np.uint64), np.array([v4], np.uint64), leaf)[0]
    radius = F(0.125)
    on = [[rep[0] + radius, rep[1], rep[2], 0.0]]
    assert mq.sqdist32(np.asarray(on, F)[:, :3], rep[None])[0] == radius * radius
    r = _one({k0: v4}, on, leaf, radius)
    assert r["result"].tolist() == [mq.CELL] and r["nn_key"].tolist() == [int(mq.PAD)] and np.isposinf(r["nn_sqdist"]).all()


def test_helper_on_a_tie_the_smaller_key_wins():
    keys, vals, q, small = mq.tie_case()
    rep = mq.decode32(keys, vals, 0.2)
    d = mq.sqdist32(q[:, :3], rep)
    assert d[0] == d[1] and 0 < d[0] < F(0.05) * F(0.05)
    for order in ((0, 1), (1, 0)):
        table = {int(keys[i]): int(vals[i]) for i in order}
        for radius in (0.05, F(0.99) * F(0.2)):
            for ex in (False, True):
                r = _one(table, q, 0.2, radius, exhaustive=ex)
                assert r["nn_key"].tolist() == [small] and r["nn_sqdist"][0] == d[0]
    assert small == int(mr.pack_key(4, 8, 2))


def test_helper_on_a_neighbour_beyond_the_cell_range():
    """the last cell of the x axis: its +1 neighbours do not exist, and a record whose key is what a wrapped neighbour key would be
    (bit 63 set, so no point can own it) is never a candidate"""
    leaf = 0.2
    top = (1 << 20) - 1
    x = F((top + 0.5) * 0.2)
    k, _, ok = mr.encode_points(IDENT, np.array([[x, 0.1, 0.1, 0]], F), leaf)
    assert ok.all() and mr.unpack_key(k)[0][0] == top
    wrapped = (np.uint64(1 << 21) << np.uint64(42)) | (np.uint64(mr.CELL_BIAS) << np.uint64(21)) | np.uint64(mr.CELL_BIAS)
    below = int(mr.pack_key(top - 1, 0, 0))
    table = {int(wrapped): int(mr.pack_val(0, 32768, 32768, 1))}
    r = _one(table, [[x, 0.1, 0.1, 0]], leaf, F(0.99) * F(leaf))
    assert r["result"].tolist() == [mq.MISS]
    table[below] = int(mr.pack_val(65535, 32768, 32768, 2))
    r = _one(table, [[x, 0.1, 0.1, 0]], leaf, F(0.99) * F(leaf))
    assert r["result"].tolist() == [mq.NEAR] and r["nn_key"].tolist() == [below]
    # beyond the range and NaN: no cell
    r = _one(table, [[3.0e5, 0, 0, 0], [np.nan, 0, 0, 0], [0, -3.0e5, 0, 0]], leaf, 0.05)
    assert r["result"].tolist() == [mq.OUT] * 3 and (r["cell_val"] == mq.PAD).all() and np.isposinf(r["nn_sqdist"]).all()


def test_helper_with_a_select_table():
    leaf = 0.2
    k_own, k_nb = int(mr.pack_key(10, 10, 10)), int(mr.pack_key(11, 10, 10))
    lab = lambda q, label: int(mr.pack_val(q, 32768, 32768, 0)) | (label << 8) | 9          # noqa: E731
    table = {k_own: lab(60000, 6), k_nb: lab(2000, 4)}
    pt = [[(10 + 0.95) * 0.2, 10.5 * 0.2, 10.5 * 0.2, 0]]
    r = _one(table, pt, leaf, 0.05, labelled=True)
    assert r["result"].tolist() == [mq.CELL] and r["cell_val"].tolist() == [table[k_own]]
    static = [v for v in range(256) if v != 6]
    r = _one(table, pt, leaf, 0.05, labelled=True, select=static)                          # the own cell is dynamic: it counts as empty
    assert r["result"].tolist() == [mq.NEAR] and r["cell_val"].tolist() == [int(mq.PAD)] and r["nn_key"].tolist() == [k_nb]
    r = _one(table, pt, leaf, 0.05, labelled=True, select=[6])
    assert r["result"].tolist() == [mq.CELL] and r["nn_key"].tolist() == [k_own]
    r = _one(table, pt, leaf, 0.05, labelled=True, select=[1])
    assert r["result"].tolist() == [mq.MISS]
    sel = np.zeros(256, np.uint8)
    sel[4] = 1
    assert _one(table, pt, leaf, 0.05, labelled=True, select=sel)["nn_key"].tolist() == [k_nb]
    with pytest.raises(AssertionError):
        _one(table, pt, leaf, 0.05, labelled=False, select=[6])


@pytest.mark.parametrize("case", mq.NEAREST_CASES, ids=lambda c: c["id"])
def test_27_cells_are_the_exhaustive_answer_on_the_seeded_clouds(case):
    """|coordinate| <= about 1010 m at leaf 0.2: fp32 rounding (6e-5 m) stays far below 0.01 * leaf"""
    ref = mq.nearest_reference(case)
    a, b = ref["cells27"], ref["exhaustive"]
    for name in ("result", "cell_val", "nn_key"):
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(a["nn_sqdist"].view(np.uint32), b["nn_sqdist"].view(np.uint32))
    assert np.array_equal(a["scan_counts"], b["scan_counts"])
    # the case is not empty: all three cell answers occur, and the nearest representative of an occupied cell is not always its own
    c = a["stats"]
    assert c[1] > 500 and c[2] > 100 and c[3] > 500 and c[4] == 0
    hit = a["nn_key"] != mq.PAD
    assert hit.sum() > 500 and (hit & (a["result"] == mq.CELL) & (a["nn_key"] != ref["own_key"])).sum() > 20
