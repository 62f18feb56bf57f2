"""scvod_map_filter / scvod_batch_map_filter / scvod_map_filter_stats / scvod_map_filter_scratch_bytes without a GPU: the symbols,
constants and struct layouts, the NULL-map errors, and the numpy statement (tests/helpers/map_filter_ref.py) on properties worked out
by hand -- the partition's order, the sides without a vote, the integer vote rule at and around equality with products beyond int32,
min_points, OUT members and vote_num == 0.  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import map_filter_ref as mf  # noqa: E402
import map_query_ref as mq  # noqa: E402
import map_ref as mr  # noqa: E402

NEW = ("scvod_map_filter_params_default", "scvod_map_filter", "scvod_batch_map_filter", "scvod_map_filter_stats",
       "scvod_map_filter_scratch_bytes")
INVALID = -1
F = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "scvod.h")).read()


def test_symbols_declared_exported_and_listed(scvod):
    lib = scvod.load_lib()
    hdr = _header()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("filter", "filter_batch", "filter_stats", "filter_scratch_bytes"):
        assert callable(getattr(scvod.StaticMap, m))
    assert callable(scvod.map_filter_params_default)


def test_constants_and_struct_layouts(scvod):
    hdr = _header()
    for name, value in (("KNOWN", 0), ("NOVEL", 1), ("OUT", 2), ("OBJECT_VOTE", 1)):
        assert re.search(r"#define\s+SCVOD_MAPF_%s\s+%d\b" % (name, value), hdr)
        assert getattr(scvod, "MAPF_" + name) == value == getattr(mf, name)
    tile = int(re.search(r"#define\s+SCVOD_MAP_FILTER_TILE\s+(\d+)", hdr).group(1))
    assert tile == scvod.MAP_FILTER_TILE and tile % 256 == 0
    P = scvod.MapFilterParams
    assert C.sizeof(P) == 24
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("radius", 0), ("flags", 4), ("vote_num", 8), ("vote_den", 12),
                                                                 ("min_points", 16), ("reserved", 20)]
    p = scvod.map_filter_params_default()
    assert (p.radius, p.flags, p.vote_num, p.vote_den, p.min_points, p.reserved) == (0.0, 0, 1, 2, 1, 0)
    assert {n: getattr(p, n) for n, _ in P._fields_} == mf.params()
    q = scvod.map_filter_params_default(radius=0.05, flags=scvod.MAPF_OBJECT_VOTE, vote_num=3, vote_den=4, min_points=10)
    assert (q.flags, q.vote_num, q.vote_den, q.min_points) == (1, 3, 4, 10) and q.radius == F(0.05)
    raw = (C.c_uint8 * 24)(*([0xAA] * 24))
    scvod.load_lib().scvod_map_filter_params_default(C.cast(raw, C.POINTER(P)))
    assert bytes(raw) == bytes(p), "the defaults leave a byte of the struct unwritten"
    scvod.load_lib().scvod_map_filter_params_default(None)            # (NULL is ignored)
    D = scvod.MAP_FILTER_OBJECT_DTYPE
    assert D.itemsize == 32 == mf.OBJECT_DTYPE.itemsize and D == mf.OBJECT_DTYPE
    assert [D.fields[n][1] for n in ("n_cell", "n_near", "n_miss", "n_out", "n_points", "verdict", "reserved")] == [0, 4, 8, 12, 16, 20, 24]
    assert re.search(r"typedef struct scvod_map_filter_object\s*{[^}]*reserved\[2\]", hdr)


def test_a_null_map_is_invalid(scvod):
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.scvod_map_filter(None, p, p, 1, None, None, None, p, p, p, p, p, p, p, None) == INVALID
    assert lib.scvod_batch_map_filter(None, None, p, None, None, p, p, p, p, p, p, p, p, 1, None) == INVALID
    assert lib.scvod_batch_map_filter(p, None, p, None, None, p, p, p, p, p, p, p, p, 1, None) == INVALID     # (the ctx is not looked at)
    assert lib.scvod_map_filter_stats(None, p) == INVALID
    assert lib.scvod_map_filter_scratch_bytes(None) == 0
    assert not buf.any()


# ---------------------------------------------------------------- the helper

def _cloud(rng, n):
    cells = rng.integers(-6, 6, (n, 3))
    return np.concatenate([(cells + rng.uniform(0.1, 0.9, (n, 3))) * 0.2, rng.uniform(0, 255, (n, 1))], axis=1).astype(F), cells


def _table(rng, cells):
    c = np.unique(cells, axis=0)
    keys = mr.pack_key(c[:, 0], c[:, 1], c[:, 2])
    return mq.table_of(keys, mr.pack_val(*rng.integers(0, 65536, (4, len(keys)))))


def test_helper_order_is_a_sorted_permutation_and_side_follows_result():
    rng = np.random.default_rng(81)
    pts, cells = _cloud(rng, 3000)
    pts[[0, 700, 1999, 2000, 2999], 0] = [np.nan, 3.0e5, np.nan, -3.0e5, np.nan]
    offs = [0, 700, 700, 2000, 3000]
    table = _table(rng, cells[::3])
    pay = rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32)
    for radius in (0.0, mq.R_SMALL, mq.R_MAX):
        r = mf.filter(table, pts, offs, [mq.IDENTITY] * 4, 0.2, mf.params(radius=radius), False, None, payload=pay)
        q = mq.query(table, pts, offs, [mq.IDENTITY] * 4, 0.2, radius)
        assert np.array_equal(r["result"], q["result"])
        assert np.array_equal(r["side"], np.array([mf.NOVEL, mf.KNOWN, mf.KNOWN, mf.OUT], np.uint8)[q["result"]])   # a function of the byte alone
        assert r["votes"] is None and r["stats"].tolist()[4:] == [0, 0, 0, 0]
        assert r["stats"].tolist()[:4] == [3000, int(q["stats"][1] + q["stats"][2]), int(q["stats"][3]), 5]
        for s in range(4):
            a, b = offs[s], offs[s + 1]
            o = r["order"][a:b]
            assert sorted(o.tolist()) == list(range(b - a))
            k, kn = r["bounds"][s]
            assert 0 <= k <= kn <= b - a
            for seg, which in ((o[:k], mf.KNOWN), (o[k:kn], mf.NOVEL), (o[kn:], mf.OUT)):
                assert (np.diff(seg) > 0).all() and (r["side"][a + seg] == which).all()
            assert np.array_equal(r["xyzi"][a:b].view(np.uint32), pts[a + o].view(np.uint32))
            assert np.array_equal(r["payload"][a:b], pay[a + o])
        assert r["bounds"][1].tolist() == [0, 0] and (r["side"] == mf.OUT).sum() == 5
        assert 0 < r["stats"][1] < 3000 and r["stats"][2] > 0


def test_helper_vote_rule_at_and_around_equality_beyond_int32():
    # 40 000 members, vote_den 2^20: both products are about 2^35
    n, den = 40000, 1 << 20
    known = 12345
    num = known * den // n                                   # known * den >= num * n, with equality iff the division is exact
    assert known * den > (1 << 31) and num * n > (1 << 31)
    assert mf.object_known(known, 0, n, num, den)
    assert not mf.object_known(known, 0, n, num + 1, den)
    # exact equality: 30 000 of 40 000 at 3 / 4 scaled to the largest denominator
    assert 30000 * den == (3 * den // 4) * n
    assert mf.object_known(29000, 1000, n, 3 * den // 4, den)
    assert not mf.object_known(29000, 999, n, 3 * den // 4, den)
    assert mf.object_known(29000, 1001, n, 3 * den // 4, den)
    # a pair whose low 32 bits order the other way round: arithmetic that wrapped would answer KNOWN
    lo = lambda v: v & 0xFFFFFFFF                                   # noqa: E731
    assert 4095 * den < 4096 * den and lo(4095 * den) > lo(4096 * den)
    assert not mf.object_known(4095, 0, 4096, den, den) and mf.object_known(4096, 0, 4096, den, den)
    # through vote(): one object of n members, `known` of them CELL
    result = np.full(n, mq.MISS, np.uint8)
    result[:30000] = mq.CELL
    po = np.zeros(n, np.int64)
    for num_, verdict, moved in ((3 * den // 4, mf.KNOWN, [10000, 0, 1, 1]), (3 * den // 4 + 1, mf.NOVEL, [0, 30000, 1, 0])):
        side, votes, words = mf.vote(result, po, [n], mf.params(flags=1, vote_num=num_, vote_den=den))
        assert (side == verdict).all() and votes[0]["verdict"] == verdict and words == moved
        assert (votes[0]["n_cell"], votes[0]["n_near"], votes[0]["n_miss"], votes[0]["n_out"], votes[0]["n_points"]) == (30000, 0, 10000, 0, n)


def test_helper_min_points_out_members_and_vote_num_zero():
    # three objects of 5, 6 and 4 members, two points that are no members, OUT points inside the objects
    result = np.array([mq.CELL, mq.MISS, mq.MISS, mq.MISS, mq.OUT,            # object 0: 1 of 5 known
                       mq.NEAR, mq.CELL, mq.CELL, mq.MISS, mq.OUT, mq.CELL,   # object 1: 4 of 6 known
                       mq.MISS, mq.MISS, mq.MISS, mq.MISS,                    # object 2: 0 of 4
                       mq.MISS, mq.CELL], np.uint8)                           # no object
    po = np.array([0] * 5 + [1] * 6 + [2] * 4 + [-1, -1])
    objects = [5, 6, 4]
    own = mf.own_side(result)
    side, votes, words = mf.vote(result, po, objects, mf.params(flags=1))                      # 1 / 2
    assert votes["verdict"].tolist() == [mf.NOVEL, mf.KNOWN, mf.NOVEL]
    assert side.tolist() == [1, 1, 1, 1, 2] + [0, 0, 0, 0, 2, 0] + [1, 1, 1, 1] + [1, 0]
    assert words == [1, 1, 3, 1]
    assert (side[result == mq.OUT] == mf.OUT).all() and (side[po < 0] == own[po < 0]).all()     # a vote never moves an OUT member
    # min_points on both sides of an object's size
    side5, v5, w5 = mf.vote(result, po, objects, mf.params(flags=1, min_points=5))
    assert v5["verdict"].tolist() == [mf.NOVEL, mf.KNOWN, -1] and w5 == [1, 1, 2, 1]
    side6, v6, w6 = mf.vote(result, po, objects, mf.params(flags=1, min_points=6))
    assert v6["verdict"].tolist() == [-1, mf.KNOWN, -1] and (side6[:5] == own[:5]).all() and w6 == [1, 0, 1, 1]
    assert v6["n_cell"].tolist() == [1, 3, 0] and v6["n_miss"].tolist() == [3, 1, 4]            # the counts are still reported
    # vote_num == 0: every voting object is KNOWN, the one without a single known member too
    side0, v0, w0 = mf.vote(result, po, objects, mf.params(flags=1, vote_num=0, vote_den=7))
    assert v0["verdict"].tolist() == [mf.KNOWN] * 3 and w0 == [8, 0, 3, 3]
    assert (side0[(po >= 0) & (result != mq.OUT)] == mf.KNOWN).all() and (side0[result == mq.OUT] == mf.OUT).all()
    # vote_num == vote_den: KNOWN only when every member is (OUT members count against it)
    _, v1, _ = mf.vote(np.array([mq.CELL, mq.NEAR, mq.CELL, mq.OUT], np.uint8), [0, 0, 0, 1], [3, 1], mf.params(flags=1, vote_num=2, vote_den=2))
    assert v1["verdict"].tolist() == [mf.KNOWN, mf.NOVEL]


def test_helper_filter_with_objects_end_to_end():
    rng = np.random.default_rng(82)
    pts, cells = _cloud(rng, 600)
    offs = [0, 250, 600]
    table = _table(rng, cells[:300])                                # the first 300 points are known
    po = np.full(600, -1, np.int64)
    po[100:200], po[280:330], po[400:410] = 0, 1, 2
    r = mf.filter(table, pts, offs, [mq.IDENTITY] * 2, 0.2, mf.params(flags=1, min_points=20), False, None, po, [100, 50, 10])
    assert r["votes"]["verdict"].tolist() == [mf.KNOWN, mf.NOVEL if (r["result"][280:330] != mq.MISS).sum() * 2 < 50 else mf.KNOWN, -1]
    assert (r["side"][100:200] == mf.KNOWN).all()
    assert r["stats"][0] == 600 and r["stats"][1] + r["stats"][2] + r["stats"][3] == 600 and r["stats"][6] == 2
    assert np.array_equal(r["bounds"][:, 0], [(r["side"][:250] == 0).sum(), (r["side"][250:] == 0).sum()])
