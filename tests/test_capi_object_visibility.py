"""The objects' vote on the seen-through verdict (scvod_batch_object_visibility) without a GPU: the symbols, the two structs and the
defaults, the argument errors, and the numpy statement of the call (tests/helpers/object_visibility_ref.py) on cases worked out by hand.
A ctx cannot be created without a device, so the refusals are made on a NULL ctx here -- which is itself the first of them -- and once
more on a live ctx, with guard regions, in tests/test_gpu_object_visibility.py.  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import object_visibility_ref as ovr  # noqa: E402

NEW = ("scvod_object_visibility_params_default", "scvod_batch_object_visibility", "scvod_batch_object_visibility_stats",
       "scvod_batch_object_visibility_scratch_bytes")
INVALID = -1
U, K, S = ovr.UNTESTED, ovr.KEEP, ovr.SEEN_THROUGH
# (vote_num, verdict) with vote_den = 1 << 20 and sum_through = sum_agree = 4500 * 255: the two values next to 1 << 19 at which products
# cut to 32 bits give the other answer
OV_WRAP_CASES = ((523069, S), (524941, K))


def test_symbols_declared_exported_and_listed(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("batch_object_visibility", "batch_object_visibility_stats", "batch_object_visibility_scratch_bytes"):
        assert callable(getattr(scvod.Ctx, m))
    for name, value in (("POOL_PAIRS", 1), ("WITH_TRACK", 2), ("TILE", 2048)):
        assert re.search(rf"#define\s+SCVOD_OBJVIS_{name}\s+{value}\b", hdr) and getattr(scvod, "OBJVIS_" + name) == value
    assert (ovr.POOL_PAIRS, ovr.WITH_TRACK, ovr.TILE) == (scvod.OBJVIS_POOL_PAIRS, scvod.OBJVIS_WITH_TRACK, scvod.OBJVIS_TILE)
    assert tuple(scvod.OBJVIS_STATS) == ovr.STATS and len(ovr.STATS) == 8
    assert "NOT from real data" in hdr[hdr.index("SCVOD_OBJVIS_POOL_PAIRS") - 6000:]


def test_struct_sizes_and_defaults(scvod):
    assert C.sizeof(scvod.ObjectVisibilityParams) == 32
    assert scvod.OBJECT_VISIBILITY_DTYPE.itemsize == 48 and scvod.OBJECT_VISIBILITY_DTYPE == ovr.DTYPE
    p = scvod.object_visibility_params_default()
    got = {k: getattr(p, k) for k in ovr.DEFAULTS}
    assert got == ovr.DEFAULTS == dict(flags=0, min_points=1, min_tested=1, min_through=2, vote_num=1, vote_den=2)
    assert list(p.reserved) == [0, 0]
    scvod.load_lib().scvod_object_visibility_params_default(None)   # a NULL struct is ignored
    assert scvod.object_visibility_params_default(flags=3, min_tested=5).min_tested == 5


def test_argument_errors_need_no_device(scvod):
    """SCVOD_ERR_INVALID with no device present, and nothing is written"""
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = C.c_void_p(buf.ctypes.data)
    odd2, odd4 = C.c_void_p(buf.ctypes.data + 2), C.c_void_p(buf.ctypes.data + 4)
    good = scvod.object_visibility_params_default()
    call = lib.scvod_batch_object_visibility
    assert call(None, p, p, p, C.byref(good), p, 4, None, None) == INVALID
    assert call(None, p, p, p, None, p, 4, None, None) == INVALID                        # no params either
    assert call(None, None, p, p, C.byref(good), p, 4, None, None) == INVALID            # NULL d_verdict
    bad_reserved = scvod.object_visibility_params_default()
    bad_reserved.reserved[1] = 1
    for bad in [scvod.object_visibility_params_default(**kw) for kw in (
            dict(flags=4), dict(flags=-1), dict(min_points=0), dict(min_tested=0), dict(vote_den=0), dict(vote_den=(1 << 20) + 1),
            dict(vote_num=-1), dict(vote_num=(1 << 20) + 1))] + [bad_reserved]:
        assert call(None, p, p, p, C.byref(bad), p, 4, None, None) == INVALID
    pool, track = scvod.object_visibility_params_default(flags=1), scvod.object_visibility_params_default(flags=2)
    assert call(None, p, None, p, C.byref(pool), p, 4, None, None) == INVALID            # POOL_PAIRS without d_votes
    assert call(None, p, p, None, C.byref(track), p, 4, None, None) == INVALID           # WITH_TRACK without d_objects
    assert call(None, p, p, p, C.byref(good), p, -1, None, None) == INVALID              # cap_records < 0
    assert call(None, p, odd2, p, C.byref(good), p, 4, None, None) == INVALID            # misaligned
    assert call(None, p, p, p, C.byref(good), odd2, 4, None, None) == INVALID
    assert call(None, p, p, odd4, C.byref(good), p, 4, None, None) == INVALID
    assert call(None, p, None, None, C.byref(good), None, 0, C.c_void_p(buf.ctypes.data + 1), None) == INVALID   # a partial overlap
    assert lib.scvod_batch_object_visibility_stats(None, p) == INVALID
    assert lib.scvod_batch_object_visibility_scratch_bytes(None) == 0
    assert not buf.any()


# ---- the helper on cases worked out by hand --------------------------------------------------------------------------------------------

def _one(n_seen, n_keep, n_untested=0, other_byte=U):
    """one object and two points of no object: (point_object, verdict bytes)"""
    v = np.array([S] * n_seen + [K] * n_keep + [other_byte] * n_untested + [S, K], np.uint8)
    po = np.array([0] * (n_seen + n_keep + n_untested) + [-1, -1], np.int32)
    return po, v


def _verdict(r):
    return int(r["records"]["verdict"][0]), int(r["records"]["how"][0])


def test_rule_at_equality_and_one_below_on_verdict_bytes():
    po, v = _one(3, 5, 2)                                       # t = 3, a = 5: 3 * den >= num * 8
    r = ovr.run(po, 1, v, p=ovr.params(vote_num=3, vote_den=8))
    assert _verdict(r) == (S, 1) and (r["verdict"][:10] == S).all() and r["verdict"][10:].tolist() == [S, K]
    assert list(r["records"][0].tolist())[:4] == [10, 2, 5, 3]
    assert r["stats"].tolist() == [1, 1, 0, 1, 7, 0, 0, 0]       # five KEEP and two UNTESTED members moved
    r = ovr.run(po, 1, v, p=ovr.params(vote_num=3, vote_den=7))   # 21 < 24
    assert _verdict(r) == (K, 1) and (r["verdict"][:10] == K).all() and r["verdict"][10:].tolist() == [S, K]
    assert r["stats"].tolist() == [1, 1, 0, 0, 0, 5, 0, 0]       # three SEEN_THROUGH and two UNTESTED members moved
    # min_through at equality and one above
    assert _verdict(ovr.run(po, 1, v, p=ovr.params(min_through=3, vote_num=0))) == (S, 1)
    assert _verdict(ovr.run(po, 1, v, p=ovr.params(min_through=4, vote_num=0))) == (K, 1)


def test_rule_at_equality_and_one_below_on_pooled_pairs():
    po, v = _one(0, 2, 1)                                       # the bytes say KEEP; the pairs: through 2 + 0 + 4, agree 1 + 3 + 0
    q = np.array([2 | 1 << 8 | 9 << 16, 0 | 3 << 8 | 1 << 24, 4 | 0 << 8, 0xFFFFFFFF, 0xFFFFFFFF], np.uint32)
    pool = ovr.POOL_PAIRS
    r = ovr.run(po, 1, v, q, p=ovr.params(flags=pool, vote_num=6, vote_den=10))   # 6 * 10 >= 6 * 10
    assert _verdict(r) == (S, 1) and list(r["records"][0].tolist())[4:8] == [6, 4, 9, 1] and r["stats"].tolist()[4:6] == [3, 0]
    assert _verdict(ovr.run(po, 1, v, q, p=ovr.params(flags=pool, vote_num=6, vote_den=9))) == (K, 1)  # 54 < 60
    # the same pairs without the flag: the sums are recorded, the bytes decide (t = 0 < min_through)
    r = ovr.run(po, 1, v, q, p=ovr.params(vote_num=0))
    assert _verdict(r) == (K, 1) and list(r["records"][0].tolist())[4:8] == [6, 4, 9, 1]
    # the members of the vote are those with a KEEP or SEEN_THROUGH byte, pooled or not: the UNTESTED member's pairs still count
    assert _verdict(ovr.run(po, 1, v, q, p=ovr.params(flags=pool, min_tested=3))) == (-1, 0)


def test_a_product_that_needs_64_bits():
    n = 4500
    po = np.zeros(n, np.int32)
    v = np.full(n, K, np.uint8)
    q = np.full(n, 0xFFFFFFFF, np.uint32)                       # sum_through = sum_agree = 4500 * 255 = 1 147 500 >= 4096
    big = 1 << 20
    r = ovr.run(po, 1, v, q, p=ovr.params(flags=ovr.POOL_PAIRS, vote_num=big // 2, vote_den=big))   # t * den == num * 2 t
    assert _verdict(r) == (S, 1) and r["records"]["sum_through"][0] == 1147500
    r = ovr.run(po, 1, v, q, p=ovr.params(flags=ovr.POOL_PAIRS, vote_num=big // 2 + 1, vote_den=big))
    assert _verdict(r) == (K, 1)

    def wrapped(num):   # the comparison as 32-bit two's complement arithmetic would make it
        w = lambda x: ((int(x) & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000  # noqa: E731
        return w(1147500 * big) >= w(w(num) * w(2 * 1147500))
    for num, want in OV_WRAP_CASES:
        assert wrapped(num) != (want == S), "the case tells 64-bit from 32-bit products"
        assert _verdict(ovr.run(po, 1, v, q, p=ovr.params(flags=ovr.POOL_PAIRS, vote_num=num, vote_den=big))) == (want, 1), num


def test_min_points_and_min_tested_at_equality_and_one_above():
    po, v = _one(4, 2, 3)
    assert _verdict(ovr.run(po, 1, v, p=ovr.params(min_points=9))) == (S, 1)
    assert _verdict(ovr.run(po, 1, v, p=ovr.params(min_points=10))) == (-1, 0)
    assert _verdict(ovr.run(po, 1, v, p=ovr.params(min_tested=6))) == (S, 1)
    r = ovr.run(po, 1, v, p=ovr.params(min_tested=7))
    assert _verdict(r) == (-1, 0) and np.array_equal(r["verdict"], v) and r["stats"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


def test_the_ends_of_the_ratio():
    po, v = _one(2, 50)
    assert _verdict(ovr.run(po, 1, v, p=ovr.params(vote_num=0))) == (S, 1)          # min_through alone
    assert _verdict(ovr.run(po, 1, v, p=ovr.params(vote_num=0, min_through=3))) == (K, 1)
    assert _verdict(ovr.run(po, 1, v, p=ovr.params(vote_num=7, vote_den=7))) == (K, 1)   # num == den: every tested member seen through
    po, v = _one(2, 0, 5)
    assert _verdict(ovr.run(po, 1, v, p=ovr.params(vote_num=7, vote_den=7))) == (S, 1)


def test_a_byte_of_seven_counts_as_untested():
    po, v = _one(2, 1, 3, other_byte=7)
    r = ovr.run(po, 1, v)
    assert list(r["records"][0].tolist())[:4] == [6, 3, 1, 2] and _verdict(r) == (S, 1)
    assert (r["verdict"][:6] == S).all() and r["stats"].tolist()[4:6] == [4, 0]     # the sevens are rewritten with the others
    assert _verdict(ovr.run(po, 1, v, p=ovr.params(min_tested=4))) == (-1, 0)       # and are no tested members


def test_with_track_forces_an_object_that_does_not_vote():
    po = np.array([0, 0, 1, 1, 1, -1], np.int32)
    v = np.array([U, U, K, K, K, U], np.uint8)
    dyn = np.array([1, 0], np.uint8)
    r = ovr.run(po, 2, v, dynamic=dyn, p=ovr.params(flags=ovr.WITH_TRACK, min_tested=3), cap=5)
    assert r["records"]["verdict"].tolist() == [S, K] and r["records"]["how"].tolist() == [2, 1]
    assert r["verdict"].tolist() == [S, S, K, K, K, U]
    assert r["stats"].tolist() == [2, 1, 1, 1, 2, 0, 2, 0]
    # without the flag the field is not read; a flag of 2 in `dynamic` is not 1
    assert ovr.run(po, 2, v, dynamic=dyn, p=ovr.params(min_tested=3))["records"]["how"].tolist() == [0, 1]
    assert ovr.run(po, 2, v, dynamic=np.array([2, 1], np.uint8), p=ovr.params(flags=ovr.WITH_TRACK))["records"]["how"].tolist() == [0, 2]
    # the capacity words
    assert ovr.run(po, 2, v, cap=1)["stats"].tolist()[6:] == [1, 1] and ovr.run(po, 2, v, cap=None)["stats"].tolist()[6:] == [0, 0]


def test_member_list_and_point_index_say_the_same():
    rec = np.zeros(2, [("scan", "i4"), ("point_begin", "i4"), ("n_points", "i4")])
    rec["scan"], rec["point_begin"], rec["n_points"] = [0, 2], [0, 3], [3, 2]
    po = ovr.point_object_from_members(rec, np.array([4, 0, 2, 1, 0], np.int32), np.array([0, 5, 5, 8], np.int32), 8)
    assert po.tolist() == [0, -1, 0, -1, 0, 1, 1, -1]
