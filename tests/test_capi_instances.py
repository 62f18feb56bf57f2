"""scvod_score_instances_device / scvod_score_instances_stats / scvod_instance_params_default / scvod_instance_finish /
scvod_instance_merge without a GPU: the symbols and the structs, the argument errors that come before a device is looked for, the
defaults, and the two host-only calls against the plain statement tests/helpers/instances_ref.py -- counts with ==, rates as double
bit patterns.  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import instances_ref as inr  # noqa: E402

NEW = ("scvod_score_instances_device", "scvod_score_instances_stats", "scvod_score_instances_scratch_bytes",
       "scvod_instance_params_default", "scvod_instance_finish", "scvod_instance_merge")
INVALID, CAPACITY = -1, -4
RATES = ("hd_removed_rate", "ld_retained_rate")


def _tab(rows):
    """rows of (label, first_point, n_points, n_inlier, n_preserved)"""
    return np.array([tuple(r) for r in rows], inr.DTYPE).reshape(-1)


def _key(cls, inst):
    return (inst << 16) | cls


def _same(got, want, what=""):
    for k in inr.COUNTS:
        assert got[k] == want[k], f"{what}: {k} {got[k]} != {want[k]}"
    for k in RATES:
        assert np.float64(got[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64) or (np.isnan(got[k]) and np.isnan(want[k])), \
            f"{what}: {k} {got[k]!r} != {want[k]!r}"


def test_symbols_declared_and_exported_and_the_structs(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("score_instances_device", "score_instances_stats", "score_instances_scratch_bytes", "batch_score_instances"):
        assert callable(getattr(scvod.Ctx, m))
    d = scvod.INSTANCE_DTYPE
    assert d.itemsize == 32 and d == inr.DTYPE
    assert [(n, d.fields[n][1]) for n in d.names] == [("label", 0), ("first_point", 4), ("n_points", 8), ("n_inlier", 16), ("n_preserved", 24)]
    body = hdr[hdr.index("typedef struct scvod_instance {"):hdr.index("} scvod_instance;")]
    assert re.findall(r"\b(label|first_point|n_points|n_inlier|n_preserved);", body) == list(d.names)
    P, R = scvod.InstanceParams, scvod.InstanceResult
    assert C.sizeof(P) == 96
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("n_dynamic_classes", 0), ("dynamic_classes", 4), ("n_static_classes", 36),
                                                                 ("static_classes", 40), ("removed_below", 72), ("retained_from", 80),
                                                                 ("min_points", 88)]
    assert C.sizeof(R) == 88 and [f for f, _ in R._fields_] == list(inr.COUNTS) + list(RATES)


def test_argument_errors_come_before_the_device(scvod):
    """a NULL ctx is SCVOD_ERR_INVALID whatever else is passed, and so is every bad argument next to it: no device is touched and
    nothing is written"""
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data_as(C.c_void_p)
    dev, stats = lib.scvod_score_instances_device, lib.scvod_score_instances_stats
    assert dev(None, p, p, 4, p, 8, p, None) == INVALID
    assert dev(None, p, p, -1, p, 8, p, None) == INVALID                # n < 0
    assert dev(None, p, p, (1 << 31), p, 8, p, None) == INVALID         # n > INT32_MAX
    assert dev(None, None, p, 4, p, 8, p, None) == INVALID              # a NULL array with n > 0
    assert dev(None, p, None, 4, p, 8, p, None) == INVALID
    for cap in (0, -1, (1 << 22) + 1):
        assert dev(None, p, p, 4, p, cap, p, None) == INVALID           # cap_instances outside 1 .. 1 << 22
    assert dev(None, p, p, 4, p, 8, None, None) == INVALID              # d_n NULL
    assert dev(None, p, p, 4, None, 8, p, None) == INVALID              # (count only, but still no ctx)
    assert stats(None, p) == INVALID
    assert stats(None, None) == INVALID
    assert lib.scvod_score_instances_scratch_bytes(None) == 0
    assert not buf.any()


def test_params_default(scvod):
    p = scvod.instance_params_default()
    assert p.n_dynamic_classes == 8 and tuple(p.dynamic_classes[:8]) == tuple(range(252, 260)) == inr.DYNAMIC and not any(p.dynamic_classes[8:])
    assert p.n_static_classes == 8 and tuple(p.static_classes[:8]) == (10, 31, 30, 32, 16, 13, 18, 20) == inr.STATIC
    assert not any(p.static_classes[8:])
    assert p.removed_below == 0.5 and p.retained_from == 0.5 and p.min_points == 1
    q = scvod.instance_params_default(dynamic_classes=[7], static_classes=[], removed_below=0.25, retained_from=0.75, min_points=30)
    assert (q.n_dynamic_classes, q.dynamic_classes[0], q.n_static_classes) == (1, 7, 0)
    assert (q.removed_below, q.retained_from, q.min_points) == (0.25, 0.75, 30)


# a crafted table: per record the class, the instance, n_points and n_preserved
CRAFTED = [
    # HD, a share of exactly 0.5: not below 0.5 -> kept; one point less preserved -> removed
    (252, 1, 10, 5), (252, 2, 10, 4), (253, 3, 3, 0), (259, 4, 7, 7),
    # LD, a share of exactly 0.5: retained; one less: not retained
    (10, 1, 10, 5), (10, 2, 10, 4), (20, 3, 1, 1), (31, 4, 9, 0),
    # instance 0 of either kind: stuff, not an object
    (252, 0, 100, 0), (10, 0, 100, 100),
    # a class in neither list
    (40, 5, 50, 50), (70, 6, 5, 0),
    # odd sizes, where the product is not an integer: 3.5 of 7
    (254, 9, 7, 3), (254, 10, 7, 4), (13, 9, 7, 3), (13, 10, 7, 4),
]


def _crafted():
    rows = sorted((_key(c, i), 11 * k, n, max(pre, min(n, pre + 1)), pre) for k, (c, i, n, pre) in enumerate(CRAFTED))
    return _tab(rows)


def test_finish_on_the_crafted_table(scvod):
    t = _crafted()
    got = scvod.instance_finish(t)
    want = inr.finish(t)
    _same(got, want, "defaults")
    # worked out by hand
    assert (got["hd_gt"], got["hd_removed"], got["ld_gt"], got["ld_retained"], got["skipped"]) == (6, 3, 6, 3, 4)
    assert (got["hd_points"], got["hd_points_preserved"]) == (10 + 10 + 3 + 7 + 7 + 7, 5 + 4 + 0 + 7 + 3 + 4)
    assert (got["ld_points"], got["ld_points_preserved"]) == (10 + 10 + 1 + 9 + 7 + 7, 5 + 4 + 1 + 0 + 3 + 4)
    assert got["hd_removed_rate"] == 50.0 and got["ld_retained_rate"] == 50.0
    # NULL params are the defaults
    r = scvod.InstanceResult()
    assert scvod.load_lib().scvod_instance_finish(t.ctypes.data_as(C.c_void_p), t.size, None, C.byref(r)) == 0
    assert r.hd_removed == 3 and r.skipped == 4


@pytest.mark.parametrize("kw", [dict(removed_below=0.4), dict(removed_below=0.5000000000000001), dict(retained_from=0.4),
                                dict(retained_from=0.5000000000000001), dict(removed_below=1.0, retained_from=0.0),
                                dict(removed_below=0.0, retained_from=1.0), dict(min_points=4), dict(min_points=8), dict(min_points=11),
                                dict(dynamic=(252,), static=(252, 10)), dict(dynamic=(), static=()), dict(dynamic=(40, 70), static=(10,))])
def test_finish_equals_the_helper_with_other_parameters(scvod, kw):
    t = _crafted()
    par = scvod.instance_params_default(dynamic_classes=kw.get("dynamic"), static_classes=kw.get("static"),
                                        removed_below=kw.get("removed_below"), retained_from=kw.get("retained_from"),
                                        min_points=kw.get("min_points"))
    got = scvod.instance_finish(t, par)
    _same(got, inr.finish(t, **kw), str(kw))
    if kw.get("dynamic") == (252,):
        # 252 is in both lists: dynamic wins, so the two 252 objects are HD and the two class-10 ones LD
        assert (got["hd_gt"], got["ld_gt"]) == (2, 2)
    if kw.get("min_points") == 11:
        assert got["hd_gt"] == 0 == got["ld_gt"] and got["skipped"] == len(t) and np.isnan(got["hd_removed_rate"])


def test_finish_equals_the_helper_on_seeded_tables(scvod):
    rng = np.random.default_rng(20261019)
    pool = np.array(list(inr.DYNAMIC) + list(inr.STATIC) + [0, 1, 40, 48, 70, 99], np.uint32)
    for it in range(200):
        m = int(rng.integers(0, 60))
        keys = np.unique(rng.choice(pool, m) | (rng.integers(0, 4, m).astype(np.uint32) << np.uint32(16)))
        n = rng.integers(1, 10 ** int(rng.integers(1, 10)), len(keys))
        pre = (n * rng.choice([0, 0.25, 0.5, 0.75, 1.0], len(keys))).astype(np.int64)
        t = _tab(zip(keys, rng.integers(0, 1 << 31, len(keys)), n, n, pre))
        kw = dict(removed_below=float(rng.choice([0.25, 0.5, 0.75])), retained_from=float(rng.choice([0.25, 0.5, 0.75])),
                  min_points=int(rng.choice([1, 5, 1000])))
        got = scvod.instance_finish(t, scvod.instance_params_default(**kw))
        _same(got, inr.finish(t, **kw), f"seeded {it}")


def test_finish_of_an_empty_table_and_bad_arguments(scvod):
    got = scvod.instance_finish(np.zeros(0, inr.DTYPE))
    assert all(got[k] == 0 for k in inr.COUNTS) and np.isnan(got["hd_removed_rate"]) and np.isnan(got["ld_retained_rate"])
    _same(got, inr.finish(np.zeros(0, inr.DTYPE)), "empty")
    lib = scvod.load_lib()
    t = _crafted()
    tp = t.ctypes.data_as(C.c_void_p)
    r = scvod.InstanceResult()
    assert lib.scvod_instance_finish(None, 3, None, C.byref(r)) == INVALID
    assert lib.scvod_instance_finish(tp, -1, None, C.byref(r)) == INVALID
    assert lib.scvod_instance_finish(tp, t.size, None, None) == INVALID
    assert lib.scvod_instance_finish(None, 0, None, C.byref(r)) == 0
    for kw in (dict(removed_below=float("nan")), dict(removed_below=float("inf")), dict(retained_from=float("nan")),
               dict(retained_from=-float("inf")), dict(dynamic_classes=range(17)), dict(static_classes=range(17))):
        assert lib.scvod_instance_finish(tp, t.size, C.byref(scvod.instance_params_default(**kw)), C.byref(r)) == INVALID
    for field in ("n_dynamic_classes", "n_static_classes"):
        q = scvod.instance_params_default()
        setattr(q, field, -1)
        assert lib.scvod_instance_finish(tp, t.size, C.byref(q), C.byref(r)) == INVALID
    q = scvod.instance_params_default(dynamic_classes=range(300, 316), static_classes=range(16))     # 16 each: the longest lists
    assert lib.scvod_instance_finish(tp, t.size, C.byref(q), C.byref(r)) == 0


# ---- merge ------------------------------------------------------------------------------------------------------------------------------

def _merge_raw(lib, a, b, cap, guard=3):
    out = np.zeros(cap + guard, inr.DTYPE)
    out["label"][cap:] = 0xDEADBEEF
    n = C.c_int64(-7)
    rc = lib.scvod_instance_merge(a.ctypes.data_as(C.c_void_p) if a.size else None, a.size, b.ctypes.data_as(C.c_void_p) if b.size else None,
                                  b.size, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    assert (out["label"][cap:] == 0xDEADBEEF).all() and not out["n_points"][cap:].any(), "written behind cap"
    return rc, n.value, out[:cap]


def test_merge(scvod):
    lib = scvod.load_lib()
    a = _tab([(0, 5, 3, 2, 1), (7, 100, 10, 9, 8), (_key(252, 1), 40, 6, 1, 0), (0xFFFFFFFF, 9, 1, 1, 1)])
    disjoint = _tab([(1, 0, 4, 4, 4), (_key(252, 2), 77, 5, 5, 5), (0xFFFFFFFE, 3, 2, 0, 0)])
    shared = _tab([(0, 2, 1, 1, 1), (7, 200, 1 << 40, 1 << 39, 5), (_key(10, 1), 6, 6, 6, 6), (0xFFFFFFFF, 10, 2, 0, 0)])
    empty = np.zeros(0, inr.DTYPE)
    for name, x, y in (("disjoint", a, disjoint), ("shared", a, shared), ("left empty", empty, a), ("right empty", a, empty),
                       ("both empty", empty, empty), ("itself", a, a)):
        want = inr.merge(x, y)
        got = scvod.instance_merge(x, y)
        assert got.dtype == inr.DTYPE and got.tobytes() == want.tobytes(), name
        assert got.tobytes() == scvod.instance_merge(y, x).tobytes(), f"{name}: not symmetric"
        rc, n, out = _merge_raw(lib, x, y, len(want))                  # a capacity that just fits
        assert rc == 0 and n == len(want) and out.tobytes() == want.tobytes(), name
        if len(want):
            rc, n, out = _merge_raw(lib, x, y, len(want) - 1)          # one too small: the true size, nothing behind cap
            assert rc == CAPACITY and n == len(want), name
            assert out.tobytes() == want[:-1].tobytes(), name
    m = scvod.instance_merge(a, shared)
    assert m["label"].tolist() == [0, 7, _key(10, 1), _key(252, 1), 0xFFFFFFFF]
    assert m[0].tolist() == (0, 2, 4, 3, 2) and m[1].tolist() == (7, 100, 10 + (1 << 40), 9 + (1 << 39), 13) and m[4].tolist() == (0xFFFFFFFF, 9, 3, 1, 1)
    # a table in three shards merges to the table of the whole, whatever the grouping
    rng = np.random.default_rng(5)
    keys = rng.choice(np.array([0, 9, _key(252, 1), _key(252, 2), _key(10, 1), 0xFFFFFFFF], np.uint32), 3000)
    res = rng.integers(0, 256, 3000).astype(np.uint8)
    parts = []
    for lo, hi in ((0, 1000), (1000, 1001), (1001, 3000)):
        t = inr.table(keys[lo:hi], res[lo:hi])
        t["first_point"] += lo
        parts.append(t)
    whole = inr.table(keys, res)
    assert scvod.instance_merge(scvod.instance_merge(parts[0], parts[1]), parts[2]).tobytes() == whole.tobytes()
    assert scvod.instance_merge(parts[0], scvod.instance_merge(parts[2], parts[1])).tobytes() == whole.tobytes()


def test_merge_refuses_unsorted_input_and_bad_arguments(scvod):
    lib = scvod.load_lib()
    good = _tab([(1, 0, 1, 1, 1), (5, 1, 1, 1, 1), (9, 2, 1, 1, 1)])
    for bad in (_tab([(5, 0, 1, 1, 1), (1, 1, 1, 1, 1)]), _tab([(1, 0, 1, 1, 1), (5, 1, 1, 1, 1), (5, 2, 1, 1, 1)]),
                _tab([(1, 0, 1, 1, 1), (0xFFFFFFFF, 1, 1, 1, 1), (2, 2, 1, 1, 1)])):
        for x, y in ((bad, good), (good, bad)):
            out = np.zeros(8, inr.DTYPE)
            n = C.c_int64(-7)
            assert lib.scvod_instance_merge(x.ctypes.data_as(C.c_void_p), x.size, y.ctypes.data_as(C.c_void_p), y.size,
                                            out.ctypes.data_as(C.c_void_p), 8, C.byref(n)) == INVALID
            assert not out["n_points"].any(), "an unsorted input must leave the output alone"
            with pytest.raises(RuntimeError):
                scvod.instance_merge(x, y)
    gp = good.ctypes.data_as(C.c_void_p)
    out = np.zeros(8, inr.DTYPE)
    op = out.ctypes.data_as(C.c_void_p)
    n = C.c_int64(0)
    assert lib.scvod_instance_merge(None, 3, gp, 3, op, 8, C.byref(n)) == INVALID
    assert lib.scvod_instance_merge(gp, 3, None, 3, op, 8, C.byref(n)) == INVALID
    assert lib.scvod_instance_merge(gp, -1, gp, 3, op, 8, C.byref(n)) == INVALID
    assert lib.scvod_instance_merge(gp, 3, gp, 3, None, 8, C.byref(n)) == INVALID
    assert lib.scvod_instance_merge(gp, 3, gp, 3, op, -1, C.byref(n)) == INVALID
    assert lib.scvod_instance_merge(gp, 3, gp, 3, op, 8, None) == INVALID
    assert lib.scvod_instance_merge(gp, 3, gp, 3, None, 0, C.byref(n)) == CAPACITY and n.value == 3      # count only


# ---- the helper itself, against answers worked out by hand ----------------------------------------------------------------------------------

def test_helper_table_by_hand():
    keys = [7, 7, 0, 0xFFFFFFFF, 7, 0, (1 << 16) | 7]
    #       inlier, static kept | inlier, gt dyn, est static | no inlier | inlier, both dyn | high bits only | inlier + high bits | dyn pair
    res = [1, 1 | 2, 0, 1 | 2 | 4, 0xF8, 0xF9, 1 | 2 | 4]
    t = inr.table(keys, res)
    assert t["label"].tolist() == [0, 7, (1 << 16) | 7, 0xFFFFFFFF]
    assert t["first_point"].tolist() == [2, 0, 6, 3]
    assert t["n_points"].tolist() == [2, 3, 1, 1]
    assert t["n_inlier"].tolist() == [1, 2, 1, 1]
    assert t["n_preserved"].tolist() == [1, 1, 1, 1]
    assert len(inr.table([], [])) == 0
