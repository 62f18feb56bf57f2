"""scvod_batch_object_truth / scvod_batch_object_truth_stats / scvod_batch_object_truth_scratch_bytes /
scvod_object_truth_params_default / scvod_object_truth_finish without a GPU: the symbols and the structs, the argument errors that
come before a device is looked for, the defaults, the host-only finish against the plain statement
tests/helpers/object_truth_ref.py -- counts with ==, rates as double bit patterns -- and that statement against a collections.Counter
loop.  Not gpu."""
import collections
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import object_truth_ref as otr  # noqa: E402

NEW = ("scvod_batch_object_truth", "scvod_batch_object_truth_stats", "scvod_batch_object_truth_scratch_bytes",
       "scvod_object_truth_params_default", "scvod_object_truth_finish")
INVALID = -1
SEED = 20261019


def _same(got, want, what=""):
    for k in otr.COUNTS:
        assert got[k] == want[k], f"{what}: {k} {got[k]} != {want[k]}"
    for k in otr.RATES:
        assert np.float64(got[k]).view(np.uint64) == np.float64(want[k]).view(np.uint64) or (np.isnan(got[k]) and np.isnan(want[k])), \
            f"{what}: {k} {got[k]!r} != {want[k]!r}"


def _tables(scvod, rows):
    """rows of (cls, state, dynamic, n_points, n_label, n_moving) -> (objects, truth)"""
    o = np.zeros(len(rows), scvod.OBJECT_DTYPE)
    t = np.zeros(len(rows), otr.DTYPE)
    for k, (cls, state, dyn, n, n_label, n_moving) in enumerate(rows):
        o[k]["cls"], o[k]["state"], o[k]["dynamic"], o[k]["n_points"] = cls, state, dyn, n
        t[k]["n_points"], t[k]["n_label"], t[k]["n_moving"], t[k]["n_class"], t[k]["n_distinct"] = n, n_label, n_moving, n_label, 1
        t[k]["label"] = (k << 16) | 252
    return o, t


def test_symbols_declared_and_exported_and_the_structs(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("batch_object_truth", "batch_object_truth_stats", "batch_object_truth_scratch_bytes"):
        assert callable(getattr(scvod.Ctx, m))
    d = scvod.OBJECT_TRUTH_DTYPE
    assert d.itemsize == 32 and d == otr.DTYPE
    assert [(n, d.fields[n][1]) for n in d.names] == [("label", 0), ("n_label", 4), ("n_class", 8), ("n_moving", 12), ("n_distinct", 16),
                                                      ("n_points", 20), ("reserved", 24)]
    body = hdr[hdr.index("typedef struct scvod_object_truth {"):hdr.index("} scvod_object_truth;")]
    assert re.findall(r"^\s*(?:u?int\d+_t)\s+(\w+)", body, re.M) == list(d.names)
    m = re.search(r"#define SCVOD_OBJ_TRUTH_ONCHIP_LABELS (\d+)", hdr)
    assert m and int(m.group(1)) == scvod.OBJ_TRUTH_ONCHIP_LABELS >= 1
    P, R = scvod.ObjectTruthParams, scvod.ObjectTruthResult
    assert C.sizeof(P) == 24 and [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("moving_from", 0), ("pure_from", 8), ("min_points", 16)]
    assert C.sizeof(R) == 88 and [f for f, _ in R._fields_] == list(otr.COUNTS) + list(otr.RATES)
    body = hdr[hdr.index("typedef struct scvod_object_truth_result {"):hdr.index("} scvod_object_truth_result;")]
    assert re.findall(r"^\s*(?:int64_t|double)\s+(\w+);", body, re.M) == [f for f, _ in R._fields_]


def test_argument_errors_come_before_the_device(scvod):
    """a NULL ctx is SCVOD_ERR_INVALID whatever else is passed: no device is touched and nothing is written"""
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data_as(C.c_void_p)
    call, stats = lib.scvod_batch_object_truth, lib.scvod_batch_object_truth_stats
    good = scvod.eval_params_default()
    assert call(None, p, C.byref(good), p, 4, None) == INVALID
    assert call(None, p, None, p, 4, None) == INVALID
    assert call(None, None, None, p, 4, None) == INVALID                  # no labels
    assert call(None, p, None, None, 4, None) == INVALID                  # no output
    assert call(None, p, None, p, -1, None) == INVALID                    # cap_truth < 0
    assert call(None, p, C.byref(scvod.eval_params_default(dynamic_classes=range(17))), p, 4, None) == INVALID
    assert stats(None, p) == INVALID
    assert stats(None, None) == INVALID
    assert lib.scvod_batch_object_truth_scratch_bytes(None) == 0
    lib.scvod_object_truth_params_default(None)
    assert not buf.any()


def test_params_default(scvod):
    p = scvod.object_truth_params_default()
    assert (p.moving_from, p.pure_from, p.min_points) == (0.5, 0.5, 1)
    q = scvod.object_truth_params_default(moving_from=0.25, pure_from=0.75, min_points=30)
    assert (q.moving_from, q.pure_from, q.min_points) == (0.25, 0.75, 30)


# (cls, state, dynamic, n_points, n_label, n_moving)
CRAFTED = [
    (2, 1, 1, 10, 10, 5),     # exactly half moving: truth-moving; found
    (2, 1, 1, 10, 10, 4),     # one less: static, and the flag is a false alarm
    (2, 0, 0, 7, 7, 4),       # 3.5 of 7: moving; a car judged static
    (2, 0, 0, 7, 7, 3),       # static, rightly
    (2, -1, 0, 100, 100, 100),  # a car the tracking never judged
    (1, -1, 0, 30, 30, 30),   # typed tree
    (3, -1, 0, 30, 14, 30),   # typed building; 14 of 30 < half: mixed
    (3, -1, 0, 30, 15, 0),    # exactly half: not mixed
    (1, -1, 0, 3, 1, 3),      # small
    (2, 1, 1, 1, 1, 1),
]


def test_finish_on_the_crafted_table(scvod):
    o, t = _tables(scvod, CRAFTED)
    got = scvod.object_truth_finish(o, t)
    _same(got, otr.finish(o, t), "defaults")
    # worked out by hand
    assert (got["moving_objects"], got["moving_dynamic"], got["moving_car_static"], got["moving_car_untracked"], got["moving_not_car"]) == (7, 2, 1, 1, 3)
    assert (got["static_objects"], got["static_dynamic"], got["mixed_objects"], got["skipped"]) == (3, 1, 2, 0)
    assert got["precision"] == 100.0 * 2 / 3 and got["recall"] == 100.0 * 2 / 7
    # NULL params are the defaults
    r = scvod.ObjectTruthResult()
    assert scvod.load_lib().scvod_object_truth_finish(o.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), len(o), None, C.byref(r)) == 0
    assert r.moving_objects == 7 and r.static_dynamic == 1
    # min_points: the small objects leave every other count
    got = scvod.object_truth_finish(o, t, scvod.object_truth_params_default(min_points=4))
    _same(got, otr.finish(o, t, min_points=4), "min_points 4")
    assert (got["skipped"], got["moving_objects"], got["moving_dynamic"], got["mixed_objects"]) == (2, 5, 1, 1)


@pytest.mark.parametrize("kw", [dict(moving_from=0.4), dict(moving_from=0.5000000000000001), dict(pure_from=0.4), dict(pure_from=0.5000000000000001),
                                dict(moving_from=0.0), dict(moving_from=1.0, pure_from=1.0), dict(moving_from=2.0), dict(pure_from=0.0),
                                dict(min_points=8), dict(min_points=31), dict(min_points=101), dict(moving_from=-1.0, pure_from=-1.0)])
def test_finish_equals_the_helper_with_other_parameters(scvod, kw):
    o, t = _tables(scvod, CRAFTED)
    got = scvod.object_truth_finish(o, t, scvod.object_truth_params_default(**kw))
    _same(got, otr.finish(o, t, **kw), str(kw))
    if kw.get("min_points") == 101:       # nothing left: every denominator is zero
        assert got["skipped"] == len(o) and np.isnan(got["precision"]) and np.isnan(got["recall"])
    if kw.get("moving_from") == 2.0:      # no object is moving: recall has no denominator, precision has the false alarms
        assert got["moving_objects"] == 0 and np.isnan(got["recall"]) and got["precision"] == 0.0
    if kw.get("moving_from") == 0.0:      # every object is moving: no false alarm is left
        assert got["static_objects"] == 0 and got["precision"] == 100.0


def test_finish_equals_the_helper_on_seeded_tables(scvod):
    rng = np.random.default_rng(SEED)
    seen_nan = {"precision": 0, "recall": 0}
    for it in range(300):
        m = int(rng.integers(0, 40))
        n = rng.integers(1, 10 ** int(rng.integers(1, 9)), m)
        share = rng.choice([0, 0.25, 0.5, 0.75, 1.0], m)
        rows = []
        for k in range(m):
            cls = int(rng.choice([1, 2, 3]))
            dyn = int(cls == 2 and rng.random() < 0.4) if it % 3 else 0
            state = -1 if cls != 2 else (1 if dyn else int(rng.choice([-1, 0])))
            n_moving = int(n[k] * share[k]) if it % 5 else 0
            rows.append((cls, state, dyn, int(n[k]), int(rng.integers(1, n[k] + 1)), n_moving))
        o, t = _tables(scvod, rows)
        kw = dict(moving_from=float(rng.choice([0.25, 0.5, 0.75])), pure_from=float(rng.choice([0.25, 0.5, 0.75])),
                  min_points=int(rng.choice([1, 5, 1000])))
        got = scvod.object_truth_finish(o, t, scvod.object_truth_params_default(**kw))
        _same(got, otr.finish(o, t, **kw), f"seeded {it}")
        assert got["moving_objects"] == got["moving_dynamic"] + got["moving_car_static"] + got["moving_car_untracked"] + got["moving_not_car"]
        assert got["moving_objects"] + got["static_objects"] + got["skipped"] == m
        for k in seen_nan:
            seen_nan[k] += bool(np.isnan(got[k]))
    assert seen_nan["precision"] > 0 and seen_nan["recall"] > 0, "no seeded table reached a zero denominator"


def test_finish_of_an_empty_table_and_bad_arguments(scvod):
    got = scvod.object_truth_finish(np.zeros(0, scvod.OBJECT_DTYPE), np.zeros(0, otr.DTYPE))
    assert all(got[k] == 0 for k in otr.COUNTS) and np.isnan(got["precision"]) and np.isnan(got["recall"])
    _same(got, otr.finish([], np.zeros(0, otr.DTYPE)), "empty")
    lib = scvod.load_lib()
    o, t = _tables(scvod, CRAFTED)
    op, tp = o.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)
    r = scvod.ObjectTruthResult()
    assert lib.scvod_object_truth_finish(None, tp, 3, None, C.byref(r)) == INVALID
    assert lib.scvod_object_truth_finish(op, None, 3, None, C.byref(r)) == INVALID
    assert lib.scvod_object_truth_finish(op, tp, -1, None, C.byref(r)) == INVALID
    assert lib.scvod_object_truth_finish(op, tp, len(o), None, None) == INVALID
    assert lib.scvod_object_truth_finish(None, None, 0, None, C.byref(r)) == 0
    for kw in (dict(moving_from=float("nan")), dict(moving_from=float("inf")), dict(pure_from=float("nan")), dict(pure_from=-float("inf"))):
        assert lib.scvod_object_truth_finish(op, tp, len(o), C.byref(scvod.object_truth_params_default(**kw)), C.byref(r)) == INVALID, kw


# ---- the helper itself -------------------------------------------------------------------------------------------------------------------

def _counter_record(labels, dynamic):
    """the record by a plain loop"""
    cnt = collections.Counter(int(v) for v in labels)
    best = max(cnt.values())
    label = min(k for k, v in cnt.items() if v == best)
    return (label, best, sum(v for k, v in cnt.items() if (k & 0xFFFF) == (label & 0xFFFF)),
            sum(v for k, v in cnt.items() if (k & 0xFFFF) in dynamic), len(cnt), len(labels))


def test_helper_record_by_hand_and_against_a_counter_loop():
    r = otr.record([7, 7, 0, 0xFFFFFFFF, 7, 0, (1 << 16) | 7])
    assert (int(r["label"]), int(r["n_label"]), int(r["n_class"]), int(r["n_moving"]), int(r["n_distinct"]), int(r["n_points"])) == (7, 3, 4, 0, 4, 7)
    r = otr.record([(2 << 16) | 252, (1 << 16) | 252, 40, 40, (1 << 16) | 252, (2 << 16) | 252])     # a three-way tie: the smallest value
    assert (int(r["label"]), int(r["n_label"]), int(r["n_class"]), int(r["n_moving"]), int(r["n_distinct"])) == (40, 2, 2, 4, 3)
    r = otr.record([0xFFFFFFFF, 0])                                                                 # 0 and all ones are labels like any other
    assert (int(r["label"]), int(r["n_label"]), int(r["n_class"]), int(r["n_distinct"])) == (0, 1, 1, 2)
    assert not r["reserved"].any()
    rng = np.random.default_rng(SEED)
    pool = np.array([0, 1, 40, 252, 253, (1 << 16) | 252, (2 << 16) | 252, (1 << 16) | 40, 0xFFFFFFFF, 0xFFFF00FC, 259 | (7 << 16)], np.uint32)
    for it in range(200):
        n = int(rng.integers(1, 200))
        lab = rng.choice(pool[:int(rng.integers(1, len(pool) + 1))], n)
        dyn = otr.DYNAMIC if it % 2 else (40, 1)
        r = otr.record(lab, dyn)
        assert (int(r["label"]), int(r["n_label"]), int(r["n_class"]), int(r["n_moving"]), int(r["n_distinct"]), int(r["n_points"])) == \
            _counter_record(lab, dyn), it
    # a table: two objects in two scans, members as input indices inside the scan
    objects = np.zeros(2, [("scan", "i4"), ("point_begin", "i4"), ("n_points", "i4")])
    objects["scan"], objects["point_begin"], objects["n_points"] = (0, 1), (0, 3), (3, 2)
    gt = np.array([5, 6, 5, 9, 252, 253 | (1 << 16), 8], np.uint32)
    out = otr.records(objects, np.array([0, 2, 1, 2, 1], np.int32), np.array([0, 4, 7], np.int32), gt)
    assert out["label"].tolist() == [5, 8] and out["n_label"].tolist() == [2, 1] and out["n_moving"].tolist() == [0, 1]
    assert out["n_distinct"].tolist() == [2, 2] and out["n_points"].tolist() == [3, 2]
