"""scvod_evaluate_device / scvod_batch_evaluate / scvod_evaluate_stats / scvod_classify_map_device without a GPU: the symbols and the
structs, scvod_eval_finish against metric.py's arithmetic (exactly: the same IEEE double operations), the NaN rule, the argument errors
that come before a device is looked for, and the numpy statement the GPU tests compare with (tests/helpers/evaluate_ref.py) against
metric.py over the oracle's brute-force search and against the golden file the reference's own tool/analysis.py wrote.  Not gpu."""
import ctypes as C
import json
import math
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
sys.path.insert(0, os.path.join(HERE, "golden"))
import evaluate_ref as evr  # noqa: E402
import metric  # noqa: E402
from metric_cases import make_case  # noqa: E402

NEW = ("scvod_eval_params_default", "scvod_eval_finish", "scvod_evaluate_device", "scvod_batch_evaluate", "scvod_evaluate_stats",
       "scvod_evaluate_scratch_bytes", "scvod_classify_map_device", "scvod_classify_map_stats")
INVALID = -1


def _gold():
    return json.load(open(os.path.join(HERE, "golden", "metric_golden.json")))


def _same_double(a, b):
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def test_symbols_declared_and_exported_and_the_structs(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("evaluate_device", "batch_evaluate", "evaluate_stats", "classify_map_device", "classify_map_stats"):
        assert callable(getattr(scvod.Ctx, m))
    assert C.sizeof(scvod.EvalParams) == 48 and scvod.EvalParams.n_dynamic_classes.offset == 8 and scvod.EvalParams.dynamic_classes.offset == 12
    assert C.sizeof(scvod.EVAL_RESULT) == 80 and [f for f, _ in scvod.EVAL_RESULT._fields_] == list(evr.COUNTS) + ["PR", "RR", "F1"]
    body = hdr[hdr.index("typedef struct scvod_eval_result {"):hdr.index("} scvod_eval_result;")]
    assert re.findall(r"\b(num_\w+|PR|RR|F1)\b", body) == list(evr.COUNTS) + ["PR", "RR", "F1"]
    assert (scvod.EVAL_INLIER, scvod.EVAL_GT_DYNAMIC, scvod.EVAL_EST_DYNAMIC) == (evr.INLIER, evr.GT_DYNAMIC, evr.EST_DYNAMIC) == (1, 2, 4)


def test_params_default(scvod):
    p = scvod.eval_params_default()
    assert p.voxelsize == 0.2 and p.n_dynamic_classes == 8
    assert tuple(p.dynamic_classes[:8]) == tuple(range(252, 260)) == tuple(metric.DYNAMIC_CLASSES) and not any(p.dynamic_classes[8:])
    q = scvod.eval_params_default(voxelsize=0.05, dynamic_classes=[7])
    assert q.voxelsize == 0.05 and q.n_dynamic_classes == 1 and q.dynamic_classes[0] == 7


def _metric_rates(c):
    """metric.py:28-30 literally"""
    n_static, n_dynamic, _, _, _, num_static_preserved, num_dynamic_preserved = (int(v) for v in c)
    pr = 100.0 * num_static_preserved / n_static
    rr = 100.0 * (n_dynamic - num_dynamic_preserved) / n_dynamic
    f1 = 2 * (pr / 100) * (rr / 100) / ((pr / 100) + (rr / 100)) if pr + rr > 0 else 0.0
    return pr, rr, f1


def test_finish_equals_metric_py_on_the_golden_counts_and_on_seeded_counts(scvod):
    vectors = [[g[k] for k in evr.COUNTS] for g in _gold()]
    rng = np.random.default_rng(20261018)
    for i in range(1000):
        n_static, n_dynamic = int(rng.integers(1, 10 ** int(rng.integers(1, 10)))), int(rng.integers(1, 10 ** int(rng.integers(1, 10))))
        sp, dp = int(rng.integers(0, n_static + 1)), int(rng.integers(0, n_dynamic + 1))
        if i % 50 == 0:
            sp, dp = 0, n_dynamic  # PR = RR = 0: the F1 branch without a sum
        vectors.append([n_static, n_dynamic, int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 40)), sp + dp + int(rng.integers(0, 100)), sp, dp])
    zero_f1 = 0
    for c in vectors:
        r = scvod.eval_finish(c)
        assert [r[k] for k in evr.COUNTS] == c
        pr, rr, f1 = _metric_rates(c)
        assert _same_double(r["PR"], pr) and _same_double(r["RR"], rr) and _same_double(r["F1"], f1), (c, r, (pr, rr, f1))
        assert tuple(map(float, evr.finish(c))) == (pr, rr, f1)
        zero_f1 += f1 == 0.0
    assert zero_f1 >= 20
    for g, c in zip(_gold(), vectors):
        r = scvod.eval_finish(c)
        assert abs(r["PR"] - g["PR"]) < 1e-9 and abs(r["RR"] - g["RR"]) < 1e-9 and abs(r["F1"] - g["F1"]) < 1e-9


def test_nan_rule_on_zero_denominators(scvod):
    r = scvod.eval_finish([0, 10, 5, 5, 3, 0, 3])     # no static gt point
    assert math.isnan(r["PR"]) and r["RR"] == 70.0 and math.isnan(r["F1"])
    r = scvod.eval_finish([10, 0, 5, 5, 3, 3, 0])     # no dynamic gt point
    assert r["PR"] == 30.0 and math.isnan(r["RR"]) and math.isnan(r["F1"])
    r = scvod.eval_finish([0, 0, 0, 0, 0, 0, 0])
    assert math.isnan(r["PR"]) and math.isnan(r["RR"]) and math.isnan(r["F1"])
    for c in ([0, 10, 5, 5, 3, 0, 3], [10, 0, 5, 5, 3, 3, 0], [0, 0, 0, 0, 0, 0, 0], [4, 4, 0, 0, 0, 0, 4]):
        want, got = evr.finish(c), scvod.eval_finish(c)
        assert all(_same_double(got[k], w) for k, w in zip(("PR", "RR", "F1"), want)), c
    assert scvod.eval_finish([4, 4, 0, 0, 0, 0, 4])["F1"] == 0.0  # both rates 0: metric.py's `else 0.0`, not NaN
    with pytest.raises(ZeroDivisionError):
        _metric_rates([0, 10, 5, 5, 3, 0, 3])          # what the library's NaN stands for


@pytest.mark.parametrize("case", range(3))
def test_helper_against_metric_py_over_the_oracle_search_and_the_golden_file(oracle, case):
    g = _gold()[case]
    xyz, lab, exyz, elab = make_case(**g["case"])
    assert 3000 <= len(xyz) <= 6000
    m = metric.preservation_rejection(xyz, lab, exyz, elab, oracle.nn_search, voxelsize=0.2)
    for nn_fn in (evr.grid_nn, evr.brute_nn):
        r = evr.evaluate(xyz, lab, exyz, elab, 0.2, nn_fn=nn_fn)
        for k in evr.COUNTS:
            assert r[k] == m[k] == g[k], (k, nn_fn.__name__)
        assert (r["PR"], r["RR"], r["F1"]) == (m["PR"], m["RR"], m["F1"])
        assert abs(r["PR"] - g["PR"]) < 1e-9 and abs(r["RR"] - g["RR"]) < 1e-9 and abs(r["F1"] - g["F1"]) < 1e-9
        # the per-point byte against the oracle's search, index by index
        idx, sqd, _ = oracle.nn_search(exyz, xyz, 0.2)
        inl = np.sqrt(sqd.astype(np.float64)) < 0.2 * np.sqrt(3) / 2
        want = inl * 1 + evr.is_dynamic(lab) * 2 + (inl & evr.is_dynamic(elab)[idx]) * 4
        assert np.array_equal(r["point_result"], want.astype(np.uint8))
    # the two look-ups agree wherever they have to: on every query with a map point inside the reach
    limit = 0.2 * np.sqrt(3) / 2
    gi, gs = evr.grid_nn(exyz, xyz, limit)
    bi, bs = evr.brute_nn(exyz, xyz)
    near = np.sqrt(bs.astype(np.float64)) < limit
    assert near.any() and np.array_equal(gi[near], bi[near]) and np.array_equal(gs[near].view(np.uint32), bs[near].view(np.uint32))


def test_helper_viewer_classes_against_metric_py(oracle):
    rng = np.random.default_rng(5)
    static = rng.uniform(-4, 4, (700, 3)).astype(np.float32)
    dynamic = rng.uniform(-4, 4, (300, 3)).astype(np.float32)
    orig = np.concatenate([static[:300] + rng.normal(0, 0.06, (300, 3)), dynamic[:200] + rng.normal(0, 0.06, (200, 3)),
                           rng.uniform(-4, 4, (300, 3))]).astype(np.float32)
    ps = rng.random(len(orig)) < 0.6
    want = metric.classify_map_points(orig, ps, static, dynamic, oracle.nn_search)
    for nn_fn in (evr.grid_nn, evr.brute_nn):
        got, counts = evr.classify(orig, ps, static, dynamic, nn_fn=nn_fn)
        assert np.array_equal(got, want) and counts.tolist() == np.bincount(want, minlength=5).tolist()
    assert (np.bincount(want, minlength=5) > 0).all()
    got, _ = evr.classify(orig, ps, static, np.zeros((0, 3), np.float32))
    assert np.array_equal(got, metric.classify_map_points(orig, ps, static, np.zeros((0, 3), np.float32), oracle.nn_search))


def test_argument_errors_come_before_the_device(scvod):
    """a NULL ctx is SCVOD_ERR_INVALID whatever else is passed: no device is touched and nothing is written"""
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data_as(C.c_void_p)
    par = scvod.eval_params_default()
    many = scvod.eval_params_default()
    many.n_dynamic_classes = 17
    assert lib.scvod_evaluate_device(None, p, p, 4, p, p, 4, C.byref(par), p, None) == INVALID
    assert lib.scvod_evaluate_device(None, p, p, -1, p, p, 4, C.byref(par), None, None) == INVALID
    assert lib.scvod_evaluate_device(None, p, p, 4, p, p, -1, C.byref(par), None, None) == INVALID
    assert lib.scvod_evaluate_device(None, p, p, 4, p, p, 4, C.byref(many), None, None) == INVALID
    assert lib.scvod_batch_evaluate(None, p, p, 0, C.byref(par), None, None) == INVALID
    assert lib.scvod_batch_evaluate(None, p, p, 8, C.byref(par), None, None) == INVALID
    assert lib.scvod_batch_evaluate(None, p, p, 0, C.byref(many), None, None) == INVALID
    assert lib.scvod_evaluate_stats(None, C.byref(scvod.EVAL_RESULT())) == INVALID
    assert lib.scvod_classify_map_device(None, p, p, 4, p, 4, p, 4, 0.15, 0.1, p, None) == INVALID
    assert lib.scvod_classify_map_device(None, p, p, -1, p, 4, p, 4, 0.15, 0.1, p, None) == INVALID
    assert lib.scvod_classify_map_stats(None, p) == INVALID
    assert lib.scvod_evaluate_scratch_bytes(None) == 0
    assert not buf.any()
