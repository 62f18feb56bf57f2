"""scvod_batch_point_classes / scvod_score_classes_device / scvod_batch_score_classes / scvod_score_classes_stats without a GPU: the
symbols and the structs, the defaults, scvod_class_finish against the numpy statement (tests/helpers/class_score_ref.py) bit for bit,
the NaN rule, the argument errors that come before a device is looked for, and the helper's rules against known answers worked out by
hand (no golden file of the reference is possible: its plotObject.cpp needs PCL).  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import class_score_ref as csr  # noqa: E402

NEW = ("scvod_batch_point_classes", "scvod_class_params_default", "scvod_class_finish", "scvod_score_classes_device",
       "scvod_batch_score_classes", "scvod_score_classes_stats", "scvod_score_classes_scratch_bytes")
INVALID = -1
OTHER, GROUND, BUILDING, TREE, NONE = range(5)
PT_GROUND, PT_REJECTED, PT_UNCLUSTERED, PT_OTHER, PT_CAR, PT_DYNAMIC, PT_BUILDING = 1, 2, 3, 4, 5, 6, 7


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_symbols_declared_and_exported_and_the_structs(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("batch_point_classes", "score_classes_device", "batch_score_classes", "score_classes_stats"):
        assert callable(getattr(scvod.Ctx, m))
    assert re.search(r"#define\s+SCVOD_PT_STATIC_BUILDING\s+7\b", hdr) and scvod.PT_STATIC_BUILDING == 7 == csr.PT_STATIC_BUILDING
    P, R = scvod.ClassParams, scvod.CLASS_RESULT
    assert C.sizeof(P) == 68
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("max_dist", 0), ("cell", 4), ("n_ground", 8), ("n_building", 12),
                                                                 ("n_tree", 16), ("ground", 20), ("building", 36), ("tree", 52)]
    assert C.sizeof(R) == 264
    assert [(f, getattr(R, f).offset) for f, _ in R._fields_] == [("conf", 0), ("pd_far", 160), ("num", 168), ("P", 200), ("rate_P", 232),
                                                                 ("rate_N", 248)]
    body = hdr[hdr.index("typedef struct scvod_class_result {"):hdr.index("} scvod_class_result;")]
    assert re.findall(r"\b(conf|pd_far|num|P|rate_P|rate_N)\b(?=[\[,;])", body) == ["conf", "pd_far", "num", "P", "rate_P", "rate_N"]


def test_params_default(scvod):
    p = scvod.class_params_default()
    assert _bits(p.max_dist) == _bits(0.75) and _bits(p.cell) == _bits(0.25)
    assert (p.n_ground, p.n_building, p.n_tree) == (6, 4, 3)
    assert tuple(p.ground[:6]) == (40, 44, 48, 49, 71, 72) == csr.GROUND and not any(p.ground[6:])
    assert tuple(p.building[:4]) == (50, 51, 52, 60) == csr.BUILDING and not any(p.building[4:])
    assert tuple(p.tree[:3]) == (70, 80, 81) == csr.TREE and not any(p.tree[3:])
    q = scvod.class_params_default(max_dist=1.5, cell=0.1, tree=[], ground=[9])
    assert _bits(q.max_dist) == _bits(1.5) and _bits(q.cell) == _bits(0.1) and q.n_tree == 0 and q.n_ground == 1 and q.ground[0] == 9
    assert q.n_building == 4


def test_finish_equals_the_helper_on_seeded_counts(scvod):
    rng = np.random.default_rng(20261018)
    for i in range(1000):
        conf = rng.integers(0, 10 ** int(rng.integers(1, 11)), (4, 5)).astype(np.int64)
        if i % 100 == 0:
            conf[int(rng.integers(0, 4))] = 0                  # a class without a point: NaN rates
        far = int(rng.integers(0, int(conf[3, 1:4].sum()) + 1))
        r = scvod.class_finish(list(conf.reshape(-1)) + [far])
        num, P, rate_P, rate_N = csr.finish(conf, far)
        assert r["conf"] == conf.tolist() and r["pd_far"] == far
        assert r["num"] == num.tolist() == conf.sum(1).tolist() and r["P"] == P.tolist()
        # fp32 bits; NaN compares through one pattern
        for got, want in ((r["rate_P"], rate_P), (r["rate_N"], rate_N)):
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(_bits(got)[~np.isnan(want)], _bits(want)[~np.isnan(want)]), (conf, far)
        for t in range(4):
            if num[t]:
                # the operations written out: both operands converted to fp32, one fp32 division
                assert _bits(r["rate_P"][t]) == _bits(np.float32(P[t]) / np.float32(num[t]))
                assert _bits(r["rate_N"][t]) == _bits(np.float32(num[t] - P[t]) / np.float32(num[t]))


def test_nan_where_a_class_has_no_point(scvod):
    r = scvod.class_finish([0] * 21)
    assert np.isnan(r["rate_P"]).all() and np.isnan(r["rate_N"]).all() and r["num"] == [0, 0, 0, 0]
    conf = np.zeros((4, 5), np.int64)
    conf[0] = [1, 3, 0, 0, 0]
    r = scvod.class_finish(list(conf.reshape(-1)) + [0])
    assert r["rate_P"][0] == np.float32(0.75) and r["rate_N"][0] == np.float32(0.25) and np.isnan(r["rate_P"][1:]).all()
    want = csr.finish(conf, 0)
    assert np.array_equal(np.isnan(r["rate_N"]), np.isnan(want[3]))


def test_argument_errors_come_before_the_device(scvod):
    """a NULL ctx is SCVOD_ERR_INVALID whatever else is passed: no device is touched and nothing is written"""
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data_as(C.c_void_p)
    par = scvod.class_params_default()
    assert lib.scvod_score_classes_device(None, p, p, 4, p, p, 4, C.byref(par), p, None) == INVALID
    assert lib.scvod_score_classes_device(None, p, p, -1, p, p, 4, C.byref(par), None, None) == INVALID
    assert lib.scvod_score_classes_device(None, p, p, 4, p, p, -1, C.byref(par), None, None) == INVALID
    assert lib.scvod_score_classes_device(None, None, p, 4, p, p, 4, C.byref(par), None, None) == INVALID
    assert lib.scvod_score_classes_device(None, p, p, 4, p, None, 4, C.byref(par), None, None) == INVALID
    bad = []
    for name in ("ground", "building", "tree"):
        q = scvod.class_params_default()
        setattr(q, "n_" + name, 9)
        bad.append(q)
    for field in ("cell", "max_dist"):
        for v in (0.0, -0.25, float("inf"), float("nan")):
            bad.append(scvod.class_params_default(**{field: v}))
    bad.append(scvod.class_params_default(max_dist=0.70))                       # 0.49 <= 0.5
    bad.append(scvod.class_params_default(max_dist=float(np.sqrt(np.float32(0.5)))))  # the fp32 product does not exceed 0.5
    for q in bad:
        assert lib.scvod_score_classes_device(None, p, p, 4, p, p, 4, C.byref(q), None, None) == INVALID
        assert lib.scvod_batch_score_classes(None, p, p, 0, C.byref(q), None, None) == INVALID
    assert lib.scvod_batch_score_classes(None, p, p, 0, C.byref(par), None, None) == INVALID
    assert lib.scvod_batch_score_classes(None, p, p, 8, C.byref(par), None, None) == INVALID
    assert lib.scvod_batch_point_classes(None, p, 64, 0, None) == INVALID
    assert lib.scvod_batch_point_classes(None, p, -1, 0, None) == INVALID
    assert lib.scvod_score_classes_stats(None, C.byref(scvod.CLASS_RESULT())) == INVALID
    assert lib.scvod_score_classes_scratch_bytes(None) == 0
    assert not buf.any()


# ---- the helper's rules against answers worked out by hand ---------------------------------------------------------------------------

def _one(gt, label, est, est_pt, **kw):
    r = csr.score(np.asarray(gt, np.float32).reshape(-1, 3), np.asarray(label, np.uint32), np.asarray(est, np.float32).reshape(-1, 3),
                  np.asarray(est_pt, np.uint8), **kw)
    assert int(np.sum(r["conf"])) == len(label)
    return r


def test_known_answer_each_truth_class_against_each_estimate_class():
    # four estimate points 10 m apart, one per estimate class; next to each (0.1 m: d = 0.01) one truth point of every class
    est = np.array([[0, 0, 0], [10, 0, 0], [20, 0, 0], [30, 0, 0]], np.float32)
    est_pt = [PT_CAR, PT_GROUND, PT_BUILDING, PT_OTHER]           # other, ground, building, tree
    labels = [40, 50, 70, 10]                                     # ground, building, tree, pd (a car)
    gt = np.array([[e[0] + 0.1, 0, 0] for e in est for _ in labels], np.float32)
    lab = np.array(labels * 4, np.uint32)
    r = _one(gt, lab, est, est_pt)
    assert r["conf"] == [[1, 1, 1, 1, 0]] * 4 and r["pd_far"] == 0
    #            neighbour: other          ground         building       tree
    want_P = [0, 0, 0, 1,   1, 0, 0, 0,   0, 1, 1, 0,   0, 1, 1, 0]    # truth ground, building, tree, pd under each
    want = [t | (e << 2) | (32 * p) for (e, t), p in zip(((e, t) for e in range(4) for t in range(4)), want_P)]
    assert r["point_result"].tolist() == want
    assert r["num"] == [4, 4, 4, 4] and r["P"] == [1, 2, 2, 1]
    assert r["rate_P"].tolist() == [0.25, 0.5, 0.5, 0.25] and r["rate_N"].tolist() == [0.75, 0.5, 0.5, 0.75]
    # the bytes that count as `other`
    for pt in (0, PT_REJECTED, PT_UNCLUSTERED, PT_CAR, PT_DYNAMIC):
        assert _one([[0.1, 0, 0]], [10], [[0, 0, 0]], [pt])["point_result"].tolist() == [3 | (OTHER << 2) | 32]


def test_known_answer_pd_at_half_a_square_metre():
    # d = 0.25 + 0.25 = 0.5f exactly: not > 0.5, the neighbour is a tree -> N
    r = _one([[0, 0, 0]], [10], [[0.5, 0.5, 0]], [PT_OTHER])
    assert _bits(r["nn_sq"][0]) == _bits(0.5)
    assert r["point_result"].tolist() == [3 | (TREE << 2)] and r["pd_far"] == 0 and r["P"][3] == 0 and r["conf"][3] == [0, 0, 0, 1, 0]


def test_known_answer_pd_one_ulp_beyond():
    # dz = 2^-12: d = (0.25 + 0.25) + 2^-24 = nextafter(0.5f, 1): > 0.5 -> P, counted in pd_far; the neighbour (< 0.5625) still counts
    r = _one([[0, 0, 0]], [10], [[0.5, 0.5, 2.0 ** -12]], [PT_OTHER])
    assert _bits(r["nn_sq"][0]) == _bits(np.nextafter(np.float32(0.5), np.float32(1)))
    assert r["point_result"].tolist() == [3 | (TREE << 2) | 32] and r["pd_far"] == 1 and r["P"][3] == 1 and r["conf"][3] == [0, 0, 0, 1, 0]
    # the same distance for a tree truth point: P by its class rule, and no pd_far
    r = _one([[0, 0, 0]], [70], [[0.5, 0.5, 2.0 ** -12]], [PT_OTHER])
    assert r["point_result"].tolist() == [2 | (TREE << 2) | 32] and r["pd_far"] == 0


def test_known_answer_tie_goes_to_the_lower_index():
    # a ground and a building estimate at d = 0.0625 on either side of a ground truth point
    gt, lab = [[1.0, 0, 0]], [40]
    pair = np.array([[0.75, 0, 0], [1.25, 0, 0]], np.float32)
    r = _one(gt, lab, pair, [PT_GROUND, PT_BUILDING])
    assert r["nn_idx"].tolist() == [0] and r["point_result"].tolist() == [0 | (GROUND << 2) | 32]
    r = _one(gt, lab, pair, [PT_BUILDING, PT_GROUND])
    assert r["nn_idx"].tolist() == [0] and r["point_result"].tolist() == [0 | (BUILDING << 2)]
    r = _one(gt, lab, pair[::-1], [PT_BUILDING, PT_GROUND])
    assert r["point_result"].tolist() == [0 | (BUILDING << 2)]


def test_known_answer_instance_bits_are_masked():
    # 50 with an instance id above it is a building; 0x0032 in the upper half alone is not
    r = _one([[0.1, 0, 0], [0.2, 0, 0]], [(77 << 16) | 50, 50 << 16], [[0, 0, 0]], [PT_BUILDING])
    assert r["point_result"].tolist() == [1 | (BUILDING << 2) | 32, 3 | (BUILDING << 2)] and r["num"] == [0, 1, 0, 1]
    assert csr.truth_class(np.array([40, 44, 48, 49, 71, 72, 50, 51, 52, 60, 70, 80, 81, 10, 252, 0, 99], np.uint32)).tolist() == \
        [0] * 6 + [1] * 4 + [2] * 3 + [3] * 4
    # a label in two lists: ground is tested first
    assert csr.truth_class(np.array([50], np.uint32), ground=(50,), building=(50,)).tolist() == [0]


def test_known_answer_the_only_estimate_beyond_max_dist():
    # 0.80 m: d = 0.64 >= 0.5625 -> none: N for the ground point, P for a pd point at the same place (d > 0.5 in the reference too)
    r = _one([[0, 0, 0], [0, 0, 0]], [40, 10], [[0.8, 0, 0]], [PT_GROUND])
    assert r["point_result"].tolist() == [0 | (NONE << 2), 3 | (NONE << 2) | 32]
    assert r["conf"][0] == [0, 0, 0, 0, 1] and r["conf"][3] == [0, 0, 0, 0, 1] and r["pd_far"] == 0 and r["P"] == [0, 0, 0, 1]
    # just inside: 0.74 m
    r = _one([[0, 0, 0]], [40], [[0.74, 0, 0]], [PT_GROUND])
    assert r["point_result"].tolist() == [0 | (GROUND << 2) | 32]


def test_the_batch_scale_lookup_equals_the_brute_force():
    rng = np.random.default_rng(4)
    est = rng.uniform(-3, 3, (1500, 3)).astype(np.float32)
    est[100:110] = est[0]                                           # eleven points in one place: more ties than candidates asked for
    est[200:202] = est[1]
    gt = np.concatenate([est[:600], est[:600] + rng.normal(0, 0.2, (600, 3)), rng.uniform(-5, 5, (800, 3)),
                         (est[300:310] + est[310:320]) / 2]).astype(np.float32)
    lab = rng.choice([40, 50, 70, 10, 252], len(gt)).astype(np.uint32)
    pt = rng.choice([1, 2, 3, 4, 5, 6, 7], len(est)).astype(np.uint8)
    a = csr.score(gt, lab, est, pt)
    b = csr.score(gt, lab, est, pt, nn_fn=csr.tree_nn)
    near = a["nn_sq"] < np.float32(0.75) * np.float32(0.75)
    assert 0 < int(near.sum()) < len(gt)
    assert np.array_equal(a["nn_idx"][near], b["nn_idx"][near]) and np.array_equal(_bits(a["nn_sq"][near]), _bits(b["nn_sq"][near]))
    assert a["conf"] == b["conf"] and a["pd_far"] == b["pd_far"] and np.array_equal(a["point_result"], b["point_result"])
    assert a["nn_idx"][0] == 0 and a["nn_idx"][1] == 1                # the lowest of the coincident points
