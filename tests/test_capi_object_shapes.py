"""scvod_batch_object_shapes and its host-only companions without a GPU: the symbols and the record's layout, the argument errors that
come before a device is looked for, scvod_feature_row / scvod_compare_feature, the restated log / exp / pow of scvod_math.h against
this image's glibc (counts and distances measured and pinned, as tests/test_math_spec.py pins atan2's), and the CPU helper
(tests/helpers/object_shape_ref.py: the C++ loop over one object's points) against independent numpy math.  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import object_shape_ref as osr  # noqa: E402

NEW = ("scvod_feature_params_default", "scvod_set_object_features", "scvod_batch_object_shapes", "scvod_batch_object_shapes_stats",
       "scvod_feature_row", "scvod_compare_feature")
FIELDS = (("cov", 0), ("eig", 24), ("flags", 36), ("feat", 40))
SEED = 20261017
# measured on the clouds of `clouds()` below (printed by the test): the largest |eig - eigvalsh(cov)| / (largest eigenvalue * 2^-24)
EIG_MEASURED = 7.01
EIG_BOUND = 4 * EIG_MEASURED   # four times the measured maximum: Jacobi sweeps accumulate a handful of roundings, other seeds need room


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return osr.build(tmp_path_factory.mktemp("objshaperef"))


def test_symbols_declared_and_exported_and_the_record_layout(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    assert C.sizeof(scvod.ObjectShape) == 96 == scvod.OBJECT_SHAPE_DTYPE.itemsize == osr.OBJECT_SHAPE_DTYPE.itemsize
    for name, off in FIELDS:
        assert getattr(scvod.ObjectShape, name).offset == off, name
        assert scvod.OBJECT_SHAPE_DTYPE.fields[name][1] == off == osr.OBJECT_SHAPE_DTYPE.fields[name][1], name
    assert scvod.OBJECT_SHAPE_DTYPE == osr.OBJECT_SHAPE_DTYPE
    body = hdr[hdr.index("typedef struct scvod_object_shape {"):hdr.index("} scvod_object_shape;")]
    assert re.findall(r"^\s*(?:u?int\d+_t|float|double)\s+(\w+)", body, re.M) == [f for f, _ in FIELDS]
    assert C.sizeof(scvod.FeatureParams) == 64
    p = scvod.feature_params()
    assert tuple(getattr(p, n) for n, _ in scvod.FeatureParams._fields_) == osr.DEFAULT_K   # utility.h:318-325
    assert len(scvod.FEATURE_NAMES) == 7


def test_argument_errors_come_before_the_device(scvod):
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data_as(C.c_void_p)
    good = scvod.feature_params()
    assert lib.scvod_set_object_features(None, C.byref(good)) == -1
    assert lib.scvod_set_object_features(None, None) == -1
    assert lib.scvod_batch_object_shapes(None, p, 4, None) == -1
    assert lib.scvod_batch_object_shapes(None, None, 4, None) == -1
    assert lib.scvod_batch_object_shapes(None, p, -1, None) == -1
    assert lib.scvod_batch_object_shapes_stats(None, p) == -1
    lib.scvod_feature_params_default(None)
    lib.scvod_feature_row(None, None, p)
    assert not buf.any()


def _object(scvod):
    o = np.zeros(1, scvod.OBJECT_DTYPE)
    o["box_min"], o["box_max"] = (1.25, -2.5, -1.5), (3.5, 0.75, 0.25)
    o["angle_diff"], o["cls"] = 37.5, 2
    return o


def test_feature_row(scvod):
    o = _object(scvod)
    row = scvod.feature_row(o)                        # shape NULL: the row the reference builds today
    sq = float(np.float32(3.5) - np.float32(1.25)) * float(np.float32(0.75) - np.float32(-2.5))
    assert row.tolist() == [1.0] * 6 + [0.25, sq, 37.5, -1.5, 2.0]
    sh = np.zeros(1, scvod.OBJECT_SHAPE_DTYPE)
    sh["feat"] = [0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875]
    row = scvod.feature_row(o, sh)
    assert row.tolist() == [0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.25, sq, 37.5, -1.5, 2.0]   # (column 6 stays point_max.z)


def test_compare_feature(scvod):
    a = np.asarray([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0])
    b = np.asarray([0.0, 4.0, 2.0, 6.0, 4.0, 8.0, 6.0, 10.0, 8.0, 110.0, -5.0])
    # |a - b| = 1 2 1 2 1 2 1 2 1 100 (16): weights 0.5 0.5 0.2 0.2 0.2 0.2 0.2 0.6 0.2 0.0, column 10 is not read
    want = np.float32(0.0)
    for d, w in zip((1, 2, 1, 2, 1, 2, 1, 2, 1, 100), (0.5, 0.5, 0.2, 0.2, 0.2, 0.2, 0.2, 0.6, 0.2, 0.0)):
        want = np.float32(np.float64(want) + np.float64(d) * np.float64(w))
    got = scvod.compare_feature(a, b)
    assert got == float(want) and abs(got - 4.3) < 1e-6       # 0.5 + 1.0 + 0.2 + 0.4 + 0.2 + 0.4 + 0.2 + 1.2 + 0.2 + 0
    assert scvod.compare_feature(a, a) == 0.0 and scvod.compare_feature(b, a) == got
    # a float accumulator is not a double one: 2^24 + 1 is not a float, so the second term is lost; a double sum would keep it
    x, z = np.zeros(11), np.zeros(11)
    x[0], x[1] = 2.0 * (1 << 24), 2.0
    got = scvod.compare_feature(x, z)
    assert got == float(1 << 24) and 0.5 * x[0] + 0.5 * x[1] == float((1 << 24) + 1)


def _ranges():
    """the arguments the features can reach: log on (0, 1] (a share e_i), pow(., 0.333) on (0, 1/27] (the product of three shares that
    sum to 1), uniform and log-uniform halves"""
    rng = np.random.default_rng(SEED)
    n = 1 << 20
    x = np.concatenate([rng.uniform(0, 1, n), np.exp(rng.uniform(-40, 0, n))])
    y = np.concatenate([rng.uniform(0, 1 / 27, n), np.exp(rng.uniform(-60, np.log(1 / 27), n))])
    return x[(x > 0) & (x <= 1)], y[(y > 0) & (y <= 1 / 27)]


def test_log_exp_pow_against_this_glibc(ref):
    """log_f64 / exp_f64 are fdlibm's, within 1 ulp of the exact value; glibc's are correctly rounded in nearly every case, so a few
    per cent of the results differ by one unit.  pow_f64 is exp(k log x) BY DEFINITION: the rounding of k * log x (up to 20 in size
    here) is magnified by that size, so it is up to 17 ulp from glibc's pow -- measured, pinned and quoted in DESIGN.md section 2"""
    x, y = _ranges()
    got = {}
    for name, arg, k in (("log", x, None), ("pow", y, 0.333), ("exp", 0.333 * np.log(y), None)):
        d = osr.ulp_distance(osr.many(ref, f"spec_{name}_many", arg, k), osr.many(ref, f"libm_{name}_many", arg, k))
        got[name] = (len(arg), int((d != 0).sum()), int(d.max()))
        print(name, got[name])
    assert got["log"] == (2097152, 79105, 1)
    assert got["exp"] == (2097152, 191213, 1)
    assert got["pow"] == (2097152, 1364442, 17)
    # the special cases of the C library
    sp = np.asarray([0.0, -0.0, np.nan, np.inf, -1.0, -np.inf, 1.0])
    with np.errstate(all="ignore"):
        for k in (0.333, -0.333, 0.0, 2.0, 3.0, -3.0):
            a, b = osr.many(ref, "spec_pow_many", sp, k), osr.many(ref, "libm_pow_many", sp, k)
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]), (k, a, b)
            assert np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)])), (k, a, b)
    lg = osr.many(ref, "spec_log_many", np.asarray([0.0, -0.0, -1.0, np.inf, np.nan, 1.0, 5e-324]))
    assert lg[0] == lg[1] == -np.inf and np.isnan(lg[2]) and lg[3] == np.inf and np.isnan(lg[4]) and lg[5] == 0.0
    assert lg[6] == np.log(5e-324)
    ex = osr.many(ref, "spec_exp_many", np.asarray([0.0, -np.inf, np.inf, np.nan, 710.0, -746.0, -740.0]))
    assert ex[0] == 1.0 and ex[1] == 0.0 and ex[2] == np.inf and np.isnan(ex[3]) and ex[4] == np.inf and ex[5] == 0.0
    assert abs(ex[6] / np.exp(-740.0) - 1.0) < 1e-9


def clouds():
    """seeded planes, lines, blobs and boxes of 3..2000 points inside a few metres, somewhere in a scan's range"""
    rng = np.random.default_rng(SEED)
    out = []
    sizes = [3, 4, 5, 7, 17, 63, 64, 65, 127, 128, 129, 500, 1000, 2000]
    for n in sizes:
        for kind in ("plane", "line", "blob", "box"):
            centre = rng.uniform(-30, 30, 3) * np.asarray([1, 1, 0.05])
            R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            if kind == "plane":
                p = rng.uniform(-1, 1, (n, 3)) * np.asarray([2.0, 1.0, 0.005])
            elif kind == "line":
                p = rng.uniform(-1, 1, (n, 3)) * np.asarray([3.0, 0.01, 0.01])
            elif kind == "blob":
                p = rng.normal(0, 0.4, (n, 3))
            else:
                p = rng.uniform(-1, 1, (n, 3)) * np.asarray([2.0, 0.9, 0.8])
            out.append((f"{kind}{n}", (p @ R.T + centre).astype(np.float32)))
    return out


def test_helper_against_independent_math(ref):
    worst_eig = 0.0
    for name, xyz in clouds():
        n = len(xyz)
        r = osr.shape(ref, xyz)
        assert r["flags"] == 0, name
        # cov: an fp64 evaluation of the same sums; sequential summation of n products, each rounded once: (n + 1) roundings per
        # entry, and the products' operands p = xyz - centroid are the specification's own fp32 values -> |error| <= (n + 4) 2^-23
        # sum |a_k b_k| holds with room (2^-24 per rounding)
        cov, mag = osr.cov64(xyz)
        assert (np.abs(r["cov"].astype(np.float64) - cov) <= (n + 4) * 2.0 ** -23 * mag).all(), name
        # eig: numpy's symmetric solver on the helper's own float cov, relative to the largest eigenvalue
        w = np.linalg.eigvalsh(osr.sym(r["cov"]))
        err = np.abs(r["eig"].astype(np.float64) - np.abs(w)[np.argsort(np.abs(w))]).max() / (np.abs(w).max() * 2.0 ** -24)
        worst_eig = max(worst_eig, err)
        assert (np.diff(r["eig"]) >= 0).all() and (r["eig"] >= 0).all(), name
        # the five rational features: the same formulas in numpy fp64 from the helper's own eig, exactly
        assert np.array_equal(r["feat"][[0, 1, 2, 4, 6]], osr.rational_features(r["eig"])), name
        # the two transcendental ones against numpy's log / power at the distance measured above (17 ulp of pow, 1 of log, + the sums)
        ev = r["eig"].astype(np.float64) / np.float64(np.float32(np.float32(r["eig"][0] + r["eig"][1]) + r["eig"][2]))
        if (ev > 0).all():
            omni = abs(np.power(ev[0] * ev[1] * ev[2], 0.333) / 0.278636)
            ent = abs(ev[0] * np.log(ev[0]) + ev[1] * np.log(ev[1]) + ev[2] * np.log(ev[2]) / 0.956129)
            assert abs(r["feat"][3] - omni) <= 20 * 2.0 ** -52 * omni, name
            assert abs(r["feat"][5] - ent) <= 8 * 2.0 ** -52 * np.abs(ev * np.log(ev)).sum(), name
    print("largest eigenvalue error in units of 2^-24 of the largest eigenvalue:", worst_eig)
    assert worst_eig <= EIG_BOUND
    assert worst_eig >= EIG_MEASURED / 4, "EIG_MEASURED no longer describes these clouds"


def test_degenerate_objects(ref):
    same = np.tile(np.asarray([[12.5, -3.25, -0.75]], np.float32), (40, 1))
    r = osr.shape(ref, same)
    assert r["flags"] == 1 and not r["cov"].any() and not r["eig"].any() and np.isnan(r["feat"]).all()
    two = np.asarray([[1.0, 2.0, 0.5], [1.5, 2.25, -0.5]], np.float32)
    r = osr.shape(ref, two)
    assert r["flags"] & 2 and r["eig"][2] > 0
    one = osr.shape(ref, two[:1])
    assert one["flags"] == 3
    # non-default constants are honoured: each rational feature scales with 1 / its maximum
    xyz = clouds()[10][1]
    a = osr.shape(ref, xyz)
    K = list(osr.DEFAULT_K)
    K[1], K[7] = K[1] * 2, K[7] * 4
    b = osr.shape(ref, xyz, K)
    assert b["feat"][0] == a["feat"][0] / 2 and b["feat"][6] == a["feat"][6] / 4 and np.array_equal(a["feat"][1:6], b["feat"][1:6])
    assert np.array_equal(a["eig"], b["eig"])
