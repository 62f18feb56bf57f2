"""The ESF descriptor (scvod_esf_device, scvod_batch_object_esf) without a GPU: the symbols and the record's layout, the argument
errors that come before a device is looked for, the cosine literals of scvod_math.h, scvod_esf_fold10 / scvod_feature_row21 against
written-out numpy, and the CPU helper (tests/helpers/object_esf_ref.py: the C++ loop over one object's points and samples in the
library's esf_* functions) against the numpy restatement of the definition that does not read the header.  The operations are the
same IEEE operations, so equality is the bar, not a tolerance.  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import object_esf_ref as oer  # noqa: E402

NEW = ("scvod_esf_params_default", "scvod_esf_device", "scvod_batch_object_esf", "scvod_esf_stats", "scvod_esf_scratch_bytes",
       "scvod_esf_fold10", "scvod_feature_row21")
FIELDS = (("fold10", 0), ("n_valid", 40), ("n_points", 44), ("flags", 48), ("lines", 52))
SAMPLES = 2000


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return oer.build(tmp_path_factory.mktemp("objesfref"))


@pytest.fixture(scope="module")
def cases(ref):
    """name -> (points, the helper's result, the numpy restatement's) at SAMPLES samples, computed once"""
    return {name: (x, oer.esf(ref, x, SAMPLES), oer.esf_numpy(x, SAMPLES)) for name, x in oer.esf_cases().items()}


def test_symbols_declared_and_exported_and_the_record_layout(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    assert scvod.EXPORTED_SYMBOLS[-len(NEW):] == list(NEW), "the new names are appended"
    assert C.sizeof(scvod.ObjectEsf) == 64 == scvod.OBJECT_ESF_DTYPE.itemsize == oer.OBJECT_ESF_DTYPE.itemsize
    for name, off in FIELDS:
        assert getattr(scvod.ObjectEsf, name).offset == off, name
        assert scvod.OBJECT_ESF_DTYPE.fields[name][1] == off == oer.OBJECT_ESF_DTYPE.fields[name][1], name
    assert scvod.OBJECT_ESF_DTYPE == oer.OBJECT_ESF_DTYPE
    body = hdr[hdr.index("typedef struct scvod_object_esf {"):hdr.index("} scvod_object_esf;")]
    assert re.findall(r"^\s*(?:u?int\d+_t|float|double)\s+(\w+)", body, re.M) == [f for f, _ in FIELDS]
    body = hdr[hdr.index("typedef struct scvod_esf_params {"):hdr.index("} scvod_esf_params;")]
    assert re.findall(r"^\s*(?:u?int\d+_t|float|double)\s+(\w+)", body, re.M) == [f for f, _ in scvod.EsfParams._fields_]
    assert C.sizeof(scvod.EsfParams) == 32
    p = scvod.esf_params_default()
    assert (p.samples, p.seed, p.min_points, p.cls_mask, list(p.reserved)) == (20000, 0, 3, 0xFFFFFFFF, [0, 0, 0, 0])
    assert f"#define SCVOD_ESF_CACHE_POINTS {scvod.ESF_CACHE_POINTS} " in hdr


def test_argument_errors_come_before_the_device(scvod):
    lib = scvod.load_lib()
    buf = np.zeros(256, np.int64)
    p = buf.ctypes.data_as(C.c_void_p)
    good = scvod.esf_params_default()
    assert lib.scvod_esf_device(None, p, p, 1, C.byref(good), p, None, 1, None) == -1
    assert lib.scvod_esf_device(None, None, None, 1, None, p, None, 1, None) == -1
    assert lib.scvod_esf_device(None, p, p, -1, None, p, None, 1, None) == -1
    assert lib.scvod_esf_device(None, p, p, 1, None, None, None, 1, None) == -1
    assert lib.scvod_esf_device(None, p, p, 1, None, p, None, -1, None) == -1
    for bad in (dict(samples=0), dict(samples=65537), dict(samples=-1), dict(min_points=2), dict(min_points=0)):
        q = scvod.esf_params_default(**bad)
        assert lib.scvod_esf_device(None, p, p, 1, C.byref(q), p, None, 1, None) == -1, bad
        assert lib.scvod_batch_object_esf(None, C.byref(q), p, None, 1, None) == -1, bad
    assert lib.scvod_batch_object_esf(None, None, p, None, 1, None) == -1
    assert lib.scvod_batch_object_esf(None, None, None, None, 1, None) == -1
    assert lib.scvod_esf_stats(None, p) == -1
    assert lib.scvod_esf_scratch_bytes(None) == 0
    lib.scvod_esf_params_default(None)
    lib.scvod_esf_fold10(None, p)
    lib.scvod_feature_row21(None, None, None, p)
    assert not buf.any()


def test_cosine_literals_against_numpy(ref):
    T = oer.cos_table(ref)
    b = np.arange(1, 64, dtype=np.float64)
    want = np.cos((b - 0.5) * np.pi / 126.0).astype(np.float32)
    assert np.array_equal(T[1:].view(np.uint32), want.view(np.uint32)), "SCVOD_ESF_COS_TABLE is not (float)cos((b - 0.5) pi / 126)"
    assert (np.diff(T[1:]) < 0).all() and T[0] > 1, "descending: the bisection of esf_angle_bin counts what the definition counts"
    hdr = open(os.path.join(ROOT, "dr-using-scv-od_amd", "csrc", "scvod_math.h")).read()
    body = hdr[hdr.index("#define SCVOD_ESF_COS_TABLE"):]
    body = body[:body.index("}")]
    lit = [np.float32(v) for v in re.findall(r"(\d+\.\d+(?:e-?\d+)?)f", body)]
    assert len(lit) == 64 and np.array_equal(np.asarray(lit[1:], np.float32).view(np.uint32), want.view(np.uint32)), "the 63 literals in the header"


def test_fold10_and_feature_row21_against_numpy(scvod, cases):
    sig = cases["block"][1]["sig"]
    assert abs(float(sig.astype(np.float64).sum()) - 1.0) < 1e-4
    want = np.asarray([np.float32(np.add.accumulate(sig[j::10].astype(np.float64))[-1]) for j in range(10)], np.float32)
    got = scvod.esf_fold10(sig)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), cases["block"][1]["record"]["fold10"].view(np.uint32)), "the record holds the same fold"
    rng = np.random.default_rng(3)
    noise = rng.random(640).astype(np.float32)
    want = np.asarray([np.float32(sum(float(v) for v in noise[j::10])) for j in range(10)], np.float32)
    assert np.array_equal(scvod.esf_fold10(noise).view(np.uint32), want.view(np.uint32))
    o = np.zeros(1, scvod.OBJECT_DTYPE)
    o["box_min"], o["box_max"], o["angle_diff"], o["cls"] = (1.25, -2.5, -1.5), (3.5, 0.75, 0.25), 37.5, 2
    sh = np.zeros(1, scvod.OBJECT_SHAPE_DTYPE)
    sh["feat"] = np.arange(7) * 0.125 + 0.0625
    e = cases["plate"][1]["record"]
    for shape in (None, sh):
        row = scvod.feature_row21(o, shape, e)
        assert np.array_equal(row[:11], scvod.feature_row(o, shape)), "columns 0-10 are scvod_feature_row's"
        assert np.array_equal(row[11:], e["fold10"].astype(np.float64)), "columns 11-20 are fold10 as doubles"
    assert row.shape == (21,)


def test_helper_equals_the_numpy_restatement_on_every_crafted_object(cases):
    for name, (x, a, b) in cases.items():
        assert np.array_equal(a["hist"], b["hist"]), f"{name}: integer counters differ at {np.nonzero(a['hist'] != b['hist'])[0][:8]}"
        for f in ("n_valid", "n_points", "flags"):
            assert a["record"][f] == b["record"][f], (name, f, a["record"], b["record"])
        assert np.array_equal(a["record"]["lines"], b["record"]["lines"]), name
        assert np.array_equal(a["triangles"], b["triangles"]), name
        assert np.array_equal(a["sig"].view(np.uint32), b["sig"].view(np.uint32)), f"{name}: the normalised signature"
        assert a["record"].tobytes() == b["record"].tobytes(), f"{name}: the record's bytes"
        r = a["record"]
        print(f"{name}: {len(x)} points, {r['n_valid']} valid of {SAMPLES}, lines IN/OUT/MIX {r['lines'].tolist()}, "
              f"triangles OUT/IN/MIX {a['triangles'].tolist()}, flags {r['flags']}")
        assert r["lines"].sum() == 3 * r["n_valid"] and a["triangles"].sum() == r["n_valid"]
        h = a["hist"].reshape(10, 64)
        assert h[:3].sum() == 3 * r["n_valid"] and h[3:6].sum() == r["n_valid"] and h[6:9].sum() == 3 * r["n_valid"]
        assert h[9].sum() == r["lines"][2], "one ratio entry per MIX line"
        if r["flags"]:
            assert not a["sig"].any() and not r["fold10"].any()
        else:
            assert np.isfinite(r["fold10"]).all() and abs(float(r["fold10"].sum()) - 1.0) < 1e-4


def test_what_the_crafted_objects_show(cases):
    for name in ("block", "plate"):
        h = cases[name][1]["hist"].reshape(10, 64)
        assert (h.sum(axis=1) > 0).all(), f"{name}: an empty histogram among the ten: {h.sum(axis=1)}"
    for name, (x, a, _) in cases.items():
        if len(np.unique(x, axis=0)) >= 30:
            # three distinct draws out of 30 happen with probability 0.90
            assert a["record"]["n_valid"] >= 0.85 * SAMPLES, (name, a["record"]["n_valid"])
    clumps = cases["clumps"][1]
    assert clumps["triangles"][0] == clumps["record"]["n_valid"] and clumps["record"]["lines"][2] == 0, "clumps far apart: all OUT"
    x = cases["xaxis"][1]["record"]
    assert x["flags"] == 1 and x["n_valid"] == 0 and x["n_points"] == 9, "collinear points: no triangle has an area"
    assert cases["equal"][1]["record"]["flags"] == 4, "four equal points have no extent"
    assert cases["two"][1]["record"]["flags"] == 2
    three = cases["three"][1]["record"]
    assert three["flags"] == 0 and 0 < three["n_valid"] < SAMPLES // 2, "three points: two draws in nine are a triangle"


def test_seed_sample_count_and_min_points(ref):
    x = oer.esf_cases()["block30"]
    a, b = oer.esf(ref, x, SAMPLES, seed=0), oer.esf(ref, x, SAMPLES, seed=1)
    assert a["record"].tobytes() != b["record"].tobytes() and not np.array_equal(a["hist"], b["hist"]), "different seeds, different records"
    assert oer.esf(ref, x, SAMPLES, seed=0)["record"].tobytes() == a["record"].tobytes(), "the same seed, the same record"
    for s, seed in ((1, 5), (63, 0), (257, 0xFFFFFFFF)):
        c, d = oer.esf(ref, x, s, seed), oer.esf_numpy(x, s, seed)
        assert c["record"].tobytes() == d["record"].tobytes() and np.array_equal(c["hist"], d["hist"]), (s, seed)
    assert oer.esf(ref, x, SAMPLES, min_points=31)["record"]["flags"] == 2 and oer.esf(ref, x, SAMPLES, min_points=30)["record"]["flags"] == 0
    # an object's record does not depend on where its points sit in a larger array
    assert oer.esf(ref, np.concatenate([x, x])[:30], SAMPLES)["record"].tobytes() == a["record"].tobytes()
    nan = x.copy()
    nan[3, 1] = np.nan
    assert oer.esf(ref, nan, 64)["record"]["flags"] == 4 == oer.esf_numpy(nan, 64)["record"]["flags"], "a point that is no number: no extent"
