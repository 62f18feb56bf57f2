"""SSC::regionGrowing (src/ssc.cpp:797-832) on the CPU (tests/helpers/region_growing_ref.cpp): the literal PCL-order restatement
against the min-key form the device runs, on random clouds; the spec's eigen33 and sin / cos.  Not gpu."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COS10 = 0x3F7C1C5C            # cosf((float)(10.0 / 180.0 * M_PI))
REF = (10, 20, 1000000)       # k, min and max segment (ssc.cpp:803-810)


def build_rg(out_dir):
    src = os.path.join(ROOT, "tests", "helpers", "region_growing_ref.cpp")
    so = os.path.join(str(out_dir), "librgref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    args = [fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_double, fp, ip]
    lib.rg_literal.argtypes = args
    lib.rg_minkey.argtypes = args + [C.POINTER(C.c_long)]
    lib.host_cosf.restype = C.c_float
    lib.host_cosf.argtypes = [C.c_float]
    return lib


def run(lib, xyz, form="literal", k=10, min_seg=20, max_seg=1000000, cos_t=None, curv=1.2, frac=0.2):
    """one cluster (points in index order): (class 3 building / 1 tree, normal_curv [n, 4], segment [n], stats or None)"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = len(xyz)
    if cos_t is None:
        cos_t = struct.unpack("<f", struct.pack("<I", COS10))[0]
    nc = np.zeros((max(n, 1), 4), np.float32)
    seg = np.zeros(max(n, 1), np.int32)
    a = [xyz.ctypes.data_as(C.POINTER(C.c_float)), n, k, min_seg, max_seg, C.c_float(cos_t), C.c_float(curv), C.c_double(frac),
         nc.ctypes.data_as(C.POINTER(C.c_float)), seg.ctypes.data_as(C.POINTER(C.c_int))]
    if form == "literal":
        return lib.rg_literal(*a), nc[:n], seg[:n], None
    st = (C.c_long * 2)()
    cls = lib.rg_minkey(*a, st)
    return cls, nc[:n], seg[:n], dict(edges=st[0], tail=st[1])


@pytest.fixture(scope="module")
def rg(tmp_path_factory):
    return build_rg(tmp_path_factory.mktemp("rgref"))


def _cloud(rng, kind):
    if kind == "plane":
        n = int(rng.integers(20, 400))
        u, v = rng.normal(size=(2, 3))
        p = rng.uniform(-3, 3, (n, 2))
        x = p[:, :1] * u + p[:, 1:] * v + rng.normal(0, rng.choice([0.0, 0.005, 0.05]), (n, 3))
    elif kind == "blob":
        n = int(rng.integers(20, 400))
        x = rng.normal(size=(n, 3)) * rng.uniform(0.2, 2.0, 3)
        x = x[rng.random(n) < 0.7]
    elif kind == "box":       # two walls and a floor: several planes meeting
        n = int(rng.integers(60, 400))
        x = rng.uniform(0, 4, (n, 3))
        w = rng.integers(0, 3, n)
        x[np.arange(n), w] = 0.0
        x += rng.normal(0, 0.01, (n, 3))
    elif kind == "dups":      # repeated points: zero covariances (NaN normals) and distance ties at zero
        n = int(rng.integers(20, 200))
        x = rng.uniform(-1, 1, (n, 3))
        x = np.repeat(x, rng.integers(1, 14, n), axis=0)
        rng.shuffle(x)
    elif kind == "small":     # n < k
        x = rng.uniform(-1, 1, (int(rng.integers(1, 10)), 3))
    else:                     # lattice: exact distance ties everywhere
        g = np.stack(np.meshgrid(*[np.arange(int(rng.integers(2, 8)))] * 3, indexing="ij"), -1).reshape(-1, 3)
        x = g[rng.random(len(g)) < 0.8].astype(np.float64) * rng.choice([0.25, 0.5, 1.0])
        if rng.random() < 0.5:
            x[:, 2] = 0.0
    return (x + rng.uniform(-50, 50, 3)).astype(np.float32)


def test_literal_and_min_key_forms_agree(rg):
    rng = np.random.default_rng(7)
    kinds = ["plane", "blob", "box", "dups", "small", "lattice"]
    seen = dict(building=0, tree=0, tail=0, nan_normals=0)
    for it in range(240):
        kind = kinds[it % len(kinds)]
        x = _cloud(rng, kind)
        curv = 0.02 if it % 5 == 0 else 1.2
        k = 10 if it % 7 else int(rng.integers(1, 17))
        a = run(rg, x, "literal", k=k, curv=curv)
        b = run(rg, x, "min-key", k=k, curv=curv)
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (it, kind)
        assert np.array_equal(a[2], b[2]), (it, kind, int((a[2] != b[2]).sum()))
        assert a[0] == b[0], (it, kind)
        seen["building" if a[0] == 3 else "tree"] += 1
        seen["tail"] += b[3]["tail"] > 0
        seen["nan_normals"] += bool(np.isnan(a[1][:, 0]).any())
    assert min(seen.values()) > 5, seen


def test_known_answers(rg):
    rng = np.random.default_rng(3)
    wall = np.stack([rng.uniform(0, 8, 600), np.zeros(600), rng.uniform(0, 3, 600)], -1).astype(np.float32)
    cls, nc, seg, _ = run(rg, wall)
    assert cls == 3 and np.all(np.abs(np.abs(nc[:, 1]) - 1) < 1e-3)
    bush = rng.normal(0, 1.0, (400, 3)).astype(np.float32)
    assert run(rg, bush)[0] == 1
    assert run(rg, wall[:19])[0] == 1              # fewer than min segment points: tree
    dup = np.repeat(np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [3, 1, 0], [1, 1, 1]], np.float32), 12, axis=0)
    cls, nc, seg, _ = run(rg, dup)
    assert np.isnan(nc[:, :3]).all() and (nc[:, 3] == 0).all()   # zero covariance: NaN normal, curvature 0
    assert np.isnan(run(rg, wall[:2])[1]).all()                  # fewer than 3 neighbours: NaN normal and curvature


def test_cos_of_the_smoothness_threshold(rg):
    got = rg.host_cosf(C.c_float(np.float32(10.0 / 180.0 * np.pi)))
    assert struct.unpack("<I", struct.pack("<f", got))[0] == COS10


def test_eigen33_smallest_pair(rg):
    rng = np.random.default_rng(11)
    ev = C.c_float()
    v = np.zeros(3, np.float32)
    for it in range(2000):
        B = rng.normal(size=(3, 3)) * rng.uniform(1e-3, 1e2)
        A = (B @ B.T).astype(np.float32)
        rg.spec_eigen33(A.ctypes.data_as(C.c_void_p), C.byref(ev), v.ctypes.data_as(C.c_void_p))
        assert abs(np.linalg.norm(v.astype(np.float64)) - 1) < 1e-5
        lam = np.linalg.eigvalsh(A.astype(np.float64))[0]
        scale = np.abs(A).max()
        assert abs(ev.value - lam) <= 2e-5 * scale
        assert np.linalg.norm(A.astype(np.float64) @ v - ev.value * v) <= 5e-3 * scale
    for it in range(500):     # rank deficient: c0 below epsilon, computeRoots2 gives the root 0 exactly
        u = rng.normal(size=3)
        w = rng.normal(size=3) if it % 2 else np.zeros(3)
        A = (np.outer(u, u) + np.outer(w, w)).astype(np.float32)
        rg.spec_eigen33(A.ctypes.data_as(C.c_void_p), C.byref(ev), v.ctypes.data_as(C.c_void_p))
        assert ev.value == 0.0
        if it % 2:            # (rank 1: the rows are parallel and the cross products carry no direction, in PCL too)
            assert abs(np.linalg.norm(v.astype(np.float64)) - 1) < 1e-5
            assert np.linalg.norm(A.astype(np.float64) @ v) <= 1e-3 * np.abs(A).max()


# sin_f32 / cos_f32 against glibc over [0, pi/3] (the range of theta in computeRoots), every 64th float: the counts DESIGN.md states
TRIG_STEP, TRIG_SIN_DIFF, TRIG_COS_DIFF = 64, 12526, 1806


def test_trig_against_glibc(rg):
    hi = struct.unpack("<I", struct.pack("<f", np.float32(np.pi / 3)))[0]
    out = (C.c_long * 3)()
    rg.spec_trig_mismatch(C.c_uint(0), C.c_uint(hi), C.c_uint(TRIG_STEP), out)
    assert out[2] == hi // TRIG_STEP + 1
    assert (out[0], out[1]) == (TRIG_SIN_DIFF, TRIG_COS_DIFF), tuple(out)

