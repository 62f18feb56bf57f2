"""Reference statement of scvod_batch_object_shapes (include/scvod.h) -- test infrastructure only.

`shape` is the C++ loop of object_shape_ref.cpp over one object's points: the library's arithmetic (scvod_math.h), one point after the
other.  The numpy functions beside it are INDEPENDENT of that header: fp64 evaluations of the same sums, numpy's symmetric
eigenvalue solver, and the rational features written out again -- what the helper itself is checked against."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OBJECT_SHAPE_DTYPE = np.dtype([("cov", "f4", 6), ("eig", "f4", 3), ("flags", "i4"), ("feat", "f8", 7)])
DEFAULT_K = (0.333, 740.0, 959.0, 1248.0, 0.278636, 1248.0, 0.956129, 0.99702)   # utility.h:318-325


def build(out_dir):
    src = os.path.join(ROOT, "tests", "helpers", "object_shape_ref.cpp")
    so = os.path.join(str(out_dir), "libobjshaperef.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.shape_ref.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.shape_ref.restype = None
    for who in ("spec", "libm"):
        for fn in ("log", "exp"):
            f = getattr(lib, f"{who}_{fn}_many")
            f.argtypes, f.restype = [C.c_void_p, C.c_long, C.c_void_p], None
        f = getattr(lib, f"{who}_pow_many")
        f.argtypes, f.restype = [C.c_void_p, C.c_double, C.c_long, C.c_void_p], None
    return lib


def shape(lib, xyz, K=DEFAULT_K):
    """the record of one object from its points [n, 3] in member order"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    k = np.asarray(K, np.float64)
    out = np.zeros(1, OBJECT_SHAPE_DTYPE)
    lib.shape_ref(xyz.ctypes.data_as(C.c_void_p), len(xyz), k.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out[0]


def many(lib, name, x, k=None):
    """spec_* / libm_* over an array of doubles"""
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(x)
    f = getattr(lib, name)
    if k is None:
        f(x.ctypes.data_as(C.c_void_p), len(x), out.ctypes.data_as(C.c_void_p))
    else:
        f(x.ctypes.data_as(C.c_void_p), float(k), len(x), out.ctypes.data_as(C.c_void_p))
    return out


def ulp_distance(a, b):
    """distance in units of the last place between finite doubles of one sign"""
    ia = np.ascontiguousarray(a, np.float64).view(np.int64)
    ib = np.ascontiguousarray(b, np.float64).view(np.int64)
    return np.abs(ia - ib)


def bits(a):
    """the raw words of a record array with every NaN as ONE pattern"""
    a = np.ascontiguousarray(a).copy()
    for name in ("cov", "eig", "feat"):
        v = a[name]
        v[np.isnan(v)] = np.nan
    return a.view(np.uint8)


def cov64(xyz):
    """(cov6 in fp64 from the fp32 centroid the specification uses, per entry sum |a_k b_k|)"""
    x = np.ascontiguousarray(xyz, np.float32)
    c = (np.add.accumulate(x, axis=0, dtype=np.float32)[-1] / np.float32(len(x))).astype(np.float32)
    p = (x - c).astype(np.float32).astype(np.float64)        # p = xyz - centroid is an fp32 operation of the specification
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    cov = np.asarray([np.sum(p[:, i] * p[:, j]) for i, j in pairs])
    mag = np.asarray([np.sum(np.abs(p[:, i] * p[:, j])) for i, j in pairs])
    return cov, mag


def sym(cov6):
    xx, xy, xz, yy, yz, zz = [float(v) for v in cov6]
    return np.asarray([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], np.float64)


def rational_features(eig, K=DEFAULT_K):
    """linearity, planarity, scattering, anisotropy, change_of_curvature in numpy fp64 from float eigenvalues (ascending)"""
    ev = np.asarray(eig, np.float32)
    s = np.float64(np.float32(np.float32(ev[0] + ev[1]) + ev[2]))
    with np.errstate(all="ignore"):
        e1, e2, e3 = np.float64(ev[0]) / s, np.float64(ev[1]) / s, np.float64(ev[2]) / s
        return np.asarray([np.abs((e1 - e2) / e1 / K[1]), np.abs((e2 - e3) / e1 / K[2]), np.abs(e3 / e1 / K[3]),
                           np.abs((e1 - e3) / e1 / K[5]), np.abs(e3 / (e1 + e2 + e3) / K[7])], np.float64)
