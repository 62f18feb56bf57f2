"""Reference statement of the ESF descriptor (include/scvod.h: scvod_esf_device) -- test infrastructure only.

`esf` is the C++ loop of object_esf_ref.cpp over one object's points and samples: the library's esf_* functions (scvod_math.h), one
sample after the other.  `esf_numpy` beside it is INDEPENDENT of that header: the definition of include/scvod.h written out again in
numpy's fp32 / integer array operations -- the same IEEE operations, so the two agree exactly, not within a tolerance: the line is
walked by the division formula (the header carries quotient and remainder), the angle bin is the literal count over numpy's own
cosines (the header bisects a table of literals), the stamps are set voxel by voxel.  `esf_cases` are the crafted objects."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OBJECT_ESF_DTYPE = np.dtype([("fold10", "f4", 10), ("n_valid", "i4"), ("n_points", "i4"), ("flags", "i4"), ("lines", "u4", 3)])
SIG = 640
F = np.float32
IN, OUT, MIX = 0, 1, 2
W = np.asarray([0.5, 0.5, 0.5, 0.5, 0.5, 1, 1, 2, 2, 2], F)


def build(out_dir):
    src = os.path.join(ROOT, "tests", "helpers", "object_esf_ref.cpp")
    so = os.path.join(str(out_dir), "libobjesfref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.esf_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.esf_ref.restype = None
    lib.esf_cos_table.argtypes, lib.esf_cos_table.restype = [C.c_void_p], None
    return lib


def esf(lib, xyz, samples=20000, seed=0, min_points=3):
    """dict(record, hist [640] int32, sig [640] float32, triangles [3] OUT / IN / MIX) of one object from its points [n, 3] in member
    order"""
    xyz = np.ascontiguousarray(np.asarray(xyz, F).reshape(-1, 3)[:, :3])
    rec, hist, sig, tri = np.zeros(1, OBJECT_ESF_DTYPE), np.zeros(SIG, np.int32), np.zeros(SIG, F), np.zeros(3, np.int32)
    lib.esf_ref(xyz.ctypes.data_as(C.c_void_p), len(xyz), int(samples), int(seed) & 0xFFFFFFFF, int(min_points),
                rec.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(C.c_void_p), sig.ctypes.data_as(C.c_void_p),
                tri.ctypes.data_as(C.c_void_p))
    return dict(record=rec[0], hist=hist, sig=sig, triangles=tri)


def cos_table(lib):
    out = np.zeros(64, F)
    lib.esf_cos_table(out.ctypes.data_as(C.c_void_p))
    return out


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------
def cos_thresholds():
    """T[b], b = 1 .. 63 (index 0 unused)"""
    b = np.arange(64, dtype=np.float64)
    return np.cos((b - 0.5) * np.pi / 126.0).astype(F)


def _mix(h):
    h = h.astype(np.uint32)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x7feb352d)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x846ca68b)
    h ^= h >> np.uint32(16)
    return h


def draw(seed, k, j, n):
    with np.errstate(over="ignore"):
        h = _mix(np.uint32(seed) + np.uint32(0x9E3779B9) * (np.uint32(3) * k.astype(np.uint32) + np.uint32(j + 1)))
    return ((h.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def _voxel(v):
    f = np.where(v < 0, np.floor(v) + F(32), np.ceil(v) + F(31))
    return np.clip(f, 0, 63).astype(np.int64)


def _dist(p, q):
    d = (p - q).astype(F)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(F))


def _dot(p, q):
    return (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1] + p[:, 2] * q[:, 2]).astype(F)


def _bin63(v):
    return np.floor(v.astype(F) * F(63) + F(0.5)).astype(np.int64)


def _line(grid, A, B):
    """per sample: (count, in) of the line between the voxels A and B [s, 3]"""
    d = B - A
    ad, sg = np.abs(d), np.where(d < 0, -1, 1)
    m = ad.max(axis=1)
    n_in = np.zeros(len(A), np.int64)
    for t in range(64):
        live = t <= m
        den = np.where(m > 0, 2 * m, 1)[:, None]
        pos = A + sg * ((2 * ad * t + m[:, None]) // den)
        pos = np.where(live[:, None], pos, 0)
        n_in += live & grid[pos[:, 2], pos[:, 1], pos[:, 0]]
    return m + 1, n_in


def esf_numpy(xyz, samples=20000, seed=0, min_points=3):
    """the same dict as esf(), from numpy alone"""
    x = np.asarray(xyz, F).reshape(-1, 3)
    n = len(x)
    rec = np.zeros(1, OBJECT_ESF_DTYPE)[0]
    rec["n_points"] = n
    out = dict(record=rec, hist=np.zeros(SIG, np.int32), sig=np.zeros(SIG, F), triangles=np.zeros(3, np.int32))
    if n < min_points:
        rec["flags"] = 2
        return out
    with np.errstate(all="ignore"):
        c = (np.add.accumulate(x, axis=0, dtype=F)[-1] / F(n)).astype(F)
        q = (x - c).astype(F)
        d2 = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]).astype(F)
        d2 = d2[~np.isnan(d2)]
        r = np.sqrt(F(d2.max() if len(d2) else 0))
    if r == 0 or not np.isfinite(r):
        rec["flags"] = 4
        return out
    u = (q * (F(32) / r)).astype(F)
    vox = _voxel(u)
    grid = np.zeros((64, 64, 64), bool)  # [z][y][x]
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                p = vox + np.asarray([dx, dy, dz])
                ok = ((p >= 0) & (p < 64)).all(axis=1)
                grid[p[ok, 2], p[ok, 1], p[ok, 0]] = True
    k = np.arange(samples, dtype=np.uint32)
    i0, i1, i2 = (draw(seed, k, j, n) for j in range(3))
    ok = (i0 != i1) & (i0 != i2) & (i1 != i2)
    p1, p2, p3 = u[i0], u[i1], u[i2]
    a, b, cc = _dist(p1, p2), _dist(p1, p3), _dist(p2, p3)
    s = ((a + b).astype(F) + cc).astype(F) * F(0.5)
    heron = (((s * (s - a)).astype(F) * (s - b)).astype(F) * (s - cc)).astype(F)
    ok &= heron > F(0.001)
    sel = np.nonzero(ok)[0]
    rec["n_valid"] = len(sel)
    if len(sel) == 0:
        rec["flags"] = 1
        return out
    p1, p2, p3, a, b, cc, heron = p1[sel], p2[sel], p3[sel], a[sel], b[sel], cc[sel], heron[sel]
    v1, v2, v3 = _voxel(p1), _voxel(p2), _voxel(p3)
    hist = np.zeros((10, 64), np.int64)
    cls, sum_in, sum_cnt = [], 0, 0
    for A, B in ((v1, v2), (v1, v3), (v2, v3)):
        cnt, n_in = _line(grid, A, B)
        lc = np.where(n_in >= cnt - 1, IN, np.where(n_in <= 7, OUT, MIX))
        ratio = (n_in.astype(F) / cnt.astype(F)).astype(F)
        np.add.at(hist[9], _bin63(ratio)[lc == MIX], 1)
        cls.append(lc)
        sum_in, sum_cnt = sum_in + n_in, sum_cnt + cnt
    for t in (IN, OUT, MIX):
        rec["lines"][t] = sum(int((lc == t).sum()) for lc in cls)
    tri = np.where(sum_in <= 21, OUT, np.where(sum_cnt - sum_in < 4, IN, MIX))
    out["triangles"][:] = [(tri == OUT).sum(), (tri == IN).sum(), (tri == MIX).sum()]
    T = cos_thresholds()
    e12, e13, e23 = (p2 - p1).astype(F), (p3 - p1).astype(F), (p3 - p2).astype(F)
    for dot, l1, l2 in ((_dot(e12, e13), a, b), (_dot(e12, e23), a, cc), (_dot(e13, e23), b, cc)):
        xq = np.minimum(F(1), (np.abs(dot) / (l1 * l2).astype(F)).astype(F))
        np.add.at(hist, (tri, (xq[:, None] <= T[None, 1:]).sum(axis=1)), 1)
    d3 = np.sqrt(np.sqrt(heron))
    max_d2, max_d3 = max(a.max(), b.max(), cc.max()), d3.max()
    np.add.at(hist, (3 + tri, _bin63((d3 / max_d3).astype(F))), 1)
    for dd, lc in zip((a, b, cc), cls):
        np.add.at(hist, (6 + lc, _bin63((dd / max_d2).astype(F))), 1)
    out["hist"][:] = hist.reshape(-1)
    cntf = hist.astype(F)
    cntf[:3] = (cntf[:3] / F(3)).astype(F)
    sig = (cntf * W[:, None]).astype(F).reshape(-1)
    total = np.add.accumulate(sig, dtype=F)[-1]
    sig = (sig / total).astype(F)
    out["sig"][:] = sig
    for j in range(10):
        rec["fold10"][j] = F(np.add.accumulate(sig[j::10].astype(np.float64))[-1])
    return out


# ---- crafted objects ------------------------------------------------------------------------------------------------------------
def esf_cases(seed=11):
    """name -> float32 [n, 3]"""
    g = np.random.default_rng(seed)
    at = np.asarray([12.5, -7.25, 0.75], F)   # the objects of a scan do not sit at the origin

    def box(n, ext):
        return (g.random((n, 3)) - 0.5).astype(F) * np.asarray(ext, F) + at

    clumps = np.concatenate([np.asarray(c, F) + (g.random((20, 3)).astype(F) - F(0.5)) * F(0.02)
                             for c in ((1, 0, 0), (-1, 0, 0), (0, 1, 0))]) + at
    return {
        "block": box(4500, (0.6, 0.6, 1.0)),
        "plate": box(300, (1.0, 0.0, 0.8)),
        "clumps": clumps.astype(F),
        "block30": box(30, (0.5, 0.4, 0.3)),
        "xaxis": np.stack([np.arange(9), np.zeros(9), np.zeros(9)], axis=1).astype(F),
        "three": np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F),
        "equal": np.tile(np.asarray([[3.5, -1.25, 0.5]], F), (4, 1)),
        "two": np.asarray([[0, 0, 0], [1, 2, 3]], F),
    }


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)
