"""Reference statements of the pose refinement (include/scvod.h: scvod_map_register, scvod_register_device) -- test infrastructure only.

`run` is the C++ loop of register_ref.cpp: the library's reg_* functions (scvod_math.h) over scans, iterations and points, with an
exhaustive search for the correspondence.  `run_numpy` beside it is INDEPENDENT of that header: the definition of include/scvod.h
written out again -- numpy's fp32 array operations for the move and the distances (one rounding per operation, as the kernels
have), an exhaustive nearest neighbour by argmin (first occurrence = lowest index; the map's targets sorted by key first), the terms
in fp64 arrays scaled by 2^20 and rounded with numpy.rint (ties to even), summed as Python ints, and an LDL^T, quaternion and pose
update in Python floats (IEEE doubles, one rounding per operation, math.sqrt correctly rounded).  Every operation is an IEEE-basic
one in a stated order, so the two agree bit for bit, not within a tolerance.  `corner_cloud` is the crafted cloud of the tests."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F = np.float32
RECORD_DTYPE = np.dtype([("status", "i4"), ("iterations", "i4"), ("n_corr", "i8"), ("sum_r2", "f8"), ("last_omega", "f8"), ("last_v", "f8"),
                         ("skip_nan", "i4"), ("skip_range", "i4"), ("skip_label", "i4"), ("skip_no_corr", "i4"), ("skip_normal", "i4"),
                         ("reserved", "i4")])
assert RECORD_DTYPE.itemsize == 64
MAX_ITERATIONS, CONVERGED, DEGENERATE = 0, 1, 2
POINT, PLANE = 0, 1
WORDS = 34  # 21 + 6 + 1 + correspondences + 5 skip counters
DEFAULTS = dict(max_iterations=10, min_corr=30, mode=POINT, max_dist=0.19, max_range=80.0, eps_rot=1e-6, eps_trans=1e-5, lam=0.0,
                pivot_eps=1e-9, use256=None)


def params(**kw):
    p = dict(DEFAULTS)
    assert all(k in p for k in kw), kw
    p.update(kw)
    return p


def build(out_dir):
    src = os.path.join(ROOT, "tests", "helpers", "register_ref.cpp")
    so = os.path.join(str(out_dir), "libregisterref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.register_ref.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                 C.c_double, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp]
    lib.register_ref.restype = None
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _inputs(src, offs, pose32, labels, tgt_xyz, tgt_key, tgt_nrm, p):
    src = np.ascontiguousarray(np.asarray(src, F).reshape(-1, 4))
    offs = np.ascontiguousarray(offs, np.int32)
    pose32 = np.ascontiguousarray(np.asarray(pose32, F).reshape(-1, 12))
    assert len(pose32) == len(offs) - 1
    labels = None if labels is None else np.ascontiguousarray(labels, np.uint8)
    use = None if p["use256"] is None else np.ascontiguousarray(np.asarray(p["use256"]) != 0, np.uint8)
    tgt_xyz = np.ascontiguousarray(np.asarray(tgt_xyz, F).reshape(-1, 3))
    tgt_key = None if tgt_key is None else np.ascontiguousarray(tgt_key, np.uint64)
    tgt_nrm = None if tgt_nrm is None else np.ascontiguousarray(np.asarray(tgt_nrm, F).reshape(-1, 3))
    return src, offs, pose32, labels, use, tgt_xyz, tgt_key, tgt_nrm


def run(lib, src, offs, pose32, tgt_xyz, p, labels=None, tgt_key=None, tgt_nrm=None):
    """dict(pose [n_scans, 12] float64, records [n_scans] RECORD_DTYPE, sums [n_scans, 34] int64, match0 [n] int32) of the C++ loop"""
    src, offs, pose32, labels, use, tgt_xyz, tgt_key, tgt_nrm = _inputs(src, offs, pose32, labels, tgt_xyz, tgt_key, tgt_nrm, p)
    n_scans = len(offs) - 1
    pose = np.zeros((max(n_scans, 1), 12), np.float64)
    rec = np.zeros(max(n_scans, 1), RECORD_DTYPE)
    sums = np.zeros((max(n_scans, 1), WORDS), np.int64)
    match0 = np.full(max(len(src), 1), -1, np.int32)
    lib.register_ref(_ptr(src), _ptr(offs), n_scans, _ptr(pose32), _ptr(labels), _ptr(use), _ptr(tgt_xyz), _ptr(tgt_key), _ptr(tgt_nrm),
                     len(tgt_xyz), int(p["max_iterations"]), int(p["min_corr"]), int(p["mode"]), float(p["max_dist"]), float(p["max_range"]),
                     float(p["eps_rot"]), float(p["eps_trans"]), float(p["lam"]), float(p["pivot_eps"]), _ptr(pose), _ptr(rec), _ptr(sums),
                     _ptr(match0))
    return dict(pose=pose[:n_scans], records=rec[:n_scans], sums=sums[:n_scans], match0=match0[:len(src)])


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------
def _fix(a):
    """fp64 array * 2^20, rounded to nearest (ties to even), summed as a Python int"""
    return sum(np.rint(a * 1048576.0).astype(np.int64).tolist())


def _row_terms(J, r, w):
    k = 0
    for i in range(6):
        for j in range(i, 6):
            w[k] += _fix(J[i] * J[j])
            k += 1
    for i in range(6):
        w[21 + i] += _fix(J[i] * r)
    w[27] += _fix(r * r)


def _solve_update(w, T, p):
    """(status, |omega|, |v|); T (a list of 12 Python floats) is updated in place unless DEGENERATE"""
    if w[28] < p["min_corr"]:
        return DEGENERATE, 0.0, 0.0
    inv = 1.0 / 1048576.0
    H = [[0.0] * 6 for _ in range(6)]
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i][j] = H[j][i] = float(w[k]) * inv
            k += 1
    x = [-(float(w[21 + i]) * inv) for i in range(6)]
    top = 0.0
    for i in range(6):
        H[i][i] = H[i][i] + p["lam"] * H[i][i]
        if H[i][i] > top:
            top = H[i][i]
    floor_pivot = p["pivot_eps"] * top
    for j in range(6):
        d = H[j][j]
        for m in range(j):
            d = d - (H[j][m] * H[j][m]) * H[m][m]
        if not d > floor_pivot:
            return DEGENERATE, 0.0, 0.0
        H[j][j] = d
        for i in range(j + 1, 6):
            a = H[i][j]
            for m in range(j):
                a = a - (H[i][m] * H[j][m]) * H[m][m]
            H[i][j] = a / d
    for i in range(6):
        for m in range(i):
            x[i] = x[i] - H[i][m] * x[m]
    for i in range(6):
        x[i] = x[i] / H[i][i]
    for i in range(5, -1, -1):
        for m in range(i + 1, 6):
            x[i] = x[i] - H[m][i] * x[m]
    on = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    vn = math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5])
    if not (math.isfinite(on) and math.isfinite(vn)):
        return DEGENERATE, 0.0, 0.0
    hx, hy, hz = 0.5 * x[0], 0.5 * x[1], 0.5 * x[2]
    qn = math.sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz))
    qw, qx, qy, qz = 1.0 / qn, hx / qn, hy / qn, hz / qn
    D = [1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw),
         2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw),
         2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)]
    for i in range(3):
        a, b, c = T[4 * i], T[4 * i + 1], T[4 * i + 2]
        T[4 * i + 3] = ((a * x[3] + b * x[4]) + c * x[5]) + T[4 * i + 3]
        T[4 * i] = (a * D[0] + b * D[3]) + c * D[6]
        T[4 * i + 1] = (a * D[1] + b * D[4]) + c * D[7]
        T[4 * i + 2] = (a * D[2] + b * D[5]) + c * D[8]
    return (CONVERGED if on < p["eps_rot"] and vn < p["eps_trans"] else MAX_ITERATIONS), on, vn


def run_numpy(src, offs, pose32, tgt_xyz, p, labels=None, tgt_key=None, tgt_nrm=None):
    """the same dict as `run`, from the definition alone"""
    src, offs, pose32, labels, use, tgt_xyz, tgt_key, tgt_nrm = _inputs(src, offs, pose32, labels, tgt_xyz, tgt_key, tgt_nrm, p)
    n_scans = len(offs) - 1
    order = np.arange(len(tgt_xyz)) if tgt_key is None else np.argsort(tgt_key, kind="stable")  # argmin's first hit = the tie rule
    tgt = tgt_xyz[order]
    r2 = F(p["max_dist"]) * F(p["max_dist"])
    with np.errstate(all="ignore"):
        range2 = F(p["max_range"]) * F(p["max_range"])
    pose = np.zeros((n_scans, 12), np.float64)
    rec = np.zeros(n_scans, RECORD_DTYPE)
    sums = np.zeros((n_scans, WORDS), np.int64)
    match0 = np.full(len(src), -1, np.int32)
    for s in range(n_scans):
        T = [float(v) for v in pose32[s]]
        a, b = int(offs[s]), int(offs[s + 1])
        P = src[a:b, :3]
        status, w = MAX_ITERATIONS, [0] * WORDS
        for it in range(int(p["max_iterations"])):
            if status != MAX_ITERATIONS:
                break
            w = [0] * WORDS
            Tf = np.asarray(T, np.float64).astype(F)
            x, y, z = P[:, 0], P[:, 1], P[:, 2]
            with np.errstate(all="ignore"):
                nan = np.isnan(x) | np.isnan(y) | np.isnan(z)
                far = ~nan & (((x * x + y * y) + z * z) > range2)
                ok = ~nan & ~far
                gated = np.zeros(len(P), bool) if labels is None or use is None else ok & (use[labels[a:b]] == 0)
                ok &= ~gated
                W = np.stack([((Tf[4 * k] * x + Tf[4 * k + 1] * y) + Tf[4 * k + 2] * z) + Tf[4 * k + 3] for k in range(3)], 1)
                best = np.full(len(P), -1, np.int64)
                if len(tgt) and ok.any():
                    dx, dy, dz = (W[ok, None, k] - tgt[None, :, k] for k in range(3))
                    d = (dx * dx + dy * dy) + dz * dz
                    d = np.where(d < r2, d, F(np.inf))
                    m = np.argmin(d, axis=1)
                    hit = d[np.arange(len(m)), m] < r2
                    best[np.flatnonzero(ok)[hit]] = order[m[hit]]
            has = best >= 0
            if it == 0:
                match0[a:b] = best
            w[29], w[30], w[31], w[32] = int(nan.sum()), int(far.sum()), int(gated.sum()), int((ok & ~has).sum())
            idx = np.flatnonzero(has)
            Pd, Q = P[idx].astype(np.float64), tgt_xyz[best[idx]].astype(np.float64)
            d0, d1, d2 = Q[:, 0] - T[3], Q[:, 1] - T[7], Q[:, 2] - T[11]
            r = [Pd[:, j] - ((T[j] * d0 + T[4 + j] * d1) + T[8 + j] * d2) for j in range(3)]
            px, py, pz = Pd[:, 0], Pd[:, 1], Pd[:, 2]
            one, zero = np.ones(len(idx)), np.zeros(len(idx))
            if p["mode"] == POINT:
                _row_terms([zero, pz, -py, one, zero, zero], r[0], w)
                _row_terms([-pz, zero, px, zero, one, zero], r[1], w)
                _row_terms([py, -px, zero, zero, zero, one], r[2], w)
                w[28] = len(idx)
            else:
                N = tgt_nrm[best[idx]].astype(np.float64)
                with np.errstate(all="ignore"):
                    nn = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
                    good = (nn >= 1e-6 * 1e-6) & np.isfinite(nn)
                w[33] = int((~good).sum())
                N, nn, px, py, pz, r = N[good], nn[good], px[good], py[good], pz[good], [c[good] for c in r]
                ln = np.sqrt(nn)
                u = [N[:, k] / ln for k in range(3)]
                nl = [(T[j] * u[0] + T[4 + j] * u[1]) + T[8 + j] * u[2] for j in range(3)]
                e = (nl[0] * r[0] + nl[1] * r[1]) + nl[2] * r[2]
                _row_terms([py * nl[2] - pz * nl[1], pz * nl[0] - px * nl[2], px * nl[1] - py * nl[0], nl[0], nl[1], nl[2]], e, w)
                w[28] = int(good.sum())
            status, on, vn = _solve_update(w, T, p)
            rec[s] = (status, it + 1, w[28], float(w[27]) / 1048576.0, on, vn, w[29], w[30], w[31], w[32], w[33], 0)
        pose[s] = T
        sums[s] = w
    return dict(pose=pose, records=rec, sums=sums, match0=match0)


# ---- the crafted cloud ------------------------------------------------------------------------------------------------------------
def rotvec_matrix(rv):
    """Rodrigues' formula in fp64"""
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def pose_matrix64(t, rv):
    M = np.zeros((3, 4))
    M[:, :3] = rotvec_matrix(rv)
    M[:, 3] = t
    return M


TRUE_T, TRUE_RV = (120.0, -45.0, 3.0), (0.3, -0.2, 1.1)


def corner_cloud(n=22, step=0.25, corner=(2.0, 3.0, -1.5)):
    """the three faces of a corner, n x n points each `step` apart (off the shared edges by half a step): (xyzi [3 n n, 4] float32 in the
    sensor frame, its image [.., 3] float32 under the true pose, the faces' world normals [.., 3] float32)"""
    g = (np.arange(n) + 0.5) * step
    u, v = (c.reshape(-1) for c in np.meshgrid(g, g, indexing="ij"))
    z = np.zeros_like(u)
    faces = [np.stack([u, v, z], 1), np.stack([u, z, v], 1), np.stack([z, u, v], 1)]
    nrm = [np.tile([0.0, 0.0, 1.0], (n * n, 1)), np.tile([0.0, 1.0, 0.0], (n * n, 1)), np.tile([1.0, 0.0, 0.0], (n * n, 1))]
    p = (np.concatenate(faces) + np.asarray(corner)).astype(F)
    M = pose_matrix64(TRUE_T, TRUE_RV)
    world = (p.astype(np.float64) @ M[:, :3].T + M[:, 3]).astype(F)
    normals = (np.concatenate(nrm) @ M[:, :3].T).astype(F)
    xyzi = np.concatenate([p, np.ones((len(p), 1), F)], 1)
    return xyzi, world, normals


def start_matrix(d_rot=0.003, d_trans=0.04, axis=(0.5, -0.6, 0.62), tdir=(0.6, 0.64, -0.48)):
    """the true pose off by d_rot rad about `axis` and d_trans m along `tdir`, as an fp32 row-major 3x4 (what the device starts from)"""
    M = pose_matrix64(TRUE_T, TRUE_RV)
    ax = np.asarray(axis, np.float64)
    E = rotvec_matrix(ax / np.linalg.norm(ax) * d_rot)
    td = np.asarray(tdir, np.float64)
    S = np.zeros((3, 4))
    S[:, :3] = M[:, :3] @ E
    S[:, 3] = M[:, 3] + td / np.linalg.norm(td) * d_trans
    return S.astype(F).reshape(12)


def pose_error(T12, cloud_xyz):
    """the largest distance (metres, fp64) between the images of the cloud's points under T12 and under the true pose"""
    M = pose_matrix64(TRUE_T, TRUE_RV)
    T = np.asarray(T12, np.float64).reshape(3, 4)
    p = np.asarray(cloud_xyz, np.float64)[:, :3]
    return float(np.linalg.norm((p @ T[:, :3].T + T[:, 3]) - (p @ M[:, :3].T + M[:, 3]), axis=1).max())
