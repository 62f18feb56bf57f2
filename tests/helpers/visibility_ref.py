"""Reference statement of the seen-through vote (include/scvod.h: scvod_visibility_device) -- test infrastructure only.

`run` is the brute-force C++ loop of visibility_ref.cpp: the library's arithmetic (scvod_math.h) for every point, plain loops over
(scan, viewer, point, window).  `viewers_of` restates the viewer lists in Python; `classify64` is INDEPENDENT of that header: the same
rule in numpy float64 (numpy.arctan2, numpy.hypot), with the distance of every decision from its threshold, so that a test can leave
out the pairs that sit on one."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
THROUGH, AGREE, OCCLUDED, OUTSIDE, EMPTY = 0, 1, 2, 3, 4
GRID_FIELDS = ("min_dis", "max_dis", "min_angle", "max_angle", "min_azimuth", "max_azimuth", "range_res", "sector_res", "azimuth_res")


def build(out_dir):
    src = os.path.join(ROOT, "tests", "helpers", "visibility_ref.cpp")
    so = os.path.join(str(out_dir), "libvisibilityref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.vis_ref.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 12
    lib.vis_ref.restype = None
    return lib


def grid_of(scvod, P):
    """(g9 float32, dims3 int32 = range / sector / azimuth bins) of a scvod_py.Params"""
    R, S, A, _ = scvod.grid_dims(P)
    return np.asarray([getattr(P, f) for f in GRID_FIELDS], np.float32), np.asarray([R, S, A], np.int32)


def viewers_of(n_scans, next_scan=None, before=2, after=2):
    """(begin [n_scans + 1], viewers): per scan up to `after` successors along next_scan, nearest first, then up to `before`
    predecessors along its inverse.  ValueError for a table the library refuses."""
    nxt = [(s + 1 if s + 1 < n_scans else -1) for s in range(n_scans)] if next_scan is None else [int(v) for v in next_scan]
    prev = {}
    for s, v in enumerate(nxt):
        if v >= n_scans or v == s:
            raise ValueError("successor outside the batch")
        if v >= 0:
            if v in prev:
                raise ValueError("two scans name one successor")
            prev[v] = s
    begin, out = [0], []
    for j in range(n_scans):
        seen = {j}
        k = j
        for _ in range(after):
            k = nxt[k]
            if k < 0:
                break
            if k in seen:
                raise ValueError("ring")
            seen.add(k)
            out.append(k)
        k = j
        for _ in range(before):
            k = prev.get(k, -1)
            if k < 0:
                break
            if k in seen:
                raise ValueError("ring")
            seen.add(k)
            out.append(k)
        begin.append(len(out))
    return np.asarray(begin, np.int32), np.asarray(out, np.int32)


def matrices(scvod, poses, begin, viewers):
    """[pairs, 12]: scvod_pose_delta(pose_j, pose_viewer) -- host only -- for every pair"""
    lib = scvod.load_lib()
    n_scans = len(begin) - 1
    p = np.zeros((n_scans, 6), np.float32) if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
    T = np.zeros((len(viewers), 12), np.float32)
    for j in range(n_scans):
        for k in range(begin[j], begin[j + 1]):
            a, b = np.ascontiguousarray(p[j]), np.ascontiguousarray(p[viewers[k]])
            lib.scvod_pose_delta(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), T[k].ctypes.data_as(C.c_void_p))
    return T


def params_tuple(prm):
    return (np.asarray([prm.halo, prm.min_through, prm.vote_num, prm.vote_den], np.int32), np.asarray([prm.gap_abs, prm.gap_rel], np.float32))


def run(lib, scvod, P, xyzi, offsets, poses, prm, next_scan=None, mask=None, pair_classes=False):
    """the vote of `xyzi` [n, 4] (offsets start at 0): dict(images [n_scans, A, S], votes uint32 [n], verdict uint8 [n],
    scan_counts int64 [n_scans, 6], begin, viewers, T, and with pair_classes: pair_class (list per pair of uint8 [n_j]))"""
    x = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    off = np.ascontiguousarray(offsets, np.int32)
    assert off[0] == 0 and off[-1] == len(x)
    n_scans = len(off) - 1
    g9, dims3 = grid_of(scvod, P)
    S, A = int(dims3[1]), int(dims3[2])
    begin, viewers = viewers_of(n_scans, next_scan, prm.before, prm.after)
    T = matrices(scvod, poses, begin, viewers)
    ip, fp = params_tuple(prm)
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    images = np.zeros((n_scans, A, S), np.float32)
    votes = np.zeros(len(x), np.uint32)
    verdict = np.zeros(len(x), np.uint8)
    counts = np.zeros((n_scans, 6), np.int64)
    sizes = np.asarray([off[j + 1] - off[j] for j in range(n_scans) for _ in range(begin[j], begin[j + 1])], np.int64)
    pc_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pc = np.zeros(max(int(pc_off[-1]), 1), np.uint8) if pair_classes else None

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)
    lib.vis_ref(ptr(g9), ptr(dims3), ptr(x), ptr(off), n_scans, ptr(begin), ptr(viewers), ptr(T), ptr(m), ptr(ip), ptr(fp), ptr(images),
                ptr(votes), ptr(verdict), ptr(counts), ptr(pc), ptr(pc_off))
    out = dict(images=images, votes=votes, verdict=verdict, scan_counts=counts, begin=begin, viewers=viewers, T=T)
    if pair_classes:
        out["pair_class"] = [pc[pc_off[k]:pc_off[k + 1]] for k in range(len(viewers))]
    return out


# ---- the same rule in numpy float64 ----
def _bin64(g9, dims3, xyz):
    """float64 binning of points [n, 3]: (dis, si, ai, keep, finite, edge) -- edge: the distance, in bins, of the nearer scaled angle
    from a bin edge; keep_margin folded in as 0 where a range / FOV comparison is closer than 1e-6 relative"""
    g = [float(v) for v in g9]
    x, y, z = (np.asarray(xyz[:, k], np.float64) for k in range(3))
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    x, y, z = np.where(fin, x, 1.0), np.where(fin, y, 1.0), np.where(fin, z, 0.0)
    dis = np.hypot(x, y)
    ang = np.degrees(np.arctan2(y, x))
    ang = np.where(y < 0, ang + 360.0, ang)
    azi = np.degrees(np.arctan2(z, dis))
    keep = (dis >= g[0]) & (dis <= g[1]) & (ang >= g[2]) & (ang <= g[3]) & (azi >= g[4]) & (azi <= g[5])
    us, ua = (ang - g[2]) / g[7], (azi - g[4]) / g[8]
    si, ai = np.ceil(us).astype(np.int64) - 1, np.ceil(ua).astype(np.int64) - 1
    es, ea = np.abs(us - np.round(us)), np.abs(ua - np.round(ua))
    near_limit = np.zeros(len(x), bool)
    for v, lim, tol in ((dis, g[0], 1e-4), (dis, g[1], 1e-4), (ang, g[2], 1e-3), (ang, g[3], 1e-3), (azi, g[4], 1e-3), (azi, g[5], 1e-3)):
        near_limit |= np.abs(v - lim) < tol
    near_limit |= (y == 0.0) | (dis == 0.0)  # the signed-zero cases of atan2f
    edge = np.where(near_limit, 0.0, np.minimum(es, ea))
    # the pixel on the other side of the nearest edge, per axis (si = ceil(us) - 1: just below an integer the next bin is one up)
    _bin64.other = (np.where(np.round(us) >= us, 1, -1), es, np.where(np.round(ua) >= ua, 1, -1), ea)
    return dis, si, ai, keep, fin, edge


def images64(g9, dims3, xyzi, offsets, edge_tol=1e-4):
    """(image, lower image) per scan in float64.  (A scan's own points are binned as they are given: the fp32 angle differs from the
    float64 one by the rounding of atan2f and of the degrees, 3e-5 degrees at 360 -- below 1e-4 bins of any grid used here; the 1e-3
    of classify64 covers the fp32 transform in front of it as well.)  The image holds the points that sit on no bin edge and no range / FOV limit; the lower
    image also takes every point within edge_tol bins of an edge into its own pixel AND the one across that edge (either axis, or
    both): whatever side the fp32 arithmetic puts such a point on, a pixel's value lies between the two"""
    S, A = int(dims3[1]), int(dims3[2])
    off = np.asarray(offsets)
    imgs, lows = [], []
    for s in range(len(off) - 1):
        p = np.asarray(xyzi[off[s]:off[s + 1], :3])
        dis, si, ai, keep, fin, edge = _bin64(g9, dims3, p)
        os_, es, oa, ea = _bin64.other
        inside = (si >= 0) & (si < S) & (ai >= 0) & (ai < A)
        sure = fin & (edge >= edge_tol)
        img = np.full(A * S, np.inf)
        ok = sure & keep & inside
        np.minimum.at(img, (ai * S + si)[ok], dis[ok])
        low = img.copy()
        for i in np.nonzero(fin & ~sure)[0]:
            for da in ((0, oa[i]) if ea[i] < edge_tol else (0,)):
                for ds in ((0, os_[i]) if es[i] < edge_tol else (0,)):
                    a, c = ai[i] + da, si[i] + ds
                    if 0 <= a < A and 0 <= c < S:
                        low[a * S + c] = min(low[a * S + c], dis[i])
        imgs.append(img)
        lows.append(low)
    return imgs, lows


def classify64(g9, dims3, img, low, T, xyz, halo, gap_abs, gap_rel, edge_tol=1e-3, depth_tol=1e-4):
    """classes of the points `xyz` [n, 3] of one scan seen by one viewer (its two float64 images, the float32 matrix T [12]) and the
    mask of the pairs that sit on no threshold: both scaled angles farther than edge_tol bins from a bin edge, every depth comparison
    farther than depth_tol metres from zero, and every pixel of the window on one side of both comparisons whichever of its two
    values is taken (a pixel's part in the rule is monotone in its value)"""
    S, A = int(dims3[1]), int(dims3[2])
    M = np.asarray(T, np.float64).reshape(3, 4)
    q = np.asarray(xyz, np.float64)
    with np.errstate(all="ignore"):
        p = q @ M[:, :3].T + M[:, 3]
    dis, si, ai, keep, fin, edge = _bin64(g9, dims3, p)
    inside = (si >= 0) & (si < S) & (ai >= 0) & (ai < A)
    cls = np.full(len(q), OUTSIDE, np.int64)
    decided = ~fin | (edge >= edge_tol)
    live = fin & keep & inside
    gap = float(gap_abs) + float(gap_rel) * dis

    def part(r):  # 0 in front of the band, 1 inside it, 2 behind it, 3 no return
        with np.errstate(invalid="ignore"):
            d = r - dis
            return np.where(np.isinf(r), 3, np.where(d > gap, 2, np.where(d < -gap, 0, 1)))
    r_min = np.full(len(q), np.inf)
    agree = np.zeros(len(q), bool)
    # what is certain about the window when every pixel may hold any value from low - depth_tol to img + depth_tol
    not_through = np.zeros(len(q), bool)
    all_behind = np.ones(len(q), bool)
    sure_agree = np.zeros(len(q), bool)
    may_agree = np.zeros(len(q), bool)
    some_return = np.zeros(len(q), bool)
    no_return = np.ones(len(q), bool)
    for da in range(-halo, halo + 1):
        for ds in range(-halo, halo + 1):
            a, c = ai + da, si + ds
            okw = live & (a >= 0) & (a < A) & (c >= 0) & (c < S)
            at = np.where(okw, a * S + c, 0)
            r = np.where(okw, img[at], np.inf)
            hi, lo = part(r + depth_tol), part(np.where(okw, low[at], np.inf) - depth_tol)
            not_through |= okw & (hi <= 1)
            all_behind &= ~okw | (lo >= 2)
            sure_agree |= okw & (lo == 1) & (hi == 1)
            may_agree |= okw & (lo <= 1) & (hi >= 1)
            some_return |= okw & (hi <= 2)
            no_return &= ~okw | (lo == 3)
            r_min = np.minimum(r_min, r)
            agree |= okw & (part(r) == 1)
    decided &= ~live | (not_through & (sure_agree | ~may_agree)) | (all_behind & (some_return | no_return))
    with np.errstate(invalid="ignore"):
        through = r_min - dis - gap
    cls[live & np.isinf(r_min)] = EMPTY
    cls[live & np.isfinite(r_min) & (through > 0)] = THROUGH
    cls[live & np.isfinite(r_min) & ~(through > 0) & agree] = AGREE
    cls[live & np.isfinite(r_min) & ~(through > 0) & ~agree] = OCCLUDED
    return cls, decided
