"""The scan stacking (src/makeScan.cpp:153-244; include/scvod.h: scvod_batch_stack_scans) stated in numpy, independent of the library:

  groups     the literal loop: g = 0, 1, ... while g * interval + window <= n_in, and with the reference's bound (makeScan.cpp:156,
             `i < size - interval`) while g * interval < n_in - interval as well; n_in < window gives none
  matrices   oracle.pose_delta(pose_k, pose_mid): the oracle's own restatement of trans_mid^-1 * trans_k
  points     float32 array operations ((T0*x + T1*y) + T2*z) + T3 per row -- numpy rounds every operation and fuses none
  copied     the middle scan, every intensity, the payload words, the source indices

Comparisons are on the uint32 images (bits); a NaN coordinate of a TRANSFORMED point counts as "a NaN" (DESIGN.md section 2), everything
else bit for bit."""
import numpy as np

NAN_IMAGE = np.uint32(0x7FC00000)


def groups(n_in, window, interval, reference_bound=False):
    """first scan of every group, by the literal loop"""
    out = []
    g = 0
    while True:
        first = g * interval
        if first + window > n_in:
            break
        if reference_bound and not (first < n_in - interval):
            break
        out.append(first)
        g += 1
    return out


def offsets(in_offsets, window, interval, reference_bound=False):
    """(out_offsets [n_out + 1], mid [n_out], largest stacked scan)"""
    off = np.asarray(in_offsets, np.int64)
    firsts = groups(len(off) - 1, window, interval, reference_bound)
    sizes = [int(off[f + window] - off[f]) for f in firsts]
    out = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32) if sizes else np.zeros(1, np.int32)
    mid = np.asarray([f + window // 2 for f in firsts], np.int32)
    return out, mid, (max(sizes) if sizes else 0)


def order(first, window):
    """scans of a group in output order: the middle one, then the others ascending"""
    mid = first + window // 2
    return [mid] + [k for k in range(first, first + window) if k != mid]


def transform(T, xyzi):
    """float32, left to right, no fused operation; the intensity column is returned as it came"""
    T = np.asarray(T, np.float32).reshape(3, 4)
    p = np.ascontiguousarray(xyzi, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = p.copy()
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    out.view(np.uint32)[:, 3] = p.view(np.uint32)[:, 3]
    return out


def stack(oracle, xyzi, in_offsets, poses, window, interval, reference_bound=False, payload=None):
    """dict(xyzi [n, 4] float32, moved [n] bool: the point was transformed, src [n] int32, payload [n] uint32 or None,
    out_offsets, mid)"""
    x = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    off = np.asarray(in_offsets, np.int64)
    poses = np.asarray(poses, np.float32).reshape(-1, 6)
    out_offsets, mid, _ = offsets(off, window, interval, reference_bound)
    parts, moved, src, pay = [], [], [], []
    for first in groups(len(off) - 1, window, interval, reference_bound):
        m = first + window // 2
        for k in order(first, window):
            seg = x[off[k]:off[k + 1]]
            if k == m:
                parts.append(seg.copy())
            else:
                parts.append(transform(oracle.pose_delta(poses[k], poses[m]), seg))
            moved.append(np.full(len(seg), k != m))
            src.append(np.arange(off[k], off[k + 1], dtype=np.int32))
            if payload is not None:
                pay.append(np.asarray(payload).view(np.uint32)[off[k]:off[k + 1]])
    cat = (lambda v, dt, shape: np.concatenate(v).astype(dt, copy=False) if v else np.zeros(shape, dt))
    return dict(xyzi=cat(parts, np.float32, (0, 4)), moved=cat(moved, bool, 0), src=cat(src, np.int32, 0),
                payload=None if payload is None else cat(pay, np.uint32, 0), out_offsets=out_offsets, mid=mid)


def image(xyzi, moved):
    """uint32 image of stacked records with the NaN coordinates of transformed points collapsed to one pattern"""
    a = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    bits = a.view(np.uint32).copy()
    nan = np.isnan(a[:, :3]) & np.asarray(moved, bool)[:, None]
    bits[:, :3][nan] = NAN_IMAGE
    return bits
