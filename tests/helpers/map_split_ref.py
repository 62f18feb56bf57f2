"""Reference statement of scvod_map_split_device (include/scvod.h) in numpy -- test infrastructure only.

Written from the header's semantics, without a grid: every query looks at every base point.  The squared distance is
d = (dx*dx + dy*dy) + dz*dz in float32 with dx = base.x - query.x; the neighbour is the smallest (d, index) lexicographically.  A base
point is MISS when no query chose it, otherwise GATED when (label & 0xFFFF) is in the reject list, otherwise HIT; the partition lists
the HIT indices ascending, then the MISS, then the GATED ones."""
import numpy as np

MISS, HIT, GATED = 0, 1, 2


def nn(base_xyz, query_xyz, chunk=256):
    """(idx int32, sqdist float32) per query; -1 / +inf for an empty base"""
    b = np.asarray(base_xyz, np.float32)[:, :3]
    q = np.asarray(query_xyz, np.float32)[:, :3]
    idx = np.full(len(q), -1, np.int32)
    sq = np.full(len(q), np.inf, np.float32)
    if len(b) == 0:
        return idx, sq
    for a in range(0, len(q), chunk):
        qq = q[a:a + chunk]
        dx = b[None, :, 0] - qq[:, None, 0]
        dy = b[None, :, 1] - qq[:, None, 1]
        dz = b[None, :, 2] - qq[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        lowest = d.min(axis=1)
        # argmin over (d, index): of the points at the smallest distance, the one with the lowest index
        first = np.where(d == lowest[:, None], np.arange(len(b))[None, :], len(b)).min(axis=1)
        idx[a:a + chunk] = first
        sq[a:a + chunk] = lowest
    return idx, sq


def split(base, query, label=None, reject=(), payload=None):
    """base [n, 3 or 4] float32, query [m, 3 or 4]; label / payload [n] uint32.  Returns a dict: nn_idx, nn_sqdist, mark, order, seg4,
    base_out (the base records in the partition's order, bit for bit), payload_out, and n_hit / n_miss / n_gated"""
    base = np.ascontiguousarray(base, np.float32)
    n = len(base)
    idx, sq = nn(base, query)
    mark = np.zeros(n, np.uint8)
    chosen = np.unique(idx[idx >= 0])
    mark[chosen] = HIT
    reject = [int(v) for v in reject]
    if reject:
        sem = np.asarray(label).astype(np.uint32) & np.uint32(0xFFFF)
        mark[chosen[np.isin(sem[chosen], reject)]] = GATED
    parts = [np.nonzero(mark == k)[0] for k in (HIT, MISS, GATED)]
    order = np.concatenate(parts).astype(np.int32)
    n_hit, n_miss, n_gated = (len(p) for p in parts)
    out = dict(nn_idx=idx, nn_sqdist=sq, mark=mark, order=order, seg4=np.array([0, n_hit, n_hit + n_miss, n], np.int64),
               base_out=base.view(np.uint32)[order].view(np.float32), n_hit=n_hit, n_miss=n_miss, n_gated=n_gated)
    out["payload_out"] = None if payload is None else np.asarray(payload).astype(np.uint32)[order]
    return out
