"""scvod_batch_object_visibility (include/scvod.h) stated in numpy: the whole call from the table's per-point object index
(d_point_object of scvod_batch_objects) or its member list (d_member_src), the caller's verdict bytes and pair counters, the `dynamic`
field of the table's records and the params.  Integers only, so the device has to agree bit for bit."""
import numpy as np

UNTESTED, KEEP, SEEN_THROUGH = 0, 1, 2
POOL_PAIRS, WITH_TRACK = 1, 2
TILE = 2048
DTYPE = np.dtype([("n_points", "<i4"), ("n_untested", "<i4"), ("n_keep", "<i4"), ("n_seen", "<i4"), ("sum_through", "<i4"),
                  ("sum_agree", "<i4"), ("sum_occluded", "<i4"), ("sum_other", "<i4"), ("verdict", "<i4"), ("how", "<i4"),
                  ("reserved", "<i4", 2)])
assert DTYPE.itemsize == 48
STATS = ("objects", "voted", "forced", "seen_through", "moved_to_seen_through", "moved_to_keep", "written", "overflow")
DEFAULTS = dict(flags=0, min_points=1, min_tested=1, min_through=2, vote_num=1, vote_den=2)


def params(**kw):
    p = dict(DEFAULTS)
    assert all(k in p for k in kw), kw
    p.update(kw)
    return p


def point_object_from_members(rec, mem, offs, n_points):
    """the per-point object index of a table from its records (scan, point_begin, n_points) and its member list (input index inside the
    scan); -1 for the points of no object.  A point is a member of at most one object"""
    po = np.full(int(n_points), -1, np.int32)
    for o, r in enumerate(rec):
        m = int(offs[r["scan"]]) + np.asarray(mem[r["point_begin"]:r["point_begin"] + r["n_points"]], np.int64)
        assert (po[m] == -1).all()
        po[m] = o
    return po


def rule(p, n_points, n_keep, n_seen, sum_through, sum_agree, dynamic):
    """(verdict, how) of one object, in Python integers"""
    t, a = (sum_through, sum_agree) if p["flags"] & POOL_PAIRS else (n_seen, n_keep)
    votes = n_points >= p["min_points"] and n_keep + n_seen >= p["min_tested"]
    through = t >= p["min_through"] and t * p["vote_den"] >= p["vote_num"] * (t + a)
    if p["flags"] & WITH_TRACK and dynamic == 1:
        return SEEN_THROUGH, 2
    if votes:
        return (SEEN_THROUGH if through else KEEP), 1
    return -1, 0


def run(point_object, n_objects, verdict, votes=None, dynamic=None, p=None, cap=None):
    """point_object int32 [points]; verdict uint8 [points]; votes uint32 [points] or None; dynamic: the `dynamic` field of the table's
    records or None; cap: the capacity of d_records, None without d_records.  -> dict(records [n_objects] DTYPE, verdict uint8 [points],
    stats int64 [8])"""
    p = params() if p is None else p
    po = np.asarray(point_object, np.int64)
    v = np.asarray(verdict, np.uint8)
    assert po.shape == v.shape
    member = po >= 0
    k = int(n_objects)
    assert not member.any() or po.max() < k
    assert not (p["flags"] & POOL_PAIRS) or votes is not None
    assert not (p["flags"] & WITH_TRACK) or dynamic is not None
    cnt = lambda sel: np.bincount(po[member & sel], minlength=k).astype(np.int64)  # noqa: E731
    rec = np.zeros(k, DTYPE)
    n_points, n_keep, n_seen = cnt(np.ones_like(member)), cnt(v == KEEP), cnt(v == SEEN_THROUGH)
    rec["n_points"], rec["n_keep"], rec["n_seen"] = n_points, n_keep, n_seen
    rec["n_untested"] = n_points - n_keep - n_seen
    sums = np.zeros((4, k), np.int64)
    if votes is not None:
        q = np.asarray(votes).view(np.uint32)
        for j in range(4):
            sums[j] = np.bincount(po[member], weights=((q[member] >> (8 * j)) & 0xFF).astype(np.float64), minlength=k).astype(np.int64)
    for j, name in enumerate(("sum_through", "sum_agree", "sum_occluded", "sum_other")):
        rec[name] = sums[j].astype(np.int32)
    out = v.copy()
    stats = np.zeros(8, np.int64)
    stats[0] = k
    obj_verdict = np.full(k, -1, np.int64)
    for o in range(k):
        verd, how = rule(p, int(n_points[o]), int(n_keep[o]), int(n_seen[o]), int(rec["sum_through"][o]), int(rec["sum_agree"][o]),
                         0 if dynamic is None else int(dynamic[o]))
        rec["verdict"][o], rec["how"][o] = verd, how
        obj_verdict[o] = verd
        stats[1] += how == 1
        stats[2] += how == 2
        stats[3] += how != 0 and verd == SEEN_THROUGH
    new = obj_verdict[np.where(member, po, 0)]
    moved = member & (new >= 0)
    out[moved] = new[moved].astype(np.uint8)
    stats[4] = int((moved & (new == SEEN_THROUGH) & (v != SEEN_THROUGH)).sum())
    stats[5] = int((moved & (new == KEEP) & (v != KEEP)).sum())
    if cap is not None:
        stats[6] = min(k, int(cap))
        stats[7] = int(k > int(cap))
    return dict(records=rec, verdict=out, stats=stats)
