"""numpy statement of scvod_map_filter / scvod_batch_map_filter (include/scvod.h) on top of map_query_ref.query: the specification the
device is held to, byte for byte.

The result byte is the query's.  A point's own side is a function of that byte alone.  With the vote, the members of every object --
given here as the object index of every INPUT point (-1: no member) and the table's n_points, since the table itself is tested
elsewhere -- are counted, the verdict is the header's integer rule in Python integers (which cannot overflow), and a member whose
result is not OUT takes it.  The partition is plain boolean indexing per scan.  Nothing here calls the library."""
import numpy as np

import map_query_ref as mq

KNOWN, NOVEL, OUT = 0, 1, 2
OBJECT_VOTE = 1
SIDE_OF_RESULT = np.array([NOVEL, KNOWN, KNOWN, OUT], np.uint8)      # indexed by MISS, CELL, NEAR, OUT
OBJECT_DTYPE = np.dtype([("n_cell", "<i4"), ("n_near", "<i4"), ("n_miss", "<i4"), ("n_out", "<i4"), ("n_points", "<i4"), ("verdict", "<i4"),
                         ("reserved", "<i4", 2)])
DEFAULTS = dict(radius=0.0, flags=0, vote_num=1, vote_den=2, min_points=1, reserved=0)
STATS = ("points", "known", "novel", "out", "moved_to_known", "moved_to_novel", "objects_voted", "objects_known")


def params(**kw):
    """the defaults of scvod_map_filter_params_default, overridden by keyword"""
    assert set(kw) <= set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


def _get(p, name):
    return p[name] if isinstance(p, dict) else getattr(p, name)


def own_side(result):
    return SIDE_OF_RESULT[np.asarray(result, np.int64)]


def object_known(n_cell, n_near, n_points, vote_num, vote_den):
    """(int64)(n_cell + n_near) * vote_den >= (int64)vote_num * n_points, in Python integers"""
    return (int(n_cell) + int(n_near)) * int(vote_den) >= int(vote_num) * int(n_points)


def vote(result, point_object, objects, p):
    """(final sides [n], votes [len(objects)] OBJECT_DTYPE, the four vote words of the stats) for result bytes [n], the object index of
    every input point [n] (-1: none) and the objects' n_points"""
    result = np.asarray(result, np.uint8)
    po = np.asarray(point_object, np.int64)
    side = own_side(result).copy()
    votes = np.zeros(len(objects), OBJECT_DTYPE)
    moved_nk = moved_kn = voted = voted_known = 0
    for o, n_points in enumerate(np.asarray(objects, np.int64).tolist()):
        mem = np.flatnonzero(po == o)
        r = result[mem]
        c = [int((r == v).sum()) for v in (mq.CELL, mq.NEAR, mq.MISS, mq.OUT)]
        assert sum(c) == n_points, "the per-point objects and the table's n_points disagree"
        votes[o]["n_cell"], votes[o]["n_near"], votes[o]["n_miss"], votes[o]["n_out"] = c
        votes[o]["n_points"] = n_points
        votes[o]["verdict"] = -1
        if n_points < int(_get(p, "min_points")):
            continue
        known = object_known(c[0], c[1], n_points, _get(p, "vote_num"), _get(p, "vote_den"))
        votes[o]["verdict"] = KNOWN if known else NOVEL
        side[mem[r != mq.OUT]] = KNOWN if known else NOVEL
        voted += 1
        voted_known += int(known)
        moved_nk += c[2] if known else 0
        moved_kn += 0 if known else c[0] + c[1]
    return side, votes, [moved_nk, moved_kn, voted, voted_known]


def partition(side, offsets, points, payload=None):
    """(order int32 [n], bounds int32 [n_scans, 2], xyzi [n, 4], payload or None): per scan the KNOWN, the NOVEL, then the OUT points,
    each in input order"""
    side = np.asarray(side, np.uint8)
    offsets = np.asarray(offsets, np.int64)
    n_scans = len(offsets) - 1
    order = np.zeros(len(side), np.int32)
    bounds = np.zeros((n_scans, 2), np.int32)
    for s in np.flatnonzero(np.diff(offsets)).tolist():              # (an empty scan has no order and bounds 0, 0)
        a, b = int(offsets[s]), int(offsets[s + 1])
        idx = np.arange(b - a, dtype=np.int32)
        sc = side[a:b]
        order[a:b] = np.concatenate([idx[sc == KNOWN], idx[sc == NOVEL], idx[sc == OUT]])
        bounds[s] = [(sc == KNOWN).sum(), (sc == KNOWN).sum() + (sc == NOVEL).sum()]
    src = order.astype(np.int64) + np.repeat(offsets[:-1], np.diff(offsets))
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    xyzi = pts.view(np.uint32)[src].view(np.float32)                 # (moved as words: NaN payloads survive)
    pay = None if payload is None else np.asarray(payload).reshape(-1)[src]
    return order, bounds, xyzi, pay


def filter(table, points, offsets, matrices, leaf, params, labelled, select, point_object=None, objects=None, payload=None):
    """The answer of scvod_map_filter (point_object None) or scvod_batch_map_filter for the cloud `points` [n, 4] with host offsets
    [n_scans + 1] starting at 0: dict(result, side, order, bounds, xyzi, payload, votes, stats [8])."""
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    result = mq.query(table, points, offsets, matrices, leaf, _get(params, "radius"), labelled=labelled, select=select)["result"]
    return filter_from_result(result, points, offsets, params, point_object, objects, payload)


def filter_from_result(result, points, offsets, params, point_object=None, objects=None, payload=None):
    """filter() behind the query: everything that follows from the result bytes (tests that ask one map with several vote rules
    compute the bytes once)"""
    p = params
    assert _get(p, "reserved") == 0 and not (_get(p, "flags") & ~OBJECT_VOTE)
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 4)
    side, votes, words = own_side(result), None, [0, 0, 0, 0]
    if _get(p, "flags") & OBJECT_VOTE:
        assert point_object is not None and objects is not None
        side, votes, words = vote(result, point_object, objects, p)
    order, bounds, xyzi, pay = partition(side, offsets, points, payload)
    stats = np.array([len(points), (side == KNOWN).sum(), (side == NOVEL).sum(), (side == OUT).sum()] + words, np.int64)
    return dict(result=result, side=side, order=order, bounds=bounds, xyzi=xyzi, payload=pay, votes=votes, stats=stats)
