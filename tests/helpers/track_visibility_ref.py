"""The numpy statement of scvod_track_visibility_device (include/scvod.h), written sequentially: object after
object, track after track, point after point.  fp32 step by step where the rule says fp32 (the world centre comes from
object_tracks_ref, d2 and the threshold product are np.float32 scalar arithmetic, which neither contracts nor widens), Python ints for
the sums.  It reports what the device reports under the same capacities: the two record tables, the per-point bytes, the eight stats
words and the latch bits."""
import numpy as np

import object_tracks_ref as otr

TRACK_VOTE_DTYPE = np.dtype([("length", "<i4"), ("n_flagged", "<i4"), ("n_moved", "<i4"), ("verdict", "<i4"), ("how", "<i4"),
                             ("max_travel2", "<f4"), ("reserved", "<i4", 2)])
OBJECT_VOTE_DTYPE = np.dtype([("track", "<i4"), ("verdict", "<i4"), ("how", "<i4"), ("travel2", "<f4")])
OBJECT_VIS_DTYPE = np.dtype([("n_points", "<i4"), ("n_untested", "<i4"), ("n_keep", "<i4"), ("n_seen", "<i4"), ("sum_through", "<i4"),
                             ("sum_agree", "<i4"), ("sum_occluded", "<i4"), ("sum_other", "<i4"), ("verdict", "<i4"), ("how", "<i4"),
                             ("reserved", "<i4", 2)])
assert (TRACK_VOTE_DTYPE.itemsize, OBJECT_VOTE_DTYPE.itemsize, OBJECT_VIS_DTYPE.itemsize) == (32, 16, 48)
NO_DYNAMIC, CLEAR = 1, 2
UNTESTED, KEEP, SEEN = 0, 1, 2
L_RECORDS, L_UPSTREAM, L_POINT, L_BROKEN = 1, 2, 4, 8
DEFAULTS = dict(flags=0, window=0, min_travel=2.0, min_length=2, min_moved=1, min_flagged=2, vote_num=1, vote_den=2)
STATS = ("objects", "tracks", "tracks_voted", "members_motion", "members_cleared", "to_seen_through", "to_keep", "latch")
F = np.float32


def travel_threshold(prm):
    """min_travel * min_travel, the fp32 product"""
    return F(F(prm["min_travel"]) * F(prm["min_travel"]))


def track_visibility_ref(objects, offsets, matrices, links, tracks, track_objects, n_tracks, prm, object_vis=None, point_object=None,
                         verdict=None, n_points=None, paint=True, cap_objects=None, cap_tracks=None, cap_track_votes=None,
                         cap_object_votes=None, want_track_votes=True, want_object_votes=True, centres=None):
    """objects / links / track_objects: the caller's tables, cap_objects (default: all) records of each vouched for; offsets
    [n_scans + 1]; matrices [n_scans][12]; tracks: cap_tracks (default: all) records; n_tracks: what d_n_tracks[0] holds; prm: a dict
    with DEFAULTS' keys; object_vis: OBJECT_VIS_DTYPE records or None; point_object int32 [n_points] or None (records only); verdict
    uint8 [n_points] or None (every byte UNTESTED); centres: object_tracks_ref.world_centres of the table when the caller has them
    already.  Returns track_votes / object_votes (the records WRITTEN: none after an upstream overflow, at most the capacity), verdict (the output bytes; None where no byte is written: records only, or a record overflow)
    and stats"""
    n_scans = len(offsets) - 1
    cap_objects = len(objects) if cap_objects is None else cap_objects
    cap_tracks = len(tracks) if cap_tracks is None else cap_tracks
    cap_tv = cap_tracks if cap_track_votes is None else cap_track_votes
    cap_ov = cap_objects if cap_object_votes is None else cap_object_votes
    raw_obj, raw_trk = int(offsets[n_scans]), int(n_tracks)
    paint = paint and point_object is not None
    if point_object is not None:
        n_points = len(point_object)
    elif n_points is None:
        n_points = 0 if verdict is None else len(verdict)
    vin = np.zeros(n_points, np.uint8) if verdict is None else np.asarray(verdict, np.uint8)
    latch = 0
    if raw_obj < 0 or raw_obj > cap_objects or raw_trk < 0 or raw_trk > cap_tracks:
        latch |= L_UPSTREAM
        return dict(track_votes=np.zeros(0, TRACK_VOTE_DTYPE), object_votes=np.zeros(0, OBJECT_VOTE_DTYPE),
                    verdict=vin.copy() if paint else None, stats=dict(zip(STATS, (raw_obj, raw_trk, 0, 0, 0, 0, 0, latch))))
    n, nt = raw_obj, raw_trk
    if (want_track_votes and nt > cap_tv) or (want_object_votes and n > cap_ov):
        latch |= L_RECORDS
    w, thr = int(prm["window"]), travel_threshold(prm)
    with np.errstate(all="ignore"):
        cw = otr.world_centres(objects[:n], matrices) if centres is None else centres
    # per object: flagged, travel2, moved
    flagged, moved, trav = [False] * n, [False] * n, np.zeros(n, np.float32)
    for o in range(n):
        flagged[o] = (not (prm["flags"] & NO_DYNAMIC) and int(objects[o]["dynamic"]) == 1) or \
            (object_vis is not None and int(object_vis[o]["verdict"]) == SEEN)
        t, r = int(links[o]["track"]), int(links[o]["rank"])
        if not (0 <= t < nt):
            continue
        L, ob = int(tracks[t]["length"]), int(tracks[t]["object_begin"])
        if L < prm["min_length"] or ob < 0 or ob + L > cap_objects or not (0 <= r < L):
            continue
        a = int(track_objects[ob + (0 if w == 0 else max(r - w, 0))])
        b = int(track_objects[ob + (L - 1 if w == 0 else min(r + w, L - 1))])
        if 0 <= a < n and 0 <= b < n:
            trav[o] = otr.dist2(cw[a], cw[b])
            moved[o] = bool(trav[o] >= thr)
    # per track
    votes = np.zeros(nt, TRACK_VOTE_DTYPE)
    state = [0] * nt                    # 0 gives a verdict, 1 below min_length, 2 refused
    for t in range(nt):
        L, ob = int(tracks[t]["length"]), int(tracks[t]["object_begin"])
        R = votes[t]
        R["length"], R["verdict"] = L, -1
        if L < prm["min_length"]:
            state[t] = 1
            continue
        members = None if ob < 0 or ob + L > cap_objects else [int(m) for m in track_objects[ob:ob + L]]
        if members is None or any(not (0 <= m < n) for m in members):
            state[t] = 2
            latch |= L_BROKEN
            continue
        nf, nm = sum(1 for m in members if flagged[m]), sum(1 for m in members if moved[m])
        R["n_flagged"], R["n_moved"] = nf, nm
        R["max_travel2"] = max([trav[m] for m in members if not np.isnan(trav[m])], default=F(0.0))
        if nf >= prm["min_flagged"] and nf * prm["vote_den"] >= prm["vote_num"] * L:
            R["verdict"], R["how"] = SEEN, 1
        elif prm["flags"] & CLEAR:
            R["verdict"], R["how"] = KEEP, 3
    # per object
    ovotes = np.zeros(n, OBJECT_VOTE_DTYPE)
    ovotes["track"] = ovotes["verdict"] = -1
    for o in range(n):
        t, r = int(links[o]["track"]), int(links[o]["rank"])
        if t < -1 or t >= nt:
            latch |= L_BROKEN
            continue
        if t < 0 or state[t] == 2:
            continue
        R = ovotes[o]
        if state[t] == 1:
            R["track"] = t
            continue
        if not (0 <= r < int(tracks[t]["length"])):
            latch |= L_BROKEN
            continue
        R["track"], R["travel2"] = t, trav[o]
        if moved[o] and (w > 0 or int(votes[t]["n_moved"]) >= prm["min_moved"]):
            R["verdict"], R["how"] = SEEN, 2
        elif int(votes[t]["how"]) == 1:
            R["verdict"], R["how"] = SEEN, 1
        elif int(votes[t]["how"]) == 3:
            R["verdict"], R["how"] = KEEP, 3
    # per point
    out, to_seen, to_keep = None, 0, 0
    if paint and not (latch & L_RECORDS):
        po = np.asarray(point_object, np.int64)
        inside = (po >= 0) & (po < n)
        if ((po != -1) & ~inside).any():
            latch |= L_POINT                          # treated as -1
        v = np.full(n_points, -1, np.int64)
        v[inside] = ovotes["verdict"][po[inside]]
        out = np.where(v >= 0, v, vin).astype(np.uint8)
        to_seen = int(((v == SEEN) & (vin != SEEN)).sum())
        to_keep = int(((v == KEEP) & (vin != KEEP)).sum())
    stats = dict(zip(STATS, (n, nt, int((votes["how"] == 1).sum()), int((ovotes["how"] == 2).sum()), int((ovotes["how"] == 3).sum()),
                             int(to_seen), int(to_keep), latch)))
    return dict(track_votes=votes[:cap_tv] if want_track_votes else votes[:0], object_votes=ovotes[:cap_ov] if want_object_votes else ovotes[:0],
                verdict=out, stats=stats)
