"""The numpy statement of scvod_object_tracks_device (include/scvod.h), written as a sequential tracker: the chains
of the successor table are walked scan by scan, every scan's objects propose to the objects of the next one, every object of that scan
accepts one proposer, and a link extends the track of its proposer at once.  No pointer jumping, no atomics, no packed keys: what the
device does in parallel must come out the same byte for byte.  fp32 where the rule says fp32, in the stated order (np.float32 scalar
arithmetic neither contracts nor widens).  Also a builder for crafted tables."""
import numpy as np

OBJECT_DTYPE = np.dtype([("scan", "i4"), ("name", "i4"), ("n_points", "i4"), ("n_voxels", "i4"), ("box_min", "f4", 3),
                         ("box_max", "f4", 3), ("center", "f4", 3), ("angle_diff", "f4"), ("cls", "i1"), ("state", "i1"),
                         ("dynamic", "u1"), ("reserved", "u1"), ("point_begin", "i4")])
LINK_DTYPE = np.dtype([("track", "<i4"), ("rank", "<i4"), ("pred", "<i4"), ("succ", "<i4"), ("kind", "<i4"), ("weight", "<i4"),
                       ("step", "<f4"), ("reserved", "<i4")])
TRACK_DTYPE = np.dtype([("first_object", "<i4"), ("last_object", "<i4"), ("length", "<i4"), ("first_scan", "<i4"), ("last_scan", "<i4"),
                        ("n_dynamic", "<i4"), ("n_gate_links", "<i4"), ("object_begin", "<i4"), ("net", "<f4", 3), ("path", "<f4"),
                        ("max_step", "<f4"), ("reserved", "<i4", 3)])
assert (OBJECT_DTYPE.itemsize, LINK_DTYPE.itemsize, TRACK_DTYPE.itemsize) == (64, 32, 64)
NO_GATE, ANY_CLASS = 1, 2
DEFAULTS = dict(flags=0, occupancy=-1.0, gate=2.0, size_ratio=1.5, min_points=10, min_length=2)
STATS = ("objects", "tracks", "written", "overlap_links", "gate_links", "refused", "longest", "overflow")
F = np.float32


def next_table(n_scans, next_scan=None):
    """the successor of every scan (-1: none), or None when scvod_visibility_viewers' rules refuse the table"""
    nxt = [(s + 1 if s + 1 < n_scans else -1) if next_scan is None else int(next_scan[s]) for s in range(n_scans)]
    prev = [-1] * n_scans
    for s, v in enumerate(nxt):
        if v >= n_scans or v == s:
            return None
        if v >= 0:
            if prev[v] >= 0:
                return None
            prev[v] = s
    reached = 0
    for s in range(n_scans):
        if prev[s] < 0:
            k = s
            while k >= 0:
                reached += 1
                k = nxt[k]
    if reached != n_scans:
        return None
    return [v if v >= 0 else -1 for v in nxt]


def world_centres(objects, matrices):
    """cW of every object: T0*x + T1*y + T2*z + T3 per row, left to right in fp32"""
    out = np.zeros((len(objects), 3), np.float32)
    for i, o in enumerate(objects):
        T = matrices[int(o["scan"])]
        x, y, z = (F(v) for v in o["center"])
        for r in range(3):
            out[i, r] = F(F(F(F(T[4 * r]) * x) + F(F(T[4 * r + 1]) * y)) + F(F(T[4 * r + 2]) * z)) + F(T[4 * r + 3])
    return out


def diagonals(objects):
    out = np.zeros(len(objects), np.float32)
    for i, o in enumerate(objects):
        ex, ey, ez = (F(F(o["box_max"][k]) - F(o["box_min"][k])) for k in range(3))
        with np.errstate(all="ignore"):
            out[i] = np.sqrt(F(F(F(ex * ex) + F(ey * ey)) + F(ez * ez)))
    return out


def dist2(a, b):
    with np.errstate(all="ignore"):
        dx, dy, dz = F(b[0] - a[0]), F(b[1] - a[1]), F(b[2] - a[2])
        return F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))


def propose(a, objects, lo, hi, cands, cw, diag, prm):
    """the proposal of object a towards the objects [lo, hi) of its successor scan: (kind, b, count, d2) or None"""
    A = objects[a]
    if int(A["cls"]) == 2:
        best = None
        for b, cnt in cands:
            if not (lo <= b < hi) or cnt < 0 or int(objects[b]["cls"]) != 2:
                continue
            with np.errstate(all="ignore"):
                ratio = F(cnt) / F(int(objects[b]["n_voxels"]))
            if not ratio >= F(prm["occupancy"]):
                continue
            if best is None or cnt > best[1] or (cnt == best[1] and b < best[0]):
                best = (b, cnt)
        if best is not None:
            return (1, best[0], best[1], None)
    if prm["flags"] & NO_GATE:
        return None
    if not ((prm["flags"] & ANY_CLASS) or int(A["cls"]) == 2) or int(A["n_points"]) < prm["min_points"]:
        return None
    ratio, g2 = F(prm["size_ratio"]), F(F(prm["gate"]) * F(prm["gate"]))
    best = None
    for b in range(lo, hi):
        Bo = objects[b]
        if int(Bo["cls"]) != int(A["cls"]) or int(Bo["n_points"]) < prm["min_points"]:
            continue
        with np.errstate(all="ignore"):
            if not (diag[a] <= F(ratio * diag[b])) or not (diag[b] <= F(ratio * diag[a])):
                continue
        d2 = dist2(cw[a], cw[b])
        if not d2 < g2:
            continue
        if best is None or d2 < best[1]:     # (ascending b: a tie keeps the smaller one)
            best = (b, d2)
    return None if best is None else (2, best[0], 0, best[1])


def object_tracks_ref(objects, offsets, next_scan, matrices, cand_begin, cand, prm, cap_links=None, cap_tracks=None,
                      want_tracks=True):
    """objects: OBJECT_DTYPE records; offsets [n_scans + 1]; next_scan [n_scans] or None; matrices [n_scans][12] float32 (the pose
    matrices); cand_begin / cand [pairs][2] or None; prm: a dict with DEFAULTS' keys, occupancy already resolved (>= 0).
    Returns links, tracks, track_objects (the whole list), n_tracks as the device reports it (-1 after an overflow) and the eight stats
    words.  After a cap_links overflow links / tracks / track_objects are None: nothing is written"""
    objects = np.ascontiguousarray(objects, OBJECT_DTYPE).reshape(-1)
    n_scans = len(offsets) - 1
    n = int(offsets[n_scans])
    cap_links = n if cap_links is None else cap_links
    cap_tracks = n if cap_tracks is None else cap_tracks
    if n > cap_links:
        return dict(links=None, tracks=None, track_objects=None, n_tracks=-1, stats=dict(zip(STATS, (n, 0, 0, 0, 0, 0, 0, 1))))
    objects = objects[:n]
    nxt = next_table(n_scans, next_scan)
    assert nxt is not None, "a refused successor table"
    cw, diag = world_centres(objects, matrices), diagonals(objects)
    links = np.zeros(n, LINK_DTYPE)
    links["track"] = links["pred"] = links["succ"] = -1
    members = {}                       # head -> its track's objects in rank order
    head_of = list(range(n))
    refused = 0
    has_prev = [False] * n_scans
    for v in nxt:
        if v >= 0:
            has_prev[v] = True
    for start in range(n_scans):
        if has_prev[start]:
            continue
        s = start
        while s >= 0:                  # the chain of scans that starts here, scan by scan
            for a in range(int(offsets[s]), int(offsets[s + 1])):
                if int(links[a]["pred"]) < 0:
                    members[a] = [a]   # nobody of the scan before continues into a: a new track
            nx = nxt[s]
            if nx >= 0:
                lo, hi = int(offsets[nx]), int(offsets[nx + 1])
                proposals = {}         # b -> [(kind, count, d2, a)]
                for a in range(int(offsets[s]), int(offsets[s + 1])):
                    cl = [] if cand_begin is None or cand is None else \
                        [(int(cand[j][0]), int(cand[j][1])) for j in range(int(cand_begin[a]), int(cand_begin[a + 1]))]
                    p = propose(a, objects, lo, hi, cl, cw, diag, prm)
                    if p is not None:
                        proposals.setdefault(p[1], []).append((p[0], p[2], p[3], a))
                for b, ps in proposals.items():
                    win = None
                    for kind, cnt, d2, a in ps:       # ascending a: a tie keeps the smaller one
                        if win is None:
                            win = (kind, cnt, d2, a)
                        elif kind < win[0] or (kind == win[0] and ((kind == 1 and cnt > win[1]) or (kind == 2 and d2 < win[2]))):
                            win = (kind, cnt, d2, a)
                    refused += len(ps) - 1
                    kind, cnt, d2, a = win
                    with np.errstate(all="ignore"):
                        step = np.sqrt(dist2(cw[a], cw[b]))
                    links[b]["pred"], links[b]["kind"], links[b]["weight"], links[b]["step"] = a, kind, cnt if kind == 1 else 0, step
                    links[a]["succ"] = b
                    links[b]["rank"] = int(links[a]["rank"]) + 1
                    head_of[b] = head_of[a]
                    members[head_of[a]].append(b)
            s = nx
    listed = [h for h in sorted(members) if len(members[h]) >= prm["min_length"]]
    tracks = np.zeros(len(listed), TRACK_DTYPE)
    track_objects = []
    for t, h in enumerate(listed):
        m = members[h]
        path, mx = F(0.0), F(0.0)
        with np.errstate(all="ignore"):
            for o in m:
                st = F(links[o]["step"])
                path = F(path + st)
                mx = st if st > mx else mx
        R = tracks[t]
        R["first_object"], R["last_object"], R["length"] = m[0], m[-1], len(m)
        R["first_scan"], R["last_scan"] = objects[m[0]]["scan"], objects[m[-1]]["scan"]
        R["n_dynamic"] = sum(1 for o in m if int(objects[o]["dynamic"]) == 1)
        R["n_gate_links"] = sum(1 for o in m if int(links[o]["kind"]) == 2)
        R["object_begin"] = len(track_objects)
        with np.errstate(all="ignore"):
            R["net"] = [F(cw[m[-1]][k] - cw[m[0]][k]) for k in range(3)]
        R["path"], R["max_step"] = path, mx
        for o in m:
            links[o]["track"] = t
        track_objects += m
    over = want_tracks and len(listed) > cap_tracks
    stats = dict(zip(STATS, (n, len(listed), (min(len(listed), cap_tracks) if want_tracks else 0), int((links["kind"] == 1).sum()),
                             int((links["kind"] == 2).sum()), refused, max([len(members[h]) for h in listed], default=0), int(over))))
    return dict(links=links, tracks=tracks[:cap_tracks], track_objects=np.asarray(track_objects, np.int32).reshape(-1),
                n_tracks=-1 if over else len(listed), stats=stats)


def identity_matrices(n_scans):
    T = np.zeros((n_scans, 12), np.float32)
    T[:, 0] = T[:, 5] = T[:, 10] = 1.0
    return T


def build_table(scans, next_scan=None):
    """crafted tables.  scans: per scan a list of dicts with the keys center (3 floats; default 0), box_min / box_max (default 0 / the
    key `size`, default (1, 1, 1)), cls (2), n_points (100), n_voxels (10), dynamic (0), cand: [(index of an object INSIDE the successor
    scan, or a ("abs", table index) pair, count)].  Returns (objects, offsets int32, cand_begin int32, cand int32 [pairs][2])"""
    n_scans = len(scans)
    nxt = next_table(n_scans, next_scan)
    assert nxt is not None
    offsets = np.zeros(n_scans + 1, np.int32)
    for s, sc in enumerate(scans):
        offsets[s + 1] = offsets[s] + len(sc)
    objects = np.zeros(int(offsets[-1]), OBJECT_DTYPE)
    cand_begin, cand = [0], []
    i = 0
    for s, sc in enumerate(scans):
        for k, d in enumerate(sc):
            o = objects[i]
            o["scan"], o["name"] = s, k
            o["n_points"], o["n_voxels"] = d.get("n_points", 100), d.get("n_voxels", 10)
            o["box_min"] = d.get("box_min", (0.0, 0.0, 0.0))
            o["box_max"] = d.get("box_max", d.get("size", (1.0, 1.0, 1.0)))
            o["center"] = d.get("center", (0.0, 0.0, 0.0))
            o["cls"], o["state"], o["dynamic"] = d.get("cls", 2), d.get("state", -1), d.get("dynamic", 0)
            o["point_begin"] = 100 * i
            for j, cnt in d.get("cand", ()):
                if isinstance(j, tuple):
                    cand.append((int(j[1]), int(cnt)))
                else:
                    cand.append((int(offsets[nxt[s]]) + int(j) if nxt[s] >= 0 else -1, int(cnt)))
            cand_begin.append(len(cand))
            i += 1
    return objects, offsets, np.asarray(cand_begin, np.int32), np.asarray(cand, np.int32).reshape(-1, 2)
