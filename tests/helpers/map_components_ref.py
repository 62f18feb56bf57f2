"""Plain statement of scvod_map_components and scvod_map_component_visibility (include/scvod.h): a union-find over a dict of cell keys
and the vote in Python ints.  No device, no numpy arithmetic inside the rules: every number is a Python int, so nothing can wrap."""
import numpy as np

import map_ref as mr

COMPONENT_DTYPE = np.dtype([("key", "<u8"), ("n_records", "<i4"), ("first_record", "<i4"), ("cell_min", "<i4", 3), ("cell_max", "<i4", 3),
                            ("reserved", "<i4", 2)])
VISIBILITY_DTYPE = np.dtype([("n_records", "<i4"), ("n_untested", "<i4"), ("n_keep", "<i4"), ("n_seen", "<i4"), ("sum_through", "<i8"),
                             ("sum_agree", "<i8"), ("sum_occluded", "<i8"), ("sum_empty", "<i8"), ("verdict", "<i4"), ("how", "<i4"),
                             ("reserved", "<i4", 2)])
assert COMPONENT_DTYPE.itemsize == 48 and VISIBILITY_DTYPE.itemsize == 64
PAD = int(mr.PAD)
BIAS, BITS = mr.CELL_BIAS, mr.CELL_BITS
FIELD = (1 << BITS) - 1
UNTESTED, KEEP, SEEN_THROUGH = 0, 1, 2
POOL_PAIRS = 1
DEFAULTS = dict(flags=0, min_cells=1, max_cells=0, min_tested=1, min_through=2, vote_num=1, vote_den=2)


def cell_of(key):
    """signed cell coordinates of a key"""
    return ((key >> (2 * BITS)) & FIELD) - BIAS, ((key >> BITS) & FIELD) - BIAS, (key & FIELD) - BIAS


def key_of(cx, cy, cz):
    return ((cx + BIAS) << (2 * BITS)) | ((cy + BIAS) << BITS) | (cz + BIAS)


def offsets(connectivity):
    limit = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
            if (dx, dy, dz) != (0, 0, 0) and abs(dx) + abs(dy) + abs(dz) <= limit]


def components(list_keys, map_keys, connectivity):
    """list_keys: the keys of the caller's list (uint64 array or ints); map_keys: the keys the map holds.  A dict: component int32 [n],
    table COMPONENT_DTYPE [components], stats (the eight words of scvod_map_components_stats, overflow 0, written = components)"""
    keys = [int(k) for k in np.asarray(list_keys, np.uint64).ravel().tolist()]
    held = set(int(k) for k in np.asarray(map_keys, np.uint64).ravel().tolist())
    n = len(keys)
    node = [k != PAD and k in held for k in keys]
    padding = sum(1 for k in keys if k == PAD)
    absent = sum(1 for k, ok in zip(keys, node) if k != PAD and not ok)
    cells = {}
    for i, (k, ok) in enumerate(zip(keys, node)):
        if ok:
            cells.setdefault(k, []).append(i)
    parent = {k: k for k in cells}

    def find(k):
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    offs = [d for d in offsets(connectivity) if d > (0, 0, 0)]     # (an edge is found from its smaller end: a union is symmetric)
    for k in cells:
        cx, cy, cz = cell_of(k)
        for dx, dy, dz in offs:
            x, y, z = cx + dx, cy + dy, cz + dz
            if not (-BIAS <= x < BIAS and -BIAS <= y < BIAS and -BIAS <= z < BIAS):
                continue                                    # a cell that does not exist
            o = key_of(x, y, z)
            if o in cells:
                a, b = find(k), find(o)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    groups = {}
    for k in cells:
        groups.setdefault(find(k), []).append(k)
    order = sorted(groups, key=lambda r: min(groups[r]))
    comp = np.full(n, -1, np.int32)
    table = np.zeros(len(order), COMPONENT_DTYPE)
    for c, r in enumerate(order):
        members = sorted(groups[r])
        idx = [i for k in members for i in cells[k]]
        comp[idx] = c
        xyz = np.array([cell_of(k) for k in members], np.int64)
        table[c] = (members[0], len(idx), min(idx), tuple(xyz.min(axis=0)), tuple(xyz.max(axis=0)), (0, 0))
    nodes = sum(node)
    stats = [n, nodes, padding, absent, nodes - len(cells), len(order), len(order), 0]
    return {"component": comp, "table": table, "stats": stats}


def decide(n_records, n_keep, n_seen, sum_through, sum_agree, p):
    """(verdict, how) of one component, every number a Python int"""
    p = dict(DEFAULTS, **p)
    votes = n_records >= p["min_cells"] and (p["max_cells"] == 0 or n_records <= p["max_cells"]) and n_keep + n_seen >= p["min_tested"]
    if not votes:
        return -1, 0
    t, a = (sum_through, sum_agree) if p["flags"] & POOL_PAIRS else (n_seen, n_keep)
    through = t >= p["min_through"] and t * p["vote_den"] >= p["vote_num"] * (t + a)
    return (SEEN_THROUGH if through else KEEP), 1


def vote(component, n_components, verdict, votes=None, params=None, cap_components=None):
    """records VISIBILITY_DTYPE [min(n_components, cap_components)], the output bytes, and the eight stats words (records written as
    if cap_records held them all, overflow 0)"""
    p = dict(DEFAULTS, **(params or {}))
    comp = np.asarray(component, np.int64).tolist()
    ver = np.asarray(verdict, np.uint8).tolist()
    n = len(comp)
    cap_components = n if cap_components is None else cap_components
    lim = min(n_components, cap_components, n)
    q = None if votes is None else np.asarray(votes).view(np.uint16).reshape(-1, 4).astype(np.int64).tolist()
    acc = [[0] * 7 for _ in range(lim)]                     # n, keep, seen, four sums
    for i in range(n):
        c = comp[i]
        if 0 <= c < lim:
            a = acc[c]
            a[0] += 1
            a[1] += ver[i] == KEEP
            a[2] += ver[i] == SEEN_THROUGH
            if q is not None:
                for j in range(4):
                    a[3 + j] += q[i][j]
    rec = np.zeros(lim, VISIBILITY_DTYPE)
    byte = [0] * lim
    voted = seen = moved_seen = moved_keep = 0
    for c, a in enumerate(acc):
        v, how = decide(a[0], a[1], a[2], a[3], a[4], p)
        rec[c] = (a[0], a[0] - a[1] - a[2], a[1], a[2], a[3], a[4], a[5], a[6], v, how, (0, 0))
        if how:
            byte[c] = v
            voted += 1
            if v == SEEN_THROUGH:
                seen += 1
                moved_seen += a[0] - a[2]
            else:
                moved_keep += a[0] - a[1]
    out = np.array([byte[comp[i]] if 0 <= comp[i] < lim and byte[comp[i]] else ver[i] for i in range(n)], np.uint8).reshape(n)
    stats = [n_components, voted, seen, moved_seen, moved_keep, lim, max(0, n_components - cap_components), 0]
    return {"records": rec, "verdict": out, "stats": stats}
