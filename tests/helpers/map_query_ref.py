"""numpy statement of scvod_map_query (include/scvod.h) on top of map_ref.py: the specification the device is held to, bit for bit.

The map is a dictionary from key to value (what scvod_map_export hands out: a key that is in the table is always met within the probe
bound, a key whose insertion was dropped is not in the export).  A point is moved with k_map_accumulate's expression, products and sums
rounded one by one; its own cell is the key map_ref.encode_points gives it.  With a radius the representatives of the 27 cells around
the own cell are decoded with k_map_export's fp32 expression and compared in fp32.  Beside that definition stands an exhaustive fp32
search over every representative, which the tests use to show that the 27 cells are enough.  Nothing here calls the library."""
import numpy as np

import map_ref as mr

MISS, CELL, NEAR, OUT = 0, 1, 2, 3
PAD = mr.PAD
_U = np.uint64
_F = np.float32


def world(T, p):
    """[n, 3] fp32 world coordinates of the points p [n, >= 3] under the row-major 3x4 matrix T (the expression of encode_points)"""
    T, p = np.asarray(T, _F), np.asarray(p, _F)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([((T[4 * i] * p[:, 0] + T[4 * i + 1] * p[:, 1]) + T[4 * i + 2] * p[:, 2]) + T[4 * i + 3] for i in range(3)], axis=1)


def decode32(keys, vals, leaf):
    """[n, 3] fp32: ((float)c + (q + 0.5f) / 65536.0f) * leaf per axis, every operation rounded to fp32"""
    c, q = mr.unpack_key(keys), mr.unpack_val(vals)
    lf = _F(leaf)
    return np.stack([(c[i].astype(_F) + (q[i].astype(_F) + _F(0.5)) / _F(65536.0)) * lf for i in range(3)], axis=1)


def sqdist32(w, rep):
    """(dx*dx + dy*dy) + dz*dz in fp32 (broadcasts)"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = (w - rep).astype(_F)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _selected(table, labelled, select):
    """(sorted keys, their values) of the cells that count: with a select table (labelled maps) only the selected labels"""
    keys = np.fromiter(table.keys(), np.uint64, len(table))
    vals = np.fromiter(table.values(), np.uint64, len(table))
    if select is not None:
        assert labelled, "a select table needs a labelled map"
        sel = np.zeros(256, bool)
        s = np.asarray(select)
        if s.shape == (256,):
            sel = s != 0
        else:
            sel[s.astype(np.int64).reshape(-1)] = True
        keep = sel[((vals >> _U(8)) & _U(0xFF)).astype(np.int64)]
        keys, vals = keys[keep], vals[keep]
    o = np.argsort(keys)
    return keys[o], vals[o]


def _lookup(skeys, svals, q):
    """(present, value or PAD) of the keys q in the sorted table"""
    if len(skeys) == 0:
        return np.zeros(q.shape, bool), np.full(q.shape, PAD, np.uint64)
    pos = np.minimum(np.searchsorted(skeys, q), len(skeys) - 1)
    hit = skeys[pos] == q
    return hit, np.where(hit, svals[pos], PAD)


def _better(d, key, best_d, best_key, r2):
    return (d < r2) & ((d < best_d) | ((d == best_d) & (key < best_key)))


def query(table, points, offsets, matrices, leaf, radius=0.0, labelled=False, select=None, exhaustive=False):
    """The answer of scvod_map_query for the cloud `points` [n, 4] with host offsets [n_scans + 1] (starting at 0) and one row-major
    3x4 matrix per scan: dict(result uint8 [n], cell_val uint64 [n], nn_key uint64 [n], nn_sqdist float32 [n], scan_counts int64
    [n_scans, 4] = {CELL, NEAR, MISS, OUT}, stats [5] = {points, CELL, NEAR, MISS, OUT}).
    exhaustive=True: candidates are ALL selected representatives instead of those of the 27 cells (same distances, same tie rule)."""
    points = np.asarray(points, _F).reshape(-1, 4)
    offsets = np.asarray(offsets, np.int64)
    n, n_scans = len(points), len(offsets) - 1
    assert n_scans == 0 or (offsets[0] == 0 and offsets[-1] == n)
    radius, leaf = _F(radius), _F(leaf)
    assert radius >= 0 and radius <= _F(0.99) * leaf
    r2 = radius * radius
    skeys, svals = _selected(table, labelled, select)
    w = np.zeros((n, 3), _F)
    key = np.full(n, PAD, np.uint64)
    ok = np.zeros(n, bool)
    for s in range(n_scans):
        a, b = int(offsets[s]), int(offsets[s + 1])
        w[a:b] = world(matrices[s], points[a:b])
        k, _, o = mr.encode_points(matrices[s], np.concatenate([points[a:b, :3], np.zeros((b - a, 1), _F)], axis=1), leaf)
        key[a:b], ok[a:b] = np.where(o, k, PAD), o
    found, cell_val = _lookup(skeys, svals, key)
    found &= ok
    cell_val = np.where(found, cell_val, PAD)
    best_d = np.full(n, np.inf, _F)
    best_key = np.full(n, PAD, np.uint64)
    if radius > 0 and exhaustive:
        rep = decode32(skeys, svals, leaf)
        for a in range(0, n, 256):
            d = sqdist32(w[a:a + 256, None, :], rep[None, :, :])                    # [chunk, cells]
            d = np.where((d < r2) & ok[a:a + 256, None], d, _F(np.inf))
            if d.shape[1] == 0:
                continue
            dmin = d.min(axis=1)
            kk = np.where(d == dmin[:, None], skeys[None, :], PAD).min(axis=1)      # equal d: the smaller key
            hit = np.isfinite(dmin)
            best_d[a:a + 256] = np.where(hit, dmin, _F(np.inf))
            best_key[a:a + 256] = np.where(hit, kk, PAD)
    elif radius > 0:
        c = mr.unpack_key(np.where(ok, key, _U(0)))
        for ox in (-1, 0, 1):
            for oy in (-1, 0, 1):
                for oz in (-1, 0, 1):
                    cc = [c[0] + ox, c[1] + oy, c[2] + oz]
                    exists = ok.copy()
                    for v in cc:
                        exists &= (v >= -mr.CELL_BIAS) & (v < mr.CELL_BIAS)             # a cell outside the range does not exist
                    nk = np.where(exists, mr.pack_key(*[np.where(exists, v, 0) for v in cc]), PAD)
                    hit, nv = _lookup(skeys, svals, nk)
                    hit &= exists
                    d = sqdist32(w, decode32(np.where(hit, nk, _U(0)), np.where(hit, nv, _U(0)), leaf))
                    take = hit & _better(d, nk, best_d, best_key, r2)
                    best_d = np.where(take, d, best_d)
                    best_key = np.where(take, nk, best_key)
    result = np.where(~ok, OUT, np.where(found, CELL, np.where(best_key != PAD, NEAR, MISS))).astype(np.uint8)
    counts = np.zeros((n_scans, 4), np.int64)
    for s in range(n_scans):
        r = result[int(offsets[s]):int(offsets[s + 1])]
        counts[s] = [(r == CELL).sum(), (r == NEAR).sum(), (r == MISS).sum(), (r == OUT).sum()]
    return dict(result=result, cell_val=cell_val, nn_key=best_key, nn_sqdist=best_d, scan_counts=counts,
                stats=np.concatenate([[n], counts.sum(axis=0)]).astype(np.int64))


def table_of(keys, vals):
    """the dictionary of a record list (one record per key, as an export gives it)"""
    keys, vals = np.asarray(keys, np.uint64).ravel(), np.asarray(vals, np.uint64).ravel()
    assert len(np.unique(keys)) == len(keys) and not (keys == PAD).any()
    return dict(zip(keys.tolist(), vals.tolist()))


def build_table(points, matrix, leaf, labels=None):
    """the dictionary an accumulate of `points` [n, 4] under one matrix leaves: per cell the smallest value (map_ref.encode_points /
    reduce_records); with label bytes the labelled kind's value, offsets << 16 | label << 8 | (int)clamp(intensity, 0, 255)"""
    points = np.asarray(points, _F)
    k, v, ok = mr.encode_points(matrix, points, leaf)
    if labels is not None:
        qi = np.clip(points[:, 3], _F(0), _F(255)).astype(np.int64).astype(np.uint64)
        v = (v & ~_U(0xFFFF)) | (np.asarray(labels, np.uint64) << _U(8)) | qi
    return table_of(*mr.reduce_records(k[ok], v[ok]))


def cell_centres(keys, leaf):
    """[n, 4] fp32 points at the centres of the cells `keys` (coordinates must be small enough for (c + 0.5) * leaf to stay inside)"""
    c = mr.unpack_key(keys)
    p = np.zeros((len(c[0]), 4), _F)
    for i in range(3):
        p[:, i] = ((c[i].astype(np.float64) + 0.5) * np.float64(_F(leaf))).astype(_F)
    return p


def seeded_cloud(seed, n=20000, centre=(1000.0, -1000.0, 990.0)):
    """the cloud of the nearest-representative tests: about n points in a 20 m cube around `centre` -- a dense ground patch and two
    walls (many points per cell, neighbours well within a cell edge) and a uniform rest -- in random order"""
    rng = np.random.default_rng(seed)
    n_g, n_w = n // 2, n // 4
    g = np.stack([rng.uniform(-5, 5, n_g), rng.uniform(-5, 5, n_g), rng.normal(-1.6, 0.02, n_g)], axis=1)   # (z on a cell face at leaf 0.2)
    w1 = np.stack([rng.uniform(-10, 10, n_w // 2), rng.normal(4.0, 0.03, n_w // 2), rng.uniform(-2, 3, n_w // 2)], axis=1)
    w2 = np.stack([rng.normal(-6.0, 0.03, n_w - n_w // 2), rng.uniform(-10, 10, n_w - n_w // 2), rng.uniform(-2, 3, n_w - n_w // 2)], axis=1)
    u = rng.uniform(-10, 10, (n - n_g - n_w, 3))
    xyz = np.concatenate([g, w1, w2, u])[rng.permutation(n)] + np.asarray(centre, np.float64)
    return np.concatenate([xyz, rng.uniform(0, 255, (n, 1))], axis=1).astype(_F)


def tie_case(leaf=0.2):
    """Two representatives symmetric about a query so that d ties exactly, in the cells (4, 8, 2) and (5, 8, 2): (keys, vals, query
    point [1, 4], the smaller key).  The case is built on the decoded fp32 coordinates themselves: the query's y and z are the
    representatives' own and its x is the fp32 midpoint of the two decoded x; the offsets are the first pair for which that midpoint
    is exact, i.e. for which both fp32 distances are equal."""
    leaf = _F(leaf)
    keys = mr.pack_key(np.array([4, 5]), np.array([8, 8]), np.array([2, 2]))
    for qa in range(60000, 60400):
        vals = mr.pack_val(np.array([qa, 65536 - qa]), np.array([30000, 30000]), np.array([1000, 1000]), np.array([7, 9]))
        rep = decode32(keys, vals, leaf)
        q = np.zeros((1, 4), _F)
        q[0, 0] = _F((rep[0, 0].astype(np.float64) + rep[1, 0].astype(np.float64)) / 2)
        q[0, 1:3] = rep[0, 1:3]
        d = sqdist32(q[:, :3], rep)
        if d[0] == d[1] and d[0] > 0:
            return keys, vals, q, int(keys.min())
    raise AssertionError("no exact tie found")


# the nearest-representative cases tests/test_capi_map_query.py (27 cells == exhaustive) and tests/test_gpu_map_query.py (device ==
# both) share: the map is built from the first half of seeded_cloud under the identity pose, the second half queries it as two scans
LEAF = 0.2
R_SMALL, R_MAX = float(_F(0.05)), float(_F(0.99) * _F(LEAF))
STATIC = [v for v in range(256) if v != 6]
NEAREST_CASES = [
    dict(id="plain-r0.05", seed=71, centre=(1000.0, -1000.0, 990.0), radius=R_SMALL, labelled=False, select=None),
    dict(id="plain-rmax", seed=72, centre=(-1000.0, 1000.0, -990.0), radius=R_MAX, labelled=False, select=None),
    dict(id="labelled-r0.05", seed=73, centre=(-1000.0, -990.0, 1000.0), radius=R_SMALL, labelled=True, select=None),
    dict(id="labelled-static-r0.05", seed=74, centre=(990.0, 1000.0, -1000.0), radius=R_SMALL, labelled=True, select=STATIC),
    dict(id="labelled-static-rmax", seed=75, centre=(1000.0, 1000.0, 1000.0), radius=R_MAX, labelled=True, select=STATIC),
]
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], _F)
_nearest = {}


def nearest_reference(case):
    """computed once per case and process: the two halves, the map's dictionary and both answers"""
    if case["id"] not in _nearest:
        cloud = seeded_cloud(case["seed"], centre=case["centre"])
        half = len(cloud) // 2
        base, q = cloud[:half], cloud[half:]
        labels = None
        if case["labelled"]:
            labels = np.random.default_rng(case["seed"] + 1000).choice(np.array([1, 3, 4, 5, 6, 7], np.uint8), half)
        table = build_table(base, IDENTITY, LEAF, labels)
        offsets = np.array([0, len(q) - 8193, len(q)], np.int32)      # (the second scan takes two workgroups, the last of them one point)
        kw = dict(labelled=case["labelled"], select=case["select"])
        _nearest[case["id"]] = dict(
            base=base, labels=labels, query=q, offsets=offsets, table=table,
            own_key=mr.encode_points(IDENTITY, q, LEAF)[0],
            cells27=query(table, q, offsets, [IDENTITY, IDENTITY], LEAF, case["radius"], **kw),
            exhaustive=query(table, q, offsets, [IDENTITY, IDENTITY], LEAF, case["radius"], exhaustive=True, **kw))
    return _nearest[case["id"]]
