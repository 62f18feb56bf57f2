"""Crafted clouds for the correspondence search (A7: scvod_nn_search, scvod_nn_radius_search, scvod_nn_search_device): named cases
(map_xyz, query_xyz, radius), all float32, built by plain arithmetic -- nothing here is random.  The expected answer of every case is the
brute-force oracle's (oracle.nn_search); tests/test_nn_search_cases.py holds every case to the property it is there for, and
tests/test_gpu_nn_search_crafted.py runs them through the three entry points.

How the literals were found: tests/devtools/nn_sliver_model.py restates the fp32 cell rule of csrc/scvod_grid.h in numpy, walks the fp32
values around every cell face for pairs (q, p) with fl(d^2) < fl(r * r) that the rule puts two cells apart when the cell edge is the radius
and the grid origin is ORIGIN, and walks the offset t of (s, t) until fl(fl(s * s) + fl(t * t)) is bit-equal to a named threshold.  Its
output is committed below as bit patterns; the values in the comments are their shortest decimal forms.
"""
import collections

import numpy as np

F = np.float32
Case = collections.namedtuple("Case", "name map query radius meta")


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def roll(p, axis):
    """the coordinates of p moved `axis` places on: a case built along x, laid along y or z"""
    return np.roll(np.asarray(p, F), axis, axis=-1)


def frac(n, k=0.6180339887498949, start=0.0):
    """n numbers in [0, 1), evenly scattered and always the same: the fractional parts of start + i * k"""
    return (start + np.arange(n, dtype=np.float64) * k) % 1.0


def sqdist(p, q):
    """the fp32 expression of the library and of the oracle"""
    d = np.asarray(p, F) - np.asarray(q, F)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def bounded(idx, sq, within):
    """what scvod_nn_radius_search promises, from the oracle's unbounded answer (as test_nn_radius_search_parity derives it)"""
    inside = within != 0
    return np.where(inside, idx, -1).astype(np.int32), np.where(inside, sq, F(np.inf)).astype(F), inside.astype(np.uint8)


_EXPECTED = {}


def expected(oracle, case, reverse=False):
    """the oracle's (idx, sqdist, within) of a case (of its map in reverse order), computed once and shared; read-only"""
    key = (case.name, reverse)
    if key not in _EXPECTED:
        out = oracle.nn_search(case.map[::-1] if reverse else case.map, case.query, case.radius)
        for a in out:
            a.setflags(write=False)
        _EXPECTED[key] = out
    return _EXPECTED[key]


def _case(name, m, q, radius, **meta):
    return Case(name, np.ascontiguousarray(m, F).reshape(-1, 3), np.ascontiguousarray(q, F).reshape(-1, 3), float(radius), meta)


# ---- the radius sliver ------------------------------------------------------------------------------------------------------------------
ORIGIN = f32(0xc2147df4)        # -37.123: the map's min corner on every axis (the first map point of a sliver case sits there)
SLIVER_RADII = (0.2, 0.3, 0.35, 1.0)
# radius -> (q, p) on one axis.  None exists for radius 1.0 (nor for any cell whose reciprocal is a power of two: the product is exact and
# the subtraction alone cannot push q up and p down at once); that radius is held by the block of separations alone
SLIVER = {
    0.2: [(0x405e8723, 0x4051ba57),    # q = 3.476998, p = 3.2769983, d2 = 0.039999925
          (0x408f438e, 0x4088dd2b),    # q = 4.4769964, p = 4.276998, d2 = 0.03999935
          (0x41713b5e, 0x416e082d),    # q = 15.076994, p = 14.876996, d2 = 0.03999916
          (0x41d89dae, 0x41d70416),    # q = 27.076992, p = 26.876995, d2 = 0.03999878
          (0x41fbd0e3, 0x41fa374a),    # q = 31.476995, p = 31.276997, d2 = 0.03999954
          (0x42bfc105, 0x42bf5a9f),    # q = 95.87699, p = 95.676994, d2 = 0.03999878
          (0x42cc8dd1, 0x42cc276b)],   # q = 102.276985, p = 102.07699, d2 = 0.03999878
    0.3: [(0x41b70417, 0x41b49db1),    # q = 22.876997, p = 22.576998, d2 = 0.08999954
          (0x41db0416, 0x41d89db2),    # q = 27.376995, p = 27.077, d2 = 0.089997254
          (0x41fa374b, 0x41f7d0e5),    # q = 31.276999, p = 30.977, d2 = 0.08999954
          (0x4241820b, 0x42404ed9),    # q = 48.376995, p = 48.077, d2 = 0.089997254
          (0x4253820b, 0x42524ed9),    # q = 52.876995, p = 52.577, d2 = 0.089997254
          (0x42b7c105, 0x42b7276c),    # q = 91.87699, p = 91.576996, d2 = 0.089997254
          (0x42ff276c, 0x42fe8dd3)],   # q = 127.576996, p = 127.277, d2 = 0.089997254
    0.35: [(0x4203820b, 0x42021ba5),   # q = 32.876995, p = 32.526997, d2 = 0.12249893
           (0x42294ed7, 0x4227e871),   # q = 42.326992, p = 41.976994, d2 = 0.12249893
           (0x4234820b, 0x42331ba5),   # q = 45.126995, p = 44.776997, d2 = 0.12249893
           (0x4250820b, 0x424f1ba5),   # q = 52.126995, p = 51.776997, d2 = 0.12249893
           (0x42764ed7, 0x4274e871),   # q = 61.576992, p = 61.226994, d2 = 0.12249893
           (0x42d40dd1, 0x42d35a9f),   # q = 106.026985, p = 105.676994, d2 = 0.122493595
           (0x42fe0dd1, 0x42fd5a9f)],  # q = 127.026985, p = 126.676994, d2 = 0.122493595
    1.0: [],
}
# radius -> a: a second map point A = q + a on ANOTHER axis has d2(p) < d2(A) = a * a < fl(r * r) for every pair above (the largest fp32
# value whose square is below fl(r * r)): A is the candidate inside the 27 cells, p the nearer point two cells away
SLIVER_A = {0.2: 0x3e4ccccc, 0.3: 0x3e999999, 0.35: 0x3eb33332}      # 0.19999999, 0.29999998, 0.34999996
SLIVER_BLOCK = 300               # queries at separations r * (1 - k * 2^-22), k = 1 .. SLIVER_BLOCK


def sliver_case(radius, axis):
    """meta: pairs [(query, map index)]: a committed pair; nearer [(query, index of p, index of A)]; block: the block's query indices.
    A pair lies along `axis`; the other two coordinates are equal in q and p (so d^2 is the one product) and keep the pairs 2.5 apart"""
    r = F(radius)
    m, q, pairs, nearer = [np.full(3, ORIGIN, F)], [], [], []
    for k, (qb, pb) in enumerate(SLIVER[radius]):
        qv, pv = f32(qb), f32(pb)
        q.append([qv, 5.0 * k, 0.0])
        m.append([pv, 5.0 * k, 0.0])
        pairs.append((len(q) - 1, len(m) - 1))
        # the same pair again with A beside it, A before p for even k and behind it for odd k
        a = f32(SLIVER_A[radius])
        q.append([qv, 5.0 * k + 2.5, 0.0])
        both = [[qv, 5.0 * k + 2.5, a], [pv, 5.0 * k + 2.5, 0.0]]
        m += both if k % 2 == 0 else both[::-1]
        nearer.append((len(q) - 1, len(m) - (1 if k % 2 == 0 else 2), len(m) - (2 if k % 2 == 0 else 1)))
    block = []
    for k in range(1, SLIVER_BLOCK + 1):
        qv = F(np.float64(ORIGIN) + (100 + k) * np.float64(r))                       # a hair from a cell face of the edge r
        pv = F(np.float64(qv) - np.float64(r) * (1.0 - k * 2.0 ** -22))
        q.append([qv, 40.0 + 3.0 * k, 0.0])
        m.append([pv, 40.0 + 3.0 * k, 0.0])
        block.append(len(q) - 1)
    return _case(f"sliver radius {radius} axis {axis}", roll(m, axis), roll(q, axis), radius, pairs=pairs, nearer=nearer, block=block, axis=axis)


def sliver_cases():
    return [sliver_case(r, a) for r in SLIVER_RADII for a in range(3)]


# ---- thresholds: the radius edge and the acceptance edge ----------------------------------------------------------------------------------
# name -> (the threshold's bits, {which: (d2, s, t)}): a map point at query + (s, t, 0) has fp32 d^2 = fl(fl(s * s) + fl(t * t)) = d2
THRESHOLDS = {
    "r2 of radius 0.25": (0x3d800000, {"below": (0x3d7fffff, 0x3e7eb77f, 0x3cccccb2),     # 0.062499996  s 0.24874686  t 0.02499995
                                       "equal": (0x3d800000, 0x3e7eb77f, 0x3ccccccd),     # 0.0625       s 0.24874686  t 0.025
                                       "above": (0x3d800001, 0x3e7eb780, 0x3ccccccd)}),   # 0.06250001   s 0.24874687  t 0.025
    "r2 of radius 0.15": (0x3cb851ec, {"below": (0x3cb851eb, 0x3e18d47f, 0x3c75c2b4),     # 0.022499999  s 0.14924811  t 0.015000034
                                       "equal": (0x3cb851ec, 0x3e18d480, 0x3c75c271),     # 0.0225       s 0.14924812  t 0.014999972
                                       "above": (0x3cb851ed, 0x3e18d480, 0x3c75c290)}),   # 0.022500003  s 0.14924812  t 0.015000001
    "h2 of cell 0.2": (0x3d209460, {"below": (0x3d20945f, 0x3e49bc56, 0x3ca2339c),        # 0.039203998  s 0.1970075   t 0.0198
                                    "equal": (0x3d209460, 0x3e49bc57, 0x3ca2339c),        # 0.039204     s 0.19700752  t 0.0198
                                    "above": (0x3d209461, 0x3e49bc58, 0x3ca2336c)}),      # 0.039204005  s 0.19700754  t 0.01979991
    "h2 of cell 0.3": (0x3db4a6ed, {"below": (0x3db4a6ec, 0x3e974d41, 0x3cf34d6a),        # 0.088209     s 0.29551128  t 0.0297
                                    "equal": (0x3db4a6ed, 0x3e974d41, 0x3cf34d85),        # 0.08820901   s 0.29551128  t 0.02970005
                                    "above": (0x3db4a6ee, 0x3e974d42, 0x3cf34d6b)}),      # 0.08820902   s 0.2955113   t 0.029700002
}
# (threshold, radius of the call): h2 is (0.99f * cell) * (0.99f * cell) with cell = max(radius, 0.2f) in the unbounded search
EDGE_CALLS = [("r2 of radius 0.25", 0.25), ("r2 of radius 0.15", 0.15), ("h2 of cell 0.2", 0.15), ("h2 of cell 0.3", 0.3)]
_SIGNS = [(1, 1), (-1, 1), (1, -1), (-1, -1)]


def edge_case(threshold, radius, axis):
    """one query per (which, signs): the query has 0 in the two coordinates of the offset, so the map point's are s and t themselves.
    meta: edges [(query, map index, which)], threshold: the fp32 value"""
    m, q, edges = [], [], []
    for which, (_, sb, tb) in THRESHOLDS[threshold][1].items():
        for sx, sy in _SIGNS:
            z = 4.0 * len(q) + 1.0
            q.append([0.0, 0.0, z])
            m.append([sx * f32(sb), sy * f32(tb), z])
            edges.append((len(q) - 1, len(m) - 1, which))
    return _case(f"edge {threshold} axis {axis}", roll(m, axis), roll(q, axis), radius, edges=edges, threshold=f32(THRESHOLDS[threshold][0]),
                 d2={w: f32(v[0]) for w, v in THRESHOLDS[threshold][1].items()})


def edge_cases():
    return [edge_case(t, r, a) for t, r in EDGE_CALLS for a in range(3)]


def list_tie_case(axis, first):
    """a candidate inside the 27 cells (A) and a map point outside them (B) at the same d^2 = 0.0625 > h2 of cell 0.2, B with the lower
    index when first == "outside".  Cell edge 0.2 from the origin 0 (the first map point, on both forms): the query's coordinate 1.1875 is
    in cell 5, A's 0.9375 in cell 4, B's 1.4375 in cell 7.  meta: tie (query, (indices that tie))"""
    A, B = [0.9375, 1.125, 1.125], [1.4375, 1.125, 1.125]
    m = [[0.0, 0.0, 0.0]] + ([B, A] if first == "outside" else [A, B])
    return _case(f"list tie axis {axis} {first} first", roll(m, axis), roll([[1.1875, 1.125, 1.125]], axis), 0.15, tie=[(0, (1, 2))])


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------
def filler(n, at=20.0):
    """n distinct map points far from where the ties are set (a lattice from `at` upwards)"""
    i = np.arange(n)
    return np.stack([at + (i % 50) * 0.375, at + ((i // 50) % 50) * 0.4375, at + (i // 2500) * 0.5], axis=1).astype(F)


def tie_cases():
    """meta: tie [(query, (map indices at the minimal d^2))].  Cell edge 0.2 from the origin 0: [1.0, 1.2) is cell 5"""
    out = []
    o = [[0.0, 0.0, 0.0]]                                  # (keeps the host form's origin at 0)
    # inside one cell: 1.0625, 1.09375 and 1.125 are all in cell 5
    out.append(_case("tie inside one cell", o + [[1.0625, 1.1, 1.1], [1.125, 1.1, 1.1]], [[1.09375, 1.1, 1.1]], 0.15, tie=[(0, (1, 2))]))
    # across a face: 1.125 in cell 5, 1.25 in cell 6
    out.append(_case("tie across a cell face", o + [[1.25, 1.1, 1.1], [1.125, 1.1, 1.1]], [[1.1875, 1.1, 1.1]], 0.15, tie=[(0, (1, 2))]))
    # six neighbours at the same distance along the three axes
    c = np.array([1.09375, 1.09375, 1.09375])
    six = [c + d * np.eye(3)[a] for a in (2, 0, 1) for d in (0.0625, -0.0625)]
    out.append(_case("tie along three axes", o + six, [c], 0.15, tie=[(0, tuple(range(1, 7)))]))
    out.append(_case("tie along three axes, radius 0.3", o + six, [c], 0.3, tie=[(0, tuple(range(1, 7)))]))
    # duplicated map points with far-apart indices: under the query, near it, and far from it (the brute-force list)
    m = filler(3000)
    m[0] = 0.0
    m[7] = m[2900] = [1.1, 1.3, 1.5]
    m[450] = m[2047] = m[2048] = [3.0625, 3.0, 3.0]
    m[1234] = m[2999] = [-5.0, -5.0, 9.0]
    q = [[1.1, 1.3, 1.5], [1.15, 1.3, 1.5], [3.0, 3.0, 3.0], [-9.0, -5.0, 9.0], [-5.0, -5.0, 9.0]]
    out.append(_case("duplicated map points", m, q, 0.15,
                     tie=[(0, (7, 2900)), (1, (7, 2900)), (2, (450, 2047, 2048)), (3, (1234, 2999)), (4, (1234, 2999))]))
    return out


# ---- cell faces ---------------------------------------------------------------------------------------------------------------------------
def face_values(cell):
    """k * cell for k = -3 .. 3 as fp32 and one ulp on either side, with -0.0 (around 0 the neighbours are the smallest subnormals)"""
    v = []
    for k in range(-3, 4):
        x = F(k) * F(cell)
        v += [np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf))]
    return np.asarray(v + [F(-0.0)], F)


def face_case(radius, axis):
    """map points and queries on the faces of the grid of the device form (origin 0, cell max(radius, 0.2)) along one axis, mid-cell in the
    other two; a second row of queries a quarter cell off.  The two subnormal map points have a row of their own each, two and four
    cells below the others: beside +-0.0 their fp32 d^2 would underflow into a tie that float64 does not see.  meta: faces: the values"""
    cell = max(radius, 0.2)
    v = face_values(cell)
    mid = F(0.5 * cell)
    m = np.stack([v, np.full_like(v, mid), np.full_like(v, -mid)], axis=1)
    tiny = np.flatnonzero((v != 0) & (np.abs(v) < np.finfo(F).tiny))
    m[tiny, 2] -= F(2 * cell) * np.arange(1, len(tiny) + 1, dtype=F)
    row = np.stack([v, np.full_like(v, mid), np.full_like(v, -mid)], axis=1)              # (the subnormals as queries beside +-0.0)
    q = np.concatenate([row, m, m + np.array([0, 0.25 * cell, 0], F), m + np.array([0.5 * cell, 0, 0.25 * cell], F)])
    return _case(f"cell faces radius {radius} axis {axis}", roll(m, axis), roll(q, axis), radius, faces=v)


def face_cases():
    return [face_case(r, a) for r in (0.15, 0.3) for a in range(3)]


# ---- the hash -----------------------------------------------------------------------------------------------------------------------------
def buckets27(q, cell, mask, origin=0.0):
    """the buckets of the 27 cells around each query (csrc/scvod_grid.h: grid_cell, grid_bucket), [n, 27]"""
    c = np.floor((np.asarray(q, F) - F(origin)) * (F(1) / F(cell))).astype(np.int64)
    c = c[:, None, :] + np.asarray([[dx, dy, dz] for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])[None]
    return cell_bucket(c, mask)


def cell_bucket(c, mask):
    u = np.asarray(c, np.int64).astype(np.uint32)
    return (u[..., 0] * np.uint32(73856093) ^ u[..., 1] * np.uint32(19349663) ^ u[..., 2] * np.uint32(83492791)) & np.uint32(mask)


def aliased_case():
    """40 map points over 500 m: 1024 buckets for 2500^3 cells, so a query meets one bucket more than once among its 27"""
    i = np.arange(40)
    m = np.stack([(i * 97) % 500 - 250 + 0.1, (i * 57) % 500 - 250 + 0.3, (i * 31) % 500 - 250 + 0.7], axis=1).astype(F)
    near = m + (np.stack([frac(40), frac(40, start=0.3), frac(40, start=0.7)], axis=1) * 0.1 - 0.05).astype(F)
    mid = m + (np.stack([frac(40, start=0.5), frac(40, start=0.1), frac(40, start=0.9)], axis=1) * 0.4 - 0.2).astype(F)
    far = (np.stack([frac(500), frac(500, 0.7548776662), frac(500, 0.5698402910)], axis=1) * 500 - 250).astype(F)
    return _case("aliased buckets", m, np.concatenate([near, mid, far]), 0.15)


def one_bucket_case():
    """thirty occupied cells, far from each other, that all hash to ONE of the 1024 buckets (cell 0.2, origin 0); the cells are the first map
    point's (0, 0, 0) and 29 more.  meta: cells [30, 3]"""
    g = np.arange(-60, 60, dtype=np.int64)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[::7]
    same = cells[cell_bucket(cells, 1023) == cell_bucket(np.zeros(3), 1023)]
    same = np.concatenate([[[0, 0, 0]], same[(np.abs(same).max(axis=1) > 4)][:: max(1, (len(same) - 1) // 29)][:29]])
    m = ((same + 0.5) * 0.2).astype(F)                   # the cells' centres
    q = np.concatenate([m + (np.stack([frac(30), frac(30, start=0.3), frac(30, start=0.7)], axis=1) * 0.18 - 0.09).astype(F),
                        m + (np.stack([frac(30, start=0.2), frac(30, start=0.6), frac(30, start=0.4)], axis=1) - 0.5).astype(F),
                        (np.stack([frac(300), frac(300, 0.7548776662), frac(300, 0.5698402910)], axis=1) * 24 - 12).astype(F)])
    return _case("one bucket", m, q, 0.15, cells=same)


def wrap_case():
    """cells around (-10000, 7500, -4500) of the device form: the 32-bit products of the hash wrap many times over, on the negative side too.
    (In the host form the origin is the map's min corner and the indices are small.)"""
    i = np.arange(600)
    m = (np.array([-2000.0, 1500.0, -900.0]) + np.stack([(i % 10) * 0.21, ((i // 10) % 10) * 0.17, (i // 100) * 0.23], axis=1)).astype(F)
    q = np.concatenate([m[::3] + (np.stack([frac(200), frac(200, start=0.3), frac(200, start=0.7)], axis=1) * 0.2 - 0.1).astype(F),
                        m[:50] + np.array([0.0, 9.0, 0.0], F)])
    return _case("hash products wrap", m, q, 0.15)


def hash_cases():
    return [aliased_case(), one_bucket_case(), wrap_case()]


# ---- the brute-force list -----------------------------------------------------------------------------------------------------------------
LIST_MAP_SIZES = (1, 2047, 2048, 2049, 4097)
LIST_LENGTHS = (1, 255, 256, 257)


def list_case(n_map, n_query):
    """every query is 20 m or more from the map, so every one of them is on the list.  The map is a lattice of step 0.25 whose last point
    repeats the first; a query has y and z midway between lattice rows, so up to four map points (and the repeated one) tie for it"""
    i = np.arange(n_map)
    m = np.stack([(i % 16) * 0.25, ((i // 16) % 16) * 0.25, (i // 256) * 0.25], axis=1).astype(F)
    if n_map > 1:
        m[-1] = m[0]
    j = np.arange(n_query)
    q = np.stack([-20.0 - (j % 7), 0.125 + 0.25 * (j % 5) - 0.25 * (j % 2), 0.125 * (j % 3)], axis=1).astype(F)
    return _case(f"list n_map {n_map} n_query {n_query}", m, q, 0.15)


# ---- far coordinates ----------------------------------------------------------------------------------------------------------------------
# include/scvod.h: every coordinate within NN_MAX_CELLS cell edges of the grid origin (DESIGN.md A7 derives it from the fp32 operations of
# grid_cell).  The far case sits at no more than half of that
NN_MAX_CELLS = 25000
FAR_OFFSET = (2000.0, -2400.0, 1200.0)          # m; cell 0.2: 10000, 12000 and 6000 cells from the origin of the device form


def far_case():
    i = np.arange(1500)
    local = np.stack([(i % 12) * 0.45, ((i // 12) % 12) * 0.4, (i // 144) * 0.35], axis=1)
    m = (local + np.asarray(FAR_OFFSET)).astype(F)
    jit = np.stack([frac(700), frac(700, start=0.3), frac(700, start=0.7)], axis=1) * 0.3 - 0.15
    q = np.concatenate([(local[::3] + np.asarray(FAR_OFFSET)).astype(F), (local[:700] + jit + np.asarray(FAR_OFFSET)).astype(F),
                        (local[:40] + np.asarray(FAR_OFFSET) + [0.0, 0.0, 30.0]).astype(F)])
    return _case("far coordinates", m, q, 0.15)


def near_case(n_map, n_query, radius=0.15):
    """a plain cloud with near and far queries, for the call sequences"""
    i = np.arange(n_map)
    m = np.stack([(i % 20) * 0.31, ((i // 20) % 20) * 0.29, (i // 400) * 0.27], axis=1).astype(F)
    j = np.arange(n_query)
    q = m[(j * 7) % max(n_map, 1)] + (np.stack([frac(n_query), frac(n_query, start=0.3), frac(n_query, start=0.7)], axis=1) * 0.5 - 0.25).astype(F)
    q[::9] += F(40.0)
    return _case(f"plain {n_map} x {n_query} radius {radius}", m, q, radius)


def all_small_cases():
    out = sliver_cases() + edge_cases() + [list_tie_case(a, f) for a in range(3) for f in ("outside", "inside")]
    out += tie_cases() + face_cases() + hash_cases() + [list_case(n, k) for n in LIST_MAP_SIZES for k in LIST_LENGTHS] + [far_case()]
    return out
