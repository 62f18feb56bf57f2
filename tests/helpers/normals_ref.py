"""Reference statements of the surface normals (include/scvod.h: scvod_normals_device) -- test infrastructure only.

`run` is the C++ loop of normals_ref.cpp: the library's nrm_* / normal_* functions (scvod_math.h) over the queries with an EXHAUSTIVE
neighbour loop, no grid.  `sums_numpy` beside it does NOT read that header and states the integers alone: numpy's fp32 array operations
for e = p - q and d = (ex*ex + ey*ey) + ez*ez (one rounding per operation), the terms as fp64 products times 2^30 through numpy.rint
(ties to even), summed as Python ints (int64 inside a chunk of 4096 neighbours, where |sum| < 2^12 * 2^35 cannot overflow).
`crafted` are the clouds both test files use."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F = np.float32
WORDS = 10
STATS = ("queries", "finite", "below_min", "nonfinite_queries", "cloud_left_out", "largest_k", "sum_k", "zero")
MAX_COORD = 1.0e6


def build(out_dir):
    src = os.path.join(ROOT, "tests", "helpers", "normals_ref.cpp")
    so = os.path.join(str(out_dir), "libnormalsref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.normals_ref.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, vp]
    lib.normals_ref.restype = None
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run(lib, cloud, query=None, radius=0.5, min_neighbours=5, seg=None, view=None):
    """dict(normals [n, 3] f32, curvature [n] f32, count [n] i32, sums [n, 10] i64, stats dict) of the C++ loop.  cloud [m, 3 or 4],
    query [n, 3 or 4] or None (the queries are the cloud)"""
    cloud = np.ascontiguousarray(cloud, F)
    cloud = cloud.reshape(-1, cloud.shape[-1] if cloud.ndim == 2 else 3)
    if query is not None:
        query = np.ascontiguousarray(query, F)
    n = len(cloud) if query is None else len(query)
    seg = None if seg is None else np.ascontiguousarray(seg, np.int32)
    view = None if view is None else np.ascontiguousarray(view, F).reshape(-1, 3)
    n_seg = 0 if seg is None else len(seg) - 1
    nrm = np.zeros((max(n, 1), 3), F)
    cur = np.zeros(max(n, 1), F)
    cnt = np.zeros(max(n, 1), np.int32)
    sums = np.zeros((max(n, 1), WORDS), np.int64)
    stats = np.zeros(8, np.int64)
    lib.normals_ref(_ptr(cloud), cloud.shape[1], len(cloud), _ptr(query), 0 if query is None else query.shape[1], n, _ptr(seg), _ptr(view), n_seg,
                    float(radius), int(min_neighbours), _ptr(nrm), _ptr(cur), _ptr(cnt), _ptr(sums), _ptr(stats))
    return dict(normals=nrm[:n], curvature=cur[:n], count=cnt[:n], sums=sums[:n], stats=dict(zip(STATS, (int(v) for v in stats))))


# ---- the numpy statement of the integers ------------------------------------------------------------------------------------------
def usable(xyz):
    with np.errstate(all="ignore"):
        return (np.abs(xyz[:, :3]) <= F(MAX_COORD)).all(axis=1)  # (NaN fails the comparison, an infinity exceeds the bound)


def sums_numpy(cloud, query=None, radius=0.5, pick=None):
    """[n][10] Python ints (a list of lists): k, the sums of e_a, the sums of e_a e_b (xx, xy, xz, yy, yz, zz); zeros for a query that
    is not usable.  pick: the query indices to state (None: all)"""
    cloud = np.asarray(cloud, F)[:, :3]
    q_all = cloud if query is None else np.asarray(query, F)[:, :3]
    pick = range(len(q_all)) if pick is None else pick
    P = cloud[usable(cloud)]
    r2 = F(radius) * F(radius)
    ok_q = usable(q_all)
    out = []
    for i in pick:
        w = [0] * WORDS
        if ok_q[i]:
            for c0 in range(0, len(P), 4096):
                E = P[c0:c0 + 4096] - q_all[i][None, :]  # fp32, one subtraction per component
                ex, ey, ez = E[:, 0], E[:, 1], E[:, 2]
                d = (ex * ex + ey * ey) + ez * ez
                E = E[d < r2].astype(np.float64)
                x, y, z = E[:, 0], E[:, 1], E[:, 2]
                w[0] += int(len(E))
                for j, term in enumerate((x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
                    w[1 + j] += int(np.rint(term * 1073741824.0).astype(np.int64).sum())
        out.append(w)
    return out


# ---- the crafted clouds -----------------------------------------------------------------------------------------------------------
ALIAS_QUERY = (0.1, 0.1, 0.3)
ALIAS_POINTS = ((-0.01, -0.01, 0.3), (0.21, 0.21, 0.3), (0.21, -0.01, 0.3), (-0.01, 0.21, 0.3))


def crafted():
    """name -> dict(cloud [m, 3 or 4] f32, query [n, 3] f32 or None, radius, min_neighbours, numpy_pick)"""
    rng = np.random.default_rng(2024)
    out = {}

    def add(name, cloud, query=None, radius=0.5, min_neighbours=5, numpy_pick=None):
        out[name] = dict(cloud=np.ascontiguousarray(cloud, F), query=None if query is None else np.ascontiguousarray(query, F), radius=radius,
                         min_neighbours=min_neighbours, numpy_pick=numpy_pick)

    tri = np.asarray([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0.02]], F)
    for n in (1, 2, 3):
        add(f"points{n}", tri[:n], min_neighbours=3)
    # k at min_neighbours - 1 and at min_neighbours: a group of four and a group of five, 20 m apart
    g = rng.uniform(-0.1, 0.1, (9, 3))
    g[4:, 0] += 20.0
    add("k4_k5", g)
    # the radius edge: the query at the origin, a point at exactly the radius (out) and the float below it (in)
    edge = np.asarray([[0.5, 0, 0], [np.nextafter(F(0.5), F(0)), 0, 0], [0, 0.25, 0], [0, 0, -0.25], [0.1, 0.1, 0.1], [-0.5, 0, 0]], F)
    add("radius_edge", edge, query=np.zeros((1, 3), F))
    # the alias case: at 1024 buckets the cells (-1,-1,dz) and (1,1,dz) around (0,0,1) share a bucket, and so do (1,-1,dz) and (-1,1,dz)
    add("alias", np.asarray(ALIAS_POINTS + (ALIAS_QUERY,), F), query=np.asarray([ALIAS_QUERY], F), radius=0.196, min_neighbours=3)
    add("alias_self", np.asarray(ALIAS_POINTS + (ALIAS_QUERY,), F), radius=0.196, min_neighbours=3)
    # cell faces and negative coordinates (edge 0.2: the lattice sits on the faces), a jittered copy, and queries with 27 empty cells
    k = np.arange(-3, 4)
    lat = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3).astype(F) * F(0.2)
    jit = lat + rng.uniform(-0.05, 0.05, lat.shape).astype(F)
    faces = np.concatenate([lat, jit, np.asarray([[50, 50, 50], [-70, 3, 0.5]], F)])
    add("faces", faces, radius=0.196, min_neighbours=4)
    add("faces_queries", np.concatenate([lat, jit]), query=np.concatenate([lat[::3], -lat[::5] + F(0.1), np.asarray([[50, 50, 50], [-9, -9, -9]], F)]),
        radius=0.196, min_neighbours=4)
    # neighbourhoods of 63, 64, 65 and 129 points: groups 10 m apart, each inside a ball of 0.2 m
    groups = [rng.uniform(-0.11, 0.11, (n, 3)) + [10.0 * i, -3.0, 1.0] for i, n in enumerate((63, 64, 65, 129))]
    add("groups", np.concatenate(groups))
    # 5000 points inside one radius at radius 4, offsets up to about 3.9: the fixed-point range (numpy states every 8th query)
    v = rng.normal(size=(5000, 3))
    v = v / np.linalg.norm(v, axis=1)[:, None] * (1.95 * rng.uniform(0.2, 1.0, 5000) ** (1 / 3))[:, None]
    v[:2500] = v[:2500] / np.linalg.norm(v[:2500], axis=1)[:, None] * 1.95  # half of them on the sphere: offsets near the diameter
    add("blob", v + [100.0, -40.0, 2.0], radius=4.0, numpy_pick=range(0, 5000, 8))
    # NaN, infinite and far coordinates in the cloud and in the queries, stride 4
    dirty = np.concatenate([rng.uniform(-0.3, 0.3, (400, 3)), np.ones((400, 1))], 1).astype(F)
    dirty[5::40, 0] = np.nan
    dirty[7::50, 1] = np.inf
    dirty[9::60, 2] = -np.inf
    dirty[11::70, 0] = 2e6
    dirty[13::80, 2] = -2e6
    add("dirty", dirty, radius=0.2)
    dq = rng.uniform(-0.3, 0.3, (90, 3)).astype(F)
    dq[3::10, 1] = np.nan
    dq[4::15, 0] = np.inf
    dq[6::20, 2] = 2e6
    add("dirty_queries", dirty, query=dq, radius=0.2)
    return out


def plane_cloud(tilt):
    """a lattice plane at one of three tilts plus fp32 noise of 1 cm on every coordinate: (cloud [625, 3] f32, the plane's unit normal
    in fp64).  Lattice point (i, j) is (8 i, 8 j, a i + b j) / 64: every coordinate a multiple of 2^-6."""
    rng = np.random.default_rng(77 + tilt)
    a, b = ((0, 0), (2, 0), (4, -2))[tilt]
    i, j = (c.reshape(-1) for c in np.meshgrid(np.arange(-12, 13), np.arange(-12, 13), indexing="ij"))
    lattice = (np.stack([8 * i, 8 * j, a * i + b * j], 1) / 64.0).astype(F)
    p = lattice + rng.normal(scale=0.01, size=lattice.shape).astype(F)
    n = np.asarray([-a / 8.0, -b / 8.0, 1.0])
    return p, n / np.linalg.norm(n)
