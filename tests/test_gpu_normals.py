"""scvod_normals_device / scvod_map_points_normals on the device, through the C-ABI: the count, the ten int64 sums, the normal and the
curvature of every query against the CPU helper (tests/helpers/normals_ref.py: the library's nrm_* / normal_* functions over an
exhaustive neighbour loop).  The sums are integers and the finish is IEEE-basic operations in a stated order, so the comparison is on
the raw bits, with one exception: in a row with k >= min_neighbours, where a NaN can only come out of the eigen solver's 0/0, the sign
and payload of a NaN that both sides hold are not compared (IEEE leaves those of 0/0 open; the positions must coincide).  The NaN rows
of k < min_neighbours and of queries that are not finite are written explicitly and compared bit for bit.  Guard regions lie around every
output."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import map_ref as mr  # noqa: E402
import normals_ref as nr  # noqa: E402
import register_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 4
WIDTH = dict(normals=12, curvature=4, count=4, sums=80)  # bytes per query
DTYPE = dict(normals=F, curvature=F, count=np.int32, sums=np.int64)
CRAFTED = nr.crafted()
VARIANTS = (1, 2, 1 | 4, 2 | 4)  # NORMALS_QUERY_ORDER / NORMALS_ENTRY_ORDER, with NORMALS_WAVE_BLOCKS
EYE = np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
LEAF = 0.1


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return nr.build(tmp_path_factory.mktemp("normalsref"))


@pytest.fixture(scope="module")
def regref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("registerref"))


@pytest.fixture(scope="module")
def ctx(scvod):
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=8192, max_scans=4)
    yield c
    c.close()


def _dev(a, dtype=F):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


class Out:
    """the four outputs of one call with guard regions of GUARD rows before the first row and behind row n"""

    def __init__(self, n):
        import torch
        self.n = n
        self.buf = {k: torch.full(((n + 2 * GUARD) * w,), 0xA5, dtype=torch.uint8, device="cuda") for k, w in WIDTH.items()}

    def ptr(self, k):
        assert self.buf[k].data_ptr() % 8 == 0
        return C.c_void_p(self.buf[k].data_ptr() + GUARD * WIDTH[k])

    def host(self):
        out = {}
        for k, w in WIDTH.items():
            a = self.buf[k].cpu().numpy()
            assert (a[:GUARD * w] == 0xA5).all(), f"{k} was written before the first row"
            assert (a[(GUARD + self.n) * w:] == 0xA5).all(), f"{k} was written behind n_query"
            out[k] = a[GUARD * w:(GUARD + self.n) * w].copy().view(DTYPE[k]).reshape({"normals": (self.n, 3), "sums": (self.n, 10)}.get(k, (self.n,)))
        return out


def _run(scvod, ctx, cloud, query=None, radius=0.5, min_neighbours=5, seg=None, view=None, stream=None, sync=True):
    """the raw call; (outputs on the host, stats) -- or the Out itself with sync False"""
    import torch
    cloud = np.ascontiguousarray(cloud, F)
    d_cloud = _dev(cloud)
    d_query = None if query is None else _dev(query if len(query) else np.zeros((1, query.shape[1]), F))  # (NULL would mean the self form)
    n = len(cloud) if query is None else len(query)
    out = Out(n)
    torch.cuda.synchronize()  # the guard fill runs on torch's stream, the call on the ctx's or the caller's
    p = scvod.normal_params_default(radius=radius, min_neighbours=min_neighbours)
    seg = None if seg is None else np.ascontiguousarray(seg, np.int32)
    view = None if view is None else np.ascontiguousarray(view, F)
    rc = ctx.lib.scvod_normals_device(ctx.h, C.c_void_p(d_cloud.data_ptr()) if len(cloud) else None, cloud.shape[1], len(cloud),
                                      None if d_query is None else C.c_void_p(d_query.data_ptr()), 0 if query is None else query.shape[1], n,
                                      None if seg is None else seg.ctypes.data_as(C.c_void_p), None if view is None else view.ctypes.data_as(C.c_void_p),
                                      0 if seg is None else len(seg) - 1, C.byref(p), out.ptr("normals"), out.ptr("curvature"), out.ptr("count"),
                                      out.ptr("sums"), C.c_void_p(stream) if stream else None)
    assert rc == 0, ctx.lib.scvod_last_error(ctx.h)
    if not sync:
        out.keep = (d_cloud, d_query)
        return out
    stats = ctx.normals_stats()
    return out.host(), stats


def _same_bits(a, b, what="", strict=None):
    """equal bits wherever not both are NaN, NaNs at the same places; rows of `strict` (a mask): every bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if strict is not None:
        assert a[strict].tobytes() == b[strict].tobytes(), (what, "rows with explicit NaNs differ in bits")
    if a.dtype == F:
        na, nb = np.isnan(a), np.isnan(b)
        assert np.array_equal(na, nb), (what, "NaNs at other places", np.flatnonzero(na != nb)[:8])
        assert np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~na]), (what, np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)) & ~na)[:8])
    else:
        assert np.array_equal(a, b), (what, np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[:8])


def _same(dev, hlp, what="", min_neighbours=5):
    """min_neighbours: the call's (rows below it hold explicit NaNs: every bit is compared)"""
    strict = hlp["count"] < min_neighbours
    for k in ("count", "sums", "normals", "curvature"):
        _same_bits(dev[k], hlp[k], f"{what}: {k}", strict)


def _stats_equal(stats, hlp):
    assert stats == hlp["stats"], (stats, hlp["stats"])


# ---------------------------------------------------------------- the crafted clouds against the helper, under every arm and geometry

@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_cloud_equals_the_helper(scvod, ctx, ref, name):
    c = CRAFTED[name]
    h = nr.run(ref, c["cloud"], c["query"], c["radius"], c["min_neighbours"])
    d, stats = _run(scvod, ctx, c["cloud"], c["query"], c["radius"], c["min_neighbours"])
    _same(d, h, name, c["min_neighbours"])
    _stats_equal(stats, h)
    try:
        for v in VARIANTS:
            ctx.set_normals_variant(v)
            dv, sv = _run(scvod, ctx, c["cloud"], c["query"], c["radius"], c["min_neighbours"])
            _same(dv, h, f"{name}, variant {v}", c["min_neighbours"])
            _stats_equal(sv, h)
    finally:
        ctx.set_normals_variant(0)


def test_the_alias_case_counts_every_point_once(scvod, ctx):
    """radius 0.196 (edge 0.2) and 1024 buckets: the cells (-1,-1,1) and (1,1,1) around the query's cell (0,0,1) share a bucket, and so do
    (1,-1,1) and (-1,1,1); k and the sums are those of the numpy statement, not double"""
    for name in ("alias", "alias_self"):
        c = CRAFTED[name]
        d, _ = _run(scvod, ctx, c["cloud"], c["query"], c["radius"], c["min_neighbours"])
        want = nr.sums_numpy(c["cloud"], c["query"], c["radius"])
        assert [[int(v) for v in row] for row in d["sums"]] == want
        assert d["count"].tolist() == [w[0] for w in want]
    assert d["count"].tolist() == [2, 2, 2, 2, 5]


def test_the_radius_edge(scvod, ctx):
    c = CRAFTED["radius_edge"]
    assert c["cloud"][0].tolist() == [0.5, 0, 0] and c["cloud"][1, 0] == np.nextafter(F(0.5), F(0)) and c["radius"] == 0.5
    d, _ = _run(scvod, ctx, c["cloud"], c["query"], 0.5)
    assert d["count"].tolist() == [4]  # the float below the radius, two points at 0.25 and one near the origin; +-0.5 are out
    alone, _ = _run(scvod, ctx, c["cloud"][:1], c["query"], 0.5)
    inside, _ = _run(scvod, ctx, c["cloud"][1:2], c["query"], 0.5)
    assert alone["count"].tolist() == [0] and inside["count"].tolist() == [1]


def test_empty_clouds_and_queries(scvod, ctx, ref):
    none = np.zeros((0, 3), F)
    q = np.asarray([[0, 0, 0], [1, 2, 3], [np.nan, 0, 0]], F)
    d, stats = _run(scvod, ctx, none)
    assert len(d["count"]) == 0 and stats["queries"] == 0 and stats["sum_k"] == 0
    d, stats = _run(scvod, ctx, none, q)
    _same(d, nr.run(ref, none, q), "no cloud")
    assert np.isnan(d["normals"]).all() and (d["count"] == 0).all() and (d["sums"] == 0).all()
    assert (stats["queries"], stats["below_min"], stats["nonfinite_queries"], stats["finite"]) == (3, 2, 1, 0)
    d, stats = _run(scvod, ctx, CRAFTED["groups"]["cloud"], none)
    assert len(d["count"]) == 0 and stats["queries"] == 0 and stats["cloud_left_out"] == 0


# ---------------------------------------------------------------- order, strides, segments

def test_point_order_does_not_matter(scvod, ctx):
    rng = np.random.default_rng(5)
    cloud = np.concatenate([CRAFTED["groups"]["cloud"], CRAFTED["faces"]["cloud"], CRAFTED["dirty"]["cloud"][:, :3]])
    base, s0 = _run(scvod, ctx, cloud, None, 0.3, 4)
    o = rng.permutation(len(cloud))
    try:
        for v in (0,) + VARIANTS:
            ctx.set_normals_variant(v)
            d, s = _run(scvod, ctx, cloud[o], None, 0.3, 4)
            back = {k: np.empty_like(a) for k, a in d.items()}
            for k in d:
                back[k][o] = d[k]
            _same(back, base, f"shuffled, variant {v}", 4)
            assert s == s0
    finally:
        ctx.set_normals_variant(0)
    assert s0["finite"] > 500 and s0["below_min"] >= 2 and s0["nonfinite_queries"] > 20


def test_separate_queries_and_strides(scvod, ctx, ref):
    """a query cloud of stride 3 against a cloud of stride 4; the cloud's own points as stride-3 queries give the self form's bits"""
    c = CRAFTED["dirty_queries"]
    assert c["cloud"].shape[1] == 4 and c["query"].shape[1] == 3
    d, stats = _run(scvod, ctx, c["cloud"], c["query"], 0.2)
    h = nr.run(ref, c["cloud"], c["query"], 0.2)
    _same(d, h, "stride 3 on stride 4")
    _stats_equal(stats, h)
    self4, _ = _run(scvod, ctx, c["cloud"], None, 0.2)
    as_q3, _ = _run(scvod, ctx, c["cloud"], c["cloud"][:, :3].copy(), 0.2)
    cloud3, _ = _run(scvod, ctx, c["cloud"][:, :3].copy(), None, 0.2)
    q4 = np.concatenate([c["query"], np.full((len(c["query"]), 1), 7, F)], 1)
    as_q4, _ = _run(scvod, ctx, c["cloud"][:, :3].copy(), q4, 0.2)
    _same(as_q3, self4, "the cloud as its own stride-3 queries")
    _same(cloud3, self4, "stride 3")
    _same(as_q4, d, "stride-4 queries on a stride-3 cloud")
    finite = nr.usable(c["cloud"])
    clean, _ = _run(scvod, ctx, c["cloud"][finite], None, 0.2)
    _same({k: v[finite] for k, v in self4.items()}, clean, "the neighbours of finite queries do not see the points left out")


def test_three_segments_with_viewpoints(scvod, ctx, ref):
    cloud, n = nr.plane_cloud(2)
    seg = [0, 200, 200, 450, len(cloud)]  # (one of the four is empty)
    view = np.asarray([30 * n, -30 * n, -30 * n + [1, 0, 0], 30 * n], F)
    d, _ = _run(scvod, ctx, cloud, None, 0.5, 5, seg=seg, view=view)
    _same(d, nr.run(ref, cloud, None, 0.5, 5, seg=seg, view=view), "segments")
    dots = d["normals"].astype(np.float64) @ n
    assert (dots[:200] > 0.9).all() and (dots[200:450] < -0.9).all() and (dots[450:] > 0.9).all()
    free, _ = _run(scvod, ctx, cloud, None, 0.5, 5)
    _same(free, nr.run(ref, cloud, None, 0.5, 5), "n_segments 0 leaves the solver's sign")
    assert np.array_equal(np.abs(free["normals"]), np.abs(d["normals"])) and free["sums"].tobytes() == d["sums"].tobytes()
    q = cloud[::7] + F(0.01)
    segq = [0, 30, len(q)]
    dq, _ = _run(scvod, ctx, cloud, q, 0.5, 5, seg=segq, view=view[:2])
    _same(dq, nr.run(ref, cloud, q, 0.5, 5, seg=segq, view=view[:2]), "segments of separate queries")


def test_the_python_wrapper(scvod, ctx, ref):
    c = CRAFTED["dirty_queries"]
    seg, view = [0, 40, len(c["query"])], [[0, 0, 9], [0, 0, -9]]
    h = nr.run(ref, c["cloud"], c["query"], 0.2, 5, seg=seg, view=view)
    d = ctx.normals_device(_dev(c["cloud"]), _dev(c["query"]), params=scvod.normal_params_default(radius=0.2), seg_offsets=seg, viewpoints=view,
                           want=("curvature", "count", "sums"))
    _same({k: v.cpu().numpy() for k, v in d.items()}, h, "Ctx.normals_device")
    _stats_equal(ctx.normals_stats(), h)
    only = ctx.normals_device(_dev(c["cloud"]), params=scvod.normal_params_default(radius=0.2), want=())
    assert sorted(only) == ["normals"]
    hs = nr.run(ref, c["cloud"], None, 0.2, 5)
    _same_bits(only["normals"].cpu().numpy(), hs["normals"], "the self form, normals only", hs["count"] < 5)
    none = ctx.normals_device(_dev(c["cloud"]), _dev(np.zeros((0, 3), F)), want=("count",))  # (an empty query cloud is not the self form)
    assert len(none["normals"]) == 0 and len(none["count"]) == 0 and ctx.normals_stats()["queries"] == 0


def test_the_calls_refuse_and_write_nothing(scvod):
    fresh = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=4096, max_scans=1)
    cloud = _dev(CRAFTED["groups"]["cloud"])
    n = len(cloud)

    def call(p, stride=3, seg=None, view=None, n_seg=0):
        out = Out(n)
        rc = fresh.lib.scvod_normals_device(fresh.h, C.c_void_p(cloud.data_ptr()), stride, n, None, 0, n, seg, view, n_seg, C.byref(p), out.ptr("normals"),
                                            out.ptr("curvature"), out.ptr("count"), out.ptr("sums"), None)
        return rc, all((a == 0xA5).all() for a in (t.cpu().numpy() for t in out.buf.values()))

    d = scvod.normal_params_default
    for bad in (dict(radius=0.0), dict(radius=4.5), dict(min_neighbours=2), dict(flags=2), dict(reserved=1)):
        assert call(d(**bad)) == (-1, True), bad
    assert call(d(), stride=5) == (-1, True)
    view = np.zeros(3, F)
    assert call(d(), view=view.ctypes.data_as(C.c_void_p), n_seg=1) == (-1, True) and b"without segment offsets" in fresh.lib.scvod_last_error(fresh.h)
    seg = np.asarray([0, n - 1], np.int32)
    assert call(d(), seg=seg.ctypes.data_as(C.c_void_p), view=view.ctypes.data_as(C.c_void_p), n_seg=1) == (-1, True)
    assert fresh.normals_scratch_bytes() == 0
    assert fresh.lib.scvod_normals_stats(fresh.h, (C.c_int64 * 8)()) == -5  # SCVOD_ERR_STATE: no call ran
    fresh.close()


# ---------------------------------------------------------------- state

def test_a_normals_call_moves_nothing_else(scvod, ref):
    import torch
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=4096, max_scans=2)
    xyzi, world, _ = rr.corner_cloud()
    d = torch.from_numpy(xyzi).cuda()
    c.batch_process(d, np.asarray([0, 700, len(xyzi)], np.int32))
    c.register_device(d, [0, len(xyzi)], torch.from_numpy(world).cuda())
    before = (c.arena_bytes(), c.register_scratch_bytes(), c.evaluate_scratch_bytes(), c.batch_objects_scratch_bytes())
    assert c.normals_scratch_bytes() == 0  # nothing is allocated before the first call
    small, big = CRAFTED["k4_k5"], CRAFTED["groups"]
    _run(scvod, c, small["cloud"])
    s1 = c.normals_scratch_bytes()
    _run(scvod, c, big["cloud"])
    s2 = c.normals_scratch_bytes()
    _run(scvod, c, small["cloud"])
    assert 0 < s1 <= s2 == c.normals_scratch_bytes()  # grow-only
    assert before == (c.arena_bytes(), c.register_scratch_bytes(), c.evaluate_scratch_bytes(), c.batch_objects_scratch_bytes())
    # two calls on two streams of one ctx give the solo results
    a, b = CRAFTED["groups"], CRAFTED["dirty"]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    oa = _run(scvod, c, a["cloud"], None, a["radius"], a["min_neighbours"], stream=sa.cuda_stream, sync=False)
    ob = _run(scvod, c, b["cloud"], None, b["radius"], b["min_neighbours"], stream=sb.cuda_stream, sync=False)
    stats_b = c.normals_stats()
    torch.cuda.synchronize()
    ha, hb = nr.run(ref, a["cloud"], None, a["radius"], a["min_neighbours"]), nr.run(ref, b["cloud"], None, b["radius"], b["min_neighbours"])
    _same(oa.host(), ha, "stream a", a["min_neighbours"])
    _same(ob.host(), hb, "stream b", b["min_neighbours"])
    _stats_equal(stats_b, hb)
    c.close()


# ---------------------------------------------------------------- the map form

def _plain_map(scvod, world):
    w4 = np.concatenate([np.asarray(world, F), np.ones((len(world), 1), F)], 1)
    keys, vals, ok = mr.encode_points(EYE, w4, LEAF)
    assert ok.all()
    m = scvod.StaticMap(1 << 13, leaf=LEAF)
    m.merge(mr.to_device(*mr.reduce_records(keys, vals)))
    return m


def _labelled_map(scvod, world, labels):
    m = scvod.StaticMap(1 << 13, leaf=LEAF, kind=scvod.MAP_KIND_LABELLED)
    w4 = np.concatenate([np.asarray(world, F), np.ones((len(world), 1), F)], 1)
    m.accumulate_labelled(_dev(w4), _dev(labels, np.uint8), [0, len(w4)], None, None)
    return m


def _by_point(xyzi):
    """a canonical order of map rows: a cell has one row, so the rows' own bytes sort them (as the record key would)"""
    return np.lexsort(np.ascontiguousarray(xyzi, F).view(np.uint32).T[::-1])


@pytest.mark.parametrize("kind", ["plain", "labelled"])
def test_map_points_with_normals(scvod, ctx, ref, kind):
    _, world, _ = rr.corner_cloud()
    labels = np.where(np.arange(len(world)) < 484, 5, 3).astype(np.uint8)
    m = _plain_map(scvod, world) if kind == "plain" else _labelled_map(scvod, world, labels)
    before = (m.count(), m.scratch_bytes(), m.query_scratch_bytes(), m.filter_scratch_bytes(), m.register_scratch_bytes(), *mr.sorted_records(m))
    p = scvod.normal_params_default(radius=0.5)
    for select in ((None,) if kind == "plain" else (None, [3])):
        if kind == "plain":
            want_xyzi, want_lab = m.points()[0].cpu().numpy(), None
        else:
            want_xyzi, want_lab, _ = (t.cpu().numpy() for t in m.points_labelled(select))
        got = {k: v.cpu().numpy() for k, v in m.points_normals(ctx, params=p, select=select, with_labels=kind == "labelled").items()}
        assert len(got["xyzi"]) == len(want_xyzi) == (968 if select else 1452)
        o, w = _by_point(got["xyzi"]), _by_point(want_xyzi)
        assert got["xyzi"][o].tobytes() == want_xyzi[w].tobytes()
        assert got["xyz"].tobytes() == np.ascontiguousarray(got["xyzi"][:, :3]).tobytes()
        if want_lab is not None:
            assert np.array_equal(got["labels"][o], want_lab[w])
        h = nr.run(ref, got["xyzi"], None, 0.5, 5)
        _same_bits(got["normals"], h["normals"], f"{kind} {select}: normals", h["count"] < 5)
        _same_bits(got["curvature"], h["curvature"], f"{kind} {select}: curvature", h["count"] < 5)
        _stats_equal(ctx.normals_stats(), h)
        assert h["stats"]["finite"] > 0.9 * len(want_xyzi)
    # SCVOD_ERR_CAPACITY writes nothing at or behind cap, and no normal at all
    import torch
    n, cap = before[0], before[0] - 5
    bufs = [torch.full((n * w,), 0xA5, dtype=torch.uint8, device="cuda") for w in (16, 12, 4)]
    n_out = C.c_int64()
    rc = m.lib.scvod_map_points_normals(ctx.h, m.h, C.byref(p), None, *(C.c_void_p(b.data_ptr()) for b in bufs[:1]), None,
                                        *(C.c_void_p(b.data_ptr()) for b in bufs[1:]), cap, C.byref(n_out), None)
    assert rc == -4 and n_out.value == n
    torch.cuda.synchronize()
    xyzi_b, nrm_b, cur_b = (b.cpu().numpy() for b in bufs)
    assert (xyzi_b[cap * 16:] == 0xA5).all() and (nrm_b == 0xA5).all() and (cur_b == 0xA5).all()
    if kind == "plain":  # a select table (or label bytes) on a plain map is refused
        sel = np.ones(256, np.uint8)
        rc = m.lib.scvod_map_points_normals(ctx.h, m.h, C.byref(p), sel.ctypes.data_as(C.c_void_p), C.c_void_p(bufs[0].data_ptr()), None,
                                            C.c_void_p(bufs[1].data_ptr()), None, n, C.byref(n_out), None)
        assert rc == -1 and b"select table" in ctx.lib.scvod_last_error(ctx.h)
    after = (m.count(), m.scratch_bytes(), m.query_scratch_bytes(), m.filter_scratch_bytes(), m.register_scratch_bytes(), *mr.sorted_records(m))
    assert before[:5] == after[:5] and np.array_equal(before[5], after[5]) and np.array_equal(before[6], after[6])
    m.close()


def test_map_normals_feed_plane_registration(scvod, ctx, ref, regref):
    """clean -> map -> the map's points with normals -> point-to-plane refinement, without leaving the device: the corner cloud, the start
    off by 0.003 rad and 0.04 m"""
    import torch
    xyzi, world, _ = rr.corner_cloud()
    m = _plain_map(scvod, world)
    tgt = m.points_normals(ctx, params=scvod.normal_params_default(radius=0.5))
    p6 = scvod.pose_from_matrix(rr.start_matrix(0.003, 0.04))
    T0 = scvod.pose_matrix(p6)
    q = scvod.register_params_default(mode=scvod.REG_PLANE, max_dist=0.2)
    res = scvod.register_result(*ctx.register_device(torch.from_numpy(xyzi).cuda(), [0, len(xyzi)], tgt["xyz"], p6[None, :], d_tgt_normals=tgt["normals"],
                                                     params=q))
    h = rr.run(regref, xyzi, [0, len(xyzi)], T0, tgt["xyz"].cpu().numpy(), rr.params(mode=rr.PLANE, max_dist=0.2), tgt_nrm=tgt["normals"].cpu().numpy())
    assert res["matrices"].reshape(-1, 12).tobytes() == h["pose"].tobytes() and res["records"].tobytes() == h["records"].tobytes()
    assert res["records"]["status"][0] == scvod.REG_CONVERGED
    M = rr.pose_matrix64(rr.TRUE_T, rr.TRUE_RV)
    e0 = float(np.linalg.norm(T0.reshape(3, 4)[:, 3].astype(np.float64) - M[:, 3]))
    e1 = float(np.linalg.norm(res["matrices"][0][:, 3] - M[:, 3]))
    print(f"translation error {e0:.4e} m at the start, {e1:.4e} m reached in {res['records']['iterations'][0]} iterations, "
          f"{res['records']['n_corr'][0]} correspondences, {res['records']['skip_normal'][0]} normals skipped")
    assert 0.039 < e0 < 0.041 and e1 < 0.04
    m.close()
