"""scvod_map_filter / scvod_batch_map_filter (csrc/scvod_mapfilter.hip) against the numpy statement tests/helpers/map_filter_ref.py, byte
for byte: tile and wave edges of the per-scan partition, OUT points, the nearest cases of the query, more scans than one launch takes,
poses and stream order, the object vote on the crafted object batch, the votes' capacity, error and state cases, and that the call
moves nothing else.  Every call goes through the C ABI into buffers with a guard region behind them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import map_filter_ref as mf  # noqa: E402
import map_query_ref as mq  # noqa: E402
import map_ref as mr  # noqa: E402
from test_gpu_map_query import _case_map, _merged, batch  # noqa: E402,F401  (the nearest cases' maps, the four-scan batch fixture)
from test_gpu_map_table import _scan  # noqa: E402
from test_gpu_object_shapes import _crafted, _prepared  # noqa: E402
from test_gpu_object_truth import Tru  # noqa: E402
from test_gpu_objects import NO_TRACK, Tab, _full  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, STATE, ERR_CAPACITY = -1, -5, -4
GUARD = 64
F = np.float32
NAMES = ("result", "side", "order", "bounds", "xyzi", "payload", "votes")
PARTITION = ("result", "side", "order", "bounds", "xyzi", "payload")
FILL = 0xA5


def _header_tile():
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scvod.h")).read()
    return int(re.search(r"#define\s+SCVOD_MAP_FILTER_TILE\s+(\d+)", hdr).group(1))


T = _header_tile()


class Out:
    """guard-backed, sentinel-filled outputs of one filter call: n points, n_scans scans, cap vote records"""
    ROW = dict(result=1, side=1, order=4, bounds=8, xyzi=16, payload=4, votes=32)

    def __init__(self, n, n_scans, cap=0, want=NAMES):
        import torch
        self.rows = dict(result=n, side=n, order=n, bounds=n_scans, xyzi=n, payload=n, votes=cap)
        self.want = tuple(want)
        # (every buffer is allocated, asked for or not: the ones not asked for must stay as they are too)
        self.t = {k: torch.full(((self.rows[k] + GUARD) * self.ROW[k],), FILL, dtype=torch.uint8, device="cuda") for k in NAMES}

    def ptr(self, k):
        return C.c_void_p(self.t[k].data_ptr()) if k in self.want else None

    def host(self):
        """the outputs asked for as numpy arrays; asserts every guard region and every buffer that was not asked for"""
        import torch
        torch.cuda.synchronize()
        dt = dict(result=np.uint8, side=np.uint8, order=np.int32, bounds=np.int32, xyzi=np.uint32, payload=np.uint32, votes=mf.OBJECT_DTYPE)
        r = {}
        for k in NAMES:
            raw = self.t[k].cpu().numpy()
            used = self.rows[k] * self.ROW[k] if k in self.want else 0
            assert (raw[used:] == FILL).all(), f"{k}: written behind its end (or although it was not asked for)"
            if k in self.want:
                r[k] = raw[:used].view(dt[k])
        r["bounds"] = r["bounds"].reshape(-1, 2) if "bounds" in r else None
        r["xyzi"] = r["xyzi"].reshape(-1, 4) if "xyzi" in r else None
        return {k: v for k, v in r.items() if v is not None}

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((t == FILL).all()) for t in self.t.values())


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stats(m):
    o = np.zeros(8, np.int64)
    rc = m.lib.scvod_map_filter_stats(m.h, o.ctypes.data_as(C.c_void_p))
    return rc, o


def _free(m, d, offs, poses, params, select, out, d_pay=None, stream=None):
    """scvod_map_filter through the C ABI"""
    offs = np.ascontiguousarray(offs, np.int32)
    p = None if poses is None else np.ascontiguousarray(poses, F).reshape(-1, 6)
    k, pk = m._table256(select)
    return m.lib.scvod_map_filter(m.h, C.c_void_p(d.data_ptr()), offs.ctypes.data_as(C.c_void_p), len(offs) - 1,
                                  None if p is None else p.ctypes.data_as(C.c_void_p), C.byref(params) if params is not None else None, pk,
                                  out.ptr("result"), out.ptr("side"), out.ptr("order"), out.ptr("bounds"), out.ptr("xyzi"),
                                  None if d_pay is None else C.c_void_p(d_pay.data_ptr()), out.ptr("payload"), C.c_void_p(stream or 0))


def _batch_call(m, ctx, poses, params, select, out, d_pay=None, cap=None, stream=None):
    """scvod_batch_map_filter through the C ABI"""
    p = np.ascontiguousarray(poses, F).reshape(-1, 6)
    k, pk = m._table256(select)
    return m.lib.scvod_batch_map_filter(ctx.h, m.h, p.ctypes.data_as(C.c_void_p), C.byref(params) if params is not None else None, pk,
                                        out.ptr("result"), out.ptr("side"), out.ptr("order"), out.ptr("bounds"), out.ptr("xyzi"),
                                        None if d_pay is None else C.c_void_p(d_pay.data_ptr()), out.ptr("payload"), out.ptr("votes"),
                                        out.rows["votes"] if cap is None else cap, C.c_void_p(stream or 0))


def _same(got, ref, what=""):
    for k, g in got.items():
        w = ref[k]
        if k == "xyzi" and np.asarray(w).dtype != np.uint32:
            w = np.ascontiguousarray(w, F).view(np.uint32)
        if k == "votes":
            g, w = g.view(np.uint8), np.ascontiguousarray(w[:len(g)]).view(np.uint8)
        assert g.shape == np.asarray(w).shape, f"{what} {k}: {g.shape} != {np.asarray(w).shape}"
        if not np.array_equal(g, w):
            bad = np.flatnonzero((np.asarray(g).reshape(len(g), -1) != np.asarray(w).reshape(len(g), -1)).any(axis=1)) if len(g) else []
            raise AssertionError(f"{what} {k}: {len(bad)} rows differ from the helper, first at {bad[:5]}")


def _filter(scvod, m, pts, offs, poses=None, select=None, pay=None, want=PARTITION, **kw):
    """the cloud (numpy [n, 4]) through scvod_map_filter: (outputs, stats); asserts status 0 twice"""
    d = _dev(np.ascontiguousarray(pts, F).reshape(-1, 4))
    n, ns = len(d), len(offs) - 1
    want = tuple(w for w in want if w != "payload" or pay is not None)
    o = Out(n, ns, want=want)
    rc = _free(m, d, offs, poses, scvod.map_filter_params_default(**kw), select, o, None if pay is None else _dev(pay))
    assert rc == 0, m.lib.scvod_map_last_error(m.h).decode()
    rc, st = _stats(m)
    assert rc == 0
    return o.host(), st


def _ident(n):
    return [mq.IDENTITY] * n


def _payload(rng, n):
    p = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if n >= 3:
        p[[0, n // 2, n - 1]] = [0, 0xFFFFFFFF, 0x7FC00001]
    return p


# ---------------------------------------------------------------- 1: tile and wave edges

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1]


def _edge_map(rng):
    """known cells with an even x index in [-40, 0) (so the cell at x + 1 is never known), far cells that no radius reaches"""
    c = np.unique(np.stack([2 * rng.integers(-20, 0, 400), rng.integers(-20, 20, 400), rng.integers(-5, 5, 400)], axis=1), axis=0)
    keys = mr.pack_key(c[:, 0], c[:, 1], c[:, 2])
    vals = mr.pack_val(*rng.integers(0, 65536, (4, len(keys))))
    return c, keys, vals


def _laid_out(rng, cells, intent):
    """points whose side at radius 0 is intent (0 KNOWN: inside a known cell; 1 NOVEL: half of them in the cell at x + 1 of a known cell,
    where a radius may find the neighbour, half far away)"""
    n = len(intent)
    c = cells[rng.integers(0, len(cells), n)].astype(np.float64)
    near = rng.random(n) < 0.5
    c[(intent == 1) & near] += [1, 0, 0]
    c[(intent == 1) & ~near] += [1000, 0, 0]
    return np.concatenate([(c + rng.uniform(0.02, 0.98, (n, 3))) * 0.2, rng.uniform(0, 255, (n, 1))], axis=1).astype(F)


def _pattern(name, n):
    i = np.arange(n)
    if name == "known":
        return np.zeros(n, np.int64)
    if name == "novel":
        return np.ones(n, np.int64)
    if name == "alternate":
        return i & 1
    runs = np.concatenate([np.full(L, k & 1) for k, L in enumerate([63, 64, 65] * (n // 192 + 1))])      # runs that straddle wave boundaries
    return runs[:n]


@pytest.mark.parametrize("pattern", ["known", "novel", "alternate", "runs"])
def test_tile_and_wave_edges(scvod, pattern):
    rng = np.random.default_rng(400 + len(pattern))
    cells, keys, vals = _edge_map(rng)
    table = mq.table_of(keys, vals)
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    assert (SIZES[-1] - 1) % T == 0, "the last scan's last tile holds one point"
    pts = np.concatenate([_laid_out(rng, cells, _pattern(pattern, n)) for n in SIZES])
    pay = _payload(rng, len(pts))
    m = _merged(scvod, 4096, keys, vals, 0.2)
    for radius in (0.0, mq.R_SMALL, mq.R_MAX):
        got, st = _filter(scvod, m, pts, offs, pay=pay, radius=radius)
        ref = mf.filter(table, pts, offs, _ident(len(SIZES)), 0.2, mf.params(radius=radius), False, None, payload=pay)
        _same(got, ref, f"{pattern} radius {radius}")
        assert np.array_equal(st, ref["stats"]), (st, ref["stats"])
        if radius == 0.0:
            intent = np.concatenate([_pattern(pattern, n) for n in SIZES])
            assert np.array_equal(got["side"], intent.astype(np.uint8)), "the layout is not what the test meant it to be"
    if pattern == "runs":
        assert (got["side"] == mf.KNOWN).sum() > (intent == 0).sum(), "no NEAR point became KNOWN at the largest radius"
    m.close()


# ---------------------------------------------------------------- 2: OUT points

def test_out_points_form_the_third_segment(scvod):
    rng = np.random.default_rng(41)
    cells, keys, vals = _edge_map(rng)
    sizes = [T + 300, 1, 700]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pts = np.concatenate([_laid_out(rng, cells, _pattern("runs", n)) for n in sizes])
    poses = np.asarray([[2.0e5, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0.5]], F)       # scan 0: in range only after the pose
    pts[:sizes[0], 0] -= F(2.0e5)
    out_at = [0, 100, 101, T // 2, T - 1, T, sizes[0] - 1, sizes[0], offs[2], offs[2] + 350, offs[3] - 1]
    for k, i in enumerate(out_at):
        if k % 2:
            pts[i, k % 3] = np.nan
        else:
            pts[i, k % 3] = F(4.5e5) if i < sizes[0] else F(-3.0e5)       # beyond +-2^20 cells after the pose
    Tm = [scvod.pose_matrix(p) for p in poses]
    m = _merged(scvod, 4096, keys, vals, 0.2)
    for radius in (0.0, mq.R_MAX):
        got, st = _filter(scvod, m, pts, offs, poses=poses, radius=radius)
        ref = mf.filter(mq.table_of(keys, vals), pts, offs, Tm, 0.2, mf.params(radius=radius), False, None)
        _same(got, ref, f"radius {radius}")
        assert np.array_equal(st, ref["stats"]) and st[3] == len(out_at)
        assert sorted(np.flatnonzero(got["side"] == mf.OUT).tolist()) == sorted(int(i) for i in out_at)
        for s in range(3):
            a, b = offs[s], offs[s + 1]
            n_out = int((got["side"][a:b] == mf.OUT).sum())
            assert got["bounds"][s, 1] == (b - a) - n_out
            assert (got["side"][a + got["order"][a + got["bounds"][s, 1]:b]] == mf.OUT).all()
        assert got["bounds"][1].tolist() == [0, 0], "a scan of one OUT point"
    m.close()


# ---------------------------------------------------------------- 3: the nearest cases

@pytest.mark.parametrize("case", mq.NEAREST_CASES, ids=lambda c: c["id"])
def test_nearest_cases(scvod, case):
    ref = mq.nearest_reference(case)
    m = _case_map(scvod, case, ref)
    rng = np.random.default_rng(case["seed"])
    pts = ref["query"].copy()
    n = len(pts)
    pts.view(np.uint32)[[1, n // 3, n - 2], 3] = [0xFFFFFFFF, 0x7FC00001, 0xFFC12345]           # NaN patterns in the intensity word
    pay = _payload(rng, n)
    d = _dev(pts)
    q = m.query(d, ref["offsets"], None, case["radius"], case["select"], ("result",))["result"].cpu().numpy()
    assert np.array_equal(q, ref["cells27"]["result"])
    got, st = _filter(scvod, m, pts, ref["offsets"], select=case["select"], pay=pay, radius=case["radius"])
    assert np.array_equal(got["result"], q), "the filter's result byte is not the query's"
    want = mf.filter_from_result(ref["cells27"]["result"], pts, ref["offsets"], mf.params(radius=case["radius"]), payload=pay)
    _same(got, want, case["id"])
    assert np.array_equal(st, want["stats"]) and st[1] > 500 and st[2] > 500
    assert (got["result"] == mq.NEAR).sum() > 100
    m.close()


# ---------------------------------------------------------------- 4: more scans than one launch takes

def test_more_scans_than_one_launch_takes(scvod):
    rng = np.random.default_rng(42)
    n_scans = 65540
    sizes = np.zeros(n_scans, np.int64)
    sizes[[0, 7, 30000, 65534, 65535, 65536, 65539]] = [2, 1, 3, 3, 1, 2, 3]                      # round the seam of the two launches
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cells, keys, vals = _edge_map(rng)
    n = int(offs[-1])
    pts = _laid_out(rng, cells, np.array([1, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 1, 1, 1, 0])[:n])
    pts[8, 0] = np.nan
    m = _merged(scvod, 4096, keys, vals, 0.2)
    got, st = _filter(scvod, m, pts, offs, want=("side", "order", "bounds", "xyzi"))
    result = mq.query(mq.table_of(keys, vals), pts, [0, n], _ident(1), 0.2, 0.0)["result"]          # one pose: the cut into scans does not matter
    ref = mf.filter_from_result(result, pts, offs, mf.params())
    _same(got, ref)
    assert np.array_equal(st, ref["stats"]) and st[3] == 1
    assert got["bounds"][sizes == 0].max() == 0 and got["bounds"][65539].tolist() == [int((got["side"][-3:] == 0).sum()), 3]
    m.close()


# ---------------------------------------------------------------- 5: poses and stream order

def test_poses_and_stream_order(scvod):
    """a filter behind an accumulate on a side stream with the accumulate's poses, then one with other poses; the host offsets, poses
    and parameters are overwritten the moment each call returns"""
    import torch
    rng = np.random.default_rng(43)
    scans = [_scan(rng, n) for n in (2100, 257, 1500)]
    pts = np.concatenate(scans)
    offs0 = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    n = len(pts)
    labels = rng.choice(np.array([1, 2, 3, 6], np.uint8), n)
    keep = [1, 3, 6]
    poses0 = np.asarray([[812.5, -903.25, 41.0, 0.03, -0.08, 2.1], [814.0, -902.0, 41.1, 0.02, -0.07, 2.15], [0, 0, 0, 0, 0, 0]], F)
    other0 = poses0[::-1].copy()
    T0, T1 = [scvod.pose_matrix(p) for p in poses0], [scvod.pose_matrix(p) for p in other0]
    m = scvod.StaticMap(1 << 14, leaf=0.2, kind=scvod.MAP_KIND_LABELLED)
    d, dl = _dev(pts), _dev(labels)
    outs = [Out(n, 3, want=PARTITION[:5]) for _ in range(2)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    st = side.cuda_stream
    m.accumulate_labelled(d, dl, offs0, poses0, keep, stream=st)
    for o, poses in zip(outs, (poses0, other0)):
        off, pos = offs0.copy(), poses.copy()
        par = scvod.map_filter_params_default(radius=mq.R_SMALL)
        rc = _free(m, d, off, pos, par, [1, 3], o, stream=st)
        off[:] = -7
        pos[:] = np.nan
        par.radius, par.flags, par.reserved = -1.0, 77, 5
        assert rc == 0, m.lib.scvod_map_last_error(m.h).decode()
    rc, stats = _stats(m)                                                      # (synchronises the side stream)
    assert rc == 0
    gk, gv = mr.sorted_records(m)
    table = mq.table_of(gk, gv)
    for o, Tm, what in zip(outs, (T0, T1), ("the accumulate's poses", "other poses")):
        ref = mf.filter(table, pts, offs0, Tm, 0.2, mf.params(radius=mq.R_SMALL), True, [1, 3])
        _same(o.host(), ref, what)
    assert np.array_equal(stats, ref["stats"]) and 0 < ref["stats"][1] < n
    assert (outs[0].host()["side"] == mf.KNOWN).sum() > n // 4, "under the accumulate's own poses the selected points are known"
    m.close()


# ---------------------------------------------------------------- 6, 7: the vote on the crafted object batch

def _half_cells(keys_in_member_order):
    """the cells met first, in member order, until they cover half of the members -- but never all of the object's cells"""
    uniq, first, inv = np.unique(keys_in_member_order, return_index=True, return_inverse=True)
    by_first = np.argsort(first)
    take, covered = [], 0
    for u in by_first[:-1].tolist():
        if covered * 2 >= len(keys_in_member_order):
            break
        take.append(u)
        covered += int((inv == u).sum())
    return uniq[take]


@pytest.fixture(scope="module")
def crafted(scvod):
    b = _crafted(scvod)
    ctx = _prepared(scvod, b)
    rec, offs, mem, pobj = _full(ctx, b, NO_TRACK)
    n = rec["n_points"]
    first = np.flatnonzero(rec["scan"] == 0)
    assert sorted(n[first].tolist()) == [30, 40, 64, 100, 128, 129, 193, 300, 4500]
    ident = scvod.pose_matrix(np.zeros(6, F))
    s0 = b.x[b.offs[0]:b.offs[1]]
    key0, val0, ok0 = mr.encode_points(ident, s0, 0.2)
    assert ok0.all()
    chosen = np.zeros(len(s0), bool)
    for o in first.tolist():
        members = mem[rec["point_begin"][o]:rec["point_begin"][o] + n[o]]
        if n[o] == 100:                                                        # one object wholly in the map
            chosen[members] = True
        elif n[o] == 193:                                                      # one wholly absent
            continue
        else:
            chosen[members] = np.isin(key0[members], _half_cells(key0[members]))
    ground = (pobj[b.offs[0]:b.offs[1]] < 0) & (s0[:, 2] < -1.5)
    chosen |= ground                                                           # all the ground
    keys, vals = mr.reduce_records(key0[chosen], val0[chosen])
    m = scvod.StaticMap(1 << 16, leaf=0.2)
    m.merge(mr.to_device(keys, vals))
    Tm = [ident] * b.n
    result = mq.query(mq.table_of(keys, vals), b.x, b.offs, Tm, 0.2, mq.R_SMALL)["result"]        # computed once, shared by every run
    base = mf.filter_from_result(result, b.x, b.offs, mf.params(radius=mq.R_SMALL, flags=1), pobj, n)
    known = (base["votes"]["n_cell"] + base["votes"]["n_near"]).astype(np.int64)
    assert ((known[first] > 0) | (n[first] == 193)).all()
    for k in (64, 129, 4500):                                                  # the objects whose own count becomes the threshold
        assert 0 < known[first][n[first] == k][0] < k
    assert known[first][n[first] == 193][0] == 0 and known[first][n[first] == 100][0] == 100
    pay = _payload(np.random.default_rng(44), len(b.x))
    yield dict(b=b, ctx=ctx, rec=rec, n=n, first=first, pobj=pobj, m=m, result=result, known=known, pay=pay, d_pay=_dev(pay),
               poses=np.zeros((b.n, 6), F), keys=keys, vals=vals)
    m.close()
    ctx.close()


def _vote_run(scvod, c, m=None, result=None, cap=None, **kw):
    """one scvod_batch_map_filter with the vote on the crafted batch, every output: (outputs, status and words of the stats call, helper)"""
    b, m = c["b"], c["m"] if m is None else m
    nobj = len(c["rec"])
    o = Out(len(b.x), b.n, nobj if cap is None else cap)
    par = dict(radius=mq.R_SMALL, flags=scvod.MAPF_OBJECT_VOTE, **kw)
    rc = _batch_call(m, c["ctx"], c["poses"], scvod.map_filter_params_default(**par), None, o, c["d_pay"])
    assert rc == 0, m.lib.scvod_map_last_error(m.h).decode()
    rc, st = _stats(m)
    ref = mf.filter_from_result(c["result"] if result is None else result, b.x, b.offs, mf.params(**par), c["pobj"], c["n"], payload=c["pay"])
    return o.host(), (rc, st), ref


def _object_of(c, members):
    return int(c["first"][c["n"][c["first"]] == members][0])


@pytest.mark.parametrize("members", [64, 129, 4500])
def test_vote_at_equality_and_one_above(scvod, crafted, members):
    c = crafted
    o = _object_of(c, members)
    k = int(c["known"][o])
    moved = np.zeros(2, np.int64)
    for num, verdict in ((k, mf.KNOWN), (k + 1, mf.NOVEL)):
        got, (rc, st), ref = _vote_run(scvod, c, vote_num=num, vote_den=members)
        assert ref["votes"][o]["verdict"] == verdict
        _same(got, ref, f"{members} members, {num} / {members}")
        assert rc == 0 and np.array_equal(st, ref["stats"]), (st, ref["stats"])
        assert got["votes"][o]["verdict"] == verdict and not got["votes"]["reserved"].any()
        in_obj = (c["pobj"] == o) & (c["result"] != mq.OUT)
        assert (got["side"][in_obj] == verdict).all()
        moved += st[4:6]
    assert moved[0] > 0 and moved[1] > 0, "the vote moved no point in one of the two directions"


@pytest.mark.parametrize("kw", [dict(min_points=129), dict(min_points=130), dict(vote_num=0, vote_den=2), dict(vote_num=2, vote_den=2)],
                         ids=["min129", "min130", "num0", "num=den"])
def test_vote_min_points_and_the_ends_of_the_rule(scvod, crafted, kw):
    c = crafted
    got, (rc, st), ref = _vote_run(scvod, c, **kw)
    _same(got, ref, str(kw))
    assert rc == 0 and np.array_equal(st, ref["stats"]), (st, ref["stats"])
    o129 = _object_of(c, 129)
    if "min_points" in kw:
        assert (got["votes"][o129]["verdict"] >= 0) == (kw["min_points"] == 129)
        assert (got["votes"]["verdict"][c["n"] < kw["min_points"]] == -1).all() and st[6] == int((c["n"] >= kw["min_points"]).sum())
    elif kw["vote_num"] == 0:
        assert (got["votes"]["verdict"] == mf.KNOWN).all() and st[5] == 0 and st[6] == st[7] == len(c["rec"])
    else:
        assert st[7] == int((c["known"] == c["n"]).sum()) >= 1


def test_vote_moves_points_both_ways_in_one_run(scvod, crafted):
    """the threshold is the share of known members of one of the crafted objects: that object comes out KNOWN and takes its missing
    members along, every object with a smaller share that is not 0 comes out NOVEL and takes its known members along"""
    c = crafted
    par = dict(radius=mq.R_SMALL, flags=1)
    for o in c["first"].tolist():
        k, n = int(c["known"][o]), int(c["n"][o])
        if not 0 < k < n:
            continue
        ref = mf.filter_from_result(c["result"], c["b"].x, c["b"].offs, mf.params(vote_num=k, vote_den=n, **par), c["pobj"], c["n"])
        if ref["stats"][4] > 0 and ref["stats"][5] > 0:
            break
    else:
        raise AssertionError("no threshold among the crafted objects' own shares moves points both ways")
    got, (rc, st), ref = _vote_run(scvod, c, vote_num=k, vote_den=n)
    _same(got, ref, f"{k} / {n}")
    assert rc == 0 and np.array_equal(st, ref["stats"]) and st[4] > 0 and st[5] > 0, st


def test_vote_on_a_map_accumulated_from_the_batch_itself(scvod, crafted):
    """scan 3 (the K64 kind) has objects of its own; the map holds everything of the batch but the ground"""
    c = crafted
    b, ctx = c["b"], c["ctx"]
    m = scvod.StaticMap(1 << 18, leaf=0.2)
    m.accumulate(ctx, c["poses"], flags=scvod.MAP_NO_GROUND | scvod.MAP_IGNORE_DYNAMIC)
    gk, gv = mr.sorted_records(m)
    ident = scvod.pose_matrix(np.zeros(6, F))
    result = mq.query(mq.table_of(gk, gv), b.x, b.offs, [ident] * b.n, 0.2, mq.R_SMALL)["result"]
    got, (rc, st), ref = _vote_run(scvod, c, m=m, result=result)
    _same(got, ref, "own map")
    assert rc == 0 and np.array_equal(st, ref["stats"]), (st, ref["stats"])
    third = c["rec"]["scan"] == 3
    assert third.sum() > 3 and (got["votes"]["verdict"][third] == mf.KNOWN).all(), "an object does not know the map made of it"
    a, e = b.offs[3], b.offs[4]
    assert got["bounds"][3, 0] == int((got["side"][a:e] == mf.KNOWN).sum()) > 0 and got["bounds"][3, 1] <= e - a
    m.close()


def test_votes_capacity(scvod, crafted):
    c = crafted
    nobj = len(c["rec"])
    full, (rc, st_full), ref = _vote_run(scvod, c)
    assert rc == 0
    _same(full, ref, "full capacity")
    for cap in (nobj, nobj - 1, 0):
        got, (rc, st), _ = _vote_run(scvod, c, cap=cap)                          # (host() asserts the guard behind cap records)
        assert rc == (0 if cap == nobj else ERR_CAPACITY), (cap, rc)
        assert np.array_equal(st, st_full), "an overflow of d_votes changed the counts"
        assert np.array_equal(got["votes"].view(np.uint8), full["votes"][:cap].view(np.uint8))
        for k in PARTITION:
            assert np.array_equal(got[k], full[k]), f"cap {cap}: {k} differs from the full-capacity run"
    with pytest.raises(scvod.ScvodError):
        c["m"].filter_stats()                                                    # the shim raises on the latch
    again, (rc, st), _ = _vote_run(scvod, c)                                     # the next call with room clears it
    assert rc == 0 and np.array_equal(st, st_full) and np.array_equal(again["votes"].view(np.uint8), full["votes"].view(np.uint8))
    assert c["m"].filter_stats() == dict(zip(scvod.MAP_FILTER_STATS, st_full.tolist()))


def test_shim_forms(scvod, crafted):
    c = crafted
    b = c["b"]
    par = scvod.map_filter_params_default(radius=mq.R_SMALL, flags=scvod.MAPF_OBJECT_VOTE)
    out = c["m"].filter_batch(c["ctx"], c["poses"], par, want=scvod.MAPF_OUTPUTS, payload=c["d_pay"], votes_cap=len(c["rec"]))
    ref = mf.filter_from_result(c["result"], b.x, b.offs, mf.params(radius=mq.R_SMALL, flags=1), c["pobj"], c["n"], payload=c["pay"])
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["xyzi"], got["payload"] = got["xyzi"].view(np.uint32), got["payload"].view(np.uint32)
    got["votes"] = np.ascontiguousarray(got["votes"]).view(mf.OBJECT_DTYPE).reshape(-1)
    _same(got, ref, "filter_batch")
    assert c["m"].filter_stats()["objects_voted"] == len(c["rec"])
    a, e = int(b.offs[0]), int(b.offs[1])
    free = c["m"].filter(b.d[a:e], [0, e - a], None, scvod.map_filter_params_default(radius=mq.R_SMALL), want=("result", "side", "bounds"))
    assert np.array_equal(free["result"].cpu().numpy(), c["result"][a:e])
    assert free["bounds"].cpu().numpy().tolist() == [[int((c["result"][a:e] % 3 != 0).sum()), e - a]]     # CELL or NEAR; no OUT point


# ---------------------------------------------------------------- 8: errors and states

def test_error_and_state_cases_launch_nothing(scvod, batch):  # noqa: F811
    lib = scvod.load_lib()
    ctx, n, ns = batch["ctx"], len(batch["x"]), batch["n_scans"]
    poses = np.zeros((ns, 6), F)
    plain = scvod.StaticMap(1024, leaf=0.2)
    lab = scvod.StaticMap(1024, leaf=0.2, kind=scvod.MAP_KIND_LABELLED)
    o = Out(n, ns, 16)
    d_pay = _dev(np.zeros(n, np.uint32))
    rmax = float(F(0.99) * F(0.2))
    above = float(np.nextafter(F(rmax), F(1)))
    P = scvod.map_filter_params_default
    offs = batch["offs"]
    d = batch["d"]

    def refused(rc, code=INVALID):
        assert rc == code, (rc, lib.scvod_map_last_error(plain.h).decode())
        assert o.untouched() and plain.filter_scratch_bytes() == 0 and lab.filter_scratch_bytes() == 0

    assert _stats(plain)[0] == STATE                                              # before the first filter
    # what the query refuses
    for radius in (above, -0.05, float("nan"), float("inf")):
        refused(_free(plain, d, offs, poses, P(radius=radius), None, o, d_pay))
    refused(_free(plain, d, offs, poses, P(), [1, 3], o, d_pay))                  # a select table on a plain map
    bad = offs.copy()
    bad[2] = bad[1] - 1
    refused(_free(plain, d, bad, poses, P(), None, o, d_pay))
    bad = offs.copy()
    bad[0] = -1
    refused(_free(plain, d, bad, poses, P(), None, o, d_pay))
    refused(lib.scvod_map_filter(plain.h, None, offs.ctypes.data_as(C.c_void_p), ns, None, None, None, o.ptr("result"), o.ptr("side"), None, None,
                                 None, None, None, None))                        # NULL points
    refused(lib.scvod_map_filter(plain.h, C.c_void_p(d.data_ptr()), None, ns, None, None, None, o.ptr("result"), o.ptr("side"), None, None,
                                 None, None, None, None))                        # NULL offsets
    refused(lib.scvod_map_filter(plain.h, C.c_void_p(d.data_ptr()), offs.ctypes.data_as(C.c_void_p), -1, None, None, None, o.ptr("result"),
                                 o.ptr("side"), None, None, None, None, None, None))
    refused(lib.scvod_map_filter(plain.h, C.c_void_p(d.data_ptr() + 8), offs.ctypes.data_as(C.c_void_p), ns, None, None, None, o.ptr("result"),
                                 o.ptr("side"), None, None, None, None, None, None))                          # a misaligned cloud
    # the parameters
    for kw in (dict(reserved=1), dict(flags=2), dict(flags=-2), dict(vote_den=0), dict(vote_num=-1), dict(vote_num=3, vote_den=2),
               dict(vote_num=1, vote_den=(1 << 20) + 1), dict(min_points=0)):
        refused(_free(plain, d, offs, poses, P(**kw), None, o, d_pay))
        refused(_batch_call(plain, ctx, poses, P(**kw), None, o, d_pay))
    refused(_free(plain, d, offs, poses, P(flags=1), None, o, d_pay))             # the vote on the ctx-free form
    refused(_batch_call(plain, ctx, poses, P(), None, o, d_pay))                  # d_votes without the flag
    refused(_batch_call(plain, ctx, poses, P(flags=1), None, o, d_pay, cap=-1))
    refused(_free(plain, d, offs, poses, P(), None, o, None))                     # a payload output without a payload input
    # outputs that overlap the input cloud, a misaligned record output
    base = d.data_ptr()

    def raw(**ptr):
        a = dict(result=None, side=None, order=None, bounds=None, xyzi=None, pay_out=None)
        a.update({k: C.c_void_p(v) for k, v in ptr.items()})
        return lib.scvod_map_filter(plain.h, C.c_void_p(base), offs.ctypes.data_as(C.c_void_p), ns, None, None, None, a["result"], a["side"],
                                    a["order"], a["bounds"], a["xyzi"], C.c_void_p(d_pay.data_ptr()), a["pay_out"], None)

    for k in ("result", "side", "order", "bounds", "xyzi", "pay_out"):
        refused(raw(**{k: base}))
        refused(raw(**{k: base + 16 * (n - 1)}))                                  # the last record
    refused(raw(xyzi=o.t["xyzi"].data_ptr() + 8))
    refused(raw(order=o.t["order"].data_ptr() + 2))
    # states
    fresh = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=ns)
    refused(lib.scvod_batch_map_filter(fresh.h, plain.h, poses.ctypes.data_as(C.c_void_p), None, None, o.ptr("result"), o.ptr("side"), None, None,
                                       None, None, None, None, 0, None), STATE)   # no batch
    fresh.close()
    refused(_batch_call(plain, ctx, poses, P(flags=1), None, o, d_pay), STATE)     # a batch without clustering: no table
    # and the same arguments made right run
    ok = Out(n, ns, want=PARTITION)
    assert _free(plain, d, offs, poses, P(radius=rmax), None, ok, d_pay) == 0
    assert _stats(plain)[0] == 0 and plain.filter_scratch_bytes() > 0 and not ok.untouched()
    assert _batch_call(lab, ctx, poses, P(radius=rmax), np.ones(256, np.uint8), ok, d_pay, cap=0) == 0
    rc, st = _stats(lab)
    assert rc == 0 and st.tolist() == [n, 0, n - 2, 2, 0, 0, 0, 0]
    plain.close()
    lab.close()


def test_vote_states(scvod):
    import torch
    from test_gpu_async_chain import _batch, _new_ctx, _track
    b = _batch(scvod, "K6")
    n = int(b.offs[-1])
    ctx = _new_ctx(scvod, [b])
    m = scvod.StaticMap(1024, leaf=0.2)
    o = Out(n, b.n, n, want=tuple(k for k in NAMES if k != "payload"))
    par = scvod.map_filter_params_default(flags=scvod.MAPF_OBJECT_VOTE)
    cnt = Tab(b, 0, 0, members=False, points=False)
    tab = Tab(b, n, n)
    torch.cuda.synchronize()

    def call():
        return _batch_call(m, ctx, b.poses, par, None, o)

    def refused(code):
        assert call() == code and o.untouched() and m.filter_scratch_bytes() == 0

    refused(STATE)                                                        # no batch
    ctx.batch_process(b.d, b.offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    refused(STATE)                                                        # a batch, but no table
    assert cnt.call(ctx, NO_TRACK, records=False) == 0
    refused(STATE)                                                        # a count-only table is none
    assert tab.call(ctx, NO_TRACK) == 0
    ctx.batch_cluster()                                                   # a table from before another clustering
    refused(STATE)
    ctx.batch_cluster_types()
    refused(STATE)
    _track(ctx, b, b.T, b.nxt, None, 1)
    assert tab.call(ctx, 0) == 0
    ctx.batch_cluster_types()                                             # a table that read a tracking result which is stale now
    refused(INVALID)
    assert tab.call(ctx, NO_TRACK) == 0 and call() == 0                   # made right, it runs
    rc, st = _stats(m)
    assert rc == 0 and st[0] == n and st[6] > 0 and not o.untouched()
    torch.cuda.synchronize()
    m.close()
    ctx.close()


@pytest.mark.skipif("__import__('torch').cuda.device_count() < 2", reason="needs two visible devices")
def test_a_map_on_another_device_is_refused(scvod, batch):  # noqa: F811
    ns = batch["n_scans"]
    m = scvod.StaticMap(1024, leaf=0.2, device=1)
    o = Out(len(batch["x"]), ns, want=PARTITION[:5])
    assert _batch_call(m, batch["ctx"], np.zeros((ns, 6), F), None, None, o, cap=0) == INVALID
    assert "different devices" in m.lib.scvod_map_last_error(m.h).decode()
    assert o.untouched() and m.filter_scratch_bytes() == 0
    m.close()


# ---------------------------------------------------------------- 9: nothing else moves

def test_the_filter_moves_nothing_else(scvod, crafted):
    import torch
    c = crafted
    b, ctx = c["b"], c["ctx"]
    n = len(b.x)
    m = scvod.StaticMap(1 << 16, leaf=0.2)
    m.merge(mr.to_device(c["keys"], c["vals"]))
    m.query_batch(ctx, c["poses"], mq.R_MAX, None, ("result",))
    d_gt = _dev((np.arange(n) % 7).astype(np.uint32))
    tr = Tru(len(c["rec"]))
    torch.cuda.synchronize()
    assert tr.call(ctx, d_gt) == 0
    truth_before = tr.buf.cpu().numpy().copy()

    def state():
        return (m.query_stats(), m.query_scratch_bytes(), m.scratch_bytes(), ctx.arena_bytes(), ctx.batch_objects_scratch_bytes(),
                ctx.batch_object_truth_scratch_bytes(), m.count())

    before, rec_before = state(), mr.sorted_records(m)
    assert m.filter_scratch_bytes() == 0
    first, (rc, st), ref = _vote_run(scvod, c, m=m)
    _same(first, ref, "first run")
    bytes_after_first = m.filter_scratch_bytes()
    second, (rc2, st2), _ = _vote_run(scvod, c, m=m)
    assert rc == rc2 == 0 and np.array_equal(st, st2)
    for k in first:
        assert np.array_equal(np.asarray(first[k]).view(np.uint8), np.asarray(second[k]).view(np.uint8)), f"two runs differ in {k}"
    assert 0 < bytes_after_first == m.filter_scratch_bytes(), "the scratch grew although nothing did"
    assert state() == before
    rec_after = mr.sorted_records(m)
    assert np.array_equal(rec_before[0], rec_after[0]) and np.array_equal(rec_before[1], rec_after[1])
    tr2 = Tru(len(c["rec"]))
    torch.cuda.synchronize()
    assert tr2.call(ctx, d_gt) == 0
    assert np.array_equal(tr2.buf.cpu().numpy(), truth_before), "the object truth on the same table changed"
    m.close()


# ---------------------------------------------------------------- 10: the batch form

def test_batch_form_equals_the_ctx_free_form(scvod, batch):  # noqa: F811
    ns = batch["n_scans"]
    n = len(batch["x"])
    poses = np.asarray([[0.7 * s, 0.1 * s, 0.01 * s, 0.002 * s, -0.003 * s, 0.01 * s] for s in range(ns)], F)
    m = scvod.StaticMap(1 << 14, leaf=0.2)
    m.accumulate_range(batch["ctx"], poses, 0, 2, flags=scvod.MAP_IGNORE_DYNAMIC)        # the map holds two of the four scans
    gk, gv = mr.sorted_records(m)
    Tm = [scvod.pose_matrix(p) for p in poses]
    pay = _payload(np.random.default_rng(45), n)
    d_pay = _dev(pay)
    for radius in (0.0, mq.R_MAX):
        par = scvod.map_filter_params_default(radius=radius)
        a, f = Out(n, ns, want=PARTITION), Out(n, ns, want=PARTITION)
        assert _batch_call(m, batch["ctx"], poses, par, None, a, d_pay, cap=0) == 0
        rc, sa = _stats(m)
        assert rc == 0 and _free(m, batch["d"], batch["offs"], poses, par, None, f, d_pay) == 0
        rc, sf = _stats(m)
        assert rc == 0 and np.array_equal(sa, sf)
        ha, hf = a.host(), f.host()
        _same(ha, hf, "batch against ctx-free")
        ref = mf.filter(mq.table_of(gk, gv), batch["x"], batch["offs"], Tm, 0.2, mf.params(radius=radius), False, None, payload=pay)
        _same(ha, ref, "batch against the helper")
        assert np.array_equal(sa, ref["stats"]) and sa[3] == 2 and sa[1] > 1000 and sa[4:].tolist() == [0, 0, 0, 0]
    m.close()
