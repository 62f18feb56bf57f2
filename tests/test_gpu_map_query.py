"""scvod_map_query / scvod_batch_map_query (csrc/scvod_mapquery.hip) against the numpy statement tests/helpers/map_query_ref.py, bit for
bit: the probe chain on tables built to go wrong, runs of equal cells across wave boundaries, the nearest representative on seeded
clouds near +-1000 m (where tests/test_capi_map_query.py shows the 27 cells to be the exhaustive answer), a query behind an accumulate,
the batch form and its error states, stream order, and that a query moves nothing else."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import map_query_ref as mq  # noqa: E402
import map_ref as mr  # noqa: E402
from test_gpu_map_table import _keys_behind_barriers, _keys_with_home, _raw_export, _scan  # noqa: E402  (the table generators)

pytestmark = pytest.mark.gpu

INVALID, STATE, ERR_CAPACITY = -1, -5, -4
ALL = ("result", "cell_val", "nn_key", "nn_sqdist", "scan_counts")
CELL_ONLY = ("result", "cell_val", "scan_counts")
F = np.float32


def _np(out):
    r = {}
    for k, v in out.items():
        a = v.cpu().numpy()
        r[k] = a.view(np.uint64) if k in ("cell_val", "nn_key") else a
    return r


def _query(m, pts, offsets, poses=None, radius=0.0, select=None, want=None):
    """the cloud (numpy [n, 4]) through StaticMap.query: numpy outputs and the stats"""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(pts, F).reshape(-1, 4)).cuda()
    both = want is None and radius > 0
    if want is None:
        want = ALL if radius > 0 else CELL_ONLY

    def ask(w):
        r = _np(m.query(d, np.asarray(offsets, np.int32), poses, float(radius), select, w))
        st = m.query_stats()
        r["stats"] = np.array([st[k] for k in ("points", "cell", "near", "miss", "out")], np.int64)
        return r

    r = ask(want)
    if both:        # without the nn pair the kernel takes another path (points without an own cell are queued): the same answers
        c = ask(CELL_ONLY)
        assert all(np.array_equal(c[k], r[k]) for k in c), "cell outputs alone differ from the same outputs beside the nn pair"
    return r


def _same(got, ref, what=""):
    for k, g in got.items():
        if k == "nn_sqdist":
            assert np.array_equal(g.view(np.uint32), ref[k].view(np.uint32)), f"{what} {k}"
        else:
            assert np.array_equal(g, ref[k]), f"{what} {k}"


def _ident(n):
    return [mq.IDENTITY] * n


def _merged(scvod, capacity, keys, vals, leaf, kind=0):
    m = scvod.StaticMap(capacity, leaf=leaf, kind=kind)
    if len(keys):
        m.merge(mr.to_device(keys, vals))
    return m


# ---------------------------------------------------------------- 1: the table alone

def _walk(occ):
    """per slot: occupied slots from it (inclusive) to the next empty one, circular (what a probe for an absent key walks)"""
    n = len(occ)
    w = np.zeros(2 * n, np.int64)
    o2 = np.concatenate([occ, occ])
    for i in range(2 * n - 2, -1, -1):
        w[i] = w[i + 1] + 1 if o2[i] else 0
    return np.minimum(w[:n], n)


def _centres_exact(keys):
    """leaf 1.0: c + 0.5 is exact in fp32 for every cell, so the centre of a key's cell encodes to that key"""
    p = mq.cell_centres(keys, 1.0)
    k, _, ok = mr.encode_points(mq.IDENTITY, p, 1.0)
    assert ok.all() and np.array_equal(k, keys)
    return p


@pytest.mark.parametrize("capacity", [1024, 4096])
def test_probe_chains_under_load_and_round_the_end(scvod, capacity):
    rng = np.random.default_rng(300 + capacity)
    keys = _keys_behind_barriers(rng, capacity, int(capacity * 0.95), first_barrier=100)
    occ = mr.simulate_table(keys, capacity)
    run, _ = mr.longest_run(occ)
    assert 100 <= run <= 400 and occ[capacity - 1] and occ[0], "precondition: long chains, one of them round the end of the table"
    vals = mr.random_keys(rng, len(keys))
    walk = _walk(occ)
    cand = mr.random_keys(rng, 6000)
    cand = cand[~np.isin(cand, keys)]
    h = mr.home(cand, capacity)
    absent = np.concatenate([cand[walk[h] >= run // 2][:300], cand[h >= capacity - 20][:50], cand[:300]])   # deep in the longest runs, before the wrap
    assert len(absent) >= 400 and walk[mr.home(absent, capacity)].max() >= run // 2
    q = rng.permutation(np.concatenate([keys, absent]))
    pts = _centres_exact(q)
    table = mq.table_of(keys, vals)
    m = _merged(scvod, capacity, keys, vals, 1.0)
    offs = [0, len(q) // 2, len(q)]
    got = _query(m, pts, offs)
    ref = mq.query(table, pts, offs, _ident(2), 1.0)
    _same(got, ref)
    assert np.array_equal(got["result"] == mq.CELL, np.isin(q, keys)) and not (got["result"] >= mq.NEAR).any()
    got = _query(m, pts, offs, radius=0.99)
    _same(got, mq.query(table, pts, offs, _ident(2), 1.0, 0.99), "radius")
    m.close()


def test_300_keys_on_one_home_slot(scvod):
    capacity = 1024
    rng = np.random.default_rng(31)
    same = _keys_with_home(rng, capacity, 420, capacity - 50, capacity - 49)
    keys, absent = same[:300], same[300:]                       # the absent ones walk all 300 slots, 250 of them behind the wrap
    vals = mr.random_keys(rng, 300)
    q = rng.permutation(np.concatenate([keys, absent]))
    pts = _centres_exact(q)
    m = _merged(scvod, capacity, keys, vals, 1.0)
    got = _query(m, pts, [0, len(q)])
    _same(got, mq.query(mq.table_of(keys, vals), pts, [0, len(q)], _ident(1), 1.0))
    assert got["stats"].tolist() == [420, 300, 0, 120, 0]
    m.close()


def test_a_table_that_overflowed(scvod):
    """the dictionary is what the table holds: a key whose insertion was dropped is absent, and a probe ends at the bound of 512 slots
    although no slot of the full table is empty"""
    capacity = 1024
    rng = np.random.default_rng(32)
    keys, vals = mr.random_keys(rng, 2000), mr.random_keys(rng, 2000)
    m = _merged(scvod, capacity, keys, vals, 1.0)
    rc, n, buf = _raw_export(m, capacity + 8)
    assert rc == ERR_CAPACITY and n == capacity, "precondition: the table is full"
    table = mq.table_of(buf[:n, 0], buf[:n, 1])
    more = mr.random_keys(rng, 500)
    q = rng.permutation(np.concatenate([keys, more[~np.isin(more, keys)]]))
    pts = _centres_exact(q)
    got = _query(m, pts, [0, len(q)])
    _same(got, mq.query(table, pts, [0, len(q)], _ident(1), 1.0))
    assert got["stats"][1] == capacity
    m.close()


# ---------------------------------------------------------------- 2: runs

def _runs_cloud(rng):
    """points in input order made of runs of equal cells (1, 63, 64, 65, 129, ... so that runs start and end at every place of a wave),
    with NaN and out-of-range points inside runs; (points, the cells of the runs)"""
    lengths = [1, 63, 64, 65, 129, 1, 1, 64, 64, 3, 129, 65, 63, 2, 127, 64, 1, 200, 65, 30]
    cells = rng.integers(-50, 50, (len(lengths), 3))
    cells[7] = cells[8]                                           # two whole waves in one cell
    cells[13] = cells[11]                                         # a cell that comes back later
    p = []
    for c, L in zip(cells, lengths):
        p.append(np.concatenate([(c + rng.uniform(0.1, 0.9, (L, 3))) * 0.2, rng.uniform(0, 255, (L, 1))], axis=1))
    p = np.concatenate(p).astype(F)
    start = np.concatenate([[0], np.cumsum(lengths)])
    p[start[4] + 64, 0] = np.nan                                  # inside the run of 129, at a wave boundary
    p[start[4] + 100, 2] = np.nan
    p[start[3] + 10, 0] = 3.0e5                                   # beyond the range, inside the run of 65
    p[start[10] + 1, 1] = -3.0e5
    p[start[17] + 50:start[17] + 53, 0] = np.nan                  # three in a row
    p[start[0], 0] = np.nan                                       # the very first point
    p[-1, 2] = 3.0e5                                              # and the very last
    return p, cells


def test_runs_across_wave_boundaries(scvod):
    rng = np.random.default_rng(33)
    p, cells = _runs_cloud(rng)
    seven = np.concatenate([(cells[2] + rng.uniform(0.1, 0.9, (7, 3))) * 0.2, np.zeros((7, 1))], axis=1).astype(F)
    pts = np.concatenate([p, seven])
    offs = [0, len(p), len(p), len(pts)]                          # the runs, a scan of 0 points, a scan of 7
    present = np.unique(cells[::2], axis=0)                        # every other run's cell is in the map ...
    nb = present[:6] + np.array([1, 0, 0])                         # ... and some neighbours of those
    c = np.unique(np.concatenate([present, nb]), axis=0)
    keys = mr.pack_key(c[:, 0], c[:, 1], c[:, 2])
    vals = mr.pack_val(*rng.integers(0, 65536, (4, len(keys))))
    table = mq.table_of(keys, vals)
    m = _merged(scvod, 1024, keys, vals, 0.2)
    for radius in (0.0, mq.R_SMALL, mq.R_MAX):
        got = _query(m, pts, offs, radius=radius)
        ref = mq.query(table, pts, offs, _ident(3), 0.2, radius)
        _same(got, ref, f"radius {radius}")
        assert got["stats"][4] == 9 and got["stats"][1] > 300 and got["scan_counts"][1].tolist() == [0, 0, 0, 0]
        assert np.array_equal(got["stats"], ref["stats"])
    m.close()


def test_no_scan_and_an_empty_map(scvod):
    import torch
    rng = np.random.default_rng(34)
    p, _ = _runs_cloud(rng)
    m = scvod.StaticMap(1024, leaf=0.2)
    assert m.query_scratch_bytes() == 0
    with pytest.raises(scvod.ScvodError):
        m.query_stats()                                            # before the first query
    d = torch.from_numpy(p).cuda()
    out = m.query(d, np.zeros(1, np.int32), None, 0.0, None, ("result", "scan_counts"))   # n_scans == 0
    assert out["result"].numel() == 0 and out["scan_counts"].shape == (0, 4)
    assert m.query_stats() == dict(points=0, cell=0, near=0, miss=0, out=0)
    rc = m.lib.scvod_map_query(m.h, None, None, 0, None, 0.0, None, None, None, None, None, None, None)
    assert rc == 0
    for radius in (0.0, mq.R_MAX):
        got = _query(m, p, [0, len(p)], radius=radius)
        _same(got, mq.query({}, p, [0, len(p)], _ident(1), 0.2, radius))
        assert got["stats"][1] == got["stats"][2] == 0 and got["stats"][3] == len(p) - 9
    assert m.query_scratch_bytes() > 0 and m.count() == 0
    m.close()


def test_more_scans_than_one_launch_takes(scvod):
    """70 000 scans of one point each: the scan index is a grid dimension, so they take two launches (65 535 + 4 465).  Under one pose
    the answer per point does not depend on how the cloud is cut into scans: the reference is the same cloud as one scan"""
    rng = np.random.default_rng(38)
    n = 70000
    cells = rng.integers(-20, 20, (n, 3))
    pts = np.concatenate([(cells + rng.uniform(0.1, 0.9, (n, 3))) * 0.2, np.zeros((n, 1))], axis=1).astype(F)
    pts[65534:65537, 0] = np.nan                                   # round the seam of the two launches
    c = np.unique(cells[::3], axis=0)
    keys = mr.pack_key(c[:, 0], c[:, 1], c[:, 2])
    vals = mr.pack_val(*rng.integers(0, 65536, (4, len(keys))))
    m = _merged(scvod, 1 << 16, keys, vals, 0.2)
    ref = mq.query(mq.table_of(keys, vals), pts, [0, n], _ident(1), 0.2, mq.R_MAX)
    got = _query(m, pts, np.arange(n + 1), radius=mq.R_MAX)
    counts = got.pop("scan_counts")
    ref.pop("scan_counts")
    _same(got, ref)
    col = np.array([2, 0, 1, 3])[ref["result"]]                    # MISS, CELL, NEAR, OUT -> the column of {CELL, NEAR, MISS, OUT}
    assert np.array_equal(counts, np.eye(4, dtype=np.int64)[col])
    assert ref["stats"][1] > 20000 and ref["stats"][2] > 1000 and ref["stats"][4] == 3
    m.close()


# ---------------------------------------------------------------- 3: nearest

def _case_map(scvod, case, ref):
    """the map of a nearest case: a labelled map through accumulate_labelled (its export is the helper's dictionary), a plain one
    through merge of the dictionary"""
    import torch
    if not case["labelled"]:
        k = np.fromiter(ref["table"].keys(), np.uint64)
        v = np.fromiter(ref["table"].values(), np.uint64)
        return _merged(scvod, 1 << 15, k, v, mq.LEAF)
    m = scvod.StaticMap(1 << 15, leaf=mq.LEAF, kind=scvod.MAP_KIND_LABELLED)
    m.accumulate_labelled(torch.from_numpy(ref["base"]).cuda(), torch.from_numpy(ref["labels"]).cuda(), [0, len(ref["base"])])
    gk, gv = mr.sorted_records(m)
    assert mq.table_of(gk, gv) == ref["table"]
    return m


@pytest.mark.parametrize("case", mq.NEAREST_CASES, ids=lambda c: c["id"])
def test_nearest_representative(scvod, case):
    ref = mq.nearest_reference(case)
    m = _case_map(scvod, case, ref)
    got = _query(m, ref["query"], ref["offsets"], radius=case["radius"], select=case["select"])
    _same(got, ref["cells27"], "27 cells")
    _same(got, ref["exhaustive"], "exhaustive")
    assert np.array_equal(got["stats"], ref["cells27"]["stats"])
    only = _query(m, ref["query"], ref["offsets"], radius=case["radius"], select=case["select"], want=("result",))
    assert np.array_equal(only["result"], got["result"]) and np.array_equal(only["stats"], got["stats"])
    own = _query(m, ref["query"], ref["offsets"], radius=0.0, select=case["select"])
    assert np.array_equal(own["cell_val"], got["cell_val"])
    assert np.array_equal(own["result"], np.where(got["result"] == mq.NEAR, mq.MISS, got["result"]))
    m.close()


def test_the_tie_goes_to_the_smaller_key(scvod):
    keys, vals, q, small = mq.tie_case()
    for order in ((0, 1), (1, 0)):
        m = scvod.StaticMap(1024, leaf=0.2)
        for i in order:
            m.merge(mr.to_device(keys[i:i + 1], vals[i:i + 1]))
        for radius in (mq.R_SMALL, mq.R_MAX):
            got = _query(m, q, [0, 1], radius=radius)
            _same(got, mq.query(mq.table_of(keys, vals), q, [0, 1], _ident(1), 0.2, radius))
            assert got["nn_key"].tolist() == [small]
        m.close()


# ---------------------------------------------------------------- 4: against the accumulate

def test_a_query_behind_the_accumulate(scvod):
    import torch
    rng = np.random.default_rng(35)
    scans = [_scan(rng, n) for n in (2100, 257, 1500)]
    pts = np.concatenate(scans)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    labels = rng.choice(np.array([1, 2, 3, 6], np.uint8), len(pts))
    keep = [1, 3, 6]
    poses = np.asarray([[812.5, -903.25, 41.0, 0.03, -0.08, 2.1], [814.0, -902.0, 41.1, 0.02, -0.07, 2.15], [0, 0, 0, 0, 0, 0]], F)
    T = [scvod.pose_matrix(p) for p in poses]
    m = scvod.StaticMap(1 << 14, leaf=0.2, kind=scvod.MAP_KIND_LABELLED)
    d = torch.from_numpy(pts).cuda()
    m.accumulate_labelled(d, torch.from_numpy(labels).cuda(), offs, poses, keep)
    kept = np.isin(labels, keep)
    ks, vs = [], []
    for s in range(3):
        a, b = offs[s], offs[s + 1]
        t = mq.build_table(pts[a:b][kept[a:b]], T[s], 0.2, labels[a:b][kept[a:b]])
        ks.append(np.fromiter(t.keys(), np.uint64))
        vs.append(np.fromiter(t.values(), np.uint64))
    ek, ev = mr.reduce_records(np.concatenate(ks), np.concatenate(vs))
    gk, gv = mr.sorted_records(m)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    table = mq.table_of(ek, ev)
    got = _np(m.query(d, offs, poses, 0.0, None, CELL_ONLY))              # the poses of the accumulate before it
    assert (got["result"][kept] == mq.CELL).all()
    own = np.concatenate([mr.encode_points(T[s], pts[offs[s]:offs[s + 1]], 0.2)[0] for s in range(3)])
    assert np.array_equal(got["cell_val"][kept], ev[np.searchsorted(ek, own[kept])])
    _same(got, mq.query(table, pts, offs, T, 0.2, 0.0, labelled=True))
    other = poses[::-1].copy()
    T2 = [scvod.pose_matrix(p) for p in other]
    for radius, select in ((0.0, None), (mq.R_MAX, None), (mq.R_SMALL, [1, 3])):
        got = _query(m, pts, offs, other, radius, select)
        ref = mq.query(table, pts, offs, T2, 0.2, radius, labelled=True, select=select)
        _same(got, ref, f"radius {radius}")
        assert 0 < ref["stats"][1] < len(pts)
    m.close()


# ---------------------------------------------------------------- 5: the batch form

class _Out:
    """sentinel-filled outputs of one call through the C ABI"""

    def __init__(self, n, n_scans):
        import torch
        self.t = [torch.full((n,), 0x55, dtype=torch.uint8, device="cuda"), torch.full((n,), 0x5555, dtype=torch.int64, device="cuda"),
                  torch.full((n,), 0x5555, dtype=torch.int64, device="cuda"), torch.full((n,), 5.5, dtype=torch.float32, device="cuda"),
                  torch.full((n_scans, 4), 0x5555, dtype=torch.int64, device="cuda")]
        self.before = [t.clone() for t in self.t]

    def ptr(self, nn=True):
        return [C.c_void_p(t.data_ptr()) if (nn or i not in (2, 3)) else None for i, t in enumerate(self.t)]

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((a == b).all()) for a, b in zip(self.t, self.before))


@pytest.fixture(scope="module")
def batch(scvod):
    import torch
    rng = np.random.default_rng(36)
    scans = [_scan(rng, n) for n in (255, 2100, 1500, 257)]
    x = np.concatenate(scans)
    x[3000, 1] = 4.0e5                                             # two points without a cell (in the scans the tests do not accumulate)
    x[3955, 0] = -4.0e5
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    ctx = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=len(x) + 64, max_scans=len(scans))
    d = torch.from_numpy(x).cuda()
    ctx.batch_process(d, offs)
    yield dict(ctx=ctx, d=d, x=x, offs=offs, n_scans=len(scans))
    ctx.close()


def test_batch_form_equals_the_ctx_free_form(scvod, batch):
    poses = np.asarray([[0.7 * s, 0.1 * s, 0.01 * s, 0.002 * s, -0.003 * s, 0.01 * s] for s in range(batch["n_scans"])], F)
    m = scvod.StaticMap(1 << 14, leaf=0.2)
    m.accumulate_range(batch["ctx"], poses, 0, 2, flags=scvod.MAP_IGNORE_DYNAMIC)        # the map holds two of the four scans
    gk, gv = mr.sorted_records(m)
    table = mq.table_of(gk, gv)
    T = [scvod.pose_matrix(p) for p in poses]
    for radius in (0.0, mq.R_MAX):
        want = ALL if radius > 0 else CELL_ONLY
        a = _np(m.query_batch(batch["ctx"], poses, radius, None, want))
        sa = m.query_stats()
        b = _np(m.query(batch["d"], batch["offs"], poses, radius, None, want))
        assert m.query_stats() == sa
        _same(a, b, "batch against ctx-free")
        _same(a, mq.query(table, batch["x"], batch["offs"], T, 0.2, radius), "batch against the helper")
        n = np.diff(batch["offs"])
        assert np.array_equal(a["scan_counts"].sum(axis=1), n)                            # every input point, the dropped ones too
        assert sa["points"] == int(n.sum()) and [sa["cell"], sa["near"], sa["miss"], sa["out"]] == a["scan_counts"].sum(axis=0).tolist()
        assert sa["out"] == 2 and sa["cell"] > 1000
        for v, name in enumerate(("miss", "cell", "near", "out")):
            assert int((a["result"] == v).sum()) == sa[name]
    m.close()


def test_error_states_launch_nothing(scvod, batch):
    import torch
    lib = scvod.load_lib()
    ctx, n, ns = batch["ctx"], len(batch["x"]), batch["n_scans"]
    poses = np.zeros((ns, 6), F)
    pp = poses.ctypes.data_as(C.c_void_p)
    sel = np.ones(256, np.uint8).ctypes.data_as(C.c_void_p)
    plain = scvod.StaticMap(1024, leaf=0.2)
    lab = scvod.StaticMap(1024, leaf=0.2, kind=scvod.MAP_KIND_LABELLED)
    o = _Out(n, ns)
    rmax = float(F(0.99) * F(0.2))
    above = float(np.nextafter(F(rmax), F(1)))

    def batch_call(m, radius, select=None, nn=True, c=ctx):
        return lib.scvod_batch_map_query(c.h, m.h, pp, radius, select, *o.ptr(nn), None)

    fresh = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=ns)
    assert batch_call(plain, 0.05, c=fresh) == STATE and o.untouched()                   # no batch
    fresh.close()
    assert batch_call(plain, 0.05, select=sel) == INVALID and o.untouched()              # a select table on a plain map
    assert batch_call(lab, above) == INVALID and o.untouched()                           # above 0.99f * leaf
    assert batch_call(lab, -0.05) == INVALID and o.untouched()
    assert batch_call(lab, float("nan")) == INVALID and o.untouched()
    assert batch_call(lab, float("inf")) == INVALID and o.untouched()
    assert batch_call(lab, 0.0, nn=True) == INVALID and o.untouched()                    # nn outputs with radius 0
    assert "radius" in lib.scvod_map_last_error(lab.h).decode()
    assert plain.query_scratch_bytes() == 0 and lab.query_scratch_bytes() == 0            # nothing was allocated either
    # the ctx-free form: a misaligned cloud, offsets that decrease or start below 0, NULL points, NULL offsets
    offs = batch["offs"]

    def free_call(m, d_ptr, off, radius=0.05, select=None, nn=True, n_scans=ns):
        return lib.scvod_map_query(m.h, d_ptr, None if off is None else off.ctypes.data_as(C.c_void_p), n_scans, pp, radius, select,
                                   *o.ptr(nn), None)

    dp = batch["d"].data_ptr()
    assert free_call(plain, C.c_void_p(dp + 8), offs) == INVALID and o.untouched()
    bad = offs.copy()
    bad[2] = bad[1] - 1
    assert free_call(plain, C.c_void_p(dp), bad) == INVALID and o.untouched()
    bad = offs.copy()
    bad[0] = -1
    assert free_call(plain, C.c_void_p(dp), bad) == INVALID and o.untouched()
    assert free_call(plain, None, offs) == INVALID and o.untouched()
    assert free_call(plain, C.c_void_p(dp), None) == INVALID and o.untouched()
    assert free_call(plain, C.c_void_p(dp), offs, n_scans=-1) == INVALID and o.untouched()
    assert free_call(plain, C.c_void_p(dp), offs, select=sel) == INVALID and o.untouched()
    assert free_call(plain, C.c_void_p(dp), offs, radius=0.0) == INVALID and o.untouched()
    assert free_call(plain, C.c_void_p(dp), offs, radius=above) == INVALID and o.untouched()
    # and the same arguments made right run
    assert batch_call(lab, rmax, select=sel) == 0 and free_call(plain, C.c_void_p(dp), offs, radius=0.0, nn=False) == 0
    assert not o.untouched()
    assert plain.query_stats()["points"] == n and lab.query_stats()["miss"] == n - 2
    plain.close()
    lab.close()


# ---------------------------------------------------------------- 6: stream order

def test_queries_are_ordered_by_the_stream(scvod):
    """accumulate A, query, accumulate B, query, clear, query on a side stream, one synchronisation at the end; the host offsets and
    poses are overwritten the moment each call returns (all calls use the same values, so nothing waits for the staging copies)"""
    import torch
    rng = np.random.default_rng(37)
    A, B, Q = [np.concatenate([(rng.integers(lo, hi, (4000, 3)) + rng.uniform(0.05, 0.95, (4000, 3))) * 0.2, rng.uniform(0, 200, (4000, 1))],
                              axis=1).astype(F) for lo, hi in ((-8, 4), (-4, 8), (-8, 8))]
    la, lb = rng.choice(np.array([1, 4], np.uint8), 4000), rng.choice(np.array([5, 6], np.uint8), 4000)
    offs0 = np.array([0, 1500, 4000], np.int32)
    poses0 = np.asarray([[1.5, -2.0, 0.25, 0.01, -0.02, 0.7], [1.0, -2.5, 0.3, 0.0, 0.01, 0.72]], F)
    T = [scvod.pose_matrix(p) for p in poses0]
    dA, dB, dQ = (torch.from_numpy(a).cuda() for a in (A, B, Q))
    dla, dlb = torch.from_numpy(la).cuda(), torch.from_numpy(lb).cuda()
    outs = [{k: torch.full(s, f, dtype=t, device="cuda") for k, s, t, f in (("result", (4000,), torch.uint8, 0x55), ("cell_val", (4000,), torch.int64, 0x55),
                                                                          ("nn_key", (4000,), torch.int64, 0x55), ("nn_sqdist", (4000,), torch.float32, 5.5),
                                                                          ("scan_counts", (2, 4), torch.int64, 0x55))} for _ in range(3)]
    m = scvod.StaticMap(1 << 13, leaf=0.2, kind=scvod.MAP_KIND_LABELLED)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    st = C.c_void_p(side.cuda_stream)
    lib = m.lib

    def scribbled(fn):
        off, pos = offs0.copy(), poses0.copy()
        rc = fn(off.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p))
        off[:] = -7
        pos[:] = np.nan
        assert rc == 0, lib.scvod_map_last_error(m.h).decode()

    def acc(d, lab):
        scribbled(lambda po, pp: lib.scvod_map_accumulate_labelled(m.h, C.c_void_p(d.data_ptr()), C.c_void_p(lab.data_ptr()), po, 2, pp, None, st))

    def ask(o):
        ptr = [C.c_void_p(o[k].data_ptr()) for k in ALL]
        scribbled(lambda po, pp: lib.scvod_map_query(m.h, C.c_void_p(dQ.data_ptr()), po, 2, pp, mq.R_MAX, None, *ptr, st))

    acc(dA, dla)
    ask(outs[0])
    acc(dB, dlb)
    ask(outs[1])
    assert lib.scvod_map_clear(m.h, st) == 0
    ask(outs[2])
    side.synchronize()
    tA = mq.build_table(A[:1500], T[0], 0.2, la[:1500]), mq.build_table(A[1500:], T[1], 0.2, la[1500:])
    tB = mq.build_table(B[:1500], T[0], 0.2, lb[:1500]), mq.build_table(B[1500:], T[1], 0.2, lb[1500:])

    def union(tables):
        k = np.concatenate([np.fromiter(t.keys(), np.uint64) for t in tables])
        v = np.concatenate([np.fromiter(t.values(), np.uint64) for t in tables])
        return mq.table_of(*mr.reduce_records(k, v))

    states = [union(tA), union(tA + tB), {}]
    refs = [mq.query(t, Q, offs0, T, 0.2, mq.R_MAX, labelled=True) for t in states]
    for i in range(3):
        _same(_np(outs[i]), refs[i], f"state {i}")
    assert refs[0]["stats"][1] < refs[1]["stats"][1] and refs[0]["stats"][1] > 100 and refs[2]["stats"][3] == 4000
    assert m.query_stats() == dict(points=4000, cell=0, near=0, miss=4000, out=0)
    m.close()


# ---------------------------------------------------------------- 7: nothing else moves

def test_a_query_moves_nothing_else(scvod, batch):
    poses = np.zeros((batch["n_scans"], 6), F)
    m = scvod.StaticMap(1 << 14, leaf=0.2, kind=scvod.MAP_KIND_LABELLED)
    ctx = batch["ctx"]
    arena = ctx.arena_bytes()
    import torch
    lab = torch.full((len(batch["x"]),), 3, dtype=torch.uint8, device="cuda")
    lab[3000] = lab[3955] = 0                                                            # the two points without a cell are not offered
    m.accumulate_labelled(batch["d"], lab, batch["offs"], poses, [3])
    before = (m.scratch_bytes(), m.count(), *mr.sorted_records(m))
    assert m.query_scratch_bytes() == 0
    m.query_batch(ctx, poses, mq.R_MAX, [3], ALL)
    m.query(batch["d"], batch["offs"], poses, 0.0, None, CELL_ONLY)
    st = m.query_stats()
    after = (m.scratch_bytes(), m.count(), *mr.sorted_records(m))
    assert before[:2] == after[:2] and np.array_equal(before[2], after[2]) and np.array_equal(before[3], after[3])
    assert ctx.arena_bytes() == arena and 0 < m.query_scratch_bytes() <= 64
    assert st["cell"] == len(batch["x"]) - 2 and st["out"] == 2                          # every point that has a cell is in the map it filled
    assert m.count() == before[1]                                                        # (and no insertion error appeared)
    m.close()
