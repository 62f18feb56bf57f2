"""scvod_batch_object_shapes / scvod_batch_object_shapes_stats on the device, through the C-ABI: one 96-byte record per object of the
table against the CPU helper (tests/helpers/object_shape_ref.py: a sequential C++ loop over the object's points in the library's
arithmetic), fed the member points the table itself lists.  Every comparison with the helper is bit for bit on the raw record bytes,
every NaN counted as one pattern."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import object_shape_ref as osr  # noqa: E402
from test_gpu_async_chain import MAP_CELLS, MERGE, Batch, _batch, _everything, _new_ctx, _same, _sorted_records, _stream, _track, _transforms  # noqa: E402
from test_gpu_export import _labels, _step, _tracked  # noqa: E402
from test_gpu_objects import GUARD, NO_TRACK, Tab, _full  # noqa: E402

pytestmark = pytest.mark.gpu

# a tight block of returns above a flat ground: (points, centre x y, extent x y z).  Chosen on the CPU with the oracle (Patchwork ->
# binning -> clustering -> box rules on this very scan): every block comes out as ONE object of exactly its point count
BLOCKS = [(64, (8.0, 2.0), (0.25, 0.25, 0.5)), (128, (0.0, 9.0), (0.3, 0.3, 0.5)), (100, (-8.0, 0.0), (0.25, 0.25, 0.5)),
          (129, (0.0, -9.0), (0.3, 0.3, 0.5)), (30, (6.0, 6.0), (0.2, 0.2, 0.4)), (4500, (-7.0, 7.0), (0.6, 0.6, 1.0)),
          (300, (7.0, -7.0), (1.0, 0.0, 0.8)),       # a vertical plate: planar
          (40, (-6.0, -6.0), (0.0, 0.0, 0.8)),       # a vertical pole of no width: collinear
          (193, (12.0, 3.0), (0.3, 0.3, 0.5))]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return osr.build(tmp_path_factory.mktemp("objshaperef"))


def _ground(rng):
    g = rng.uniform(-25, 25, (30000, 2))
    r = np.hypot(g[:, 0], g[:, 1])
    g = g[(r > 2.0) & (r < 28)]
    return np.column_stack([g, -1.73 + rng.normal(0, 0.01, len(g)), rng.uniform(0, 100, len(g))])


def _crafted_scan(seed=7):
    rng = np.random.default_rng(seed)
    pts = [_ground(rng)]
    for n, (cx, cy), (dx, dy, dz) in BLOCKS:
        pts.append(np.column_stack([cx + rng.uniform(-.5, .5, n) * dx, cy + rng.uniform(-.5, .5, n) * dy,
                                    -0.6 + rng.uniform(-.5, .5, n) * dz, rng.uniform(0, 100, n)]))
    x = np.concatenate(pts).astype(np.float32)
    return x[rng.permutation(len(x))]


_CRAFTED = {}


def _crafted(scvod):
    """scan 0: the blocks; 1: empty; 2: ground alone, no object; 3: a scan of the K64 kind"""
    if "b" in _CRAFTED:
        return _CRAFTED["b"]
    import synth
    import torch
    real = synth.make_scan(5, 300, "K64", device="cuda")[0].cpu().numpy()
    scans = [_crafted_scan(), np.zeros((0, 4), np.float32), _ground(np.random.default_rng(11)).astype(np.float32), real]
    x = np.ascontiguousarray(np.concatenate(scans), np.float32)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    poses = np.zeros((len(scans), 6), np.float32)
    nxt = np.full(len(scans), -1, np.int32)
    d = torch.from_numpy(x).cuda().contiguous()
    torch.cuda.synchronize()
    b = Batch(name="CRAFTED", kind="K64", P=scvod.make_params("semantickitti"), d=d, x=x, offs=offs, poses=poses, nxt=nxt,
              T=_transforms(scvod, poses, nxt), n=len(scans), ext=None, dyn_from_solo=())
    _CRAFTED["b"] = b
    return b


class Shp:
    """output buffer of one scvod_batch_object_shapes call with a guard region behind `cap` records"""

    def __init__(self, cap):
        import torch
        self.cap = cap
        self.buf = torch.full(((cap + GUARD) * 96,), 0xA5, dtype=torch.uint8, device="cuda")

    def call(self, ctx, stream=None):
        return ctx.lib.scvod_batch_object_shapes(ctx.h, C.c_void_p(self.buf.data_ptr()), int(self.cap), C.c_void_p(stream or 0))

    def host(self):
        raw = self.buf.cpu().numpy()
        assert (raw[self.cap * 96:] == 0xA5).all(), "shape records were written at or behind cap_shapes"
        return raw[:self.cap * 96]


def _sstats(ctx):
    out = np.zeros(4, np.int64)
    rc = ctx.lib.scvod_batch_object_shapes_stats(ctx.h, out.ctypes.data_as(C.c_void_p))
    return rc, out.tolist()


def _shapes(ctx, k, stream=None):
    """one call into a buffer of exactly k records, synchronised: (records, stats)"""
    import torch
    s = Shp(k)
    torch.cuda.synchronize()
    assert s.call(ctx, stream) == 0, ctx.lib.scvod_last_error(ctx.h)
    rc, st = _sstats(ctx)
    assert rc == 0 and st[0] == st[1] == k and st[3] == 0, (rc, st, k)
    return s.host().view(osr.OBJECT_SHAPE_DTYPE).copy(), st


def _helper(ref, b, rec, mem, K=osr.DEFAULT_K):
    """the helper's record of every object of the table, from the INPUT points its member list names"""
    out = np.zeros(len(rec), osr.OBJECT_SHAPE_DTYPE)
    for o, r in enumerate(rec):
        m = mem[r["point_begin"]:r["point_begin"] + r["n_points"]]
        out[o] = osr.shape(ref, b.x[b.offs[r["scan"]] + m][:, :3], K)
    return out


def _check(ref, b, rec, mem, got, st, what, K=osr.DEFAULT_K):
    want = _helper(ref, b, rec, mem, K)
    same = (osr.bits(got).reshape(-1, 96) == osr.bits(want).reshape(-1, 96)).all(axis=1)
    assert same.all(), f"{what}: {int((~same).sum())} of {len(rec)} records differ from the helper, first {int(np.argmin(same))}: " \
                       f"{got[int(np.argmin(same))]} != {want[int(np.argmin(same))]}"
    assert st[2] == int((want["flags"] & 1).sum()), f"{what}: the count of records with a feature that is not finite"
    return want


def _prepared(scvod, b, setup=None):
    """Patchwork, clustering and types of b on a fresh ctx: what a table with SCVOD_OBJ_NO_TRACK needs"""
    ctx = _new_ctx(scvod, [b], setup)
    ctx.batch_process(b.d, b.offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    return ctx


# ---- 1. every class of run length -------------------------------------------------------------------------------------------------------

def test_every_class_of_run_length_against_the_helper(scvod, ref):
    b = _crafted(scvod)
    ctx = _prepared(scvod, b)
    rec, offs, mem, _ = _full(ctx, b, NO_TRACK)
    n = rec["n_points"]
    first = n[rec["scan"] == 0]
    assert sorted(first.tolist()) == sorted(k for k, _, _ in BLOCKS), "the crafted blocks are not the objects of scan 0"
    assert offs[1] == offs[2] == offs[3] == len(first) and offs[4] > offs[3], "an empty scan, a scan without objects, a scan with objects"
    for what, ok in (("fewer than 64 members", (n < 64).any()), ("exactly 64", (n == 64).any()), ("exactly 128", (n == 128).any()),
                     ("65..127", ((n > 64) & (n < 128)).any()), ("a multiple of 64 plus 1", ((n % 64 == 1) & (n > 64)).any()),
                     ("at least 4096", (n >= 4096).any())):
        assert ok, f"no object with {what} in the batch"
    got, st = _shapes(ctx, len(rec))
    want = _check(ref, b, rec, mem, got, st, "crafted")
    e = got["eig"]
    plate, pole = got[(rec["scan"] == 0) & (n == 300)][0], got[(rec["scan"] == 0) & (n == 40)][0]
    assert plate["eig"][0] < 1e-4 * plate["eig"][2] and plate["eig"][1] > 0.1 * plate["eig"][2], "the plate is not planar"
    assert pole["eig"][1] < 1e-4 * pole["eig"][2] and pole["eig"][2] > 0, "the pole is not collinear"
    assert pole["flags"] & 1 and st[2] >= 1, "a collinear cluster divides by a zero eigenvalue: flagged and counted"
    assert (got["flags"] & 2).tolist() == (n < 3).tolist()
    assert (np.diff(e, axis=1) >= 0).all() and (e >= 0).all()
    ok = got["flags"] == 0
    assert ok.sum() > len(rec) // 2 and np.isfinite(got["feat"][ok]).all() and (want["flags"] == got["flags"]).all()
    # the shim's form
    import torch
    d = torch.zeros((len(rec), 96), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.batch_object_shapes(d)
    assert ctx.batch_object_shapes_stats() == dict(written=len(rec), objects=len(rec), not_finite=st[2], overflow=False)
    assert np.array_equal(d.cpu().numpy().reshape(-1), got.view(np.uint8))
    # a table that asked for members alone serves too; the caller's offsets and records of the table call are not read again
    t = Tab(b, 0, int(b.offs[-1]), points=False)
    torch.cuda.synchronize()
    assert t.call(ctx, NO_TRACK, records=False) == 0
    torch.cuda.synchronize()
    t.offs.fill_(-1)
    t.mem.fill_(-1)
    again, _ = _shapes(ctx, len(rec))
    assert np.array_equal(again.view(np.uint8), got.view(np.uint8))
    ctx.close()


# ---- 2. capacity ---------------------------------------------------------------------------------------------------------------------------

def test_capacity_latch_and_guard_regions(scvod, ref):
    import torch
    b = _batch(scvod, "K6")
    ctx = _tracked(scvod, b)
    rec, offs, mem, _ = _full(ctx, b)
    k = len(rec)
    assert k > 2
    full, st = _shapes(ctx, k)
    _check(ref, b, rec, mem, full, st, "K6")
    for cap in (k - 1, k // 2, 1, 0):
        s = Shp(cap)
        torch.cuda.synchronize()
        assert s.call(ctx) == 0
        rc, got = _sstats(ctx)
        assert rc == -4 and got == [cap, k, int((full["flags"][:cap] & 1).sum()), 1], (cap, rc, got)
        with pytest.raises(scvod.ScvodError):
            ctx.batch_object_shapes_stats()
        assert np.array_equal(s.host(), full[:cap].view(np.uint8)), cap     # (host() asserts the guard region)
        again, st2 = _shapes(ctx, k)                                        # the latch belongs to the LAST call
        assert st2 == st and np.array_equal(again.view(np.uint8), full.view(np.uint8))
    big = Shp(k + 37)                                                       # nothing behind the last record either
    torch.cuda.synchronize()
    assert big.call(ctx) == 0 and _sstats(ctx) == (0, st)
    assert (big.host()[k * 96:] == 0xA5).all() and np.array_equal(big.host()[:k * 96], full.view(np.uint8))
    ctx.close()


# ---- 3. state and argument errors ----------------------------------------------------------------------------------------------------------

def test_state_and_argument_errors(scvod):
    import torch
    b = _batch(scvod, "K6")
    n = int(b.offs[-1])
    ctx = _new_ctx(scvod, [b])
    s = Shp(n)
    cnt = Tab(b, 0, 0, members=False, points=False)
    t = Tab(b, n, n)
    torch.cuda.synchronize()
    assert _sstats(ctx)[0] == -5                                            # before the first call
    assert s.call(ctx) == -5                                                # no batch, no table
    ctx.batch_process(b.d, b.offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    assert s.call(ctx) == -5                                                # a batch, but no table yet
    assert cnt.call(ctx, NO_TRACK, records=False) == 0
    assert s.call(ctx) == -5                                                # a count-only table is none
    assert t.call(ctx, NO_TRACK) == 0 and s.call(ctx) == 0 and _sstats(ctx)[0] == 0
    assert cnt.call(ctx, NO_TRACK, records=False) == 0 and s.call(ctx) == 0  # a count-only call later leaves the lists as they are
    assert ctx.lib.scvod_batch_object_shapes(ctx.h, None, n, None) == -1
    assert ctx.lib.scvod_batch_object_shapes(ctx.h, C.c_void_p(s.buf.data_ptr()), -1, None) == -1
    ctx.batch_cluster()                                                     # another clustering: the lists are stale
    assert s.call(ctx) == -5
    ctx.batch_cluster_types()
    assert s.call(ctx) == -5
    _track(ctx, b, b.T, b.nxt, None, 1)
    assert t.call(ctx, 0) == 0 and s.call(ctx) == 0                         # a table that read the tracking result
    ctx.batch_cluster_types()                                               # ... which is stale now: the table's own rule
    assert t.call(ctx, 0) == -1 and s.call(ctx) == -1
    assert t.call(ctx, NO_TRACK) == 0 and s.call(ctx) == 0
    ctx.batch_process(b.d, b.offs)                                          # a new batch
    assert s.call(ctx) == -5
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    assert s.call(ctx) == -5
    # the constants: every maximum a positive finite number, kOneThird finite
    for bad in (dict(kLinearityMax=0.0), dict(kPlanarityMax=-1.0), dict(kScatteringMax=np.inf), dict(kOmnivarianceMax=np.nan),
                dict(kAnisotropyMax=-np.inf), dict(kEigenEntropyMax=0.0), dict(kChangeOfCurvatureMax=np.nan), dict(kOneThird=np.nan),
                dict(kOneThird=np.inf)):
        p = scvod.feature_params(**bad)
        assert ctx.lib.scvod_set_object_features(ctx.h, C.byref(p)) == -1, bad
    assert ctx.lib.scvod_set_object_features(ctx.h, None) == -1
    torch.cuda.synchronize()
    ctx.close()


# ---- 4. stream order -----------------------------------------------------------------------------------------------------------------------

def test_behind_the_whole_chain_on_a_side_stream_across_two_batches(scvod, ref):
    import torch
    b1, b2 = _batch(scvod, "D"), _batch(scvod, "B")
    stream = _stream()
    st = stream.cuda_stream
    runs = []
    for _ in range(2):
        ctx = _new_ctx(scvod, [b1, b2])
        tabs = [Tab(b, int(b.offs[-1]), int(b.offs[-1])) for b in (b1, b2)]
        shps = [Shp(int(b.offs[-1]) // 8) for b in (b1, b2)]
        torch.cuda.synchronize()
        keep = []
        for b, t, s in zip((b1, b2), tabs, shps):
            offs_h, T, nxt = b.offs.copy(), b.T.copy(), b.nxt.copy()
            ctx.batch_process(b.d, offs_h, stream=st, sync=False)
            ctx.batch_cluster(stream=st, sync=False)
            ctx.batch_cluster_types(stream=st, sync=False)
            keep.append(_track(ctx, b, T, nxt, st, 0))
            assert t.call(ctx, 0, st) == 0, ctx.lib.scvod_last_error(ctx.h)
            assert s.call(ctx, st) == 0, ctx.lib.scvod_last_error(ctx.h)
        stream.synchronize()
        rc, stt = _sstats(ctx)
        assert rc == 0
        out = []
        for b, t, s in zip((b1, b2), tabs, shps):
            rec, offs, mem, _ = t.host(b)
            k = int(offs[-1])
            assert 0 < k <= s.cap
            raw = s.host()
            assert (raw[k * 96:] == 0xA5).all(), "something was written behind the last record"
            out.append((b, rec[:k], mem, raw[:k * 96].view(osr.OBJECT_SHAPE_DTYPE).copy()))
        assert stt[0] == stt[1] == len(out[1][1])
        runs.append(out)
        ctx.close()
    for (b, rec, mem, got), (_, _, _, got2) in zip(runs[0], runs[1]):
        assert np.array_equal(got.view(np.uint8), got2.view(np.uint8)), f"{b.name}: two runs differ"
        _check(ref, b, rec, mem, got, [0, 0, int((got["flags"] & 1).sum()), 0], f"{b.name} on the side stream")


# ---- 5. no side effects --------------------------------------------------------------------------------------------------------------------

def test_the_shapes_change_nothing_else(scvod):
    import torch
    b = _batch(scvod, "D")
    ctx = _tracked(scvod, b)
    table = _full(ctx, b)
    k = len(table[0])
    before_map = scvod.StaticMap(MAP_CELLS)
    before_map.accumulate(ctx, b.poses)
    want_all, _ = _everything(ctx, b, before_map)
    lab = _labels(ctx, b)
    arena, scratch = ctx.arena_bytes(), ctx.batch_objects_scratch_bytes()
    t = Tab(b, int(b.offs[-1]), int(b.offs[-1]))
    torch.cuda.synchronize()
    assert t.call(ctx) == 0
    torch.cuda.synchronize()
    raw = [x.cpu().numpy().copy() for x in (t.rec, t.offs, t.mem, t.pobj)]
    one, _ = _shapes(ctx, k)
    two, _ = _shapes(ctx, k)
    assert np.array_equal(osr.bits(one), osr.bits(two)), "two consecutive calls differ"
    for x, y in zip(raw, (t.rec, t.offs, t.mem, t.pobj)):
        assert np.array_equal(x, y.cpu().numpy()), "the table's buffers changed"
    assert ctx.arena_bytes() == arena
    assert ctx.batch_objects_scratch_bytes() == scratch + 32, "four stats words, documented in include/scvod.h"
    assert np.array_equal(_labels(ctx, b), lab)
    after_map = scvod.StaticMap(MAP_CELLS)
    after_map.accumulate(ctx, b.poses)
    got_all, _ = _everything(ctx, b, after_map)
    _same(got_all, want_all, "fetches and map records after the shapes")
    for x, y in zip(_full(ctx, b), table):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    before_map.close()
    after_map.close()
    ctx.close()


# ---- 6. the intensity merge and the constants ----------------------------------------------------------------------------------------------

def test_shapes_follow_the_merge_and_forget_it_again_and_honour_the_constants(scvod, ref):
    b = _batch(scvod, "D")
    ctx = _tracked(scvod, b)
    rec, _, mem, _ = _full(ctx, b)
    plain, st = _shapes(ctx, len(rec))
    _check(ref, b, rec, mem, plain, st, "plain")
    ctx.set_intensity_merge(*MERGE)
    _step(ctx, b)
    assert ctx.batch_cluster_merge_stats()["fusions"] > 0
    frec, _, fmem, _ = _full(ctx, b)
    assert len(frec) < len(rec), "the merge fused no object: the case shows nothing"
    fused, st = _shapes(ctx, len(frec))
    _check(ref, b, frec, fmem, fused, st, "merge on")
    ctx.set_intensity_merge(0, MERGE[1], MERGE[2], MERGE[3])
    _step(ctx, b)
    rec2, _, mem2, _ = _full(ctx, b)
    back, st = _shapes(ctx, len(rec2))
    assert np.array_equal(osr.bits(back), osr.bits(plain)), "merge off again"
    # other constants
    K = (0.5, 370.0, 959.0 / 4, 1248.0, 0.5, 624.0, 2.0, 0.25)
    ctx.set_object_features(scvod.FeatureParams(*K))
    other, st = _shapes(ctx, len(rec2))
    _check(ref, b, rec2, mem2, other, st, "other constants", K)
    ok = (plain["flags"] == 0) & (other["flags"] == 0)
    assert ok.any() and np.array_equal(other["feat"][ok][:, 0], plain["feat"][ok][:, 0] * 2) and (other["feat"][ok][:, 3] != plain["feat"][ok][:, 3]).any()
    assert np.array_equal(other["eig"], plain["eig"]) and np.array_equal(other["cov"], plain["cov"])
    ctx.set_object_features()                           # the defaults again
    again, _ = _shapes(ctx, len(rec2))
    assert np.array_equal(osr.bits(again), osr.bits(plain))
    ctx.close()
