"""scvod_esf_device / scvod_batch_object_esf / scvod_esf_stats on the device, through the C-ABI: one 64-byte record and one 640-value
signature per object against the CPU helper (tests/helpers/object_esf_ref.py: a sequential C++ loop over the object's points and
samples in the library's esf_* functions).  All counters are integers and the maxima exact, so every comparison with the helper is
on the raw bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import object_esf_ref as oer  # noqa: E402
from test_gpu_async_chain import MAP_CELLS, Batch, _batch, _everything, _new_ctx, _same, _stream, _track, _transforms  # noqa: E402
from test_gpu_export import _labels, _tracked  # noqa: E402
from test_gpu_object_shapes import BLOCKS, Shp, _crafted, _crafted_scan, _ground, _prepared  # noqa: E402
from test_gpu_objects import GUARD, NO_TRACK, Tab, _full  # noqa: E402

pytestmark = pytest.mark.gpu

CACHE = 3584  # SCVOD_ESF_CACHE_POINTS
REC, SIG = 64, 640


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return oer.build(tmp_path_factory.mktemp("objesfref"))


class Esf:
    """output buffers of one ESF call with a guard region behind `cap` records / signatures"""

    def __init__(self, cap, sig=True):
        import torch
        self.cap = cap
        self.rec = torch.full(((cap + GUARD) * REC,), 0xA5, dtype=torch.uint8, device="cuda")
        self.sig = torch.full(((cap + GUARD) * SIG * 4,), 0xA5, dtype=torch.uint8, device="cuda") if sig else None

    def _sig(self):
        return C.c_void_p(self.sig.data_ptr()) if self.sig is not None else None

    def device(self, ctx, xyzi, begin, params=None, stream=None):
        return ctx.lib.scvod_esf_device(ctx.h, C.c_void_p(xyzi.data_ptr()), C.c_void_p(begin.data_ptr()), begin.numel() - 1,
                                        C.byref(params) if params is not None else None, C.c_void_p(self.rec.data_ptr()), self._sig(),
                                        int(self.cap), C.c_void_p(stream or 0))

    def batch(self, ctx, params=None, stream=None):
        return ctx.lib.scvod_batch_object_esf(ctx.h, C.byref(params) if params is not None else None, C.c_void_p(self.rec.data_ptr()),
                                              self._sig(), int(self.cap), C.c_void_p(stream or 0))

    def host(self):
        """(record bytes [cap * 64], signature bytes [cap * 2560] or None); asserts the guard regions"""
        raw = self.rec.cpu().numpy()
        assert (raw[self.cap * REC:] == 0xA5).all(), "records were written at or behind cap"
        sig = None
        if self.sig is not None:
            sig = self.sig.cpu().numpy()
            assert (sig[self.cap * SIG * 4:] == 0xA5).all(), "signatures were written at or behind cap"
            sig = sig[:self.cap * SIG * 4]
        return raw[:self.cap * REC], sig


def _estats(ctx):
    out = np.zeros(8, np.int64)
    rc = ctx.lib.scvod_esf_stats(ctx.h, out.ctypes.data_as(C.c_void_p))
    return rc, out.tolist()


def _cloud(objs):
    """(xyzi device tensor, begin device tensor) of a list of [n, 3] objects, with an intensity column the stage does not read"""
    import torch
    begin = np.concatenate([[0], np.cumsum([len(o) for o in objs])]).astype(np.int32)
    xyz = np.concatenate([np.asarray(o, np.float32).reshape(-1, 3) for o in objs] + [np.zeros((1, 3), np.float32)])
    xyzi = np.column_stack([xyz, np.arange(len(xyz), dtype=np.float32)]).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(xyzi)).cuda(), torch.from_numpy(begin).cuda()


def _want(ref, objs, p):
    rec, sig = np.zeros(len(objs), oer.OBJECT_ESF_DTYPE), np.zeros((len(objs), SIG), np.float32)
    for o, x in enumerate(objs):
        r = oer.esf(ref, x, p.samples, p.seed, p.min_points)
        rec[o], sig[o] = r["record"], r["sig"]
    return rec, sig


def _compare(got, want, what):
    got_rec, got_sig = got
    rec, sig = want
    g = got_rec.view(oer.OBJECT_ESF_DTYPE)
    same = (got_rec.reshape(-1, REC) == oer.bits(rec).reshape(-1, REC)).all(axis=1)
    assert same.all(), f"{what}: {int((~same).sum())} of {len(rec)} records differ from the helper, first {int(np.argmin(same))}: " \
                       f"{g[int(np.argmin(same))]} != {rec[int(np.argmin(same))]}"
    if got_sig is not None:
        same = (got_sig.reshape(-1, SIG * 4) == oer.bits(sig).reshape(-1, SIG * 4)).all(axis=1)
        assert same.all(), f"{what}: the signatures of {np.nonzero(~same)[0][:8]} differ from the helper"


def _want_stats(rec, k_all=None, masked=0, uncached=0):
    k = len(rec)
    return [k, k if k_all is None else k_all, int((rec["flags"] != 0).sum()), int(k_all is not None and k_all > k), int(rec["n_valid"].sum()),
            masked, uncached, 0]


def _objects():
    """the crafted objects, every class of point count, and an empty run"""
    rng = np.random.default_rng(5)
    objs = list(oer.esf_cases().values())
    for n in (3, 63, 64, 65, CACHE, CACHE + 1):
        objs.append((rng.random((n, 3)).astype(np.float32) - np.float32(0.5)) * np.asarray([1.5, 0.8, 1.1], np.float32) + np.asarray([-4, 9, 0.5], np.float32))
    objs.insert(5, np.zeros((0, 3), np.float32))
    return objs


@pytest.fixture(scope="module")
def ctx0(scvod):
    """a ctx that never saw a batch: the device form needs none"""
    ctx = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    yield ctx
    ctx.close()


# ---- (a) the crafted objects in one call ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("samples", [1, 63, 64, 65, 257, 2000])
def test_crafted_objects_in_one_call_against_the_helper(scvod, ref, ctx0, samples):
    import torch
    objs = _objects()
    xyzi, begin = _cloud(objs)
    p = scvod.esf_params_default(samples=samples, seed=samples * 7 + 1)
    e = Esf(len(objs))
    torch.cuda.synchronize()
    assert e.device(ctx0, xyzi, begin, p) == 0, ctx0.lib.scvod_last_error(ctx0.h)
    rc, st = _estats(ctx0)
    want = _want(ref, objs, p)
    _compare(e.host(), want, f"{samples} samples")
    n = np.asarray([len(o) for o in objs])
    assert (n > CACHE).sum() == 2 and (n == CACHE).any(), "one object at the cache limit, two above it"
    assert rc == 0 and st == _want_stats(want[0], uncached=int((n > CACHE).sum())), (rc, st)
    assert want[0]["flags"].tolist().count(2) == 2 and 4 in want[0]["flags"] and (want[0]["n_points"] == n).all()
    if samples == 2000:
        assert 1 in want[0]["flags"] and (want[0]["flags"] == 0).sum() >= 10
        # without the signatures, through the shim, and a cls_mask that the device form does not read
        d = torch.zeros((len(objs), REC), dtype=torch.uint8, device="cuda")
        p.cls_mask = 0
        torch.cuda.synchronize()
        ctx0.esf_device(xyzi, begin, d, params=p)
        assert ctx0.esf_stats() == dict(written=st[0], objects=st[1], flagged=st[2], overflow=False, valid_samples=st[4], masked=0, uncached=2)
        assert np.array_equal(d.cpu().numpy().reshape(-1), oer.bits(want[0]))
        sg = torch.zeros((len(objs), SIG), dtype=torch.float32, device="cuda")
        ctx0.esf_device(xyzi, begin, d, sg, params=p)
        torch.cuda.synchronize()
        assert np.array_equal(sg.cpu().numpy().view(np.uint32), want[1].view(np.uint32))


# ---- (b) PCL's sample count -----------------------------------------------------------------------------------------------------

def test_twenty_thousand_samples(scvod, ref, ctx0):
    import torch
    cases = oer.esf_cases()
    objs = [cases["block"], cases["plate"], cases["clumps"]]
    xyzi, begin = _cloud(objs)
    e = Esf(len(objs))
    torch.cuda.synchronize()
    assert e.device(ctx0, xyzi, begin, None) == 0, ctx0.lib.scvod_last_error(ctx0.h)   # NULL: the defaults
    rc, st = _estats(ctx0)
    want = _want(ref, objs, scvod.esf_params_default())
    _compare(e.host(), want, "20000 samples")
    assert rc == 0 and st == _want_stats(want[0], uncached=1)
    assert (want[0]["n_valid"] >= 0.85 * 20000).all() and (want[0]["flags"] == 0).all()


# ---- (c) the batch form -----------------------------------------------------------------------------------------------------------

def _members(b, rec, mem):
    return [b.x[b.offs[r["scan"]] + mem[r["point_begin"]:r["point_begin"] + r["n_points"]]][:, :3] for r in rec]


def test_batch_form_on_the_crafted_scan_and_the_class_mask(scvod, ref):
    import torch
    b = _crafted(scvod)
    ctx = _prepared(scvod, b)
    assert ctx.esf_scratch_bytes() == 0
    rec, offs, mem, _ = _full(ctx, b, NO_TRACK)
    k = len(rec)
    first = rec["n_points"][rec["scan"] == 0]
    assert sorted(first.tolist()) == sorted(n for n, _, _ in BLOCKS), "the crafted blocks are not the objects of scan 0"
    objs = _members(b, rec, mem)
    p = scvod.esf_params_default(samples=384, seed=9)
    e = Esf(k)
    torch.cuda.synchronize()
    assert e.batch(ctx, p) == 0, ctx.lib.scvod_last_error(ctx.h)
    rc, st = _estats(ctx)
    want = _want(ref, objs, p)
    full = e.host()
    _compare(full, want, "crafted batch")
    assert rc == 0 and st == _want_stats(want[0], uncached=int((rec["n_points"] > CACHE).sum())) and st[6] >= 1
    # (the pole of no width is no exact zero here: at this scale the rounding of a + b against c leaves Heron products above 0.001;
    # the integer points of the device form's x-axis object are the exact case)
    assert (want[0]["flags"] == 0).sum() > k // 2
    # one class alone: the rest carries bit 3 and is counted, the selected records are those of the full run
    classes, counts = np.unique(rec["cls"], return_counts=True)
    assert len(classes) >= 2, "one class alone in the batch: the mask shows nothing"
    c = int(classes[np.argmax(counts)])
    p.cls_mask = 1 << c
    m = Esf(k)
    torch.cuda.synchronize()
    assert m.batch(ctx, p) == 0
    rc, stm = _estats(ctx)
    sel = rec["cls"] == c
    mrec = want[0].copy()
    msig = want[1].copy()
    mrec[~sel] = np.zeros(1, oer.OBJECT_ESF_DTYPE)[0]
    mrec["n_points"] = rec["n_points"]
    mrec["flags"][~sel] = 8
    msig[~sel] = 0
    _compare(m.host(), (mrec, msig), "masked batch")
    assert rc == 0 and stm == _want_stats(mrec, masked=int((~sel).sum()), uncached=int(((rec["n_points"] > CACHE) & sel).sum())), (rc, stm)
    # the shim's form, without signatures
    d = torch.zeros((k, REC), dtype=torch.uint8, device="cuda")
    p.cls_mask = 0xFFFFFFFF
    torch.cuda.synchronize()
    ctx.batch_object_esf(d, params=p)
    assert ctx.esf_stats()["written"] == k
    assert np.array_equal(d.cpu().numpy().reshape(-1), full[0])
    ctx.close()


# ---- (d) capacity ---------------------------------------------------------------------------------------------------------------

def test_capacity_latch_and_guard_regions(scvod, ref, ctx0):
    import torch
    cases = oer.esf_cases()
    objs = [cases[n] for n in ("plate", "two", "block30", "clumps", "xaxis", "three")]
    k = len(objs)
    xyzi, begin = _cloud(objs)
    p = scvod.esf_params_default(samples=300, seed=4)
    want = _want(ref, objs, p)
    f = Esf(k)
    torch.cuda.synchronize()
    assert f.device(ctx0, xyzi, begin, p) == 0
    assert _estats(ctx0) == (0, _want_stats(want[0]))
    full = f.host()
    _compare(full, want, "full run")
    for cap in (k - 1, 1, 0):
        e = Esf(cap)
        torch.cuda.synchronize()
        assert e.device(ctx0, xyzi, begin, p) == 0
        rc, st = _estats(ctx0)
        assert rc == -4 and st == _want_stats(want[0][:cap], k_all=k), (cap, rc, st)
        with pytest.raises(scvod.ScvodError):
            ctx0.esf_stats()
        r, s = e.host()                                                     # (host() asserts both guard regions)
        assert np.array_equal(r, full[0][:cap * REC]) and np.array_equal(s, full[1][:cap * SIG * 4]), cap
        again = Esf(k)                                                      # the latch belongs to the LAST call
        torch.cuda.synchronize()
        assert again.device(ctx0, xyzi, begin, p) == 0 and _estats(ctx0) == (0, _want_stats(want[0]))
        assert np.array_equal(again.host()[0], full[0])
    big = Esf(k + 5)
    torch.cuda.synchronize()
    assert big.device(ctx0, xyzi, begin, p) == 0 and _estats(ctx0) == (0, _want_stats(want[0]))
    r, s = big.host()
    assert (r[k * REC:] == 0xA5).all() and (s[k * SIG * 4:] == 0xA5).all() and np.array_equal(r[:k * REC], full[0])


# ---- (e) state and argument errors of the batch form ----------------------------------------------------------------------------

def test_state_and_argument_errors(scvod):
    import torch
    b = _batch(scvod, "K6")
    n = int(b.offs[-1])
    ctx = _new_ctx(scvod, [b])
    p = scvod.esf_params_default(samples=8)
    e = Esf(n, sig=False)
    cnt = Tab(b, 0, 0, members=False, points=False)
    t = Tab(b, n, n)
    torch.cuda.synchronize()

    def call():
        return e.batch(ctx, p)
    assert _estats(ctx)[0] == -5                                            # before the first call
    assert call() == -5                                                     # no batch, no table
    ctx.batch_process(b.d, b.offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    assert call() == -5                                                     # a batch, but no table yet
    assert cnt.call(ctx, NO_TRACK, records=False) == 0
    assert call() == -5                                                     # a count-only table is none
    assert t.call(ctx, NO_TRACK) == 0 and call() == 0 and _estats(ctx)[0] == 0
    assert cnt.call(ctx, NO_TRACK, records=False) == 0 and call() == 0      # a count-only call later leaves the lists as they are
    assert ctx.lib.scvod_batch_object_esf(ctx.h, C.byref(p), None, None, n, None) == -1
    assert ctx.lib.scvod_batch_object_esf(ctx.h, C.byref(p), C.c_void_p(e.rec.data_ptr()), None, -1, None) == -1
    for bad in (dict(samples=0), dict(samples=65537), dict(min_points=2)):
        assert e.batch(ctx, scvod.esf_params_default(**bad)) == -1, bad
    ctx.batch_cluster_types()                                               # the classes the mask reads may differ from the table's now
    assert call() == -5 and b"scvod_batch_cluster_types ran since" in ctx.lib.scvod_last_error(ctx.h)
    assert t.call(ctx, NO_TRACK) == 0 and call() == 0
    ctx.batch_cluster()                                                     # another clustering: the lists are stale
    assert call() == -5
    ctx.batch_cluster_types()
    assert call() == -5
    _track(ctx, b, b.T, b.nxt, None, 1)
    assert t.call(ctx, 0) == 0 and call() == 0                              # a table that read the tracking result
    ctx.batch_cluster_types()                                               # ... which is stale now: the table's own rule
    assert t.call(ctx, 0) == -1 and call() == -1
    assert t.call(ctx, NO_TRACK) == 0 and call() == 0
    ctx.batch_process(b.d, b.offs)                                          # a new batch
    assert call() == -5
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    assert call() == -5
    torch.cuda.synchronize()
    ctx.close()


def test_argument_errors_of_the_device_form_on_a_ctx(scvod, ctx0):
    """with a real ctx the checks of the arguments themselves decide, not the NULL ctx; nothing is launched by a refused call"""
    import torch
    objs = [oer.esf_cases()["block30"]]
    xyzi, begin = _cloud(objs)
    e = Esf(1)
    good = scvod.esf_params_default(samples=16)
    torch.cuda.synchronize()
    lib, h = ctx0.lib, ctx0.h
    x, bg, r, sg = (C.c_void_p(t.data_ptr()) for t in (xyzi, begin, e.rec, e.sig))
    assert lib.scvod_esf_device(h, x, bg, 1, C.byref(good), r, sg, 1, None) == 0
    assert _estats(ctx0) == (0, [1, 1, 0, 0, _estats(ctx0)[1][4], 0, 0, 0])
    before = e.host()[0].copy()
    for bad in (dict(samples=0), dict(samples=65537), dict(samples=-5), dict(min_points=2), dict(min_points=-1)):
        assert lib.scvod_esf_device(h, x, bg, 1, C.byref(scvod.esf_params_default(**bad)), r, sg, 1, None) == -1, bad
    assert lib.scvod_esf_device(h, None, bg, 1, C.byref(good), r, sg, 1, None) == -1
    assert lib.scvod_esf_device(h, x, None, 1, C.byref(good), r, sg, 1, None) == -1
    assert lib.scvod_esf_device(h, x, bg, -1, C.byref(good), r, sg, 1, None) == -1
    assert lib.scvod_esf_device(h, x, bg, 1, C.byref(good), None, sg, 1, None) == -1
    assert lib.scvod_esf_device(h, x, bg, 1, C.byref(good), r, sg, -1, None) == -1
    assert lib.scvod_esf_device(h, C.c_void_p(xyzi.data_ptr() + 4), bg, 1, C.byref(good), r, sg, 1, None) == -1, "d_xyzi: 16-byte aligned"
    assert lib.scvod_esf_device(h, x, C.c_void_p(begin.data_ptr() + 2), 1, C.byref(good), r, sg, 1, None) == -1
    assert lib.scvod_esf_device(h, x, bg, 1, C.byref(good), C.c_void_p(e.rec.data_ptr() + 1), sg, 1, None) == -1
    assert lib.scvod_esf_device(h, x, bg, 1, C.byref(good), r, C.c_void_p(e.sig.data_ptr() + 2), 1, None) == -1
    assert lib.scvod_esf_stats(h, None) == -1
    assert lib.scvod_esf_device(h, None, None, 0, C.byref(good), r, sg, 1, None) == 0, "no objects need no cloud"
    assert _estats(ctx0) == (0, [0] * 8)
    assert np.array_equal(e.host()[0], before), "a refused call and a call on no objects write nothing"


# ---- (f) stream order -----------------------------------------------------------------------------------------------------------

def test_behind_the_whole_chain_on_a_side_stream_across_two_batches(scvod, ref):
    import torch
    b1, b2 = _batch(scvod, "D"), _batch(scvod, "B")
    stream = _stream()
    st = stream.cuda_stream
    p = scvod.esf_params_default(samples=200, seed=77)
    runs = []
    for _ in range(2):
        ctx = _new_ctx(scvod, [b1, b2])
        tabs = [Tab(b, int(b.offs[-1]), int(b.offs[-1])) for b in (b1, b2)]
        esfs = [Esf(int(b.offs[-1]) // 8) for b in (b1, b2)]
        torch.cuda.synchronize()
        keep = []
        for b, t, e in zip((b1, b2), tabs, esfs):
            offs_h, T, nxt = b.offs.copy(), b.T.copy(), b.nxt.copy()
            ctx.batch_process(b.d, offs_h, stream=st, sync=False)
            ctx.batch_cluster(stream=st, sync=False)
            ctx.batch_cluster_types(stream=st, sync=False)
            keep.append(_track(ctx, b, T, nxt, st, 0))
            assert t.call(ctx, 0, st) == 0, ctx.lib.scvod_last_error(ctx.h)
            assert e.batch(ctx, p, st) == 0, ctx.lib.scvod_last_error(ctx.h)
        stream.synchronize()
        rc, stt = _estats(ctx)
        assert rc == 0
        out = []
        for b, t, e in zip((b1, b2), tabs, esfs):
            rec, offs, mem, _ = t.host(b)
            k = int(offs[-1])
            assert 0 < k <= e.cap
            r, s = e.host()
            assert (r[k * REC:] == 0xA5).all() and (s[k * SIG * 4:] == 0xA5).all(), "something was written behind the last record"
            out.append((b, rec[:k], mem, r[:k * REC].copy(), s[:k * SIG * 4].copy()))
        assert stt[0] == stt[1] == len(out[1][1])
        runs.append(out)
        ctx.close()
    # two calls of one ctx on two streams share its counters and scratch: the later one waits for the earlier on the device
    cases = oer.esf_cases()
    objs = [cases["block"], cases["plate"], cases["block30"]] * 8
    xyzi, begin = _cloud(objs)
    q1, q2 = scvod.esf_params_default(samples=4000, seed=1), scvod.esf_params_default(samples=3000, seed=2)
    ctx = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    e1, e2 = Esf(len(objs)), Esf(len(objs))
    other = _stream()
    torch.cuda.synchronize()
    assert e1.device(ctx, xyzi, begin, q1, st) == 0 and e2.device(ctx, xyzi, begin, q2, other.cuda_stream) == 0
    assert _estats(ctx)[0] == 0
    torch.cuda.synchronize()
    _compare(e1.host(), _want(ref, objs, q1), "the first of two calls on two streams")
    _compare(e2.host(), _want(ref, objs, q2), "the second of two calls on two streams")
    ctx.close()
    for (b, rec, mem, r, s), (_, _, _, r2, s2) in zip(runs[0], runs[1]):
        assert np.array_equal(r, r2) and np.array_equal(s, s2), f"{b.name}: two runs differ"
        _compare((r, s), _want(ref, _members(b, rec, mem), p), f"{b.name} on the side stream")


# ---- (g) no side effects --------------------------------------------------------------------------------------------------------

def test_the_descriptor_changes_nothing_else(scvod):
    import torch
    b = _batch(scvod, "D")
    ctx = _tracked(scvod, b)
    table = _full(ctx, b)
    k = len(table[0])
    before_map = scvod.StaticMap(MAP_CELLS)
    before_map.accumulate(ctx, b.poses)
    want_all, _ = _everything(ctx, b, before_map)
    lab = _labels(ctx, b)
    t = Tab(b, int(b.offs[-1]), int(b.offs[-1]))
    torch.cuda.synchronize()
    assert t.call(ctx) == 0
    torch.cuda.synchronize()
    raw = [x.cpu().numpy().copy() for x in (t.rec, t.offs, t.mem, t.pobj)]
    shp = Shp(k)
    assert shp.call(ctx) == 0
    torch.cuda.synchronize()
    shapes = shp.host().copy()
    arena, scratch = ctx.arena_bytes(), ctx.batch_objects_scratch_bytes()
    assert ctx.esf_scratch_bytes() == 0, "nothing is allocated before the first call"
    p = scvod.esf_params_default(samples=100)
    one, two = Esf(k), Esf(k)
    assert one.batch(ctx, p) == 0 and two.batch(ctx, p) == 0
    assert _estats(ctx)[0] == 0
    assert all(np.array_equal(x, y) for x, y in zip(one.host(), two.host())), "two consecutive calls differ"
    grown = ctx.esf_scratch_bytes()
    assert grown > 0 and two.batch(ctx, p) == 0 and ctx.esf_scratch_bytes() == grown, "grow-only, and steady at the same request"
    for x, y in zip(raw, (t.rec, t.offs, t.mem, t.pobj)):
        assert np.array_equal(x, y.cpu().numpy()), "the table's buffers changed"
    assert ctx.arena_bytes() == arena
    assert ctx.batch_objects_scratch_bytes() == scratch, "the table's scratch is not the ESF stage's"
    shp2 = Shp(k)
    assert shp2.call(ctx) == 0
    torch.cuda.synchronize()
    assert np.array_equal(shp2.host(), shapes), "the shapes before and after"
    assert np.array_equal(_labels(ctx, b), lab)
    after_map = scvod.StaticMap(MAP_CELLS)
    after_map.accumulate(ctx, b.poses)
    got_all, _ = _everything(ctx, b, after_map)
    _same(got_all, want_all, "fetches and map records after the descriptor")
    for x, y in zip(_full(ctx, b), table):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    before_map.close()
    after_map.close()
    ctx.close()


# ---- (h) an object's descriptor does not depend on the batch around it ----------------------------------------------------------

def test_the_same_object_in_two_batches(scvod):
    import torch
    b = _crafted(scvod)
    scans = [_ground(np.random.default_rng(23)).astype(np.float32), _crafted_scan()]   # the blocks' scan behind another, alone
    x = np.ascontiguousarray(np.concatenate(scans), np.float32)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    poses, nxt = np.zeros((2, 6), np.float32), np.full(2, -1, np.int32)
    other = Batch(name="CRAFTED2", kind="K64", P=b.P, d=torch.from_numpy(x).cuda().contiguous(), x=x, offs=offs, poses=poses, nxt=nxt,
                  T=_transforms(scvod, poses, nxt), n=2, ext=None, dyn_from_solo=())
    p = scvod.esf_params_default(samples=500, seed=3)
    got = []
    for bb, scan in ((b, 0), (other, 1)):
        ctx = _prepared(scvod, bb)
        rec, _, _, _ = _full(ctx, bb, NO_TRACK)
        e = Esf(len(rec))
        torch.cuda.synchronize()
        assert e.batch(ctx, p) == 0 and _estats(ctx)[0] == 0
        r, s = e.host()
        mine = np.nonzero(rec["scan"] == scan)[0]
        assert sorted(rec["n_points"][mine].tolist()) == sorted(n for n, _, _ in BLOCKS)
        order = mine[np.argsort(rec["n_points"][mine])]                     # (the blocks' point counts all differ)
        got.append((r.reshape(-1, REC)[order], s.reshape(-1, SIG * 4)[order]))
        ctx.close()
    assert got[0][0].shape == got[1][0].shape == (len(BLOCKS), REC)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert (got[0][0].view(oer.OBJECT_ESF_DTYPE)["n_valid"] > 0).sum() >= len(BLOCKS) - 1
