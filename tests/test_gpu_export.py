"""scvod_batch_point_labels / scvod_batch_export_points / scvod_batch_export_stats on the device, all through the C-ABI: the label
byte of every input point and the compacted scans against the numpy statement of the label table and the keep rule
(tests/helpers/point_labels_ref.py, fed from the existing per-scan fetches of the same ctx), and against the oracle's chain
(oracle_time_sequence: nothing the device computed).  Every comparison is np.array_equal / bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import point_labels_ref as plr  # noqa: E402
from test_gpu_async_chain import MERGE, _batch, _everything, _new_ctx, _same, _stream, _track  # noqa: E402

pytestmark = pytest.mark.gpu

CAR, OTHER = 2, 1
GUARD = 64
NO_GROUND, NO_REJECTED, IGNORE_DYNAMIC = 1, 2, 4
FLAG_SETS = (0, NO_GROUND, NO_REJECTED, NO_GROUND | NO_REJECTED, IGNORE_DYNAMIC)


def _tracked(scvod, b, setup=None):
    ctx = _new_ctx(scvod, [b], setup)
    _step(ctx, b)
    return ctx


def _step(ctx, b, stream=None, sync=1):
    ctx.batch_process(b.d, b.offs, stream=stream, sync=bool(sync))
    ctx.batch_cluster(stream=stream, sync=bool(sync))
    ctx.batch_cluster_types(stream=stream, sync=bool(sync))
    _track(ctx, b, b.T, b.nxt, stream, sync)


def _helper_labels(ctx, b, use_dyn=True):
    """the helper fed from the per-scan fetches: (labels of the batch, dynamic points, dropped points)"""
    out, n_dyn = [], 0
    for s in range(b.n):
        r = ctx.batch_fetch(s)
        ty = ctx.batch_fetch_cluster_types(s, r["n_apri"], car_label=CAR, other_label=OTHER)
        t = ctx.batch_fetch_track(s)
        n_dyn += int(t["n_dynamic_points"])
        assert int((t["pt_dyn"] == 1).sum()) == t["n_dynamic_points"]
        out.append(plr.scan_labels(r["n_points"], r["cls"], r["ground_idx"], r["rejected_src"], r["apri_src"], ty,
                                   t["pt_dyn"] if use_dyn else None, car=CAR))
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), n_dyn


def _labels(ctx, b, flags=0, stream=None):
    """scvod_batch_point_labels into a buffer of exactly the batch's size with a guard region behind it"""
    import torch
    n = int(b.offs[-1])
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx._chk(ctx.lib.scvod_batch_point_labels(ctx.h, C.c_void_p(buf.data_ptr()), n, int(flags), C.c_void_p(stream or 0)))
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[n:] == 0xA5).all(), "scvod_batch_point_labels wrote behind the batch's points"
    return h[:n]


class Out:
    """output buffers of one export with a guard region behind `cap` records"""

    def __init__(self, b, cap, payload=True, src=True):
        import torch
        self.cap = cap
        self.xyzi = torch.full((cap + GUARD, 4), float("nan"), dtype=torch.float32, device="cuda")
        self.src = torch.full((cap + GUARD,), -7, dtype=torch.int32, device="cuda") if src else None
        self.pay = torch.full((cap + GUARD,), -7, dtype=torch.int32, device="cuda") if payload else None
        self.offs = torch.full((b.n + 1 + GUARD,), -7, dtype=torch.int32, device="cuda")

    def call(self, ctx, b, flags, poses=None, d_payload_in=None, stream=None, count_only=False):
        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        pp = None if poses is None else poses.ctypes.data_as(C.c_void_p)
        return ctx.lib.scvod_batch_export_points(ctx.h, int(flags), pp, ptr(d_payload_in), None if count_only else ptr(self.xyzi),
                                                 None if count_only else (ptr(self.pay) if d_payload_in is not None else None),
                                                 None if count_only else ptr(self.src), int(self.cap), ptr(self.offs), C.c_void_p(stream or 0))

    def host(self, b):
        offs = self.offs.cpu().numpy()
        assert (offs[b.n + 1:] == -7).all(), "the offsets were written behind n_scans + 1"
        xyzi = self.xyzi.cpu().numpy()
        assert np.isnan(xyzi[self.cap:]).all(), "records were written behind the capacity"
        src = pay = None
        if self.src is not None:
            src = self.src.cpu().numpy()
            assert (src[self.cap:] == -7).all()
        if self.pay is not None:
            pay = self.pay.cpu().numpy()
            assert (pay[self.cap:] == -7).all()
        return offs[:b.n + 1], xyzi, src, pay


def _stats(ctx):
    out = np.zeros(4, np.int64)
    rc = ctx.lib.scvod_batch_export_stats(ctx.h, out.ctypes.data_as(C.c_void_p))
    return rc, out


def _payload(b):
    import torch
    n = int(b.offs[-1])
    h = ((np.arange(n, dtype=np.int64) * 2654435761) & 0x7FFFFFFF).astype(np.int32)
    return h, torch.from_numpy(h).cuda()


def _check_export(b, lab, flags, offs, xyzi, src, pay, h_pay, want_xyz=None):
    keep = plr.keep_of(lab, flags)
    counts = np.asarray([int(keep[b.offs[s]:b.offs[s + 1]].sum()) for s in range(b.n)], np.int64)
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(counts)])), f"{b.name} flags {flags}: offsets"
    k = int(counts.sum())
    want = b.x[keep]
    if want_xyz is not None:
        want = want.copy()
        want[:, :3] = want_xyz[keep]
    assert np.array_equal(xyzi[:k].view(np.uint32), want.view(np.uint32)), f"{b.name} flags {flags}: records differ from x[keep] in input order"
    if src is not None:
        local = np.concatenate([np.nonzero(keep[b.offs[s]:b.offs[s + 1]])[0] for s in range(b.n)]) if b.n else np.zeros(0, np.int64)
        assert np.array_equal(src[:k], local), f"{b.name} flags {flags}: source indices"
    if pay is not None:
        assert np.array_equal(pay[:k], h_pay[keep]), f"{b.name} flags {flags}: payload"
    return k


# ---- 1. labels ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "PARK", "C"])
def test_labels_against_the_helper_and_the_oracle_chain(scvod, oracle, name):
    b = _batch(scvod, name)
    ctx = _tracked(scvod, b)
    want, n_dyn = _helper_labels(ctx, b)
    got = _labels(ctx, b)
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} label bytes differ from the helper"
    raw, _ = _helper_labels(ctx, b, use_dyn=False)
    assert np.array_equal(_labels(ctx, b, IGNORE_DYNAMIC), raw)
    assert n_dyn > 0 and int((got == plr.PT_DYNAMIC).sum()) == n_dyn and not (raw == plr.PT_DYNAMIC).any()
    seen = set(np.unique(got).tolist())
    assert seen >= {plr.PT_DROPPED, plr.PT_GROUND, plr.PT_STATIC_OTHER, plr.PT_STATIC_CAR, plr.PT_DYNAMIC}, f"{name}: labels {sorted(seen)} only"
    if name == "A":
        assert seen == set(range(7)), f"{name}: the batch does not exercise every label"
    # the shim's form (a tensor of its own)
    assert np.array_equal(ctx.batch_point_labels().cpu().numpy()[:len(want)], want)
    # the oracle's chain over the same scans: nothing of the device in it.  Every scan with a successor
    assert np.array_equal(b.nxt[:-1], np.arange(1, b.n))
    _, ref, _ = oracle.time_sequence(b.P, b.x, b.offs, b.poses, car=CAR, other=OTHER)
    m = int(b.offs[b.n - 1])
    assert np.array_equal(plr.collapse(got)[:m], ref[:m]), f"{name}: {int((plr.collapse(got)[:m] != ref[:m]).sum())} points differ from the oracle chain"
    ctx.close()


# ---- 2. export, per flag combination -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "PARK", "C"])
def test_export_against_the_helper_per_flag_combination(scvod, name):
    import torch
    b = _batch(scvod, name)
    ctx = _tracked(scvod, b)
    lab, n_dyn = _helper_labels(ctx, b)
    raw, _ = _helper_labels(ctx, b, use_dyn=False)
    h_pay, d_pay = _payload(b)
    n = int(b.offs[-1])
    for flags in FLAG_SETS:
        o = Out(b, n)
        torch.cuda.synchronize()
        assert o.call(ctx, b, flags, d_payload_in=d_pay) == 0, ctx.lib.scvod_last_error(ctx.h)
        rc, st = _stats(ctx)
        offs, xyzi, src, pay = o.host(b)
        k = _check_export(b, raw if flags & IGNORE_DYNAMIC else lab, flags, offs, xyzi, src, pay, h_pay)
        assert rc == 0 and st.tolist() == [k, k, 0, 0]
        assert np.isnan(xyzi[k:]).all() and (src[k:] == -7).all() and (pay[k:] == -7).all(), "something was written behind the last record"
        if flags == 0:
            counts = ctx.batch_counts()
            assert k == int(counts[:, 0].sum()) - int(counts[:, 3].sum()) - n_dyn
            assert 0 < n_dyn and k < n
    ctx.close()


# ---- 3. world frame ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "PARK"])
def test_export_in_the_world_frame(scvod, name):
    import quality
    import torch
    b = _batch(scvod, name)
    ctx = _tracked(scvod, b)
    lab, _ = _helper_labels(ctx, b)
    w = quality.world_points(scvod, b.x, b.offs, b.poses)
    assert not np.array_equal(w, b.x[:, :3])
    o = Out(b, int(b.offs[-1]), payload=False)
    torch.cuda.synchronize()
    assert o.call(ctx, b, 0, poses=b.poses.copy()) == 0
    assert _stats(ctx)[0] == 0
    offs, xyzi, src, _ = o.host(b)
    _check_export(b, lab, 0, offs, xyzi, src, None, None, want_xyz=w)   # (xyz bit-equal to world_points, the intensity to the input's)
    # the shim's form, in the sensor frame again: the pose table of the call before must not leak into this one
    d_off = torch.zeros(b.n + 1, dtype=torch.int32, device="cuda")
    d_out = torch.zeros((int(b.offs[-1]), 4), dtype=torch.float32, device="cuda")
    ctx.batch_export_points(d_off, d_out)
    st = ctx.batch_export_stats()
    keep = plr.keep_of(lab, 0)
    assert st == dict(written=int(keep.sum()), kept=int(keep.sum()), overflow=False)
    assert np.array_equal(d_out.cpu().numpy()[:st["kept"]].view(np.uint32), b.x[keep].view(np.uint32))
    ctx.close()


# ---- 4. stream order and capacity --------------------------------------------------------------------------------------------------

def test_the_whole_step_on_a_side_stream_and_the_capacity_latch(scvod):
    import quality
    import torch
    b = _batch(scvod, "A")
    n = int(b.offs[-1])
    stream = _stream()
    ctx = _new_ctx(scvod, [b])
    h_pay, d_pay = _payload(b)
    lab_buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    o, cnt = Out(b, n), Out(b, 0, payload=False, src=False)
    torch.cuda.synchronize()
    st = stream.cuda_stream
    # before the tracking: refused without IGNORE_DYNAMIC, fine with it
    ctx.batch_process(b.d, b.offs, stream=st, sync=False)
    ctx.batch_cluster(stream=st, sync=False)
    assert ctx.lib.scvod_batch_point_labels(ctx.h, C.c_void_p(lab_buf.data_ptr()), n, IGNORE_DYNAMIC, C.c_void_p(st)) == -5   # no types yet
    ctx.batch_cluster_types(stream=st, sync=False)
    assert ctx.lib.scvod_batch_point_labels(ctx.h, C.c_void_p(lab_buf.data_ptr()), n, 0, C.c_void_p(st)) == -1
    assert o.call(ctx, b, 0, stream=st) == -1
    assert o.call(ctx, b, 8, stream=st) == -1 and o.call(ctx, b, 16 | IGNORE_DYNAMIC, stream=st) == -1   # the part flags are refused
    assert cnt.call(ctx, b, IGNORE_DYNAMIC, stream=st, count_only=True) == 0
    _track(ctx, b, b.T.copy(), b.nxt.copy(), st, 0)
    # the step's tail: labels, export in the world frame with a payload -- and the poses overwritten the moment the call returns
    assert ctx.lib.scvod_batch_point_labels(ctx.h, C.c_void_p(lab_buf.data_ptr()), n, 0, C.c_void_p(st)) == 0
    poses = b.poses.copy()
    assert o.call(ctx, b, 0, poses=poses, d_payload_in=d_pay, stream=st) == 0
    poses[:] = poses[::-1] + np.float32(1.5)
    stream.synchronize()
    rc, stats = _stats(ctx)
    lab, n_dyn = _helper_labels(ctx, b)
    raw, _ = _helper_labels(ctx, b, use_dyn=False)
    got = lab_buf.cpu().numpy()
    assert np.array_equal(got[:n], lab) and (got[n:] == 0xA5).all()
    offs, xyzi, src, pay = o.host(b)
    k = _check_export(b, lab, 0, offs, xyzi, src, pay, h_pay, want_xyz=quality.world_points(scvod, b.x, b.offs, b.poses))
    assert rc == 0 and stats.tolist() == [k, k, 0, 0]
    # the count-only call before the tracking: true sizes, nothing else
    keep_raw = plr.keep_of(raw, IGNORE_DYNAMIC)
    c_offs = cnt.offs.cpu().numpy()
    assert np.array_equal(c_offs[:b.n + 1], np.concatenate([[0], np.cumsum([int(keep_raw[b.offs[s]:b.offs[s + 1]].sum()) for s in range(b.n)])]))
    assert (c_offs[b.n + 1:] == -7).all() and np.isnan(cnt.xyzi.cpu().numpy()).all()
    # count only, after the tracking
    assert cnt.call(ctx, b, 0, stream=st, count_only=True) == 0
    rc, stats = _stats(ctx)
    assert rc == 0 and stats.tolist() == [0, k, 0, 0] and np.array_equal(cnt.offs.cpu().numpy()[:b.n + 1], offs)
    # one record short: the latch, the needed capacity, the guard region, and the records that did fit
    short = Out(b, k - 1)
    torch.cuda.synchronize()
    assert short.call(ctx, b, 0, d_payload_in=d_pay, stream=st) == 0
    rc, stats = _stats(ctx)
    assert rc == -4 and stats.tolist() == [k - 1, k, 1, 0]
    with pytest.raises(scvod.ScvodError):
        ctx.batch_export_stats()
    s_offs, s_xyzi, s_src, s_pay = short.host(b)                       # (asserts the guard regions)
    assert np.array_equal(s_offs, offs), "the offsets must hold the true sizes"
    keep = plr.keep_of(lab, 0)
    assert np.array_equal(s_xyzi[:k - 1].view(np.uint32), b.x[keep][:k - 1].view(np.uint32)) and np.array_equal(s_pay[:k - 1], h_pay[keep][:k - 1])
    # the latch belongs to the LAST export
    assert o.call(ctx, b, 0, stream=st) == 0
    assert _stats(ctx)[0] == 0
    ctx.close()


# ---- 5. no side effects ------------------------------------------------------------------------------------------------------------

def _map_records(scvod, ctx, b, flags):
    m = scvod.StaticMap(1 << 22)
    m.accumulate(ctx, b.poses, flags=flags)
    rec = m.export().cpu().numpy().reshape(-1, 2)
    m.close()
    return rec[np.argsort(rec[:, 0].view(np.uint64), kind="stable")]


def _export_all(ctx, b, flags=0):
    import torch
    o = Out(b, int(b.offs[-1]), payload=False)
    torch.cuda.synchronize()
    assert o.call(ctx, b, flags) == 0
    assert _stats(ctx)[0] == 0
    return o


def test_an_export_changes_nothing_else(scvod):
    import torch
    b = _batch(scvod, "D")
    fresh = _tracked(scvod, b)                       # never exports
    want_maps = {f: _map_records(scvod, fresh, b, f) for f in (0, NO_GROUND | NO_REJECTED, IGNORE_DYNAMIC)}
    want_all, _ = _everything(fresh, b)
    fresh.close()
    ctx = _tracked(scvod, b)
    arena = ctx.arena_bytes()
    lab = _labels(ctx, b)
    o1 = _export_all(ctx, b, NO_GROUND | NO_REJECTED)
    o1b = _export_all(ctx, b, NO_GROUND | NO_REJECTED)
    for x, y in ((o1.xyzi, o1b.xyzi), (o1.src, o1b.src), (o1.offs, o1b.offs)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "two consecutive exports differ"
    _export_all(ctx, b, 0)
    _export_all(ctx, b, IGNORE_DYNAMIC)
    assert ctx.arena_bytes() == arena, "the export's scratch is not part of the arena"
    for f, want in want_maps.items():
        assert np.array_equal(_map_records(scvod, ctx, b, f), want), f"the map (flags {f}) after an export differs from a ctx that never exported"
    got_all, _ = _everything(ctx, b)
    _same(got_all, want_all, "fetches after an export")
    assert np.array_equal(_labels(ctx, b), lab)
    ctx.close()


def test_labels_follow_the_fused_types_and_forget_them_again(scvod):
    b = _batch(scvod, "D")
    plain = _tracked(scvod, b)
    want_plain = _labels(plain, b)
    plain.close()
    ctx = _tracked(scvod, b, setup=lambda c: c.set_intensity_merge(*MERGE))
    assert ctx.batch_cluster_merge_stats()["fusions"] > 0
    want, _ = _helper_labels(ctx, b)                 # (batch_fetch_cluster_types reports the fused partition's types)
    got = _labels(ctx, b)
    assert np.array_equal(got, want)
    assert (got != want_plain).any(), "the merge changed no label: the case shows nothing"
    o = _export_all(ctx, b, 0)
    offs, xyzi, src, _ = o.host(b)
    _check_export(b, want, 0, offs, xyzi, src, None, None)
    # the stage off again on the same ctx: the labels of a ctx that never had it on
    ctx.set_intensity_merge(0, MERGE[1], MERGE[2], MERGE[3])
    _step(ctx, b)
    assert np.array_equal(_labels(ctx, b), want_plain)
    o = _export_all(ctx, b, 0)
    offs, xyzi, src, _ = o.host(b)
    _check_export(b, want_plain, 0, offs, xyzi, src, None, None)
    ctx.close()
