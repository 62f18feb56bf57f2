"""The batch API the way the benchmark and every real caller drive it: batch_process -> batch_cluster -> batch_cluster_types ->
batch_track(T, next_scan) with sync=False on a caller's stream that is not the current one, the static map cleared and accumulated
in two ranges on that stream, step after step on ONE ctx without a host synchronisation in between -- against two references at once:

  (a) the oracle: the cluster partition (oracle.cluster), the types (oracle.cluster_types), the voxel descriptors (oracle.voxelize),
      the carrier of Frame::max_name (oracle.cluster_last_name) and the per-point dynamic bytes of the literal chain
      (oracle.sequence_tracking_literal, one run per chain of the successor table).  This is the check that counts.
  (b) a fresh ctx that only ever saw that batch, run synchronously on its own stream: everything a caller can fetch, compared key by
      key and bit for bit (planes, vox_*, pair tables, map records ...: what the oracle does not restate).

What a reused ctx could get wrong without the rest of the suite noticing: a host read that races the stream, a host array consumed
after the call returned, a counter row / table / cached upload left over from the previous (larger) batch, an adaptive setting (warm-up
length, segments cut by measured time) that changes a result rather than a time.

Of batch_track_stats and batch_cluster_stats only the words that are RESULTS are compared with (b) (mode, error bits, undetermined
max_names; approximated scans, runs settled / clustered again ...): the number of segments, the segment and warm-up lengths, the
chunks helper blocks took and the region growing's sweep count follow timing and may differ from a fresh ctx by design.  Every comparison is np.array_equal."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import intensity_merge_ref as imr  # noqa: E402
from test_gpu_intensity_calibration import _bits, _check_scan as _check_calibrated_scan, ic  # noqa: E402,F401  (ic: the helper's fixture)
from test_gpu_parity import _canonical  # noqa: E402
from test_gpu_region_growing import _add, _check_scan as _check_rg_scan, rg  # noqa: E402,F401  (rg: the helper's fixture)

pytestmark = pytest.mark.gpu

CAR, OTHER = 2, 1
MAP_CELLS = 1 << 23
CAL = (True, 10, 200.0)
MERGE = (3, 2, 2.0, 1.0)
SENTINEL = 0x5A5A5A5A
# name: (kind, preset, first scan of seq 5, scans, stride, stride of the successor table)
SPECS = {
    "A": ("K64", "semantickitti", 300, 48, 5, 1),
    "B": ("K64", "semantickitti", 1200, 20, 3, 2),       # fewer scans, fewer points, two interleaved chains: another T, another next_scan
    "C": ("K64", "semantickitti", 2000, 22, 4, 1),       # + an empty scan first, in the middle and last, and a scan of 7 points
    "D": ("K64", "semantickitti", 700, 12, 5, 1),
    "E": ("K64", "semantickitti", 1263, 2, 3, 1),        # the scan that really follows B's second chain (1257 + 2 x 3), and the one after
    "PARK": ("PARK", "parkinglot", 30, 48, 1, 1),
    "OS128": ("OS128", "os128_fine", 301, 5, 1, 1),      # scan 303 goes through k_cc_exact (test_gpu_intensity_merge.py)
    "K6": ("K64", "semantickitti", 300, 6, 5, 1),
    "OS3": ("OS128", "os128_fine", 302, 3, 1, 1),
    "R3": ("K64", "semantickitti", 300, 3, 7, 1),        # the region growing's K64 job (test_gpu_region_growing.py)
}
CLUSTER_RESULTS = ("scans_approximated", "nodes_concerned", "exact", "scans_on_hbm_forest", "runs_settled_by_rule", "runs_clustered_again")
TRACK_RESULTS = ("chain", "error_bits", "max_name_undetermined")
# the region growing's labels are propagated by Gauss-Seidel sweeps whose waves read each other's writes (scvod_k_rgrow.inc): the fixed
# point -- segments, classes, every other counter -- is unique, the number of sweeps it takes is not (the synchronous suite asserts >= 1)
MEASURES_NOT_RESULTS = ("region_growing_stats", "max_rounds")


class Batch:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def variant(self, name, **kw):
        d = dict(self.__dict__)
        d.update(kw, name=name)
        return Batch(**d)


_BATCHES, _SOLO, _MEMO = {}, {}, {}


def _pose_delta(scvod, a, b):
    pa, pb = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    T = np.zeros(12, np.float32)
    scvod.load_lib().scvod_pose_delta(pa.ctypes.data_as(C.c_void_p), pb.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p))
    return T


def _transforms(scvod, poses, nxt):
    T = np.zeros((len(nxt), 12), np.float32)
    for s, v in enumerate(nxt):
        if v >= 0:
            T[s] = _pose_delta(scvod, poses[s], poses[v])
    return T


def _batch(scvod, name):
    if name in _BATCHES:
        return _BATCHES[name]
    import synth
    import torch
    kind, preset, first, count, stride, hop = SPECS[name]
    scans = [synth.make_scan(5, first + k * stride, kind, device="cuda") for k in range(count)]
    clouds, poses = [sc[0] for sc in scans], [sc[2] for sc in scans]
    if name == "C":
        empty = clouds[0][:0]
        clouds = [empty] + clouds[:5] + [clouds[5][:7]] + clouds[5:12] + [empty] + clouds[12:] + [empty]
        poses = [poses[0]] + poses[:5] + [poses[5]] + poses[5:12] + [poses[12]] + poses[12:] + [poses[-1]]
    n = len(clouds)
    d = torch.cat(clouds).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    poses = np.asarray(poses, np.float32)
    nxt = np.asarray([s + hop if s + hop < n else -1 for s in range(n)], np.int32)
    x = d.cpu().numpy()
    torch.cuda.synchronize()
    b = Batch(name=name, kind=kind, P=scvod.make_params(preset), d=d, x=x, offs=offs, poses=poses, nxt=nxt,
              T=_transforms(scvod, poses, nxt), n=n, ext=None, dyn_from_solo=())
    _BATCHES[name] = b
    return b


def _memo(tag, arrays, fn):
    """fn() cached under the CONTENT of its inputs: the oracle is a pure function, and the cases hand it the same scans many times"""
    h = hashlib.sha1(tag.encode())
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.view(np.uint8).reshape(-1).data)
    k = h.hexdigest()
    if k not in _MEMO:
        _MEMO[k] = fn()
    return _MEMO[k]


def _norm(v):
    v = np.ascontiguousarray(v)
    if v.dtype == np.float32:
        return _bits(v)      # (NaN normals of the calibrated fetch: one pattern, as test_gpu_intensity_calibration.py compares them)
    if v.dtype.fields is not None:
        return v.view(np.uint8)
    return v


def _sorted_records(smap, stream):
    rec = smap.export(stream=stream).cpu().numpy().reshape(-1, 2)
    return rec[np.argsort(rec[:, 0].view(np.uint64), kind="stable")]


def _everything(ctx, b, smap=None, stream=None):
    """everything a caller can fetch of the last step, as {key: array}, and the per-scan fetch results"""
    n = b.n
    out = {"counts": ctx.batch_counts()}
    res = []
    for s in range(n):
        r = ctx.batch_fetch(s)
        res.append(r)
        for k, v in r.items():
            out[f"fetch[{s}].{k}"] = np.asarray(v)
        out[f"clusters[{s}]"] = ctx.batch_fetch_clusters(s, r["n_apri"])
        out[f"types[{s}]"] = ctx.batch_fetch_cluster_types(s, r["n_apri"], car_label=CAR, other_label=OTHER)
        out[f"classes[{s}]"] = ctx.batch_fetch_cluster_classes(s, r["n_apri"])
        for k, v in ctx.batch_fetch_track(s).items():
            out[f"track[{s}].{k}"] = np.asarray(v)
    cs = ctx.batch_cluster_stats()
    for k in CLUSTER_RESULTS:
        out["cluster_stats." + k] = np.asarray(int(cs[k]))
    ln, lst = ctx.batch_cluster_last_name(n)
    out["last_name"] = ln
    out["last_name_stats"] = np.asarray([lst["unknown_too_large"], lst["unknown_irregular"]])
    ts = ctx.batch_track_stats()
    for k in TRACK_RESULTS:
        out["track_stats." + k] = np.asarray(int(ts[k]))
    for what, st in (("merge_stats", ctx.batch_cluster_merge_stats()), ("region_growing_stats", ctx.batch_region_growing_stats()),
                     ("calibration_stats", ctx.batch_intensity_calibration_stats())):
        for k, v in st.items():
            if (what, k) != MEASURES_NOT_RESULTS:
                out[f"{what}.{k}"] = np.asarray(int(v))
    if smap is not None:
        out["map"] = _sorted_records(smap, stream)
    return out, res


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert np.array_equal(_norm(got[k]), _norm(want[k])), f"{what}: {k} differs from the fresh ctx that only saw this batch"


def _track(ctx, b, T, nxt, stream, sync):
    """scvod_batch_track through the C-ABI with a pointer table of the test's own (the shim builds its table inside the call)"""
    tab = None
    if b.ext is not None:
        tab = (C.c_void_p * len(b.ext))(*[C.c_void_p(e.data_ptr()) for e in b.ext])
    ctx._chk(ctx.lib.scvod_batch_track(ctx.h, T.ctypes.data_as(C.c_void_p), nxt.ctypes.data_as(C.c_void_p), tab,
                                       len(b.ext) if b.ext is not None else 0, C.c_void_p(stream or 0), int(sync)))
    return tab


def _enqueue(ctx, smap, b, stream, scribble=False, d=None, after_process=None, decoys=None):
    """the benchmark's step (bench.py step()): nothing here synchronises.  scribble: every host array is overwritten right after the
    call it was passed to returned -- with other VALID values (offsets that still rise from 0 inside the batch, a rigid transform, "no
    successor", other poses, another exported table), so that a late read would change the result, never an address"""
    offs, T, nxt = b.offs.copy(), b.T.copy(), b.nxt.copy()
    ctx.batch_process(b.d if d is None else d, offs, stream=stream, sync=False)
    if scribble:
        offs[:] = offs // 2
    if after_process is not None:
        after_process()
    ctx.batch_cluster(stream=stream, sync=False)
    ctx.batch_cluster_types(stream=stream, sync=False)
    tab = _track(ctx, b, T, nxt, stream, 0)
    if scribble:
        T[:] = np.asarray([1, 0, 0, 3, 0, 1, 0, -2, 0, 0, 1, 0], np.float32)
        nxt[:] = -1
        if tab is not None:
            for e in range(len(tab)):
                tab[e] = decoys[e].data_ptr()
    if smap is not None:
        smap.clear(stream=stream)
        half = b.n // 2
        for first, count in ((0, half), (half, b.n - half)):
            poses = b.poses.copy()
            smap.accumulate_range(ctx, poses, first, count, stream=stream)
            if scribble:
                poses[:] = poses[::-1] + np.float32(1.5)


def _new_ctx(scvod, batches, setup=None):
    ctx = scvod.Ctx(batches[0].P, max_points_total=max(int(b.offs[-1]) for b in batches) + 64, max_scans=max(b.n for b in batches))
    if setup is not None:
        setup(ctx)
    return ctx


def _solo(scvod, b, tag="plain", setup=None):
    """reference (b): a fresh ctx created for this batch alone, every call synchronous on the ctx's own stream, the map in one call"""
    if (b.name, tag) in _SOLO:
        return _SOLO[(b.name, tag)]
    ctx = _new_ctx(scvod, [b], setup)
    ctx.batch_process(b.d, b.offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    _track(ctx, b, b.T, b.nxt, None, 1)
    smap = scvod.StaticMap(MAP_CELLS)
    smap.accumulate(ctx, b.poses)
    out, _ = _everything(ctx, b, smap)
    smap.close()
    ctx.close()
    _SOLO[(b.name, tag)] = out
    return out


def _chains(nxt):
    heads = sorted(set(range(len(nxt))) - {int(v) for v in nxt if v >= 0})
    for h in heads:
        chain = [h]
        while nxt[chain[-1]] >= 0:
            chain.append(int(nxt[chain[-1]]))
        yield chain


def _check_oracle(oracle, b, out, res, merge=None):
    """reference (a).  The apri records come from the device (the calibrated cases check their intensities against the helper before
    this); everything derived from them is the oracle's.  Returns the merge helper's counters."""
    P, n = b.P, b.n
    pk = bytes(P).hex() + ":"                            # (the oracle's answers depend on the parameters too)
    grid = tuple(int(g) for g in oracle.grid_dims(P)[:3])
    names = [out[f"clusters[{s}]"] for s in range(n)]
    types = [out[f"types[{s}]"] for s in range(n)]
    ln = out["last_name"]
    collide = np.full(n, -1, np.int32)
    merge_stats = dict(clusters_before=0, fusions=0, clusters_after=0)
    assert np.array_equal(out["counts"][:, 0], np.diff(b.offs)), f"{b.name}: batch_counts n_points"
    for s in range(n):
        apri = res[s]["apri"]
        assert len(apri) == out["counts"][s, 4] == len(names[s]) == len(types[s]), f"{b.name} scan {s}"
        vox = _memo(pk + "voxelize", [apri], lambda: oracle.voxelize(P, apri))
        for k in ("vox_key", "vox_pt_begin", "vox_pts", "vox_av", "vox_cov"):
            assert np.array_equal(_norm(res[s][k]), _norm(vox[k])), f"{b.name} scan {s}: {k} differs from the oracle"
        pre = _memo(pk + "cluster", [apri], lambda: _canonical(oracle.cluster(P, apri)[0]).astype(np.int32)) if len(apri) else np.zeros(0, np.int32)
        want = pre
        if merge is not None and len(apri):
            st = {}
            want = _memo(pk + "merge" + repr(merge), [apri], lambda: (imr.convention(vox, pre, grid, *merge, stats=st), st))
            want, st = want
            for k in merge_stats:
                merge_stats[k] += st[k]
        assert np.array_equal(names[s], want), f"{b.name} scan {s}: the cluster partition differs from the oracle's"
        ty = _memo(pk + "types", [apri, names[s]], lambda: oracle.cluster_types(P, apri, names[s], car_label=CAR, other_label=OTHER))
        assert np.array_equal(types[s], ty), f"{b.name} scan {s}: the cluster types differ from the oracle's"
        c = _memo(pk + "last_name", [apri], lambda: oracle.cluster_last_name(P, apri)[0]) if len(apri) else -1
        collide[s] = names[s][c] if c >= 0 else -1      # (the carrier's fusion when the merge is on; c itself otherwise)
        if ln[s, 2] == 0:
            assert ln[s, 0] == collide[s] or (ln[s, 0] == -1 and collide[s] >= 0 and types[s][collide[s]] == -1), \
                f"{b.name} scan {s}: device says cluster {ln[s, 0]} carries max_name, the literal loop {collide[s]}"
    collide[ln[:, 2] != 0] = -1                          # (reported undetermined: the chain hands out a fresh number there)
    assert out["track_stats.max_name_undetermined"] == int((ln[:, 2] != 0).sum())
    total = 0
    for chain in _chains(b.nxt):
        apri = np.concatenate([res[s]["apri"] for s in chain])
        ao = np.concatenate([[0], np.cumsum([len(res[s]["apri"]) for s in chain])]).astype(np.int32)
        nm, ty = np.concatenate([names[s] for s in chain]).astype(np.int32), np.concatenate([types[s] for s in chain]).astype(np.int32)
        co, ps = collide[chain], b.poses[chain]
        dyn = _memo(pk + "chain", [apri, ao, nm, ty, co, ps], lambda: oracle.sequence_tracking_literal(P, apri, ao, nm, ty, co, ps, chain=3)[0])
        for k, s in enumerate(chain):
            got = out[f"track[{s}].pt_dyn"]
            total += int(got.sum())
            if s in b.dyn_from_solo:
                continue
            want = dyn[ao[k]:ao[k + 1]]
            assert np.array_equal(got, want), f"{b.name} scan {s}: {int((got != want).sum())} of {len(want)} per-point bytes differ from the oracle's literal chain"
    assert total > 0, f"{b.name}: no dynamic or unclustered point at all"
    assert out["track_stats.error_bits"] == 0 and out["track_stats.chain"] == 1
    return merge_stats


def _finish(scvod, oracle, ctx, smap, b, stream, tag="plain", setup=None, merge=None):
    """after the step's synchronisation: fetch everything, check (a), then (b)"""
    out, res = _everything(ctx, b, smap, stream.cuda_stream)
    st = _check_oracle(oracle, b, out, res, merge)
    _same(out, _solo(scvod, b, tag, setup), f"{b.name} [{tag}]")
    return out, res, st


def _stream():
    import torch
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != torch.cuda.current_stream().cuda_stream
    return stream


def _assert_os128(out):
    assert out["cluster_stats.runs_clustered_again"] > 0 and out["cluster_stats.scans_approximated"] == 0


# ---- 1. the benchmark's step, asynchronously ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "PARK", "OS128"])
def test_the_benchmark_step_on_a_side_stream(scvod, oracle, name):
    b = _batch(scvod, name)
    stream = _stream()
    ctx, smap = _new_ctx(scvod, [b]), scvod.StaticMap(MAP_CELLS)
    _enqueue(ctx, smap, b, stream.cuda_stream)
    stream.synchronize()
    out, _, _ = _finish(scvod, oracle, ctx, smap, b, stream)
    if name == "OS128":
        _assert_os128(out)
    smap.close()
    ctx.close()


# ---- 2. changing batches on one ctx ------------------------------------------------------------------------------------------------

def _rows_beyond_the_batch_are_not_live(scvod, ctx, b, cap_scans):
    """include/scvod.h: scvod_batch_counts writes the n_scans rows of the LAST batch and nothing behind them; a scan index >= n_scans
    is SCVOD_ERR_INVALID for the five per-scan fetches the header names -- the rows a larger batch left in the arena cannot be read as
    live data"""
    buf = np.full((cap_scans + 1, 8), SENTINEL, np.int32)
    ctx._chk(ctx.lib.scvod_batch_counts(ctx.h, buf.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(buf[:b.n, 0], np.diff(b.offs)) and (buf[b.n:] == SENTINEL).all()
    from scvod_py import ScanResult, TrackResult
    one = np.zeros(1 << 20, np.int32)
    for s in (b.n, cap_scans - 1 if cap_scans - 1 >= b.n else b.n, cap_scans + 3):
        assert ctx.lib.scvod_batch_fetch(ctx.h, s, C.byref(ScanResult())) == -1
        assert ctx.lib.scvod_batch_fetch_track(ctx.h, s, C.byref(TrackResult())) == -1
        assert ctx.lib.scvod_batch_fetch_clusters(ctx.h, s, one.ctypes.data_as(C.c_void_p), len(one)) == -1
        assert ctx.lib.scvod_batch_fetch_cluster_types(ctx.h, s, CAR, OTHER, one.ctypes.data_as(C.c_void_p), len(one)) == -1
        assert ctx.lib.scvod_batch_fetch_cluster_classes(ctx.h, s, CAR, 0, 1, one.ctypes.data_as(C.c_void_p), len(one)) == -1
    small = np.zeros((max(b.n - 1, 1), 4), np.int32)
    if b.n > 1:  # the last-name rows are refused rather than cut short
        assert ctx.lib.scvod_batch_cluster_last_name(ctx.h, small.ctypes.data_as(C.c_void_p), b.n - 1, None) == -4


def test_changing_batches_on_one_ctx(scvod, oracle):
    """A -> B -> C -> A -> A, asynchronously, on a ctx sized for the largest: once with the tracking mode left at its adaptive default
    (segments per job, warm-up per stream; the second A in a row is the one step whose segments can be cut by the times its predecessor
    measured: the planner takes them only for the plan of frames that measured them) and once with segment_steps fixed.  Every step is
    synchronised and fetched here: the feedback of a step has always arrived when the next one is planned (case 3 is the other way)"""
    seq = [_batch(scvod, k) for k in ("A", "B", "C", "A", "A")]
    b, c = seq[1], seq[2]
    assert b.n < seq[0].n and b.offs[-1] < seq[0].offs[-1] and c.n > b.n
    n_pts = np.diff(c.offs)
    assert n_pts[0] == 0 and n_pts[-1] == 0 and (n_pts[1:-1] == 0).sum() == 1 and (n_pts == 7).sum() == 1
    cap = max(x.n for x in seq)
    dyn = {}
    for mode in ("adaptive", "fixed"):
        stream = _stream()
        ctx, smap = _new_ctx(scvod, seq), scvod.StaticMap(MAP_CELLS)
        if mode == "fixed":
            ctx.set_track_mode(chain=True, segment_steps=6)
        for k, x in enumerate(seq):
            _enqueue(ctx, smap, x, stream.cuda_stream)
            stream.synchronize()
            out, _, _ = _finish(scvod, oracle, ctx, smap, x, stream)
            _rows_beyond_the_batch_are_not_live(scvod, ctx, x, cap)
            if mode == "fixed":
                assert ctx.batch_track_stats()["segment_steps"] == 6
            dyn[(mode, k)] = np.concatenate([out[f"track[{s}].pt_dyn"] for s in range(x.n)])
        smap.close()
        ctx.close()
    for k in range(len(seq)):
        assert np.array_equal(dyn[("adaptive", k)], dyn[("fixed", k)]), f"step {k}: the adaptive plan changed a result, not only a time"


# ---- 3. back-to-back steps without host synchronisation ----------------------------------------------------------------------------

def test_back_to_back_steps_with_alternating_input_buffers(scvod, oracle):
    """Two passes over A, B, C, D/2, D enqueued on one stream with nothing between the steps but the calls, ONE synchronisation at the end.
    Which calls of a step may wait on the host inside the library, and what the test does about it:
      - scvod_batch_map_accumulate* waits for the stream when the poses differ from the previous call's (include/scvod.h): a map after
        every step would drain the stream between the steps, so only the LAST step accumulates the map;
      - scvod_batch_track allocates the chain's workspace when a job needs more than it has (device synchronisation): the first pass
        may do that, the second pass finds the workspace of the largest job in place;
      - a changed table travels through one of eight pinned slots, and a slot is reused only when the copy that read it is done: a
        step with new tables may wait for an upload of the step BEFORE (which sits in front of that step's tracking kernels), never for
        the chain it has just enqueued.
    So in the second pass the host plans and enqueues step k + 1 while step k's chain is still on the device, and the counters and
    per-step times the planner takes from earlier batches (hipEventQuery) arrive late or not at all, as in the benchmark."""
    import torch
    d = _batch(scvod, "D")
    nxt2 = np.asarray([s + 2 if s + 2 < d.n else -1 for s in range(d.n)], np.int32)
    # D as two interleaved chains right before D as one: tables of the SAME size with other contents (a cache that compared sizes only
    # would keep them)
    once = [_batch(scvod, k) for k in ("A", "B", "C")] + [d.variant("D/2", nxt=nxt2, T=_transforms(scvod, d.poses, nxt2)), d]
    seq = once + once
    stream = _stream()
    ctx, smap = _new_ctx(scvod, seq), scvod.StaticMap(MAP_CELLS)
    cap = max(int(x.offs[-1]) for x in seq) + 8
    bufs = [torch.zeros((cap, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for k, x in enumerate(seq):
        with torch.cuda.stream(stream):
            bufs[k % 2][:int(x.offs[-1])].copy_(x.d)

        def overwrite_the_previous_input(k=k):
            # include/scvod.h: d_xyzi must stay valid until the NEXT batch call -- this one has just been enqueued
            if k > 0:
                with torch.cuda.stream(stream):
                    bufs[(k - 1) % 2].fill_(7.0)
        _enqueue(ctx, smap if k == len(seq) - 1 else None, x, stream.cuda_stream, d=bufs[k % 2], after_process=overwrite_the_previous_input)
    stream.synchronize()
    last = seq[-1]
    _finish(scvod, oracle, ctx, smap, last, stream)
    assert ctx.batch_track_stats()["error_bits"] == 0
    smap.close()
    ctx.close()


# ---- 4. host arrays are the caller's again when the call returns ---------------------------------------------------------------------

def test_host_arrays_may_be_overwritten_when_the_call_returns(scvod, oracle):
    """scan_offsets, T, next_scan, the external-table pointers and the map's poses are overwritten right after the asynchronous call
    they were passed to returned, before any synchronisation (include/scvod.h: every one of them is copied before the call returns).
    The last scan of B's second chain is tracked against an external table: the scan that really follows it in the sequence, exported by
    another ctx.  That scan's bytes are a first-order decision the oracle's chain does not restate -- they are compared with the fresh
    ctx, every other scan's with the oracle -- so the test first shows that the decoy table (the scan after, 3 m further on), which
    replaces the pointer as soon as the call returned, WOULD change that scan's tracking result: a late read could not pass.  Then the
    pointer table of scvod_batch_track_compare_device."""
    import torch
    b0, dd = _batch(scvod, "B"), _batch(scvod, "E")
    other = _new_ctx(scvod, [dd])
    other.batch_process(dd.d, dd.offs)
    other.batch_cluster()
    other.batch_cluster_types()
    other.batch_track_tables()
    table, decoy = (torch.zeros((1 << 17, 4), dtype=torch.int32, device="cuda") for _ in range(2))
    other.batch_export_table(0, table)
    other.batch_export_table(1, decoy)
    torch.cuda.synchronize()
    assert int(table[0, 0]) > 0 and not torch.equal(table, decoy)
    nxt = b0.nxt.copy()
    last = b0.n - 1
    nxt[last] = -2
    T = b0.T.copy()
    T[last] = _pose_delta(scvod, b0.poses[last], dd.poses[0])
    b = b0.variant("B+external", nxt=nxt, T=T, ext=[table], dyn_from_solo=(last,))
    want, wrong = _solo(scvod, b), _solo(scvod, b.variant("B+decoy", ext=[decoy]))
    assert any(not np.array_equal(want[f"track[{last}].{k}"], wrong[f"track[{last}].{k}"]) for k in ("n_unique", "pair_label", "pair_count", "cluster_state", "pt_dyn")), \
        "the decoy table gives the same result: overwriting the pointer table could not be noticed"
    a = _batch(scvod, "A")
    stream = _stream()
    ctx, smap = _new_ctx(scvod, [a, b]), scvod.StaticMap(MAP_CELLS)
    _enqueue(ctx, smap, b0, stream.cuda_stream)   # (a step before: every cached upload of the ctx holds ANOTHER batch's tables)
    for x in (a, b):
        _enqueue(ctx, smap, x, stream.cuda_stream, scribble=True, decoys=[decoy])
        stream.synchronize()
        _finish(scvod, oracle, ctx, smap, x, stream)
        # the state pointer table of the device compare: rows nobody wrote differ (one per chain), NULL rows are not compared
        n_chains = len(ctx.batch_track_chains())
        assert n_chains == len(list(_chains(x.nxt))) > 0
        rows = [torch.zeros(int(ctx.lib.scvod_chain_state_bytes(ctx.h)), dtype=torch.uint8, device="cuda") for _ in range(n_chains)]
        torch.cuda.synchronize()
        assert ctx.batch_track_compare(rows, stream=stream.cuda_stream) == n_chains
        assert ctx.batch_track_compare([None] * n_chains, stream=stream.cuda_stream) == 0
        word = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        written, null = [r.data_ptr() for r in rows], [None] * n_chains
        for k, (first, then) in enumerate(((written, null), (null, written), (written, null))):
            tab = (C.c_void_p * n_chains)(*first)
            ctx._chk(ctx.lib.scvod_batch_track_compare_device(ctx.h, tab, n_chains, C.c_void_p(word[k % 2:].data_ptr()), C.c_void_p(stream.cuda_stream)))
            for e in range(n_chains):
                tab[e] = then[e]
        stream.synchronize()
        assert word.cpu().tolist() == [2 * n_chains, 0]
    smap.close()
    ctx.close()
    other.close()


# ---- 5. the opt-in stages on the same path -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["K6", "OS3"])
def test_calibration_and_merge_on_the_asynchronous_path_and_off_again(scvod, oracle, ic, name):  # noqa: F811
    b = _batch(scvod, name)
    stream = _stream()

    def stages_on(c):
        c.set_intensity_calibration(*CAL)
        c.set_intensity_merge(*MERGE)
    ctx, smap = _new_ctx(scvod, [b], stages_on), scvod.StaticMap(MAP_CELLS)
    _enqueue(ctx, smap, b, stream.cuda_stream)
    stream.synchronize()
    want_cal = {}
    for s in range(b.n):  # the calibrated intensities, apri records and voxel descriptors against the calibration helper
        _check_calibrated_scan(ctx, ic, oracle, b.P, s, b.x[b.offs[s]:b.offs[s + 1]], CAL, want_cal)
    got_cal = ctx.batch_intensity_calibration_stats()
    assert {k: got_cal[k] for k in want_cal} == want_cal and got_cal["points"] > 0
    # ... the fused partition against the merge helper, its types and the chain on it against the oracle; then the fresh ctx
    out, _, want_merge = _finish(scvod, oracle, ctx, smap, b, stream, tag="calibration+merge", setup=stages_on, merge=MERGE)
    got_merge = ctx.batch_cluster_merge_stats()
    assert {k: got_merge[k] for k in want_merge} == want_merge and got_merge["fusions"] > 0
    if name == "OS3":
        _assert_os128(out)
    # both stages off again on the same ctx: every output is the plain fresh ctx's, the stage counters are zero
    ctx.set_intensity_calibration(False, CAL[1], CAL[2])
    ctx.set_intensity_merge(0, *MERGE[1:])
    _enqueue(ctx, smap, b, stream.cuda_stream)
    stream.synchronize()
    out, _, _ = _finish(scvod, oracle, ctx, smap, b, stream)
    assert all(int(out[k]) == 0 for k in out if k.startswith(("merge_stats.", "calibration_stats.")))
    assert ctx.batch_intensity_calibration_candidates() == 0
    if name == "OS3":
        _assert_os128(out)
    smap.close()
    ctx.close()


def test_region_growing_on_the_asynchronous_path_and_off_again(scvod, oracle, rg):  # noqa: F811
    b = _batch(scvod, "R3")
    assert b.n <= 8
    stream = _stream()

    def stage_on(c):
        c.set_region_growing(True)
    ctx, smap = _new_ctx(scvod, [b], stage_on), scvod.StaticMap(MAP_CELLS)
    _enqueue(ctx, smap, b, stream.cuda_stream)
    stream.synchronize()
    want = {}
    for s in range(b.n):  # normals, curvatures, segments and classes against the region-growing helper
        _add(want, _check_rg_scan(ctx, rg, b.P, s, ctx.batch_fetch(s)["apri"]))
    got = ctx.batch_region_growing_stats()
    assert {k: got[k] for k in want} == want and got["candidate_clusters"] > 0 and got["max_rounds"] >= 1
    _finish(scvod, oracle, ctx, smap, b, stream, tag="region growing", setup=stage_on)
    ctx.set_region_growing(False)
    _enqueue(ctx, smap, b, stream.cuda_stream)
    stream.synchronize()
    out, _, _ = _finish(scvod, oracle, ctx, smap, b, stream)
    assert all(int(out[k]) == 0 for k in out if k.startswith("region_growing_stats.")) and ctx.batch_region_growing_stats()["max_rounds"] == 0
    smap.close()
    ctx.close()


# ---- 6. two ctxs, two streams, one process ---------------------------------------------------------------------------------------------

def test_two_ctxs_on_two_streams(scvod, oracle):
    """the 128-beam batch (its k_cc_exact scan publishes passes to helper blocks that spin on a board in global memory, at most 20 ms per
    batch when nobody asks) beside a K64 batch of another ctx: both enqueued before either stream is synchronised"""
    jobs = []
    for name in ("OS128", "A"):
        b = _batch(scvod, name)
        jobs.append((b, _stream(), _new_ctx(scvod, [b]), scvod.StaticMap(MAP_CELLS)))
    for b, stream, ctx, smap in jobs:
        _enqueue(ctx, smap, b, stream.cuda_stream)
    for b, stream, ctx, smap in jobs:
        stream.synchronize()
    for b, stream, ctx, smap in jobs:
        out, _, _ = _finish(scvod, oracle, ctx, smap, b, stream)
        if b.name == "OS128":
            _assert_os128(out)
        smap.close()
        ctx.close()
