"""scvod_batch_stack_scans (include/scvod.h; csrc/scvod_stack.hip) on the device against the numpy statement of tests/helpers/stack_ref.py:
part sizes around every wave and tile boundary in every position of a group, special values, group counts, capacity and argument
errors with sentinels, the untouched batch state, stream order in front of the batch chain, repeatability.  Comparisons are on the
uint32 images; a NaN coordinate of a transformed point counts as "a NaN", everything else is bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import stack_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 2048                       # kStackTile
SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 130, 300]   # 11 sizes: coprime with every interval below
CONFIGS = [(1, 1, False), (1, 1, True), (1, 3, False), (1, 3, True), (3, 3, False), (3, 3, True), (3, 1, False), (5, 2, False),
           (9, 9, False)]
SENT_F = 0x5A5A5A5A               # sentinel word of the output buffers
PAD = 96                          # records behind the capacity that must stay untouched
INVALID, CAPACITY = -1, -4


def _torch():
    import torch
    return torch


def _poses(n, seed):
    """yaw / pitch / roll and translations that are not small: a wrong matrix or a swapped pre / next shows"""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 6), np.float32)
    p[:, :3] = rng.uniform(-50, 50, (n, 3))
    p[:, 3:] = rng.uniform(-1.0, 1.0, (n, 3))
    return p


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-60, 60, (n, 4)).astype(np.float32)
    x[:, 3] = rng.uniform(0, 255, n).astype(np.float32)
    return x


def _job(window, interval, seed):
    """scan sizes: an entirely empty group first, then the 11 sizes cyclically for 11 * interval scans -- every size at every residue
    of the interval, hence in every position of a group --, then `window` more scans to close the last windows"""
    sizes = [0] * window + [SIZES[k % len(SIZES)] for k in range(11 * interval + window)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(off[-1])
    rng = np.random.default_rng(seed + 1)
    payload = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    payload[::3] |= np.uint32(0x80000000)
    return _cloud(n, seed), off, _poses(len(sizes), seed + 2), payload


class Out:
    """output buffers with PAD sentinel records behind the capacity the call is given"""

    def __init__(self, cap, payload, src, dev="cuda"):
        torch = _torch()
        self.cap = cap
        self.xyzi = torch.full(((cap + PAD) * 4,), SENT_F, dtype=torch.int32, device=dev)
        self.payload = torch.full((cap + PAD,), SENT_F, dtype=torch.int32, device=dev) if payload else None
        self.src = torch.full((cap + PAD,), SENT_F, dtype=torch.int32, device=dev) if src else None

    def args(self):
        return dict(d_xyzi_out=self.xyzi[:4 * self.cap].view(_torch().float32).reshape(self.cap, 4), d_payload_out=self.payload, d_src_out=self.src)

    def tails_intact(self, used):
        ok = bool((self.xyzi[4 * used:] == SENT_F).all())
        for t in (self.payload, self.src):
            ok = ok and (t is None or bool((t[used:] == SENT_F).all()))
        return ok


def _check(scvod, oracle, ctx, x, off, poses, payload, window, interval, bound, with_payload, with_src, d_in=None, d_pay=None, stream=None):
    torch = _torch()
    want = stack_ref.stack(oracle, x, off, poses, window, interval, bound, payload)
    need = int(want["out_offsets"][-1])
    if d_in is None:       # (an empty tensor has no address: a job without points still hands over valid arrays)
        d_in = torch.from_numpy(x).cuda() if len(x) else torch.zeros((1, 4), device="cuda")
    if d_pay is None:
        d_pay = torch.from_numpy(payload.view(np.int32)).cuda() if len(payload) else torch.zeros(1, dtype=torch.int32, device="cuda")
    out = Out(need, with_payload, with_src)
    got_off, got_mid = ctx.batch_stack_scans(d_in, off, poses, window=window, interval=interval, reference_bound=bound,
                                             d_payload_in=d_pay if with_payload else None, stream=stream, **out.args())
    torch.cuda.synchronize()
    tag = (window, interval, bound, with_payload, with_src)
    assert np.array_equal(got_off, want["out_offsets"]) and np.array_equal(got_mid, want["mid"]), tag
    got = out.xyzi[:4 * need].cpu().numpy().view(np.float32).reshape(-1, 4)
    gi, wi = stack_ref.image(got, want["moved"]), stack_ref.image(want["xyzi"], want["moved"])
    bad = np.nonzero((gi != wi).any(axis=1))[0]
    assert bad.size == 0, (tag, bad[:5], got[bad[:3]], want["xyzi"][bad[:3]])
    if with_payload:
        assert np.array_equal(out.payload[:need].cpu().numpy().view(np.uint32), want["payload"]), tag
    if with_src:
        assert np.array_equal(out.src[:need].cpu().numpy(), want["src"]), tag
    assert out.tails_intact(need), tag
    return want, out


@pytest.fixture(scope="module")
def ctx(scvod):
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1 << 18, max_scans=64)
    yield c
    c.close()


@pytest.mark.parametrize("window,interval,bound", CONFIGS)
def test_part_sizes_in_every_position(scvod, oracle, ctx, window, interval, bound):
    torch = _torch()
    x, off, poses, payload = _job(window, interval, 100 * window + interval)
    d_in = torch.from_numpy(x).cuda()
    d_pay = torch.from_numpy(payload.view(np.int32)).cuda()
    n_groups = len(stack_ref.groups(len(off) - 1, window, interval, bound))
    assert n_groups >= 11
    for with_payload in (False, True):
        for with_src in (False, True):
            want, _ = _check(scvod, oracle, ctx, x, off, poses, payload, window, interval, bound, with_payload, with_src, d_in, d_pay)
    assert len(want["mid"]) == n_groups
    if window > 1:   # the job does move points, and by more than rounding
        moved = want["moved"]
        assert moved.any() and np.abs(want["xyzi"][moved][:, :3] - x[want["src"][moved]][:, :3]).max() > 10


def test_special_values(scvod, oracle, ctx):
    """-0.0, inf, NaN and denormal coordinates and intensities, payload words with the top bit set: the middle part and every intensity
    are the input's bit for bit"""
    specials = np.asarray([-0.0, 0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.4e-45, 3.0e38, -3.0e38, 1.0, -2.5], np.float32)
    rng = np.random.default_rng(5)
    n_per = 700
    x = _cloud(3 * n_per, 6)
    pick = rng.integers(0, len(specials), x.shape)
    mask = rng.random(x.shape) < 0.35
    x[mask] = specials[pick][mask]
    x.view(np.uint32)[::7, 3] = 0xFFC12345          # a NaN intensity with a payload of its own
    x.view(np.uint32)[3::11, 3] = 0x00000001        # the smallest denormal
    off = np.asarray([0, n_per, 2 * n_per, 3 * n_per], np.int32)
    poses = _poses(3, 8)
    payload = (rng.integers(0, 2 ** 31, 3 * n_per, dtype=np.int64).astype(np.uint32) | np.uint32(0x80000000))
    want, out = _check(scvod, oracle, ctx, x, off, poses, payload, 3, 3, False, True, True)
    got = out.xyzi[:4 * 3 * n_per].cpu().numpy().view(np.uint32).reshape(-1, 4)
    xb = x.view(np.uint32)
    assert np.array_equal(got[:n_per], xb[n_per:2 * n_per])                       # the middle scan first, untouched
    assert np.array_equal(got[:, 3], xb[want["src"], 3])                          # every intensity word
    assert np.isnan(want["xyzi"][want["moved"]][:, :3]).any() and np.isinf(want["xyzi"][want["moved"]][:, :3]).any()
    # equal poses: the matrices are (nearly) the identity and their translation is tiny, so denormal coordinates survive the products
    same = np.repeat(_poses(1, 9), 3, axis=0)
    same[:, 3:] = 0
    _check(scvod, oracle, ctx, x, off, same, payload, 3, 3, False, False, False)


@pytest.mark.parametrize("n_in,window,interval,bound,n_out", [(2, 3, 3, False, 0), (2, 3, 3, True, 0), (0, 1, 1, False, 0), (4, 5, 1, False, 0),
                                                              (9, 3, 3, False, 3), (9, 3, 3, True, 2), (10, 3, 3, True, 3), (6, 1, 3, True, 1),
                                                              (6, 1, 3, False, 2), (3, 3, 3, True, 0)])
def test_group_counts(scvod, oracle, ctx, n_in, window, interval, bound, n_out):
    sizes = [37 + 11 * k for k in range(n_in)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    x = _cloud(int(off[-1]), 3)
    payload = np.arange(int(off[-1]), dtype=np.uint32)
    want, out = _check(scvod, oracle, ctx, x, off, _poses(n_in, 4), payload, window, interval, bound, True, True)
    assert len(want["mid"]) == n_out
    if n_out == 0:
        assert out.tails_intact(0)


def test_capacity_and_argument_errors(scvod, oracle, ctx):
    torch = _torch()
    lib = scvod.load_lib()
    sizes = [500, 0, 2100, 65, 1, 900]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(off[-1])
    x, poses = _cloud(n, 12), _poses(6, 13)
    payload = np.arange(n, dtype=np.uint32)
    d_in = torch.from_numpy(x).cuda()
    d_pay = torch.from_numpy(payload.view(np.int32)).cuda()
    need = n                                            # window 3, interval 3: both groups, every scan once
    # the capacity equal to the need succeeds (and _check sees the sentinels behind it)
    _check(scvod, oracle, ctx, x, off, poses, payload, 3, 3, False, True, True, d_in, d_pay)

    def refused(status, out, **kw):
        a = dict(out.args())
        a.update(kw.pop("override", {}))
        args = dict(d_xyzi_in=d_in, offsets=off, poses=poses, window=3, interval=3, d_payload_in=d_pay)
        args.update(a)
        args.update(kw)
        with pytest.raises(scvod.ScvodError, match=f"status {status}\\b"):
            ctx.batch_stack_scans(**args)
        torch.cuda.synchronize()
        assert out.tails_intact(0)

    refused(CAPACITY, Out(need - 1, True, True))
    refused(CAPACITY, Out(0, True, True))
    refused(INVALID, Out(need, True, True), window=2)
    refused(INVALID, Out(need, True, True), window=11)
    refused(INVALID, Out(need, True, True), interval=0)
    refused(INVALID, Out(need, True, True), d_payload_in=None)                       # a payload output without an input
    o = Out(need + 1, False, False)                                                  # a misaligned xyzi view: 4 bytes off
    refused(INVALID, o, override=dict(d_xyzi_out=o.xyzi[1:1 + 4 * need].view(torch.float32)))
    o = Out(need, False, False)
    refused(INVALID, o, d_xyzi_in=d_in.view(-1)[1:-3])                               # ... of the input
    # the output inside the input's range, and just touching its last record
    o = Out(need, False, False)
    big = torch.zeros((3 * n, 4), dtype=torch.float32, device="cuda")
    big[:n] = d_in
    refused(INVALID, o, d_xyzi_in=big, override=dict(d_xyzi_out=big[n - 1:]))
    refused(INVALID, o, d_xyzi_in=big, override=dict(d_xyzi_out=big))
    paybig = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    o = Out(need, False, False)
    refused(INVALID, o, d_payload_in=paybig, override=dict(d_payload_out=paybig[n - 1:]))
    # directly behind the input is fine
    got_off, _ = ctx.batch_stack_scans(big, off, poses, big[n:], d_payload_in=paybig, d_payload_out=paybig[n:])
    torch.cuda.synchronize()
    g1 = n + int(got_off[1])                                                          # group 1 starts with its middle scan, scan 4
    assert got_off[-1] == need and torch.equal(big[g1:g1 + sizes[4]].view(torch.int32), big[off[4]:off[5]].view(torch.int32))
    # pointers that are not 4-byte aligned, and an unknown flag bit: the raw entry point
    o = Out(need, True, True)
    p = np.ascontiguousarray(poses, np.float32)

    def raw(flags=0, pay_in=d_pay.data_ptr(), pay_out=o.payload.data_ptr(), src=o.src.data_ptr()):
        return lib.scvod_batch_stack_scans(ctx.h, C.c_void_p(d_in.data_ptr()), off.ctypes.data_as(C.c_void_p), 6, p.ctypes.data_as(C.c_void_p), 3, 3,
                                           flags, C.c_void_p(pay_in), C.c_void_p(o.xyzi.data_ptr()), C.c_void_p(pay_out), C.c_void_p(src), need, None)
    assert raw(flags=2) == INVALID
    assert raw(pay_in=d_pay.data_ptr() + 2) == INVALID
    assert raw(pay_out=o.payload.data_ptr() + 1) == INVALID
    assert raw(src=o.src.data_ptr() + 2) == INVALID
    bad = off.copy()
    bad[2] = bad[1] - 1
    assert lib.scvod_batch_stack_scans(ctx.h, C.c_void_p(d_in.data_ptr()), bad.ctypes.data_as(C.c_void_p), 6, p.ctypes.data_as(C.c_void_p), 3, 3, 0,
                                       None, C.c_void_p(o.xyzi.data_ptr()), None, None, need, None) == INVALID
    torch.cuda.synchronize()
    assert o.tails_intact(0)
    assert raw() == 0
    torch.cuda.synchronize()
    assert o.tails_intact(need) and not o.tails_intact(need - 1)


def _small_scans(count, first, stride, keep_every):
    """small synthetic K64-style scans: every keep_every-th return of a synthetic 64-beam sweep (a few thousand points)"""
    import synth
    clouds, labels, poses = [], [], []
    for k in range(count):
        pts, lab, pose = synth.make_scan(5, first + k * stride, "K64", device="cuda")
        clouds.append(pts[k % 3::keep_every].contiguous().cpu().numpy())
        labels.append(lab[k % 3::keep_every].contiguous().cpu().numpy().astype(np.int32).view(np.uint32))
        poses.append(pose)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    return np.concatenate(clouds), off, np.asarray(poses, np.float32), np.concatenate(labels)


def _results(ctx, n_scans, sizes):
    """what a caller can fetch of a processed, clustered, typed batch"""
    out = {"counts": ctx.batch_counts()}
    for s in range(n_scans):
        r = ctx.batch_fetch(s)
        for k, v in r.items():
            out[f"{s}.{k}"] = np.ascontiguousarray(v).copy() if isinstance(v, np.ndarray) else v
        out[f"{s}.clusters"] = ctx.batch_fetch_clusters(s, max(int(sizes[s]), 1))
        out[f"{s}.types"] = ctx.batch_fetch_cluster_types(s, max(int(sizes[s]), 1))
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        va, vb = a[k], b[k]
        if isinstance(va, np.ndarray):
            assert va.shape == vb.shape and va.dtype == vb.dtype, k
            assert np.array_equal(np.ascontiguousarray(va).view(np.uint8), np.ascontiguousarray(vb).view(np.uint8)), k
        else:
            assert va == vb, k


def test_batch_state_is_untouched(scvod, oracle):
    """a ctx that holds a processed, clustered batch: stacking unrelated data changes no result and not the arena"""
    torch = _torch()
    x, off, _, _ = _small_scans(3, 300, 5, 24)
    ctx = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=int(off[-1]) + 64, max_scans=4)
    try:
        d = torch.from_numpy(x).cuda()
        ctx.batch_process(d, off)
        ctx.batch_cluster()
        ctx.batch_cluster_types()
        sizes = np.diff(off)
        before = _results(ctx, 3, sizes)
        arena = ctx.arena_bytes()
        assert ctx.stack_scratch_bytes() == 0                       # no scratch before the first stacking call
        ux, uoff, uposes, upay = _job(3, 1, 41)
        _check(scvod, oracle, ctx, ux, uoff, uposes, upay, 3, 1, False, True, True)
        assert ctx.stack_scratch_bytes() > 0
        assert ctx.arena_bytes() == arena
        _same(before, _results(ctx, 3, sizes))
    finally:
        ctx.close()


def test_stream_order_in_front_of_the_batch_chain(scvod, oracle):
    """on a side stream with one synchronisation at the end of a step: stack -> batch_process(sync=False) -> batch_cluster ->
    batch_cluster_types; the host arrays are overwritten the moment the stacking call returns; two steps of different sizes back to back
    on one ctx, the second step's stacking enqueued before the first step is fetched (it must not disturb the batch).  Against a fresh
    ctx that processed the helper's stacked array uploaded from the host."""
    torch = _torch()
    P = scvod.make_params("semantickitti")
    steps = [_small_scans(9, 300, 5, 24), _small_scans(6, 1200, 3, 40)]
    wants = [stack_ref.stack(oracle, x, off, poses, 3, 3, False, lab) for (x, off, poses, lab) in steps]
    cap = max(int(w["out_offsets"][-1]) for w in wants)
    ctx = scvod.Ctx(P, max_points_total=cap + 64, max_scans=4)
    side = torch.cuda.Stream()
    try:
        dev = [(torch.from_numpy(x).cuda(), torch.from_numpy(lab.view(np.int32)).cuda()) for (x, _, _, lab) in steps]
        outs = [(torch.zeros((int(w["out_offsets"][-1]), 4), device="cuda"), torch.zeros(int(w["out_offsets"][-1]), dtype=torch.int32, device="cuda"))
                for w in wants]
        torch.cuda.synchronize()
        st = side.cuda_stream

        def stack_step(i):
            x, off, poses, lab = steps[i]
            h_off, h_poses = off.copy(), poses.copy()
            out_off, mid = ctx.batch_stack_scans(dev[i][0], h_off, h_poses, outs[i][0], d_payload_in=dev[i][1], d_payload_out=outs[i][1], stream=st)
            h_off[1:] = np.arange(1, len(h_off), dtype=np.int32)      # other valid values, at once
            h_poses[:] = h_poses[::-1] + 3.0
            assert np.array_equal(out_off, wants[i]["out_offsets"]) and np.array_equal(mid, wants[i]["mid"])
            return out_off

        def chain(i, out_off):
            h = out_off.copy()
            ctx.batch_process(outs[i][0], h, stream=st, sync=False)
            h[:] = 0
            ctx.batch_cluster(stream=st, sync=False)
            ctx.batch_cluster_types(stream=st, sync=False)

        off0 = stack_step(0)
        chain(0, off0)
        off1 = stack_step(1)                                        # enqueued behind step 0's chain, before anything is fetched
        side.synchronize()
        got = [_results(ctx, len(off0) - 1, np.diff(off0))]
        chain(1, off1)
        side.synchronize()
        got.append(_results(ctx, len(off1) - 1, np.diff(off1)))
        for i, w in enumerate(wants):
            gi = stack_ref.image(outs[i][0].cpu().numpy(), w["moved"])
            assert np.array_equal(gi, stack_ref.image(w["xyzi"], w["moved"])), i
            assert np.array_equal(outs[i][1].cpu().numpy().view(np.uint32), w["payload"]), i
            assert not np.isnan(w["xyzi"]).any()
            fresh = scvod.Ctx(P, max_points_total=cap + 64, max_scans=4)
            try:
                d = torch.from_numpy(w["xyzi"]).cuda()
                fresh.batch_process(d, w["out_offsets"])
                fresh.batch_cluster()
                fresh.batch_cluster_types()
                ref = _results(fresh, len(w["mid"]), np.diff(w["out_offsets"]))
            finally:
                fresh.close()
            _same(ref, got[i])
            assert ref["counts"][:, 4].sum() > 500 and ref["counts"][:, 6].sum() > 100      # the job does bin points and build voxels
    finally:
        ctx.close()


def test_repeatability(scvod, ctx):
    torch = _torch()
    x, off, poses, payload = _job(3, 1, 77)
    d_in = torch.from_numpy(x).cuda()
    d_pay = torch.from_numpy(payload.view(np.int32)).cuda()
    need = int(stack_ref.offsets(off, 3, 1)[0][-1])
    runs = []
    for _ in range(2):
        o = Out(need, True, True)
        ctx.batch_stack_scans(d_in, off, poses, window=3, interval=1, d_payload_in=d_pay, **o.args())
        torch.cuda.synchronize()
        runs.append(o)
    assert torch.equal(runs[0].xyzi, runs[1].xyzi) and torch.equal(runs[0].payload, runs[1].payload) and torch.equal(runs[0].src, runs[1].src)
