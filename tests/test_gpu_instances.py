"""scvod_score_instances_device on the device, through the C-ABI: the instance table against the numpy statement
tests/helpers/instances_ref.py (np.unique, np.add.at, np.minimum.at).  Every comparison is exact: records are compared as bytes, counts
with ==.  Every output buffer carries guard elements behind it, which must stay untouched."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
sys.path.insert(0, os.path.join(HERE, "golden"))
import evaluate_ref as evr  # noqa: E402
import instances_ref as inr  # noqa: E402
import metric  # noqa: E402
from metric_cases import make_case  # noqa: E402
from test_gpu_async_chain import _stream  # noqa: E402
from test_gpu_evaluate import _k6  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4                       # records behind the table, words behind d_n
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -4, -5
REC = inr.DTYPE.itemsize
LDS_SLOTS, TILE = 1024, 2048    # the on-chip table of k_in_aggregate and the points of a tile


@pytest.fixture(scope="module")
def ctx(scvod):
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    yield c
    c.close()


def _cuda(a, dtype):
    import torch
    a = np.ascontiguousarray(a, dtype)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _stats(ctx):
    out = np.full(4, -9, np.int64)
    rc = ctx.lib.scvod_score_instances_stats(ctx.h, out.ctypes.data_as(C.c_void_p))
    return rc, dict(zip(("written", "distinct", "overflow", "spilled_tiles"), (int(v) for v in out)))


def _run(ctx, d_key, d_res, cap, count_only=False, stream=None, sync=True):
    """the call through the C-ABI with guarded outputs -> (status of the stats call, stats, d_n, the records or None)"""
    import torch
    n = int(d_key.numel())
    buf = torch.full(((cap + GUARD) * REC,), 0xA5, dtype=torch.uint8, device="cuda")
    d_n = torch.full((1 + GUARD,), -77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.lib.scvod_score_instances_device(ctx.h, C.c_void_p(d_key.data_ptr()) if n else None, C.c_void_p(d_res.data_ptr()) if n else None, n,
                                              None if count_only else C.c_void_p(buf.data_ptr()), cap, C.c_void_p(d_n.data_ptr()),
                                              C.c_void_p(stream or 0))
    assert rc == 0, ctx.lib.scvod_last_error(ctx.h).decode()
    if not sync:
        return buf, d_n
    return _read(ctx, buf, d_n, cap, count_only)


def _read(ctx, buf, d_n, cap, count_only=False):
    rc, st = _stats(ctx)                        # (synchronises the call's stream)
    h, hn = buf.cpu().numpy(), d_n.cpu().numpy()
    assert (h[cap * REC:] == 0xA5).all(), "records were written behind cap_instances"
    assert (hn[1:] == -77).all(), "written behind d_n"
    if count_only:
        assert (h == 0xA5).all(), "a counting call wrote records"
    got = None
    if hn[0] >= 0 and not count_only:
        got = h[:int(hn[0]) * REC].view(inr.DTYPE)
        assert (h[int(hn[0]) * REC:] == 0xA5).all(), "records were written behind the count"
    return rc, st, int(hn[0]), got


def _check(ctx, keys, res, cap=1024, what=""):
    keys, res = np.asarray(keys, np.uint32), np.asarray(res, np.uint8)
    want = inr.table(keys, res)
    rc, st, n, got = _run(ctx, _cuda(keys, np.uint32), _cuda(res, np.uint8), cap)
    assert rc == 0 and n == len(want), f"{what}: {n} records, status {rc}, want {len(want)}"
    assert got.tobytes() == want.tobytes(), f"{what}: the table differs"
    assert (st["written"], st["distinct"], st["overflow"]) == (len(want), len(want), 0), f"{what}: {st}"
    return want, st


# ---- 1. sizes: around the wave, the workgroup and the tile -------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 5])
def test_sizes(ctx, n):
    for distinct in (1, 7, 300):
        rng = np.random.default_rng(1000 * distinct + n)
        pool = rng.integers(0, 1 << 32, distinct, dtype=np.uint64).astype(np.uint32)
        keys = rng.choice(pool, n)
        res = rng.integers(0, 256, n).astype(np.uint8)          # all eight bits: the upper five must be ignored
        want, st = _check(ctx, keys, res, what=f"n {n}, {distinct} keys")
        assert int(want["n_points"].sum()) == n and st["spilled_tiles"] == 0
    if n == 0:
        assert len(want) == 0


def test_runs_of_equal_keys_and_unaligned_arrays(ctx):
    """scan order: long runs of one label with a few strays, as a labelled cloud has them; then the same arrays from an element further
    in (the keys no longer 16-byte aligned, the bytes no longer 4-byte aligned: the kernel's other load path)"""
    rng = np.random.default_rng(8)
    n = 3 * TILE + 5
    keys = np.repeat(rng.integers(0, 1 << 32, 40, dtype=np.uint64).astype(np.uint32), rng.integers(1, 400, 40))[:n]
    keys = np.concatenate([keys, np.full(n - len(keys), 7, np.uint32)])
    stray = rng.random(n) < 0.02
    keys[stray] = rng.integers(0, 5, int(stray.sum())).astype(np.uint32)
    res = rng.integers(0, 8, n).astype(np.uint8)
    _check(ctx, keys, res, what="runs")
    d_key, d_res = _cuda(np.concatenate([[0], keys]), np.uint32), _cuda(np.concatenate([[0], res]), np.uint8)
    want = inr.table(keys, res)
    for off in (1, 2, 3):
        rc, st, m, got = _run(ctx, d_key[off:], d_res[off:], 1024)
        w = inr.table(keys[off - 1:], res[off - 1:])
        assert rc == 0 and m == len(w) and got.tobytes() == w.tobytes(), f"offset {off}"
    assert len(want) >= 30


# ---- 2. special keys ---------------------------------------------------------------------------------------------------------------------

def test_special_keys(ctx):
    pool = np.array([0, 0xFFFFFFFF, 0x0001000A, 0x0002000A, 0x7FFF000A, 0x8000000A, 0x00050014, 0x00050015, 0x0005FFFF, 0x00050000,
                     0xFFFF0000, 0x0000FFFF, 1, 0x80000000], np.uint32)
    rng = np.random.default_rng(2)
    keys = np.concatenate([pool, rng.choice(pool, 300 - len(pool))])
    res = rng.integers(0, 256, 300).astype(np.uint8)
    want, _ = _check(ctx, keys, res, what="special keys")
    assert want["label"].tolist() == sorted(int(v) for v in pool), "every key, 0 and 0xFFFFFFFF included, is a record of its own"
    # a table of one slot pair: cap_instances 1 with the one key 0, then with the one key 0xFFFFFFFF
    for k in (0, 0xFFFFFFFF):
        _check(ctx, np.full(300, k, np.uint32), res, cap=1, what=f"only key {k:#x}")


# ---- 3. one hot key --------------------------------------------------------------------------------------------------------------------

def test_hot_key_in_sorted_and_shuffled_order(ctx):
    rng = np.random.default_rng(3)
    n = 1_000_000
    rare = (rng.integers(1, 1 << 16, 50).astype(np.uint32) << np.uint32(16)) | np.uint32(252)
    keys = np.full(n, 40, np.uint32)
    at = rng.choice(n, 2000, replace=False)
    keys[at] = rng.choice(rare, 2000)
    res = rng.integers(0, 256, n).astype(np.uint8)
    order = np.argsort(keys, kind="stable")
    ks, rs = keys[order], res[order]
    want, st = _check(ctx, ks, rs, what="hot key, sorted")
    assert len(want) == 1 + len(np.unique(rare)) and int(want["n_points"][0]) == n - 2000 and st["spilled_tiles"] == 0
    perm = np.random.default_rng(4).permutation(n)
    rc, st, m, got = _run(ctx, _cuda(ks[perm], np.uint32), _cuda(rs[perm], np.uint8), 1024)
    assert rc == 0 and m == len(want)
    # the same points in another order: the same sums; first_point is an index into the order it was given
    for f in ("label", "n_points", "n_inlier", "n_preserved"):
        assert got[f].tobytes() == want[f].tobytes(), f
    assert got.tobytes() == inr.table(ks[perm], rs[perm]).tobytes()


def test_more_tiles_than_resident_workgroups(ctx):
    """k_in_aggregate launches four workgroups per compute unit and hands each a run of consecutive tiles: 2.3 M points are 1124 tiles,
    more than the 1024 workgroups of a 256-CU device, so workgroups walk more than one tile and their tables carry over"""
    rng = np.random.default_rng(9)
    n = 2_300_007
    keys = np.repeat(rng.integers(0, 1 << 32, 6000, dtype=np.uint64).astype(np.uint32), rng.integers(1, 800, 6000))[:n]
    assert len(keys) == n
    stray = rng.random(n) < 0.01
    keys[stray] = rng.integers(0, 50, int(stray.sum())).astype(np.uint32)
    res = rng.integers(0, 256, n).astype(np.uint8)
    want, _ = _check(ctx, keys, res, cap=8192, what="2.3 M points")
    assert len(want) > 5000


# ---- 4. every point its own key ------------------------------------------------------------------------------------------------------------

def test_every_point_its_own_key(ctx):
    """The tile-local table has 1024 slots and a tile 2048 points, so the FULL PATH of the on-chip table applies: the two whole tiles
    cannot fit and their surplus keys go straight to the global table (counted as spilled tiles).  The global table has 16384 slots
    for cap_instances 8192: 5000 keys are a load of 0.3."""
    assert LDS_SLOTS < TILE
    rng = np.random.default_rng(5)
    n = 5000
    keys = rng.permutation(np.unique(rng.integers(0, 1 << 32, n + 1000, dtype=np.uint64))[:n]).astype(np.uint32)
    res = rng.integers(0, 256, n).astype(np.uint8)
    want, st = _check(ctx, keys, res, cap=8192, what="own keys")
    assert len(want) == n and (want["n_points"] == 1).all() and np.array_equal(np.sort(want["first_point"]), np.arange(n))
    assert 2 <= st["spilled_tiles"] <= 3


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------------------

def test_capacity(ctx):
    rng = np.random.default_rng(6)
    res = rng.integers(0, 256, 4000).astype(np.uint8)

    def keys_of(distinct):
        pool = (np.arange(distinct, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0xABCD)
        assert len(np.unique(pool)) == distinct
        return np.concatenate([pool, rng.choice(pool, 4000 - distinct)])

    _check(ctx, keys_of(64), res, cap=64, what="exactly cap_instances keys")
    for distinct in (65, 200):                                 # 200: more than the 128 slots of the table
        k = keys_of(distinct)
        rc, st, n, got = _run(ctx, _cuda(k, np.uint32), _cuda(res, np.uint8), 64)
        assert rc == ERR_CAPACITY and n == -1 and got is None, f"{distinct} keys"
        assert st["overflow"] == 1 and st["written"] == 0 and 64 < st["distinct"] <= distinct, st
        with pytest.raises(Exception):
            ctx.score_instances_stats()
        rc, st, n, _ = _run(ctx, _cuda(k, np.uint32), _cuda(res, np.uint8), 64, count_only=True)
        assert rc == ERR_CAPACITY and n == -1 and st["overflow"] == 1
        _check(ctx, keys_of(40), res, cap=64, what=f"a call that fits after {distinct} keys")


# ---- 6. count only, run twice ----------------------------------------------------------------------------------------------------------------

def test_count_only_and_run_twice(scvod, ctx):
    rng = np.random.default_rng(7)
    n = 2 * TILE + 77
    keys = rng.choice(rng.integers(0, 1 << 32, 500, dtype=np.uint64).astype(np.uint32), n)
    res = rng.integers(0, 256, n).astype(np.uint8)
    d_key, d_res = _cuda(keys, np.uint32), _cuda(res, np.uint8)
    rc1, st1, n1, a = _run(ctx, d_key, d_res, 4096)
    rc0, st0, n0, none = _run(ctx, d_key, d_res, 4096, count_only=True)
    rc2, st2, n2, b = _run(ctx, d_key, d_res, 4096)
    assert rc0 == rc1 == rc2 == 0 and n0 == n1 == n2 == len(inr.table(keys, res)) and none is None
    assert st0 == st1 == st2
    assert a.tobytes() == b.tobytes() == inr.table(keys, res).tobytes()
    # the shim: it allocates the output, and reading the stats does not clear them
    d_inst, d_n = ctx.score_instances_device(d_key, d_res, cap_instances=4096)
    st = ctx.score_instances_stats()
    assert st == ctx.score_instances_stats() and st["written"] == n1 == int(d_n.cpu()[0]) and st["overflow"] == 0
    assert d_inst.cpu().numpy()[:n1 * REC].tobytes() == a.tobytes()
    none, d_n = ctx.score_instances_device(d_key, d_res, cap_instances=4096, count_only=True)
    assert none is None and ctx.score_instances_stats() == st and int(d_n.cpu()[0]) == n1


def test_the_measurement_variant_gives_the_same_table(scvod, ctx):
    """scvod_set_score_instances_variant(1): every point adds into the on-chip table on its own (the comparison of
    profiles/instance_score_cost.txt).  The same bytes, also through the full path of the on-chip table"""
    rng = np.random.default_rng(10)
    n = 2 * TILE + 5
    for distinct in (9, 3000):
        keys = rng.choice(rng.integers(0, 1 << 32, distinct, dtype=np.uint64).astype(np.uint32), n)
        res = rng.integers(0, 256, n).astype(np.uint8)
        assert ctx.lib.scvod_set_score_instances_variant(ctx.h, 1) == 0
        try:
            _check(ctx, keys, res, cap=4096, what=f"variant 1, {distinct} keys")
        finally:
            assert ctx.lib.scvod_set_score_instances_variant(ctx.h, 0) == 0
        _check(ctx, keys, res, cap=4096, what=f"variant 0, {distinct} keys")
    assert ctx.lib.scvod_set_score_instances_variant(ctx.h, 2) == ERR_INVALID
    assert ctx.lib.scvod_set_score_instances_variant(None, 0) == ERR_INVALID


# ---- 7. chained with the evaluation ----------------------------------------------------------------------------------------------------------

def test_chained_with_the_evaluation_on_another_stream(scvod, ctx):
    import torch
    g = json.load(open(os.path.join(HERE, "golden", "metric_golden.json")))[1]
    xyz, lab, exyz, elab = make_case(**g["case"])
    lab = (lab | ((np.arange(len(lab), dtype=np.uint32) // np.uint32(97) + np.uint32(1)) << np.uint32(16))).astype(np.uint32)
    want_ev = evr.evaluate(xyz, lab, exyz, elab)
    want = inr.table(lab, want_ev["point_result"])
    n = len(lab)
    d_xyz, d_lab = _cuda(xyz, np.float32).reshape(-1, 3), _cuda(lab, np.uint32)
    d_exyz, d_elab = _cuda(exyz, np.float32).reshape(-1, 3), _cuda(elab, np.uint32)
    d_bytes = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    s = _stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.evaluate_device(d_xyz, d_lab, d_exyz, d_elab, d_point_result=d_bytes, stream=s.cuda_stream)
    buf, d_n = _run(ctx, d_lab, d_bytes[:n], 4096, stream=s.cuda_stream, sync=False)       # no synchronisation in between
    rc, st, m, got = _read(ctx, buf, d_n, 4096)
    assert rc == 0 and m == len(want) and got.tobytes() == want.tobytes()
    assert np.array_equal(d_bytes.cpu().numpy()[:n], want_ev["point_result"])
    ev = ctx.evaluate_stats()
    dyn = np.isin(got["label"] & 0xFFFF, list(metric.DYNAMIC_CLASSES))
    assert dyn.any() and not dyn.all() and len(got) > n // 97
    assert (int(got["n_points"][dyn].sum()), int(got["n_preserved"][dyn].sum())) == (ev["num_gt_dynamic"], ev["num_dynamic_preserved"])
    assert (int(got["n_points"][~dyn].sum()), int(got["n_preserved"][~dyn].sum())) == (ev["num_gt_static"], ev["num_static_preserved"])
    assert int(got["n_inlier"].sum()) == ev["num_preserved"] and ev["num_dynamic_preserved"] > 0 < ev["num_static_preserved"]
    # with no stream given, the call runs on the stream of that evaluation
    ctx.evaluate_device(d_xyz, d_lab, d_exyz, d_elab, d_point_result=d_bytes, stream=s.cuda_stream)
    buf, d_n = _run(ctx, d_lab, d_bytes[:n], 4096, sync=False)
    rc, st, m, got = _read(ctx, buf, d_n, 4096)
    assert rc == 0 and got.tobytes() == want.tobytes()
    # the object rule on top: the helper's numbers
    fin = scvod.instance_finish(got)
    ref = inr.finish(want)
    assert all(fin[k] == ref[k] for k in inr.COUNTS) and fin["hd_gt"] > 0


# ---- 8. batch ------------------------------------------------------------------------------------------------------------------------------

def test_batch_score_instances(scvod):
    import torch
    k = _k6(scvod)
    b, kctx = k["b"], k["ctx"]
    n = int(b.offs[-1])
    lab = (k["gt"] | ((np.arange(n, dtype=np.uint32) // np.uint32(997) + np.uint32(1)) << np.uint32(16))).astype(np.uint32)
    d_lab = _cuda(lab, np.uint32)
    d_bytes = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    kctx.batch_evaluate(d_lab, b.poses.copy(), d_point_result=d_bytes)
    ev = kctx.evaluate_stats()
    h = d_bytes.cpu().numpy()
    assert (h[n:] == 0xA5).all()
    want = inr.table(lab, h[:n])
    kctx.score_instances_device(d_lab, d_bytes[:n], cap_instances=1 << 15)     # (the scratch of this capacity exists from here on)
    kctx.score_instances_stats()
    before = (kctx.arena_bytes(), kctx.evaluate_scratch_bytes(), kctx.score_classes_scratch_bytes(), kctx.score_instances_scratch_bytes())
    labels0 = kctx.batch_point_labels().cpu().numpy()[:n].copy()
    got = kctx.batch_score_instances(d_lab, b.poses.copy(), cap_instances=1 << 15)
    assert got.dtype == inr.DTYPE and got.tobytes() == want.tobytes() and len(got) > n // 997
    ev2 = kctx.evaluate_stats()
    assert all(ev2[c] == ev[c] for c in evr.COUNTS)
    assert (int(got["n_points"].sum()), int(got["n_inlier"].sum())) == (n, ev["num_preserved"])
    assert (kctx.arena_bytes(), kctx.evaluate_scratch_bytes(), kctx.score_classes_scratch_bytes(), kctx.score_instances_scratch_bytes()) == before
    assert before[3] > 40 * (1 << 16)
    assert np.array_equal(kctx.batch_point_labels().cpu().numpy()[:n], labels0)
    # on a stream of the caller's
    s = _stream()
    torch.cuda.synchronize()
    assert kctx.batch_score_instances(d_lab, b.poses.copy(), cap_instances=1 << 15, stream=s.cuda_stream).tobytes() == want.tobytes()
    fin = scvod.instance_finish(got)
    ref = inr.finish(want)
    assert all(fin[c] == ref[c] for c in inr.COUNTS)


# ---- 9. state ------------------------------------------------------------------------------------------------------------------------------

def test_state_and_argument_errors_of_a_live_ctx(scvod):
    import torch
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    out = np.zeros(4, np.int64)
    assert c.score_instances_scratch_bytes() == 0
    assert c.lib.scvod_score_instances_stats(c.h, out.ctypes.data_as(C.c_void_p)) == ERR_STATE
    assert c.lib.scvod_score_instances_stats(c.h, None) == ERR_INVALID
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = C.c_void_p(z.data_ptr())
    dev = c.lib.scvod_score_instances_device
    for args in ((p, p, -1, p, 8, p), (p, p, 1 << 31, p, 8, p), (None, p, 4, p, 8, p), (p, None, 4, p, 8, p), (p, p, 4, p, 0, p),
                 (p, p, 4, p, (1 << 22) + 1, p), (p, p, 4, p, 8, None), (p, p, 4, C.c_void_p(z.data_ptr() + 4), 8, p)):
        assert dev(c.h, *args, None) == ERR_INVALID, args
    assert c.score_instances_scratch_bytes() == 0 and c.evaluate_scratch_bytes() == 0
    assert c.lib.scvod_score_instances_stats(c.h, out.ctypes.data_as(C.c_void_p)) == ERR_STATE
    torch.cuda.synchronize()
    assert not z.cpu().numpy().any()
    # the first call allocates; n == 0 is a call like any other
    rc, st, n, got = _run(c, z[:0].view(torch.int32), z[:0].view(torch.uint8), 16)
    assert rc == 0 and n == 0 and len(got) == 0 and st == dict(written=0, distinct=0, overflow=0, spilled_tiles=0)
    assert c.score_instances_scratch_bytes() >= 40 * 32 + 8 * 8
    c.close()
