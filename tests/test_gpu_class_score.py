"""scvod_batch_point_classes / scvod_score_classes_device / scvod_batch_score_classes on the device, through the C-ABI: the confusion
counts, pd_far, the per-point bytes and the fp32 rates against the numpy statement tests/helpers/class_score_ref.py (an exhaustive fp32
1-NN with the lowest-index tie rule).  Everything is an integer or one fixed fp32 operation: compared with ==, the rates as fp32 bits
(NaN == NaN)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import class_score_ref as csr  # noqa: E402
from test_gpu_async_chain import SPECS, _batch, _new_ctx, _track  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
NO_GROUND, IGNORE_DYNAMIC = 1, 4
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -4, -5
PT_GROUND, PT_REJECTED, PT_UNCLUSTERED, PT_OTHER, PT_CAR, PT_DYNAMIC, PT_BUILDING = 1, 2, 3, 4, 5, 6, 7
LABELS = np.array([40, 50, 70, 10, 252, 44, 60, 81], np.uint32)
BYTES = np.array([0, 1, 2, 3, 4, 5, 6, 7], np.uint8)


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


def _rate_bits(v):
    b = np.asarray(v, np.float32).view(np.uint32).copy()
    b[np.isnan(np.asarray(v, np.float32))] = 0x7FC00000
    return b


def _assert_result(got, got_bytes, want, what):
    assert got["conf"] == want["conf"], f"{what}: conf {got['conf']} != {want['conf']}"
    assert got["pd_far"] == want["pd_far"], f"{what}: pd_far {got['pd_far']} != {want['pd_far']}"
    assert got["num"] == want["num"] and got["P"] == want["P"], what
    for k in ("rate_P", "rate_N"):
        assert np.array_equal(_rate_bits(got[k]), _rate_bits(want[k])), f"{what}: {k} {got[k]} != {want[k]}"
    if got_bytes is not None:
        assert np.array_equal(got_bytes, want["point_result"]), f"{what}: {int((got_bytes != want['point_result']).sum())} result bytes differ"


def _device(scvod, ctx, gxyz, glab, exyz, ept, params=None, with_bytes=True):
    import torch
    n = len(gxyz)
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") if with_bytes else None
    torch.cuda.synchronize()
    ctx.score_classes_device(_cuda(gxyz, np.float32).reshape(-1, 3), _cuda(glab, np.uint32), _cuda(exyz, np.float32).reshape(-1, 3),
                             _cuda(ept, np.uint8), params=params, d_point_result=buf)
    st = ctx.score_classes_stats()
    if buf is None:
        return st, None
    h = buf.cpu().numpy()
    assert (h[n:] == 0xA5).all(), "result bytes were written behind the gt points"
    return st, h[:n]


def _check(scvod, ctx, gxyz, glab, exyz, ept, what, **par):
    gxyz, exyz = np.asarray(gxyz, np.float32).reshape(-1, 3), np.asarray(exyz, np.float32).reshape(-1, 3)
    glab, ept = np.asarray(glab, np.uint32), np.asarray(ept, np.uint8)
    kw = {k: par[k] for k in ("max_dist", "ground", "building", "tree") if k in par}
    want = csr.score(gxyz, glab, exyz, ept, **kw)
    got, got_bytes = _device(scvod, ctx, gxyz, glab, exyz, ept, scvod.class_params_default(**par) if par else None)
    _assert_result(got, got_bytes, want, what)
    assert int(np.sum(got["conf"])) == len(gxyz), f"{what}: the counts do not add up to the truth points"
    return want


# ---- 1. sizes: partial waves, a partial last block, an LDS histogram that sees invalid lanes ---------------------------------------------

@pytest.mark.parametrize("n_gt", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes(scvod, ctx, n_gt):
    rng = np.random.default_rng(100 + n_gt)
    gt = rng.uniform(-1.5, 1.5, (n_gt, 3)).astype(np.float32)
    glab = rng.choice(LABELS, n_gt)
    est = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    ept = rng.choice(BYTES, 300)
    r = _check(scvod, ctx, gt, glab, est, ept, f"n_gt {n_gt}")
    if n_gt == 1000:
        assert all(n > 0 for n in r["num"]) and (np.asarray(r["conf"]) > 0).all()
    got, _ = _device(scvod, ctx, gt, glab, est, ept, with_bytes=False)          # without the bytes: the same counters
    _assert_result(got, None, r, f"n_gt {n_gt}, counters only")
    r0 = _check(scvod, ctx, gt, glab, est[:0], ept[:0], f"n_gt {n_gt} n_est 0")
    assert np.asarray(r0["conf"])[:, :4].sum() == 0 and r0["P"][:3] == [0, 0, 0] and r0["P"][3] == r0["num"][3]
    _check(scvod, ctx, gt, glab, est[:1], ept[:1], f"n_gt {n_gt} n_est 1")
    if n_gt == 0:
        assert np.isnan(r["rate_P"]).all() and np.isnan(r["rate_N"]).all()


# ---- 2. the ring search ---------------------------------------------------------------------------------------------------------------

def _ring_case(seed=31):
    rng = np.random.default_rng(seed)
    est = rng.uniform(-10, 10, (500, 3)).astype(np.float32)
    ept = rng.choice(BYTES, 500)
    j = rng.integers(0, 500, 2000)
    u = rng.normal(0, 1, (2000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    gt = (est[j] + u * rng.uniform(0.2, 0.9, (2000, 1))).astype(np.float32)
    return gt, rng.choice(LABELS, 2000), est, ept


@pytest.mark.parametrize("cell", [0.25, 0.1, 0.7])
def test_every_ring_stops_some_query_and_some_end_without_a_neighbour(scvod, ctx, cell):
    gt, glab, est, ept = _ring_case()
    r = _check(scvod, ctx, gt, glab, est, ept, f"rings, cell {cell}", cell=cell)
    R = int(np.ceil(0.75 / (0.99 * cell)))
    assert R == {0.25: 4, 0.1: 8, 0.7: 2}[cell]
    d = np.sqrt(r["nn_sq"].astype(np.float64))
    inside = d < 0.75
    for ring in range(1, R + 1):   # the queries ring `ring` stops: the candidate is closer than 0.99 ring cells, and no ring before saw that
        band = inside & (d >= 0.99 * (ring - 1) * cell) & (d < 0.99 * ring * cell)
        reachable = 0.99 * ring * cell > 0.2 and 0.99 * (ring - 1) * cell < 0.75     # (the distances start at 0.2 m)
        assert band.sum() > 0 or not reachable, f"no query stops at ring {ring}"
    assert (~inside).sum() > 50 and np.asarray(r["conf"])[:, 4].sum() == (~inside).sum()
    # the second pass took exactly the queries without a candidate inside the first pass's radius
    g1 = np.float32(0.99) * np.float32(cell)
    assert ctx.score_classes_pass2_queries() == int((r["nn_sq"] >= g1 * g1).sum()) > 400


def test_the_stop_rule_does_not_take_an_inner_ring_candidate_that_is_farther(scvod, ctx):
    # cell 0.25: the query sits in cell 0 at x = 0.24; A in cell -1 (ring 1) is 0.48 away, B in cell 2 (ring 2) only 0.27
    q = [[0.24, 0.01, 0.01]]
    a, b = [-0.24, 0.01, 0.01], [0.51, 0.01, 0.01]
    for est, ept, nearest in (([a, b], [PT_GROUND, PT_BUILDING], 1), ([b, a], [PT_BUILDING, PT_GROUND], 0)):
        r = _check(scvod, ctx, q, [40], est, ept, "inner ring farther")
        assert r["nn_idx"].tolist() == [nearest] and r["point_result"].tolist() == [0 | (2 << 2)]   # ground truth, building neighbour: N
    assert ctx.score_classes_pass2_queries() == 1
    # the same along every axis and in the negative direction
    for axis in range(3):
        for sign in (1.0, -1.0):
            pts = np.roll(np.array([q[0], a, b], np.float32) * np.float32(sign), axis, axis=1)
            r = _check(scvod, ctx, pts[:1], [40], pts[1:], [PT_GROUND, PT_BUILDING], f"inner ring farther, axis {axis} sign {sign}")
            assert r["nn_idx"].tolist() == [1]


def test_ties_go_to_the_lowest_estimate_index(scvod, ctx):
    # in one cell: d = 1/256 on both sides
    q = [[0.125, 0.125, 0.125]]
    pair = np.array([[0.0625, 0.125, 0.125], [0.1875, 0.125, 0.125]], np.float32)
    for est in (pair, pair[::-1]):
        r = _check(scvod, ctx, q, [40], est, [PT_GROUND, PT_BUILDING], "tie in a cell")
        assert r["nn_idx"].tolist() == [0] and r["point_result"].tolist() == [0 | (1 << 2) | 32]
        r = _check(scvod, ctx, q, [40], est, [PT_BUILDING, PT_GROUND], "tie in a cell, classes swapped")
        assert r["point_result"].tolist() == [0 | (2 << 2)]
    # in cells of different rings: the query in cell 0 at x = 0.1875, A at -0.1875 (cell -1, ring 1), B at 0.5625 (cell 2, ring 2),
    # d = 0.140625 exactly on both sides, beyond the first pass's radius
    q = [[0.1875, 0.0, 0.0]]
    pair = np.array([[-0.1875, 0.0, 0.0], [0.5625, 0.0, 0.0]], np.float32)
    assert np.floor(pair[:, 0] / 0.25).tolist() == [-1, 2]
    for est in (pair, pair[::-1]):
        r = _check(scvod, ctx, q, [50], est, [PT_GROUND, PT_OTHER], "tie across rings")
        assert r["nn_idx"].tolist() == [0] and r["nn_sq"].tolist() == [0.140625] and r["point_result"].tolist() == [1 | (1 << 2)]
        r = _check(scvod, ctx, q, [50], est, [PT_OTHER, PT_GROUND], "tie across rings, classes swapped")
        assert r["point_result"].tolist() == [1 | (3 << 2) | 32]
    assert ctx.score_classes_pass2_queries() == 1


def test_the_pd_threshold(scvod, ctx):
    r = _check(scvod, ctx, [[0, 0, 0]], [10], [[0.5, 0.5, 0]], [PT_OTHER], "pd at 0.5")
    assert r["nn_sq"].view(np.uint32).tolist() == [np.float32(0.5).view(np.uint32)] and r["point_result"].tolist() == [3 | (3 << 2)]
    assert r["pd_far"] == 0
    r = _check(scvod, ctx, [[0, 0, 0]], [10], [[0.5, 0.5, 2.0 ** -12]], [PT_OTHER], "pd one ulp beyond 0.5")
    assert r["nn_sq"][0] == np.nextafter(np.float32(0.5), np.float32(1)) and r["point_result"].tolist() == [3 | (3 << 2) | 32]
    assert r["pd_far"] == 1
    # the only estimate at 0.80 m: none; N for ground, P for pd
    r = _check(scvod, ctx, [[0, 0, 0], [0, 0, 0]], [40, 10], [[0.8, 0, 0]], [PT_GROUND], "beyond max_dist")
    assert r["point_result"].tolist() == [0 | (4 << 2), 3 | (4 << 2) | 32]
    # a wider max_dist takes it
    r = _check(scvod, ctx, [[0, 0, 0], [0, 0, 0]], [40, 10], [[0.8, 0, 0]], [PT_GROUND], "inside max_dist 1.0", max_dist=1.0)
    assert r["point_result"].tolist() == [0 | (1 << 2) | 32, 3 | (1 << 2) | 32] and r["pd_far"] == 1


def test_a_crowded_cell(scvod, ctx):
    rng = np.random.default_rng(8)
    est = (np.array([3.0, -2.0, 0.5]) + rng.uniform(0.001, 0.249, (5000, 3))).astype(np.float32)
    assert len(np.unique(np.floor(est * np.float32(4.0)), axis=0)) == 1
    ept = rng.choice(BYTES, 5000)
    gt = (np.array([3.125, -1.875, 0.625]) + rng.normal(0, 0.4, (300, 3))).astype(np.float32)
    r = _check(scvod, ctx, gt, rng.choice(LABELS, 300), est, ept, "crowded cell")
    assert 0 < np.asarray(r["conf"])[:, 4].sum() < 300


def test_class_lists_and_the_upper_label_bits(scvod, ctx):
    rng = np.random.default_rng(9)
    est = rng.uniform(-2, 2, (400, 3)).astype(np.float32)
    ept = rng.choice(BYTES, 400)
    gt = (est[rng.integers(0, 400, 1200)] + rng.normal(0, 0.15, (1200, 3))).astype(np.float32)
    pool = np.array([7, 8, 9, 40, 50, 70, 300, 65535], np.uint32)
    glab = rng.choice(pool, 1200) | (rng.integers(0, 1 << 16, 1200).astype(np.uint32) << np.uint32(16))
    r = _check(scvod, ctx, gt, glab, est, ept, "custom lists", ground=[7, 65535], building=[8, 7], tree=[9, 300, 1, 2, 3, 4, 5, 6])
    assert r["num"][0] == int(np.isin(glab & 0xFFFF, [7, 65535]).sum()) > 0 and r["num"][1] == int(((glab & 0xFFFF) == 8).sum()) > 0
    r = _check(scvod, ctx, gt, glab, est, ept, "an empty list", ground=[], tree=[40])
    assert r["num"][0] == 0 and np.isnan(r["rate_P"][0]) and r["num"][2] == int(((glab & 0xFFFF) == 40).sum())
    r = _check(scvod, ctx, gt, glab, est, ept, "default lists, instance bits")
    assert r["num"][:3] == [int(((glab & 0xFFFF) == v).sum()) for v in (40, 50, 70)]


def test_two_runs_of_the_ring_case_are_equal(scvod, ctx):
    gt, glab, est, ept = _ring_case(32)
    a, ab = _device(scvod, ctx, gt, glab, est, ept)
    n2 = ctx.score_classes_pass2_queries()
    b, bb = _device(scvod, ctx, gt, glab, est, ept)
    assert a["conf"] == b["conf"] and a["pd_far"] == b["pd_far"] and np.array_equal(ab, bb) and n2 == ctx.score_classes_pass2_queries() > 0
    assert int(np.sum(a["conf"])) == len(gt)
    _assert_result(a, ab, csr.score(gt, glab, est, ept), "determinism case")


def test_stats_before_the_first_call_and_argument_errors_of_a_live_ctx(scvod):
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    assert c.score_classes_scratch_bytes() == 0
    assert c.lib.scvod_score_classes_stats(c.h, C.byref(scvod.CLASS_RESULT())) == ERR_STATE
    z = np.zeros(16, np.int64).ctypes.data_as(C.c_void_p)
    assert c.lib.scvod_score_classes_device(c.h, z, z, -1, z, z, 1, None, None, None) == ERR_INVALID
    assert c.lib.scvod_score_classes_device(c.h, None, z, 1, z, z, 1, None, None, None) == ERR_INVALID
    for par in (scvod.class_params_default(max_dist=0.7), scvod.class_params_default(cell=0.0), scvod.class_params_default(tree=range(9))):
        assert c.lib.scvod_score_classes_device(c.h, z, z, 1, z, z, 1, C.byref(par), None, None) == ERR_INVALID
    assert c.score_classes_scratch_bytes() == 0 and c.evaluate_scratch_bytes() == 0
    c.close()


# ---- 3. the class byte and the scores of a batch ------------------------------------------------------------------------------------------

BATCH = "R3"   # three K64 scans; the region growing's CPU restatement finds building clusters in every one of them
_R3 = {}


def _r3(scvod):
    if _R3:
        return _R3
    import synth
    import torch
    b = _batch(scvod, BATCH)
    kind, _, first, count, stride, _ = SPECS[BATCH]
    scans = [synth.make_scan(5, first + k * stride, kind, device="cuda") for k in range(count)]
    assert torch.equal(torch.cat([sc[0] for sc in scans]), b.d), "the labels do not belong to the batch's points"
    gt = torch.cat([sc[1] for sc in scans]).to(torch.int32).contiguous()
    ctx = _new_ctx(scvod, [b])
    ctx.batch_process(b.d, b.offs)
    ctx.batch_cluster()
    _R3.update(b=b, d_gt=gt, gt=gt.cpu().numpy().view(np.uint32), ctx=ctx, n=int(b.offs[-1]), rg=None)
    return _R3


def _r3_with(scvod, rg_on):
    """the shared ctx with the region growing off / on (the reference's values), types and tracking current"""
    k = _r3(scvod)
    if k["rg"] is not rg_on:
        k["ctx"].set_region_growing(rg_on)
        k["ctx"].batch_cluster_types()
        _track(k["ctx"], k["b"], k["b"].T, k["b"].nxt, None, 1)
        k["rg"] = rg_on
    return k


def _classes(k, flags=0):
    import torch
    buf = torch.full((k["n"] + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    k["ctx"].batch_point_classes(buf, flags=flags)
    h = buf.cpu().numpy()
    return h[:k["n"]], h[k["n"]:]


def test_point_classes_off_on_off(scvod):
    k = _r3_with(scvod, False)
    ctx, b = k["ctx"], k["b"]
    for flags in (0, IGNORE_DYNAMIC):
        got, guard = _classes(k, flags)
        assert not (got == PT_BUILDING).any() and (guard == 0xA5).all()
        assert np.array_equal(got, ctx.batch_point_labels(flags=flags).cpu().numpy()[:k["n"]])
        assert np.array_equal(got, csr.batch_point_classes(ctx, b.offs, flags))
    k = _r3_with(scvod, True)
    assert ctx.batch_region_growing_stats()["building_clusters"] > 0
    for flags in (0, IGNORE_DYNAMIC):
        got, guard = _classes(k, flags)
        want = csr.batch_point_classes(ctx, b.offs, flags)
        assert np.array_equal(got, want), int((got != want).sum())
        assert (got == PT_BUILDING).sum() > 1000 and (got == PT_OTHER).any() and (guard == 0xA5).all()
        lab = ctx.batch_point_labels(flags=flags).cpu().numpy()[:k["n"]]
        assert not (lab == PT_BUILDING).any() and np.array_equal(np.where(got == PT_BUILDING, PT_OTHER, got), lab)
    k = _r3_with(scvod, False)
    got, _ = _classes(k)
    assert not (got == PT_BUILDING).any()


def test_point_classes_errors(scvod):
    import torch
    k = _r3_with(scvod, True)
    b = k["b"]
    buf = torch.full((k["n"] + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    ctx = k["ctx"]
    assert ctx.lib.scvod_batch_point_classes(ctx.h, p, k["n"] - 1, 0, None) == ERR_CAPACITY
    assert ctx.lib.scvod_batch_point_classes(ctx.h, p, k["n"], 1, None) == ERR_INVALID          # a flag it does not take
    assert ctx.lib.scvod_batch_point_classes(ctx.h, None, k["n"], 0, None) == ERR_INVALID
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0xA5).all(), "a refused call wrote"
    other = _new_ctx(scvod, [b])
    other.batch_process(b.d, b.offs)
    other.batch_cluster()
    assert other.lib.scvod_batch_point_classes(other.h, p, k["n"], 0, None) == ERR_STATE        # before the types
    assert other.lib.scvod_batch_point_classes(other.h, p, k["n"], IGNORE_DYNAMIC, None) == ERR_STATE
    other.batch_cluster_types()
    assert other.lib.scvod_batch_point_classes(other.h, p, k["n"], 0, None) == ERR_INVALID      # no tracking result
    _track(other, b, b.T, b.nxt, None, 1)
    assert other.lib.scvod_batch_point_classes(other.h, p, k["n"], 0, None) == 0
    other.batch_cluster_types()                                                                 # the tracking result is stale now
    assert other.lib.scvod_batch_point_classes(other.h, p, k["n"], 0, None) == ERR_INVALID
    assert other.lib.scvod_batch_score_classes(other.h, C.c_void_p(k["d_gt"].data_ptr()), b.poses.ctypes.data_as(C.c_void_p), 0, None, None, None) == ERR_INVALID
    assert other.lib.scvod_batch_point_classes(other.h, p, k["n"], IGNORE_DYNAMIC, None) == 0
    other.close()


def _batch_device(k, flags):
    import torch
    buf = torch.full((k["n"] + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    k["ctx"].batch_score_classes(k["d_gt"], k["b"].poses.copy(), flags=flags, d_point_result=buf)
    st = k["ctx"].score_classes_stats()
    h = buf.cpu().numpy()
    assert (h[k["n"]:] == 0xA5).all()
    return st, h[:k["n"]]


@pytest.mark.parametrize("flags", [0, NO_GROUND, IGNORE_DYNAMIC])
def test_batch_score_against_the_helper_and_the_device_form(scvod, flags):
    import torch
    k = _r3_with(scvod, True)
    b, ctx, n = k["b"], k["ctx"], k["n"]
    cls = csr.batch_point_classes(ctx, b.offs, flags)
    want = csr.batch_score(scvod, b.x, b.offs, b.poses, cls, k["gt"], flags)
    got, got_bytes = _batch_device(k, flags)
    _assert_result(got, got_bytes, want, f"{BATCH} flags {flags}")
    conf = np.asarray(want["conf"])
    assert int(conf.sum()) == n and all(v > 0 for v in want["num"]) and conf[1, 2] > 0
    if flags == NO_GROUND:
        assert conf[:, 1].sum() == 0 and conf[0, 4] > 0 and want["P"][0] == 0      # the ground truth points: none or mismatches
    else:
        assert conf[0, 1] > 0 and want["rate_P"][0] > 0.5
    # the compaction cross-check: the export in the world frame with its source indices, the class bytes gathered through them
    offs = torch.empty(b.n + 1, dtype=torch.int32, device="cuda")
    xyzi = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.batch_export_points(offs, xyzi, flags=flags, poses=b.poses, d_src_out=src)
    kept = ctx.batch_export_stats()["kept"]
    assert kept == int(want["keep"].sum())
    o = offs.cpu().numpy()
    scan_of = np.repeat(np.arange(b.n), np.diff(o))
    gidx = torch.from_numpy(b.offs[:-1].astype(np.int64)[scan_of]).cuda() + src[:kept].to(torch.int64)
    d_cls = ctx.batch_point_classes(flags=flags & IGNORE_DYNAMIC)
    est_cls = d_cls[gidx].contiguous()
    res = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.score_classes_device(_cuda(want["world"], np.float32), k["d_gt"], xyzi[:kept, :3].contiguous(), est_cls, d_point_result=res)
    _assert_result(ctx.score_classes_stats(), res.cpu().numpy(), want, f"{BATCH} flags {flags}: device form")


def test_the_new_calls_leave_every_other_output_as_it_was(scvod):
    import torch
    k = _r3_with(scvod, True)
    b, ctx, n = k["b"], k["ctx"], k["n"]

    def snapshot():
        offs = torch.empty(b.n + 1, dtype=torch.int32, device="cuda")
        xyzi = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        ctx.batch_export_points(offs, xyzi, poses=b.poses)
        ctx.batch_evaluate(k["d_gt"], b.poses)
        return (ctx.arena_bytes(), ctx.batch_point_labels().cpu().numpy()[:n].copy(), offs.cpu().numpy(), xyzi.cpu().numpy().view(np.uint32),
                ctx.batch_export_stats(), ctx.evaluate_stats(), ctx.evaluate_scratch_bytes())

    before = snapshot()
    _classes(k)
    _batch_device(k, 0)
    assert ctx.score_classes_scratch_bytes() >= 14 * n
    after = snapshot()
    for x, y in zip(before, after):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y)
        elif isinstance(x, dict):
            assert {a: repr(v) for a, v in x.items()} == {a: repr(v) for a, v in y.items()}
        else:
            assert x == y
