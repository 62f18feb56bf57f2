"""scvod_evaluate_device / scvod_batch_evaluate / scvod_classify_map_device on the device, through the C-ABI: counters, rates and the
per-point bytes against the numpy statement tests/helpers/evaluate_ref.py (metric.py's expressions over an exact 1-NN with the
lowest-index tie rule).  Counts and bytes are compared with ==, rates as doubles bit for bit (NaN == NaN)."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
sys.path.insert(0, os.path.join(HERE, "golden"))
import evaluate_ref as evr  # noqa: E402
import metric  # noqa: E402
from metric_cases import make_case  # noqa: E402
from test_gpu_async_chain import SPECS, _batch, _new_ctx, _sorted_records, _stream, _track  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
NO_GROUND, IGNORE_DYNAMIC = 1, 4
ERR_INVALID, ERR_STATE = -1, -5
RATES = ("PR", "RR", "F1")


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


def _same_double(a, b):
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def _assert_result(got, got_bytes, want, what):
    for k in evr.COUNTS:
        assert got[k] == want[k], f"{what}: {k} {got[k]} != {want[k]}"
    for k in RATES:
        assert _same_double(got[k], want[k]), f"{what}: {k} {got[k]!r} != {want[k]!r}"
    if got_bytes is not None:
        assert np.array_equal(got_bytes, want["point_result"]), f"{what}: {int((got_bytes != want['point_result']).sum())} result bytes differ"


def _device(scvod, ctx, gxyz, glab, exyz, elab, voxelsize=0.2, classes=None, with_bytes=True, stream=None):
    import torch
    n = len(gxyz)
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") if with_bytes else None
    par = scvod.eval_params_default(voxelsize=voxelsize, dynamic_classes=classes)
    torch.cuda.synchronize()
    ctx.evaluate_device(_cuda(gxyz, np.float32).reshape(-1, 3), _cuda(glab, np.uint32), _cuda(exyz, np.float32).reshape(-1, 3),
                        _cuda(elab, np.uint32), params=par, d_point_result=buf, stream=stream)
    st = ctx.evaluate_stats()
    if buf is None:
        return st, None
    h = buf.cpu().numpy()
    assert (h[n:] == 0xA5).all(), "result bytes were written behind the gt points"
    return st, h[:n]


def _check(scvod, ctx, gxyz, glab, exyz, elab, what, voxelsize=0.2, classes=None, nn_fn=evr.brute_nn):
    gxyz, exyz = np.asarray(gxyz, np.float32).reshape(-1, 3), np.asarray(exyz, np.float32).reshape(-1, 3)
    glab, elab = np.asarray(glab, np.uint32), np.asarray(elab, np.uint32)
    want = evr.evaluate(gxyz, glab, exyz, elab, voxelsize, classes if classes is not None else metric.DYNAMIC_CLASSES, nn_fn)
    got, got_bytes = _device(scvod, ctx, gxyz, glab, exyz, elab, voxelsize, classes)
    _assert_result(got, got_bytes, want, what)
    return want


# ---- 1. the golden cases: through the helper, the numbers the reference's analysis.py wrote ------------------------------------------

@pytest.mark.parametrize("case", range(3))
def test_golden_cases(scvod, ctx, case):
    g = json.load(open(os.path.join(HERE, "golden", "metric_golden.json")))[case]
    xyz, lab, exyz, elab = make_case(**g["case"])
    want = _check(scvod, ctx, xyz, lab, exyz, elab, f"golden {case}", nn_fn=evr.grid_nn)
    for k in evr.COUNTS:
        assert want[k] == g[k]
    got, _ = _device(scvod, ctx, xyz, lab, exyz, elab, with_bytes=False)  # (without the bytes: the same counters)
    _assert_result(got, None, want, f"golden {case}, counters only")
    assert all(abs(got[k] - g[k]) < 1e-9 for k in RATES)


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------------

def test_ties_go_to_the_lowest_estimate_index(scvod, ctx):
    S, D = 40, 252
    gt = np.array([[3.0, 1.0, 0.5], [3.01, 1.0, 0.5]], np.float32)
    glab = np.array([D, S], np.uint32)
    twin = np.array([[3.0, 1.0, 0.5], [3.0, 1.0, 0.5]], np.float32)
    a = _check(scvod, ctx, gt, glab, twin, [S, D], "twin static first")
    assert a["point_result"].tolist() == [1 | 2, 1] and (a["num_static_preserved"], a["num_dynamic_preserved"]) == (1, 0)
    b = _check(scvod, ctx, gt, glab, twin, [D, S], "twin dynamic first")
    assert b["point_result"].tolist() == [1 | 2 | 4, 1 | 4] and (b["num_static_preserved"], b["num_dynamic_preserved"]) == (0, 1)
    # an equidistant pair on either side of the cell face x = 1.0 (cell edge 0.2): d = 1/256 exactly on both sides
    pair = np.array([[0.9375, 0, 0], [1.0625, 0, 0]], np.float32)
    q = np.array([[1.0, 0, 0]], np.float32)
    assert int(np.floor(0.9375 * 5)) != int(np.floor(1.0625 * 5))
    for order, est_dyn in (([S, D], 0), ([D, S], 4)):
        r = _check(scvod, ctx, q, [D], pair, order, f"face pair {order}")
        assert r["point_result"].tolist() == [1 | 2 | est_dyn]
        r = _check(scvod, ctx, q, [D], pair[::-1], order, f"face pair reversed {order}")
        assert r["point_result"].tolist() == [1 | 2 | est_dyn]


# ---- 3. the inlier edge ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("voxelsize", [0.2, 0.05])
def test_inlier_edge(scvod, ctx, voxelsize):
    limit = voxelsize * np.sqrt(3) / 2
    x = np.float32(limit)
    for _ in range(6):
        x = np.nextafter(x, np.float32(0))
    xs = [x]
    for _ in range(12):
        xs.append(np.nextafter(xs[-1], np.float32(1)))
    xs = np.asarray(xs, np.float32)
    d = xs * xs                                   # the fp32 squared distance to the origin
    inl = np.sqrt(d.astype(np.float64)) < limit
    k = int(inl.sum())
    assert 0 < k < len(xs) and inl[:k].all() and not inl[k:].any(), "the run does not straddle the limit"
    gt = np.zeros((len(xs), 3), np.float32)
    gt[:, 0] = xs
    for axis in range(3):
        g = np.roll(gt, axis, axis=1)
        r = _check(scvod, ctx, g, np.full(len(xs), 40, np.uint32), np.zeros((1, 3), np.float32), [40], f"edge {voxelsize} axis {axis}", voxelsize)
        assert (r["point_result"] & 1).astype(bool).tolist() == inl.tolist() and r["num_preserved"] == k
    # the floats of d themselves, one ulp apart around limit^2: gt on the diagonal of a plane cannot hit them, an axis point whose
    # square rounds to them does
    lo = np.float32(limit * limit)
    ds = [np.nextafter(lo, np.float32(0)), lo, np.nextafter(lo, np.float32(1))]
    want = [bool(np.sqrt(np.float64(v)) < limit) for v in ds]
    assert want[0] and not want[2]
    hit = []
    for v in ds:
        c = np.float32(np.sqrt(np.float64(v)))
        cand = [c, np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(1))]
        hit += [t for t in cand if np.float32(t * t) == v][:1]
    if hit:
        g = np.zeros((len(hit), 3), np.float32)
        g[:, 0] = hit
        _check(scvod, ctx, g, np.full(len(hit), 40, np.uint32), np.zeros((1, 3), np.float32), [40], f"edge {voxelsize} exact d", voxelsize)


# ---- 4. cell faces, negative coordinates, far from the origin ---------------------------------------------------------------------------

@pytest.mark.parametrize("centre", [(0.0, 0.0, 0.0), (-7.0, -3.0, -1.0), (2000.0, -2000.0, 3.0)])
def test_cell_faces_and_offsets(scvod, ctx, centre):
    rng = np.random.default_rng(11)
    k = rng.integers(-12, 13, (400, 3))
    est = (k * np.float32(0.2)).astype(np.float32) + np.asarray(centre, np.float32)       # at multiples of the cell edge
    est[:100] = (k[:100].astype(np.float64) / 5).astype(np.float32) + np.asarray(centre, np.float32)
    elab = rng.choice([40, 252, 70, 255], len(est)).astype(np.uint32)
    gt = np.concatenate([est, est + rng.choice([-0.1, 0.0, 0.1, 0.17], (400, 3)).astype(np.float32),
                         est + rng.normal(0, 0.08, (400, 3)).astype(np.float32)]).astype(np.float32)
    glab = rng.choice([40, 252, 70, 255], len(gt)).astype(np.uint32)
    r = _check(scvod, ctx, gt, glab, est, elab, f"faces {centre}")
    assert 0 < r["num_preserved"] < len(gt) and r["num_dynamic_preserved"] > 0


# ---- 5. aliased buckets ----------------------------------------------------------------------------------------------------------------

def test_aliased_buckets(scvod, ctx):
    rng = np.random.default_rng(12)
    est = rng.uniform(-250, 250, (40, 3)).astype(np.float32)   # 40 points: 1024 buckets for 2500^3 cells
    elab = rng.choice([40, 252], 40).astype(np.uint32)
    gt = np.concatenate([est + rng.normal(0, 0.05, (40, 3)), est + rng.normal(0, 0.12, (40, 3)), rng.uniform(-250, 250, (3000, 3))]).astype(np.float32)
    glab = rng.choice([40, 252], len(gt)).astype(np.uint32)
    # several of a query's 27 probes land in one bucket here (the candidates are then seen twice)
    c = np.floor(gt[:, None, :] * np.float32(5)).astype(np.int64) + np.asarray([[dx, dy, dz] for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])[None]
    c = c.astype(np.uint32)
    b = (c[..., 0] * np.uint32(73856093) ^ c[..., 1] * np.uint32(19349663) ^ c[..., 2] * np.uint32(83492791)) & np.uint32(1023)
    assert any(len(set(row.tolist())) < 27 for row in b), "no query probes a bucket twice"
    r = _check(scvod, ctx, gt, glab, est, elab, "aliased")
    assert 30 <= r["num_preserved"] < 120


# ---- 6. sizes --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_gt", [0, 1, 63, 64, 65, 255, 256, 257])
def test_sizes(scvod, ctx, n_gt):
    rng = np.random.default_rng(100 + n_gt)
    gt = rng.uniform(-1, 1, (n_gt, 3)).astype(np.float32)
    glab = rng.choice([40, 252], n_gt).astype(np.uint32)
    est = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    elab = rng.choice([40, 252], 300).astype(np.uint32)
    r = _check(scvod, ctx, gt, glab, est, elab, f"n_gt {n_gt}")
    assert r["num_gt_static"] + r["num_gt_dynamic"] == n_gt and r["num_est_static"] + r["num_est_dynamic"] == 300
    for n_est in (0, 1):
        r = _check(scvod, ctx, gt, glab, est[:n_est], elab[:n_est], f"n_gt {n_gt} n_est {n_est}")
        if n_est == 0:
            assert r["num_preserved"] == 0 and not (r["point_result"] & 5).any()
    if n_gt == 0:
        assert math.isnan(r["PR"]) and math.isnan(r["RR"]) and math.isnan(r["F1"])


def test_no_dynamic_gt_point_gives_nan_rr(scvod, ctx):
    rng = np.random.default_rng(7)
    gt = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    r = _check(scvod, ctx, gt, np.full(500, 40, np.uint32), gt[::2], np.full(250, 40, np.uint32), "static only")
    assert r["PR"] > 50 and math.isnan(r["RR"]) and math.isnan(r["F1"])


# ---- 7. class lists and instance bits ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("classes", [(7,), tuple(range(100, 116))])
def test_class_lists_and_the_upper_label_bits(scvod, ctx, classes):
    rng = np.random.default_rng(len(classes))
    pool = np.asarray(list(classes) + [40, 252, 99, 116], np.uint32)
    gt = rng.uniform(-2, 2, (1500, 3)).astype(np.float32)
    glab = rng.choice(pool, 1500) | (rng.integers(0, 1 << 16, 1500).astype(np.uint32) << np.uint32(16))   # instance bits on both kinds
    keep = rng.random(1500) < 0.7
    est = (gt[keep] + rng.normal(0, 0.03, (int(keep.sum()), 3))).astype(np.float32)
    elab = glab[keep].copy()
    flip = rng.random(len(elab)) < 0.1
    elab[flip] = rng.choice(pool, int(flip.sum())) | np.uint32(0xABCD0000)
    r = _check(scvod, ctx, gt, glab, est, elab, f"classes {classes}", classes=classes)
    assert r["num_gt_dynamic"] == int(np.isin(glab & 0xFFFF, classes).sum()) > 0 and r["num_dynamic_preserved"] > 0
    assert r["num_static_preserved"] > 0


# ---- 8. every call overwrites the counters of the one before ----------------------------------------------------------------------------

def test_a_second_call_overwrites_the_counters(scvod, ctx):
    rng = np.random.default_rng(3)
    gt = rng.uniform(-1, 1, (2000, 3)).astype(np.float32)
    glab = rng.choice([40, 252], 2000).astype(np.uint32)
    first = _check(scvod, ctx, gt, glab, gt[:1500], glab[:1500], "first")
    second = _check(scvod, ctx, gt[:300], glab[:300], gt[100:200], glab[100:200], "second")
    assert second["num_gt_static"] + second["num_gt_dynamic"] == 300 and first["num_preserved"] > second["num_preserved"]
    again = ctx.evaluate_stats()   # (reading does not clear)
    _assert_result(again, None, second, "read twice")


def test_stats_before_the_first_evaluation(scvod):
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    assert c.evaluate_scratch_bytes() == 0
    assert c.lib.scvod_evaluate_stats(c.h, C.byref(scvod.EVAL_RESULT())) == ERR_STATE
    assert c.lib.scvod_classify_map_stats(c.h, np.zeros(5, np.int64).ctypes.data_as(C.c_void_p)) == ERR_STATE
    # argument errors of a live ctx
    z = np.zeros(16, np.int64).ctypes.data_as(C.c_void_p)
    many = scvod.eval_params_default()
    many.n_dynamic_classes = 17
    assert c.lib.scvod_evaluate_device(c.h, z, z, 1, z, z, 1, C.byref(many), None, None) == ERR_INVALID
    assert c.lib.scvod_evaluate_device(c.h, z, z, -1, z, z, 1, None, None, None) == ERR_INVALID
    assert c.lib.scvod_evaluate_device(c.h, None, z, 1, z, z, 1, None, None, None) == ERR_INVALID
    assert c.lib.scvod_classify_map_device(c.h, z, z, 1, z, 1, z, 1, 0.25, 0.1, None, None) == ERR_INVALID
    assert c.evaluate_scratch_bytes() == 0 and c.arena_bytes() > 0
    c.close()


# ---- 9. the viewer's classes ------------------------------------------------------------------------------------------------------------

def _classify(ctx, orig, ps, static, dynamic, with_bytes=True):
    import torch
    n = len(orig)
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") if with_bytes else None
    torch.cuda.synchronize()
    ctx.classify_map_device(_cuda(orig, np.float32).reshape(-1, 3), _cuda(np.asarray(ps, np.uint8), np.uint8), _cuda(static, np.float32).reshape(-1, 3),
                            _cuda(dynamic, np.float32).reshape(-1, 3), d_class=buf)
    st = ctx.classify_map_stats()
    counts = [st[k] for k in evr.CLASS_NAMES]
    if buf is None:
        return None, counts
    h = buf.cpu().numpy()
    assert (h[n:] == 0xA5).all()
    return h[:n], counts


def test_viewer_classes_by_hand(scvod, ctx):
    static = np.array([[0, 0, 0], [10, 0, 0]], np.float32)
    dynamic = np.array([[5, 0, 0], [20, 0, 0]], np.float32)
    orig = np.array([[0.10, 0, 0], [5.05, 0, 0], [5.12, 0, 0], [5.12, 0, 0], [10.08, 0, 0], [10.12, 0, 0], [50, 0, 0]], np.float32)
    ps = np.array([1, 1, 1, 0, 0, 0, 1], bool)
    want = [metric.TP_STATIC, metric.FN_STATIC, metric.UNMATCHED, metric.TN_DYNAMIC, metric.FN_DYNAMIC, metric.UNMATCHED, metric.UNMATCHED]
    got, counts = _classify(ctx, orig, ps, static, dynamic)
    assert got.tolist() == want == evr.classify(orig, ps, static, dynamic, nn_fn=evr.brute_nn)[0].tolist()
    assert counts == np.bincount(want, minlength=5).tolist()
    # an empty dynamic cloud matches nothing
    got, counts = _classify(ctx, orig, ps, static, np.zeros((0, 3), np.float32))
    assert got.tolist() == evr.classify(orig, ps, static, np.zeros((0, 3), np.float32), nn_fn=evr.brute_nn)[0].tolist()
    assert got[[1, 3]].tolist() == [0, 0] and counts == np.bincount(got, minlength=5).tolist()
    _, counts2 = _classify(ctx, orig, ps, static, np.zeros((0, 3), np.float32), with_bytes=False)
    assert counts2 == counts


def test_viewer_classes_seeded(scvod, ctx):
    rng = np.random.default_rng(21)
    static = rng.uniform(-6, 6, (1500, 3)).astype(np.float32)
    dynamic = rng.uniform(-6, 6, (600, 3)).astype(np.float32)
    orig = np.concatenate([static[:800] + rng.normal(0, 0.06, (800, 3)), dynamic[:500] + rng.normal(0, 0.06, (500, 3)),
                           rng.uniform(-6, 6, (700, 3))]).astype(np.float32)
    ps = rng.random(2000) < 0.6
    want, wc = evr.classify(orig, ps, static, dynamic, nn_fn=evr.brute_nn)
    got, counts = _classify(ctx, orig, ps, static, dynamic)
    assert np.array_equal(got, want) and counts == wc.tolist() and (wc > 0).all()
    # an evaluation in between leaves the class counters alone, and the other way round
    ev = _check(scvod, ctx, orig, np.full(2000, 40, np.uint32), static, np.full(1500, 40, np.uint32), "between")
    st = ctx.classify_map_stats()
    assert [st[k] for k in evr.CLASS_NAMES] == wc.tolist()
    _assert_result(ctx.evaluate_stats(), None, ev, "after the class stats")


# ---- 10. batch mode ---------------------------------------------------------------------------------------------------------------------

BATCH = "K6"
_K6 = {}


def _k6(scvod):
    """the batch, its ground-truth labels, a tracked ctx, and per flag set the device's own label bytes with the helper's answer"""
    if _K6:
        return _K6
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
    ctx.batch_cluster_types()
    _track(ctx, b, b.T, b.nxt, None, 1)
    _K6.update(b=b, d_gt=gt, gt=gt.cpu().numpy().view(np.uint32), ctx=ctx, ref={})
    return _K6


def _k6_ref(scvod, flags):
    k = _k6(scvod)
    if flags not in k["ref"]:
        b = k["b"]
        lab = k["ctx"].batch_point_labels(flags=flags & IGNORE_DYNAMIC).cpu().numpy()[:int(b.offs[-1])]
        k["ref"][flags] = (lab, evr.batch_evaluate(scvod, b.x, b.offs, b.poses, lab, k["gt"], flags))
    return k["ref"][flags]


def _batch_device(k, ctx, flags, stream=None, sync=True):
    import torch
    n = int(k["b"].offs[-1])
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.batch_evaluate(k["d_gt"], k["b"].poses.copy(), flags=flags, d_point_result=buf, stream=stream)
    if not sync:
        return buf
    st = ctx.evaluate_stats()
    h = buf.cpu().numpy()
    assert (h[n:] == 0xA5).all()
    return st, h[:n]


@pytest.mark.parametrize("flags", [0, NO_GROUND, IGNORE_DYNAMIC])
def test_batch_evaluate_against_the_helper(scvod, flags):
    import torch
    k = _k6(scvod)
    b, ctx = k["b"], k["ctx"]
    lab, want = _k6_ref(scvod, flags)
    got, got_bytes = _batch_device(k, ctx, flags)
    _assert_result(got, got_bytes, want, f"{BATCH} flags {flags}")
    assert want["num_gt_dynamic"] > 0 and 0 < want["num_preserved"] < len(lab) and want["num_est_static"] > 0
    if flags == 0:
        assert (lab == 6).any()
    if flags == IGNORE_DYNAMIC:
        assert want["num_est_dynamic"] > 0
    # the compaction cross-check: the export in the world frame with the labels as payload, through scvod_evaluate_device
    n = int(b.offs[-1])
    offs = torch.empty(b.n + 1, dtype=torch.int32, device="cuda")
    xyzi = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    pay = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.batch_export_points(offs, xyzi, flags=flags, poses=b.poses, d_payload_in=k["d_gt"], d_payload_out=pay)
    kept = ctx.batch_export_stats()["kept"]
    assert kept == int(want["keep"].sum())
    est = xyzi[:kept, :3].contiguous()
    assert np.array_equal(est.cpu().numpy().view(np.uint32), want["world"][want["keep"]].view(np.uint32))
    res = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.evaluate_device(_cuda(want["world"], np.float32), k["d_gt"], est, pay[:kept].contiguous(), d_point_result=res)
    _assert_result(ctx.evaluate_stats(), res.cpu().numpy(), want, f"{BATCH} flags {flags}: compaction")


def test_batch_evaluate_state_rules_and_side_effects(scvod):
    import torch
    k = _k6(scvod)
    b, ctx = k["b"], k["ctx"]
    n = int(b.offs[-1])
    pp = b.poses.ctypes.data_as(C.c_void_p)
    gp = C.c_void_p(k["d_gt"].data_ptr())
    # part flags and unknown bits are refused
    for bad in (8, 16, 32, 1 | 8):
        assert ctx.lib.scvod_batch_evaluate(ctx.h, gp, pp, bad, None, None, None) == ERR_INVALID
    assert ctx.lib.scvod_batch_evaluate(ctx.h, None, pp, 0, None, None, None) == ERR_INVALID
    assert ctx.lib.scvod_batch_evaluate(ctx.h, gp, None, 0, None, None, None) == ERR_INVALID
    # nothing of the batch moves: the label bytes, the static map's records, the arena's size
    arena = ctx.arena_bytes()
    lab0 = ctx.batch_point_labels().cpu().numpy()[:n].copy()
    m0 = scvod.StaticMap(1 << 23)
    m0.accumulate(ctx, b.poses)
    rec0 = _sorted_records(m0, None)
    _, want = _k6_ref(scvod, 0)
    got, got_bytes = _batch_device(k, ctx, 0)
    _assert_result(got, got_bytes, want, "before the side-effect check")
    m1 = scvod.StaticMap(1 << 23)
    m1.accumulate(ctx, b.poses)
    assert np.array_equal(ctx.batch_point_labels().cpu().numpy()[:n], lab0) and np.array_equal(_sorted_records(m1, None), rec0)
    assert ctx.arena_bytes() == arena and ctx.evaluate_scratch_bytes() >= 14 * n
    m0.close()
    m1.close()
    # a second ctx on another stream, evaluating at the same time with other flags: each gets its own numbers
    other = _new_ctx(scvod, [b])
    other.batch_process(b.d, b.offs)
    other.batch_cluster()
    other.batch_cluster_types()
    _track(other, b, b.T, b.nxt, None, 1)
    torch.cuda.synchronize()
    s1, s2 = _stream(), _stream()
    buf1 = _batch_device(k, ctx, 0, stream=s1.cuda_stream, sync=False)
    buf2 = _batch_device(k, other, NO_GROUND, stream=s2.cuda_stream, sync=False)
    st2, st1 = other.evaluate_stats(), ctx.evaluate_stats()
    _assert_result(st1, buf1.cpu().numpy()[:n], want, "ctx 1 of two")
    _assert_result(st2, buf2.cpu().numpy()[:n], _k6_ref(scvod, NO_GROUND)[1], "ctx 2 of two")
    assert st1["num_est_static"] != st2["num_est_static"]
    # SCVOD_ERR_STATE before the clustering; SCVOD_ERR_INVALID with a stale tracking result
    other.batch_process(b.d, b.offs)
    assert other.lib.scvod_batch_evaluate(other.h, gp, pp, 0, None, None, None) == ERR_STATE
    assert other.lib.scvod_batch_evaluate(other.h, gp, pp, IGNORE_DYNAMIC, None, None, None) == ERR_STATE
    other.batch_cluster()
    other.batch_cluster_types()
    assert other.lib.scvod_batch_evaluate(other.h, gp, pp, 0, None, None, None) == ERR_INVALID
    other.batch_evaluate(k["d_gt"], b.poses, flags=IGNORE_DYNAMIC)
    _assert_result(other.evaluate_stats(), None, _k6_ref(scvod, IGNORE_DYNAMIC)[1], "without a tracking result")
    other.close()
