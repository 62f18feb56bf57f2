"""scvod_visibility_device / scvod_batch_visibility (csrc/scvod_visibility.hip) against the brute-force helper
tests/helpers/visibility_ref.cpp, bit for bit: votes, verdicts, range images and per-scan counts are np.array_equal on crafted clouds of a
few thousand points per scan -- scan sizes around the 2048-point tile, a small grid and the two sensor grids, both windows, clipped
windows, records that are not finite, one-sided and over-long viewer windows, interleaved chains, tilted poses, a query mask, the batch
form, scratch reuse, and the verdict as the label of a labelled map."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import class_map_ref as cmr  # noqa: E402
import map_ref as mr  # noqa: E402
import visibility_ref as vr  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5
F = np.float32
SIZES = (2049, 0, 2048, 1, 2047, 4500, 3000)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return vr.build(tmp_path_factory.mktemp("visibility_ref"))


def _cloud(rng, n, P, shift):
    """n points of one scan: a wavy wall around the sensor, things in front of it that differ from scan to scan, rays past the range
    and the field of view on every side"""
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    wall = 14.0 + 4.0 * np.sin(3.0 * ang + shift)
    front = rng.random(n) < 0.35
    dis = np.where(front, rng.uniform(0.3, 1.0, n) * wall, wall + rng.normal(0.0, 0.05, n))
    dis = np.where(rng.random(n) < 0.03, rng.uniform(P.max_dis, P.max_dis + 5.0, n), dis)
    wide = rng.uniform(P.min_azimuth - 2.0, min(P.max_azimuth, 60.0) + 2.0, n)
    az = np.radians(np.where(rng.random(n) < 0.2, wide, rng.uniform(max(P.min_azimuth, -26.0), min(P.max_azimuth, 4.0), n)))
    return np.stack([dis * np.cos(ang), dis * np.sin(ang), dis * np.tan(az), rng.uniform(0, 255, n)], 1).astype(F)


def _scene(P, sizes=SIZES, seed=0, tilt=False):
    rng = np.random.default_rng(seed)
    x = np.concatenate([_cloud(rng, n, P, 0.2 * s) for s, n in enumerate(sizes)]).astype(F)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    poses = np.zeros((len(sizes), 6), F)
    poses[:, 0] = 0.8 * np.arange(len(sizes))
    poses[:, 1] = 0.1 * np.sin(np.arange(len(sizes)))
    poses[:, 5] = 0.03 * np.arange(len(sizes))
    if tilt:
        poses[:, 3] = 0.05 * np.cos(np.arange(len(sizes)))   # roll
        poses[:, 4] = -0.04 * np.arange(len(sizes))           # pitch
    return x, off, poses


def _device(ctx, x, off, poses, prm, next_scan=None, mask=None):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(x, F).reshape(-1, 4)).cuda()
    m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()
    out = ctx.visibility_device(d, off, poses, next_scan, prm, m, want=None)
    return _np(out), ctx.visibility_stats()


def _np(out):
    r = {k: v.cpu().numpy() for k, v in out.items()}
    if "votes" in r:
        r["votes"] = r["votes"].view(np.uint32)
    return r


def _same(got, stats, want, what=""):
    assert np.array_equal(got["images"].view(np.uint32), want["images"].view(np.uint32)), f"{what}: images"
    for k in ("votes", "verdict", "scan_counts"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k}"
    sums = want["scan_counts"].sum(0)
    assert [stats[k] for k in ("queries", "seen_through", "through", "agree", "occluded", "outside_or_empty")] == sums.tolist(), what
    assert stats["pairs"] == int(sums[2:].sum())


def _check(ctx, ref, scvod, P, x, off, poses, prm, next_scan=None, mask=None, what=""):
    want = vr.run(ref, scvod, P, x, off, poses, prm, next_scan, mask)
    got, stats = _device(ctx, x, off, poses, prm, next_scan, mask)
    _same(got, stats, want, what)
    return got, want


@pytest.fixture(scope="module")
def kitti(scvod):
    P = scvod.make_params("semantickitti")
    ctx = scvod.Ctx(P, max_points_total=sum(SIZES) + 64, max_scans=len(SIZES))
    yield P, ctx
    ctx.close()


def test_tile_sized_scans_defaults_and_both_windows(scvod, ref, kitti):
    P, ctx = kitti
    x, off, poses = _scene(P)
    assert ctx.visibility_scratch_bytes() == 0
    arena = ctx.arena_bytes()
    got, want = _check(ctx, ref, scvod, P, x, off, poses, scvod.visibility_params_default(), what="defaults")
    # the case is worth something: every class and both verdicts occur, the one-point and the empty scan are there
    sums = want["scan_counts"].sum(0)
    assert (sums > 0).all() and (want["verdict"] == scvod.VIS_KEEP).any()
    assert want["scan_counts"][1].tolist() == [0] * 6 and want["scan_counts"][3, 0] == 1
    assert np.isinf(want["images"][1]).all()
    assert 0 < ctx.visibility_scratch_bytes() and ctx.arena_bytes() == arena
    # the 3 x 3 window: row 0 and columns 0 and S - 1 hold returns, so windows are clipped there and at the seam (row A - 1: the small grid)
    img = want["images"]
    assert all(np.isfinite(img[:, sl[0], sl[1]]).any() for sl in ((0, slice(None)), (slice(None), 0), (slice(None), -1)))
    got1, want1 = _check(ctx, ref, scvod, P, x, off, poses, scvod.visibility_params_default(halo=1), what="halo 1")
    assert not np.array_equal(want1["votes"], want["votes"])
    # a repeat run is bit-identical
    again, _ = _device(ctx, x, off, poses, scvod.visibility_params_default(halo=1))
    assert all(np.array_equal(again[k].view(np.uint8), got1[k].view(np.uint8)) for k in got1)


def test_records_that_are_not_finite_and_the_origin(scvod, ref, kitti):
    P, ctx = kitti
    x, off, poses = _scene(P, sizes=(2500, 2100, 2300), seed=1)
    x[5, 0], x[6, 1], x[7, 2] = np.nan, np.inf, -np.inf
    x[8, :3] = 0.0
    x[2500 + 9, :3] = 0.0
    x[2500 + 10, 0] = np.nan
    x[11, :3] = (3.0e38, 3.0e38, 0.0)   # finite, its distance is not
    x[12, :2] = (5.0, 0.0)              # y == 0: the reference arithmetic
    x[13, :2] = (-5.0, -0.0)
    got, want = _check(ctx, ref, scvod, P, x, off, poses, scvod.visibility_params_default(halo=1), what="non-finite")
    assert (got["votes"][5:8] >> 24 == 2).all()   # OUTSIDE for both viewers of scan 0


@pytest.mark.parametrize("before,after", [(0, 2), (3, 0), (32, 32)])
def test_one_sided_and_over_long_windows(scvod, ref, kitti, before, after):
    P, ctx = kitti
    x, off, poses = _scene(P, sizes=(2100, 2200, 2050, 2300, 2000), seed=2)
    got, want = _check(ctx, ref, scvod, P, x, off, poses, scvod.visibility_params_default(before=before, after=after, min_through=1),
                       what=f"{before}/{after}")
    n_viewers = (want["votes"].astype(np.int64)[:, None] >> np.arange(0, 32, 8) & 255).sum(1)
    if (before, after) == (0, 2):
        assert (n_viewers[off[4]:] == 0).all() and (want["verdict"][off[4]:] == scvod.VIS_UNTESTED).all()
    if (before, after) == (32, 32):
        assert (n_viewers == 4).all()


def test_interleaved_chains_tilted_poses_and_a_mask(scvod, ref, kitti):
    P, ctx = kitti
    x, off, poses = _scene(P, sizes=(2100, 2200, 2050, 2300, 2000, 2150), seed=3, tilt=True)
    nxt = [2, 3, 4, 5, -1, -1]
    _check(ctx, ref, scvod, P, x, off, poses, scvod.visibility_params_default(), next_scan=nxt, what="two chains")
    mask = (np.random.default_rng(4).random(len(x)) < 0.6).astype(np.uint8)
    got, want = _check(ctx, ref, scvod, P, x, off, poses, scvod.visibility_params_default(halo=1), next_scan=nxt, mask=mask, what="mask")
    assert (got["votes"][mask == 0] == 0).all() and (got["verdict"][mask == 0] == scvod.VIS_UNTESTED).all()
    assert want["scan_counts"][:, 0].tolist() == [int(mask[off[s]:off[s + 1]].sum()) for s in range(6)]
    # NULL poses: the zero pose for every scan
    _check(ctx, ref, scvod, P, x, off, None, scvod.visibility_params_default(), what="zero poses")


def test_two_calls_with_different_windows_on_one_ctx(scvod, ref, kitti):
    """the scratch is reused (and grows), the counters are cleared: each call equals the helper on its own"""
    P, ctx = kitti
    x, off, poses = _scene(P, sizes=(2100, 2200, 2050), seed=5)
    _check(ctx, ref, scvod, P, x, off, poses, scvod.visibility_params_default(before=1, after=0), what="first")
    small = ctx.visibility_scratch_bytes()
    x2, off2, poses2 = _scene(P, seed=6)
    _check(ctx, ref, scvod, P, x2, off2, poses2, scvod.visibility_params_default(before=2, after=3, halo=1), what="second")
    assert ctx.visibility_scratch_bytes() >= small
    _check(ctx, ref, scvod, P, x, off, poses, scvod.visibility_params_default(before=1, after=0), what="first again")
    # with d_images left out the images live in the scratch: the other outputs are the same
    import torch
    d = torch.from_numpy(x).cuda()
    prm = scvod.visibility_params_default(before=1, after=0)
    a = _np(ctx.visibility_device(d, off, poses, None, prm, None, want=("votes", "verdict", "scan_counts")))
    b = _np(ctx.visibility_device(d, off, poses, None, prm, None, want=None))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # an empty cloud is a success
    e = _np(ctx.visibility_device(d[:0], [0, 0], None, None, prm, None, want=None))
    assert np.isinf(e["images"]).all() and ctx.visibility_stats()["pairs"] == 0


def test_a_small_grid(scvod, ref):
    P = scvod.make_params(sensor_height=1.0, min_dis=0.5, max_dis=40.0, min_angle=0.0, max_angle=360.0, min_azimuth=-25.0, max_azimuth=25.0,
                          range_res=1.0, sector_res=5.0, azimuth_res=5.0)
    assert scvod.grid_dims(P)[1:3] == (72, 10)
    ctx = scvod.Ctx(P, max_points_total=8192, max_scans=4)
    x, off, poses = _scene(P, sizes=(2500, 2049, 2100), seed=7, tilt=True)
    for halo in (0, 1):
        got, want = _check(ctx, ref, scvod, P, x, off, poses, scvod.visibility_params_default(halo=halo, gap_abs=0.25, gap_rel=0.0),
                           what=f"small grid {halo}")
    # returns in the first and last row and column of every image: the window is clipped on all four borders and at the sector seam
    img = want["images"]
    assert all(np.isfinite(img[:, sl[0], sl[1]]).any(1).all() for sl in ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1)))
    ctx.close()


def test_the_os128_grid_once(scvod, ref):
    P = scvod.make_params("os128_fine")
    assert scvod.grid_dims(P)[1:3] == (600, 120)
    ctx = scvod.Ctx(P, max_points_total=16384, max_scans=2)
    x, off, poses = _scene(P, sizes=(6000, 5500), seed=8)
    _check(ctx, ref, scvod, P, x, off, poses, scvod.visibility_params_default(halo=1, min_through=1), what="os128")
    small = ctx.visibility_scratch_bytes()                     # the images were the caller's
    import torch
    ctx.visibility_device(torch.from_numpy(x).cuda(), off, poses, None, scvod.visibility_params_default(), None, want=("verdict",))
    assert small < 288000 and ctx.visibility_scratch_bytes() >= 2 * 288000   # 288 KB per scan of this grid live in the scratch now
    ctx.close()


def test_argument_errors_on_a_live_ctx(scvod, kitti):
    import torch
    P, ctx = kitti
    d = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    off = [0, 4, 8]
    for kw in (dict(halo=2), dict(before=33), dict(before=0, after=0), dict(vote_den=0), dict(gap_abs=-1.0), dict(gap_rel=float("inf"))):
        with pytest.raises(scvod.ScvodError, match="status -1"):
            ctx.visibility_device(d, off, None, None, scvod.visibility_params_default(**kw))
    with pytest.raises(scvod.ScvodError, match="status -1"):
        ctx.visibility_device(d, [0, 4, 8, 8], None, [2, 2, -1], scvod.visibility_params_default())    # a shared successor
    with pytest.raises(scvod.ScvodError, match="status -1"):
        ctx.visibility_device(d, [0, 6, 4], None, None, scvod.visibility_params_default())              # offsets that decrease
    fresh = scvod.Ctx(P, max_points_total=1024, max_scans=2)
    fresh._n_scans, fresh._n_pts = 1, 8
    with pytest.raises(scvod.ScvodError, match="status -5"):
        fresh.batch_visibility(None)                                                                     # no batch yet
    fresh.close()


@pytest.fixture(scope="module")
def batch(scvod):
    """six thinned synthetic street scans through Patchwork"""
    import synth
    import torch
    P = scvod.make_params("semantickitti")
    scans, poses = [], []
    for idx in range(8, 14):
        pts, _, pose = synth.make_scan(5, idx, "K64")
        scans.append(pts.numpy()[idx % 5::24])
        poses.append(pose)
    x = np.concatenate(scans).astype(F)
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    ctx = scvod.Ctx(P, max_points_total=len(x) + 64, max_scans=len(scans))
    d = torch.from_numpy(x).cuda()
    ctx.batch_process(d, off)
    yield P, ctx, x, off, np.asarray(poses, F), d
    ctx.close()


def test_the_batch_form(scvod, ref, batch):
    P, ctx, x, off, poses, d = batch
    assert 2000 < min(np.diff(off)) and max(np.diff(off)) < 6500
    arena = ctx.arena_bytes()
    prm = scvod.visibility_params_default()
    got = _np(ctx.batch_visibility(poses, params=prm, want=None))
    stats = ctx.visibility_stats()
    assert ctx.arena_bytes() == arena
    mask = np.zeros(len(x), np.uint8)
    for s in range(len(off) - 1):
        mask[off[s] + ctx.batch_fetch(s)["nonground_idx"]] = 1
    assert 0 < mask.sum() < len(x)
    arena = ctx.arena_bytes()   # (a fetch may allocate the PointAPRI side buffer, which counts)
    want = vr.run(ref, scvod, P, x, off, poses, prm, mask=mask)
    _same(got, stats, want, "batch form")
    alone, stats2 = _device(ctx, x, off, poses, prm, mask=mask)
    _same(alone, stats2, want, "standalone form with the batch's mask")
    # every input point with SCVOD_VIS_WITH_GROUND; two interleaved chains
    nxt = [2, 3, 4, 5, -1, -1]
    got = _np(ctx.batch_visibility(poses, nxt, scvod.visibility_params_default(halo=1), scvod.VIS_WITH_GROUND, want=None))
    _same(got, ctx.visibility_stats(), vr.run(ref, scvod, P, x, off, poses, scvod.visibility_params_default(halo=1), nxt), "with ground")
    assert ctx.arena_bytes() == arena
    with pytest.raises(scvod.ScvodError, match="status -1"):
        ctx.batch_visibility(poses, flags=4)
    # the range images alone: the same images, no vote (and no other output may be asked for)
    only = _np(ctx.batch_visibility(poses, flags=scvod.VIS_IMAGES_ONLY, want=("images",)))
    assert np.array_equal(only["images"].view(np.uint32), got["images"].view(np.uint32)) and ctx.visibility_stats()["pairs"] == 0
    with pytest.raises(scvod.ScvodError, match="status -1"):
        ctx.batch_visibility(poses, flags=scvod.VIS_IMAGES_ONLY, want=("images", "verdict"))
    # the batch itself is untouched: the non-ground list is what it was
    assert mask[off[0] + ctx.batch_fetch(0)["nonground_idx"]].all()


def test_the_verdict_gates_a_labelled_map(scvod, ref, batch):
    """the intended use: batch_visibility, then accumulate_labelled with a keep table of everything but SEEN_THROUGH"""
    import torch
    P, ctx, x, off, poses, d = batch
    prm = scvod.visibility_params_default(min_through=1)
    out = ctx.batch_visibility(poses, params=prm, want=("verdict",))
    keep = [v for v in range(256) if v != scvod.VIS_SEEN_THROUGH]
    leaf = 0.2
    m = scvod.StaticMap(1 << 17, leaf=leaf, kind=scvod.MAP_KIND_LABELLED)
    m.accumulate_labelled(d, out["verdict"], off, poses, keep=keep)
    torch.cuda.synchronize()
    mask = np.zeros(len(x), np.uint8)
    for s in range(len(off) - 1):
        mask[off[s] + ctx.batch_fetch(s)["nonground_idx"]] = 1
    want = vr.run(ref, scvod, P, x, off, poses, prm, mask=mask)
    assert (want["verdict"] == scvod.VIS_SEEN_THROUGH).any()
    ek, ev, _ = cmr.definition(scvod, x, want["verdict"], off, poses, leaf, keep=cmr.table256(keep))
    gk, gv = mr.sorted_records(m)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    assert not (cmr.unpack_labelled(gv)[3] == scvod.VIS_SEEN_THROUGH).any()
    m.close()
