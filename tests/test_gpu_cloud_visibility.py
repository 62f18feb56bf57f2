"""scvod_cloud_visibility_device (csrc/scvod_cloudvis.hip) against the brute-force helper tests/helpers/cloud_visibility_ref.cpp, bit for
bit: votes, verdicts and stats words 0..8 are np.array_equal on world-frame clouds against the range images of scans of a few thousand
points -- query sizes around the wave, the 512-point chunk and 2048, two sensor grids, both windows, a trajectory long enough that scans are
skipped, points on both sides of the reach, clouds nobody can see, records that are not finite, duplicates, one crowded tile, no scan at
all, zero poses, the scratch, and the verdict as the label of a cleaned map."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import class_map_ref as cmr  # noqa: E402
import cloud_visibility_ref as cr  # noqa: E402
import map_ref as mr  # noqa: E402
from test_gpu_visibility import _cloud  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
CHUNK = 512
SIZES = (2049, 2000, 2048, 2500, 2047, 4500, 3000)


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return cr.build(tmp_path_factory.mktemp("cloud_visibility_ref"))


def _to_world(scan, pose):
    """the records of a sensor-frame scan in the world frame: moved in float64, rounded to fp32"""
    M = mr.pose64(pose)[:3]
    w = scan[:, :3].astype(np.float64) @ M[:, :3].T + M[:, 3]
    return np.concatenate([w, scan[:, 3:4].astype(np.float64)], 1).astype(F)


def _poses(n, step, origin=(0.0, 0.0, 0.0)):
    k = np.arange(n)
    p = np.zeros((n, 6), F)
    p[:, 0] = origin[0] + step * k
    p[:, 1] = origin[1] + 0.15 * step * np.sin(0.9 * k)
    p[:, 2] = origin[2] + 0.02 * k
    p[:, 3] = 0.05 * np.cos(k)       # roll
    p[:, 4] = -0.03 * np.sin(0.7 * k)  # pitch
    p[:, 5] = 0.04 * k               # yaw
    return p


class Scene:
    """sensor-frame scans, their poses, their range images on the device (written by the scan stage) and on the host, the world -> viewer
    matrices, and all their points in the world frame in shuffled order"""

    def __init__(self, scvod, preset, sizes, step, seed, origin=(0.0, 0.0, 0.0)):
        import torch
        self.P = scvod.make_params(preset)
        rng = np.random.default_rng(seed)
        self.scans = [_cloud(rng, n, self.P, 0.2 * s) for s, n in enumerate(sizes)]
        self.poses = _poses(len(sizes), step, origin)
        x = np.concatenate(self.scans).astype(F)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self.ctx = scvod.Ctx(self.P, max_points_total=len(x) + 64, max_scans=len(sizes))
        self.scratch_before = self.ctx.cloud_visibility_scratch_bytes()
        prm = scvod.visibility_params_default(before=0, after=1)
        self.d_images = self.ctx.visibility_device(torch.from_numpy(x).cuda(), off, None, None, prm, None, want=("images",))["images"]
        self.images = self.d_images.cpu().numpy()
        self.T = cr.matrices(scvod, self.poses)
        w = np.concatenate([_to_world(s, p) for s, p in zip(self.scans, self.poses)])
        self.world = np.ascontiguousarray(w[rng.permutation(len(w))])

    def close(self):
        self.ctx.close()


def _device(sc, q, prm, flags=0, poses="scene", images=None):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(q, F).reshape(-1, 4)).cuda()
    out = sc.ctx.cloud_visibility(d, sc.d_images if images is None else images, sc.poses if isinstance(poses, str) else poses, prm, flags)
    got = {"votes": out["votes"].cpu().numpy().view(np.uint16), "verdict": out["verdict"].cpu().numpy()}
    return got, sc.ctx.cloud_visibility_stats()


def _same(scvod, got, stats, want, what=""):
    assert np.array_equal(got["votes"], want["votes"]), f"{what}: votes"
    assert np.array_equal(got["verdict"], want["verdict"]), f"{what}: verdict"
    assert [stats[k] for k in scvod.CVIS_STATS[:9]] == want["stats"].tolist(), what


def _check(scvod, cref, sc, q, prm, flags=0, what="", T=None, poses="scene", images=None):
    want = cr.run(cref, scvod, sc.P, q, sc.images if images is None else images.cpu().numpy(), sc.T if T is None else T, prm)
    got, stats = _device(sc, q, prm, flags, poses, images)
    _same(scvod, got, stats, want, what)
    return got, want, stats


@pytest.fixture(scope="module")
def kitti(scvod):
    sc = Scene(scvod, "semantickitti", SIZES, 0.8, seed=0)
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def park(scvod):
    sc = Scene(scvod, "parkinglot", SIZES, 0.8, seed=1, origin=(120.0, -75.0, 3.0))
    yield sc
    sc.close()


@pytest.mark.parametrize("preset", ["semantickitti", "parkinglot"])
@pytest.mark.parametrize("halo", [0, 1])
def test_query_sizes_around_the_wave_and_the_chunk(scvod, cref, kitti, park, preset, halo):
    sc = kitti if preset == "semantickitti" else park
    prm = scvod.cloud_visibility_params_default(halo=halo)
    for n in (0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 10000):
        got, want, stats = _check(scvod, cref, sc, sc.world[:n], prm, what=f"{preset} halo {halo} n {n}")
        assert stats["points"] == n and stats["steps"] <= -(-n // CHUNK) * len(SIZES)
    # the case is worth something: every class and both tested verdicts occur
    assert (want["stats"][5:] > 0).all() and all((want["verdict"] == v).any() for v in (scvod.VIS_KEEP, scvod.VIS_SEEN_THROUGH))
    # and the order of the input does not matter: the same points in the same order without the sort
    got2, _, _ = _check(scvod, cref, sc, sc.world[:10000], prm, flags=scvod.CVIS_NO_SORT, what="no sort")
    assert all(np.array_equal(got[k], got2[k]) for k in got)


@pytest.fixture(scope="module")
def trajectory(scvod):
    sc = Scene(scvod, "semantickitti", (2200,) * 24, 6.0, seed=2, origin=(-60.0, 40.0, 1.0))
    yield sc
    sc.close()


def test_a_long_trajectory_skips_scans(scvod, cref, trajectory):
    sc = trajectory
    q = sc.world
    prm = scvod.cloud_visibility_params_default(min_through=1)
    got, want, stats = _check(scvod, cref, sc, q, prm, what="trajectory")
    chunks = -(-len(q) // CHUNK)
    assert 0 < stats["steps"] < chunks * 24, "no scan was skipped"
    # a point sees a few of the 24 scans: most pairs are OUTSIDE, and the counted ones are all there
    assert 0 < int(want["stats"][5:].sum()) < 0.5 * len(q) * 24
    got2, _, stats2 = _check(scvod, cref, sc, q, prm, flags=scvod.CVIS_NO_SORT, what="trajectory, no sort")
    assert all(got[k].tobytes() == got2[k].tobytes() for k in got)
    assert stats2["steps"] <= chunks * 24 and [stats2[k] for k in scvod.CVIS_STATS[:9]] == [stats[k] for k in scvod.CVIS_STATS[:9]]
    # the input in scan order is coherent as it is: scans are skipped without the sort too
    w = np.concatenate([_to_world(s, p) for s, p in zip(sc.scans, sc.poses)])
    _, _, stats3 = _check(scvod, cref, sc, w, prm, flags=scvod.CVIS_NO_SORT, what="trajectory in scan order, no sort")
    assert stats3["steps"] < chunks * 24


def _ring(sensor_pose, dis, n, rng):
    """n points in the sensor's horizontal plane (moved to the world) at 2-D distances `dis` [n] from it"""
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    p = np.stack([dis * np.cos(ang), dis * np.sin(ang), rng.uniform(-0.5, 0.5, n), np.zeros(n)], 1)
    return _to_world(p.astype(F), sensor_pose)


@pytest.mark.parametrize("max_range", [0.0, 17.3])
def test_points_around_the_reach(scvod, cref, trajectory, max_range):
    """rings within 5 cm of max_dis (and of max_range) around two sensors, and a tight cluster just outside the reach of a third of which
    a few points are inside: whatever the chunk's bound says, every pair has its exact class"""
    sc = trajectory
    rng = np.random.default_rng(3)
    reach = [float(sc.P.max_dis)] + ([max_range] if max_range > 0 else [])
    parts = []
    for s in (0, 11):
        for r in reach:
            parts.append(_ring(sc.poses[s], r + rng.uniform(-0.05, 0.05, 1500), 1500, rng))
    centre = _ring(sc.poses[23], np.asarray([min(reach) + 0.45]), 1, rng)[0]
    ball = rng.normal(0.0, 1.0, (3000, 3))
    ball = 0.5 * ball / np.linalg.norm(ball, axis=1, keepdims=True) * rng.uniform(0.0, 1.0, (3000, 1)) ** (1.0 / 3.0)
    cluster = np.zeros((3000, 4), F)
    cluster[:, :3] = centre[:3] + ball
    parts.append(cluster)
    q = np.concatenate(parts).astype(F)
    prm = scvod.cloud_visibility_params_default(max_range=max_range, min_through=1)
    want = cr.run(cref, scvod, sc.P, cluster, sc.images[23:], sc.T[23:], prm, pair_classes=True)
    inside = int((want["pair_class"][0] != cr.OUTSIDE).sum())
    assert 0 < inside < 1000, inside      # only a few points of the cluster are in reach of the scan next to it
    for flags in (0, scvod.CVIS_NO_SORT):
        got, want, stats = _check(scvod, cref, sc, q, prm, flags=flags, what=f"reach {max_range} flags {flags}")
    on_ring = cr.run(cref, scvod, sc.P, parts[len(reach) - 1], sc.images[:1], sc.T[:1], prm, pair_classes=True)["pair_class"][0]
    assert (on_ring == cr.OUTSIDE).any() and (on_ring != cr.OUTSIDE).any()   # the ring has points on both sides


def test_all_far(scvod, cref, trajectory):
    """every query within a 10 m ball, 1 km from every sensor: nothing is counted and no scan is looked at"""
    sc = trajectory
    rng = np.random.default_rng(4)
    q = np.zeros((5000, 4), F)
    q[:, :3] = np.asarray([1000.0, -300.0, 5.0]) + rng.uniform(-5.0, 5.0, (5000, 3))
    for flags in (0, scvod.CVIS_NO_SORT):
        got, want, stats = _check(scvod, cref, sc, q, scvod.cloud_visibility_params_default(), flags=flags, what="all far")
        assert (got["verdict"] == scvod.VIS_UNTESTED).all() and not got["votes"].any()
        assert [stats[k] for k in scvod.CVIS_STATS] == [5000, 5000, 0, 0, 5000, 0, 0, 0, 0, 0]


def test_degenerate_inputs(scvod, cref, kitti):
    sc = kitti
    prm = scvod.cloud_visibility_params_default(halo=1, min_through=1)
    q = sc.world[:6000].copy()
    clean = cr.run(cref, scvod, sc.P, q, sc.images, sc.T, prm)
    bad = np.arange(5, 6000, 97)
    q[bad[0::3], 0] = np.nan
    q[bad[1::3], 1] = np.inf
    q[bad[2::3], 2] = -np.inf
    q[3, :3] = (3.0e38, -3.0e38, 0.0)     # finite; its transform is not
    got, want, stats = _check(scvod, cref, sc, q, prm, what="non-finite")
    assert (got["verdict"][bad] == scvod.VIS_UNTESTED).all() and not got["votes"][bad].any()
    ok = np.ones(6000, bool)
    ok[bad] = False
    ok[3] = False
    assert np.array_equal(got["votes"][ok], clean["votes"][ok]) and np.array_equal(got["verdict"][ok], clean["verdict"][ok])
    assert stats["finite"] == 6000 - len(bad)
    # a cloud of nothing but such records
    _check(scvod, cref, sc, np.full((300, 4), np.nan, F), prm, what="all NaN")
    # exact duplicates: every copy gets the same answer
    dup = np.repeat(sc.world[:700], 5, axis=0)
    got, _, _ = _check(scvod, cref, sc, dup, prm, what="duplicates")
    assert all(np.array_equal(got["votes"][k::5], got["votes"][0::5]) for k in range(1, 5))
    # one crowded tile, more than one chunk: 5000 points within 3 m of each other next to sensor 2
    rng = np.random.default_rng(5)
    crowd = np.zeros((5000, 4), F)
    crowd[:, :3] = _to_world(np.asarray([[6.0, 1.0, 0.0, 0.0]], F), sc.poses[2])[0, :3] + rng.uniform(-1.5, 1.5, (5000, 3))
    assert len(np.unique(np.floor(crowd[:, :2] / 8.0), axis=0)) <= 2
    _, want, _ = _check(scvod, cref, sc, crowd, prm, what="one tile")
    assert want["stats"][5:].sum() > 5000
    # no scan at all: every finite point is UNTESTED
    got, _, stats = _check(scvod, cref, sc, q, prm, what="no scans", T=sc.T[:0], poses=sc.poses[:0], images=sc.d_images[:0])
    assert (got["verdict"] == scvod.VIS_UNTESTED).all() and stats["untested"] == stats["finite"] and stats["steps"] == 0
    # NULL poses: the zero pose for every scan
    sens = np.concatenate(sc.scans)[::3]
    _check(scvod, cref, sc, sens, prm, what="zero poses", T=cr.matrices(scvod, None, len(SIZES)), poses=None)


def test_scratch_arena_and_repeat(scvod, cref, park):
    import torch
    sc = park
    assert sc.scratch_before == 0
    fresh = scvod.Ctx(sc.P, max_points_total=4096, max_scans=2)
    assert fresh.cloud_visibility_scratch_bytes() == 0
    prm = scvod.visibility_params_default(before=0, after=1)
    x = np.concatenate(sc.scans[:2]).astype(F)
    img = fresh.visibility_device(torch.from_numpy(x).cuda(), [0, SIZES[0], SIZES[0] + SIZES[1]], None, None, prm, None, want=("images",))["images"]
    arena, vis_stats, vis_scratch = fresh.arena_bytes(), fresh.visibility_stats(), fresh.visibility_scratch_bytes()
    d = torch.from_numpy(sc.world[:9000]).cuda()
    cprm = scvod.cloud_visibility_params_default(halo=1)
    a = fresh.cloud_visibility(d, img, sc.poses[:2], cprm)
    big = fresh.cloud_visibility_scratch_bytes()
    assert big > 16 * 9000
    st = fresh.cloud_visibility_stats()
    want = cr.run(cref, scvod, sc.P, sc.world[:9000], img.cpu().numpy(), sc.T[:2], cprm)
    assert [st[k] for k in scvod.CVIS_STATS[:9]] == want["stats"].tolist()
    assert np.array_equal(a["votes"].cpu().numpy().view(np.uint16), want["votes"]) and np.array_equal(a["verdict"].cpu().numpy(), want["verdict"])
    # a second, smaller call reuses the scratch; a repeat run is bit-identical
    b = fresh.cloud_visibility(d[:3000], img, sc.poses[:2], cprm)
    assert fresh.cloud_visibility_scratch_bytes() == big
    assert torch.equal(b["votes"], a["votes"][:3000]) and torch.equal(b["verdict"], a["verdict"][:3000])
    c = fresh.cloud_visibility(d, img, sc.poses[:2], cprm)
    assert torch.equal(c["votes"], a["votes"]) and torch.equal(c["verdict"], a["verdict"]) and fresh.cloud_visibility_stats() == st
    # nothing else of the ctx moved
    assert fresh.arena_bytes() == arena and fresh.visibility_stats() == vis_stats and fresh.visibility_scratch_bytes() == vis_scratch
    # one output alone
    only = fresh.cloud_visibility(d, img, sc.poses[:2], cprm, want=("verdict",))
    assert list(only) == ["verdict"] and torch.equal(only["verdict"], a["verdict"])
    fresh.close()


def test_argument_errors_on_a_live_ctx(scvod, kitti):
    import torch
    sc = kitti
    d = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    for kw in (dict(halo=2), dict(vote_den=0), dict(gap_abs=-1.0), dict(max_range=float("inf")), dict(reserved=1)):
        with pytest.raises(scvod.ScvodError, match="status -1"):
            sc.ctx.cloud_visibility(d, sc.d_images, sc.poses, scvod.cloud_visibility_params_default(**kw))
    with pytest.raises(scvod.ScvodError, match="status -1"):
        sc.ctx.cloud_visibility(d, sc.d_images, sc.poses, flags=2)
    with pytest.raises(scvod.ScvodError, match="status -1"):
        sc.ctx.cloud_visibility(d.reshape(-1)[1:29].reshape(7, 4), sc.d_images, sc.poses)   # not 16-byte aligned


def _moving_object_scans(P, rng, n_scans=7):
    """a wall 15 m around the sensor and a 0.6 m box at 7 m that moves 2 m to the side from scan to scan"""
    scans, centres = [], []
    for s in range(n_scans):
        n = 4300
        ang = rng.uniform(0.0, 2.0 * np.pi, n)
        az = np.radians(rng.uniform(-10.0, 6.0, n))
        wall = np.stack([15.0 * np.cos(ang), 15.0 * np.sin(ang), 15.0 * np.tan(az), rng.uniform(0, 255, n)], 1)
        th = 0.4 + 0.3 * s
        c = np.asarray([7.0 * np.cos(th), 7.0 * np.sin(th), -0.2])
        box = np.concatenate([c + rng.uniform(-0.3, 0.3, (200, 3)), rng.uniform(0, 255, (200, 1))], 1)
        scans.append(np.concatenate([wall, box]).astype(F))
        centres.append(c)
    return scans, np.asarray(centres)


def test_end_to_end_cleaned_map(scvod, cref):
    """the intended use: a static map of 7 scans in which an object moves, its points voted against the 7 range images, and a cleaned
    labelled map built from the same points with a keep table of everything but SEEN_THROUGH"""
    import torch
    P = scvod.make_params("semantickitti")
    rng = np.random.default_rng(6)
    scans, centres = _moving_object_scans(P, rng)
    poses = np.zeros((7, 6), F)
    poses[:, 0] = 0.2 * np.arange(7)
    centres_w = centres + poses[:, :3]
    x = np.concatenate(scans)
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    ctx = scvod.Ctx(P, max_points_total=len(x) + 64, max_scans=7)
    d = torch.from_numpy(x).cuda()
    imgs = ctx.visibility_device(d, off, None, None, scvod.visibility_params_default(before=0, after=1), None, want=("images",))["images"]
    leaf = 0.2
    static = scvod.StaticMap(1 << 17, leaf=leaf, kind=scvod.MAP_KIND_LABELLED)
    static.accumulate_labelled(d, torch.zeros(len(x), dtype=torch.uint8, device="cuda"), off, poses)
    pts, _ = static.points()
    pts = pts.contiguous()
    prm = scvod.cloud_visibility_params_default()
    out = ctx.cloud_visibility(pts, imgs, poses, prm)
    keep = [v for v in range(256) if v != scvod.VIS_SEEN_THROUGH]
    clean = scvod.StaticMap(1 << 17, leaf=leaf, kind=scvod.MAP_KIND_LABELLED)
    clean.accumulate_labelled(pts, out["verdict"], [0, len(pts)], None, keep=keep)
    torch.cuda.synchronize()
    p = pts.cpu().numpy()
    want = cr.run(cref, scvod, P, p, imgs.cpu().numpy(), cr.matrices(scvod, poses), prm)
    assert np.array_equal(out["verdict"].cpu().numpy(), want["verdict"])
    assert np.array_equal(out["votes"].cpu().numpy().view(np.uint16), want["votes"])
    ek, ev, _ = cmr.definition(scvod, p, want["verdict"], [0, len(p)], None, leaf, keep=cmr.table256(keep))
    gk, gv = mr.sorted_records(clean)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    assert not (cmr.unpack_labelled(gv)[3] == scvod.VIS_SEEN_THROUGH).any() and 0 < len(gk) < len(p)
    on_object = (np.abs(p[:, None, :3] - centres_w[None]).max(2) < 0.35).any(1)
    on_wall = np.abs(np.hypot(p[:, 0] - 0.6, p[:, 1]) - 15.0) < 0.7
    assert (want["verdict"][on_object] == scvod.VIS_SEEN_THROUGH).any()
    assert (want["verdict"][on_wall] == scvod.VIS_KEEP).any()
    static.close()
    clean.close()
    ctx.close()
