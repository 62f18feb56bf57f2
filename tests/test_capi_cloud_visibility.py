"""The cloud vote (scvod_cloud_visibility_device) without a GPU: the symbols, the struct and its defaults, the argument errors, known
answers worked out by hand on a tiny grid through the brute-force helper (tests/helpers/cloud_visibility_ref.cpp), that helper tied
pair by pair to the pinned helper of the scan stage (visibility_ref.cpp), and against the float64 numpy statement of the rule on a
trajectory far from the origin.  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import cloud_visibility_ref as cr  # noqa: E402
import visibility_ref as vr  # noqa: E402
from test_capi_visibility import _dir, _scans, _tiny  # noqa: E402
from test_gpu_visibility import _cloud, _scene  # noqa: E402

NEW = ("scvod_cloud_visibility_params_default", "scvod_cloud_visibility_device", "scvod_cloud_visibility_stats",
       "scvod_cloud_visibility_scratch_bytes")
INVALID = -1
F = np.float32


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return vr.build(tmp_path_factory.mktemp("visibility_ref"))


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return cr.build(tmp_path_factory.mktemp("cloud_visibility_ref"))


def test_symbols_declared_exported_and_listed(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("cloud_visibility", "cloud_visibility_stats", "cloud_visibility_scratch_bytes"):
        assert callable(getattr(scvod.Ctx, m))
    assert re.search(r"#define\s+SCVOD_CVIS_NO_SORT\s+1\b", hdr) and scvod.CVIS_NO_SORT == 1
    assert len(scvod.CVIS_STATS) == 10
    # the header says what the defaults are worth
    assert "NOT tuned for maps" in hdr and "NOT from real data" in hdr


def test_struct_size_and_defaults(scvod):
    assert C.sizeof(scvod.CloudVisibilityParams) == 32
    p = scvod.cloud_visibility_params_default()
    assert (p.halo, p.min_through, p.vote_num, p.vote_den, p.reserved) == (0, 2, 1, 2, 0)
    assert p.gap_abs == F(0.4) and p.gap_rel == F(0.02) and p.max_range == 0.0
    s = scvod.visibility_params_default()   # the scan stage's values
    assert (p.halo, p.gap_abs, p.gap_rel, p.min_through, p.vote_num, p.vote_den) == (s.halo, s.gap_abs, s.gap_rel, s.min_through, s.vote_num, s.vote_den)
    scvod.load_lib().scvod_cloud_visibility_params_default(None)   # a NULL struct is ignored
    assert scvod.cloud_visibility_params_default(halo=1, max_range=30.0).max_range == 30.0


def test_argument_errors_need_no_device(scvod):
    """SCVOD_ERR_INVALID with no device present, and nothing is written"""
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = C.c_void_p(buf.ctypes.data)
    good = scvod.cloud_visibility_params_default()
    dev = lib.scvod_cloud_visibility_device
    assert dev(None, p, 2, p, None, 1, C.byref(good), 0, p, p, None) == INVALID
    assert dev(None, p, 2, p, None, 1, None, 0, p, p, None) == INVALID                 # no params either
    assert dev(None, p, -1, p, None, 1, C.byref(good), 0, p, p, None) == INVALID
    assert dev(None, p, 2, p, None, -1, C.byref(good), 0, p, p, None) == INVALID
    assert dev(None, p, 2, p, None, 65536, C.byref(good), 0, p, p, None) == INVALID
    for kw in (dict(reserved=1), dict(halo=2), dict(halo=-1), dict(vote_den=0), dict(vote_den=(1 << 20) + 1), dict(vote_num=-1),
               dict(vote_num=(1 << 20) + 1), dict(gap_abs=-0.1), dict(gap_rel=float("nan")), dict(gap_abs=float("inf")),
               dict(max_range=-1.0), dict(max_range=float("inf")), dict(max_range=float("nan"))):
        bad = scvod.cloud_visibility_params_default(**kw)
        assert dev(None, p, 2, p, None, 1, C.byref(bad), 0, p, p, None) == INVALID, kw
    odd = C.c_void_p(buf.ctypes.data + 4)
    assert dev(None, None, 2, p, None, 1, C.byref(good), 0, p, p, None) == INVALID     # a NULL cloud that is not empty
    assert dev(None, p, 2, None, None, 1, C.byref(good), 0, p, p, None) == INVALID     # NULL images of one scan
    assert dev(None, odd, 2, p, None, 1, C.byref(good), 0, p, p, None) == INVALID      # misaligned
    assert dev(None, p, 2, odd, None, 1, C.byref(good), 0, p, p, None) == INVALID
    assert dev(None, p, 2, p, None, 1, C.byref(good), 0, odd, p, None) == INVALID
    assert dev(None, p, 2, p, None, 1, C.byref(good), 2, p, p, None) == INVALID        # an unknown flag
    assert lib.scvod_cloud_visibility_stats(None, p) == INVALID
    assert lib.scvod_cloud_visibility_scratch_bytes(None) == 0
    assert not buf.any()


# ---- known answers on the tiny grid of test_capi_visibility: 36 sectors and 6 azimuth rows of 10 degrees ----
def _images(ref, scvod, P, scans):
    """the range images of sensor-frame scans, by the pinned helper"""
    x, off = _scans(*scans)
    return vr.run(ref, scvod, P, x, off, None, scvod.visibility_params_default(before=0, after=1))["images"]


def _world(*pts):
    p = np.asarray(pts, F).reshape(-1, 3)
    return np.concatenate([p, np.zeros((len(p), 1), F)], 1)


def test_known_answers(scvod, ref, cref):
    P = _tiny(scvod)
    wall, obj, screen = _dir(20.0), _dir(8.0), _dir(3.0)
    # five viewers, four at the origin: one sees the wall behind the object's place, one the object, one a screen in front of it, one
    # looks elsewhere; the fifth stands 1 km away
    scans = [[wall], [obj], [screen], [[-6.0, 6.0, 0.3]], [obj]]
    poses = np.zeros((5, 6), F)
    poses[4, 0] = 1000.0
    img = _images(ref, scvod, P, scans)
    T = cr.matrices(scvod, poses)
    assert T[4].reshape(3, 4)[:, 3].tolist() == [-1000.0, 0.0, 0.0]
    q = _world(obj, wall, [1000.0 + obj[0], obj[1], obj[2]])
    r = cr.run(cref, scvod, P, q, img, T, scvod.cloud_visibility_params_default(min_through=1), pair_classes=True)
    assert r["pair_class"][:, 0].tolist() == [vr.THROUGH, vr.AGREE, vr.OCCLUDED, vr.EMPTY, vr.OUTSIDE]
    assert r["votes"][0].tolist() == [1, 1, 1, 1]                      # OUTSIDE is not counted
    assert r["pair_class"][:, 1].tolist() == [vr.AGREE, vr.OCCLUDED, vr.OCCLUDED, vr.EMPTY, vr.OUTSIDE]
    # the point beside the far viewer: seen by it alone
    assert r["pair_class"][:, 2].tolist() == [vr.OUTSIDE] * 4 + [vr.AGREE] and r["votes"][2].tolist() == [0, 1, 0, 0]
    assert r["verdict"].tolist() == [scvod.VIS_SEEN_THROUGH, scvod.VIS_KEEP, scvod.VIS_KEEP]
    assert r["stats"].tolist() == [3, 3, 1, 2, 0, 1, 3, 3, 2]
    # the far viewer alone counts nothing: UNTESTED
    r = cr.run(cref, scvod, P, q[:2], img[4:], T[4:], scvod.cloud_visibility_params_default())
    assert not r["votes"].any() and r["verdict"].tolist() == [scvod.VIS_UNTESTED] * 2 and r["stats"].tolist() == [2, 2, 0, 0, 2, 0, 0, 0, 0]
    # no scan at all, and records that are not finite
    q2 = _world(obj, [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0])
    r = cr.run(cref, scvod, P, q2, img[:0], T[:0], scvod.cloud_visibility_params_default())
    assert r["verdict"].tolist() == [0, 0, 0] and r["stats"].tolist() == [3, 1, 0, 0, 1, 0, 0, 0, 0]
    r = cr.run(cref, scvod, P, q2, img, T, scvod.cloud_visibility_params_default(min_through=1))
    assert r["votes"].tolist() == [[1, 1, 1, 1], [0] * 4, [0] * 4] and r["verdict"].tolist() == [2, 0, 0]
    assert r["stats"].tolist() == [3, 1, 1, 0, 0, 1, 1, 1, 1]


def test_verdict_rule_on_both_sides(scvod, ref, cref):
    P = _tiny(scvod)
    wall, obj = _dir(20.0), _dir(8.0)
    img = _images(ref, scvod, P, [[wall], [wall], [obj], [_dir(3.0)]])
    T = cr.matrices(scvod, None, 4)
    q = _world(obj)
    for kw, verdict in ((dict(min_through=2), scvod.VIS_SEEN_THROUGH), (dict(min_through=3), scvod.VIS_KEEP),
                        (dict(vote_num=2, vote_den=3), scvod.VIS_SEEN_THROUGH),      # 2 * 3 >= 2 * 3
                        (dict(vote_num=3, vote_den=4), scvod.VIS_KEEP),              # 2 * 4 <  3 * 3
                        (dict(vote_num=1, vote_den=1), scvod.VIS_KEEP), (dict(vote_num=0, vote_den=1), scvod.VIS_SEEN_THROUGH),
                        (dict(min_through=0, vote_num=1 << 20, vote_den=1), scvod.VIS_KEEP)):
        r = cr.run(cref, scvod, P, q, img, T, scvod.cloud_visibility_params_default(**kw))
        assert r["votes"][0].tolist() == [2, 1, 1, 0]       # the OCCLUDED pair does not enter the ratio
        assert r["verdict"][0] == verdict, kw
    # min_through 0 with nothing but an OCCLUDED pair: 0 >= 0 and 0 * den >= num * 0
    r = cr.run(cref, scvod, P, q, img[3:], T[3:], scvod.cloud_visibility_params_default(min_through=0))
    assert r["votes"][0].tolist() == [0, 0, 1, 0] and r["verdict"][0] == scvod.VIS_SEEN_THROUGH


def test_max_range_on_both_sides(scvod, ref, cref):
    """dis' == 8 exactly: max_range 8 keeps the pair (OUTSIDE needs dis' > max_range), the float below 8 drops it"""
    P = _tiny(scvod)
    img = _images(ref, scvod, P, [[[0.0, 20.0, 0.3]]])
    T = cr.matrices(scvod, None, 1)
    q = _world([0.0, 8.0, 0.3])
    below = float(np.nextafter(F(8.0), F(0.0)))
    for max_range, cls in ((0.0, vr.THROUGH), (8.0, vr.THROUGH), (below, vr.OUTSIDE), (7.5, vr.OUTSIDE), (8.5, vr.THROUGH)):
        r = cr.run(cref, scvod, P, q, img, T, scvod.cloud_visibility_params_default(max_range=max_range, min_through=1), pair_classes=True)
        assert r["pair_class"][0].tolist() == [cls], max_range
        assert r["verdict"][0] == (scvod.VIS_SEEN_THROUGH if cls == vr.THROUGH else scvod.VIS_UNTESTED)


@pytest.mark.parametrize("halo", [0, 1])
def test_tie_to_the_pinned_helper(scvod, ref, cref, halo):
    """scan j's points with the matrix the pinned helper built for (j, viewer): every pair gets the pinned helper's class"""
    P = scvod.make_params("semantickitti")
    x, off, poses = _scene(P, sizes=(2500, 2100, 2300), seed=1, tilt=True)
    old = vr.run(ref, scvod, P, x, off, poses, scvod.visibility_params_default(before=2, after=2, halo=halo), pair_classes=True)
    seen = set()
    for j in range(3):
        T = np.zeros((3, 12), F)
        T[:, [0, 5, 10]] = 1.0                              # (row j: the scan itself, not a pair of the pinned helper)
        ks = list(range(old["begin"][j], old["begin"][j + 1]))
        assert len(ks) == 2
        for k in ks:
            T[old["viewers"][k]] = old["T"][k]
        new = cr.run(cref, scvod, P, x[off[j]:off[j + 1]], old["images"], T, scvod.cloud_visibility_params_default(halo=halo), pair_classes=True)
        n_counted = np.zeros(off[j + 1] - off[j], np.int64)
        for k in ks:
            v = int(old["viewers"][k])
            assert np.array_equal(new["pair_class"][v], old["pair_class"][k]), (j, v)
            seen.update(np.unique(old["pair_class"][k]).tolist())
        # and the counters are those classes counted
        for cls, col in ((vr.THROUGH, 0), (vr.AGREE, 1), (vr.OCCLUDED, 2), (vr.EMPTY, 3)):
            want = sum((new["pair_class"][s] == cls).astype(np.int64) for s in range(3))
            assert np.array_equal(new["votes"][:, col], want)
    assert seen == {vr.THROUGH, vr.AGREE, vr.OCCLUDED, vr.OUTSIDE, vr.EMPTY}


def _trajectory(P, n_scans=12, n_pts=2500, seed=11):
    """sensor-frame scans along a curved, tilted path whose world coordinates stay within +-500 m, and their points in the world
    frame (moved in float64, rounded to fp32)"""
    import map_ref as mr
    rng = np.random.default_rng(seed)
    k = np.arange(n_scans)
    poses = np.zeros((n_scans, 6), F)
    poses[:, 0] = 380.0 + 3.0 * k
    poses[:, 1] = -420.0 + 1.5 * k + 0.8 * np.sin(k)
    poses[:, 2] = 12.0 + 0.1 * k
    poses[:, 3] = 0.05 * np.cos(k)
    poses[:, 4] = -0.03 * np.sin(0.7 * k)
    poses[:, 5] = 0.6 + 0.08 * k
    scans = [_cloud(rng, n_pts, P, 0.2 * s) for s in range(n_scans)]
    world = []
    for s in range(n_scans):
        M = mr.pose64(poses[s])[:3]
        w = scans[s][:, :3].astype(np.float64) @ M[:, :3].T + M[:, 3]
        world.append(np.concatenate([w, scans[s][:, 3:4]], 1).astype(F))
    return scans, poses, world


@pytest.mark.parametrize("halo", [0, 1])
def test_helper_against_float64_numpy_far_from_the_origin(scvod, ref, cref, halo):
    """12 scans with tilted poses around (400, -410): every (world point, viewer) pair that the float64 statement marks decided has the
    helper's class, and at most 2 % of the pairs that are not OUTSIDE are left undecided.  The tolerances are classify64's own (1e-3
    bins, 1e-4 m: the fp32 binning of a point given in the sensor frame) plus the rounding of the fp32 transform at these coordinates,
    which classify64 redoes in float64 from the same fp32 matrix and point: a product or partial sum of magnitude <= 512 is off by up
    to 2^-16 = 1.5e-5 m, a coordinate of p' (three products, two large partial sums; the last sum is small) by up to 7.5e-5 m, the
    position across the ray and dis' by up to 1.1e-4 m.  The nearest returns of these clouds are 3 m away, so the direction is off by
    up to 3.7e-5 rad = 2.1e-3 degrees = 1.75e-3 of the 1.2 degree sector bin (1.05e-3 of the 2 degree azimuth bin): edge_tol 3e-3
    bins, depth_tol 2.5e-4 m."""
    P = scvod.make_params("parkinglot")
    g9, dims3 = vr.grid_of(scvod, P)
    scans, poses, world = _trajectory(P)
    assert max(np.abs(w[:, :3]).max() for w in world) < 500.0
    x = np.concatenate(scans).astype(F)
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    images = vr.run(ref, scvod, P, x, off, poses, scvod.visibility_params_default(before=0, after=1))["images"]
    imgs, lows = vr.images64(g9, dims3, x, off)
    T = cr.matrices(scvod, poses)
    prm = scvod.cloud_visibility_params_default(halo=halo)
    q = np.concatenate(world)
    new = cr.run(cref, scvod, P, q, images, T, prm, pair_classes=True)
    live = left_out = 0
    seen = set()
    for v in range(len(scans)):
        cls, decided = vr.classify64(g9, dims3, imgs[v], lows[v], T[v], q[:, :3], halo, prm.gap_abs, prm.gap_rel, edge_tol=3e-3, depth_tol=2.5e-4)
        got = new["pair_class"][v].astype(np.int64)
        bad = decided & (cls != got)
        assert not bad.any(), (v, halo, np.nonzero(bad)[0][:5], cls[bad][:5], got[bad][:5])
        inside = (cls != vr.OUTSIDE) | (got != vr.OUTSIDE)
        live += int(inside.sum())
        left_out += int((inside & ~decided).sum())
        seen.update(np.unique(got).tolist())
    print(f"parkinglot halo {halo}: {left_out} of {live} pairs that are not OUTSIDE left undecided ({100.0 * left_out / live:.3f} %)")
    assert left_out <= 0.02 * live
    assert seen == {vr.THROUGH, vr.AGREE, vr.OCCLUDED, vr.OUTSIDE, vr.EMPTY}
