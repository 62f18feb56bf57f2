"""The seen-through vote (scvod_visibility_device / scvod_batch_visibility) without a GPU: the symbols, the struct and its defaults, the
argument errors, the viewer lists of the host-only scvod_visibility_viewers, the brute-force helper (tests/helpers/visibility_ref.cpp)
against a float64 numpy statement of the rule on seeded scans, and known answers worked out by hand on a tiny grid.  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import visibility_ref as vr  # noqa: E402

NEW = ("scvod_visibility_params_default", "scvod_visibility_viewers", "scvod_visibility_device", "scvod_batch_visibility",
       "scvod_visibility_stats", "scvod_visibility_scratch_bytes")
INVALID, CAPACITY = -1, -4
F = np.float32


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return vr.build(tmp_path_factory.mktemp("visibility_ref"))


def test_symbols_declared_exported_and_listed(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("visibility_device", "batch_visibility", "visibility_stats", "visibility_scratch_bytes"):
        assert callable(getattr(scvod.Ctx, m))
    for name, value in (("UNTESTED", 0), ("KEEP", 1), ("SEEN_THROUGH", 2), ("WITH_GROUND", 1), ("IMAGES_ONLY", 2), ("MAX_WINDOW", 32)):
        assert re.search(r"#define\s+SCVOD_VIS_%s\s+%d\b" % (name, value), hdr)
        assert getattr(scvod, "VIS_" + name) == value


def test_struct_size_and_defaults(scvod):
    assert C.sizeof(scvod.VisibilityParams) == 32
    p = scvod.visibility_params_default()
    assert (p.before, p.after, p.halo, p.min_through, p.vote_num, p.vote_den) == (2, 2, 0, 2, 1, 2)
    assert p.gap_abs == F(0.4) and p.gap_rel == F(0.02)
    scvod.load_lib().scvod_visibility_params_default(None)   # a NULL struct is ignored
    assert scvod.visibility_params_default(halo=1, after=0).halo == 1


def test_argument_errors_need_no_device(scvod):
    """a NULL ctx is SCVOD_ERR_INVALID whatever else is passed: no device is touched and nothing is written"""
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = C.c_void_p(buf.ctypes.data)
    good = scvod.visibility_params_default()
    off = np.asarray([0, 2], np.int32).ctypes.data_as(C.c_void_p)
    dev, bat = lib.scvod_visibility_device, lib.scvod_batch_visibility
    assert dev(None, p, off, 1, None, None, None, C.byref(good), p, p, p, p, None) == INVALID
    assert dev(None, p, off, 1, None, None, None, None, p, p, p, p, None) == INVALID              # no params either
    assert dev(None, p, off, -1, None, None, None, C.byref(good), p, p, p, p, None) == INVALID
    for kw in (dict(before=-1), dict(after=33), dict(before=0, after=0), dict(halo=2), dict(halo=-1), dict(vote_den=0), dict(vote_den=-3),
               dict(gap_abs=-0.1), dict(gap_rel=float("nan")), dict(gap_abs=float("inf"))):
        bad = scvod.visibility_params_default(**kw)
        assert dev(None, p, off, 1, None, None, None, C.byref(bad), p, p, p, p, None) == INVALID, kw
        assert bat(None, None, None, C.byref(bad), 0, p, p, p, p, None) == INVALID, kw
    odd = C.c_void_p(buf.ctypes.data + 2)
    assert dev(None, odd, off, 1, None, None, None, C.byref(good), p, p, p, p, None) == INVALID   # misaligned
    assert dev(None, p, off, 1, None, None, None, C.byref(good), odd, p, odd, odd, None) == INVALID
    assert bat(None, None, None, C.byref(good), 0, p, p, p, p, None) == INVALID
    assert bat(None, None, None, C.byref(good), 4, p, p, p, p, None) == INVALID                   # an unknown flag
    assert lib.scvod_visibility_stats(None, p) == INVALID
    assert lib.scvod_visibility_scratch_bytes(None) == 0
    assert not buf.any()


def _lists(begin, viewers):
    return [viewers[begin[j]:begin[j + 1]].tolist() for j in range(len(begin) - 1)]


def test_viewer_lists(scvod):
    # NULL: s + 1; fewer viewers at the ends of the chain
    b, v = scvod.visibility_viewers(5, None, before=2, after=2)
    assert _lists(b, v) == [[1, 2], [2, 3, 0], [3, 4, 1, 0], [4, 2, 1], [3, 2]]
    b, v = scvod.visibility_viewers(4, None, before=0, after=1)
    assert _lists(b, v) == [[1], [2], [3], []]
    b, v = scvod.visibility_viewers(4, None, before=3, after=0)
    assert _lists(b, v) == [[], [0], [1, 0], [2, 1, 0]]
    # a window longer than the chain
    b, v = scvod.visibility_viewers(3, None, before=32, after=32)
    assert _lists(b, v) == [[1, 2], [2, 0], [1, 0]]
    # two interleaved chains: 0 -> 2 -> 4, 1 -> 3 -> 5 (the bench layout)
    nxt = [2, 3, 4, 5, -1, -1]
    b, v = scvod.visibility_viewers(6, nxt, before=1, after=2)
    assert _lists(b, v) == [[2, 4], [3, 5], [4, 0], [5, 1], [2], [3]]
    # an external table of the tracking (<= -2) ends the chain inside the batch like -1
    b, v = scvod.visibility_viewers(3, [1, -2, -1], before=1, after=1)
    assert _lists(b, v) == [[1], [0], []]
    # an order that is not ascending
    b, v = scvod.visibility_viewers(3, [-1, 0, 1], before=1, after=1)
    assert _lists(b, v) == [[1], [0, 2], [1]]
    assert _lists(*scvod.visibility_viewers(0, None)) == []
    # and the restatement the reference helper uses agrees
    for n, t, bf, af in ((5, None, 2, 2), (6, nxt, 1, 2), (3, [-1, 0, 1], 1, 1), (7, [3, 4, 5, 6, -1, -1, 1], 3, 2)):
        b, v = scvod.visibility_viewers(n, t, bf, af)
        b2, v2 = vr.viewers_of(n, t, bf, af)
        assert b.tolist() == b2.tolist() and v.tolist() == v2.tolist()


def test_viewer_tables_that_are_refused(scvod):
    lib = scvod.load_lib()

    def raw(table, n, before=2, after=2, cap=64, want=True):
        t = None if table is None else np.asarray(table, np.int32)
        b, v = np.zeros(n + 1 if n >= 0 else 1, np.int32), np.zeros(max(cap, 1), np.int32)
        return lib.scvod_visibility_viewers(None if t is None else t.ctypes.data_as(C.c_void_p), n, before, after,
                                            b.ctypes.data_as(C.c_void_p) if want else None, v.ctypes.data_as(C.c_void_p) if want else None, cap)
    assert raw([1, 2, -1], 3) == 6
    assert raw([2, 2, -1], 3) == INVALID          # two scans name one successor
    assert raw([1, 3, -1], 3) == INVALID          # an index outside the batch
    assert raw([0, 2, -1], 3) == INVALID          # a scan is its own successor
    assert raw([1, 2, 0], 3) == INVALID           # a ring
    assert raw([-1, 2, 1], 3) == INVALID          # a ring beside a chain
    assert raw(None, -1) == INVALID
    assert raw(None, 3, before=0, after=0) == INVALID
    assert raw(None, 3, before=33) == INVALID and raw(None, 3, after=-1) == INVALID
    assert raw(None, 5, cap=3) == CAPACITY
    assert raw(None, 5, cap=0, want=False) == 14  # count only
    with pytest.raises(ValueError):
        vr.viewers_of(3, [2, 2, -1])
    with pytest.raises(ValueError):
        vr.viewers_of(3, [1, 2, 0])


# ---- known answers on a tiny grid: 36 sectors of 10 degrees, 6 azimuth rows of 10 degrees, the sensor at rest ----
def _tiny(scvod):
    return scvod.make_params(sensor_height=1.0, min_dis=0.5, max_dis=50.0, min_angle=0.0, max_angle=360.0, min_azimuth=-30.0, max_azimuth=30.0,
                             range_res=1.0, sector_res=10.0, azimuth_res=10.0)


def _scans(*scans):
    pts = [np.asarray(s, F).reshape(-1, 3) for s in scans]
    x = np.concatenate([np.concatenate([p, np.zeros((len(p), 1), F)], 1) for p in pts]) if pts else np.zeros((0, 4), F)
    return x, np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)


def _dir(dis, z=0.3):
    """a point at 2-D distance `dis` in the direction of 45 degrees (sector 4), azimuth row 3"""
    return [dis * np.sqrt(0.5), dis * np.sqrt(0.5), z]


def _votes(v):
    return [int(v) & 255, (int(v) >> 8) & 255, (int(v) >> 16) & 255, int(v) >> 24]


def test_known_answers(scvod, ref):
    P = _tiny(scvod)
    assert scvod.grid_dims(P)[1:3] == (36, 6)
    wall, obj = _dir(20.0), _dir(8.0)
    prm = scvod.visibility_params_default(before=0, after=2)
    # the object in front of the wall moves away: both later scans look through its place; the wall itself is seen again
    x, off = _scans([wall, obj], [wall], [wall])
    r = vr.run(ref, scvod, P, x, off, None, prm, pair_classes=True)
    assert abs(r["images"][0, 3, 4] - 8.0) < 1e-5 and abs(r["images"][1, 3, 4] - 20.0) < 1e-5 and np.isinf(r["images"][0]).sum() == 36 * 6 - 1
    assert _votes(r["votes"][0]) == [0, 2, 0, 0] and _votes(r["votes"][1]) == [2, 0, 0, 0]
    assert r["verdict"].tolist() == [scvod.VIS_KEEP, scvod.VIS_SEEN_THROUGH, scvod.VIS_KEEP, scvod.VIS_UNTESTED]
    assert _votes(r["votes"][2]) == [0, 1, 0, 0] and r["votes"][3] == 0                        # one viewer, none: the end of the chain
    assert r["scan_counts"].tolist() == [[2, 1, 2, 2, 0, 0], [1, 0, 0, 1, 0, 0], [1, 0, 0, 0, 0, 0]]
    assert [c.tolist() for c in r["pair_class"]] == [[vr.AGREE, vr.THROUGH], [vr.AGREE, vr.THROUGH], [vr.AGREE]]
    # the object is still there: AGREE; a nearer screen: OCCLUDED; sky: EMPTY; above the field of view: OUTSIDE
    screen, high = _dir(3.0), [8.0 * np.sqrt(0.5), 8.0 * np.sqrt(0.5), 8.0]
    x, off = _scans([obj, high], [wall, obj], [screen], [_dir(20.0, z=-8.0)])
    r = vr.run(ref, scvod, P, x, off, None, scvod.visibility_params_default(before=0, after=3), pair_classes=True)
    assert [int(c[0]) for c in r["pair_class"][:3]] == [vr.AGREE, vr.OCCLUDED, vr.EMPTY]
    assert [int(c[1]) for c in r["pair_class"][:3]] == [vr.OUTSIDE] * 3
    assert _votes(r["votes"][0]) == [0, 1, 1, 1] and _votes(r["votes"][1]) == [0, 0, 0, 3]
    assert r["verdict"][:2].tolist() == [scvod.VIS_KEEP, scvod.VIS_KEEP]
    # a query mask: the point that is no query gets 0 and counts nowhere
    r = vr.run(ref, scvod, P, x, off, None, scvod.visibility_params_default(before=0, after=3), mask=[1, 0, 1, 1, 1, 1])
    assert r["votes"][1] == 0 and r["verdict"][1] == scvod.VIS_UNTESTED and r["scan_counts"][0].tolist() == [1, 0, 0, 1, 1, 1]


def test_through_is_strict(scvod, ref):
    """r_min == dis' + gap exactly is not THROUGH: 8.5 == 8 + 0.5 with gap_rel 0, every number exact in fp32"""
    P = _tiny(scvod)
    prm = scvod.visibility_params_default(before=0, after=1, gap_abs=0.5, gap_rel=0.0, min_through=1)
    for far, cls in ((8.5, vr.AGREE), (float(np.nextafter(F(8.5), F(9.0))), vr.THROUGH), (8.0, vr.AGREE)):
        x, off = _scans([[0.0, 8.0, 0.3]], [[0.0, far, 0.3]])
        r = vr.run(ref, scvod, P, x, off, None, prm, pair_classes=True)
        assert r["pair_class"][0].tolist() == [cls], far
        assert r["verdict"][0] == (scvod.VIS_SEEN_THROUGH if cls == vr.THROUGH else scvod.VIS_KEEP)


def test_halo_window_is_clipped_not_wrapped(scvod, ref):
    """halo 1 looks at the pixels around; the last sector does not see the first across the seam"""
    P = _tiny(scvod)

    def at(deg, dis, z=0.3):
        return [dis * np.cos(np.radians(deg)), dis * np.sin(np.radians(deg)), z]
    # the query in sector 4; the viewer's only return one sector on: EMPTY without the halo, AGREE with it
    x, off = _scans([at(45.0, 8.0)], [at(55.0, 8.0)])
    for halo, cls in ((0, vr.EMPTY), (1, vr.AGREE)):
        r = vr.run(ref, scvod, P, x, off, None, scvod.visibility_params_default(before=0, after=1, halo=halo), pair_classes=True)
        assert r["pair_class"][0].tolist() == [cls]
    # sector 35 and sector 0 are neighbours on the sensor but not in the image
    x, off = _scans([at(355.0, 8.0), at(5.0, 8.0)], [at(5.0, 8.0)])
    r = vr.run(ref, scvod, P, x, off, None, scvod.visibility_params_default(before=0, after=1, halo=1), pair_classes=True)
    assert r["pair_class"][0].tolist() == [vr.EMPTY, vr.AGREE]


def test_verdict_rule_on_both_sides(scvod, ref):
    P = _tiny(scvod)
    wall, obj = _dir(20.0), _dir(8.0)
    # three viewers: two look through, one agrees
    x, off = _scans([obj], [wall], [wall], [obj])
    for kw, verdict in ((dict(min_through=2), scvod.VIS_SEEN_THROUGH), (dict(min_through=3), scvod.VIS_KEEP),
                        (dict(vote_num=2, vote_den=3), scvod.VIS_SEEN_THROUGH),      # 2 * 3 >= 2 * 3
                        (dict(vote_num=3, vote_den=4), scvod.VIS_KEEP),              # 2 * 4 <  3 * 3
                        (dict(vote_num=1, vote_den=1), scvod.VIS_KEEP), (dict(vote_num=0, vote_den=1), scvod.VIS_SEEN_THROUGH)):
        r = vr.run(ref, scvod, P, x, off, None, scvod.visibility_params_default(before=0, after=3, **kw))
        assert _votes(r["votes"][0]) == [2, 1, 0, 0]
        assert r["verdict"][0] == verdict, kw
    # OCCLUDED and OUTSIDE pairs do not enter the ratio
    x, off = _scans([obj], [wall], [wall], [_dir(3.0)])
    r = vr.run(ref, scvod, P, x, off, None, scvod.visibility_params_default(before=0, after=3, vote_num=1, vote_den=1))
    assert _votes(r["votes"][0]) == [2, 0, 1, 0] and r["verdict"][0] == scvod.VIS_SEEN_THROUGH


def test_a_moving_sensor_uses_the_pose_delta(scvod, ref):
    """the viewer stands 5 m further on: the wall 20 m ahead of the first pose is 15 m ahead of the second"""
    P = _tiny(scvod)
    poses = np.asarray([[0, 0, 0, 0, 0, 0], [5, 0, 0, 0, 0, 0]], F)
    x, off = _scans([[20.0, 1.0, 0.3], [8.0, 0.5, 0.3]], [[15.0, 1.0, 0.3]])
    r = vr.run(ref, scvod, P, x, off, poses, scvod.visibility_params_default(before=1, after=1, min_through=1), pair_classes=True)
    assert r["T"][0].reshape(3, 4)[:, 3].tolist() == [-5.0, 0.0, 0.0]
    assert r["pair_class"][0].tolist() == [vr.AGREE, vr.THROUGH]   # (8, 0.5) is (3, 0.5) for the viewer: the same sector, 3 m < 15 m
    assert r["pair_class"][1].tolist() == [vr.OCCLUDED]             # and back: (15, 1) is (20, 1) for scan 0, behind its object at 8 m
    assert r["verdict"].tolist() == [scvod.VIS_KEEP, scvod.VIS_SEEN_THROUGH, scvod.VIS_KEEP]


@pytest.mark.parametrize("kind,preset,halos", [("K64", "semantickitti", (0,)), ("PARK", "parkinglot", (0, 1))])
def test_helper_against_float64_numpy(scvod, ref, kind, preset, halos):
    """on seeded scans every (point, viewer) pair that sits on no threshold gets the class the float64 statement gives it, and at most
    2 % of the pairs sit on one.  (The top beam of the synthetic K64 sensor points at exactly 2.0 degrees, an azimuth bin edge of the
    SemanticKITTI grid: 1.4 % of its points are edge cases by construction, and a 3-row window meets that row three times as often --
    3.05 % of the pairs left out, measured -- so the 3 x 3 window is checked on the PARK sensor, which has no beam on an edge.)"""
    import synth
    P = scvod.make_params(preset)
    g9, dims3 = vr.grid_of(scvod, P)
    scans, poses = [], []
    for idx in (9, 10, 11):
        pts, _, pose = synth.make_scan(5, idx, kind)
        scans.append(pts.numpy())
        poses.append(pose)
    x = np.concatenate(scans).astype(F)
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    imgs, lows = vr.images64(g9, dims3, x, off)
    for halo in halos:
        prm = scvod.visibility_params_default(before=1, after=1, halo=halo)
        r = vr.run(ref, scvod, P, x, off, np.asarray(poses, F), prm, pair_classes=True)
        total = left_out = 0
        seen = set()
        for j in range(3):
            for k in range(r["begin"][j], r["begin"][j + 1]):
                v = int(r["viewers"][k])
                cls, decided = vr.classify64(g9, dims3, imgs[v], lows[v], r["T"][k], x[off[j]:off[j + 1], :3], halo, prm.gap_abs, prm.gap_rel)
                got = r["pair_class"][k].astype(np.int64)
                bad = decided & (cls != got)
                assert not bad.any(), (j, v, halo, np.nonzero(bad)[0][:5], cls[bad][:5], got[bad][:5])
                total += len(cls)
                left_out += int((~decided).sum())
                seen.update(np.unique(got).tolist())
        print(f"{kind} halo {halo}: {left_out} of {total} pairs left out ({100.0 * left_out / total:.3f} %)")
        assert left_out <= 0.02 * total
        assert {vr.THROUGH, vr.AGREE, vr.OCCLUDED, vr.OUTSIDE}.issubset(seen)
