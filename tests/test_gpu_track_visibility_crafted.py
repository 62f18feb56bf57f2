"""scvod_track_visibility_device on crafted tables: every output byte against the sequential numpy statement of the rule
(tests/helpers/track_visibility_ref.py), with 0xA5 guard regions in front of and behind every output.  The tables are small dicts turned
into 64-byte records by object_tracks_ref.build_table and linked by the device's own tracks stage (ctx.object_tracks_device); a test
that needs a broken table damages the linked one.  The sizes are those at which a kernel takes another path: tracks of 1 / 2 / 63 / 64 /
65 / 129 / 1025 members (the wave walks a track 64 at a time), windows that clamp at either end, point counts around 16 (a lane's run),
64 and 1024 (a wave's), byte pointers at every kind of offset from a 16-byte boundary.  The SCVOD_ERR_STATE of the stats call needs a
ctx and therefore a device: it is checked here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import object_tracks_ref as otr  # noqa: E402
import track_visibility_ref as tvr  # noqa: E402
from test_capi_track_visibility import _call, invalid_cases  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4            # guard rows of a record buffer, on either side
PAD = 48             # guard bytes of the per-point output, on either side (+ the offset from the 16-byte boundary)
INVALID, CAPACITY, STATE = -1, -4, -5
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
F = np.float32
ALL = ("track_votes", "object_votes", "verdict")


@pytest.fixture(scope="module")
def ctx(scvod):
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=4096, max_scans=2)
    yield c
    c.close()


def _dev(a):
    """a host array as device bytes behind a 256-byte aligned pointer; an empty one becomes 64 unused bytes, so that its pointer is real"""
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(64, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else None


def link(scvod, ctx, scans, next_scan=None, poses=None, **trk):
    """the crafted scans as a table, linked on the device: a dict of host arrays"""
    import torch
    objects, offsets, cb, cand = otr.build_table(scans, next_scan)
    n, n_scans = len(objects), len(offsets) - 1
    d_obj, d_off = _dev(objects), _dev(offsets).view(torch.int32)
    d_cb, d_cand = _dev(cb).view(torch.int32), (_dev(cand).view(torch.int32) if len(cand) else None)
    out = ctx.object_tracks_device(d_obj, d_off, n_scans, next_scan, poses, d_cb, d_cand, scvod.track_params_default(**trk), n, n)
    ctx.object_tracks_stats()
    T = np.stack([scvod.pose_matrix(poses[s] if poses is not None else np.zeros(6, np.float32)) for s in range(n_scans)]) \
        if n_scans else np.zeros((0, 12), np.float32)
    n_tracks = int(out["n_tracks"].cpu().numpy().reshape(-1).view(np.int32)[0])
    assert 0 <= n_tracks <= n
    return dict(objects=objects, offsets=offsets, n_scans=n_scans, poses=poses, T=T, n_tracks=n_tracks,
                links=out["links"].cpu().numpy().reshape(-1).view(otr.LINK_DTYPE).copy(),
                tracks=out["tracks"].cpu().numpy().reshape(-1).view(otr.TRACK_DTYPE)[:n_tracks].copy(),
                tobj=out["track_objects"].cpu().numpy().reshape(-1).view(np.int32).copy())


def run(scvod, ctx, tab, po="rand", vin="rand", n_points=200, vis=None, in_off=0, out_off=0, in_place=False, want=ALL, cap_objects=None,
        cap_tracks=None, cap_track_votes=None, cap_object_votes=None, stream=None, seed=0, **prm):
    """one device call on linked tables, compared with the helper byte for byte; returns the helper's result.  po: "rand" (seeded entries
    in [-1, objects)), an int32 array, or None (records only); vin: "rand" (any bytes), a uint8 array, or None (NULL d_verdict)"""
    import torch
    objects, n = tab["objects"], len(tab["objects"])
    rng = np.random.default_rng(seed)
    if isinstance(po, str):
        po = rng.integers(-1, max(n, 1), n_points).astype(np.int32) if n else np.full(n_points, -1, np.int32)
    if po is not None:
        n_points = len(po)
    if isinstance(vin, str):
        vin = rng.integers(0, 256, n_points).astype(np.uint8)
    paint = po is not None and "verdict" in want
    cap_o = n if cap_objects is None else cap_objects
    cap_t = len(tab["tracks"]) if cap_tracks is None else cap_tracks
    cap_tv = cap_t if cap_track_votes is None else cap_track_votes
    cap_ov = cap_o if cap_object_votes is None else cap_object_votes
    # inputs
    d_obj, d_off, d_links, d_tracks = _dev(objects), _dev(tab["offsets"]), _dev(tab["links"]), _dev(tab["tracks"])
    d_tobj, d_ntr = _dev(tab["tobj"]), _dev(np.asarray([tab["n_tracks"]], np.int32))
    d_vis = _dev(vis) if vis is not None else None
    d_po = _dev(po) if po is not None else None
    d_in = None
    if vin is not None:
        d_in = torch.full((n_points + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        d_in[in_off:in_off + n_points] = torch.from_numpy(vin).cuda()
    # outputs between their guards
    rec = {"track_votes": (cap_tv, 32), "object_votes": (cap_ov, 16)}
    d_rec = {w: torch.full((rec[w][0] + 2 * GUARD, rec[w][1]), 0xA5, dtype=torch.uint8, device="cuda") for w in rec if w in want}
    d_out, o0 = None, PAD + out_off
    if paint and not in_place:
        d_out = torch.full((n_points + 2 * PAD + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    params = scvod.track_visibility_params_default(**prm)
    torch.cuda.synchronize()
    p_in = _ptr(d_in, in_off)
    p_out = None if not paint else (p_in if in_place else _ptr(d_out, o0))
    rc = ctx.lib.scvod_track_visibility_device(
        ctx.h, _ptr(d_obj), _ptr(d_off), tab["n_scans"], None if tab["poses"] is None else tab["poses"].ctypes.data_as(C.c_void_p),
        _ptr(d_links), cap_o, _ptr(d_tracks), cap_t, _ptr(d_tobj), _ptr(d_ntr), _ptr(d_vis), _ptr(d_po), p_in, p_out, n_points,
        C.byref(params), _ptr(d_rec.get("track_votes"), 32 * GUARD), cap_tv, _ptr(d_rec.get("object_votes"), 16 * GUARD), cap_ov,
        C.c_void_p(stream.cuda_stream if stream is not None else 0))
    assert rc == 0, ctx.lib.scvod_last_error(ctx.h)
    st = np.zeros(8, np.int64)
    rc = ctx.lib.scvod_track_visibility_stats(ctx.h, st.ctypes.data_as(C.c_void_p))
    ref = tvr.track_visibility_ref(objects, tab["offsets"], tab["T"], tab["links"], tab["tracks"][:cap_t], tab["tobj"], tab["n_tracks"],
                                   dict(tvr.DEFAULTS, **prm), object_vis=vis, point_object=po, verdict=vin, n_points=n_points, paint=paint,
                                   cap_objects=cap_o, cap_tracks=cap_t, cap_track_votes=cap_tv, cap_object_votes=cap_ov,
                                   want_track_votes="track_votes" in want, want_object_votes="object_votes" in want)
    assert dict(zip(tvr.STATS, st.tolist())) == ref["stats"]
    assert rc == (CAPACITY if ref["stats"]["latch"] & 3 else 0)
    for w in d_rec:
        got = d_rec[w].cpu().numpy()
        exp = ref[w].view(np.uint8).reshape(-1, rec[w][1])
        assert (got[:GUARD] == 0xA5).all(), f"{w}: something was written in front of the first record"
        assert np.array_equal(got[GUARD:GUARD + len(exp)], exp), f"{w} differ from the helper"
        assert (got[GUARD + len(exp):] == 0xA5).all(), f"{w}: something was written behind the last record"
    if paint:
        if in_place:
            got = d_in.cpu().numpy()
            exp = vin if ref["verdict"] is None else ref["verdict"]
            assert np.array_equal(got[in_off:in_off + n_points], exp), "the bytes rewritten in place differ from the helper"
            assert (got[:in_off] == 0x5A).all() and (got[in_off + n_points:] == 0x5A).all(), "in place: a byte outside the points changed"
        else:
            got = d_out.cpu().numpy()
            exp = np.full(n_points, 0xA5, np.uint8) if ref["verdict"] is None else ref["verdict"]
            assert np.array_equal(got[o0:o0 + n_points], exp), "verdict bytes differ from the helper"
            assert (got[:o0] == 0xA5).all() and (got[o0 + n_points:] == 0xA5).all(), "a byte outside the points was written"
            if d_in is not None:
                assert np.array_equal(d_in.cpu().numpy()[in_off:in_off + n_points], vin), "the input bytes changed"
    return ref


def vis_records(n, seed):
    """records of the objects' vote with every kind of verdict"""
    v = np.zeros(n, tvr.OBJECT_VIS_DTYPE)
    v["verdict"] = np.random.default_rng(900 + seed).choice([-1, 1, 2, 2], n)
    v["how"] = (v["verdict"] >= 0).astype(np.int32)
    return v


def lanes(n_scans, speed=0.7):
    """per scan: a mover (dynamic on odd scans), a parked car with one stray flag, and on every fifth scan a loner nothing links to"""
    return [[dict(center=(speed * s, 0.0, 0.0), dynamic=s % 2), dict(center=(0.001 * (s % 3), 10.0, 0.0), dynamic=int(s == 1))] +
            ([dict(center=(0.0, 40.0 + 5.0 * s, 0.0), dynamic=1)] if s % 5 == 0 else []) for s in range(n_scans)]


@pytest.fixture(scope="module")
def mixed(scvod, ctx):
    """the table most tests paint with: 9 scans, a mover, a parked car, a car that parks for four scans and then drives, loners"""
    scans = lanes(9)
    for s in range(9):
        scans[s].append(dict(center=(1.2 * max(s - 4, 0), 20.0, 0.0), dynamic=int(s in (5, 7))))
    tab = link(scvod, ctx, scans)
    assert tab["n_tracks"] == 3 and list(tab["tracks"]["length"]) == [9, 9, 9] and (tab["links"]["track"] == -1).sum() == 2
    return tab


# ---- 1. track lengths: the rounds of the wave walk ----
@pytest.mark.parametrize("length", [1, 2, 63, 64, 65, 129, 1025])
def test_track_lengths(scvod, ctx, length):
    tab = link(scvod, ctx, lanes(length), min_length=1)
    assert tab["n_tracks"] >= 2 and max(tab["tracks"]["length"]) == length == tab["tracks"]["length"][0]
    vis = vis_records(len(tab["objects"]), length)
    ref = run(scvod, ctx, tab, min_length=1, min_travel=1.0)
    assert ref["stats"]["members_motion"] == (length if length > 2 else 0)
    run(scvod, ctx, tab, vis=vis, min_length=1, min_travel=1e4, flags=tvr.CLEAR)          # nothing moves: vote or clear
    # one flag in the last member alone, counted at the end of the last round
    last = np.zeros(len(tab["objects"]), tvr.OBJECT_VIS_DTYPE)
    last["verdict"][int(tab["tracks"]["last_object"][0])] = 2
    ref = run(scvod, ctx, tab, vis=last, flags=tvr.NO_DYNAMIC, min_length=1, min_travel=1e4, min_flagged=1, vote_num=0)
    assert ref["track_votes"]["n_flagged"][0] == 1 and ref["track_votes"]["how"][0] == 1 and ref["stats"]["tracks_voted"] == 1


def test_two_tracks_interleaved_over_the_scans(scvod, ctx):
    nxt = [s + 2 if s + 2 < 11 else -1 for s in range(11)]
    tab = link(scvod, ctx, lanes(11, speed=0.4), nxt)
    assert tab["n_tracks"] == 4 and sorted(tab["tracks"]["length"]) == [5, 5, 6, 6]
    ref = run(scvod, ctx, tab, min_travel=1.5)
    assert ref["stats"]["members_motion"] == 11 and ref["stats"]["latch"] == 0
    run(scvod, ctx, tab, window=1, min_travel=0.7, flags=tvr.CLEAR, vis=vis_records(len(tab["objects"]), 3))


# ---- 2. the window: local motion, the rank clamped at both ends ----
@pytest.mark.parametrize("length", [65, 129])
@pytest.mark.parametrize("window", [0, 1, 3, 64, "L+5"])
def test_windows(scvod, ctx, length, window):
    w = length + 5 if window == "L+5" else window
    # parked for a third of the track, then 0.5 m a scan: the thresholds fall inside the track for every window
    scans = [[dict(center=(0.5 * max(s - length // 3, 0), 0.0, 0.0), dynamic=int(s % 7 == 0))] for s in range(length)]
    tab = link(scvod, ctx, scans)
    assert tab["n_tracks"] == 1
    ref = run(scvod, ctx, tab, window=w, min_travel=0.75, flags=tvr.CLEAR, min_flagged=50)
    how = list(ref["object_votes"]["how"])
    if window == 1:          # at the last rank the look-ahead is clamped: one step of 0.5 m is below 0.75, the two steps before it above
        assert (how[0], how[-2], how[-1]) == (3, 2, 3) and ref["object_votes"]["travel2"][-1] == F(0.25)
    elif window == 3:
        assert (how[0], how[-1]) == (3, 2) and 0 < ref["stats"]["members_motion"] < length
    else:
        assert how == [2] * length


# ---- 3. thresholds at equality and one ulp beside; NaN and infinite centres; poses ----
def test_thresholds(scvod, ctx):
    tab = link(scvod, ctx, [[dict(center=(0, 0, 0), cand=[(0, 9)])], [dict(center=(3, 4, 0))]])
    assert tab["n_tracks"] == 1
    assert list(run(scvod, ctx, tab, min_travel=5.0)["object_votes"]["how"]) == [2, 2]
    up, down = float(np.nextafter(F(5), F(9))), float(np.nextafter(F(5), F(0)))
    assert list(run(scvod, ctx, tab, min_travel=up)["object_votes"]["how"]) == [0, 0]
    assert list(run(scvod, ctx, tab, min_travel=down)["object_votes"]["how"]) == [2, 2]
    assert list(run(scvod, ctx, tab, min_travel=5.0, min_moved=3)["object_votes"]["how"]) == [0, 0]
    assert list(run(scvod, ctx, tab, min_travel=5.0, min_moved=2)["object_votes"]["how"]) == [2, 2]
    # the vote: 2 of 6 against 1 / 3 passes at equality, 2 / 5 does not; the largest legal numerator and denominator
    still = link(scvod, ctx, [[dict(center=(0.1 * s, 0, 0), dynamic=int(s in (0, 3)))] for s in range(6)])
    assert list(run(scvod, ctx, still, vote_num=1, vote_den=3)["object_votes"]["how"]) == [1] * 6
    assert list(run(scvod, ctx, still, vote_num=2, vote_den=5)["object_votes"]["how"]) == [0] * 6
    assert list(run(scvod, ctx, still, vote_num=1 << 18, vote_den=3 << 18)["object_votes"]["how"]) == [1] * 6
    assert list(run(scvod, ctx, still, vote_num=1 << 20, vote_den=1 << 20)["object_votes"]["how"]) == [0] * 6
    assert list(run(scvod, ctx, still, vote_num=0, min_flagged=2)["object_votes"]["how"]) == [1] * 6
    assert list(run(scvod, ctx, still, vote_num=0, min_flagged=3, flags=tvr.CLEAR)["object_votes"]["how"]) == [3] * 6
    assert list(run(scvod, ctx, still, vote_num=0, min_flagged=-5, flags=tvr.NO_DYNAMIC)["object_votes"]["how"]) == [1] * 6


def test_nan_and_infinite_centres(scvod, ctx):
    nan, inf = float("nan"), float("inf")
    for c, how in (((nan, 0, 0), 0), ((inf, 0, 0), 0), ((inf, inf, inf), 0), ((3e38, 0, 0), 2)):
        tab = link(scvod, ctx, [[dict(center=(-3e38 if how else 0, 0, 0), cand=[(0, 9)])], [dict(center=c, cand=[(0, 9)])], [dict(center=c)]])
        assert tab["n_tracks"] == 1 and tab["tracks"]["length"][0] == 3
        ref = run(scvod, ctx, tab)
        assert list(ref["object_votes"]["how"]) == [how] * 3
        ref = run(scvod, ctx, tab, window=1)      # rank 1 sees (0, 2): NaN or inf; the ends see one finite and one not
        assert ref["track_votes"]["max_travel2"][0] == (F(inf) if how else 0)


def test_poses(scvod, ctx):
    """a parked car seen from a sensor that drives and turns: still in the world, moving in the sensor frame -- and the reverse"""
    n = 7
    poses = np.zeros((n, 6), np.float32)
    poses[:, 0], poses[:, 1], poses[:, 5] = 1.5 * np.arange(n), 0.25 * np.arange(n), 0.2 * np.arange(n)

    def to_sensor(s, w):
        T = scvod.pose_matrix(poses[s]).astype(np.float64).reshape(3, 4)
        return tuple(float(v) for v in T[:, :3].T @ (np.asarray(w, np.float64) - T[:, 3]))
    scans = [[dict(center=to_sensor(s, (20.0, 3.0, 0.0)), cand=[(0, 9)]), dict(center=(8.0, -4.0, 0.0), cand=[(1, 9)])] for s in range(n)]
    tab = link(scvod, ctx, scans, poses=poses)
    assert tab["n_tracks"] == 2
    ref = run(scvod, ctx, tab, flags=tvr.CLEAR)
    assert list(ref["track_votes"]["how"]) == [3, 3] and list(ref["track_votes"]["n_moved"]) == [0, 7]
    assert sorted(ref["object_votes"]["how"]) == [2] * 7 + [3] * 7
    flat = dict(tab, poses=None, T=otr.identity_matrices(n))                # without the poses it is the other way round
    assert list(run(scvod, ctx, flat, flags=tvr.CLEAR)["track_votes"]["n_moved"]) == [7, 0]


# ---- 4. the cues and the switches ----
def test_cues_and_switches(scvod, ctx, mixed):
    n = len(mixed["objects"])
    vis, all_seen = vis_records(n, 1), vis_records(n, 1)
    all_seen["verdict"] = 2
    seen = set()
    for flags in (0, tvr.NO_DYNAMIC, tvr.CLEAR, tvr.NO_DYNAMIC | tvr.CLEAR):
        for v in (None, vis, all_seen):
            for w in (0, 2):
                ref = run(scvod, ctx, mixed, vis=v, flags=flags, window=w, seed=flags)
                seen |= set(int(h) for h in ref["object_votes"]["how"])
                assert (ref["object_votes"]["track"] == mixed["links"]["track"]).all()
    assert seen == {0, 1, 2, 3}
    ref = run(scvod, ctx, mixed, flags=tvr.CLEAR, min_length=10)              # min_length above every track: nothing is said
    assert (ref["object_votes"]["verdict"] == -1).all() and ref["stats"]["to_keep"] == 0 and (ref["track_votes"]["how"] == 0).all()
    assert (ref["object_votes"]["track"] == mixed["links"]["track"]).all()
    ref = run(scvod, ctx, mixed, flags=tvr.CLEAR, window=2)                   # the loners are on no listed track
    loners = np.nonzero(mixed["links"]["track"] == -1)[0]
    assert len(loners) == 2 and (ref["object_votes"]["verdict"][loners] == -1).all() and (ref["object_votes"]["verdict"] >= 0).sum() == n - 2


# ---- 5. the paint: sizes, addresses, in place, no input, any bytes, broken entries ----
@pytest.mark.parametrize("n_points", [0, 1, 3, 15, 16, 17, 63, 64, 65, 1023, 1025, 4097])
def test_paint_sizes(scvod, ctx, mixed, n_points):
    run(scvod, ctx, mixed, n_points=n_points, flags=tvr.CLEAR, window=2, seed=n_points)
    run(scvod, ctx, mixed, n_points=n_points, flags=tvr.CLEAR, window=2, seed=n_points, in_off=5, out_off=3)
    run(scvod, ctx, mixed, n_points=n_points, flags=tvr.CLEAR, window=2, seed=n_points, in_off=1, in_place=True)


@pytest.mark.parametrize("in_off", [0, 1, 3, 5, 15])
@pytest.mark.parametrize("out_off", [0, 1, 3, 5, 15])
def test_paint_addresses(scvod, ctx, mixed, in_off, out_off):
    for n_points in (14, 100, 1100):        # less than a head, a few lanes, more than a wave's 1024
        run(scvod, ctx, mixed, n_points=n_points, flags=tvr.CLEAR, window=2, in_off=in_off, out_off=out_off, seed=in_off * 16 + out_off)
    run(scvod, ctx, mixed, n_points=1100, flags=tvr.CLEAR, window=2, in_off=in_off, in_place=True, seed=in_off)
    run(scvod, ctx, mixed, n_points=1100, flags=tvr.CLEAR, window=2, vin=None, out_off=out_off, seed=out_off)        # NULL d_verdict


def test_paint_broken_entries(scvod, ctx, mixed):
    n = len(mixed["objects"])
    po = np.random.default_rng(5).integers(-1, n, 300).astype(np.int32)
    ref = run(scvod, ctx, mixed, po=po, flags=tvr.CLEAR)
    assert ref["stats"]["latch"] == 0
    for k, v in ((0, -1), (7, n - 1), (16, n), (40, INT_MAX), (299, INT_MIN), (150, -2)):
        po[k] = v
    vin = np.arange(300, dtype=np.uint8)
    ref = run(scvod, ctx, mixed, po=po, vin=vin, flags=tvr.CLEAR, out_off=1)
    assert ref["stats"]["latch"] == tvr.L_POINT and all(ref["verdict"][k] == vin[k] for k in (0, 16, 40, 299, 150))
    for only in ((16, n), (299, INT_MIN)):                                 # one broken entry alone, in the body and in the tail
        q = np.where((po >= 0) & (po < n), po, -1).astype(np.int32)
        q[only[0]] = only[1]
        assert run(scvod, ctx, mixed, po=q, vin=vin, flags=tvr.CLEAR)["stats"]["latch"] == tvr.L_POINT


# ---- 6. the latches ----
def test_upstream_overflow(scvod, ctx, mixed):
    n, nt = len(mixed["objects"]), mixed["n_tracks"]
    for kw in (dict(tab=dict(mixed, n_tracks=-1)), dict(tab=mixed, cap_objects=n - 1), dict(tab=mixed, cap_tracks=nt - 1),
               dict(tab=dict(mixed, offsets=np.where(np.arange(10) == 9, -3, mixed["offsets"]).astype(np.int32)))):
        tab = kw.pop("tab")
        for extra in (dict(), dict(in_place=True, in_off=3), dict(vin=None, out_off=5)):
            ref = run(scvod, ctx, tab, flags=tvr.CLEAR, n_points=333, **kw, **extra)
            assert ref["stats"]["latch"] == tvr.L_UPSTREAM and len(ref["object_votes"]) == 0 and len(ref["track_votes"]) == 0
            assert list(ref["stats"].values())[2:7] == [0] * 5


def test_record_overflow(scvod, ctx, mixed):
    n, nt = len(mixed["objects"]), mixed["n_tracks"]
    full = run(scvod, ctx, mixed, flags=tvr.CLEAR)
    for kw in (dict(cap_object_votes=n - 1), dict(cap_object_votes=0), dict(cap_track_votes=nt - 1), dict(cap_track_votes=0),
               dict(cap_track_votes=0, cap_object_votes=0)):
        for extra in (dict(), dict(in_place=True, in_off=1)):
            ref = run(scvod, ctx, mixed, flags=tvr.CLEAR, **kw, **extra)
            assert ref["stats"]["latch"] == tvr.L_RECORDS and ref["verdict"] is None
            assert ref["stats"]["members_cleared"] == full["stats"]["members_cleared"] and ref["stats"]["to_keep"] == 0
    # a buffer that is not asked for cannot overflow
    assert run(scvod, ctx, mixed, flags=tvr.CLEAR, cap_track_votes=0, want=("object_votes", "verdict"))["stats"]["latch"] == 0
    assert run(scvod, ctx, mixed, flags=tvr.CLEAR, cap_object_votes=0, want=("track_votes", "verdict"))["stats"]["latch"] == 0


def test_broken_references(scvod, ctx, mixed):
    n = len(mixed["objects"])
    po = np.arange(-1, n + 1, dtype=np.int32).repeat(3)[:-3]          # every object three times, and -1
    good = run(scvod, ctx, mixed, po=po, flags=tvr.CLEAR)
    assert good["stats"]["latch"] == 0

    def damaged(name, index, field, value):
        a = mixed[name].copy()
        if field is None:
            a[index] = value
        else:
            a[field][index] = value
        return dict(mixed, **{name: a})
    t1 = int(mixed["tracks"]["object_begin"][1])
    for value in (n - 8, -1, INT_MAX, INT_MIN):                        # a run that leaves the table: the track is refused, the others stand
        ref = run(scvod, ctx, damaged("tracks", 1, "object_begin", value), po=po, flags=tvr.CLEAR)
        assert ref["stats"]["latch"] == tvr.L_BROKEN and ref["track_votes"]["verdict"][1] == -1 and (ref["track_votes"]["verdict"][[0, 2]] >= 0).all()
        assert (ref["object_votes"]["track"][mixed["links"]["track"] == 1] == -1).all()
    ref = run(scvod, ctx, damaged("tracks", 2, "length", n), po=po, flags=tvr.CLEAR)
    assert ref["stats"]["latch"] == tvr.L_BROKEN and ref["track_votes"]["length"][2] == n
    for value in (n, -1, INT_MAX, INT_MIN):                            # a list entry outside the table, in the middle and at the end of a run
        for k in (t1 + 4, t1 + 8, t1):
            ref = run(scvod, ctx, damaged("tobj", k, None, value), po=po, flags=tvr.CLEAR, window=2)
            assert ref["stats"]["latch"] == tvr.L_BROKEN and ref["track_votes"]["how"][1] == 0
    for field, value in (("track", 3), ("track", -2), ("track", INT_MAX), ("track", INT_MIN), ("rank", 9), ("rank", -1), ("rank", INT_MAX)):
        ref = run(scvod, ctx, damaged("links", 4, field, value), po=po, flags=tvr.CLEAR, window=2)
        assert ref["stats"]["latch"] == tvr.L_BROKEN and ref["object_votes"]["verdict"][4] == -1 and ref["object_votes"]["track"][4] == -1
        assert (ref["object_votes"]["verdict"][[0, 7, 11]] >= 0).all()        # the members around it keep their verdicts


# ---- 7. records only, paint only, empty tables ----
def test_records_only_and_paint_only(scvod, ctx, mixed):
    full = run(scvod, ctx, mixed, flags=tvr.CLEAR, window=2)
    ref = run(scvod, ctx, mixed, po=None, flags=tvr.CLEAR, window=2)                              # no d_point_object
    assert ref["verdict"] is None and ref["object_votes"].tobytes() == full["object_votes"].tobytes() and ref["stats"]["to_keep"] == 0
    ref = run(scvod, ctx, mixed, flags=tvr.CLEAR, window=2, want=("track_votes", "object_votes"))  # d_point_object, no d_verdict_out
    assert ref["verdict"] is None and ref["stats"]["to_seen_through"] == 0
    ref = run(scvod, ctx, mixed, flags=tvr.CLEAR, window=2, want=("verdict",))                     # paint only
    assert np.array_equal(ref["verdict"], full["verdict"]) and ref["stats"] == full["stats"]
    run(scvod, ctx, mixed, flags=tvr.CLEAR, want=("track_votes",), po=None)
    run(scvod, ctx, mixed, flags=tvr.CLEAR, want=(), po=None)
    for scans in ([], [[], [], []], [[dict()], []]):                                               # no scan, no object, no track
        tab = link(scvod, ctx, scans)
        ref = run(scvod, ctx, tab, n_points=50, flags=tvr.CLEAR)
        assert ref["stats"]["tracks"] == 0 and ref["stats"]["latch"] == 0 and ref["stats"]["to_keep"] == 0


# ---- 8. the same ctx twice with different sizes, a side stream, the stats before the first call ----
def test_scratch_growth_and_a_side_stream(scvod):
    import torch
    ctx = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=4096, max_scans=2)
    small = link(scvod, ctx, lanes(3))
    big = link(scvod, ctx, lanes(300))
    a = run(scvod, ctx, small, flags=tvr.CLEAR)
    before = ctx.track_visibility_scratch_bytes()
    b = run(scvod, ctx, big, flags=tvr.CLEAR, n_points=3000)
    assert ctx.track_visibility_scratch_bytes() > before > 0
    assert run(scvod, ctx, small, flags=tvr.CLEAR)["object_votes"].tobytes() == a["object_votes"].tobytes()
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    c = run(scvod, ctx, big, flags=tvr.CLEAR, n_points=3000, stream=side)
    assert c["verdict"].tobytes() == b["verdict"].tobytes()
    ctx.close()


def test_python_entry_and_state(scvod, mixed):
    import torch
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=4096, max_scans=2)
    st = np.zeros(8, np.int64)
    assert c.lib.scvod_track_visibility_stats(c.h, st.ctypes.data_as(C.c_void_p)) == STATE
    assert c.track_visibility_scratch_bytes() == 0
    n = len(mixed["objects"])
    d_obj, d_off = _dev(mixed["objects"]), _dev(mixed["offsets"]).view(torch.int32)
    trk = c.object_tracks_device(d_obj, d_off, 9)
    po = np.random.default_rng(1).integers(-1, n, 500).astype(np.int32)
    vin = np.random.default_rng(2).integers(0, 3, 500).astype(np.uint8)
    d_po, d_in = _dev(po).view(torch.int32), _dev(vin)
    prm = scvod.track_visibility_params_default(flags=tvr.CLEAR, window=2)
    ref = tvr.track_visibility_ref(mixed["objects"], mixed["offsets"], mixed["T"], mixed["links"], mixed["tracks"], mixed["tobj"], mixed["n_tracks"],
                                   dict(tvr.DEFAULTS, flags=tvr.CLEAR, window=2), point_object=po, verdict=vin, cap_tracks=n)
    out, whole = c.track_visibility(d_obj, d_off, 9, None, trk, d_po, d_in, params=prm, guard=GUARD, full=True)
    assert c.track_visibility_stats() == ref["stats"]
    assert np.array_equal(out["verdict"].cpu().numpy(), ref["verdict"]) and (whole["verdict"].cpu().numpy()[:16 * GUARD] == 0xA5).all()
    assert out["object_votes"].cpu().numpy().tobytes() == ref["object_votes"].tobytes()
    tv = out["track_votes"].cpu().numpy()
    assert tv[:3].tobytes() == ref["track_votes"].tobytes() and (tv[3:] == 0xA5).all()
    out2 = c.track_visibility(d_obj, d_off, 9, None, trk, d_po, d_in, params=prm, in_place=True, want=("verdict",))
    assert out2["verdict"].data_ptr() == d_in.data_ptr() and np.array_equal(d_in.cpu().numpy(), ref["verdict"])
    assert set(c.track_visibility(d_obj, d_off, 9, None, trk, None, None, params=prm)) == {"track_votes", "object_votes"}
    c.close()


# ---- the argument errors on a live ctx, with host pointers: refused before anything is launched ----
def test_argument_errors_on_a_live_ctx(scvod, ctx):
    buf = np.zeros(4096, np.int64)                          # host memory: no call below may get as far as reading it
    for what, kw in invalid_cases(scvod, buf):
        assert _call(ctx.lib, ctx.h, buf, **kw) == INVALID, what
    assert b"" != ctx.lib.scvod_last_error(ctx.h)
