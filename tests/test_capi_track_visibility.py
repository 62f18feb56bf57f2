"""The tracks' vote on the seen-through verdict (scvod_track_visibility_device) without a GPU: the symbols, the three structs and the
defaults, the argument errors, the numpy statement of the rule (tests/helpers/track_visibility_ref.py) against cases worked out by hand
and against a brute-force restatement that recomputes everything per point and shares no code with it.  A ctx cannot be created
without a device, so the refusals are made on a NULL ctx here -- which is itself the first of them -- and once more on a live ctx, with
NULL device pointers, in tests/test_gpu_track_visibility_crafted.py.  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import object_tracks_ref as otr  # noqa: E402
import track_visibility_ref as tvr  # noqa: E402

NEW = ("scvod_track_visibility_params_default", "scvod_track_visibility_device", "scvod_track_visibility_stats",
       "scvod_track_visibility_scratch_bytes")
INVALID = -1
F = np.float32


def test_symbols_declared_exported_and_listed(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("track_visibility", "track_visibility_stats", "track_visibility_scratch_bytes"):
        assert callable(getattr(scvod.Ctx, m))
    assert callable(scvod.track_visibility_params_default)
    for name, value in (("NO_DYNAMIC", 1), ("CLEAR", 2)):
        assert re.search(rf"#define\s+SCVOD_TRKVIS_{name}\s+{value}\b", hdr) and getattr(scvod, "TRKVIS_" + name) == value
    assert (tvr.NO_DYNAMIC, tvr.CLEAR) == (scvod.TRKVIS_NO_DYNAMIC, scvod.TRKVIS_CLEAR)
    assert tuple(scvod.TRKVIS_STATS) == tvr.STATS and len(tvr.STATS) == 8
    assert scvod.TRKVIS_OUTPUTS == ("track_votes", "object_votes", "verdict")
    assert "NOT from real data" in hdr[hdr.index("the tracks of a batch vote on the seen-through verdict"):hdr.index("SCVOD_TRKVIS_NO_DYNAMIC")]


def test_struct_sizes_and_defaults(scvod):
    assert C.sizeof(scvod.TrackVisibilityParams) == 40
    assert scvod.TRACK_VOTE_DTYPE.itemsize == 32 and scvod.TRACK_VOTE_DTYPE == tvr.TRACK_VOTE_DTYPE
    assert scvod.OBJECT_TRACK_VOTE_DTYPE.itemsize == 16 and scvod.OBJECT_TRACK_VOTE_DTYPE == tvr.OBJECT_VOTE_DTYPE
    assert scvod.OBJECT_VISIBILITY_DTYPE == tvr.OBJECT_VIS_DTYPE
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    for name, size in (("scvod_track_visibility_params", 40), ("scvod_track_vote", 32), ("scvod_object_track_vote", 16)):
        assert re.search(rf"typedef struct {name} {{\s+/\* {size} bytes", hdr), name
    p = scvod.track_visibility_params_default()
    got = {k: getattr(p, k) for k in tvr.DEFAULTS}
    assert got == tvr.DEFAULTS == dict(flags=0, window=0, min_travel=2.0, min_length=2, min_moved=1, min_flagged=2, vote_num=1, vote_den=2)
    assert list(p.reserved) == [0, 0]
    scvod.load_lib().scvod_track_visibility_params_default(None)   # a NULL struct is ignored
    assert scvod.track_visibility_params_default(flags=3, window=4).window == 4
    assert (tvr.UNTESTED, tvr.KEEP, tvr.SEEN) == (0, 1, 2)
    for name, value in (("UNTESTED", 0), ("KEEP", 1), ("SEEN_THROUGH", 2)):
        assert re.search(rf"#define\s+SCVOD_VIS_{name}\s+{value}\b", hdr)


def _call(lib, ctx, buf, **kw):
    """scvod_track_visibility_device with every pointer at `buf` (host memory: no call may get as far as reading it) unless overridden"""
    p = C.c_void_p(buf.ctypes.data)
    a = dict(objects=p, offs=p, n_scans=2, links=p, cap=4, tracks=p, cap_t=4, tobj=p, ntr=p, ovis=None, po=None, vin=None, vout=None,
             n_points=0, prm=None, tv=None, cap_tv=4, ov=None, cap_ov=4)
    a.update(kw)
    return lib.scvod_track_visibility_device(ctx, a["objects"], a["offs"], a["n_scans"], None, a["links"], a["cap"], a["tracks"], a["cap_t"],
                                             a["tobj"], a["ntr"], a["ovis"], a["po"], a["vin"], a["vout"], a["n_points"],
                                             C.byref(a["prm"]) if a["prm"] is not None else None, a["tv"], a["cap_tv"], a["ov"], a["cap_ov"],
                                             None)


def invalid_cases(scvod, buf):
    """(what, keyword arguments of _call): every refusal the header lists, but the NULL ctx"""
    base = buf.ctypes.data
    p, odd = C.c_void_p(base), C.c_void_p(base + 2)

    def at(off):
        return C.c_void_p(base + off)
    bad_reserved = scvod.track_visibility_params_default()
    bad_reserved.reserved[1] = 1
    out = [("reserved", dict(prm=bad_reserved))]
    for kw in (dict(flags=4), dict(flags=-1), dict(window=-1), dict(min_travel=0.0), dict(min_travel=-1.0), dict(min_travel=float("inf")),
               dict(min_travel=float("nan")), dict(min_length=0), dict(min_moved=0), dict(vote_num=-1), dict(vote_num=(1 << 20) + 1),
               dict(vote_den=0), dict(vote_den=(1 << 20) + 1)):
        out.append((str(kw), dict(prm=scvod.track_visibility_params_default(**kw))))
    out += [(str(kw), kw) for kw in (dict(n_scans=-1), dict(cap=-1), dict(cap=1 << 31), dict(cap_t=-1), dict(cap_tv=-1), dict(cap_ov=-1),
                                     dict(n_points=-1), dict(offs=None), dict(links=None), dict(tracks=None), dict(tobj=None), dict(ntr=None),
                                     dict(objects=None), dict(vout=at(4096), n_points=16))]       # d_verdict_out without d_point_object
    out += [("misaligned " + k, {k: odd}) for k in ("objects", "offs", "links", "tracks", "tobj", "ntr", "ovis", "po", "tv", "ov")]
    out.append(("objects 4-byte aligned only", dict(objects=at(4))))
    # d_verdict_out [4096, 4096 + 64) against every input and record buffer, one byte of overlap at either end
    paint = dict(po=at(8192), vin=at(16384), vout=at(4096), n_points=64)
    assert _call(scvod.load_lib(), None, buf, **paint) == INVALID
    for k, size in (("vin", 64), ("po", 256), ("objects", 64 * 4), ("offs", 12), ("links", 32 * 4), ("tracks", 64 * 4), ("tobj", 16), ("ntr", 4),
                    ("ovis", 48 * 4), ("tv", 32 * 4), ("ov", 16 * 4)):
        lo = (4096 - size + 8) if k == "objects" else (4096 - size + 4 if k != "vin" else 4096 - size + 1)
        hi = 4096 + 56 if k == "objects" else (4096 + 60 if k != "vin" else 4096 + 63)
        for off in (lo, hi):
            out.append((f"overlap {k} at {off}", dict(paint, **{k: at(off)})))
    return out


def test_argument_errors_need_no_device(scvod):
    """SCVOD_ERR_INVALID with no device present: on a NULL ctx everything is; the single cases are told apart on a live ctx"""
    lib = scvod.load_lib()
    buf = np.zeros(4096, np.int64)
    assert _call(lib, None, buf) == INVALID
    assert _call(lib, None, buf, prm=scvod.track_visibility_params_default()) == INVALID
    for what, kw in invalid_cases(scvod, buf):
        assert _call(lib, None, buf, **kw) == INVALID, what
    assert lib.scvod_track_visibility_stats(None, C.c_void_p(buf.ctypes.data)) == INVALID
    assert lib.scvod_track_visibility_scratch_bytes(None) == 0


# ---- the helper against cases worked out by hand ----
def tables(scans, next_scan=None, **trk):
    """crafted scans -> (objects, offsets, the tracker's result)"""
    objects, offsets, cb, cand = otr.build_table(scans, next_scan)
    prm = dict(otr.DEFAULTS, occupancy=0.4, **trk)
    with np.errstate(all="ignore"):
        ref = otr.object_tracks_ref(objects, offsets, next_scan, otr.identity_matrices(len(offsets) - 1), cb, cand, prm)
    return objects, offsets, ref


def chain(centres, dynamic=None, **kw):
    """one car per scan, linked by an overlap candidate whatever the distance: one track"""
    dynamic = [0] * len(centres) if dynamic is None else dynamic
    return tables([[dict(center=c, dynamic=d, cand=[(0, 9)])] for c, d in zip(centres, dynamic)], **kw)


def run_ref(tab, vis=None, po=None, vin=None, **prm):
    objects, offsets, ref = tab
    return tvr.track_visibility_ref(objects, offsets, otr.identity_matrices(len(offsets) - 1), ref["links"], ref["tracks"],
                                    ref["track_objects"], ref["n_tracks"], dict(tvr.DEFAULTS, **prm), object_vis=vis, point_object=po,
                                    verdict=vin)


def test_travel_threshold_by_hand():
    tab = chain([(0, 0, 0), (3, 4, 0)])
    assert tab[2]["n_tracks"] == 1 and list(tab[2]["tracks"]["length"]) == [2]
    r = run_ref(tab, min_travel=5.0)                                          # 9 + 16 = 25 >= 5 * 5
    assert list(r["object_votes"]["verdict"]) == [2, 2] and list(r["object_votes"]["how"]) == [2, 2]
    assert list(r["object_votes"]["travel2"]) == [F(25), F(25)] and r["track_votes"]["n_moved"][0] == 2
    assert r["track_votes"]["max_travel2"][0] == F(25) and r["track_votes"]["verdict"][0] == -1 and r["track_votes"]["how"][0] == 0
    assert r["stats"]["members_motion"] == 2 and r["stats"]["tracks_voted"] == 0
    up = float(np.nextafter(F(5.0), F(np.inf)))
    assert F(up) * F(up) > F(25)
    r = run_ref(tab, min_travel=up)
    assert list(r["object_votes"]["verdict"]) == [-1, -1] and r["track_votes"]["n_moved"][0] == 0 and r["stats"]["members_motion"] == 0
    # min_moved above the track's length switches the whole-track motion off; it is not read with a window
    assert list(run_ref(tab, min_travel=5.0, min_moved=3)["object_votes"]["how"]) == [0, 0]
    assert list(run_ref(tab, min_travel=5.0, min_moved=3, window=1)["object_votes"]["how"]) == [2, 2]
    # a NaN never moves, an infinite displacement does
    nan, inf = float("nan"), float("inf")
    assert list(run_ref(chain([(0, 0, 0), (nan, 0, 0)]))["object_votes"]["how"]) == [0, 0]
    r = run_ref(chain([(-3e38, 0, 0), (3e38, 0, 0)]))                         # dx overflows: travel2 is inf
    assert list(r["object_votes"]["how"]) == [2, 2] and r["track_votes"]["max_travel2"][0] == F(inf)
    for c in ((inf, 0, 0), (inf, inf, inf)):                                  # an infinite centre: 0 * inf in cW, or inf - inf
        r = run_ref(chain([c, c]))
        assert list(r["object_votes"]["how"]) == [0, 0] and r["track_votes"]["max_travel2"][0] == 0
        assert np.isnan(r["object_votes"]["travel2"]).all()


def test_vote_at_equality_by_hand():
    still = [(0.1 * k, 0, 0) for k in range(6)]
    # 2 of 6 flagged against 1 / 3: 2 * 3 == 1 * 6 passes; 1 / 3 with one flag fewer, or 2 / 5 (10 < 12), does not
    tab = chain(still, [1, 0, 0, 1, 0, 0])
    r = run_ref(tab, vote_num=1, vote_den=3)
    assert list(r["object_votes"]["how"]) == [1] * 6 and list(r["object_votes"]["verdict"]) == [2] * 6
    assert (r["track_votes"]["n_flagged"][0], r["track_votes"]["verdict"][0], r["track_votes"]["how"][0]) == (2, 2, 1)
    assert r["stats"]["tracks_voted"] == 1
    assert list(run_ref(tab, vote_num=2, vote_den=5)["object_votes"]["how"]) == [0] * 6
    assert list(run_ref(chain(still, [1, 0, 0, 0, 0, 0]), vote_num=1, vote_den=3, min_flagged=1)["object_votes"]["how"]) == [0] * 6
    # min_flagged at equality and above; vote_num 0 leaves min_flagged alone to decide
    assert list(run_ref(tab, vote_num=0, min_flagged=2)["object_votes"]["how"]) == [1] * 6
    assert list(run_ref(tab, vote_num=0, min_flagged=3)["object_votes"]["how"]) == [0] * 6
    # the flags: NO_DYNAMIC silences the table's byte, the objects' vote flags on its own
    assert list(run_ref(tab, vote_num=1, vote_den=3, flags=tvr.NO_DYNAMIC)["object_votes"]["how"]) == [0] * 6
    vis = np.zeros(6, tvr.OBJECT_VIS_DTYPE)
    vis["verdict"] = [2, 1, -1, 2, 0, -1]
    r = run_ref(chain(still), vis=vis, vote_num=1, vote_den=3)
    assert list(r["object_votes"]["how"]) == [1] * 6 and r["track_votes"]["n_flagged"][0] == 2
    r = run_ref(tab, vis=vis, vote_num=1, vote_den=3, flags=tvr.NO_DYNAMIC)   # the union of both cues is counted once per object
    assert r["track_votes"]["n_flagged"][0] == 2


def test_window_clear_and_precedence_by_hand():
    # parked for four scans, then 3 m a scan
    xs = [0, 0, 0, 0, 3, 6, 9]
    tab = chain([(x, 0, 0) for x in xs])
    r = run_ref(tab, window=0)
    assert list(r["object_votes"]["how"]) == [2] * 7 and list(r["object_votes"]["travel2"]) == [F(81)] * 7
    r = run_ref(tab, window=1)                                  # |x[r + 1] - x[r - 1]| with the ranks clamped: 0 0 0 3 6 6 3
    assert list(r["object_votes"]["travel2"]) == [F(v * v) for v in (0, 0, 0, 3, 6, 6, 3)]
    assert list(r["object_votes"]["how"]) == [0, 0, 0, 2, 2, 2, 2] and r["track_votes"]["n_moved"][0] == 4
    assert r["track_votes"]["max_travel2"][0] == F(36)
    for w in (7, 12, 1 << 30, 2 ** 31 - 1):                          # a window larger than the track is the whole track
        r = run_ref(tab, window=w)
        assert list(r["object_votes"]["travel2"]) == [F(81)] * 7 and list(r["object_votes"]["how"]) == [2] * 7
    # the clear: a still track with one stray flag; without CLEAR it says nothing
    still = chain([(0.1 * k, 0, 0) for k in range(5)], [0, 1, 0, 0, 0])
    assert list(run_ref(still)["object_votes"]["verdict"]) == [-1] * 5
    r = run_ref(still, flags=tvr.CLEAR)
    assert list(r["object_votes"]["verdict"]) == [1] * 5 and list(r["object_votes"]["how"]) == [3] * 5
    assert (r["track_votes"]["verdict"][0], r["track_votes"]["how"][0]) == (1, 3) and r["stats"]["members_cleared"] == 5
    # precedence: motion over vote over clear.  With the window the parked phase takes the vote, or else the clear
    flags = [1, 1, 1, 1, 0, 0, 0]
    tabf = chain([(x, 0, 0) for x in xs], flags)
    r = run_ref(tabf, window=1, flags=tvr.CLEAR)
    assert list(r["object_votes"]["how"]) == [1, 1, 1, 2, 2, 2, 2] and list(r["object_votes"]["verdict"]) == [2] * 7
    r = run_ref(tabf, window=1, flags=tvr.CLEAR, min_flagged=5)
    assert list(r["object_votes"]["how"]) == [3, 3, 3, 2, 2, 2, 2] and list(r["object_votes"]["verdict"]) == [1, 1, 1, 2, 2, 2, 2]
    assert r["stats"]["members_motion"] == 4 and r["stats"]["members_cleared"] == 3 and r["stats"]["tracks_voted"] == 0
    # the points take their object's verdict; -1 and objects without one keep the input byte
    po = np.asarray([0, 0, -1, 3, 6, 6, -1, 2], np.int32)
    vin = np.asarray([2, 0, 2, 1, 2, 77, 200, 1], np.uint8)
    r = run_ref(tabf, window=1, flags=tvr.CLEAR, min_flagged=5, po=po, vin=vin)
    assert list(r["verdict"]) == [1, 1, 2, 2, 2, 2, 200, 1]
    assert r["stats"]["to_seen_through"] == 2 and r["stats"]["to_keep"] == 2 and r["stats"]["latch"] == 0
    r = run_ref(tabf, window=1, po=po, vin=None)
    assert list(r["verdict"]) == [2, 2, 0, 2, 2, 2, 0, 2]
    # min_length above the track, and an object on no listed track
    r = run_ref(tabf, min_length=8, po=po, vin=vin)
    assert list(r["object_votes"]["verdict"]) == [-1] * 7 and list(r["object_votes"]["track"]) == [0] * 7 and list(r["verdict"]) == list(vin)
    assert (r["track_votes"]["length"][0], r["track_votes"]["n_flagged"][0]) == (7, 0)
    lone = tables([[dict(center=(0, 0, 0), cand=[(0, 9)]), dict(center=(50, 0, 0), dynamic=1)], [dict(center=(5, 0, 0))]])
    r = run_ref(lone)
    assert list(r["object_votes"]["track"]) == [0, -1, 0] and list(r["object_votes"]["how"]) == [2, 0, 2]


def test_helper_latches_by_hand():
    tab = chain([(x, 0, 0) for x in (0, 1, 2, 3)], [1, 1, 0, 0])
    objects, offsets, ref = tab
    T = otr.identity_matrices(4)
    po = np.asarray([0, 1, 2, 3, -1, 4, 2 ** 31 - 1, -2 ** 31, -2], np.int32)
    vin = np.arange(9, dtype=np.uint8)
    prm = dict(tvr.DEFAULTS)

    def go(links=ref["links"], tracks=ref["tracks"], tobj=ref["track_objects"], n_tracks=1, offs=offsets, **kw):
        return tvr.track_visibility_ref(objects, offs, T, links, tracks, tobj, n_tracks, prm, point_object=po, verdict=vin, **kw)
    r = go()
    assert r["stats"]["latch"] == tvr.L_POINT and list(r["verdict"]) == [2, 2, 2, 2, 4, 5, 6, 7, 8] and r["stats"]["to_seen_through"] == 3
    for kw in (dict(n_tracks=-1), dict(cap_objects=3), dict(n_tracks=2)):
        r = go(**kw)
        assert r["stats"]["latch"] == tvr.L_UPSTREAM and list(r["verdict"]) == list(vin) and len(r["object_votes"]) == 0
        assert list(r["stats"].values())[2:7] == [0] * 5
    for kw in (dict(cap_object_votes=3), dict(cap_track_votes=0)):
        r = go(**kw)
        assert r["stats"]["latch"] == tvr.L_RECORDS and r["verdict"] is None and r["stats"]["members_motion"] == 4
    assert len(go(cap_object_votes=3)["object_votes"]) == 3 and go(cap_object_votes=3, want_object_votes=False)["stats"]["latch"] == tvr.L_POINT
    for field, value in (("object_begin", 1), ("object_begin", -1), ("length", 5)):
        tr = ref["tracks"].copy()
        tr[field][0] = value
        r = go(tracks=tr)
        assert r["stats"]["latch"] == tvr.L_BROKEN | tvr.L_POINT and list(r["verdict"]) == list(vin)
        assert list(r["object_votes"]["track"]) == [-1] * 4 and r["track_votes"]["verdict"][0] == -1
    for value in (4, -1, 2 ** 31 - 1):
        tobj = ref["track_objects"].copy()
        tobj[2] = value
        r = go(tobj=tobj)
        assert r["stats"]["latch"] == tvr.L_BROKEN | tvr.L_POINT and list(r["object_votes"]["verdict"]) == [-1] * 4
    for field, value in (("track", 1), ("track", -2), ("rank", 4), ("rank", -1)):
        lk = ref["links"].copy()
        lk[field][1] = value
        r = go(links=lk)
        assert r["stats"]["latch"] == tvr.L_BROKEN | tvr.L_POINT and list(r["object_votes"]["verdict"]) == [2, -1, 2, 2]
        assert list(r["object_votes"]["track"]) == [0, -1, 0, 0]


# ---- the helper against a brute-force restatement that recomputes everything per point ----
def brute_point(i, objects, offsets, T, links, tracks, tobj, n_tracks, prm, vis, po, vin):
    """the output byte of point i and the verdict of its object, from the tables alone: array arithmetic, nothing shared with the helper"""
    n = int(offsets[-1])
    o = int(po[i])
    if o < 0 or o >= n:
        return int(vin[i]), None
    t = int(links["track"][o])
    if t < 0:
        return int(vin[i]), -1
    L, ob = int(tracks["length"][t]), int(tracks["object_begin"][t])
    if L < prm["min_length"]:
        return int(vin[i]), -1
    mem = np.asarray(tobj[ob:ob + L], np.int64)
    M = T[objects["scan"][mem]]
    c = objects["center"][mem].astype(np.float32)
    cw = np.stack([((M[:, 4 * r] * c[:, 0] + M[:, 4 * r + 1] * c[:, 1]) + M[:, 4 * r + 2] * c[:, 2]) + M[:, 4 * r + 3] for r in range(3)], 1)
    rk = np.arange(L)
    w = prm["window"]
    ia = np.zeros(L, np.int64) if w == 0 else np.maximum(rk - w, 0)
    ib = np.full(L, L - 1) if w == 0 else np.minimum(rk + w, L - 1)
    d = cw[ib] - cw[ia]
    with np.errstate(all="ignore"):
        t2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        mv = t2 >= F(prm["min_travel"]) * F(prm["min_travel"])
    fl = np.zeros(L, bool) if prm["flags"] & tvr.NO_DYNAMIC else objects["dynamic"][mem] == 1
    if vis is not None:
        fl = fl | (vis["verdict"][mem] == 2)
    r = int(links["rank"][o])
    if mv[r] and (w > 0 or mv.sum() >= prm["min_moved"]):
        v = 2
    elif fl.sum() >= prm["min_flagged"] and int(fl.sum()) * prm["vote_den"] >= prm["vote_num"] * L:
        v = 2
    elif prm["flags"] & tvr.CLEAR:
        v = 1
    else:
        v = -1
    return (v if v >= 0 else int(vin[i])), v


def random_case(scvod, seed):
    rng = np.random.default_rng(4000 + seed)
    n_scans = int(rng.integers(2, 9))
    scans = [[] for _ in range(n_scans)]
    for k in range(int(rng.integers(1, 7))):                      # k-th object: lives over a run of scans, parked, driving or both
        s0 = int(rng.integers(0, n_scans - 1))
        s1 = int(rng.integers(s0 + 1, n_scans + 1))
        speed, go_from = float(rng.choice([0.0, 0.25, 1.0, 1.5])), int(rng.integers(s0, s1))
        x = 0.0
        for s in range(s0, s1):
            x += speed if s >= go_from else 0.0
            scans[s].append(dict(center=(x, 6.0 * k, 0.0), dynamic=int(rng.random() < 0.35)))
    objects, offsets, cb, cand = otr.build_table(scans)
    poses = np.zeros((n_scans, 6), np.float32)
    if seed % 2:
        poses[:, 0] = 0.5 * np.arange(n_scans)
        poses[:, 5] = rng.choice([0.0, 0.25, -1.0], n_scans)
    T = np.stack([scvod.pose_matrix(p) for p in poses])
    Tinv = [np.linalg.inv(np.vstack([t.reshape(3, 4).astype(np.float64), [0, 0, 0, 1]])) for t in T]
    for o in objects:                                             # the centres above are world-frame: into the sensor frame
        o["center"] = (Tinv[int(o["scan"])] @ np.append(o["center"].astype(np.float64), 1.0))[:3]
    ref = otr.object_tracks_ref(objects, offsets, None, T, cb, cand, dict(otr.DEFAULTS, occupancy=0.4, gate=2.0,
                                                                         min_length=int(rng.integers(1, 3))))
    n = len(objects)
    vis = None
    if seed % 3:
        vis = np.zeros(n, tvr.OBJECT_VIS_DTYPE)
        vis["verdict"] = rng.choice([-1, 1, 2, 2], n)
    po = rng.integers(-1, max(n, 1), int(rng.integers(0, 80))).astype(np.int32)
    vin = rng.integers(0, 256, len(po)).astype(np.uint8)
    prm = dict(tvr.DEFAULTS, flags=int(rng.integers(0, 4)), window=int(rng.choice([0, 0, 1, 2, 50])), min_travel=float(rng.choice([0.5, 2.0, 3.0])),
               min_length=int(rng.integers(1, 5)), min_moved=int(rng.choice([1, 1, 3])), min_flagged=int(rng.integers(0, 4)),
               vote_num=int(rng.integers(0, 4)), vote_den=int(rng.integers(1, 5)))
    return objects, offsets, T, ref, vis, po, vin, prm


def test_helper_against_brute_force_on_random_tables(scvod):
    seen = dict(motion=0, vote=0, clear=0, none=0, points=0)
    for seed in range(60):
        objects, offsets, T, ref, vis, po, vin, prm = random_case(scvod, seed)
        r = tvr.track_visibility_ref(objects, offsets, T, ref["links"], ref["tracks"], ref["track_objects"], ref["n_tracks"], prm,
                                     object_vis=vis, point_object=po, verdict=vin)
        assert r["stats"]["latch"] == 0
        for i in range(len(po)):
            byte, v = brute_point(i, objects, offsets, T, ref["links"], ref["tracks"], ref["track_objects"], ref["n_tracks"], prm, vis, po, vin)
            assert int(r["verdict"][i]) == byte, (seed, i)
            assert v is None or int(r["object_votes"]["verdict"][int(po[i])]) == v, (seed, i)
        moved = sum(1 for i in range(len(po)) if r["verdict"][i] != vin[i])
        assert r["stats"]["to_seen_through"] + r["stats"]["to_keep"] == moved
        assert r["stats"]["tracks"] == ref["n_tracks"] == len(r["track_votes"]) and r["stats"]["objects"] == len(objects)
        how = r["object_votes"]["how"]
        for k, h in (("motion", 2), ("vote", 1), ("clear", 3), ("none", 0)):
            seen[k] += int((how == h).sum())
        seen["points"] += moved
    assert min(seen.values()) > 20, seen   # the cases reach every part of the rule
