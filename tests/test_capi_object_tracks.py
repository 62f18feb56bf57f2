"""Object tracks (scvod_object_tracks_device / scvod_batch_object_tracks) without a GPU: the symbols, the three structs and the
defaults, the argument errors, scvod_tracks_finish against a numpy restatement, and the sequential numpy tracker
(tests/helpers/object_tracks_ref.py) against a brute-force restatement of the rule that shares no code with it.  A ctx cannot be created
without a device, so the refusals are made on a NULL ctx here -- which is itself the first of them -- and once more on a live ctx, with
NULL device pointers, in tests/test_gpu_object_tracks_crafted.py.  Not gpu."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import object_tracks_ref as otr  # noqa: E402

NEW = ("scvod_track_params_default", "scvod_object_tracks_device", "scvod_batch_object_tracks", "scvod_object_tracks_stats",
       "scvod_object_tracks_scratch_bytes", "scvod_tracks_finish")
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
    for m in ("object_tracks_device", "batch_object_tracks", "object_tracks_stats"):
        assert callable(getattr(scvod.Ctx, m))
    assert callable(scvod.track_params_default) and callable(scvod.tracks_finish)
    for name, value in (("NO_GATE", 1), ("ANY_CLASS", 2)):
        assert re.search(rf"#define\s+SCVOD_TRK_{name}\s+{value}\b", hdr) and getattr(scvod, "TRK_" + name) == value
    assert (otr.NO_GATE, otr.ANY_CLASS) == (scvod.TRK_NO_GATE, scvod.TRK_ANY_CLASS)
    assert tuple(scvod.TRK_STATS) == otr.STATS and len(otr.STATS) == 8
    assert "NOT from real data" in hdr[hdr.index("SCVOD_TRK_NO_GATE") - 4000:]


def test_struct_sizes_and_defaults(scvod):
    assert C.sizeof(scvod.TrackParams) == 32
    assert scvod.OBJECT_LINK_DTYPE.itemsize == 32 and scvod.OBJECT_LINK_DTYPE == otr.LINK_DTYPE
    assert scvod.TRACK_DTYPE.itemsize == 64 and scvod.TRACK_DTYPE == otr.TRACK_DTYPE
    assert scvod.OBJECT_DTYPE == otr.OBJECT_DTYPE
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    for name, size in (("scvod_track_params", 32), ("scvod_object_link", 32), ("scvod_track", 64)):
        assert re.search(rf"typedef struct {name} {{ /\* {size} bytes", hdr), name
    p = scvod.track_params_default()
    got = {k: getattr(p, k) for k in otr.DEFAULTS}
    assert got == otr.DEFAULTS == dict(flags=0, occupancy=-1.0, gate=2.0, size_ratio=1.5, min_points=10, min_length=2)
    assert list(p.reserved) == [0, 0]
    scvod.load_lib().scvod_track_params_default(None)   # a NULL struct is ignored
    assert scvod.track_params_default(flags=3, min_length=5).min_length == 5


def test_argument_errors_need_no_device(scvod):
    """SCVOD_ERR_INVALID with no device present"""
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = C.c_void_p(buf.ctypes.data)
    good = scvod.track_params_default()
    dev, bat = lib.scvod_object_tracks_device, lib.scvod_batch_object_tracks
    assert dev(None, p, p, 2, None, None, None, None, C.byref(good), p, 4, p, 4, p, p, None) == INVALID
    assert dev(None, p, p, 2, None, None, None, None, None, p, 4, p, 4, p, p, None) == INVALID       # no params either
    assert bat(None, p, None, C.byref(good), p, 4, p, 4, p, p, None) == INVALID
    bad_reserved = scvod.track_params_default()
    bad_reserved.reserved[1] = 1
    for bad in [scvod.track_params_default(**kw) for kw in (
            dict(flags=4), dict(flags=-1), dict(gate=0.0), dict(gate=-1.0), dict(gate=float("inf")), dict(gate=float("nan")),
            dict(size_ratio=0.99), dict(min_points=0), dict(min_length=0))] + [bad_reserved]:
        assert dev(None, p, p, 2, None, None, None, None, C.byref(bad), p, 4, p, 4, p, p, None) == INVALID
        assert bat(None, p, None, C.byref(bad), p, 4, p, 4, p, p, None) == INVALID
    assert dev(None, p, p, -1, None, None, None, None, C.byref(good), p, 4, p, 4, p, p, None) == INVALID     # n_scans < 0
    assert dev(None, p, p, 2, None, None, None, p, C.byref(good), p, 4, p, 4, p, p, None) == INVALID         # d_cand without d_cand_begin
    for nx in ([1, 1, -1], [1, 2, 0], [3, -1, -1], [0, -1, -1]):   # one successor twice, a ring, outside the batch, itself
        t = np.asarray(nx, np.int32)
        assert dev(None, p, p, 3, t.ctypes.data_as(C.c_void_p), None, None, None, C.byref(good), p, 4, p, 4, p, p, None) == INVALID
    odd = C.c_void_p(buf.ctypes.data + 2)
    assert dev(None, odd, p, 2, None, None, None, None, C.byref(good), p, 4, p, 4, p, p, None) == INVALID    # misaligned
    assert dev(None, p, p, 2, None, None, None, None, C.byref(good), odd, 4, p, 4, p, p, None) == INVALID
    assert lib.scvod_object_tracks_stats(None, p) == INVALID
    assert lib.scvod_object_tracks_scratch_bytes(None) == 0
    assert lib.scvod_tracks_finish(None, 1, 2.0, None) == INVALID


def test_next_table_of_the_helper_refuses_what_the_library_refuses(scvod):
    for nx, ok in (([1, 2, -1], True), ([2, 3, -1, -1], True), ([1, -1, -5], True), ([1, 1, -1], False), ([1, 2, 0], False),
                   ([3, -1, -1], False), ([0, -1, -1], False), (None, True)):
        t = None if nx is None else np.asarray(nx, np.int32)
        rc = scvod.load_lib().scvod_visibility_viewers(None if t is None else t.ctypes.data_as(C.c_void_p), 3 if nx is None else len(nx),
                                                       0, 1, None, None, 0)
        assert (rc >= 0) == ok == (otr.next_table(3 if nx is None else len(nx), nx) is not None), nx


# ---- scvod_tracks_finish ----
def finish_ref(tracks, min_travel):
    net = tracks["net"].astype(np.float64)
    d = np.sqrt(net[:, 0] * net[:, 0] + net[:, 1] * net[:, 1] + net[:, 2] * net[:, 2])
    mov = d >= min_travel
    ln, dy = tracks["length"].astype(np.int64), tracks["n_dynamic"].astype(np.int64)
    r = dict(tracks=len(tracks), moving_tracks=int(mov.sum()), moving_members=int(ln[mov].sum()), moving_members_dynamic=int(dy[mov].sum()),
             still_tracks=int((~mov).sum()), still_members=int(ln[~mov].sum()), still_members_dynamic=int(dy[~mov].sum()))
    along = r["moving_members"] - r["moving_tracks"]
    r["recall_along"] = 100.0 * r["moving_members_dynamic"] / along if along else float("nan")
    r["false_alarm"] = 100.0 * r["still_members_dynamic"] / r["still_members"] if r["still_members"] else float("nan")
    return r


def same_result(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] == b[k]) or (isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


def test_tracks_finish_against_numpy(scvod):
    rng = np.random.default_rng(7)
    t = np.zeros(40, otr.TRACK_DTYPE)
    t["net"] = rng.normal(0, 2.0, (40, 3)).astype(np.float32)
    t["length"] = rng.integers(2, 30, 40)
    t["n_dynamic"] = (t["length"] * rng.random(40)).astype(np.int32)
    for travel in (0.0, 2.0, 3.5, 100.0):
        same_result(scvod.tracks_finish(t, travel), finish_ref(t, travel))
    # zero denominators: no track at all, no moving track, no still track, moving tracks of one member only
    same_result(scvod.tracks_finish(t[:0], 2.0), finish_ref(t[:0], 2.0))
    assert math.isnan(scvod.tracks_finish(t[:0], 2.0)["recall_along"]) and math.isnan(scvod.tracks_finish(t[:0], 2.0)["false_alarm"])
    r = scvod.tracks_finish(t, 1e9)
    assert r["moving_tracks"] == 0 and math.isnan(r["recall_along"]) and not math.isnan(r["false_alarm"])
    r = scvod.tracks_finish(t, 0.0)
    assert r["still_tracks"] == 0 and math.isnan(r["false_alarm"]) and not math.isnan(r["recall_along"])
    one = t[:3].copy()
    one["length"], one["n_dynamic"] = 1, 0
    assert math.isnan(scvod.tracks_finish(one, 0.0)["recall_along"])
    # min_travel exactly at |net|: 3-4-12 has the exact length 13
    edge = t[:1].copy()
    edge["net"], edge["length"], edge["n_dynamic"] = (3.0, 4.0, 12.0), 5, 2
    assert scvod.tracks_finish(edge, 13.0)["moving_tracks"] == 1 and scvod.tracks_finish(edge, 13.0)["recall_along"] == 50.0
    assert scvod.tracks_finish(edge, np.nextafter(13.0, 14.0))["moving_tracks"] == 0
    same_result(scvod.tracks_finish(edge, 13.0), finish_ref(edge, 13.0))


# ---- the helper against a brute-force restatement ----
def brute(objects, offsets, nxt, T, cand_begin, cand, prm):
    """the rule over the whole table at once: array arithmetic for the geometry, sorts for the choices, a walk along pred per object for
    the ranks, a grouping by head for the tracks"""
    n = len(objects)
    sc = objects["scan"].astype(np.int64)
    c = objects["center"].astype(np.float32)
    M = T[sc] if n else np.zeros((0, 12), np.float32)
    cw = np.stack([((M[:, 4 * r] * c[:, 0] + M[:, 4 * r + 1] * c[:, 1]) + M[:, 4 * r + 2] * c[:, 2]) + M[:, 4 * r + 3] for r in range(3)], 1)
    e = objects["box_max"] - objects["box_min"]
    diag = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    cls, npts = objects["cls"].astype(np.int64), objects["n_points"].astype(np.int64)
    nx_of = np.asarray([nxt[s] for s in sc], np.int64) if n else np.zeros(0, np.int64)
    diff = cw[None, :, :] - cw[:, None, :]                      # [a][b] = cW(b) - cW(a)
    d2 = (diff[:, :, 0] * diff[:, :, 0] + diff[:, :, 1] * diff[:, :, 1]) + diff[:, :, 2] * diff[:, :, 2]
    g2 = F(prm["gate"]) * F(prm["gate"])
    ratio = F(prm["size_ratio"])
    prop = []                                                    # (b, sort key of the acceptance, a, kind, weight)
    for a in range(n):
        if nx_of[a] < 0:
            continue
        succ = np.arange(n)[sc == nx_of[a]]
        rows = []
        if cls[a] == 2 and cand_begin is not None:
            for b, cnt in cand[cand_begin[a]:cand_begin[a + 1]]:
                if b in succ and cnt >= 0 and cls[b] == 2 and F(cnt) / F(objects["n_voxels"][b]) >= F(prm["occupancy"]):
                    rows.append((-int(cnt), int(b)))
        if rows:
            cnt, b = min(rows)
            prop.append((b, (1, cnt, a), a, 1, -cnt))
            continue
        if (prm["flags"] & otr.NO_GATE) or not ((prm["flags"] & otr.ANY_CLASS) or cls[a] == 2) or npts[a] < prm["min_points"]:
            continue
        ok = (cls[succ] == cls[a]) & (npts[succ] >= prm["min_points"]) & (diag[a] <= ratio * diag[succ]) & \
            (diag[succ] <= ratio * diag[a]) & (d2[a, succ] < g2)
        if ok.any():
            b = min(zip(d2[a, succ][ok], succ[ok]))[1]
            prop.append((int(b), (2, d2[a, b], a), a, 2, 0))
    links = np.zeros(n, otr.LINK_DTYPE)
    links["track"] = links["pred"] = links["succ"] = -1
    for b in sorted({p[0] for p in prop}):
        _, _, a, kind, w = min((p for p in prop if p[0] == b), key=lambda p: p[1])
        links[b]["pred"], links[b]["kind"], links[b]["weight"], links[b]["step"] = a, kind, w, np.sqrt(d2[a, b])
        links[a]["succ"] = b
    head = np.zeros(n, np.int64)
    for i in range(n):
        k, r = i, 0
        while links[k]["pred"] >= 0:
            k, r = int(links[k]["pred"]), r + 1
        links[i]["rank"], head[i] = r, k
    tracks, tobj = [], []
    for h in range(n):
        m = np.arange(n)[head == h]
        if h != (head[h] if n else -1) or len(m) < prm["min_length"]:
            continue
        m = m[np.argsort(links["rank"][m])]
        R = np.zeros((), otr.TRACK_DTYPE)
        R["first_object"], R["last_object"], R["length"], R["first_scan"], R["last_scan"] = m[0], m[-1], len(m), sc[m[0]], sc[m[-1]]
        R["n_dynamic"], R["n_gate_links"] = (objects["dynamic"][m] == 1).sum(), (links["kind"][m] == 2).sum()
        R["object_begin"], R["net"] = len(tobj), cw[m[-1]] - cw[m[0]]
        R["path"], R["max_step"] = np.cumsum(links["step"][m], dtype=np.float32)[-1], links["step"][m].max()
        links["track"][m] = len(tracks)
        tracks.append(R)
        tobj += list(m)
    refused = len(prop) - int((links["pred"] >= 0).sum())
    return links, np.asarray(tracks, otr.TRACK_DTYPE).reshape(-1), np.asarray(tobj, np.int32), refused


def random_case(scvod, seed):
    rng = np.random.default_rng(1000 + seed)
    n_scans = int(rng.integers(1, 7))
    order = rng.permutation(n_scans)
    next_scan = np.full(n_scans, -1, np.int32)
    for k in range(n_scans - 1):
        if rng.random() < 0.8:
            next_scan[order[k]] = order[k + 1]
    if rng.random() < 0.2:
        next_scan[order[-1]] = -3                                # an external table
    scans = []
    for s in range(n_scans):
        objs = []
        for _ in range(int(rng.integers(0, 9))):
            size = rng.choice([1.0, 1.0, 1.5, 4.0]) * np.ones(3)
            centre = (0.5 * rng.integers(-2, 3), 0.5 * rng.integers(-2, 3), 0.5 * rng.integers(0, 2))   # a coarse grid: equal d2 happen
            objs.append(dict(center=centre, size=tuple(size), cls=int(rng.choice([1, 2, 2, 2, 3])),
                             n_points=int(rng.choice([5, 10, 50, 50])), n_voxels=int(rng.choice([4, 10])), dynamic=int(rng.random() < 0.3),
                             cand=[(int(rng.integers(0, 7)), int(rng.choice([2, 6, 6, 9])))
                                   for _ in range(int(rng.integers(0, 4)) if rng.random() < 0.4 else 0)]))
        scans.append(objs)
    objects, offsets, cb, cand = otr.build_table(scans, next_scan)
    poses = np.zeros((n_scans, 6), np.float32)
    if seed % 2:
        poses[:, :3] = 0.5 * rng.integers(-2, 3, (n_scans, 3))
        poses[:, 5] = rng.choice([0.0, 0.25, -1.0], n_scans)
    T = np.stack([scvod.pose_matrix(p) for p in poses])
    prm = dict(otr.DEFAULTS, occupancy=0.6, flags=int(rng.choice([0, 0, 0, 1, 2, 2, 3])), min_length=int(rng.integers(1, 4)),
               gate=float(rng.choice([1.0, 2.0, 3.0])))
    return objects, offsets, next_scan, T, cb, cand, prm


def test_helper_against_brute_force_on_random_tables(scvod):
    seen = dict(k1=0, k2=0, refused=0, tracks=0)
    for seed in range(50):
        objects, offsets, next_scan, T, cb, cand, prm = random_case(scvod, seed)
        ref = otr.object_tracks_ref(objects, offsets, next_scan, T, cb, cand, prm)
        with np.errstate(all="ignore"):
            links, tracks, tobj, refused = brute(objects, offsets, otr.next_table(len(offsets) - 1, next_scan), T, cb, cand, prm)
        assert ref["links"].tobytes() == links.tobytes(), seed
        assert ref["tracks"].tobytes() == tracks.tobytes(), seed
        assert np.array_equal(ref["track_objects"], tobj) and ref["stats"]["refused"] == refused, seed
        assert ref["n_tracks"] == len(tracks) == ref["stats"]["tracks"]
        seen["k1"] += ref["stats"]["overlap_links"]
        seen["k2"] += ref["stats"]["gate_links"]
        seen["refused"] += refused
        seen["tracks"] += len(tracks)
    assert min(seen.values()) > 10, seen   # the cases reach every part of the rule


def test_helper_reports_overflows():
    scans = [[dict(center=(0, 0, 0))], [dict(center=(0.5, 0, 0))], [dict(center=(9, 0, 0))]]
    objects, offsets, cb, cand = otr.build_table(scans)
    prm = dict(otr.DEFAULTS, occupancy=0.6, min_length=1)
    full = otr.object_tracks_ref(objects, offsets, None, otr.identity_matrices(3), cb, cand, prm)
    assert full["n_tracks"] == 2 and list(full["links"]["pred"]) == [-1, 0, -1] and list(full["track_objects"]) == [0, 1, 2]
    assert full["links"]["step"][1] == F(0.5) and full["tracks"]["path"][0] == F(0.5)
    short = otr.object_tracks_ref(objects, offsets, None, otr.identity_matrices(3), cb, cand, prm, cap_tracks=1)
    assert short["n_tracks"] == -1 and short["stats"]["overflow"] == 1 and len(short["tracks"]) == 1 and short["stats"]["written"] == 1
    none = otr.object_tracks_ref(objects, offsets, None, otr.identity_matrices(3), cb, cand, prm, cap_links=2)
    assert none["n_tracks"] == -1 and none["links"] is None and none["stats"] == dict(zip(otr.STATS, (3, 0, 0, 0, 0, 0, 0, 1)))
