"""scvod_object_tracks_device on crafted tables: every output byte against the sequential numpy tracker of
tests/helpers/object_tracks_ref.py, with guard regions behind every output buffer.  The tables are small dicts turned into 64-byte
records by the helper's builder; the sizes are those at which the kernels take another path: pointer-jumping rounds at 2^k and 2^k + 1
scans, candidate runs of 63 / 64 / 65 / 129 (a wave strides over them 64 at a time), 70 proposers of one slot."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import object_tracks_ref as otr  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 8
INVALID, CAPACITY = -1, -4
F = np.float32


@pytest.fixture(scope="module")
def ctx(scvod):
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=4096, max_scans=2)
    yield c
    c.close()


def _dev(a, dtype):
    """a host array on the device; an empty one becomes one unused element, so that its pointer is real"""
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.zeros(64, dtype=dtype, device="cuda")
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda().view(dtype)


def run(scvod, ctx, table, next_scan=None, poses=None, with_cand=True, cap_links=None, cap_tracks=None, want=None, stream=None,
        expect_overflow=False, **prm):
    """one device call on a crafted table, compared with the helper byte for byte; returns (helper's result, device bytes)"""
    import torch
    objects, offsets, cb, cand = table
    n, n_scans = len(objects), len(offsets) - 1
    d_obj, d_off = _dev(objects, torch.uint8), _dev(offsets, torch.int32)
    d_cb = _dev(cb, torch.int32) if with_cand else None
    d_cand = _dev(cand, torch.int32) if with_cand and len(cand) else None
    params = scvod.track_params_default(**prm)
    cap_links = n if cap_links is None else cap_links
    cap_tracks = cap_links if cap_tracks is None else cap_tracks
    want = scvod.TRK_OUTPUTS if want is None else want
    torch.cuda.synchronize()
    out, whole = ctx.object_tracks_device(d_obj, d_off, n_scans, next_scan, poses, d_cb, d_cand, params, cap_links, cap_tracks, want,
                                          guard=GUARD, stream=stream.cuda_stream if stream is not None else None, full=True)
    st = np.zeros(8, np.int64)
    rc = ctx.lib.scvod_object_tracks_stats(ctx.h, st.ctypes.data_as(C.c_void_p))
    got = {w: whole[w].cpu().numpy() for w in whole}
    T = np.stack([scvod.pose_matrix(poses[s] if poses is not None else np.zeros(6, np.float32)) for s in range(n_scans)]) \
        if n_scans else np.zeros((0, 12), np.float32)
    pd = dict(otr.DEFAULTS, **prm)
    if pd["occupancy"] < 0:
        pd["occupancy"] = float(ctx.params.occupancy)
    ref = otr.object_tracks_ref(objects, offsets, next_scan, T, cb if with_cand else None, cand if with_cand else None, pd, cap_links,
                                cap_tracks, want_tracks="tracks" in want)
    assert dict(zip(otr.STATS, st.tolist())) == ref["stats"]
    assert rc == (CAPACITY if ref["stats"]["overflow"] else 0) and bool(ref["stats"]["overflow"]) == expect_overflow
    written = {"links": 0 if ref["links"] is None else ref["links"].view(np.uint8).reshape(-1, 32),
               "tracks": 0 if ref["tracks"] is None else ref["tracks"].view(np.uint8).reshape(-1, 64),
               "track_objects": 0 if ref["track_objects"] is None else ref["track_objects"].view(np.uint8).reshape(-1, 4),
               "n_tracks": np.asarray([ref["n_tracks"]], np.int32).view(np.uint8).reshape(-1, 4)}
    for w in want:
        exp = written[w] if not isinstance(written[w], int) else np.zeros((0, got[w].shape[1]), np.uint8)
        assert np.array_equal(got[w][:len(exp)], exp), f"{w} differ from the helper"
        assert (got[w][len(exp):] == 0xA5).all(), f"{w}: something was written behind the last record"
    return ref, got


def chain_table(n_scans, overlap):
    """one car per scan; overlap: 10 m apart with a candidate each; otherwise 0.5 m apart and no candidate"""
    step = 10.0 if overlap else 0.5
    return otr.build_table([[dict(center=(step * s, 0.25 * (s % 3), 0.0), dynamic=s % 2, cand=[(0, 7 + s % 5)] if overlap else [])]
                            for s in range(n_scans)])


# ---- 1. one object per scan, chained: the round count at 2^k and 2^k + 1 ----
@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("n_scans", [1, 2, 3, 64, 65, 1024, 1025])
def test_chains_of_one_object_per_scan(scvod, ctx, n_scans, overlap):
    ref, _ = run(scvod, ctx, chain_table(n_scans, overlap), min_length=1)
    assert ref["n_tracks"] == 1 and int(ref["tracks"]["length"][0]) == n_scans
    assert list(ref["links"]["rank"]) == list(range(n_scans)) and (ref["links"]["kind"][1:] == (1 if overlap else 2)).all()
    assert ref["stats"]["longest"] == n_scans and ref["tracks"]["n_dynamic"][0] == n_scans // 2


# ---- 2. runs of 63 / 64 / 65 / 129 candidates, the winner in the first lane, the last lane and behind the first 64 ----
RUNS = [(63, 0), (63, 62), (64, 0), (64, 63), (65, 0), (65, 63), (65, 64), (129, 0), (129, 63), (129, 64), (129, 128)]


@pytest.mark.parametrize("n,win", RUNS)
def test_gate_over_a_successor_run(scvod, ctx, n, win):
    succ = [dict(center=(0.5 if j == win else 1.0 + 0.005 * j, 0.0, 0.0)) for j in range(n)]
    ref, _ = run(scvod, ctx, otr.build_table([[dict()], succ]))
    assert ref["links"]["succ"][0] == 1 + win and ref["links"]["kind"][1 + win] == 2 and ref["stats"]["gate_links"] == 1


@pytest.mark.parametrize("n,win", RUNS)
def test_overlap_over_a_candidate_list(scvod, ctx, n, win):
    succ = [dict(center=(50.0 + j, 0.0, 0.0)) for j in range(n)]
    order = list(np.random.default_rng(n * 131 + win).permutation(n))          # the list names the successors in any order
    cand = [(int(j), 100 if k == win else 10 + k % 7) for k, j in enumerate(order)]
    ref, _ = run(scvod, ctx, otr.build_table([[dict(cand=cand)], succ]))
    assert ref["links"]["succ"][0] == 1 + order[win] and ref["links"]["weight"][1 + order[win]] == 100


# ---- 3. ties and edges ----
def test_ties_and_edges(scvod, ctx):
    one = dict(center=(0.0, 0.0, 0.0))
    # equal counts: the smaller B, whatever the order of the list
    for cand in ([(2, 8), (1, 8), (0, 3)], [(1, 8), (2, 8)]):
        ref, _ = run(scvod, ctx, otr.build_table([[dict(cand=cand)], [dict(center=(30.0 + j, 0, 0)) for j in range(3)]]))
        assert ref["links"]["succ"][0] == 2
    # equal d2, placed symmetrically around the query: the smaller B, on either side
    for xs in ((1.0, -1.0), (-1.0, 1.0)):
        ref, _ = run(scvod, ctx, otr.build_table([[one], [dict(center=(x, 0.0, 0.0)) for x in xs]]))
        assert ref["links"]["succ"][0] == 1 and ref["links"]["step"][1] == F(1.0)
    # d2 exactly gate * gate is refused, one ulp below is linked
    below = float(np.nextafter(F(2.0), F(0.0)))
    assert F(below) * F(below) < F(4.0)
    for x, linked in ((2.0, False), (below, True)):
        ref, _ = run(scvod, ctx, otr.build_table([[one], [dict(center=(x, 0.0, 0.0))]]), gate=2.0)
        assert (ref["links"]["succ"][0] == 1) == linked
    # count / n_voxels exactly at the occupancy (the ctx's 0.4f and an exact 0.5), and just below
    assert F(4) / F(10) == F(ctx.params.occupancy)
    for occ, cnt, linked in ((-1.0, 4, True), (-1.0, 3, False), (0.5, 5, True), (0.5, 4, False)):
        ref, _ = run(scvod, ctx, otr.build_table([[dict(cand=[(0, cnt)])], [dict(center=(40.0, 0, 0), n_voxels=10)]]), occupancy=occ)
        assert (ref["links"]["succ"][0] == 1) == linked and ref["stats"]["overlap_links"] == int(linked)
    # diag exactly at the ratio, both ways round, and one ulp beyond
    beyond = float(np.nextafter(F(3.0), F(4.0)))
    for a, b, linked in ((2.0, 3.0, True), (3.0, 2.0, True), (2.0, beyond, False), (beyond, 2.0, False)):
        ref, _ = run(scvod, ctx, otr.build_table([[dict(size=(a, 0.0, 0.0))], [dict(center=(0.5, 0, 0), size=(b, 0.0, 0.0))]]),
                     size_ratio=1.5)
        assert (ref["links"]["succ"][0] == 1) == linked
    # a NaN centre never qualifies, on either side; the finite neighbour is taken instead
    nan = float("nan")
    ref, _ = run(scvod, ctx, otr.build_table([[one, dict(center=(nan, 0.0, 0.0))], [dict(center=(0.1, nan, 0.0)), dict(center=(1.5, 0, 0))]]))
    assert list(ref["links"]["succ"][:2]) == [3, -1] and ref["stats"]["gate_links"] == 1
    # min_points at equality, for the proposer and for the successor
    for pa, pb, linked in ((10, 10, True), (9, 10, False), (10, 9, False)):
        ref, _ = run(scvod, ctx, otr.build_table([[dict(n_points=pa)], [dict(center=(0.5, 0, 0), n_points=pb)]]), min_points=10)
        assert (ref["links"]["succ"][0] == 1) == linked


# ---- 4. competing proposers ----
def test_competing_proposers(scvod, ctx):
    far = dict(center=(60.0, 0.0, 0.0))
    # 1 + 1: the larger count; equal counts: the smaller A
    ref, _ = run(scvod, ctx, otr.build_table([[dict(cand=[(0, 7)]), dict(cand=[(0, 9)])], [far]]))
    assert list(ref["links"]["succ"][:2]) == [-1, 2] and ref["stats"]["refused"] == 1 and ref["links"]["weight"][2] == 9
    ref, _ = run(scvod, ctx, otr.build_table([[dict(cand=[(0, 9)]), dict(cand=[(0, 9)])], [far]]))
    assert list(ref["links"]["succ"][:2]) == [2, -1] and ref["stats"]["refused"] == 1
    # 1 + 2: the overlap wins although the gate's proposer sits on the successor; the refused one stays unlinked, with a free neighbour
    # in reach that it does not get a second try at
    ref, _ = run(scvod, ctx, otr.build_table([[dict(center=(5.0, 0, 0)), dict(center=(50.0, 0, 0), cand=[(0, 9)])],
                                              [dict(center=(5.0, 0, 0)), dict(center=(5.5, 0, 0))]]))
    assert list(ref["links"]["succ"][:2]) == [-1, 2] and ref["links"]["kind"][2] == 1 and ref["stats"]["refused"] == 1
    # 2 + 2: the smaller d2; equal d2: the smaller A
    ref, _ = run(scvod, ctx, otr.build_table([[dict(center=(1.0, 0, 0)), dict(center=(-0.5, 0, 0))], [dict()]]))
    assert list(ref["links"]["succ"][:2]) == [-1, 2] and ref["stats"]["refused"] == 1
    ref, _ = run(scvod, ctx, otr.build_table([[dict(center=(1.0, 0, 0)), dict(center=(-1.0, 0, 0))], [dict()]]))
    assert list(ref["links"]["succ"][:2]) == [2, -1]
    # 70 proposers of one successor: more than a wave of them
    prop = [dict(center=(0.3 + 0.01 * ((k * 37 + 11) % 70), 0.0, 0.0)) for k in range(70)]
    ref, _ = run(scvod, ctx, otr.build_table([prop, [dict()]]), min_length=1)
    winner = min(range(70), key=lambda k: (k * 37 + 11) % 70)
    assert ref["links"]["pred"][70] == winner and ref["stats"]["refused"] == 69 and (ref["links"]["succ"][:70] >= 0).sum() == 1
    assert ref["n_tracks"] == 70 and ref["stats"]["longest"] == 2


# ---- 5. successor tables and poses ----
def test_successor_tables(scvod, ctx):
    def car(x, y=0.0, **kw):
        return dict(center=(x, y, 0.0), **kw)
    scans = [[car(0.3 * s), car(0.3 * s, 8.0), car(20.0 - 0.4 * s, -9.0, cls=1)] for s in range(7)]
    # two interleaved chains
    nxt = [s + 2 if s + 2 < 7 else -1 for s in range(7)]
    ref, _ = run(scvod, ctx, otr.build_table(scans, nxt), nxt)
    assert ref["n_tracks"] == 4 and sorted(ref["tracks"]["length"]) == [3, 3, 4, 4] and ref["links"]["pred"][6] == 0
    # a -1 in the middle, and a negative "external" entry: both end the tracks there
    for end in (-1, -3):
        nxt = [1, 2, end, 4, 5, 6, -1]
        ref, _ = run(scvod, ctx, otr.build_table(scans, nxt), nxt)
        assert ref["n_tracks"] == 4 and sorted(ref["tracks"]["length"]) == [3, 3, 4, 4] and (ref["links"]["succ"][6:9] == -1).all()
    # ANY_CLASS lets the cls 1 objects of the same table link too
    ref, _ = run(scvod, ctx, otr.build_table(scans), flags=otr.ANY_CLASS)
    assert ref["n_tracks"] == 3 and list(ref["tracks"]["length"]) == [7, 7, 7]
    # empty scans first, in the middle and last: a track does not cross an empty scan
    scans = [[], [car(0.0)], [car(0.2)], [], [], [car(0.6)], [car(0.8), car(0.8, 5.0)], []]
    ref, _ = run(scvod, ctx, otr.build_table(scans))
    assert ref["n_tracks"] == 2 and list(ref["tracks"]["first_scan"]) == [1, 5] and list(ref["tracks"]["last_scan"]) == [2, 6]
    # no scan at all, and scans without any object
    for scans in ([], [[], [], []]):
        ref, _ = run(scvod, ctx, otr.build_table(scans))
        assert ref["n_tracks"] == 0 and ref["stats"]["objects"] == 0


def test_poses_decide_not_sensor_frame_distances(scvod, ctx):
    """a parked car and a decoy, seen from a sensor that drives and turns: in the sensor frame the decoy of the next scan sits exactly
    where the car was, in the world it is far away"""
    n = 6
    poses = np.zeros((n, 6), np.float32)
    poses[:, 0], poses[:, 1], poses[:, 5] = 4.0 * np.arange(n), 0.5 * np.arange(n), 0.3 * np.arange(n)

    def to_sensor(s, w):
        T = scvod.pose_matrix(poses[s]).astype(np.float64).reshape(3, 4)
        return tuple(float(v) for v in T[:, :3].T @ (np.asarray(w, np.float64) - T[:, 3]))
    world = (30.0, 3.0, 0.0)
    scans = []
    for s in range(n):
        objs = [dict(center=to_sensor(s, world))]
        if s > 0:
            objs.append(dict(center=to_sensor(s - 1, world)))        # the decoy: the car's sensor-frame place of the scan before
        scans.append(objs)
    table = otr.build_table(scans)
    ref, _ = run(scvod, ctx, table, poses=poses, gate=1.0, min_length=2)
    assert ref["n_tracks"] == 1 and ref["tracks"]["length"][0] == n and (ref["links"]["step"] < 0.01).all()
    wrong, _ = run(scvod, ctx, table, gate=1.0, min_length=2)                # without the poses the decoys are taken
    assert ref["tracks"].tobytes() != wrong["tracks"].tobytes() and wrong["links"]["succ"][0] == 2


# ---- 6. switches and capacities ----
def mixed_table():
    def car(x, y=0.0, **kw):
        return dict(center=(x, y, 0.0), **kw)
    scans = [[car(0.4 * s, 0.0, dynamic=1), car(30.0 + 6.0 * s, 4.0, cand=[(1, 9)])] + ([car(-7.0, 3.0 * s)] if s % 2 else []) +
             ([car(0.4 * s, -12.0, cls=3)] if s < 3 else []) for s in range(5)]
    return otr.build_table(scans)


def test_switches(scvod, ctx):
    t = mixed_table()
    lens = {}
    for ml in (1, 2, 3):
        ref, _ = run(scvod, ctx, t, min_length=ml)
        lens[ml] = sorted(ref["tracks"]["length"])
        assert all(v >= ml for v in lens[ml])
    assert lens[1].count(1) == 5 and lens[2] == [5, 5] and lens[3] == [5, 5]
    ref, _ = run(scvod, ctx, t, flags=otr.NO_GATE)
    assert ref["stats"]["gate_links"] == 0 and ref["stats"]["overlap_links"] == 4 and ref["n_tracks"] == 1
    ref, _ = run(scvod, ctx, t, flags=otr.ANY_CLASS)
    assert ref["n_tracks"] == 3 and sorted(ref["tracks"]["length"]) == [3, 5, 5]
    ref, _ = run(scvod, ctx, t, flags=otr.ANY_CLASS | otr.NO_GATE, with_cand=False)
    assert ref["n_tracks"] == 0 and ref["stats"]["longest"] == 0


def test_capacities_and_count_only(scvod, ctx):
    t = mixed_table()
    n = len(t[0])
    full, _ = run(scvod, ctx, t, min_length=1)
    k = full["n_tracks"]
    assert k > 3
    ref, got = run(scvod, ctx, t, min_length=1, cap_tracks=k - 1, expect_overflow=True)
    assert ref["n_tracks"] == -1 and ref["stats"]["written"] == k - 1 and ref["links"].tobytes() == full["links"].tobytes()
    ref, got = run(scvod, ctx, t, min_length=1, cap_links=n - 1, expect_overflow=True)
    assert ref["n_tracks"] == -1 and ref["stats"]["objects"] == n
    assert (got["links"] == 0xA5).all() and (got["tracks"] == 0xA5).all() and (got["track_objects"] == 0xA5).all()
    # count only: every output NULL but d_n_tracks; then not even that
    ref, got = run(scvod, ctx, t, min_length=1, want=("n_tracks",))
    assert ref["n_tracks"] == k and ref["stats"]["written"] == 0
    run(scvod, ctx, t, min_length=1, want=())
    run(scvod, ctx, t, min_length=1, cap_tracks=0, want=("tracks", "n_tracks"), expect_overflow=True)
    # the tracks without the links: the stage keeps its own link array
    ref, got = run(scvod, ctx, t, want=("tracks", "n_tracks"))
    assert ref["tracks"].tobytes() == run(scvod, ctx, t)[0]["tracks"].tobytes()
    assert ctx.object_tracks_scratch_bytes() > 0


# ---- 7. the same call twice, and on a side stream ----
def test_twice_and_on_a_side_stream(scvod, ctx):
    import torch
    t = otr.build_table([[dict(center=(0.1 * ((k * 13 + s) % 40), 0.7 * k, 0.0), cand=[((k + s) % 90, 5 + k % 4)] if k % 3 == 0 else [])
                          for k in range(90)] for s in range(9)])
    _, a = run(scvod, ctx, t, min_length=1)
    _, b = run(scvod, ctx, t, min_length=1)
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    _, c = run(scvod, ctx, t, min_length=1, stream=side)
    for w in a:
        assert a[w].tobytes() == b[w].tobytes() == c[w].tobytes(), w


# ---- the argument errors on a live ctx, with NULL device pointers: refused before anything is launched ----
def test_argument_errors_on_a_live_ctx(scvod, ctx):
    lib = ctx.lib
    good = scvod.track_params_default()
    dev = lib.scvod_object_tracks_device
    buf = np.zeros(16, np.int64)                          # host memory: no call below may get as far as reading it
    p, odd = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 2)

    def call(objects=p, offs=p, n_scans=2, nxt=None, cb=None, cand=None, prm=good, links=None, cap=4, tracks=None, cap_t=4):
        return dev(ctx.h, objects, offs, n_scans, nxt, None, cb, cand, C.byref(prm) if prm is not None else None, links, cap, tracks,
                   cap_t, None, None, None)
    bad_reserved = scvod.track_params_default()
    bad_reserved.reserved[0] = 1
    for bad in [scvod.track_params_default(**kw) for kw in (
            dict(flags=4), dict(flags=-1), dict(gate=0.0), dict(gate=-1.0), dict(gate=float("inf")), dict(gate=float("nan")),
            dict(size_ratio=0.99), dict(size_ratio=float("nan")), dict(occupancy=float("nan")), dict(min_points=0),
            dict(min_length=0))] + [bad_reserved]:
        assert call(prm=bad) == INVALID
        assert lib.scvod_batch_object_tracks(ctx.h, p, None, C.byref(bad), None, 4, None, 4, None, None, None) == INVALID
    assert call(n_scans=-1) == INVALID
    assert call(cand=p) == INVALID                                             # d_cand without d_cand_begin
    assert call(offs=None) == INVALID and call(objects=None) == INVALID and call(cap=-1) == INVALID and call(cap_t=-1) == INVALID
    for nx in ([1, 1, -1], [1, 2, 0], [3, -1, -1], [0, -1, -1]):
        t = np.asarray(nx, np.int32)
        assert call(n_scans=3, nxt=t.ctypes.data_as(C.c_void_p)) == INVALID
    for kw in (dict(objects=odd), dict(offs=odd), dict(cb=odd), dict(cb=p, cand=odd), dict(links=odd), dict(tracks=odd)):
        assert call(**kw) == INVALID, kw
    assert b"" != lib.scvod_last_error(ctx.h)
