"""scvod_batch_object_visibility (csrc/scvod_objvis.hip) against the numpy statement of the call (tests/helpers/object_visibility_ref.py),
byte for byte: records, output bytes and the 8 stats words, with a guard region behind every capacity.  The crafted batch of
test_gpu_object_shapes.py holds objects of 30 .. 4500 members and a K64 scan: objects inside a tile, across one tile edge, and over a
whole tile with parts of both neighbours.  The verdict bytes and the pair counters are seeded per member by the tests themselves, so no
visibility call is needed until the end-to-end chain."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import class_map_ref as cmr  # noqa: E402
import map_ref as mr  # noqa: E402
import object_visibility_ref as ovr  # noqa: E402
from test_capi_object_visibility import OV_WRAP_CASES  # noqa: E402
from test_gpu_async_chain import _batch, _new_ctx, _stream, _track  # noqa: E402
from test_gpu_object_shapes import _crafted, _prepared  # noqa: E402
from test_gpu_object_truth import Tru, _dev, _tstats  # noqa: E402
from test_gpu_objects import GUARD, NO_TRACK, Tab, _full  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, STATE = -1, -4, -5
FILL = 0xA5
SEED = 20261
U, K, S = ovr.UNTESTED, ovr.KEEP, ovr.SEEN_THROUGH
TILE = ovr.TILE


class Run:
    """the buffers of one call with a guard region behind every capacity.  cap None: no d_records; out: "new", "in_place" or None"""

    def __init__(self, v, q=None, objects=None, cap=None, out="new"):
        import torch
        self.n, self.cap, self.mode = len(v), cap, out
        self.v = torch.full((self.n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.v[:self.n] = torch.from_numpy(np.ascontiguousarray(v, np.uint8)).cuda()
        self.q = None if q is None else torch.from_numpy(np.ascontiguousarray(q, np.uint32).view(np.int32)).cuda()
        self.obj = None if objects is None else torch.from_numpy(np.ascontiguousarray(objects).view(np.uint8).reshape(-1).copy()).cuda()
        self.rec = None if cap is None else torch.full(((cap + GUARD) * 48,), FILL, dtype=torch.uint8, device="cuda")
        self.out = self.v if out == "in_place" else (torch.full((self.n + GUARD,), FILL, dtype=torch.uint8, device="cuda") if out else None)
        torch.cuda.synchronize()

    def call(self, ctx, prm=None, stream=None):
        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        return ctx.lib.scvod_batch_object_visibility(ctx.h, ptr(self.v), ptr(self.q), ptr(self.obj), C.byref(prm) if prm is not None else None,
                                                     ptr(self.rec), int(self.cap or 0), ptr(self.out), C.c_void_p(stream or 0))

    def host(self, v_in):
        """dict(records bytes [cap * 48] or None, verdict [n] or None); asserts the guard regions and that the input is untouched"""
        r = dict(records=None, verdict=None)
        if self.rec is not None:
            raw = self.rec.cpu().numpy()
            assert (raw[self.cap * 48:] == FILL).all(), "records were written at or behind cap_records"
            r["records"] = raw[:self.cap * 48]
        if self.out is not None:
            o = self.out.cpu().numpy()
            assert (o[self.n:] == FILL).all(), "output bytes were written behind the batch's points"
            r["verdict"] = o[:self.n]
        if self.mode != "in_place":
            vv = self.v.cpu().numpy()
            assert np.array_equal(vv[:self.n], v_in) and (vv[self.n:] == FILL).all(), "the input bytes changed"
        return r


def _ostats(ctx):
    out = np.zeros(8, np.int64)
    rc = ctx.lib.scvod_batch_object_visibility_stats(ctx.h, out.ctypes.data_as(C.c_void_p))
    return rc, out


def _prm(scvod, p):
    return scvod.object_visibility_params_default(**p)


def _against_helper(scvod, c, v, q, dyn, p, out="new", cap="all", what=""):
    """one call against the helper: every byte.  Returns (device result, helper result)"""
    k = len(c["rec"])
    cap = k if cap == "all" else cap
    objects = None
    if dyn is not None:
        objects = c["rec"].copy()
        objects["dynamic"] = dyn
    run = Run(v, q, objects, cap, out)
    assert run.call(c["ctx"], _prm(scvod, p)) == 0, c["ctx"].lib.scvod_last_error(c["ctx"].h)
    rc, st = _ostats(c["ctx"])
    want = ovr.run(c["pobj"], k, v, q, dyn, ovr.params(**p), cap)
    got = run.host(v)
    assert np.array_equal(st, want["stats"]), (what, st.tolist(), want["stats"].tolist())
    assert rc == (CAPACITY if want["stats"][7] else 0), (what, rc)
    if cap is not None:
        w = want["records"][:cap].view(np.uint8).reshape(-1)
        assert (got["records"][len(w):] == FILL).all(), f"{what}: something was written behind the last record"
        same = (got["records"][:len(w)].reshape(-1, 48) == w.reshape(-1, 48)).all(axis=1)
        assert same.all(), f"{what}: {int((~same).sum())} of {len(same)} records differ from the helper, first {int(np.argmin(same))}: " \
                           f"{got['records'].view(ovr.DTYPE)[int(np.argmin(same))]} != {want['records'][int(np.argmin(same))]}"
    if out:
        bad = np.nonzero(got["verdict"] != want["verdict"])[0]
        assert bad.size == 0, f"{what}: {bad.size} output bytes differ from the helper, first at point {bad[:5]}, objects {c['pobj'][bad[:5]]}"
    return got, want


def _object_of(c, n_points):
    o = np.nonzero((c["rec"]["scan"] == 0) & (c["rec"]["n_points"] == n_points))[0]
    assert len(o) == 1, (n_points, o)
    return int(o[0])


def _seeded(c, seed, small_pairs=False):
    """verdict bytes and pair counters per input point: every object draws its own share of SEEN_THROUGH, KEEP, UNTESTED and a stray
    byte 7, so that both verdicts and objects that do not vote occur; the points of no object get bytes too"""
    rng = np.random.default_rng(seed)
    n, k = len(c["pobj"]), len(c["rec"])
    share = rng.dirichlet([0.7, 0.7, 0.5, 0.1], k + 1)                 # (row k: the points of no object)
    cum = np.cumsum(share[c["pobj"]], axis=1)                          # (-1 indexes row k)
    v = np.array([S, K, U, 7], np.uint8)[(rng.random(n)[:, None] > cum[:, :3]).sum(axis=1)]
    q = rng.integers(0, 4 if small_pairs else 256, (n, 4), dtype=np.uint32)
    q = (q[:, 0] | q[:, 1] << 8 | q[:, 2] << 16 | q[:, 3] << 24).astype(np.uint32)
    return v, q


@pytest.fixture(scope="module")
def crafted(scvod):
    import torch
    b = _crafted(scvod)
    ctx = _prepared(scvod, b)
    rec, offs, mem, pobj = _full(ctx, b, NO_TRACK)
    assert np.array_equal(ovr.point_object_from_members(rec, mem, b.offs, int(b.offs[-1])), pobj), "a member is what the member list names"
    c = dict(ctx=ctx, b=b, rec=rec, mem=mem, pobj=pobj, n=int(b.offs[-1]))
    # the table holds every way an object can lie in the tiles
    first, last = rec["point_begin"] // TILE, (rec["point_begin"] + rec["n_points"] - 1) // TILE
    assert set([30, 40, 64, 100, 128, 129, 193, 300, 4500]) <= set(rec["n_points"][rec["scan"] == 0].tolist())
    assert (first == last).any(), "no object inside one tile"
    assert (last == first + 1).any(), "no object that crosses exactly one tile edge"
    whole = (last >= first + 2) & (rec["point_begin"] % TILE != 0) & ((rec["point_begin"] + rec["n_points"]) % TILE != 0)
    assert whole.any(), "no object that covers a whole tile and parts of both neighbours"
    # ... and the 512-position ranges of the waves: inside one, across one edge, over a whole range
    wf, wl = rec["point_begin"] // 512, (rec["point_begin"] + rec["n_points"] - 1) // 512
    assert (wf == wl).any() and ((wl == wf + 1) & (first == last)).any() and (wl >= wf + 2).any(), "wave ranges"
    assert (rec["scan"] == 3).sum() > 16 and int(rec["point_begin"][-1] + rec["n_points"][-1]) == len(mem) > 4 * TILE
    yield c
    torch.cuda.synchronize()
    ctx.close()


# ---- 1. every combination of the flags, in place and not -------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("out", ["new", "in_place"])
def test_flags_against_the_helper(scvod, crafted, flags, out):
    c = crafted
    v, q = _seeded(c, SEED + flags)
    dyn = (np.arange(len(c["rec"])) % 3 == 1).astype(np.uint8)       # the table is a SCVOD_OBJ_NO_TRACK one: the flags are the test's own
    p = dict(flags=flags, min_points=35, min_tested=20)
    got, want = _against_helper(scvod, c, v, q, dyn if flags & 2 else None, p, out, what=f"flags {flags} {out}")
    rec = want["records"]
    assert (rec["how"] == 0).any() and (rec["how"] == 1).any() and ((rec["how"] == 2).any() == bool(flags & 2))
    assert (rec["verdict"] == K).any() and (rec["verdict"] == S).any() and want["stats"][4] > 0 and want["stats"][5] > 0
    assert (want["verdict"] != v).any() and (want["verdict"][c["pobj"] < 0] == v[c["pobj"] < 0]).all()
    if flags == 0:                                                     # the pair counters are summed whether or not they vote ...
        assert rec["sum_through"].any() and rec["sum_other"].any()
        none, _ = _against_helper(scvod, c, v, None, None, p, out, what="no d_votes")   # ... and are 0 without d_votes
        assert not none["records"].view(ovr.DTYPE)["sum_agree"].any()
        assert np.array_equal(none["verdict"], got["verdict"])


def test_defaults_and_null_params(scvod, crafted):
    c = crafted
    v, q = _seeded(c, SEED + 9)
    run = Run(v, q, None, len(c["rec"]))
    assert run.call(c["ctx"], None) == 0
    rc, st = _ostats(c["ctx"])
    want = ovr.run(c["pobj"], len(c["rec"]), v, q, None, ovr.params(), len(c["rec"]))
    got = run.host(v)
    assert rc == 0 and np.array_equal(st, want["stats"])
    assert np.array_equal(got["records"], want["records"].view(np.uint8).reshape(-1)) and np.array_equal(got["verdict"], want["verdict"])
    out = c["ctx"].batch_object_visibility(run.v[:c["n"]], run.q)                   # the shim, both outputs
    assert np.array_equal(out["verdict"].cpu().numpy(), want["verdict"])
    k = c["ctx"].batch_object_visibility_stats()["written"]
    assert k == len(c["rec"]) and np.array_equal(out["records"][:k].cpu().numpy().reshape(-1), got["records"])


# ---- 2. equality and one above ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("members", [64, 129, 4500])
@pytest.mark.parametrize("pool", [0, 1])
def test_vote_at_equality_and_one_above(scvod, crafted, members, pool):
    c = crafted
    o = _object_of(c, members)
    v, q = _seeded(c, SEED + 20 + members, small_pairs=True)
    m = np.nonzero(c["pobj"] == o)[0]
    v[m] = np.array([S, K, U, 7], np.uint8)[np.arange(members) % 4]                # a quarter each
    if pool:
        t, a = int((q[m] & 0xFF).sum()), int(((q[m] >> 8) & 0xFF).sum())
    else:
        t, a = int((v[m] == S).sum()), int((v[m] == K).sum())
    assert t > 0 and a > 0 and t + a <= 1 << 20
    moved = np.zeros(2, np.int64)
    for num, verdict in ((t, S), (t + 1, K)):
        p = dict(flags=pool, vote_num=num, vote_den=t + a, min_through=1)
        got, want = _against_helper(scvod, c, v, q, None, p, what=f"{members} members, {num} / {t + a}, pool {pool}")
        assert want["records"][o]["verdict"] == verdict and want["records"][o]["how"] == 1
        assert (got["verdict"][m] == verdict).all() and (v[m] == U).any() and (v[m] == 7).any(), "the UNTESTED members go with the object"
        moved += want["stats"][4:6]
    assert moved[0] > 0 and moved[1] > 0, "the vote moved no member in one of the two directions"


@pytest.mark.parametrize("kw, verdict", [(dict(min_points=129), S), (dict(min_points=130), -1), (dict(min_tested=65), S), (dict(min_tested=66), -1),
                                         (dict(vote_num=0), S), (dict(vote_num=5, vote_den=5), K), (dict(vote_num=8, vote_den=13), S),
                                         (dict(min_through=41), K), (dict(min_through=-3, vote_num=0), S)],
                         ids=["points129", "points130", "tested65", "tested66", "num0", "num=den", "8/13", "through41", "through-3"])
def test_min_points_min_tested_and_the_ends_of_the_rule(scvod, crafted, kw, verdict):
    c = crafted
    o = _object_of(c, 129)
    v, q = _seeded(c, SEED + 30)
    m = np.nonzero(c["pobj"] == o)[0]
    v[m] = np.array([S] * 40 + [K] * 25 + [U] * 64, np.uint8)                      # 65 tested members
    got, want = _against_helper(scvod, c, v, q, None, kw, what=str(kw))
    assert want["records"][o]["verdict"] == verdict and want["records"][o]["how"] == (1 if verdict >= 0 else 0)   # (40 * 13 == 8 * 65)
    assert (got["verdict"][m] == (verdict if verdict >= 0 else v[m])).all()


# ---- 3. a product that needs 64 bits ------------------------------------------------------------------------------------------------------

def test_the_64_bit_product_on_the_largest_object(scvod, crafted):
    c = crafted
    o = _object_of(c, 4500)
    v, q = _seeded(c, SEED + 40)
    m = np.nonzero(c["pobj"] == o)[0]
    q[m] = 0xFFFFFFFF                                                               # every byte counter at 255
    v[m] = K
    big = 1 << 20
    for num, verdict in ((big // 2, S), (big // 2 + 1, K)) + OV_WRAP_CASES:
        got, want = _against_helper(scvod, c, v, q, None, dict(flags=1, vote_num=num, vote_den=big), what=f"num {num}")
        r = got["records"].view(ovr.DTYPE)[o]
        assert r["sum_through"] == r["sum_agree"] == r["sum_occluded"] == r["sum_other"] == 4500 * 255 and r["verdict"] == verdict, (num, r)
        assert (got["verdict"][m] == verdict).all()


# ---- 4. capacity ----------------------------------------------------------------------------------------------------------------------------

def test_capacity_latch_and_guard_regions(scvod, crafted):
    c = crafted
    ctx, k = c["ctx"], len(c["rec"])
    v, q = _seeded(c, SEED + 50)
    p = dict(flags=1)
    full, want = _against_helper(scvod, c, v, q, None, p, what="full")
    for cap in (k - 1, 0):
        got, w = _against_helper(scvod, c, v, q, None, p, cap=cap, what=f"cap {cap}")   # (asserts SCVOD_ERR_CAPACITY and the words)
        assert w["stats"][6] == cap and w["stats"][7] == 1
        assert np.array_equal(got["verdict"], full["verdict"]), "an overflow changes no output byte"
        assert np.array_equal(got["records"], full["records"][:cap * 48])
        with pytest.raises(scvod.ScvodError):
            ctx.batch_object_visibility_stats()
        again, _ = _against_helper(scvod, c, v, q, None, p, what="after the overflow")    # the latch belongs to the LAST call
        assert np.array_equal(again["records"], full["records"]) and np.array_equal(again["verdict"], full["verdict"])
    none, w = _against_helper(scvod, c, v, q, None, p, cap=None, what="no d_records")     # NULL: no records, nothing to overflow
    assert w["stats"][6] == 0 and w["stats"][7] == 0 and np.array_equal(none["verdict"], full["verdict"])
    only, _ = _against_helper(scvod, c, v, q, None, p, out=None, what="records alone")
    assert np.array_equal(only["records"], full["records"])
    big, _ = _against_helper(scvod, c, v, q, None, p, cap=k + 37, what="a larger buffer")
    assert (big["records"][k * 48:] == FILL).all() and np.array_equal(big["records"][:k * 48], full["records"])


# ---- the refusals on a live ctx: nothing is written -------------------------------------------------------------------------------------

def test_argument_errors_on_a_live_ctx(scvod, crafted):
    import torch
    c = crafted
    ctx, n, k = c["ctx"], c["n"], len(c["rec"])
    v, q = _seeded(c, SEED + 60)
    run = Run(v, q, c["rec"], k)
    call = ctx.lib.scvod_batch_object_visibility
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    good = _prm(scvod, {})
    ok = [ctx.h, ptr(run.v), ptr(run.q), ptr(run.obj), C.byref(good), ptr(run.rec), k, ptr(run.out), None]

    def refused(**kw):
        a = list(ok)
        for name, val in kw.items():
            a[("ctx", "v", "q", "obj", "prm", "rec", "cap", "out", "stream").index(name)] = val
        return call(*a) == INVALID
    assert refused(v=None)
    bad_reserved = _prm(scvod, {})
    bad_reserved.reserved[0] = 7
    for bad in [_prm(scvod, kw) for kw in (dict(flags=4), dict(flags=8 | 1), dict(min_points=0), dict(min_tested=0), dict(min_tested=-2),
                                           dict(vote_den=0), dict(vote_den=(1 << 20) + 1), dict(vote_num=-1),
                                           dict(vote_num=(1 << 20) + 1))] + [bad_reserved]:
        assert refused(prm=C.byref(bad))
    assert refused(prm=C.byref(_prm(scvod, dict(flags=1))), q=None)
    assert refused(prm=C.byref(_prm(scvod, dict(flags=2))), obj=None)
    assert refused(cap=-1)
    assert refused(q=ptr(run.q, 2)) and refused(rec=ptr(run.rec, 2)) and refused(obj=ptr(run.obj, 4))
    assert refused(out=ptr(run.v, 1)) and refused(out=ptr(run.v, n - 1)), "a partial overlap with d_verdict"
    assert refused(out=ptr(run.q, 4 * n - 1)) and refused(out=ptr(run.rec, 48 * k - 1)) and refused(out=ptr(run.obj, 8))
    assert ctx.lib.scvod_batch_object_visibility_stats(ctx.h, None) == INVALID
    torch.cuda.synchronize()
    got = run.host(v)
    assert (got["records"] == FILL).all() and (got["verdict"] == FILL).all(), "a refused call wrote something"
    # vote_num above vote_den is legal (nothing is ever seen through by the ratio), and so is d_verdict_out right behind d_verdict
    _against_helper(scvod, c, v, q, None, dict(vote_num=3, vote_den=2), what="num > den")
    both = torch.full((2 * n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    both[:n] = run.v[:n]
    assert call(ctx.h, ptr(both), None, None, None, None, 0, ptr(both, n), None) == 0
    want = ovr.run(c["pobj"], k, v)
    assert np.array_equal(both.cpu().numpy()[n:2 * n], want["verdict"]) and (both.cpu().numpy()[2 * n:] == FILL).all()


# ---- 5. state -------------------------------------------------------------------------------------------------------------------------------

def test_state_errors_are_those_of_the_object_truth(scvod):
    import torch
    b = _batch(scvod, "K6")
    n = int(b.offs[-1])
    ctx = _new_ctx(scvod, [b])
    run = Run(np.ones(n, np.uint8), None, None, n)
    cnt = Tab(b, 0, 0, members=False, points=False)
    tab = Tab(b, n, n)
    torch.cuda.synchronize()
    assert _ostats(ctx)[0] == STATE                                        # before the first call
    assert run.call(ctx) == STATE                                          # no batch, no table
    assert ctx.batch_object_visibility_scratch_bytes() == 0
    ctx.batch_process(b.d, b.offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    assert run.call(ctx) == STATE                                          # a batch, but no table yet
    assert cnt.call(ctx, NO_TRACK, records=False) == 0
    assert run.call(ctx) == STATE                                          # a count-only table is none
    assert _ostats(ctx)[0] == STATE and ctx.batch_object_visibility_scratch_bytes() == 0
    assert tab.call(ctx, NO_TRACK) == 0 and run.call(ctx) == 0 and _ostats(ctx)[0] == 0
    assert cnt.call(ctx, NO_TRACK, records=False) == 0 and run.call(ctx) == 0   # a count-only call later leaves the lists as they are
    ctx.batch_cluster()                                                    # another clustering: the lists are stale
    assert run.call(ctx) == STATE
    ctx.batch_cluster_types()
    assert run.call(ctx) == STATE
    _track(ctx, b, b.T, b.nxt, None, 1)
    assert tab.call(ctx, 0) == 0 and run.call(ctx) == 0                    # a table that read the tracking result
    ctx.batch_cluster_types()                                              # ... which is stale now: the table's own rule
    assert tab.call(ctx, 0) == INVALID and run.call(ctx) == INVALID
    assert tab.call(ctx, NO_TRACK) == 0 and run.call(ctx) == 0
    ctx.batch_process(b.d, b.offs)                                         # a new batch
    assert run.call(ctx) == STATE
    torch.cuda.synchronize()
    got = run.host(np.ones(n, np.uint8))                                   # (the guard regions of every call above)
    ctx.close()


# ---- 6. / 7. two runs, no side effects ------------------------------------------------------------------------------------------------------

def test_two_runs_and_nothing_else_moves(scvod, crafted):
    import torch
    c = crafted
    ctx, b, k = c["ctx"], c["b"], len(c["rec"])
    v, q = _seeded(c, SEED + 70)
    gt = np.random.default_rng(SEED + 71).integers(0, 1 << 32, c["n"], dtype=np.uint64).astype(np.uint32)
    d_gt = _dev(gt)

    def truth():
        t = Tru(k)
        assert t.call(ctx, d_gt) == 0
        rc, st = _tstats(ctx)
        assert rc == 0
        return t.host().copy(), st
    truth_before = truth()
    _against_helper(scvod, c, v, q, None, dict(flags=1), what="warm")      # (the stage's own scratch exists from here on)
    others = sorted(name for name in dir(ctx) if name.endswith("scratch_bytes") and name != "batch_object_visibility_scratch_bytes")
    assert len(others) >= 8 and "batch_objects_scratch_bytes" in others and "visibility_scratch_bytes" in others
    sizes = {name: getattr(ctx, name)() for name in others}
    arena, own = ctx.arena_bytes(), ctx.batch_object_visibility_scratch_bytes()
    assert own >= 32 * ((c["n"] + TILE - 1) // TILE) + 64
    tab = Tab(b, c["n"], c["n"])
    assert tab.call(ctx, NO_TRACK) == 0
    torch.cuda.synchronize()
    raw = [x.cpu().numpy().copy() for x in (tab.rec, tab.offs, tab.mem, tab.pobj)]
    one, _ = _against_helper(scvod, c, v, q, c["rec"]["dynamic"], dict(flags=3), what="first run")
    two, _ = _against_helper(scvod, c, v, q, c["rec"]["dynamic"], dict(flags=3), what="second run")
    assert np.array_equal(one["records"], two["records"]) and np.array_equal(one["verdict"], two["verdict"]), "two runs differ"
    for x, y in zip(raw, (tab.rec, tab.offs, tab.mem, tab.pobj)):
        assert np.array_equal(x, y.cpu().numpy()), "the table's buffers changed"
    assert ctx.arena_bytes() == arena and ctx.batch_object_visibility_scratch_bytes() == own
    assert {name: getattr(ctx, name)() for name in others} == sizes, "another stage's scratch moved"
    after = truth()
    assert np.array_equal(after[0], truth_before[0]) and after[1] == truth_before[1], "scvod_batch_object_truth sees another table"


# ---- 8. the chain it is meant for ---------------------------------------------------------------------------------------------------------------

def test_the_whole_chain_on_a_side_stream_without_a_host_read(scvod):
    """batch_process -> cluster -> types -> track -> batch_objects -> batch_visibility -> the vote with SCVOD_OBJVIS_WITH_TRACK ->
    accumulate_labelled keeping everything but SEEN_THROUGH, all enqueued on one stream that is not the current one, synchronised once"""
    import torch
    b = _batch(scvod, "D")
    n = int(b.offs[-1])
    stream = _stream()
    st = stream.cuda_stream
    ctx = _new_ctx(scvod, [b])
    tab = Tab(b, n, n)
    leaf = 0.2
    m = scvod.StaticMap(1 << 22, leaf=leaf, kind=scvod.MAP_KIND_LABELLED)
    keep_table = [x for x in range(256) if x != S]
    torch.cuda.synchronize()                                               # (nothing is pending on the current stream, which stays idle)
    assert torch.cuda.current_stream().cuda_stream != st
    ctx.batch_process(b.d, b.offs.copy(), stream=st, sync=False)
    ctx.batch_cluster(stream=st, sync=False)
    ctx.batch_cluster_types(stream=st, sync=False)
    keep = _track(ctx, b, b.T.copy(), b.nxt.copy(), st, 0)
    assert tab.call(ctx, 0, st) == 0, ctx.lib.scvod_last_error(ctx.h)
    vis = ctx.batch_visibility(b.poses, b.nxt, want=("votes", "verdict"), stream=st)
    out = ctx.batch_object_visibility(vis["verdict"], vis["votes"], tab.rec, scvod.object_visibility_params_default(flags=scvod.OBJVIS_WITH_TRACK),
                                      cap=n // 8, stream=st)
    m.accumulate_labelled(b.d, out["verdict"], b.offs, b.poses, keep=keep_table, stream=st)
    stream.synchronize()
    rec, offs, mem, pobj = tab.host(b)
    k = int(offs[-1])
    stats = ctx.batch_object_visibility_stats()
    v, q = vis["verdict"].cpu().numpy(), vis["votes"].cpu().numpy().view(np.uint32)
    want = ovr.run(pobj, k, v, q, rec[:k]["dynamic"], ovr.params(flags=ovr.WITH_TRACK), n // 8)
    assert [stats[name] for name in ovr.STATS] == want["stats"].tolist()
    assert stats["forced"] == int((rec[:k]["dynamic"] == 1).sum()) > 0 and stats["voted"] > 0 and stats["moved_to_seen_through"] > 0
    assert np.array_equal(out["records"][:k].cpu().numpy().reshape(-1), want["records"].view(np.uint8).reshape(-1))
    got = out["verdict"].cpu().numpy()
    assert np.array_equal(got, want["verdict"]) and (got != v).any()
    ek, ev, _ = cmr.definition(scvod, b.x, got, b.offs, b.poses, leaf, keep=cmr.table256(keep_table))
    gk, gv = mr.sorted_records(m)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    assert not (cmr.unpack_labelled(gv)[3] == S).any()
    del keep
    m.close()
    ctx.close()
