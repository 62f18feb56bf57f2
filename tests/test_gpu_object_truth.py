"""scvod_batch_object_truth / scvod_batch_object_truth_stats on the device, through the C-ABI: one 32-byte record per object of the
table against the numpy statement (tests/helpers/object_truth_ref.py: np.unique over the labels of the object's member list).  Every
labelling is built FROM the table's own member list, so the test controls the multiset of every object; every comparison with the
helper is on the raw record bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import object_truth_ref as otr  # noqa: E402
from test_gpu_async_chain import MAP_CELLS, Batch, _batch, _everything, _new_ctx, _same, _stream, _track, _transforms  # noqa: E402
from test_gpu_export import _labels, _tracked  # noqa: E402
from test_gpu_object_shapes import BLOCKS, _crafted, _crafted_scan, _prepared  # noqa: E402
from test_gpu_objects import GUARD, NO_TRACK, Tab, _full  # noqa: E402

pytestmark = pytest.mark.gpu

STATE, CAPACITY, INVALID = -5, -4, -1
SEED = 20261019
FILL = 0xA5
CAR_M = 252   # a moving class of the default list


def _key(cls, inst):
    return (inst << 16) | cls


class Tru:
    """output buffer of one scvod_batch_object_truth call with a guard region behind `cap` records"""

    def __init__(self, cap):
        import torch
        self.cap = cap
        self.buf = torch.full(((cap + GUARD) * 32,), FILL, dtype=torch.uint8, device="cuda")

    def call(self, ctx, d_gt, params=None, stream=None):
        return ctx.lib.scvod_batch_object_truth(ctx.h, C.c_void_p(d_gt.data_ptr()), C.byref(params) if params is not None else None,
                                                C.c_void_p(self.buf.data_ptr()), int(self.cap), C.c_void_p(stream or 0))

    def host(self):
        raw = self.buf.cpu().numpy()
        assert (raw[self.cap * 32:] == FILL).all(), "truth records were written at or behind cap_truth"
        return raw[:self.cap * 32]


def _tstats(ctx):
    out = np.full(8, -7, np.int64)
    rc = ctx.lib.scvod_batch_object_truth_stats(ctx.h, out.ctypes.data_as(C.c_void_p))
    return rc, out.tolist()


def _dev(gt):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(gt, np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return d


def _truth(ctx, gt, k, params=None, stream=None):
    """one call into a buffer of exactly k records, synchronised: (records, stats)"""
    t = Tru(k)
    assert t.call(ctx, _dev(gt), params, stream) == 0, ctx.lib.scvod_last_error(ctx.h)
    rc, st = _tstats(ctx)
    assert rc == 0 and st[0] == st[1] == k and st[2] == 0 and st[6] == st[7] == 0, (rc, st, k)
    return t.host().view(otr.DTYPE).copy(), st


def _check(b, rec, mem, gt, got, st, what, dynamic=otr.DYNAMIC):
    """the records against the helper, and the stats words 4 and 5 against numpy"""
    want = otr.records(rec, mem, b.offs, gt, dynamic)
    same = (got.view(np.uint8).reshape(-1, 32) == want.view(np.uint8).reshape(-1, 32)).all(axis=1)
    assert same.all(), f"{what}: {int((~same).sum())} of {len(rec)} records differ from the helper, first {int(np.argmin(same))}: " \
                       f"{got[int(np.argmin(same))]} != {want[int(np.argmin(same))]}"
    assert np.array_equal(got["n_points"], rec["n_points"])
    assert st[4] == int(otr.moving_mask(gt, dynamic).sum()), f"{what}: the moving points of the batch"
    assert st[5] == int(want["n_moving"].sum()), f"{what}: the moving members of all objects"
    assert st[3] == int((want["n_distinct"] > otr_onchip()).sum()), f"{what}: exactly the objects beyond the on-chip bound take the fallback"
    return want


def otr_onchip():
    import scvod_py
    return scvod_py.OBJ_TRUTH_ONCHIP_LABELS


def _members(b, rec, mem, o):
    """the batch indices of object o's member points, in member order"""
    r = rec[o]
    return int(b.offs[r["scan"]]) + mem[r["point_begin"]:r["point_begin"] + r["n_points"]].astype(np.int64)


def _background(b, seed=3):
    """labels of the points of no object: anything, they must not matter to a record (some of a moving class: stats word 4 sees them)"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 40, 48, 70, CAR_M, _key(CAR_M, 9), 0xFFFFFFFF], np.uint32), int(b.offs[-1]))


def _object_of(rec, n_points, scan=0):
    idx = np.flatnonzero((rec["scan"] == scan) & (rec["n_points"] == n_points))
    assert len(idx) == 1, f"the crafted batch has no single object of {n_points} members in scan {scan}"
    return int(idx[0])


@pytest.fixture(scope="module")
def crafted(scvod):
    """the crafted batch on a ctx with a SCVOD_OBJ_NO_TRACK table (10.): (ctx, batch, records, members)"""
    b = _crafted(scvod)
    ctx = _prepared(scvod, b)
    rec, offs, mem, _ = _full(ctx, b, NO_TRACK)
    assert sorted(rec["n_points"][rec["scan"] == 0].tolist()) == sorted(k for k, _, _ in BLOCKS)
    assert offs[4] > offs[3], "the K64 scan holds no object"
    yield ctx, b, rec, mem
    ctx.close()


# ---- 1. one label per object ----------------------------------------------------------------------------------------------------------------

def test_one_label_per_object(scvod, crafted):
    ctx, b, rec, mem = crafted
    gt = _background(b)
    special = [0, 0xFFFFFFFF, _key(CAR_M, 1), _key(CAR_M, 0xFFFF), 0xFFFF, 1 << 16, 40]
    for o in range(len(rec)):
        gt[_members(b, rec, mem, o)] = special[o] if o < len(special) else _key(10 + o % 50, o)
    got, st = _truth(ctx, gt, len(rec))
    _check(b, rec, mem, gt, got, st, "one label per object")
    assert (got["n_distinct"] == 1).all() and np.array_equal(got["n_label"], rec["n_points"]) and np.array_equal(got["n_class"], rec["n_points"])
    assert got["label"][:len(special)].tolist() == special and st[3] == 0
    assert got["n_moving"][:4].tolist() == [0, 0, rec["n_points"][2], rec["n_points"][3]]
    assert not got["reserved"].any()
    # the shim's form
    d = ctx.batch_object_truth(_dev(gt))
    stats = ctx.batch_object_truth_stats()
    assert stats == dict(written=len(rec), objects=len(rec), overflow=False, fallback_objects=0, moving_points=st[4], moving_members=st[5])
    assert np.array_equal(d.cpu().numpy()[:len(rec)].reshape(-1), got.view(np.uint8))
    assert ctx.batch_object_truth_scratch_bytes() > 0


# ---- 2. ties -----------------------------------------------------------------------------------------------------------------------------------

def test_exact_ties_go_to_the_smallest_label(scvod, crafted):
    ctx, b, rec, mem = crafted
    slots = 2 * otr_onchip()      # the wave's table
    gt = _background(b)
    rng = np.random.default_rng(SEED)
    for o in range(len(rec)):
        gt[_members(b, rec, mem, o)] = _key(70, o)
    expect = {}
    # two-way, the labels differ only above bit 16: one class, two instances
    o = _object_of(rec, 64)
    m = _members(b, rec, mem, o)
    gt[m] = np.where(rng.permutation(64) < 32, _key(CAR_M, 7), _key(CAR_M, 3)).astype(np.uint32)
    expect[o] = (_key(CAR_M, 3), 32, 64, 64, 2)
    # three-way among labels a multiple of the table size apart, and a fourth label that loses
    o = _object_of(rec, 128)
    m = _members(b, rec, mem, o)
    lab = np.repeat(np.array([5 + 2 * slots, 5, 5 + slots, 6], np.uint32), [42, 42, 42, 2])
    gt[m] = lab[rng.permutation(128)]
    expect[o] = (5, 42, 42, 0, 4)
    # two-way in the 40-member object, 0 against all ones
    o = _object_of(rec, 40)
    m = _members(b, rec, mem, o)
    gt[m] = np.where(np.arange(40) % 2 == 0, 0xFFFFFFFF, 0).astype(np.uint32)
    expect[o] = (0, 20, 20, 0, 2)
    # the winner first appears in the last, partial round: 64 members with a label each, then 36 with one
    o = _object_of(rec, 100)
    m = _members(b, rec, mem, o)
    gt[m] = np.concatenate([_key(40, 1) + np.arange(64) * 65536, np.full(36, _key(CAR_M, 2))]).astype(np.uint32)
    expect[o] = (_key(CAR_M, 2), 36, 36, 36, 65)
    # ... and as a tie of single members won by the very last one (member 129 of 129; 193 = 3 x 64 + 1): more labels than the wave's
    # table takes, so the tie rule of the fallback
    for n in (129, 193):
        o = _object_of(rec, n)
        m = _members(b, rec, mem, o)
        gt[m] = np.concatenate([1000 + rng.permutation(n - 1) * slots, [999]]).astype(np.uint32)
        expect[o] = (999, 1, 1, 0, n)
    # a three-way tie in the largest object, the smallest label last in the member list
    o = _object_of(rec, 4500)
    m = _members(b, rec, mem, o)
    gt[m] = np.repeat(np.array([_key(CAR_M, 9), _key(30, 1), _key(30, 0)], np.uint32), 1500)
    expect[o] = (_key(30, 0), 1500, 3000, 1500, 3)
    got, st = _truth(ctx, gt, len(rec))
    _check(b, rec, mem, gt, got, st, "ties")
    for o, (label, n_label, n_class, n_moving, n_distinct) in expect.items():
        r = got[o]
        assert (int(r["label"]), int(r["n_label"]), int(r["n_class"]), int(r["n_moving"]), int(r["n_distinct"])) == \
            (label, n_label, n_class, n_moving, n_distinct), (o, r)
    assert st[3] == 2


# ---- 3. the on-chip bound --------------------------------------------------------------------------------------------------------------------

def test_the_onchip_bound_and_the_fallback_counter(scvod, crafted):
    ctx, b, rec, mem = crafted
    L = otr_onchip()
    assert L + 1 < 4500, "the largest crafted object cannot pass the bound"
    o = _object_of(rec, 4500)
    m = _members(b, rec, mem, o)
    rng = np.random.default_rng(SEED + 3)
    counters = []
    for distinct in (L - 1, L, L + 1, 4500):
        gt = _background(b)
        for k in range(len(rec)):
            gt[_members(b, rec, mem, k)] = _key(CAR_M, k)
        # every label at least once, the rest drawn: the last new label may come in any round
        lab = np.concatenate([np.arange(distinct), rng.integers(0, distinct, 4500 - distinct)]).astype(np.uint32)
        gt[m] = (lab[rng.permutation(4500)] * np.uint32(2654435761)) ^ np.uint32(0x9E3779B9)     # spread over all 32 bits, still distinct
        got, st = _truth(ctx, gt, len(rec))
        want = _check(b, rec, mem, gt, got, st, f"{distinct} distinct labels")
        assert int(got[o]["n_distinct"]) == distinct == int(want[o]["n_distinct"])
        counters.append(st[3])
    assert counters == [0, 0, 1, 1]


# ---- 4. more spilled objects than the fallback has workgroups -----------------------------------------------------------------------------

def test_every_fallback_region_is_reused(scvod):
    import torch
    L = otr_onchip()
    per_scan = [n for n, _, _ in BLOCKS if n > L]
    copies = -(-65 // len(per_scan))                   # at least 65 spilled objects: 32 workgroups, every region used twice or more
    scan = _crafted_scan()
    x = np.ascontiguousarray(np.concatenate([scan] * copies), np.float32)
    offs = (np.arange(copies + 1) * len(scan)).astype(np.int32)
    poses, nxt = np.zeros((copies, 6), np.float32), np.full(copies, -1, np.int32)
    d = torch.from_numpy(x).cuda().contiguous()
    torch.cuda.synchronize()
    b = Batch(name="CRAFTEDxN", kind="K64", P=scvod.make_params("semantickitti"), d=d, x=x, offs=offs, poses=poses, nxt=nxt,
              T=_transforms(scvod, poses, nxt), n=copies, ext=None, dyn_from_solo=())
    ctx = _prepared(scvod, b)
    rec, _, mem, _ = _full(ctx, b, NO_TRACK)
    assert len(rec) == copies * len(BLOCKS)
    rng = np.random.default_rng(SEED + 4)
    gt = _background(b)
    big = 0
    for o in range(len(rec)):
        m = _members(b, rec, mem, o)
        if len(m) > L:                                   # all distinct; where that leaves room, but for one pair
            lab = rng.permutation(len(m)).astype(np.uint32) * np.uint32(2654435761) + np.uint32(o)
            if len(m) - 1 > L:
                lab[int(rng.integers(1, len(m)))] = lab[0]
            gt[m] = lab
            big += 1
        else:
            gt[m] = _key(CAR_M, o)
    assert big == copies * len(per_scan) > 64
    got, st = _truth(ctx, gt, len(rec))
    want = _check(b, rec, mem, gt, got, st, "many spilled objects")
    assert st[3] == big and set(want["n_label"][want["n_distinct"] > L].tolist()) == {1, 2}
    again, st2 = _truth(ctx, gt, len(rec))
    assert st2 == st and np.array_equal(again.view(np.uint8), got.view(np.uint8)), "two runs differ"
    ctx.close()


# ---- 5. / 6. / 7. class lists, the stats, a palette on the K64 scan -----------------------------------------------------------------------------

def test_class_lists_and_a_palette_on_the_k64_scan(scvod, crafted):
    ctx, b, rec, mem = crafted
    rng = np.random.default_rng(SEED + 5)
    palette = np.array([0, 40, 48, 70, _key(10, 1), _key(10, 2), _key(CAR_M, 1), _key(CAR_M, 2), _key(253, 1), _key(259, 3), _key(30, 1),
                        0xFFFFFFFF], np.uint32)
    assert len(palette) == 12
    gt = palette[rng.integers(0, 12, int(b.offs[-1]))]
    # neighbouring members share labels, as real ones do: runs of a label along the member list of the K64 scan's objects
    for o in np.flatnonzero(rec["scan"] == 3):
        m = _members(b, rec, mem, int(o))
        gt[m] = np.repeat(palette[rng.integers(0, 12, len(m) // 16 + 1)], 16)[:len(m)]
    sixteen = [0, 40, 48, 70, 10, 30, 252, 253, 259, 0xFFFF, 1, 2, 3, 4, 5, 6]
    for what, classes in (("default list", None), ("empty list", []), ("16 classes", sixteen), ("one class", [10])):
        par = None if classes is None else scvod.eval_params_default(dynamic_classes=classes)
        dyn = otr.DYNAMIC if classes is None else tuple(classes)
        got, st = _truth(ctx, gt, len(rec), par)
        want = _check(b, rec, mem, gt, got, st, what, dyn)
        if classes == []:
            assert st[4] == 0 == st[5] and not got["n_moving"].any()
        if classes is sixteen:
            assert st[4] == int(b.offs[-1]) and np.array_equal(got["n_moving"], rec["n_points"]), "every label of the palette is in the list"
        if classes is None:
            assert 0 < st[5] < st[4], "moving points inside and outside the objects"
            k64 = rec["scan"] == 3
            assert (want["n_distinct"][k64] > 1).any() and (want["n_class"][k64] > want["n_label"][k64]).any()
            # voxelsize is not read
            par = scvod.eval_params_default(voxelsize=-1.0)
            again, st2 = _truth(ctx, gt, len(rec), par)
            assert st2 == st and np.array_equal(again.view(np.uint8), got.view(np.uint8))
    par = scvod.eval_params_default(dynamic_classes=range(17))
    assert Tru(4).call(ctx, _dev(gt), par) == INVALID
    par = scvod.eval_params_default()
    par.n_dynamic_classes = -1
    assert Tru(4).call(ctx, _dev(gt), par) == INVALID


# ---- 8. capacity -------------------------------------------------------------------------------------------------------------------------------

def test_capacity_latch_and_guard_region(scvod, crafted):
    ctx, b, rec, mem = crafted
    k = len(rec)
    rng = np.random.default_rng(SEED + 8)
    gt = np.array([_key(CAR_M, 1), _key(CAR_M, 2), 40, 0], np.uint32)[rng.integers(0, 4, int(b.offs[-1]))]
    o = _object_of(rec, 300)                                     # one object for the fallback, behind most capacities
    gt[_members(b, rec, mem, o)] = np.arange(300, dtype=np.uint32) * 7
    full, st = _truth(ctx, gt, k)
    _check(b, rec, mem, gt, full, st, "full")
    assert st[3] == 1
    d_gt = _dev(gt)
    for cap in (k - 1, k // 2, 1, 0):
        t = Tru(cap)
        assert t.call(ctx, d_gt) == 0
        rc, got = _tstats(ctx)
        assert rc == CAPACITY and got == [cap, k, 1] + st[3:], (cap, rc, got)      # word 5 still sums over ALL objects
        with pytest.raises(scvod.ScvodError):
            ctx.batch_object_truth_stats()
        assert np.array_equal(t.host(), full[:cap].view(np.uint8)), cap          # (host() asserts the guard region)
        again, st2 = _truth(ctx, gt, k)                                           # the latch belongs to the LAST call
        assert st2 == st and np.array_equal(again.view(np.uint8), full.view(np.uint8))
    big = Tru(k + 37)                                                             # nothing behind the last record either
    assert big.call(ctx, d_gt) == 0 and _tstats(ctx) == (0, st)
    assert (big.host()[k * 32:] == FILL).all() and np.array_equal(big.host()[:k * 32], full.view(np.uint8))
    assert ctx.lib.scvod_batch_object_truth(ctx.h, None, None, C.c_void_p(big.buf.data_ptr()), k, None) == INVALID
    assert ctx.lib.scvod_batch_object_truth(ctx.h, C.c_void_p(d_gt.data_ptr()), None, None, k, None) == INVALID
    assert ctx.lib.scvod_batch_object_truth(ctx.h, C.c_void_p(d_gt.data_ptr()), None, C.c_void_p(big.buf.data_ptr()), -1, None) == INVALID
    assert ctx.lib.scvod_batch_object_truth(ctx.h, C.c_void_p(d_gt.data_ptr() + 2), None, C.c_void_p(big.buf.data_ptr()), k, None) == INVALID


# ---- 9. state ----------------------------------------------------------------------------------------------------------------------------------

def test_state_errors(scvod):
    import torch
    b = _batch(scvod, "K6")
    n = int(b.offs[-1])
    ctx = _new_ctx(scvod, [b])
    d_gt = _dev(np.zeros(n, np.uint32))
    t = Tru(n)
    cnt = Tab(b, 0, 0, members=False, points=False)
    tab = Tab(b, n, n)
    torch.cuda.synchronize()
    assert _tstats(ctx)[0] == STATE                                       # before the first call
    assert t.call(ctx, d_gt) == STATE                                     # no batch, no table
    assert ctx.batch_object_truth_scratch_bytes() == 0
    ctx.batch_process(b.d, b.offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    assert t.call(ctx, d_gt) == STATE                                     # a batch, but no table yet
    assert cnt.call(ctx, NO_TRACK, records=False) == 0
    assert t.call(ctx, d_gt) == STATE                                     # a count-only table is none
    assert _tstats(ctx)[0] == STATE
    assert tab.call(ctx, NO_TRACK) == 0 and t.call(ctx, d_gt) == 0 and _tstats(ctx)[0] == 0
    assert cnt.call(ctx, NO_TRACK, records=False) == 0 and t.call(ctx, d_gt) == 0   # a count-only call later leaves the lists as they are
    ctx.batch_cluster()                                                   # another clustering: the lists are stale
    assert t.call(ctx, d_gt) == STATE
    ctx.batch_cluster_types()
    assert t.call(ctx, d_gt) == STATE
    _track(ctx, b, b.T, b.nxt, None, 1)
    assert tab.call(ctx, 0) == 0 and t.call(ctx, d_gt) == 0               # a table that read the tracking result
    ctx.batch_cluster_types()                                             # ... which is stale now: the table's own rule
    assert tab.call(ctx, 0) == INVALID and t.call(ctx, d_gt) == INVALID
    assert tab.call(ctx, NO_TRACK) == 0 and t.call(ctx, d_gt) == 0
    ctx.batch_process(b.d, b.offs)                                        # a new batch
    assert t.call(ctx, d_gt) == STATE
    torch.cuda.synchronize()
    ctx.close()


# ---- 11. / 12. stream order, two runs -----------------------------------------------------------------------------------------------------------

def test_behind_the_whole_chain_on_a_side_stream_twice(scvod):
    import torch
    b = _batch(scvod, "D")
    n = int(b.offs[-1])
    rng = np.random.default_rng(SEED + 12)
    gt = np.array([_key(CAR_M, 1), _key(CAR_M, 2), _key(10, 1), 40, 70, 0], np.uint32)[rng.integers(0, 6, n)]
    d_gt = _dev(gt)
    stream = _stream()
    st = stream.cuda_stream
    runs = []
    for _ in range(2):
        ctx = _new_ctx(scvod, [b])
        tab, t = Tab(b, n, n), Tru(n // 8)
        torch.cuda.synchronize()
        offs_h, T, nxt = b.offs.copy(), b.T.copy(), b.nxt.copy()
        ctx.batch_process(b.d, offs_h, stream=st, sync=False)
        ctx.batch_cluster(stream=st, sync=False)
        ctx.batch_cluster_types(stream=st, sync=False)
        keep = _track(ctx, b, T, nxt, st, 0)
        assert tab.call(ctx, 0, st) == 0, ctx.lib.scvod_last_error(ctx.h)
        assert t.call(ctx, d_gt, None, st) == 0, ctx.lib.scvod_last_error(ctx.h)
        stream.synchronize()
        rc, stt = _tstats(ctx)
        rec, offs, mem, _ = tab.host(b)
        k = int(offs[-1])
        assert rc == 0 and 0 < k <= t.cap and stt[0] == stt[1] == k
        raw = t.host()
        assert (raw[k * 32:] == FILL).all(), "something was written behind the last record"
        got = raw[:k * 32].view(otr.DTYPE).copy()
        _check(b, rec[:k], mem, gt, got, stt, "on the side stream")
        assert (rec[:k]["dynamic"] == 1).any(), "a table that read the tracking result"
        fin = scvod.object_truth_finish(rec[:k], got)
        want = otr.finish(rec[:k], got)
        assert all(fin[key] == want[key] for key in otr.COUNTS) and fin["moving_objects"] + fin["static_objects"] == k
        runs.append(got)
        del keep
        ctx.close()
    assert np.array_equal(runs[0].view(np.uint8), runs[1].view(np.uint8)), "two runs differ"


# ---- 13. no side effects ---------------------------------------------------------------------------------------------------------------------

def test_the_call_changes_nothing_else(scvod):
    import torch
    b = _batch(scvod, "D")
    ctx = _tracked(scvod, b)
    table = _full(ctx, b)
    k = len(table[0])
    before_map = scvod.StaticMap(MAP_CELLS)
    before_map.accumulate(ctx, b.poses)
    want_all, _ = _everything(ctx, b, before_map)
    lab = _labels(ctx, b)
    arena, scratch = ctx.arena_bytes(), ctx.batch_objects_scratch_bytes()
    tab = Tab(b, int(b.offs[-1]), int(b.offs[-1]))
    torch.cuda.synchronize()
    assert tab.call(ctx) == 0
    torch.cuda.synchronize()
    raw = [x.cpu().numpy().copy() for x in (tab.rec, tab.offs, tab.mem, tab.pobj)]
    rng = np.random.default_rng(SEED + 13)
    gt = rng.integers(0, 1 << 32, int(b.offs[-1]), dtype=np.uint64).astype(np.uint32)      # any 32-bit value is a label
    one, st = _truth(ctx, gt, k)
    two, _ = _truth(ctx, gt, k)
    _check(b, table[0], table[2], gt, one, st, "random 32-bit labels")
    assert np.array_equal(one.view(np.uint8), two.view(np.uint8)), "two consecutive calls differ"
    for x, y in zip(raw, (tab.rec, tab.offs, tab.mem, tab.pobj)):
        assert np.array_equal(x, y.cpu().numpy()), "the table's buffers changed"
    assert ctx.arena_bytes() == arena
    assert ctx.batch_objects_scratch_bytes() == scratch, "the stage's scratch is its own"
    assert ctx.batch_object_truth_scratch_bytes() > 0
    assert np.array_equal(_labels(ctx, b), lab)
    after_map = scvod.StaticMap(MAP_CELLS)
    after_map.accumulate(ctx, b.poses)
    got_all, _ = _everything(ctx, b, after_map)
    _same(got_all, want_all, "fetches and map records after the truth call")
    for x, y in zip(_full(ctx, b), table):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    before_map.close()
    after_map.close()
    ctx.close()
