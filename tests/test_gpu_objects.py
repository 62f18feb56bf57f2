"""scvod_batch_objects / scvod_batch_objects_stats on the device, all through the C-ABI: the object table, its offsets, the member
list and the per-input-point object index against the numpy statement of the table (tests/helpers/objects_ref.py, fed from the
existing per-scan fetches of the same ctx) and against the table the helper builds from the oracle's stages alone.  Every comparison
is np.array_equal / bit for bit on the raw record bytes.

The oracle's chain reports per-point tracking bytes, not Cluster::state: against the oracle every field but `state` is compared (and
`state == 1` exactly where `dynamic == 1`); against the helper fed from scvod_batch_fetch_track the whole record is."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import objects_ref as obr  # noqa: E402
import point_labels_ref as plr  # noqa: E402
from test_capi_objects import oracle_stages, oracle_table  # noqa: E402
from test_gpu_async_chain import MERGE, _batch, _everything, _new_ctx, _same, _stream, _track  # noqa: E402
from test_gpu_export import _labels, _step, _tracked  # noqa: E402

pytestmark = pytest.mark.gpu

CAR, OTHER = 2, 1
GUARD = 64
NO_TRACK = 1


@pytest.fixture(scope="module")
def objlib(tmp_path_factory):
    return obr.build(tmp_path_factory.mktemp("objref"))


class Tab:
    """output buffers of one scvod_batch_objects call with a guard region behind every capacity"""

    def __init__(self, b, cap_obj, cap_mem, members=True, points=True):
        import torch
        self.cap_obj, self.cap_mem, self.n = cap_obj, cap_mem, int(b.offs[-1])
        self.rec = torch.full(((cap_obj + GUARD) * 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.offs = torch.full((b.n + 1 + GUARD,), -7, dtype=torch.int32, device="cuda")
        self.mem = torch.full((cap_mem + GUARD,), -7, dtype=torch.int32, device="cuda") if members else None
        self.pobj = torch.full((self.n + GUARD,), -7, dtype=torch.int32, device="cuda") if points else None

    def call(self, ctx, flags=0, stream=None, records=True):
        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        return ctx.lib.scvod_batch_objects(ctx.h, int(flags), ptr(self.rec) if records else None, int(self.cap_obj), ptr(self.offs),
                                           ptr(self.mem), int(self.cap_mem), ptr(self.pobj), C.c_void_p(stream or 0))

    def host(self, b):
        """(records [cap_obj], offsets, members [cap_mem] or None, per-point object or None); asserts the guard regions"""
        offs = self.offs.cpu().numpy()
        assert (offs[b.n + 1:] == -7).all(), "the offsets were written behind n_scans + 1"
        raw = self.rec.cpu().numpy()
        assert (raw[self.cap_obj * 64:] == 0xA5).all(), "records were written at or behind cap_objects"
        mem = pobj = None
        if self.mem is not None:
            mem = self.mem.cpu().numpy()
            assert (mem[self.cap_mem:] == -7).all(), "members were written at or behind cap_members"
            mem = mem[:self.cap_mem]
        if self.pobj is not None:
            pobj = self.pobj.cpu().numpy()
            assert (pobj[self.n:] == -7).all(), "the per-point objects were written behind the batch's points"
            pobj = pobj[:self.n]
        return raw[:self.cap_obj * 64].view(obr.OBJECT_DTYPE), offs[:b.n + 1], mem, pobj


def _stats(ctx):
    out = np.zeros(4, np.int64)
    rc = ctx.lib.scvod_batch_objects_stats(ctx.h, out.ctypes.data_as(C.c_void_p))
    return rc, out.tolist()


def _helper_table(ctx, b, objlib, track=True):
    """the helper fed from the per-scan fetches of the ctx: (records, offsets, members, per-point object), and what was fetched"""
    per_scan, fetched = [], []
    for s in range(b.n):
        r = ctx.batch_fetch(s)
        n = r["n_apri"]
        cl = ctx.batch_fetch_clusters(s, n)
        ty = ctx.batch_fetch_cluster_types(s, n, car_label=CAR, other_label=OTHER)
        cls = ctx.batch_fetch_cluster_classes(s, n, car_label=2, building_label=3, tree_label=1)
        dyn = state = None
        if track:
            t = ctx.batch_fetch_track(s)
            dyn = t["pt_dyn"]
            state = {int(a): int(v) for a, v in zip(t["cluster_root"], t["cluster_state"])}
        rec, mem, po = obr.scan_objects(objlib, s, r["apri"], cl, ty, classes=cls, pt_dyn=dyn, car_state=state, car=CAR)
        per_scan.append((rec,) + obr.to_input(r["n_points"], r["apri_src"], mem, po))
        fetched.append(dict(r=r, cl=cl, ty=ty))
    return obr.batch_table(per_scan), fetched


def _full(ctx, b, flags=0, stream=None):
    """one call with buffers that hold everything (sized by the batch's points), synchronised"""
    import torch
    t = Tab(b, int(b.offs[-1]), int(b.offs[-1]))
    torch.cuda.synchronize()
    assert t.call(ctx, flags, stream) == 0, ctx.lib.scvod_last_error(ctx.h)
    rc, st = _stats(ctx)
    rec, offs, mem, pobj = t.host(b)
    assert rc == 0 and st[0] == st[1] == offs[-1] and st[3] == 0
    raw = t.rec.cpu().numpy()
    assert (raw[st[1] * 64:] == 0xA5).all() and (mem[st[2]:] == -7).all(), "something was written behind the last record / member"
    return rec[:st[1]], offs, mem[:st[2]], pobj


def _equal(got, want, what):
    for k, name in enumerate(("records", "offsets", "members", "point objects")):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape, f"{what}: {name}: {g.shape} != {w.shape}"
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"{what}: {name} differ from the helper"


# ---- 1. the table against the helper ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "PARK", "OS128", "C"])
def test_table_against_the_helper(scvod, objlib, name):
    b = _batch(scvod, name)
    ctx = _new_ctx(scvod, [b])
    ctx.batch_process(b.d, b.offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    # before any tracking: the clustering and the types suffice with SCVOD_OBJ_NO_TRACK
    want0, _ = _helper_table(ctx, b, objlib, track=False)
    got0 = _full(ctx, b, NO_TRACK)
    _equal(got0, want0, f"{name} NO_TRACK")
    assert (got0[0]["state"] == -1).all() and (got0[0]["dynamic"] == 0).all()
    _track(ctx, b, b.T, b.nxt, None, 1)
    want, fetched = _helper_table(ctx, b, objlib)
    got = _full(ctx, b)
    _equal(got, want, name)
    _equal(_full(ctx, b, NO_TRACK), want0, f"{name} NO_TRACK after the tracking")
    rec, offs, mem, pobj = got
    assert len(rec) > 0 and (rec["cls"] == 2).any() and (rec["cls"] == 1).any()
    if name != "OS128":                              # (five scans: the other batches are the ones the export's tests know to hold dynamic points)
        assert (rec["dynamic"] == 1).any()
    assert np.array_equal(rec["point_begin"], np.concatenate([[0], np.cumsum(rec["n_points"])[:-1]]))
    # the per-point object composed with the table reproduces pt_cluster through apri_src
    lab = _labels(ctx, b)
    for s, f in enumerate(fetched):
        po = pobj[b.offs[s]:b.offs[s + 1]][f["r"]["apri_src"]]
        kept = f["ty"] != -1
        assert (po[~kept] == -1).all() and ((po[kept] >= offs[s]) & (po[kept] < offs[s + 1])).all()
        assert np.array_equal(rec["name"][po[kept]], f["cl"][kept]) and (rec["scan"][po[kept]] == s).all()
    # the labels' STATIC_OTHER / STATIC_CAR / DYNAMIC points are exactly those of an object, DYNAMIC those of a dynamic one
    in_obj = np.isin(lab, (plr.PT_STATIC_OTHER, plr.PT_STATIC_CAR, plr.PT_DYNAMIC))
    assert np.array_equal(in_obj, pobj >= 0)
    assert np.array_equal(lab == plr.PT_DYNAMIC, (pobj >= 0) & (rec["dynamic"][np.maximum(pobj, 0)] == 1))
    # the shim's form
    import torch
    d_off = torch.zeros(b.n + 1, dtype=torch.int32, device="cuda")
    d_rec = torch.zeros((len(rec), 64), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.batch_objects(d_off, d_rec)
    assert ctx.batch_objects_stats() == dict(written=len(rec), objects=len(rec), members=len(mem), overflow=False)
    assert np.array_equal(d_rec.cpu().numpy().reshape(-1).view(scvod.OBJECT_DTYPE).view(np.uint8), rec.view(np.uint8))
    ctx.close()


# ---- 2. the table against the oracle ---------------------------------------------------------------------------------------------------

def test_table_against_the_oracle(scvod, oracle, objlib):
    b = _batch(scvod, "K6")                          # synth.make_scan(5, 300 + 5 k, "K64"), k < 6: the scans of test_capi_objects.py
    ctx = _tracked(scvod, b)
    rec, offs, mem, pobj = _full(ctx, b)
    # Patchwork's canonical order (ties on z by input index), the one the device implements and test_gpu_parity.py compares with: the
    # reference's std::sort leaves the order of equal z, hence the order of an object's members, to the implementation
    res, names, types, dyn = oracle_stages(oracle, b.P, b.x, b.offs, b.poses, sort_mode=1)
    want, w_offs, w_mem, w_pobj = oracle_table(objlib, res, names, types, dyn)
    assert np.array_equal(offs, w_offs), "offsets"
    assert np.array_equal(mem, w_mem), "member list"
    assert np.array_equal(pobj, w_pobj), "per-point object"
    assert (rec["state"] == 1).tolist() == (rec["dynamic"] == 1).tolist()
    last = rec["scan"] == b.n - 1                    # (the last scan has no successor: the oracle's chain says nothing about it)
    assert (rec["dynamic"][last] == 0).all()
    got = rec.copy()
    got["state"] = -1
    want = want.copy()
    want["dynamic"][last] = 0
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), "the device table differs from the table built from the oracle's stages"
    assert (rec["cls"] == 2).any() and (rec["cls"] == 1).any() and (rec["dynamic"] == 1).any()
    assert sum(int((t[np.nonzero(c == np.arange(len(c)))[0]] == -1).any()) for t, c in zip(types, names)) > 0
    ctx.close()


# ---- 3. the opt-in stages --------------------------------------------------------------------------------------------------------------

def test_table_follows_the_merge_and_the_region_growing_and_forgets_them_again(scvod, objlib):
    b = _batch(scvod, "D")
    ctx = _tracked(scvod, b)
    first = _full(ctx, b)
    ctx.set_intensity_merge(*MERGE)
    ctx.set_region_growing(True)
    _step(ctx, b)
    assert ctx.batch_cluster_merge_stats()["fusions"] > 0
    want, _ = _helper_table(ctx, b, objlib)          # (the fetches report the fused partition and the region growing's classes)
    got = _full(ctx, b)
    _equal(got, want, "merge + region growing")
    assert len(got[0]) < len(first[0]), "the merge fused no object: the case shows nothing"
    ctx.set_intensity_merge(0, MERGE[1], MERGE[2], MERGE[3])
    ctx.set_region_growing(False)
    _step(ctx, b)
    _equal(_full(ctx, b), first, "both stages off again")
    ctx.close()
    r3 = _batch(scvod, "R3")
    ctx = _tracked(scvod, r3, setup=lambda c: c.set_region_growing(True))
    want, _ = _helper_table(ctx, r3, objlib)
    got = _full(ctx, r3)
    _equal(got, want, "region growing")
    assert (got[0]["cls"] == 3).any(), "no building: the case shows nothing"
    for s in range(r3.n):
        n = ctx.batch_fetch(s)["n_apri"]
        cls = ctx.batch_fetch_cluster_classes(s, n, car_label=2, building_label=3, tree_label=1)
        rs = got[0][got[1][s]:got[1][s + 1]]
        assert np.array_equal(rs["cls"], cls[rs["name"]])
    ctx.close()


# ---- 4. no side effects ----------------------------------------------------------------------------------------------------------------

def test_the_table_changes_nothing_else(scvod):
    import torch
    b = _batch(scvod, "D")
    fresh = _tracked(scvod, b)                       # never asks for the table
    want_all, _ = _everything(fresh, b)
    assert fresh.batch_objects_scratch_bytes() == 0
    fresh.close()
    ctx = _tracked(scvod, b)
    arena = ctx.arena_bytes()
    assert ctx.batch_objects_scratch_bytes() == 0, "scratch before the first call"
    cnt = Tab(b, 0, 0, members=False, points=False)
    torch.cuda.synchronize()
    assert cnt.call(ctx, records=False) == 0
    assert 0 < ctx.batch_objects_scratch_bytes() < (1 << 20), "a count-only call allocates the small tables only"
    one = _full(ctx, b)
    two = _full(ctx, b)
    for x, y in zip(one, two):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), "two consecutive calls differ"
    _full(ctx, b, NO_TRACK)
    assert ctx.arena_bytes() == arena, "the table's scratch is not part of the arena"
    assert ctx.batch_objects_scratch_bytes() >= 28 * int(b.offs[-1])
    got_all, _ = _everything(ctx, b)
    _same(got_all, want_all, "fetches after the object table")
    ctx.close()


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------------------

def test_capacity_latch_and_guard_regions(scvod):
    import torch
    b = _batch(scvod, "K6")
    ctx = _tracked(scvod, b)
    rec, offs, mem, pobj = _full(ctx, b)
    k, m = len(rec), len(mem)
    assert k > 2 and m > k
    cnt = Tab(b, 0, 0, members=False, points=False)
    torch.cuda.synchronize()
    assert cnt.call(ctx, records=False) == 0
    assert _stats(ctx) == (0, [0, k, m, 0])
    assert np.array_equal(cnt.host(b)[1], offs) and (cnt.rec.cpu().numpy() == 0xA5).all()
    for cap_obj, cap_mem in ((k - 1, m), (k // 2, m), (0, m), (k, m - 1), (k, m // 2), (k, 0), (k - 1, m - 1), (0, 0)):
        t = Tab(b, cap_obj, cap_mem)
        torch.cuda.synchronize()
        assert t.call(ctx) == 0
        rc, st = _stats(ctx)
        assert rc == -4 and st == [cap_obj, k, m, 1], (cap_obj, cap_mem, rc, st)
        with pytest.raises(scvod.ScvodError):
            ctx.batch_objects_stats()
        s_rec, s_offs, s_mem, s_pobj = t.host(b)                       # (asserts the guard regions)
        assert np.array_equal(s_offs, offs), "the offsets must hold the true sizes"
        assert np.array_equal(s_rec.view(np.uint8), rec[:cap_obj].view(np.uint8)) and np.array_equal(s_mem, mem[:cap_mem])
        assert np.array_equal(s_pobj, pobj)
        # the latch belongs to the LAST call
        _full(ctx, b)
    ctx.close()


# ---- 6. stream order -------------------------------------------------------------------------------------------------------------------

def test_the_table_behind_the_tracking_on_a_side_stream_across_two_batches(scvod):
    import torch
    b1, b2 = _batch(scvod, "D"), _batch(scvod, "B")
    want = []
    for b in (b1, b2):
        solo = _tracked(scvod, b)
        want.append(_full(solo, b))
        solo.close()
    stream = _stream()
    st = stream.cuda_stream
    ctx = _new_ctx(scvod, [b1, b2])
    tabs = [Tab(b, int(b.offs[-1]), int(b.offs[-1])) for b in (b1, b2)]
    torch.cuda.synchronize()
    keep = []
    for b, t in zip((b1, b2), tabs):
        offs_h, T, nxt = b.offs.copy(), b.T.copy(), b.nxt.copy()
        ctx.batch_process(b.d, offs_h, stream=st, sync=False)
        ctx.batch_cluster(stream=st, sync=False)
        ctx.batch_cluster_types(stream=st, sync=False)
        keep.append(_track(ctx, b, T, nxt, st, 0))
        assert t.call(ctx, 0, st) == 0, ctx.lib.scvod_last_error(ctx.h)
    stream.synchronize()
    rc, stt = _stats(ctx)
    assert rc == 0 and stt[1] == len(want[1][0]) and stt[2] == len(want[1][2])
    for b, t, w in zip((b1, b2), tabs, want):
        rec, offs, mem, pobj = t.host(b)
        k, m = len(w[0]), len(w[2])
        _equal((rec[:k], offs, mem[:m], pobj), w, f"{b.name} on the side stream")
        assert (t.rec.cpu().numpy()[k * 64:] == 0xA5).all() and (mem[m:] == -7).all()
    ctx.close()


# ---- 7. state errors -------------------------------------------------------------------------------------------------------------------

def test_state_errors_are_those_of_the_point_labels(scvod):
    import torch
    b = _batch(scvod, "K6")
    n = int(b.offs[-1])
    ctx = _new_ctx(scvod, [b])
    t = Tab(b, n, n)
    lab = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def both(flags_obj, flags_lab):
        a = t.call(ctx, flags_obj)
        c = ctx.lib.scvod_batch_point_labels(ctx.h, C.c_void_p(lab.data_ptr()), n, flags_lab, None)
        assert a == c, (a, c)
        return a

    assert _stats(ctx)[0] == -5                       # before the first call
    assert both(0, 0) == -5 and both(NO_TRACK, 4) == -5            # no batch
    ctx.batch_process(b.d, b.offs)
    assert both(0, 0) == -5 and both(NO_TRACK, 4) == -5            # before the clustering
    ctx.batch_cluster()
    assert both(0, 0) == -5 and both(NO_TRACK, 4) == -5            # before the types
    ctx.batch_cluster_types()
    assert both(0, 0) == -1 and both(NO_TRACK, 4) == 0             # no tracking result
    assert t.call(ctx, 2) == -1 and t.call(ctx, NO_TRACK | 4) == -1   # unknown flag bits
    assert ctx.lib.scvod_batch_objects(ctx.h, 0, None, -1, C.c_void_p(t.offs.data_ptr()), None, 0, None, None) == -1
    assert ctx.lib.scvod_batch_objects(ctx.h, 0, None, 0, None, None, 0, None, None) == -1
    _track(ctx, b, b.T, b.nxt, None, 1)
    assert both(0, 0) == 0 and both(NO_TRACK, 4) == 0
    ctx.batch_cluster_types()                                       # the tracking result is stale now
    assert both(0, 0) == -1 and both(NO_TRACK, 4) == 0
    torch.cuda.synchronize()
    ctx.close()
