"""scvod_batch_object_tracks on the batches of the asynchronous chain's and the object table's tests (imported, not edited): the
sequential numpy tracker of tests/helpers/object_tracks_ref.py, fed from scvod_batch_fetch_track's pair tables and the fetched object
table, must equal the device output byte for byte; the same table through the device form, with candidate lists built from those
fetches, must equal the batch form; the state errors; and the call changes nothing else."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import object_tracks_ref as otr  # noqa: E402
from test_gpu_async_chain import _batch, _new_ctx, _track  # noqa: E402
from test_gpu_export import _labels, _step, _tracked  # noqa: E402
from test_gpu_objects import NO_TRACK, Tab, _full  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 8
STATE = -5


def _table(ctx, b, flags=0):
    """scvod_batch_objects with lists: (the device tensor of exactly the table's records, the records and the offsets on the host)"""
    import torch
    t = Tab(b, int(b.offs[-1]), int(b.offs[-1]))
    torch.cuda.synchronize()
    assert t.call(ctx, flags) == 0, ctx.lib.scvod_last_error(ctx.h)
    torch.cuda.synchronize()
    rec, offs, _, _ = t.host(b)
    n = int(offs[-1])
    return t.rec[:max(n, 1) * 64].view(max(n, 1), 64)[:n], rec[:n].copy(), offs.copy()


def _candidates(ctx, b, rec, offs):
    """the overlap candidates of every object from scvod_batch_fetch_track: the pairs of its root, every label mapped to the object of
    the successor scan with that name; a label that names no object of the table is left out"""
    index = {(int(r["scan"]), int(r["name"])): i for i, r in enumerate(rec)}
    per_object = [[] for _ in rec]
    for s in range(b.n):
        nx = int(b.nxt[s])
        if nx < 0:
            continue
        t = ctx.batch_fetch_track(s)
        for k, root in enumerate(t["cluster_root"]):
            a = index.get((s, int(root)))
            if a is None:
                continue
            for j in range(int(t["pair_begin"][k]), int(t["pair_begin"][k + 1])):
                o = index.get((nx, int(t["pair_label"][j])))
                if o is not None:
                    per_object[a].append((o, int(t["pair_count"][j])))
    cb = np.concatenate([[0], np.cumsum([len(c) for c in per_object])]).astype(np.int32)
    cand = np.asarray([p for c in per_object for p in c], np.int32).reshape(-1, 2)
    return cb, cand


def _check(got, ref, what):
    n_links, n_tracks, n_tobj = len(ref["links"]), len(ref["tracks"]), len(ref["track_objects"])
    exp = {"links": ref["links"].view(np.uint8).reshape(-1, 32), "tracks": ref["tracks"].view(np.uint8).reshape(-1, 64),
           "track_objects": ref["track_objects"].view(np.uint8).reshape(-1, 4),
           "n_tracks": np.asarray([ref["n_tracks"]], np.int32).view(np.uint8).reshape(-1, 4)}
    for w, e in exp.items():
        g = got[w].cpu().numpy()
        assert np.array_equal(g[:len(e)], e), f"{what}: {w} differ from the helper"
        assert (g[len(e):] == 0xA5).all(), f"{what}: {w}: something was written behind the last record"
    return n_links, n_tracks, n_tobj


@pytest.mark.parametrize("name", ["PARK", "B", "C", "K6"])
def test_batch_form_against_the_helper_and_the_device_form(scvod, name):
    import torch
    b = _batch(scvod, name)
    ctx = _tracked(scvod, b)
    d_rec, rec, offs = _table(ctx, b)
    labels0, arena0 = _labels(ctx, b), ctx.arena_bytes()
    cb, cand = _candidates(ctx, b, rec, offs)
    T = np.stack([scvod.pose_matrix(p) for p in b.poses])
    for prm in (dict(), dict(min_length=1, flags=otr.ANY_CLASS), dict(flags=otr.NO_GATE, min_length=3)):
        params = scvod.track_params_default(**prm)
        _, whole = ctx.batch_object_tracks(d_rec, b.poses, params, guard=GUARD, full=True)
        stats = ctx.object_tracks_stats()
        pd = dict(otr.DEFAULTS, **prm)
        pd["occupancy"] = float(b.P.occupancy)
        ref = otr.object_tracks_ref(rec, offs, b.nxt, T, cb, cand, pd)
        _check(whole, ref, f"{name} {prm}")
        assert stats == ref["stats"], (name, prm)
        # the same table through the device form, its candidates built from the fetches
        d_off = torch.from_numpy(offs).cuda()
        d_cb = torch.from_numpy(cb).cuda()
        d_cand = torch.from_numpy(cand).cuda() if len(cand) else None
        _, again = ctx.object_tracks_device(d_rec, d_off, b.n, b.nxt, b.poses, d_cb, d_cand, params, guard=GUARD, full=True)
        assert ctx.object_tracks_stats() == stats
        for w in whole:
            assert torch.equal(whole[w], again[w]), f"{name} {prm}: {w}: the device form differs from the batch form"
    first = otr.object_tracks_ref(rec, offs, b.nxt, T, cb, cand, dict(otr.DEFAULTS, occupancy=float(b.P.occupancy)))
    if name in ("PARK", "B"):
        assert first["stats"]["overlap_links"] > 0 and first["n_tracks"] > 0 and first["stats"]["longest"] >= 2
    if name == "B":                                                          # two interleaved chains: a link skips a scan
        linked = np.nonzero(first["links"]["pred"] >= 0)[0]
        assert (rec["scan"][linked] - rec["scan"][first["links"]["pred"][linked]] == 2).all()
    # nothing else moved: the table, the per-point labels, the arena
    d_rec2, rec2, offs2 = _table(ctx, b)
    assert rec2.tobytes() == rec.tobytes() and np.array_equal(offs2, offs)
    assert np.array_equal(_labels(ctx, b), labels0) and ctx.arena_bytes() == arena0
    assert ctx.object_tracks_scratch_bytes() > 0
    ctx.close()


def test_state_errors(scvod):
    import torch
    b = _batch(scvod, "K6")
    ctx = _new_ctx(scvod, [b])
    n = int(b.offs[-1])
    d_rec = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")

    def call():
        return ctx.lib.scvod_batch_object_tracks(ctx.h, C.c_void_p(d_rec.data_ptr()), None, None, None, n, None, n, None, None, None)
    assert call() == STATE                                   # nothing ran at all
    _step(ctx, b)
    assert call() == STATE                                   # tracked, but no table
    t = Tab(b, n, n, members=False, points=False)
    assert ctx.lib.scvod_batch_objects(ctx.h, 0, None, 0, C.c_void_p(t.offs.data_ptr()), None, 0, None, None) == 0
    assert call() == STATE                                   # a count-only call leaves no table
    _full(ctx, b, NO_TRACK)
    assert call() == STATE                                   # a SCVOD_OBJ_NO_TRACK table
    _full(ctx, b)
    assert call() == 0
    torch.cuda.synchronize()
    ctx.batch_cluster()                                      # a new clustering: the tracking result and the table are stale
    ctx.batch_cluster_types()
    assert call() == STATE
    _track(ctx, b, b.T, b.nxt, None, 1)
    assert call() == STATE                                   # tracked again, but the table still belongs to the old clustering
    _full(ctx, b)
    assert call() == 0
    st = np.zeros(8, np.int64)
    assert ctx.lib.scvod_object_tracks_stats(ctx.h, st.ctypes.data_as(C.c_void_p)) == 0 and st[0] > 0
    ctx.close()
