"""The whole seen-through recipe on the batches of the asynchronous chain's tests (imported, not edited): scvod_batch_visibility ->
scvod_batch_track -> scvod_batch_objects -> scvod_batch_object_visibility -> scvod_batch_object_tracks -> scvod_track_visibility_device,
one stream, no host read in between.  The last stage must equal the numpy statement of its rule (tests/helpers/track_visibility_ref.py),
fed with what the stages before it wrote, byte for byte; with parameters under which no track gives a verdict its output is its input.
Nothing is asserted about how good the verdict is."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import object_tracks_ref as otr  # noqa: E402
import track_visibility_ref as tvr  # noqa: E402
from test_gpu_async_chain import _batch  # noqa: E402
from test_gpu_export import _tracked  # noqa: E402
from test_gpu_objects import Tab  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4
CASES = (dict(), dict(flags=tvr.CLEAR), dict(window=2, min_travel=1.0, flags=tvr.CLEAR), dict(flags=tvr.NO_DYNAMIC, min_flagged=1, vote_num=1, vote_den=4),
         dict(min_length=3, min_travel=0.5, min_moved=2))


@pytest.mark.parametrize("name", ["PARK", "B", "C", "K6"])        # B: two interleaved chains in the successor table
def test_the_recipe_against_the_helper(scvod, name):
    import torch
    b = _batch(scvod, name)
    ctx = _tracked(scvod, b)
    n_pts = int(b.offs[-1])
    t = Tab(b, n_pts, n_pts)
    torch.cuda.synchronize()
    assert t.call(ctx, 0) == 0, ctx.lib.scvod_last_error(ctx.h)
    torch.cuda.synchronize()
    rec, offs, _, pobj = t.host(b)
    k = int(offs[-1])
    assert k > 0
    d_rec, d_off, d_po = t.rec[:k * 64].view(k, 64), t.offs[:b.n + 1], t.pobj[:n_pts]
    # the recipe of the README: every call enqueued, nothing read until the end
    out = ctx.batch_visibility(b.poses, b.nxt)
    obj = ctx.batch_object_visibility(out["verdict"], out["votes"], d_rec, cap=k)
    trk = ctx.batch_object_tracks(d_rec, b.poses)
    fin, whole = ctx.track_visibility(d_rec, d_off, b.n, b.poses, trk, d_po, obj["verdict"], d_object_vis=obj["records"], guard=GUARD, full=True)
    torch.cuda.synchronize()
    host = dict(links=trk["links"].cpu().numpy().reshape(-1).view(otr.LINK_DTYPE), tracks=trk["tracks"].cpu().numpy().reshape(-1).view(otr.TRACK_DTYPE),
                tobj=trk["track_objects"].cpu().numpy().reshape(-1).view(np.int32), n_tracks=int(trk["n_tracks"].cpu().numpy().reshape(-1).view(np.int32)[0]),
                vis=obj["records"].cpu().numpy().reshape(-1).view(tvr.OBJECT_VIS_DTYPE), vin=obj["verdict"].cpu().numpy())
    T = np.stack([scvod.pose_matrix(p) for p in b.poses])
    with np.errstate(all="ignore"):
        centres = otr.world_centres(rec[:k], T)            # computed once, shared by every comparison below
    assert 0 <= host["n_tracks"] <= k and len(host["vin"]) == n_pts == len(pobj)

    def check(prm, fin, whole, vin, in_place=False):
        ref = tvr.track_visibility_ref(rec[:k], offs, T, host["links"], host["tracks"], host["tobj"], host["n_tracks"], dict(tvr.DEFAULTS, **prm),
                                       object_vis=host["vis"], point_object=pobj, verdict=vin, centres=centres)
        assert ctx.track_visibility_stats() == ref["stats"], (name, prm)
        assert ref["stats"]["latch"] == 0 and ref["stats"]["objects"] == k
        got = fin["verdict"].cpu().numpy()
        assert np.array_equal(got, ref["verdict"]), f"{name} {prm}: the verdict bytes differ from the helper"
        tv, ov = whole["track_votes"].cpu().numpy(), whole["object_votes"].cpu().numpy()
        nt = host["n_tracks"]
        assert np.array_equal(tv[GUARD:GUARD + nt], ref["track_votes"].view(np.uint8).reshape(-1, 32)), f"{name} {prm}: track votes"
        assert (tv[:GUARD] == 0xA5).all() and (tv[GUARD + nt:] == 0xA5).all()
        assert np.array_equal(ov[GUARD:GUARD + k], ref["object_votes"].view(np.uint8).reshape(-1, 16)), f"{name} {prm}: object votes"
        assert (ov[:GUARD] == 0xA5).all() and (ov[GUARD + k:] == 0xA5).all()
        if not in_place:
            w = whole["verdict"].cpu().numpy()
            assert (w[:16 * GUARD] == 0xA5).all() and (w[16 * GUARD + n_pts:] == 0xA5).all()
        return ref

    check(dict(), fin, whole, host["vin"])
    said = 0
    for prm in CASES[1:]:
        fin, whole = ctx.track_visibility(d_rec, d_off, b.n, b.poses, trk, d_po, obj["verdict"], d_object_vis=obj["records"],
                                          params=scvod.track_visibility_params_default(**prm), guard=GUARD, full=True)
        ref = check(prm, fin, whole, host["vin"])
        said += int((ref["object_votes"]["verdict"] >= 0).sum())
    if name in ("PARK", "B"):
        assert host["n_tracks"] > 0 and said > 0
    assert np.array_equal(obj["verdict"].cpu().numpy(), host["vin"]), "the input bytes changed"
    # no track gives a verdict: the output is the input
    fin = ctx.track_visibility(d_rec, d_off, b.n, b.poses, trk, d_po, obj["verdict"], d_object_vis=obj["records"],
                               params=scvod.track_visibility_params_default(min_length=1 << 30, flags=tvr.CLEAR))
    assert torch.equal(fin["verdict"], obj["verdict"])
    st = ctx.track_visibility_stats()
    assert st["to_seen_through"] == st["to_keep"] == st["members_motion"] == st["members_cleared"] == st["tracks_voted"] == 0
    # in place, on a copy of the bytes; and without the objects' records
    for with_vis in (True, False):
        mine = obj["verdict"].clone()
        prm = dict(flags=tvr.CLEAR, window=1)
        fin, whole = ctx.track_visibility(d_rec, d_off, b.n, b.poses, trk, d_po, mine, d_object_vis=obj["records"] if with_vis else None,
                                          params=scvod.track_visibility_params_default(**prm), in_place=True, guard=GUARD, full=True)
        assert fin["verdict"].data_ptr() == mine.data_ptr()
        if with_vis:
            check(prm, fin, whole, host["vin"], in_place=True)
        else:
            ref = tvr.track_visibility_ref(rec[:k], offs, T, host["links"], host["tracks"], host["tobj"], host["n_tracks"], dict(tvr.DEFAULTS, **prm),
                                           point_object=pobj, verdict=host["vin"], centres=centres)
            assert ctx.track_visibility_stats() == ref["stats"] and np.array_equal(mine.cpu().numpy(), ref["verdict"])
    assert ctx.track_visibility_scratch_bytes() > 0
    ctx.close()
