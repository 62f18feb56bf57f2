#!/usr/bin/env python3
"""Development tool: what linking the table's objects into tracks costs on the bench-shaped jobs -- scvod_batch_object_tracks
(csrc/scvod_tracks.hip) next to scvod_batch_object_shapes of the same table, both behind a tracked step and an object table with records
and members.  Timed with stream events after a warm-up call each, the two calls taking turns inside every round (one process,
interleaved), medians of the rounds.  Also what the stage found: tracks, longest track, links by kind, refused proposals, and
scvod_tracks_finish at min_travel 2.0 -- an observation on synthetic scenes, with the untuned default gate and size ratio.
Writes profiles/object_tracks_cost.txt (after every job, so a run that is cut short leaves what it measured).
usage: python tools/object_tracks_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--rounds 7] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scvod_py
import synth
from object_truth_cost import interleaved
from objects_cost import JOBS

MIN_TRAVEL = 2.0


def run(kind, scale, rounds):
    preset, seq, count, skip = JOBS[kind]
    count = max(skip + 1, int(count * scale))
    P = scvod_py.make_params(preset)
    scans = [synth.make_scan(seq, i, kind, device="cuda") for i in range(count)]
    d = torch.cat([s[0] for s in scans]).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(s[0]) for s in scans])]).astype(np.int32)
    poses = np.asarray([s[2] for s in scans], np.float32)
    del scans
    n = int(offs[-1])
    print(f"{kind}: {count} scans, {n} points", file=sys.stderr, flush=True)
    ctx = scvod_py.Ctx(P, max_points_total=n + 64, max_scans=count)
    nxt = np.asarray([s + skip if s + skip < count else -1 for s in range(count)], np.int32)
    T = np.zeros((count, 12), np.float32)
    for s in range(count):
        if nxt[s] >= 0:
            T[s] = ctx.pose_delta(poses[s], poses[nxt[s]])
    st = torch.cuda.current_stream().cuda_stream
    ctx.batch_process(d, offs, stream=st, sync=False)
    ctx.batch_cluster(stream=st, sync=False)
    ctx.batch_cluster_types(stream=st, sync=False)
    ctx.batch_track(T, next_scan=nxt, stream=st, sync=False)
    d_off = torch.empty(count + 1, dtype=torch.int32, device="cuda")
    ctx.batch_objects(d_off, None, stream=st)
    s0 = ctx.batch_objects_stats()
    k, m = s0["objects"], s0["members"]
    rec = torch.empty((max(k, 1), 64), dtype=torch.uint8, device="cuda")[:k]
    mem = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
    shp = torch.empty((max(k, 1), 96), dtype=torch.uint8, device="cuda")
    ctx.batch_objects(d_off, rec, d_member_src=mem, stream=st)
    lnk = torch.empty((max(k, 1), 32), dtype=torch.uint8, device="cuda")
    trk = torch.empty((max(k, 1), 64), dtype=torch.uint8, device="cuda")
    tob = torch.empty(max(k, 1), dtype=torch.int32, device="cuda")
    ntr = torch.empty(1, dtype=torch.int32, device="cuda")

    def tracks():   # the C entry point with buffers made once: no allocation inside the timed call
        ctx._chk(ctx.lib.scvod_batch_object_tracks(ctx.h, rec.data_ptr(), poses.ctypes.data, None, lnk.data_ptr(), k, trk.data_ptr(), k,
                                                   tob.data_ptr(), ntr.data_ptr(), st))

    t = interleaved({"shapes": lambda: ctx.batch_object_shapes(shp, stream=st), "tracks": tracks}, rounds)
    out = dict(kind=kind, scans=count, successor_stride=skip, points=n, objects=k, members=m)
    for name, (med, lo, hi) in t.items():
        out[name] = dict(ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3))
    out["ratio"] = round(out["tracks"]["ms"] / out["shapes"]["ms"], 3)
    tracks()
    out["stats"] = ctx.object_tracks_stats()
    found = out["stats"]["tracks"]
    assert int(ntr.cpu()[0]) == found == out["stats"]["written"]
    h = trk.cpu().numpy().reshape(-1).view(scvod_py.TRACK_DTYPE)[:found]
    out["finish"] = scvod_py.tracks_finish(h, MIN_TRAVEL)
    out["cars"] = int((rec.cpu().numpy().reshape(-1).view(scvod_py.OBJECT_DTYPE)["cls"] == 2).sum())
    out["scratch_bytes"] = ctx.object_tracks_scratch_bytes()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_tracks_cost.txt"))
    a = ap.parse_args()
    scvod_py.load_lib()
    lines = ["Object tracks (scvod_batch_object_tracks, csrc/scvod_tracks.hip): cost and yield on the bench-shaped jobs", "=" * 110, "",
             f"python tools/object_tracks_cost.py --jobs {a.jobs} --scale {a.scale} --rounds {a.rounds} on {torch.cuda.get_device_name(0)}: ms per "
             "call from stream events,", f"median (min .. max) of {a.rounds} rounds in which the two calls take turns, after one warm-up call "
             "each; links, tracks, the track-object list", "and the count are all written.  Default parameters: gate 2.0 m, size_ratio 1.5, "
             "min_points 10, min_length 2 -- this project's values, untuned, NOT from real data.", ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for kind in a.jobs.split(","):
        r = run(kind, a.scale, a.rounds)
        print(json.dumps(r), flush=True)
        f = lambda c: f"{r[c]['ms']:.3f} ({r[c]['ms_min']:.3f} .. {r[c]['ms_max']:.3f})"  # noqa: E731
        s, fin = r["stats"], r["finish"]
        lines += [f"{kind}: {r['scans']} scans (successor s + {r['successor_stride']}), {r['points']} points, {r['objects']} objects of which "
                  f"{r['cars']} cars, scratch {r['scratch_bytes']} bytes",
                  f"  scvod_batch_object_shapes   {f('shapes')}",
                  f"  scvod_batch_object_tracks   {f('tracks')}   = {r['ratio']:.3f} x shapes",
                  f"  tracks {s['tracks']}, longest {s['longest']}, overlap links {s['overlap_links']}, gate links {s['gate_links']}, proposals "
                  f"refused {s['refused']}",
                  f"  scvod_tracks_finish(min_travel {MIN_TRAVEL}): moving {fin['moving_tracks']} tracks / {fin['moving_members']} members / "
                  f"{fin['moving_members_dynamic']} dynamic, still {fin['still_tracks']} / {fin['still_members']} / "
                  f"{fin['still_members_dynamic']}, recall_along {fin['recall_along']:.2f} %, false_alarm {fin['false_alarm']:.2f} %", ""]
        with open(a.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
