#!/usr/bin/env python3
"""Development tool: what the object table costs on the bench-shaped jobs -- scvod_batch_objects (csrc/scvod_objects.hip) after a
tracked step, timed with stream events after a warm-up, next to the plain step (process -> cluster -> types -> track) of the same
run.  The cases add one output at a time, so their differences attribute the time: count only (the tile counts and the two scans),
members only (+ object indices, keys, the radix sort, the run starts), records (+ the voxel counts and the one-wave-per-object
reduction), everything.  Per-kernel times come from a run of this tool under rocprofv3 --kernel-trace --stats.
usage: python tools/objects_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
import scvod_py
import synth

JOBS = {"K64": ("semantickitti", 5, 2761, 5), "PARK": ("parkinglot", 3, 2000, 1), "OS128": ("os128_fine", 5, 1000, 5)}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def run(kind, scale, reps):
    preset, seq, count, skip = JOBS[kind]
    count = max(skip + 1, int(count * scale))
    P = scvod_py.make_params(preset)
    scans = [synth.make_scan(seq, i, kind, device="cuda") for i in range(count)]
    d = torch.cat([s[0] for s in scans]).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(s[0]) for s in scans])]).astype(np.int32)
    poses = np.asarray([s[2] for s in scans], np.float32)
    del scans
    n = int(offs[-1])
    ctx = scvod_py.Ctx(P, max_points_total=n + 64, max_scans=count)
    nxt = np.asarray([s + skip if s + skip < count else -1 for s in range(count)], np.int32)
    T = np.zeros((count, 12), np.float32)
    for s in range(count):
        if nxt[s] >= 0:
            T[s] = ctx.pose_delta(poses[s], poses[nxt[s]])
    st = torch.cuda.current_stream().cuda_stream

    def step():
        ctx.batch_process(d, offs, stream=st, sync=False)
        ctx.batch_cluster(stream=st, sync=False)
        ctx.batch_cluster_types(stream=st, sync=False)
        ctx.batch_track(T, next_scan=nxt, stream=st, sync=False)

    med, lo, hi = timed(step, reps)
    torch.cuda.synchronize()
    c = ctx.batch_counts().astype(np.int64).sum(0)
    out = dict(kind=kind, scans=count, points=n, apri=int(c[4]), plain_step=dict(ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3)))
    d_off = torch.empty(count + 1, dtype=torch.int32, device="cuda")
    ctx.batch_objects(d_off, None, stream=st)
    s0 = ctx.batch_objects_stats()
    k, m = s0["objects"], s0["members"]
    out.update(objects=k, members=m)
    rec = torch.empty((max(k, 1), 64), dtype=torch.uint8, device="cuda")
    mem = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
    pobj = torch.empty(n, dtype=torch.int32, device="cuda")
    cases = {
        "count_only": lambda: ctx.batch_objects(d_off, None, stream=st),
        "members_only": lambda: ctx.batch_objects(d_off, None, d_member_src=mem, stream=st),
        "records": lambda: ctx.batch_objects(d_off, rec, stream=st),
        "records_no_track": lambda: ctx.batch_objects(d_off, rec, flags=scvod_py.OBJ_NO_TRACK, stream=st),
        "records_members": lambda: ctx.batch_objects(d_off, rec, d_member_src=mem, stream=st),
        "records_members_point_object": lambda: ctx.batch_objects(d_off, rec, d_member_src=mem, d_point_object=pobj, stream=st),
    }
    for name, fn in cases.items():
        med, lo, hi = timed(fn, reps)
        out[name] = dict(ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3))
    s1 = ctx.batch_objects_stats()
    assert s1["objects"] == k and s1["members"] == m and s1["written"] == k
    h = rec.cpu().numpy().reshape(-1).view(scvod_py.OBJECT_DTYPE)[:k]
    out["largest_object_points"] = int(h["n_points"].max()) if k else 0
    out["scratch_bytes"] = ctx.batch_objects_scratch_bytes()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    scvod_py.load_lib()
    for kind in a.jobs.split(","):
        print(json.dumps(run(kind, a.scale, a.reps)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
