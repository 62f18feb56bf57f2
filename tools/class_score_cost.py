#!/usr/bin/env python3
"""Development tool: what the class scores on the device cost on the bench-shaped jobs -- scvod_batch_score_classes
(csrc/scvod_classes.hip) after a tracked step, with the region growing off and on, next to scvod_batch_evaluate (csrc/scvod_eval.hip) on
the same batch in the same process: the yardstick, since the first pass does the evaluation's work on a wider cell.  Only the scoring /
evaluation call is timed: stream-event times, the median of --reps runs after --warmup calls.  Per run also the length of the second
pass's list, the rings the parameters ask for and the scratch bytes.  Writes one block per job to profiles/class_score_cost.txt.
usage: python tools/class_score_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 5] [--warmup 2]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
import scvod_py
import synth

JOBS = {"K64": ("semantickitti", 5, 2761, 5), "PARK": ("parkinglot", 3, 2000, 1), "OS128": ("os128_fine", 5, 1000, 5)}
OUT = os.path.join(ROOT, "profiles", "class_score_cost.txt")


def timed(fn, reps, warmup):
    for _ in range(warmup):
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
    return dict(ms=round(float(np.median(ms)), 3), ms_min=round(float(min(ms)), 3), ms_max=round(float(max(ms)), 3))


def run(kind, scale, reps, warmup):
    preset, seq, count, skip = JOBS[kind]
    count = max(skip + 1, int(count * scale))
    P = scvod_py.make_params(preset)
    scans = [synth.make_scan(seq, i, kind, device="cuda") for i in range(count)]
    d = torch.cat([s[0] for s in scans]).contiguous()
    d_gt = torch.cat([s[1] for s in scans]).to(torch.int32).contiguous()
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
    par = scvod_py.class_params_default()
    out = dict(kind=kind, scans=count, points=n, max_dist=par.max_dist, cell=par.cell,
               rings=int(math.ceil(par.max_dist / (0.99 * par.cell))))
    ctx.batch_process(d, offs, stream=st, sync=False)
    ctx.batch_cluster(stream=st, sync=False)
    for rg in (False, True):
        ctx.set_region_growing(rg)
        ctx.batch_cluster_types(stream=st, sync=False)
        ctx.batch_track(T, next_scan=nxt, stream=st, sync=False)
        torch.cuda.synchronize()
        tag = "rg_on" if rg else "rg_off"
        ev = timed(lambda: ctx.batch_evaluate(d_gt, poses, stream=st), reps, warmup)
        cs = timed(lambda: ctx.batch_score_classes(d_gt, poses, params=par, stream=st), reps, warmup)
        res = ctx.score_classes_stats()
        out[tag] = dict(batch_evaluate=ev, batch_score_classes=cs, ratio=round(cs["ms"] / max(ev["ms"], 1e-6), 3),
                        pass2_queries=ctx.score_classes_pass2_queries(), conf=res["conf"], pd_far=res["pd_far"],
                        rate_P=[round(float(v), 6) for v in res["rate_P"]])
        if rg:
            out[tag]["building_clusters"] = ctx.batch_region_growing_stats()["building_clusters"]
    out["score_scratch_bytes"] = ctx.score_classes_scratch_bytes()
    out["evaluate_scratch_bytes"] = ctx.evaluate_scratch_bytes()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    scvod_py.load_lib()
    head = ("Class scores on the device (scvod_batch_score_classes, csrc/scvod_classes.hip): cost on the bench-shaped jobs\n"
            f"written by tools/class_score_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --warmup {a.warmup} on "
            f"{torch.cuda.get_device_name(0)}\n"
            "per job, with the region growing off and on: ms per call (median / min / max of stream-event times after the warm-up calls) of\n"
            "scvod_batch_evaluate and of scvod_batch_score_classes on the same tracked batch in the same process, their ratio (the target is\n"
            "1.5), the queries the second pass took, the confusion counts and the P rates (ground, building, tree, pd).  Only the call itself\n"
            "is timed.  --scale is the fraction of the bench job's scans.  A job that is missing below was not measured.\n\n")
    with open(a.out, "w") as f:
        f.write(head)
    for kind in a.jobs.split(","):
        r = run(kind, a.scale, a.reps, a.warmup)
        line = json.dumps(r)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(f"{kind}: {line}\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
