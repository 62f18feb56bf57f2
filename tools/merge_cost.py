#!/usr/bin/env python3
"""Development tool: what the opt-in intensity merge (scvod_set_intensity_merge, csrc/scvod_k_merge.inc) costs and changes on the
bench-shaped jobs.  Per job: the step (process + cluster + types + tracking chain) with the merge off and on, the merge's own
launches (driver-timed), its counters, and the fraction of per-point dynamic bytes that differ.  YAML parameters (3 / 2 / 2.0 / 1.0).
usage: python tools/merge_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
import scvod_py
import synth

JOBS = {"K64": ("semantickitti", 5, 2761), "PARK": ("parkinglot", 3, 2000), "OS128": ("os128_fine", 5, 1000)}


def step(ctx, d, offs, T, reps):
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.batch_process(d, offs, sync=False)
        ctx.batch_cluster(sync=False)
        ctx.batch_cluster_types(sync=False)
        ctx.batch_track(T, sync=True)
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def run(kind, scale, reps):
    preset, seq, count = JOBS[kind]
    count = max(2, int(count * scale))
    P = scvod_py.make_params(preset)
    scans = [synth.make_scan(seq, i, kind, device="cuda") for i in range(count)]
    d = torch.cat([s[0] for s in scans]).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(s[0]) for s in scans])]).astype(np.int32)
    poses = np.asarray([s[2] for s in scans], np.float32)
    del scans
    ctx = scvod_py.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=count)
    T = np.zeros((count, 12), np.float32)
    for s in range(count - 1):
        T[s] = ctx.pose_delta(poses[s], poses[s + 1])
    out = dict(kind=kind, scans=count, points=int(offs[-1]))
    dyn = {}
    for tag, it in (("off", 0), ("on", 3)):
        ctx.set_intensity_merge(it, 2, 2.0, 1.0)
        out[f"step_ms_{tag}"] = step(ctx, d, offs, T, reps)
        ctx.set_timing(True)
        ctx.batch_process(d, offs)
        ctx.batch_cluster()
        kt = {}
        for name, ms in ctx.timings():
            kt[name] = kt.get(name, 0.0) + ms
        ctx.set_timing(False)
        out[f"cluster_launches_ms_{tag}"] = {k: round(v, 3) for k, v in kt.items()}
        ctx.batch_process(d, offs)
        ctx.batch_cluster()
        ctx.batch_cluster_types()
        ctx.batch_track(T)
        dyn[tag] = np.concatenate([ctx.batch_fetch_track(s)["pt_dyn"] for s in range(count)])
        if it:
            out["merge_stats"] = ctx.batch_cluster_merge_stats()
    out["merge_ms"] = round(sum(v for k, v in out["cluster_launches_ms_on"].items() if k.startswith("im_")), 3)
    out["dynamic_bytes_changed_fraction"] = float((dyn["off"] != dyn["on"]).mean())
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    scvod_py.load_lib()
    for kind in a.jobs.split(","):
        print(json.dumps(run(kind, a.scale, a.reps)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
