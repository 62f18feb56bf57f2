#!/usr/bin/env python3
"""Development tool: what the opt-in region growing (scvod_set_region_growing, csrc/scvod_k_rgrow.inc) costs on the bench-shaped
jobs.  Per job: the step (process + cluster + types + tracking chain) with the stage off and on, the stage's own launches
(driver-timed, summed over the chunks), its counters (candidate points per scan, largest number of propagation sweeps), and how
the building / tree points fall on the synthetic labels (50/51 structure against 70/71 vegetation).  The reference's parameters.
usage: python tools/region_growing_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 3]"""
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


def run(kind, scale, reps, label_scans=20):
    preset, seq, count = JOBS[kind]
    count = max(2, int(count * scale))
    P = scvod_py.make_params(preset)
    scans = [synth.make_scan(seq, i, kind, device="cuda") for i in range(count)]
    labels = [scans[i][1].cpu().numpy() for i in range(min(label_scans, count))]
    d = torch.cat([s[0] for s in scans]).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(s[0]) for s in scans])]).astype(np.int32)
    poses = np.asarray([s[2] for s in scans], np.float32)
    del scans
    ctx = scvod_py.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=count)
    T = np.zeros((count, 12), np.float32)
    for s in range(count - 1):
        T[s] = ctx.pose_delta(poses[s], poses[s + 1])
    out = dict(kind=kind, scans=count, points=int(offs[-1]))
    for tag, on in (("off", False), ("on", True)):
        ctx.set_region_growing(on)
        out[f"step_ms_{tag}"] = step(ctx, d, offs, T, reps)
    ctx.set_region_growing(True)
    ctx.batch_process(d, offs)
    ctx.batch_cluster()
    ctx.set_timing(True)
    ctx.batch_cluster_types()
    kt = {}
    for name, ms in ctx.timings(cap=4096):
        kt[name] = kt.get(name, 0.0) + ms
    ctx.set_timing(False)
    out["stage_launches_ms"] = {k: round(v, 3) for k, v in kt.items()}
    out["stage_ms"] = round(sum(kt.values()), 3)
    st = ctx.batch_region_growing_stats()
    out["stats"] = st
    out["candidate_points_per_scan"] = round(st["candidate_points"] / count, 1)
    # building / tree points against the synthetic labels of the first scans (apri points matched to input points by coordinates)
    tab = {}
    for s, lab in enumerate(labels):
        r = ctx.batch_fetch(s)
        cls = ctx.batch_fetch_cluster_classes(s, r["n_apri"])
        x = d[offs[s]:offs[s + 1], :3].cpu().numpy()
        key = {tuple(v): i for i, v in enumerate(x.view(np.uint32).reshape(-1, 3).tolist())}
        a = np.stack([r["apri"]["x"], r["apri"]["y"], r["apri"]["z"]], -1).astype(np.float32)
        src = np.asarray([key[tuple(v)] for v in a.view(np.uint32).reshape(-1, 3).tolist()], np.int64)
        for c, nm in ((0, "building"), (1, "tree")):
            sel = lab[src[cls == c]] & 0xFFFF
            for g, labs in (("structure_50_51", (50, 51)), ("vegetation_70_71", (70, 71)), ("other", None)):
                m = np.isin(sel, labs) if labs else ~np.isin(sel, (50, 51, 70, 71))
                tab[f"{nm}/{g}"] = tab.get(f"{nm}/{g}", 0) + int(m.sum())
    out["labels_first_scans"] = dict(scans=len(labels), **tab)
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
