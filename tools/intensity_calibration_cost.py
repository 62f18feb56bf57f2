#!/usr/bin/env python3
"""Development tool: what the opt-in intensity calibration (scvod_set_intensity_calibration, csrc/scvod_k_calib.inc) costs on the
bench-shaped jobs.  Per job: scvod_batch_process with the stage off and on (host clock around a synchronised call, median of
--reps after a warm-up call of each), the stage's own launches (driver-timed, summed over the chunks: cal_slot + cal_grid = the index
build, cal_knn = kNN with the fused normal + calibration), its counters, the share of queries on the fallback path and the mean
candidates a query examined.  --baseline runs the job once more in a child process with SCVOD_CALIB_FORCE_FALLBACK=1: no tile is
staged and no dynamic LDS is reserved (so the registers alone set the residency), every query walks the cell-sorted copy in HBM one
thread per query, which is k_rg_knn's loop on the per-scan index.
--k3 adds the stage with search_num 3 (the cheapest normal: what is left is the search).
usage: python tools/intensity_calibration_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 3] [--baseline] [--k3]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
import scvod_py
import synth

JOBS = {"K64": ("semantickitti", 5, 2761), "PARK": ("parkinglot", 3, 2000), "OS128": ("os128_fine", 5, 1000)}


def process_ms(ctx, d, offs, reps):
    ctx.batch_process(d, offs)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.batch_process(d, offs)
        ms.append((time.perf_counter() - t0) * 1e3)
    return [round(v, 2) for v in ms]


def stage(ctx, d, offs, k):
    ctx.set_intensity_calibration(True, k, 200.0)
    ctx.batch_process(d, offs)
    ctx.set_timing(True)
    ctx.batch_process(d, offs)
    kt = {}
    for name, ms in ctx.timings(cap=8192):
        if name.startswith("cal_"):
            kt[name] = kt.get(name, 0.0) + ms
    ctx.set_timing(False)
    st = ctx.batch_intensity_calibration_stats()
    cand = ctx.batch_intensity_calibration_candidates()
    q = max(st["points"], 1)
    return dict(search_num=k, index_build_ms=round(kt.get("cal_slot", 0.0) + kt.get("cal_grid", 0.0), 3), knn_normal_calibration_ms=round(kt.get("cal_knn", 0.0), 3),
                stage_ms=round(sum(kt.values()), 3), stats=st, fallback_share=round(st["fallback_queries"] / q, 4), candidates_per_query=round(cand / q, 1))


def run(kind, scale, reps, k3):
    preset, seq, count = JOBS[kind]
    count = max(2, int(count * scale))
    P = scvod_py.make_params(preset)
    scans = [synth.make_scan(seq, i, kind, device="cuda")[0] for i in range(count)]
    d = torch.cat(scans).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    del scans
    ctx = scvod_py.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=count)
    out = dict(kind=kind, scans=count, points=int(offs[-1]), forced_fallback=bool(os.environ.get("SCVOD_CALIB_FORCE_FALLBACK")))
    out["process_ms_off"] = process_ms(ctx, d, offs, reps)
    ctx.set_intensity_calibration(True, 10, 200.0)
    out["process_ms_on"] = process_ms(ctx, d, offs, reps)
    out["stage"] = stage(ctx, d, offs, 10)
    if k3:
        out["stage_k3"] = stage(ctx, d, offs, 3)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline", action="store_true", help="also run with every query on the one-thread-per-query HBM path (a child process)")
    ap.add_argument("--k3", action="store_true")
    a = ap.parse_args()
    scvod_py.load_lib()
    for kind in a.jobs.split(","):
        print(json.dumps(run(kind, a.scale, a.reps, a.k3)), flush=True)
        torch.cuda.empty_cache()
    if a.baseline and not os.environ.get("SCVOD_CALIB_FORCE_FALLBACK"):
        torch.cuda.synchronize()
        env = dict(os.environ, SCVOD_CALIB_FORCE_FALLBACK="1")
        cmd = [sys.executable, os.path.abspath(__file__), "--jobs", a.jobs, "--scale", str(a.scale), "--reps", str(a.reps)]
        sys.exit(subprocess.call(cmd, env=env))


if __name__ == "__main__":
    main()
