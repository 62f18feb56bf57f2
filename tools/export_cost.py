#!/usr/bin/env python3
"""Development tool: what handing the result on costs on the bench-shaped jobs -- scvod_batch_point_labels and
scvod_batch_export_points (csrc/scvod_export.hip) after a tracked step, timed with stream events after a warm-up, next to the bytes
the passes have to move (counted from the batch's own counters) and the fraction of the copy ceiling of this machine that makes
(4.60 TB/s, profiles/r06_pmc_calibration.md).
usage: python tools/export_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 5]"""
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
COPY_CEILING_TBS = 4.60


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
    ctx.batch_process(d, offs, stream=st, sync=False)
    ctx.batch_cluster(stream=st, sync=False)
    ctx.batch_cluster_types(stream=st, sync=False)
    ctx.batch_track(T, next_scan=nxt, stream=st, sync=True)
    c = ctx.batch_counts().astype(np.int64).sum(0)
    n_g, n_a, n_r = int(c[1]), int(c[4]), int(c[5])
    lab = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(count + 1, dtype=torch.int32, device="cuda")
    xyzi = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    pay_in = torch.arange(n, dtype=torch.int32, device="cuda")
    pay_out = torch.empty(n, dtype=torch.int32, device="cuda")
    out = dict(kind=kind, scans=count, points=n, ground=n_g, apri=n_a, rejected=n_r, dropped=int(c[3]))
    ctx.batch_export_points(d_off, None, stream=st)
    k = ctx.batch_export_stats()["kept"]
    out["kept"] = k
    # bytes every pass has to move at least: clear + the three lists (index, and type + tracking byte per apri point) + one byte stored per listed point
    b_labels = n + 4 * (n_g + n_a + n_r) + 2 * n_a + (n_g + n_a + n_r)
    b_count = n                                   # the count pass reads the label bytes
    b_write = n + 16 * k + 16 * k                 # the write pass reads them again, reads and stores the kept records
    cases = {
        "labels": (lambda: ctx.batch_point_labels(lab, stream=st), b_labels),
        "export_count_only": (lambda: ctx.batch_export_points(d_off, None, stream=st), b_labels + b_count),
        "export_xyzi": (lambda: ctx.batch_export_points(d_off, xyzi, stream=st), b_labels + b_count + b_write),
        "export_xyzi_world": (lambda: ctx.batch_export_points(d_off, xyzi, poses=poses, stream=st), b_labels + b_count + b_write),
        "export_xyzi_src_payload": (lambda: ctx.batch_export_points(d_off, xyzi, d_payload_in=pay_in, d_payload_out=pay_out, d_src_out=src, stream=st),
                                    b_labels + b_count + b_write + 12 * k),
    }
    for name, (fn, nbytes) in cases.items():
        med, lo, hi = timed(fn, reps)
        out[name] = dict(ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), gbytes=round(nbytes / 1e9, 3),
                         tbytes_per_s=round(nbytes / med / 1e9, 3), fraction_of_copy_ceiling=round(nbytes / med / 1e9 / COPY_CEILING_TBS, 3))
    assert ctx.batch_export_stats()["kept"] == k
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
