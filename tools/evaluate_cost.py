#!/usr/bin/env python3
"""Development tool: what the evaluation on the device costs on the bench-shaped jobs -- scvod_batch_evaluate (csrc/scvod_eval.hip) after
a tracked step, scvod_evaluate_device on the clouds scvod_batch_export_points hands out, and the host path on the same input:
metric.preservation_rejection over Ctx.nn_radius_search (quality.compare's call) on the first `--host-scans` scans of the job, the sample
size of the benchmark's quality block.  Device times are stream-event times after a warm-up call (median, min, max of --reps); the
host path is wall time of one call, uploads and downloads included.  Appends one block per job to profiles/evaluate_cost.txt.
usage: python tools/evaluate_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 5] [--host-scans 320]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
import metric
import quality
import scvod_py
import synth

JOBS = {"K64": ("semantickitti", 5, 2761, 5), "PARK": ("parkinglot", 3, 2000, 1), "OS128": ("os128_fine", 5, 1000, 5)}
OUT = os.path.join(ROOT, "profiles", "evaluate_cost.txt")


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
    return dict(ms=round(float(np.median(ms)), 3), ms_min=round(float(min(ms)), 3), ms_max=round(float(max(ms)), 3))


def run(kind, scale, reps, host_scans):
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
    ctx.batch_process(d, offs, stream=st, sync=False)
    ctx.batch_cluster(stream=st, sync=False)
    ctx.batch_cluster_types(stream=st, sync=False)
    ctx.batch_track(T, next_scan=nxt, stream=st, sync=False)
    torch.cuda.synchronize()
    out = dict(kind=kind, scans=count, points=n)
    out["batch_evaluate"] = timed(lambda: ctx.batch_evaluate(d_gt, poses, stream=st), reps)
    res = ctx.evaluate_stats()
    out["result"] = {k: res[k] for k in ("num_gt_static", "num_gt_dynamic", "num_preserved", "PR", "RR", "F1")}
    out["scratch_bytes"] = ctx.evaluate_scratch_bytes()
    # the exported clouds through scvod_evaluate_device: gt = every point in the world frame (an export that keeps everything Patchwork
    # kept would not do: the dropped points are ground truth too), estimate = the export
    d_off = torch.empty(count + 1, dtype=torch.int32, device="cuda")
    xyzi = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    pay = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.batch_export_points(d_off, xyzi, poses=poses, d_payload_in=d_gt, d_payload_out=pay, stream=st)
    kept = ctx.batch_export_stats()["kept"]
    est = xyzi[:kept, :3].contiguous()
    est_lab = pay[:kept].contiguous()
    del xyzi, pay
    x = d.cpu().numpy()
    gt = d_gt.cpu().numpy().view(np.uint32)
    w = quality.world_points(scvod_py, x, offs, poses)
    d_w = torch.from_numpy(w).cuda()
    out["kept_points"] = kept
    out["evaluate_device"] = timed(lambda: ctx.evaluate_device(d_w, d_gt, est, est_lab, stream=st), reps)
    res2 = ctx.evaluate_stats()
    assert all(res2[k] == res[k] for k in scvod_py.EVAL_COUNTS), "the compacted estimate gives other counters than the keep mask"
    # the host path on the benchmark's sample size
    hs = min(host_scans, count)
    m = int(offs[hs])
    keep = np.zeros(n, bool)
    src = est.cpu().numpy()
    lab_b = ctx.batch_point_labels(stream=st).cpu().numpy()[:n]
    keep = (lab_b != scvod_py.PT_DROPPED) & (lab_b != scvod_py.PT_DYNAMIC)
    assert int(keep.sum()) == kept and np.array_equal(w[keep].view(np.uint32), src.view(np.uint32))
    k = keep[:m]
    t0 = time.perf_counter()
    hm = metric.preservation_rejection(w[:m], gt[:m], w[:m][k], gt[:m][k], ctx.nn_radius_search, 0.2)
    host_ms = (time.perf_counter() - t0) * 1e3
    out["host_path"] = dict(scans=hs, points=m, ms=round(host_ms, 1), PR=hm["PR"], RR=hm["RR"])
    dev_same = timed(lambda: ctx.evaluate_device(d_w[:m], d_gt[:m], torch.from_numpy(w[:m][k]).cuda(), torch.from_numpy(gt[:m][k].view(np.int32)).cuda(),
                                                 stream=st), 1)
    rs = ctx.evaluate_stats()
    assert all(rs[c] == hm[c] for c in scvod_py.EVAL_COUNTS), "device and host path disagree on the sample"
    out["evaluate_device_on_host_sample"] = dev_same  # (includes the upload of the sample's estimate)
    out["host_over_device_on_sample"] = round(host_ms / max(dev_same["ms"], 1e-3), 1)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-scans", type=int, default=320)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    scvod_py.load_lib()
    head = ("Evaluation on the device (scvod_batch_evaluate / scvod_evaluate_device, csrc/scvod_eval.hip): cost on the bench-shaped jobs\n"
            f"written by tools/evaluate_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --host-scans {a.host_scans} on "
            f"{torch.cuda.get_device_name(0)}\n"
            "per job: ms per call (median / min / max of stream-event times after a warm-up call) of scvod_batch_evaluate on the whole job and\n"
            "of scvod_evaluate_device on its exported clouds; wall ms of the host path (metric.preservation_rejection over Ctx.nn_radius_search)\n"
            "on the first --host-scans scans, of scvod_evaluate_device on that same sample (one call, the upload of its estimate included), and\n"
            "their ratio.  A job that is missing below was not measured.\n\n")
    with open(a.out, "w") as f:
        f.write(head)
    for kind in a.jobs.split(","):
        r = run(kind, a.scale, a.reps, a.host_scans)
        line = json.dumps(r)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(f"{kind}: {line}\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
