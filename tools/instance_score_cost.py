#!/usr/bin/env python3
"""Development tool: what the instance table on the device costs on the bench-shaped jobs -- scvod_score_instances_device
(csrc/scvod_instances.hip) alone, on the result bytes of scvod_batch_evaluate (csrc/scvod_eval.hip) of the same tracked batch in the
same process: the evaluation is the yardstick.  Keys: the synthetic labels OR-ed with ((object of the point + 1) mod 4096) << 16, the
object index being scvod_batch_objects' d_point_object: a few thousand distinct keys in scan order, one hot class.  Two variants of
k_in_aggregate are timed in interleaved rounds (evaluate, variant 0, variant 1, evaluate, ...): 0 combines the equal keys of a wave by
ballot before the LDS table, 1 lets every point add into the LDS table on its own.  Stream-event times; median, min and max of --reps
rounds after --warmup rounds; GB/s = 5 bytes per point (key and result byte) over the median.  Writes one line per job to
profiles/instance_score_cost.txt.
usage: python tools/instance_score_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 7] [--warmup 2]"""
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
OUT = os.path.join(ROOT, "profiles", "instance_score_cost.txt")
CAP = 65536
COPY_CEILING_TBS = 4.60  # profiles/r06_kernel_table.md


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(ms):
    return dict(ms=round(float(np.median(ms)), 4), ms_min=round(float(min(ms)), 4), ms_max=round(float(max(ms)), 4))


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
    ctx.batch_process(d, offs, stream=st, sync=False)
    ctx.batch_cluster(stream=st, sync=False)
    ctx.batch_cluster_types(stream=st, sync=False)
    ctx.batch_track(T, next_scan=nxt, stream=st, sync=False)
    d_obj = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.batch_objects(torch.empty(count + 1, dtype=torch.int32, device="cuda"), d_point_object=d_obj, stream=st)
    ctx.batch_objects_stats()
    d_key = (d_gt | (((d_obj + 1) % 4096) << 16)).contiguous()
    del d_obj
    d_res = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_inst = torch.empty(CAP * scvod_py.INSTANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    calls = dict(batch_evaluate=lambda: ctx.batch_evaluate(d_key, poses, d_point_result=d_res, stream=st))
    for v, name in ((0, "wave_match"), (1, "lds_atomics")):
        def call(v=v):
            ctx.lib.scvod_set_score_instances_variant(ctx.h, v)
            ctx.score_instances_device(d_key, d_res, cap_instances=CAP, d_instances=d_inst, stream=st)
        calls[name] = call
    ms = {k: [] for k in calls}
    tables = {}
    for r in range(warmup + reps):
        for k, fn in calls.items():
            t = once(fn)
            if r >= warmup:
                ms[k].append(t)
            if k != "batch_evaluate":
                stats = ctx.score_instances_stats()
                tables[k] = d_inst[:stats["written"] * scvod_py.INSTANCE_DTYPE.itemsize].cpu().numpy().tobytes()
    ctx.lib.scvod_set_score_instances_variant(ctx.h, 0)
    assert tables["wave_match"] == tables["lds_atomics"], "the two variants disagree"
    out = dict(kind=kind, scans=count, points=n, distinct_keys=stats["distinct"], spilled_tiles=stats["spilled_tiles"], cap_instances=CAP)
    for k in calls:
        out[k] = spread(ms[k])
        if k != "batch_evaluate":
            gbs = 5.0 * n / (out[k]["ms"] * 1e-3) / 1e9
            out[k]["GBps"] = round(gbs, 1)
            out[k]["of_copy_ceiling"] = round(gbs / (COPY_CEILING_TBS * 1e3), 3)
    out["share_of_evaluate"] = round(out["wave_match"]["ms"] / max(out["batch_evaluate"]["ms"], 1e-6), 4)
    out["instances_scratch_bytes"] = ctx.score_instances_scratch_bytes()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    scvod_py.load_lib()
    head = ("Instance table on the device (scvod_score_instances_device, csrc/scvod_instances.hip): cost on the bench-shaped jobs\n"
            f"written by tools/instance_score_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --warmup {a.warmup} on "
            f"{torch.cuda.get_device_name(0)}\n"
            "per job: ms per call (median / min / max of stream-event times over interleaved rounds after the warm-up rounds) of\n"
            "scvod_batch_evaluate (the yardstick) and of scvod_score_instances_device alone on its result bytes, in two variants of\n"
            "k_in_aggregate: wave_match (equal keys of a wave combined by ballot before the LDS table; shipped) and lds_atomics (every point\n"
            "adds into the LDS table on its own).  The call is the whole pass: two memsets, aggregate, compact, radix sort, gather.  GBps: 5\n"
            f"bytes per point over the median; of_copy_ceiling: against the {COPY_CEILING_TBS} TB/s copy ceiling (the hbm class starts at 0.6).\n"
            "--scale is the fraction of the bench job's scans.  A job that is missing below was not measured.\n\n")
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
