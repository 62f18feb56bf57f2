#!/usr/bin/env python3
"""Development tool: what one iteration of the pose refinement costs on the bench-shaped jobs -- scvod_batch_map_register
(csrc/scvod_register.hip, k_reg_accumulate + k_reg_solve) next to the yardstick, scvod_batch_map_query (csrc/scvod_mapquery.hip) at the
same radius with the result byte and the nn pair, on the same points and the same map, in the same process.
Timed in interleaved rounds (query, reg1, reg1_gated, reg10, query, ...):
  query       scvod_batch_map_query, radius --radius-share * leaf, d_result + d_nn_key + d_nn_sqdist
  reg1        scvod_batch_map_register, max_iterations 1, max_dist = that radius, max_range +inf, no labels
  reg1_gated  the same with the labels of scvod_batch_point_labels and a use256 that leaves out PT_DYNAMIC and PT_DROPPED
  reg10       max_iterations 10 from poses off by --offset metres (scans converge and latch at different iterations)
Stream-event times; the median, minimum and maximum of --reps rounds after --warmup rounds.  `spread` is (max - min) / median.
One child process per job.  Writes one block per job to profiles/register_cost.txt.
usage: python tools/register_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 7] [--warmup 2] [--radius-share 0.99] [--note TEXT]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))

JOBS = {"K64": ("semantickitti", 5, 2761, 5), "PARK": ("parkinglot", 3, 2000, 1), "OS128": ("os128_fine", 5, 1000, 5)}
OUT = os.path.join(ROOT, "profiles", "register_cost.txt")
LEAF = 0.2


def summary(ms):
    med = float(np.median(ms))
    return dict(ms=round(med, 3), ms_min=round(float(min(ms)), 3), ms_max=round(float(max(ms)), 3),
                spread=round((max(ms) - min(ms)) / max(med, 1e-9), 3))


def run(kind, scale, reps, warmup, radius_share, offset):
    import torch

    import scvod_py
    import synth
    scvod_py.load_lib()
    RADIUS = float(np.float32(radius_share) * np.float32(LEAF))
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
    ctx.batch_track(T, next_scan=nxt, stream=st, sync=False)
    torch.cuda.synchronize()
    cells = 1 << int(np.ceil(np.log2(max(n * 0.25, 1 << 22))))       # the benchmark's sizing
    full = scvod_py.StaticMap(cells, leaf=LEAF)
    full.accumulate(ctx, poses, stream=st)
    n_cells = full.count()
    labels = ctx.batch_point_labels(stream=st)
    res = torch.empty(n, dtype=torch.uint8, device="cuda")
    key = torch.empty(n, dtype=torch.int64, device="cuda")
    sq = torch.empty(n, dtype=torch.float32, device="cuda")
    pose_out = torch.empty((count, 12), dtype=torch.float64, device="cuda")
    rec = torch.empty(count * 64, dtype=torch.uint8, device="cuda")
    lib, vp = full.lib, scvod_py.C.c_void_p
    off_poses = poses.copy()
    off_poses[:, 0] += np.float32(offset)
    use = np.ones(256, np.uint8)
    use[[scvod_py.PT_DROPPED, scvod_py.PT_DYNAMIC]] = 0
    one = scvod_py.register_params_default(max_iterations=1, max_dist=RADIUS, max_range=float("inf"))
    gated = scvod_py.register_params_default(max_iterations=1, max_dist=RADIUS, max_range=float("inf"), use256=use)
    ten = scvod_py.register_params_default(max_iterations=10, max_dist=RADIUS, max_range=float("inf"))

    def p(t):
        return vp(t.data_ptr())

    def query():
        rc = lib.scvod_batch_map_query(ctx.h, full.h, poses.ctypes.data_as(vp), RADIUS, None, p(res), None, p(key), p(sq), None, vp(st))
        assert rc == 0, lib.scvod_map_last_error(full.h).decode()

    def register(h_poses, params, lab):
        rc = lib.scvod_batch_map_register(ctx.h, full.h, h_poses.ctypes.data_as(vp), p(lab) if lab is not None else None,
                                          scvod_py.C.byref(params), None, p(pose_out), p(rec), vp(st))
        assert rc == 0, lib.scvod_map_last_error(full.h).decode()

    arms = (("query", query), ("reg1", lambda: register(poses, one, None)), ("reg1_gated", lambda: register(poses, gated, labels)),
            ("reg10", lambda: register(off_poses, ten, None)))
    ms = {name: [] for name, _ in arms}
    stats = {}
    for r in range(warmup + reps):
        for name, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms[name].append(e0.elapsed_time(e1))
            if r == 0:
                stats[name] = full.query_stats() if name == "query" else full.register_stats()
    out = dict(kind=kind, scans=count, points=n, map_cells=cells, cells=n_cells, leaf=LEAF, radius=round(RADIUS, 6), offset=offset)
    for name in ms:
        out[name] = summary(ms[name])
    out["stats"] = stats
    assert full.count() == n_cells                                    # the register calls moved nothing
    out["reg1_over_query"] = round(out["reg1"]["ms"] / max(out["query"]["ms"], 1e-9), 3)
    out["reg1_gated_over_query"] = round(out["reg1_gated"]["ms"] / max(out["query"]["ms"], 1e-9), 3)
    out["reg10_over_reg1"] = round(out["reg10"]["ms"] / max(out["reg1"]["ms"], 1e-9), 3)
    full.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radius-share", type=float, default=0.99, help="the radius as a share of the leaf (at most 0.99)")
    ap.add_argument("--offset", type=float, default=0.03, help="metres the poses of reg10 are off along x")
    ap.add_argument("--note", default="", help="a line for the head of the file (e.g. the build that was measured)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--one", default="", help="(internal) measure this job in this process and print its JSON line")
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(run(a.one, a.scale, a.reps, a.warmup, a.radius_share, a.offset)), flush=True)
        return
    head = ("One iteration of the pose refinement (scvod_batch_map_register, k_reg_accumulate + k_reg_solve in csrc/scvod_register.hip) next to\n"
            "scvod_batch_map_query at the same radius with the byte and the nn pair: cost on the bench-shaped jobs\n"
            f"written by tools/register_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --warmup {a.warmup} --radius-share {a.radius_share} "
            f"--offset {a.offset}\n"
            + (a.note + "\n" if a.note else "") +
            "per job, on one tracked batch in one process of its own, interleaved rounds:\n"
            "  query       scvod_batch_map_query, radius --radius-share * leaf, d_result + d_nn_key + d_nn_sqdist -- the yardstick\n"
            "  reg1        scvod_batch_map_register, max_iterations 1, max_dist = that radius, no range gate, no labels\n"
            "  reg1_gated  the same with the labels of scvod_batch_point_labels, PT_DYNAMIC and PT_DROPPED left out\n"
            "  reg10       max_iterations 10 from poses off by --offset metres along x\n"
            "ms = median of the stream-event times after the warm-up rounds, with minimum, maximum and spread = (max - min) / median.\n"
            "stats = {points, cell, near, miss, out} of the query, the eight totals of scvod_map_register_stats of the others.\n"
            "The aim: reg1_over_query <= 1.  --scale is the fraction of the bench job's scans.  A job that is missing below was not measured.\n\n")
    with open(a.out, "w") as f:
        f.write(head)
    for kind in a.jobs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", kind, "--scale", str(a.scale), "--reps", str(a.reps), "--warmup", str(a.warmup),
               "--radius-share", str(a.radius_share), "--offset", str(a.offset)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        got = [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"{kind}: the child process failed with status {r.returncode}")
        line = f"{kind}: {got[0]}"
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
