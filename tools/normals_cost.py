#!/usr/bin/env python3
"""Development tool: what the surface normals cost on the bench-shaped jobs -- scvod_normals_device (csrc/scvod_normals.hip: k_nrm_keep,
the grid build, k_nrm_accumulate) on two clouds of every job, the world-frame static export of the batch and the points of its map, at
radius 0.3 and 0.5, next to the yardstick: scvod_nn_search_device of the same cloud against itself at the same radius, which builds the
same grid and walks the same 27 probes but keeps only the nearest candidate.
Timed in interleaved rounds (nn, query_order, entry_order, nn, ...):
  nn           scvod_nn_search_device, the packed xyz of the cloud as map and as queries (every query finds itself: no second pass)
  query_order  the self form, a thread per query in the caller's order (scvod_set_normals_variant 1), normals + curvature
  entry_order  the self form, a thread per grid entry (variant 2)
  cpu          tests/helpers/normals_ref.cpp (the exhaustive loop, one thread) on --cpu-queries queries of the cloud, as ms per query
Stream-event times; the median, minimum and maximum of --reps rounds after --warmup rounds.  `spread` is (max - min) / median.
One child process per job.  Writes one block per job to profiles/normals_cost.txt.
usage: python tools/normals_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 7] [--warmup 2] [--cpu-queries 32] [--note TEXT]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))

JOBS = {"K64": ("semantickitti", 5, 2761, 5), "PARK": ("parkinglot", 3, 2000, 1), "OS128": ("os128_fine", 5, 1000, 5)}
OUT = os.path.join(ROOT, "profiles", "normals_cost.txt")
LEAF = 0.2
RADII = (0.3, 0.5)


def summary(ms):
    med = float(np.median(ms))
    return dict(ms=round(med, 3), ms_min=round(float(min(ms)), 3), ms_max=round(float(max(ms)), 3),
                spread=round((max(ms) - min(ms)) / max(med, 1e-9), 3))


def cpu_ms_per_query(cloud4, radius, n_queries):
    """the exhaustive helper on one thread: ms per query against the whole cloud"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import normals_ref
    lib = normals_ref.build(tempfile.mkdtemp(prefix="normalsref"))
    pick = np.linspace(0, len(cloud4) - 1, n_queries).astype(np.int64)
    q = np.ascontiguousarray(cloud4[pick, :3])
    t0 = time.perf_counter()
    h = normals_ref.run(lib, cloud4, q, radius, 5)
    dt = time.perf_counter() - t0
    return round(1000.0 * dt / max(n_queries, 1), 3), round(float(h["count"].mean()), 1)


def run(kind, scale, reps, warmup, cpu_queries):
    import torch

    import scvod_py
    import synth
    scvod_py.load_lib()
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
    map_pts = full.points(stream=st)[0].contiguous()
    d_off = torch.empty(count + 1, dtype=torch.int32, device="cuda")
    export = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ctx.batch_export_points(d_off, export, poses=poses, stream=st)
    export = export[:ctx.batch_export_stats()["kept"]].contiguous()
    out = dict(kind=kind, scans=count, points=n, leaf=LEAF)
    for cloud_name, cloud in (("export", export), ("map", map_pts)):
        xyz = cloud[:, :3].contiguous()
        m = len(cloud)
        nrm = torch.empty((max(m, 1), 3), dtype=torch.float32, device="cuda")
        cur = torch.empty(max(m, 1), dtype=torch.float32, device="cuda")
        idx = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
        sq = torch.empty(max(m, 1), dtype=torch.float32, device="cuda")
        within = torch.empty(max(m, 1), dtype=torch.uint8, device="cuda")
        host = cloud.cpu().numpy()
        vp = scvod_py.C.c_void_p
        for radius in RADII:
            par = scvod_py.normal_params_default(radius=radius)

            def nn():
                ctx._chk(ctx.lib.scvod_nn_search_device(ctx.h, vp(xyz.data_ptr()), m, vp(xyz.data_ptr()), m, float(radius), vp(idx.data_ptr()),
                                                        vp(sq.data_ptr()), vp(within.data_ptr()), vp(st)))

            def normals(variant):
                ctx.set_normals_variant(variant)
                ctx._chk(ctx.lib.scvod_normals_device(ctx.h, vp(cloud.data_ptr()), 4, m, None, 0, m, None, None, 0, scvod_py.C.byref(par),
                                                      vp(nrm.data_ptr()), vp(cur.data_ptr()), None, None, vp(st)))

            arms = (("nn", nn), ("query_order", lambda: normals(scvod_py.NORMALS_QUERY_ORDER)),
                    ("entry_order", lambda: normals(scvod_py.NORMALS_ENTRY_ORDER)))
            ms = {name: [] for name, _ in arms}
            stats = None
            for r in range(warmup + reps):
                for name, fn in arms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if r >= warmup:
                        ms[name].append(e0.elapsed_time(e1))
                    if r == 0 and name == "entry_order":
                        stats = ctx.normals_stats()
            row = dict(cloud_points=m, radius=radius)
            for name in ms:
                row[name] = summary(ms[name])
            row["query_order_over_nn"] = round(row["query_order"]["ms"] / max(row["nn"]["ms"], 1e-9), 3)
            row["entry_order_over_nn"] = round(row["entry_order"]["ms"] / max(row["nn"]["ms"], 1e-9), 3)
            row["mean_k"] = round(stats["sum_k"] / max(stats["queries"] - stats["nonfinite_queries"], 1), 1)
            row["largest_k"] = stats["largest_k"]
            row["finite"] = stats["finite"]
            if cpu_queries > 0 and m > 0:
                row["cpu_ms_per_query"], row["cpu_mean_k"] = cpu_ms_per_query(host, radius, cpu_queries)
                row["cpu_ms_whole_cloud_extrapolated"] = round(row["cpu_ms_per_query"] * m, 0)
            out[f"{cloud_name}_r{radius}"] = row
    ctx.set_normals_variant(0)
    out["scratch_bytes"] = ctx.normals_scratch_bytes()
    full.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-queries", type=int, default=32, help="queries the one-thread CPU helper is timed on (0: skip it)")
    ap.add_argument("--note", default="", help="a line for the head of the file (e.g. the build that was measured)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--one", default="", help="(internal) measure this job in this process and print its JSON line")
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(run(a.one, a.scale, a.reps, a.warmup, a.cpu_queries)), flush=True)
        return
    head = ("Surface normals of a cloud (scvod_normals_device: k_nrm_keep, the grid build, k_nrm_accumulate in csrc/scvod_normals.hip) next to\n"
            "scvod_nn_search_device of the same cloud against itself at the same radius: cost on the bench-shaped jobs\n"
            f"written by tools/normals_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --warmup {a.warmup} --cpu-queries {a.cpu_queries}\n"
            + (a.note + "\n" if a.note else "") +
            "per job, in one process of its own, on two clouds -- export: the world-frame static export of the tracked batch; map: the points\n"
            "of the map accumulated from it (leaf 0.2) -- at radius 0.3 and 0.5, interleaved rounds:\n"
            "  nn           the same grid and the same 27 probes, only the nearest candidate kept -- the yardstick\n"
            "  query_order  the self form, a thread per query in the caller's order; normals + curvature\n"
            "  entry_order  the self form, a thread per grid entry\n"
            "ms = median of the stream-event times after the warm-up rounds, with minimum, maximum and spread = (max - min) / median.\n"
            "cpu_ms_per_query = the exhaustive one-thread helper (tests/helpers/normals_ref.cpp) on --cpu-queries queries against the whole\n"
            "cloud; cpu_ms_whole_cloud_extrapolated = that times the cloud's points (never run in full).  mean_k = neighbours per finite query.\n"
            "There is no pass or fail on time.  --scale is the fraction of the bench job's scans.  A job that is missing below was not measured.\n\n")
    with open(a.out, "w") as f:
        f.write(head)
    for kind in a.jobs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", kind, "--scale", str(a.scale), "--reps", str(a.reps), "--warmup", str(a.warmup),
               "--cpu-queries", str(a.cpu_queries)]
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
