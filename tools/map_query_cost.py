#!/usr/bin/env python3
"""Development tool: what asking the static map costs on the bench-shaped jobs -- scvod_batch_map_query / scvod_map_query
(csrc/scvod_mapquery.hip, k_mq_query) next to the plain scvod_batch_map_accumulate (csrc/scvod_map.hip, k_map_accumulate) of the same
tracked batch into a map of the same capacity, in the same process, and next to the route a caller had to take before:
scvod_map_split_device on the exported map.
Timed in interleaved rounds (accumulate, again, own, count, near, all, free_all, split, accumulate, ...):
  accumulate  scvod_batch_map_accumulate into a map cleared just before the first event        the yardstick of the other map tools
  again       the same call into the map that already holds the batch: every probe finds its cell, no insertion (the like-for-like
              of a query: the accumulate's probes WITH its value test, against the query's without)
  own         scvod_batch_map_query, radius 0, d_result only, against that map
  count       scvod_batch_map_query, radius 0, d_scan_counts only: the same probes without the byte per point
  near        scvod_batch_map_query, radius --radius-share * leaf, d_result only
  all         scvod_batch_map_query, radius --radius-share * leaf, every output
  free_all    scvod_map_query, radius --radius-share * leaf, d_result + the nn pair, of the world-frame export of the first --split-share of the
              scans (identity pose)
  split       scvod_map_split_device: base = the exported map's points, query = that same export, d_mark + the nn pair
Stream-event times; the median, minimum and maximum of --reps rounds after --warmup rounds.  `spread` of a row is (max - min) / median.
Writes one block per job to profiles/map_query_cost.txt.
usage: python tools/map_query_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 7] [--warmup 2] [--split-share 0.1] [--radius-share 0.99] [--note TEXT]"""
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
OUT = os.path.join(ROOT, "profiles", "map_query_cost.txt")
LEAF = 0.2


def summary(ms):
    med = float(np.median(ms))
    return dict(ms=round(med, 3), ms_min=round(float(min(ms)), 3), ms_max=round(float(max(ms)), 3),
                spread=round((max(ms) - min(ms)) / max(med, 1e-9), 3))


def run(kind, scale, reps, warmup, split_share, radius_share):
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
    fresh = scvod_py.StaticMap(cells, leaf=LEAF)
    full = scvod_py.StaticMap(cells, leaf=LEAF)
    full.accumulate(ctx, poses, stream=st)
    n_cells = full.count()
    base, _ = full.points(stream=st)
    base = base.contiguous()
    # the world-frame export of the first scans: the cloud both routes are asked about
    d_off = torch.empty(count + 1, dtype=torch.int32, device="cuda")
    xyzi = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    ctx.batch_export_points(d_off, xyzi, poses=poses, stream=st)
    torch.cuda.synchronize()
    k = max(1, int(count * split_share))
    kept = int(d_off[count].item())                                  # the points the accumulate offers the table; a query asks about all n
    eoff = d_off.cpu().numpy()[:k + 1].astype(np.int32)
    nq = int(eoff[-1])
    query = xyzi[:nq].clone()
    del xyzi
    res = torch.empty(n, dtype=torch.uint8, device="cuda")
    val = torch.empty(n, dtype=torch.int64, device="cuda")
    key = torch.empty(n, dtype=torch.int64, device="cuda")
    sq = torch.empty(n, dtype=torch.float32, device="cuda")
    cnt = torch.empty((count, 4), dtype=torch.int64, device="cuda")
    mark = torch.empty(max(n_cells, 1), dtype=torch.uint8, device="cuda")
    nn_idx = torch.empty(max(nq, 1), dtype=torch.int32, device="cuda")
    nn_sq = torch.empty(max(nq, 1), dtype=torch.float32, device="cuda")
    sp = scvod_py.split_params_default(cell=LEAF)
    lib, vp = full.lib, scvod_py.C.c_void_p
    pp, po = poses.ctypes.data_as(vp), eoff.ctypes.data_as(vp)

    def p(t):
        return vp(t.data_ptr())

    def batch_query(radius, outs):
        rc = lib.scvod_batch_map_query(ctx.h, full.h, pp, radius, None, *outs, vp(st))
        assert rc == 0, lib.scvod_map_last_error(full.h).decode()

    def free_query():
        rc = lib.scvod_map_query(full.h, p(query), po, k, None, RADIUS, None, p(res), None, p(key), p(sq), None, vp(st))
        assert rc == 0, lib.scvod_map_last_error(full.h).decode()

    arms = (("accumulate", lambda: fresh.accumulate(ctx, poses, stream=st)),
            ("again", lambda: full.accumulate(ctx, poses, stream=st)),
            ("own", lambda: batch_query(0.0, (p(res), None, None, None, None))),
            ("count", lambda: batch_query(0.0, (None, None, None, None, p(cnt)))),
            ("near", lambda: batch_query(RADIUS, (p(res), None, None, None, None))),
            ("all", lambda: batch_query(RADIUS, (p(res), p(val), p(key), p(sq), p(cnt)))),
            ("free_all", free_query),
            ("split", lambda: ctx.map_split_device(base, query, params=sp, d_mark=mark, d_nn_idx=nn_idx, d_nn_sqdist=nn_sq, stream=st)))
    ms = {name: [] for name, _ in arms}
    stats = {}
    for r in range(warmup + reps):
        for name, fn in arms:
            if name == "accumulate":
                fresh.clear(stream=st)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms[name].append(e0.elapsed_time(e1))
            if r == 0 and name in ("own", "near", "all", "free_all"):
                stats[name] = full.query_stats()
    out = dict(kind=kind, scans=count, points=n, kept_points=kept, map_cells=cells, cells=n_cells, leaf=LEAF, radius=round(RADIUS, 6), export_scans=k,
               export_points=nq)
    for name in ms:
        out[name] = summary(ms[name])
    out["stats"] = stats
    out["split_stats"] = ctx.map_split_stats()
    assert fresh.count() == n_cells == full.count()                   # the queries moved nothing
    a, g, o = out["accumulate"], out["again"], out["own"]
    out["own_over_accumulate"] = round(o["ms"] / max(a["ms"], 1e-9), 3)
    out["own_over_again"] = round(o["ms"] / max(g["ms"], 1e-9), 3)
    out["free_all_over_split"] = round(out["free_all"]["ms"] / max(out["split"]["ms"], 1e-9), 3)
    out["Mpoints_per_ms"] = {name: round(n / 1e6 / max(out[name]["ms"], 1e-9), 1) for name in ("accumulate", "again", "own", "count", "near", "all")}
    for m in (fresh, full):
        m.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--split-share", type=float, default=0.1, help="share of the scans whose export is the cloud of free_all and split")
    ap.add_argument("--radius-share", type=float, default=0.99, help="the radius of near / all / free_all as a share of the leaf (at most 0.99)")
    ap.add_argument("--note", default="", help="a line for the head of the file (e.g. the build that was measured)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    scvod_py.load_lib()
    head = ("Asking the static map (scvod_batch_map_query / scvod_map_query, k_mq_query in csrc/scvod_mapquery.hip): cost on the bench-shaped jobs\n"
            f"written by tools/map_query_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --warmup {a.warmup} --split-share {a.split_share} "
            f"--radius-share {a.radius_share} on "
            f"{torch.cuda.get_device_name(0)}\n"
            + (a.note + "\n" if a.note else "") +
            "per job, on one tracked batch in one process, interleaved rounds:\n"
            "  accumulate  scvod_batch_map_accumulate into a map cleared before the timed call -- the yardstick\n"
            "  again       the same call into the map that already holds the batch (probes and value tests, no insertion)\n"
            "  own         scvod_batch_map_query, radius 0, d_result only\n"
            "  count       scvod_batch_map_query, radius 0, d_scan_counts only (the same probes without the byte per point)\n"
            "  near        scvod_batch_map_query, radius --radius-share * leaf, d_result only\n"
            "  all         scvod_batch_map_query, radius --radius-share * leaf, every output\n"
            "  free_all    scvod_map_query, radius --radius-share * leaf, d_result + nn pair, of the world-frame export of the first scans\n"
            "  split       scvod_map_split_device, base = the map's points, query = that export, d_mark + nn pair (the route before)\n"
            "ms = median of the stream-event times after the warm-up rounds, with minimum, maximum and spread = (max - min) / median.\n"
            "kept_points = the points the accumulate offers the table (a query asks about all of `points`).  stats = {points, cell, near, miss, out}\n"
            "of each query arm.  --scale is the fraction of the bench job's scans.  A job that is\n"
            "missing below was not measured.\n\n")
    with open(a.out, "w") as f:
        f.write(head)
    for kind in a.jobs.split(","):
        r = run(kind, a.scale, a.reps, a.warmup, a.split_share, a.radius_share)
        line = f"{kind}: {json.dumps(r)}"
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
