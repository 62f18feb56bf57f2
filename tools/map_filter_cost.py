#!/usr/bin/env python3
"""Development tool: what cleaning a batch against a prior map costs on the bench-shaped jobs -- scvod_batch_map_filter
(csrc/scvod_mapfilter.hip) next to the three existing calls that make the same passes, on one tracked batch in one process.  The prior
map is the batch's own static map, so most points are known and the objects vote on real member lists.
Timed in interleaved rounds (query, export, truth, side, all, vote, query, ...):
  query   (a) scvod_batch_map_query, radius --radius-share * leaf, d_result only                       yardstick of the probe
  export  (b) scvod_batch_export_points, every output (records, source indices, payload), sensor frame  yardstick of the partition
  truth   (c) scvod_batch_object_truth on the batch's object table                                      yardstick of the vote
  side    (d) scvod_batch_map_filter, d_side only
  all     (e) scvod_batch_map_filter, every output, no vote
  vote    (f) scvod_batch_map_filter, every output, with SCVOD_MAPF_OBJECT_VOTE and d_votes
Stream-event times; the median, minimum and maximum of --reps rounds after --warmup rounds.  `spread` of a row is (max - min) / median.
The aims: all <= query + export, and vote - all <= truth.  Writes one block per job to profiles/map_filter_cost.txt.
usage: python tools/map_filter_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 7] [--warmup 2] [--radius-share 0.99] [--note TEXT]"""
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
OUT = os.path.join(ROOT, "profiles", "map_filter_cost.txt")
LEAF = 0.2


def summary(ms):
    med = float(np.median(ms))
    return dict(ms=round(med, 3), ms_min=round(float(min(ms)), 3), ms_max=round(float(max(ms)), 3),
                spread=round((max(ms) - min(ms)) / max(med, 1e-9), 3))


def run(kind, scale, reps, warmup, radius_share):
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
    prior = scvod_py.StaticMap(cells, leaf=LEAF)
    prior.accumulate(ctx, poses, stream=st)
    n_cells = prior.count()
    # the object table: counted first, then with buffers that hold it
    d_oo = torch.empty(count + 1, dtype=torch.int32, device="cuda")
    ctx.batch_objects(d_oo, stream=st)
    ts = ctx.batch_objects_stats()
    n_obj, n_mem = int(ts["objects"]), int(ts["members"])
    d_obj = torch.empty((max(n_obj, 1), 64), dtype=torch.uint8, device="cuda")
    d_mem = torch.empty(max(n_mem, 1), dtype=torch.int32, device="cuda")
    ctx.batch_objects(d_oo, d_obj, d_member_src=d_mem, stream=st)
    ctx.batch_objects_stats()
    sizes = np.sort(d_obj.cpu().numpy().view(scvod_py.OBJECT_DTYPE).reshape(-1)["n_points"][:n_obj].astype(np.int64))
    skew = dict(objects=n_obj, members=n_mem)
    if n_obj:
        skew.update(median=int(sizes[n_obj // 2]), p99=int(sizes[min(n_obj - 1, (n_obj * 99) // 100)]), max=int(sizes[-1]),
                    rounds_of_64_mean=round(float(np.mean((sizes + 63) // 64)), 2), rounds_of_64_max=int((sizes[-1] + 63) // 64),
                    share_of_members_in_objects_above_4096=round(float(sizes[sizes > 4096].sum()) / max(n_mem, 1), 4))
    pay = torch.arange(n, dtype=torch.int32, device="cuda")
    gt = (pay % 7).contiguous()
    res = torch.empty(n, dtype=torch.uint8, device="cuda")
    side = torch.empty(n, dtype=torch.uint8, device="cuda")
    order = torch.empty(n, dtype=torch.int32, device="cuda")
    bounds = torch.empty((count, 2), dtype=torch.int32, device="cuda")
    xyzi = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    pay_out = torch.empty(n, dtype=torch.int32, device="cuda")
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    d_off = torch.empty(count + 1, dtype=torch.int32, device="cuda")
    truth = torch.empty((max(n_obj, 1), 32), dtype=torch.uint8, device="cuda")
    votes = torch.empty((max(n_obj, 1), 32), dtype=torch.uint8, device="cuda")
    lib, vp = prior.lib, scvod_py.C.c_void_p
    pp = poses.ctypes.data_as(vp)
    plain = scvod_py.map_filter_params_default(radius=RADIUS)
    voting = scvod_py.map_filter_params_default(radius=RADIUS, flags=scvod_py.MAPF_OBJECT_VOTE)
    byref = scvod_py.C.byref

    def p(t):
        return vp(t.data_ptr())

    def query():
        rc = lib.scvod_batch_map_query(ctx.h, prior.h, pp, RADIUS, None, p(res), None, None, None, None, vp(st))
        assert rc == 0, lib.scvod_map_last_error(prior.h).decode()

    def truth_call():
        rc = lib.scvod_batch_object_truth(ctx.h, p(gt), None, p(truth), n_obj, vp(st))
        assert rc == 0, lib.scvod_last_error(ctx.h).decode()

    def filt(par, outs, d_votes=None):
        rc = lib.scvod_batch_map_filter(ctx.h, prior.h, pp, byref(par), None, *outs, p(d_votes) if d_votes is not None else None,
                                        n_obj if d_votes is not None else 0, vp(st))
        assert rc == 0, lib.scvod_map_last_error(prior.h).decode()

    every = (p(res), p(side), p(order), p(bounds), p(xyzi), p(pay), p(pay_out))
    arms = (("query", query),
            ("export", lambda: ctx.batch_export_points(d_off, xyzi, d_payload_in=pay, d_payload_out=pay_out, d_src_out=src, stream=st)),
            ("truth", truth_call),
            ("side", lambda: filt(plain, (None, p(side), None, None, None, None, None))),
            ("all", lambda: filt(plain, every)),
            ("vote", lambda: filt(voting, every, votes)))
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
            if r == 0 and name in ("side", "all", "vote"):
                stats[name] = prior.filter_stats()
    out = dict(kind=kind, scans=count, points=n, map_cells=cells, cells=n_cells, leaf=LEAF, radius=round(RADIUS, 6), object_sizes=skew)
    for name in ms:
        out[name] = summary(ms[name])
    out["stats"] = stats
    out["filter_scratch_bytes"] = prior.filter_scratch_bytes()
    assert prior.count() == n_cells                                    # the filter moved nothing
    q, x, t, a, v = (out[k]["ms"] for k in ("query", "export", "truth", "all", "vote"))
    out["all_over_query_plus_export"] = round(a / max(q + x, 1e-9), 3)
    out["vote_minus_all_over_truth"] = round((v - a) / max(t, 1e-9), 3)
    out["side_over_query"] = round(out["side"]["ms"] / max(q, 1e-9), 3)
    prior.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radius-share", type=float, default=0.99, help="the radius of every map arm as a share of the leaf (at most 0.99)")
    ap.add_argument("--note", default="", help="a line for the head of the file (e.g. the build that was measured)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    scvod_py.load_lib()
    head = ("Cleaning a batch against a prior map (scvod_batch_map_filter, csrc/scvod_mapfilter.hip): cost on the bench-shaped jobs\n"
            f"written by tools/map_filter_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --warmup {a.warmup} "
            f"--radius-share {a.radius_share} on {torch.cuda.get_device_name(0)}\n"
            + (a.note + "\n" if a.note else "") +
            "per job, on one tracked batch in one process, the prior map = the batch's own static map, interleaved rounds:\n"
            "  query   (a) scvod_batch_map_query, radius --radius-share * leaf, d_result only\n"
            "  export  (b) scvod_batch_export_points, every output, sensor frame\n"
            "  truth   (c) scvod_batch_object_truth on the batch's object table\n"
            "  side    (d) scvod_batch_map_filter, d_side only\n"
            "  all     (e) scvod_batch_map_filter, every output, no vote\n"
            "  vote    (f) scvod_batch_map_filter, every output, the objects vote, d_votes\n"
            "ms = median of the stream-event times after the warm-up rounds, with minimum, maximum and spread = (max - min) / median.\n"
            "all_over_query_plus_export = (e) / ((a) + (b)); vote_minus_all_over_truth = ((f) - (e)) / (c): both aim at <= 1.\n"
            "object_sizes = the table's n_points (what one wave of the vote walks: rounds of 64 members).  stats = scvod_map_filter_stats\n"
            "of each filter arm.  --scale is the fraction of the bench job's scans.  A job that is missing below was not measured.\n\n")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(head)
    for kind in a.jobs.split(","):
        r = run(kind, a.scale, a.reps, a.warmup, a.radius_share)
        line = f"{kind}: {json.dumps(r)}"
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
