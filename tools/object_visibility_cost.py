#!/usr/bin/env python3
"""Development tool: what the objects' vote on the seen-through verdict costs on the bench-shaped jobs -- scvod_batch_object_visibility
(k_ov_tiles + k_ov_straddle in csrc/scvod_objvis.hip), which cuts the table's sorted member list into tiles, next to the vote of
scvod_batch_map_filter (k_mf_vote in csrc/scvod_mapfilter.hip), which gives one wave a whole object, on the SAME object table of one
tracked batch in one process.  The verdict bytes and pair counters are what scvod_batch_visibility wrote for the batch.
Timed in interleaved rounds (mf_all, mf_vote, ov, ov_pool, ov_place, ov_sums, mf_all, ...):
  mf_all    scvod_batch_map_filter, every output, no vote                                  (e) of tools/map_filter_cost.py
  mf_vote   the same with SCVOD_MAPF_OBJECT_VOTE and d_votes                               (f) of tools/map_filter_cost.py
  (a)       mf_vote - mf_all: k_mf_vote on this table (difference of the medians)
  ov        (b) scvod_batch_object_visibility, default flags, no d_votes, records + a separate d_verdict_out: k_mf_vote's gathers
  ov_pool   (c) the same with d_votes and SCVOD_OBJVIS_POOL_PAIRS: one more 4-byte gather per member
  ov_place  (d) as (b), in place, no records
  ov_sums   as (b) with d_votes: the four sums are recorded, the bytes decide
Stream-event times; the median, minimum and maximum of --reps rounds after --warmup rounds.  `spread` of a row is (max - min) / median.
The aim: ov_over_mf_vote = (b) / (a) <= 1.  No hardware counters are taken.
The same run counts, among the queries of the per-point vote (Patchwork's non-ground points), the truth-moving points (label & 0xFFFF
in 252..259) and the others that carry SCVOD_VIS_SEEN_THROUGH before the objects vote, after the vote with the defaults, and after the
vote with SCVOD_OBJVIS_WITH_TRACK; next to them what scvod_batch_point_labels marks DYNAMIC and what either cue marks.  Synthetic scans:
recorded, not asserted; the figures say nothing about real data.
Writes one block per job to profiles/object_visibility_cost.txt; one process per job.
usage: python tools/object_visibility_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 7] [--warmup 2] [--note TEXT]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))

JOBS = {"K64": ("semantickitti", 5, 2761, 5), "PARK": ("parkinglot", 3, 2000, 1), "OS128": ("os128_fine", 5, 1000, 5)}
OUT = os.path.join(ROOT, "profiles", "object_visibility_cost.txt")
LEAF = 0.2


def summary(ms):
    med = float(np.median(ms))
    return dict(ms=round(med, 3), ms_min=round(float(min(ms)), 3), ms_max=round(float(max(ms)), 3),
                spread=round((max(ms) - min(ms)) / max(med, 1e-9), 3))


def run(kind, scale, reps, warmup):
    import torch
    import scvod_py
    import synth
    C = scvod_py.C
    preset, seq, count, skip = JOBS[kind]
    count = max(skip + 1, int(count * scale))
    P = scvod_py.make_params(preset)
    scans = [synth.make_scan(seq, i, kind, device="cuda") for i in range(count)]
    d = torch.cat([s[0] for s in scans]).contiguous()
    labels = torch.cat([s[1] for s in scans]).contiguous()
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
    # the object table: counted first, then with buffers that hold it
    d_oo = torch.empty(count + 1, dtype=torch.int32, device="cuda")
    ctx.batch_objects(d_oo, stream=st)
    ts = ctx.batch_objects_stats()
    n_obj, n_mem = int(ts["objects"]), int(ts["members"])
    d_obj = torch.empty((max(n_obj, 1), 64), dtype=torch.uint8, device="cuda")
    d_mem = torch.empty(max(n_mem, 1), dtype=torch.int32, device="cuda")
    ctx.batch_objects(d_oo, d_obj, d_member_src=d_mem, stream=st)
    ctx.batch_objects_stats()
    del d_mem
    begin = d_obj.cpu().numpy().view(scvod_py.OBJECT_DTYPE).reshape(-1)[:n_obj]
    sizes = np.sort(begin["n_points"].astype(np.int64))
    first, last = begin["point_begin"].astype(np.int64) // scvod_py.OBJVIS_TILE, \
        (begin["point_begin"].astype(np.int64) + begin["n_points"] - 1) // scvod_py.OBJVIS_TILE
    skew = dict(objects=n_obj, members=n_mem, tiles=int((n_mem + scvod_py.OBJVIS_TILE - 1) // scvod_py.OBJVIS_TILE),
                objects_across_a_tile_edge=int((last > first).sum()))
    if n_obj:
        skew.update(median=int(sizes[n_obj // 2]), max=int(sizes[-1]), rounds_of_64_max=int((sizes[-1] + 63) // 64),
                    share_of_members_in_objects_above_4096=round(float(sizes[sizes > 4096].sum()) / max(n_mem, 1), 4))
    # the per-point vote of the batch: the input of the stage
    vis = ctx.batch_visibility(poses, nxt, want=("votes", "verdict"), stream=st)
    verdict, votes = vis["verdict"], vis["votes"]
    torch.cuda.synchronize()
    pay = torch.arange(n, dtype=torch.int32, device="cuda")
    res = torch.empty(n, dtype=torch.uint8, device="cuda")
    side = torch.empty(n, dtype=torch.uint8, device="cuda")
    order = torch.empty(n, dtype=torch.int32, device="cuda")
    bounds = torch.empty((count, 2), dtype=torch.int32, device="cuda")
    xyzi = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    pay_out = torch.empty(n, dtype=torch.int32, device="cuda")
    mf_votes = torch.empty((max(n_obj, 1), 32), dtype=torch.uint8, device="cuda")
    rec = torch.empty((max(n_obj, 1), 48), dtype=torch.uint8, device="cuda")
    out_bytes = torch.empty(n, dtype=torch.uint8, device="cuda")
    place = torch.empty(n, dtype=torch.uint8, device="cuda")
    lib, vp, byref = ctx.lib, C.c_void_p, C.byref
    pp = poses.ctypes.data_as(vp)
    radius = float(np.float32(0.99) * np.float32(LEAF))
    plain = scvod_py.map_filter_params_default(radius=radius)
    voting = scvod_py.map_filter_params_default(radius=radius, flags=scvod_py.MAPF_OBJECT_VOTE)

    def p(t):
        return vp(t.data_ptr())

    every = (p(res), p(side), p(order), p(bounds), p(xyzi), p(pay), p(pay_out))

    def filt(par, d_votes=None):
        rc = lib.scvod_batch_map_filter(ctx.h, prior.h, pp, byref(par), None, *every, p(d_votes) if d_votes is not None else None,
                                        n_obj if d_votes is not None else 0, vp(st))
        assert rc == 0, lib.scvod_map_last_error(prior.h).decode()

    def ov(flags, d_in, d_rec, d_out, with_objects=False, with_votes=False):
        prm = scvod_py.object_visibility_params_default(flags=flags)
        rc = lib.scvod_batch_object_visibility(ctx.h, p(d_in), p(votes) if with_votes else None, p(d_obj) if with_objects else None, byref(prm),
                                               p(d_rec) if d_rec is not None else None, n_obj if d_rec is not None else 0,
                                               p(d_out) if d_out is not None else None, vp(st))
        assert rc == 0, lib.scvod_last_error(ctx.h).decode()

    def ov_place():
        ov(0, place, None, place)

    arms = (("mf_all", lambda: filt(plain)), ("mf_vote", lambda: filt(voting, mf_votes)),
            ("ov", lambda: ov(0, verdict, rec, out_bytes)), ("ov_pool", lambda: ov(scvod_py.OBJVIS_POOL_PAIRS, verdict, rec, out_bytes, with_votes=True)),
            ("ov_place", ov_place), ("ov_sums", lambda: ov(0, verdict, rec, out_bytes, with_votes=True)))
    ms = {name: [] for name, _ in arms}
    stats = {}
    for r in range(warmup + reps):
        for name, fn in arms:
            if name == "ov_place":
                place.copy_(verdict)                                   # (outside the timed span: every round votes on the same bytes)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms[name].append(e0.elapsed_time(e1))
            if r == 0 and name.startswith("ov"):
                stats[name] = ctx.batch_object_visibility_stats()
    out = dict(kind=kind, scans=count, points=n, skip=skip, object_sizes=skew, scratch_bytes=ctx.batch_object_visibility_scratch_bytes())
    for name in ms:
        out[name] = summary(ms[name])
    a = out["mf_vote"]["ms"] - out["mf_all"]["ms"]
    out["mf_vote_minus_mf_all_ms"] = round(a, 3)
    out["ov_over_mf_vote"] = round(out["ov"]["ms"] / max(a, 1e-9), 3)
    out["ov_pool_over_mf_vote"] = round(out["ov_pool"]["ms"] / max(a, 1e-9), 3)
    out["ov_place_over_mf_vote"] = round(out["ov_place"]["ms"] / max(a, 1e-9), 3)
    out["stats"] = stats
    # what is flagged, by truth, before and after the objects vote
    ov(0, verdict, None, out_bytes)
    voted = out_bytes.clone()
    ov(scvod_py.OBJVIS_WITH_TRACK, verdict, None, out_bytes, with_objects=True)
    stats["with_track"] = ctx.batch_object_visibility_stats()
    pt = ctx.batch_point_labels(stream=st)
    torch.cuda.synchronize()
    cls = labels.to(torch.int64) & 0xFFFF
    moving = (cls >= 252) & (cls <= 259)
    query = verdict != scvod_py.VIS_UNTESTED
    seen = verdict == scvod_py.VIS_SEEN_THROUGH
    seen_vote = (voted == scvod_py.VIS_SEEN_THROUGH) & query
    seen_track = (out_bytes == scvod_py.VIS_SEEN_THROUGH) & query
    dyn = (pt[:n] == scvod_py.PT_DYNAMIC) & query

    def c(t):
        return int(t.sum().item())
    out["flags"] = dict(moving_queries=c(moving & query), static_queries=c(~moving & query),
                        moving_seen_through=c(moving & seen), static_seen_through=c(~moving & seen),
                        moving_dynamic=c(moving & dyn), static_dynamic=c(~moving & dyn),
                        moving_either=c(moving & (seen | dyn)), static_either=c(~moving & (seen | dyn)),
                        moving_after_vote=c(moving & seen_vote), static_after_vote=c(~moving & seen_vote),
                        moving_after_vote_with_track=c(moving & seen_track), static_after_vote_with_track=c(~moving & seen_track))
    prior.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--note", default="", help="a line for the head of the file (e.g. the build that was measured)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", default="", help="internal: run this one job and print its line")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(run(a.child, a.scale, a.reps, a.warmup)), flush=True)
        return
    head = ("The objects' vote on the seen-through verdict (scvod_batch_object_visibility, k_ov_tiles + k_ov_straddle in csrc/scvod_objvis.hip):\n"
            "cost on the bench-shaped jobs\n"
            f"written by tools/object_visibility_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --warmup {a.warmup}\n"
            + (a.note + "\n" if a.note else "") +
            "per job, one process, on one tracked batch and its object table, interleaved rounds:\n"
            "  mf_all    scvod_batch_map_filter, every output, no vote (the prior map = the batch's own static map, radius 0.99 leaf)\n"
            "  mf_vote   the same with SCVOD_MAPF_OBJECT_VOTE and d_votes\n"
            "  (a)       mf_vote_minus_mf_all_ms: k_mf_vote, one wave per object, on this table\n"
            "  ov        (b) scvod_batch_object_visibility, default flags, no d_votes, records + a separate d_verdict_out: k_mf_vote's gathers\n"
            "  ov_pool   (c) the same with d_votes and SCVOD_OBJVIS_POOL_PAIRS: one more 4-byte gather per member\n"
            "  ov_place  (d) as (b), in place, no records\n"
            "  ov_sums   as (b) with d_votes: the four sums are recorded, the bytes decide\n"
            "ms = median of the stream-event times after the warm-up rounds, with minimum, maximum and spread = (max - min) / median.\n"
            "ov_over_mf_vote = (b) / (a), and the same for (c) and (d): the aim is (b) / (a) <= 1.  No hardware counters were taken.\n"
            "object_sizes = the table (objects_across_a_tile_edge: decided by k_ov_straddle).  stats = scvod_batch_object_visibility_stats.\n"
            "flags = the queries of the per-point vote (Patchwork's non-ground points) by truth (moving: label & 0xFFFF in 252..259) that\n"
            "carry SCVOD_VIS_SEEN_THROUGH before the objects vote, that scvod_batch_point_labels marks DYNAMIC, that either marks, and that\n"
            "carry SCVOD_VIS_SEEN_THROUGH after the vote with the defaults and after the vote with SCVOD_OBJVIS_WITH_TRACK.  Synthetic\n"
            "scans: recorded, not asserted; they say nothing about real data.\n"
            "--scale is the fraction of the bench job's scans.  A job that is missing below was not measured.\n\n")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(head)
    for kind in a.jobs.split(","):
        # a process per job: a fresh device context, nothing left over from the job before
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--scale", str(a.scale), "--reps", str(a.reps),
                            "--warmup", str(a.warmup)], stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        line = f"{kind}: {lines[-1][7:]}" if r.returncode == 0 and lines else f"{kind}: failed with status {r.returncode}"
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        if r.returncode != 0:   # (nothing more is started on a device a job has failed on)
            sys.exit(1)


if __name__ == "__main__":
    main()
