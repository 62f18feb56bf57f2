#!/usr/bin/env python3
"""Development tool: what the seen-through vote costs on the bench-shaped jobs and what it flags -- scvod_batch_visibility
(csrc/scvod_visibility.hip, k_vis_image + k_vis_vote) with the default parameters next to scvod_batch_map_query at radius 0, byte only
(csrc/scvod_mapquery.hip): per point one transform and one random probe, the same kind of work as one (point, viewer) pair.
One process per job; on one tracked batch, timed in interleaved rounds (image, vote, vote_images, vote_ground, own, image, ...):
  image        scvod_batch_visibility with SCVOD_VIS_IMAGES_ONLY: the +inf fill and k_vis_image alone, images in the scratch
  vote         scvod_batch_visibility, queries = Patchwork's non-ground list, d_votes + d_verdict, images in the scratch
  vote_images  the same with d_images as well
  vote_ground  SCVOD_VIS_WITH_GROUND: every input point is a query (no mask), d_votes + d_verdict
  own          scvod_batch_map_query, radius 0, d_result only, against a map that holds the batch
Stream-event times; the median, minimum and maximum of --reps rounds after --warmup rounds.  `spread` of a row is (max - min) / median.
The viewers follow the job's successor table (scan s -> s + skip: the interleaved chains of the benchmark).
The same run counts the truth-moving points (label & 0xFFFF in 252..259) and the others that get SCVOD_VIS_SEEN_THROUGH, that
scvod_batch_point_labels marks DYNAMIC on the same tracked batch, and that either does.  Recorded, not asserted.
Writes one block per job to profiles/visibility_cost.txt.
usage: python tools/visibility_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 7] [--warmup 2] [--note TEXT]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))

JOBS = {"K64": ("semantickitti", 5, 2761, 5), "PARK": ("parkinglot", 3, 2000, 1), "OS128": ("os128_fine", 5, 1000, 5)}
OUT = os.path.join(ROOT, "profiles", "visibility_cost.txt")
LEAF = 0.2


def summary(ms):
    med = float(np.median(ms))
    return dict(ms=round(med, 3), ms_min=round(float(min(ms)), 3), ms_max=round(float(max(ms)), 3),
                spread=round((max(ms) - min(ms)) / max(med, 1e-9), 3))


def run(kind, scale, reps, warmup):
    import torch
    import scvod_py
    import synth
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
    full = scvod_py.StaticMap(cells, leaf=LEAF)
    full.accumulate(ctx, poses, stream=st)
    _, S, A, _ = scvod_py.grid_dims(P)
    votes = torch.empty(n, dtype=torch.int32, device="cuda")
    verdict = torch.empty(n, dtype=torch.uint8, device="cuda")
    images = torch.empty((count, A, S), dtype=torch.float32, device="cuda")
    res = torch.empty(n, dtype=torch.uint8, device="cuda")
    prm = scvod_py.visibility_params_default()
    lib, vp = ctx.lib, scvod_py.C.c_void_p
    pp, pn = poses.ctypes.data_as(vp), nxt.ctypes.data_as(vp)

    def p(t):
        return vp(t.data_ptr())

    def vote(flags, outs):
        rc = lib.scvod_batch_visibility(ctx.h, pp, pn, scvod_py.C.byref(prm), flags, *outs, vp(st))
        assert rc == 0, lib.scvod_last_error(ctx.h).decode()

    def own():
        rc = lib.scvod_batch_map_query(ctx.h, full.h, pp, 0.0, None, p(res), None, None, None, None, vp(st))
        assert rc == 0, lib.scvod_map_last_error(full.h).decode()

    arms = (("image", lambda: vote(scvod_py.VIS_IMAGES_ONLY, (None, None, None, None))),
            ("vote", lambda: vote(0, (p(votes), p(verdict), None, None))),
            ("vote_images", lambda: vote(0, (p(votes), p(verdict), p(images), None))),
            ("vote_ground", lambda: vote(scvod_py.VIS_WITH_GROUND, (p(votes), p(verdict), None, None))),
            ("own", own))
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
            if r == 0 and name in ("vote", "vote_ground"):
                stats[name] = ctx.visibility_stats()
    out = dict(kind=kind, scans=count, points=n, grid=[A, S], skip=skip, scratch_bytes=ctx.visibility_scratch_bytes())
    for name in ms:
        out[name] = summary(ms[name])
    out["stats"] = stats
    v = stats["vote"]["pairs"] / max(stats["vote"]["queries"], 1)
    out["viewers_per_query"] = round(v, 3)
    out["vote_over_own"] = round(out["vote"]["ms"] / max(out["own"]["ms"], 1e-9), 3)
    out["vote_over_viewers_x_own"] = round(out["vote"]["ms"] / max(v * out["own"]["ms"], 1e-9), 3)
    out["ns_per_pair"] = {name: round(1e6 * out[name]["ms"] / max(stats[name]["pairs"], 1), 5) for name in ("vote", "vote_ground")}
    # what it flags, next to the tracking's verdict on the same batch
    vote(0, (p(votes), p(verdict), None, None))
    pt = ctx.batch_point_labels(stream=st)
    torch.cuda.synchronize()
    cls = labels.to(torch.int64) & 0xFFFF
    moving = (cls >= 252) & (cls <= 259)
    seen = verdict == scvod_py.VIS_SEEN_THROUGH
    dyn = pt[:n] == scvod_py.PT_DYNAMIC
    query = verdict != scvod_py.VIS_UNTESTED

    def c(t):
        return int(t.sum().item())
    out["flags"] = dict(moving=c(moving), static=c(~moving), moving_queries=c(moving & query), static_queries=c(~moving & query),
                        moving_seen_through=c(moving & seen), static_seen_through=c(~moving & seen),
                        moving_dynamic=c(moving & dyn), static_dynamic=c(~moving & dyn),
                        moving_either=c(moving & (seen | dyn)), static_either=c(~moving & (seen | dyn)))
    full.close()
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
    head = ("Seen-through points (scvod_batch_visibility, k_vis_image + k_vis_vote in csrc/scvod_visibility.hip): cost on the bench-shaped jobs\n"
            f"written by tools/visibility_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --warmup {a.warmup}\n"
            + (a.note + "\n" if a.note else "") +
            "per job, one process, on one tracked batch, interleaved rounds, the default parameters (2 viewers on each side, halo 0):\n"
            "  image        SCVOD_VIS_IMAGES_ONLY: the +inf fill and k_vis_image alone, images in the scratch\n"
            "  vote         queries = Patchwork's non-ground list, d_votes + d_verdict, images in the scratch\n"
            "  vote_images  the same with d_images as well\n"
            "  vote_ground  SCVOD_VIS_WITH_GROUND: every input point is a query, d_votes + d_verdict\n"
            "  own          scvod_batch_map_query, radius 0, d_result only, against a map that holds the batch\n"
            "ms = median of the stream-event times after the warm-up rounds, with minimum, maximum and spread = (max - min) / median.\n"
            "stats = scvod_visibility_stats of the arm.  vote_over_viewers_x_own = vote / (viewers_per_query * own): the aim is <= 1.\n"
            "flags = input points by truth (moving: label & 0xFFFF in 252..259) that are queries, that get SCVOD_VIS_SEEN_THROUGH, that\n"
            "scvod_batch_point_labels marks DYNAMIC on the same batch, and that either does.  Synthetic scans: recorded, not asserted.\n"
            "--scale is the fraction of the bench job's scans.  A job that is missing below was not measured.\n\n")
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
