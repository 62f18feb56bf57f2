#!/usr/bin/env python3
"""Development tool: what the cloud vote costs on the bench-shaped jobs and what it flags -- scvod_cloud_visibility_device
(csrc/scvod_cloudvis.hip: k_cvis_key, rocprim's radix sort, k_cvis_vote) on the representatives of the batch's static map (table-slot
order: spatially random) against the range images of ALL scans of the batch, next to the scan stage's scvod_batch_visibility with
SCVOD_VIS_WITH_GROUND (csrc/scvod_visibility.hip, the parent commit's kernels) as the yardstick.
One process per job; on one processed batch, timed in interleaved rounds (sorted, no_sort, half_range, sorted_no_scans,
no_sort_no_scans, scan_stage, sorted, ...):
  sorted            the default call: key, sort, vote; d_votes + d_verdict
  no_sort           SCVOD_CVIS_NO_SORT: chunks of consecutive map points in table-slot order
  half_range        sorted, max_range = max_dis / 2
  sorted_no_scans   the sorted call with n_scans = 0: key, sort, and the vote kernel's loads and write-back without a single scan
  no_sort_no_scans  the same without the sort; the difference of the two is the key and the sort alone
  scan_stage        scvod_batch_visibility, SCVOD_VIS_WITH_GROUND, d_votes + d_verdict, images in its scratch
Stream-event times; the median, minimum and maximum of --reps rounds after --warmup rounds.  `spread` of a row is (max - min) / median.
ns_per_pair: the time of an arm over its pairs that are not OUTSIDE (stats words 5..8); for the scan stage over all its pairs.
steps: stats word 9, the (chunk, scan) steps that were not skipped, next to chunks x n_scans.
The same run counts, on these SYNTHETIC jobs, the map cells whose representative is truth-moving (label & 0xFFFF in 252..259) and the
others that the cloud verdict flags, and the cells of either kind that remain in a map built from the points the per-scan verdict
(scvod_batch_visibility, defaults, along the job's successor table) does not flag.  Recorded, not asserted.  No hardware counters.
Writes one block per job to profiles/cloud_visibility_cost.txt.
usage: python tools/cloud_visibility_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 7] [--warmup 2] [--note TEXT]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))

JOBS = {"K64": ("semantickitti", 5, 2761, 5), "PARK": ("parkinglot", 3, 2000, 1), "OS128": ("os128_fine", 5, 1000, 5)}
OUT = os.path.join(ROOT, "profiles", "cloud_visibility_cost.txt")
LEAF = 0.2
CHUNK = 512


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
    print(f"{kind}: {count} scans, {n} points", file=sys.stderr, flush=True)
    ctx = scvod_py.Ctx(P, max_points_total=n + 64, max_scans=count)
    nxt = np.asarray([s + skip if s + skip < count else -1 for s in range(count)], np.int32)
    st = torch.cuda.current_stream().cuda_stream
    ctx.batch_process(d, offs, stream=st, sync=False)
    torch.cuda.synchronize()
    cls = labels.to(torch.int64) & 0xFFFF
    moving = ((cls >= 252) & (cls <= 259)).to(torch.uint8)
    del cls, labels
    # the per-scan verdict and the range images of every scan
    scan_out = ctx.batch_visibility(poses, nxt, flags=scvod_py.VIS_WITH_GROUND, want=("verdict", "images"), stream=st)
    images = scan_out["images"]
    byte = moving + 2 * (scan_out["verdict"] == scvod_py.VIS_SEEN_THROUGH).to(torch.uint8)   # bit 0: truth-moving, bit 1: flagged per scan
    cells = 1 << int(np.ceil(np.log2(max(n * 0.25, 1 << 22))))       # the benchmark's sizing
    full = scvod_py.StaticMap(cells, leaf=LEAF, kind=scvod_py.MAP_KIND_LABELLED)
    full.accumulate_labelled(d, byte, offs, poses, stream=st)
    pts, lab, _ = full.points_labelled(stream=st)
    pts, lab = pts.contiguous(), lab.contiguous()
    per_scan = scvod_py.StaticMap(cells, leaf=LEAF, kind=scvod_py.MAP_KIND_LABELLED)
    per_scan.accumulate_labelled(d, byte, offs, poses, keep=[0, 1], stream=st)
    _, lab_ps, _ = per_scan.points_labelled(stream=st)
    torch.cuda.synchronize()
    m = int(pts.shape[0])
    print(f"{kind}: {m} map points", file=sys.stderr, flush=True)
    _, S, A, _ = scvod_py.grid_dims(P)
    votes = torch.empty((m, 4), dtype=torch.int16, device="cuda")
    verdict = torch.empty(m, dtype=torch.uint8, device="cuda")
    s_votes = torch.empty(n, dtype=torch.int32, device="cuda")
    s_verdict = torch.empty(n, dtype=torch.uint8, device="cuda")
    prm = scvod_py.cloud_visibility_params_default()
    half = scvod_py.cloud_visibility_params_default(max_range=0.5 * float(P.max_dis))
    sprm = scvod_py.visibility_params_default()
    lib, vp = ctx.lib, scvod_py.C.c_void_p
    pp, pn = poses.ctypes.data_as(vp), nxt.ctypes.data_as(vp)

    def p(t):
        return vp(t.data_ptr())

    def cloud(params, flags, n_scans):
        rc = lib.scvod_cloud_visibility_device(ctx.h, p(pts), m, p(images) if n_scans else None, pp, n_scans, scvod_py.C.byref(params), flags,
                                               p(votes), p(verdict), vp(st))
        assert rc == 0, lib.scvod_last_error(ctx.h).decode()

    def scan_stage():
        rc = lib.scvod_batch_visibility(ctx.h, pp, pn, scvod_py.C.byref(sprm), scvod_py.VIS_WITH_GROUND, p(s_votes), p(s_verdict), None, None, vp(st))
        assert rc == 0, lib.scvod_last_error(ctx.h).decode()

    # (the scan stage writes its images into its own scratch: the cloud arms keep reading the tensor taken above)
    arms = (("sorted", lambda: cloud(prm, 0, count)),
            ("no_sort", lambda: cloud(prm, scvod_py.CVIS_NO_SORT, count)),
            ("half_range", lambda: cloud(half, 0, count)),
            ("sorted_no_scans", lambda: cloud(prm, 0, 0)),
            ("no_sort_no_scans", lambda: cloud(prm, scvod_py.CVIS_NO_SORT, 0)),
            ("scan_stage", scan_stage))
    ms = {name: [] for name, _ in arms}
    stats = {}
    for r in range(warmup + reps):
        print(f"{kind}: round {r}", file=sys.stderr, flush=True)
        for name, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms[name].append(e0.elapsed_time(e1))
            if r == 0:
                stats[name] = ctx.visibility_stats() if name == "scan_stage" else ctx.cloud_visibility_stats()
    chunks = -(-m // CHUNK)
    out = dict(kind=kind, scans=count, input_points=n, map_points=m, grid=[A, S], chunks=chunks, chunk_scan_steps=chunks * count,
               scratch_bytes=ctx.cloud_visibility_scratch_bytes())
    for name in ms:
        out[name] = summary(ms[name])
    out["stats"] = stats
    out["sort_alone_ms"] = round(out["sorted_no_scans"]["ms"] - out["no_sort_no_scans"]["ms"], 3)

    def live(s):
        return s["through"] + s["agree"] + s["occluded"] + s["empty"]
    out["ns_per_pair"] = {name: round(1e6 * out[name]["ms"] / max(live(stats[name]), 1), 5) for name in ("sorted", "no_sort", "half_range")}
    out["ns_per_pair"]["scan_stage"] = round(1e6 * out["scan_stage"]["ms"] / max(stats["scan_stage"]["pairs"], 1), 5)
    out["sorted_over_scan_stage_per_pair"] = round(out["ns_per_pair"]["sorted"] / max(out["ns_per_pair"]["scan_stage"], 1e-12), 3)
    out["steps_share"] = {name: round(stats[name]["steps"] / max(chunks * count, 1), 5) for name in ("sorted", "no_sort", "half_range")}
    out["live_pair_share"] = round(live(stats["sorted"]) / max(m * count, 1), 6)
    # what it flags
    cloud(prm, 0, count)
    torch.cuda.synchronize()
    mov = (lab & 1) != 0
    seen = verdict == scvod_py.VIS_SEEN_THROUGH
    tested = verdict != scvod_py.VIS_UNTESTED

    def c(t):
        return int(t.sum().item())
    out["flags"] = dict(moving_cells=c(mov), static_cells=c(~mov), moving_tested=c(mov & tested), static_tested=c(~mov & tested),
                        moving_seen_through=c(mov & seen), static_seen_through=c(~mov & seen),
                        per_scan_map_moving_cells=c((lab_ps & 1) != 0), per_scan_map_static_cells=c((lab_ps & 1) == 0))
    full.close()
    per_scan.close()
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
    head = ("Cloud vote (scvod_cloud_visibility_device, k_cvis_key + rocprim radix sort + k_cvis_vote in csrc/scvod_cloudvis.hip): cost on the bench-shaped jobs\n"
            f"written by tools/cloud_visibility_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --warmup {a.warmup}\n"
            + (a.note + "\n" if a.note else "") +
            "per job, one process, on one processed batch, interleaved rounds, the default parameters; the queries are the representatives of\n"
            "the batch's labelled map (all input points, 0.2 m cells) in table-slot order, the viewers ALL scans of the batch:\n"
            "  sorted            the default call: key, sort, vote; d_votes + d_verdict\n"
            "  no_sort           SCVOD_CVIS_NO_SORT\n"
            "  half_range        sorted, max_range = max_dis / 2\n"
            "  sorted_no_scans   the sorted call with n_scans = 0: key, sort, the vote kernel's loads and write-back\n"
            "  no_sort_no_scans  the same without the sort; sort_alone_ms is the difference of the two medians\n"
            "  scan_stage        scvod_batch_visibility, SCVOD_VIS_WITH_GROUND, defaults, d_votes + d_verdict (the parent commit's kernels)\n"
            "ms = median of the stream-event times after the warm-up rounds, with minimum, maximum and spread = (max - min) / median.\n"
            "stats = scvod_cloud_visibility_stats (scvod_visibility_stats for scan_stage) of the arm.  ns_per_pair = ms over the pairs that are\n"
            "not OUTSIDE (through + agree + occluded + empty); for scan_stage over all its pairs.  sorted_over_scan_stage_per_pair: the aim is <= 2.\n"
            "steps_share = stats word 9 over chunks x scans: the share of (chunk, scan) steps that were NOT skipped.  live_pair_share = pairs\n"
            "that are not OUTSIDE over map points x scans.  No hardware counters were taken.\n"
            "flags = map cells by the truth of their representative (moving: label & 0xFFFF in 252..259) that are tested and that get\n"
            "SCVOD_VIS_SEEN_THROUGH, and the cells of either kind left in a map built without the points the per-scan verdict flags.\n"
            "Synthetic scans: recorded, not asserted.  --scale is the fraction of the bench job's scans.  A job that is missing below was not measured.\n\n")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
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
