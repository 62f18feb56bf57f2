#!/usr/bin/env python3
"""Development tool: what the tracks' vote on the seen-through verdict costs on the bench-shaped jobs -- scvod_track_visibility_device
(k_tv_* in csrc/scvod_trackvis.hip) behind the whole recipe on one tracked batch: scvod_batch_visibility, scvod_batch_objects with the
per-point object index, scvod_batch_object_visibility, scvod_batch_object_tracks.  Timed in interleaved rounds:
  whole     records + the per-point bytes into a buffer of their own, default parameters
  records   the two record tables only (no d_verdict_out): k_tv_world / member / track / spread
  paint     the per-point bytes only (no record buffers)
  window2   as whole with window = 2
  ov        yardstick 1: scvod_batch_object_visibility on the same batch (default flags, records + a separate d_verdict_out), row (b) of
            tools/object_visibility_cost.py
  copy      yardstick 2: one device-to-device hipMemcpyAsync of 3 bytes per input point, which reads 3 and writes 3: the 6 bytes per
            point k_tv_paint moves (4 of d_point_object and 1 of d_verdict read, 1 written)
Stream-event times; the median, minimum and maximum of --reps rounds after --warmup rounds.  k_tv_paint alone is taken as whole -
records (difference of the medians); its rate is 6 bytes per point over that time, the copy's rate 6 bytes per point over its own.
The aims: whole <= ov, and paint_rate / copy_rate >= 0.6 (the "hbm" class of profiles/r06_kernel_table.md).  No hardware counters.
The same run counts, among the queries of the per-point vote, the truth-moving points (label & 0xFFFF in 252..259) and the others that
carry SCVOD_VIS_SEEN_THROUGH before the stage (after the objects' vote), after it with the defaults, with SCVOD_TRKVIS_CLEAR and with
window = 2.  Synthetic scans, untuned defaults: recorded, not asserted; the figures say nothing about real data.
Writes one block per job to profiles/track_visibility_cost.txt; one process per job.
usage: python tools/track_visibility_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 7] [--warmup 2] [--note TEXT]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))

JOBS = {"K64": ("semantickitti", 5, 2761, 5), "PARK": ("parkinglot", 3, 2000, 1), "OS128": ("os128_fine", 5, 1000, 5)}
OUT = os.path.join(ROOT, "profiles", "track_visibility_cost.txt")


def summary(ms):
    med = float(np.median(ms))
    return dict(ms=round(med, 3), ms_min=round(float(min(ms)), 3), ms_max=round(float(max(ms)), 3))


def run(kind, scale, reps, warmup):
    import torch
    import scvod_py
    import synth
    C = scvod_py.C
    preset, seq, count, skip = JOBS[kind]
    count = max(skip + 1, int(count * scale))
    P = scvod_py.make_params(preset)
    scans = []
    for i in range(count):
        scans.append(synth.make_scan(seq, i, kind, device="cuda"))
        if i % 500 == 499:
            print(f"{kind}: {i + 1} of {count} scans made", file=sys.stderr, flush=True)
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
    d_off = torch.empty(count + 1, dtype=torch.int32, device="cuda")
    ctx.batch_objects(d_off, stream=st)
    ts = ctx.batch_objects_stats()
    k, m = int(ts["objects"]), int(ts["members"])
    d_obj = torch.empty((max(k, 1), 64), dtype=torch.uint8, device="cuda")
    d_mem = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
    d_po = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
    ctx.batch_objects(d_off, d_obj, d_member_src=d_mem, d_point_object=d_po, stream=st)
    ctx.batch_objects_stats()
    vis = ctx.batch_visibility(poses, nxt, want=("votes", "verdict"), stream=st)
    obj = ctx.batch_object_visibility(vis["verdict"], vis["votes"], d_obj, cap=max(k, 1), stream=st)
    trk = ctx.batch_object_tracks(d_obj, poses, cap_links=k, cap_tracks=k, stream=st)
    print(f"{kind}: {n} points, {k} objects: the recipe ran", file=sys.stderr, flush=True)
    tracks = ctx.object_tracks_stats()
    before = obj["verdict"]
    out_bytes = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
    ov_bytes = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
    ov_rec = torch.empty((max(k, 1), 48), dtype=torch.uint8, device="cuda")
    tv = torch.empty((max(k, 1), 32), dtype=torch.uint8, device="cuda")
    ovt = torch.empty((max(k, 1), 16), dtype=torch.uint8, device="cuda")
    src3 = torch.empty(3 * max(n, 1), dtype=torch.uint8, device="cuda")
    dst3 = torch.empty(3 * max(n, 1), dtype=torch.uint8, device="cuda")
    src3.zero_()
    lib, vp, byref = ctx.lib, C.c_void_p, C.byref
    pp = poses.ctypes.data_as(vp)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    hip.hipMemcpyAsync.restype = C.c_int

    def p(t):
        return vp(t.data_ptr())

    def call(prm, records=True, paint=True, dst=out_bytes):
        rc = lib.scvod_track_visibility_device(ctx.h, p(d_obj), p(d_off), count, pp, p(trk["links"]), k, p(trk["tracks"]), k, p(trk["track_objects"]),
                                               p(trk["n_tracks"]), p(obj["records"]), p(d_po), p(before), p(dst) if paint else None, n, byref(prm),
                                               p(tv) if records else None, k, p(ovt) if records else None, k, vp(st))
        assert rc == 0, lib.scvod_last_error(ctx.h).decode()

    def ov():
        prm = scvod_py.object_visibility_params_default()
        rc = lib.scvod_batch_object_visibility(ctx.h, p(vis["verdict"]), None, None, byref(prm), p(ov_rec), k, p(ov_bytes), vp(st))
        assert rc == 0, lib.scvod_last_error(ctx.h).decode()

    def copy():
        assert hip.hipMemcpyAsync(p(dst3), p(src3), 3 * n, 3, vp(st)) == 0      # 3: hipMemcpyDeviceToDevice

    dflt = scvod_py.track_visibility_params_default()
    win2 = scvod_py.track_visibility_params_default(window=2)
    arms = (("whole", lambda: call(dflt)), ("records", lambda: call(dflt, paint=False)), ("paint", lambda: call(dflt, records=False)),
            ("window2", lambda: call(win2)), ("ov", ov), ("copy", copy))
    ms = {name: [] for name, _ in arms}
    for r in range(warmup + reps):
        for name, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    out = dict(kind=kind, scans=count, points=n, skip=skip, objects=k, tracks=tracks["tracks"], longest=tracks["longest"],
               scratch_bytes=ctx.track_visibility_scratch_bytes())
    for name in ms:
        out[name] = summary(ms[name])
    kernel = max(out["whole"]["ms"] - out["records"]["ms"], 1e-9)
    out["paint_kernel_ms"] = round(kernel, 3)
    out["paint_GBps"] = round(6.0 * n / kernel * 1e-6, 1)
    out["copy_GBps"] = round(6.0 * n / max(out["copy"]["ms"], 1e-9) * 1e-6, 1)
    out["paint_over_copy_rate"] = round(out["paint_GBps"] / max(out["copy_GBps"], 1e-9), 3)
    out["whole_over_ov"] = round(out["whole"]["ms"] / max(out["ov"]["ms"], 1e-9), 3)
    # what is flagged, by truth, before and after the stage
    cls = labels.to(torch.int64) & 0xFFFF
    moving = (cls >= 252) & (cls <= 259)
    query = vis["verdict"] != scvod_py.VIS_UNTESTED

    def count_flags(t):
        seen = (t[:n] == scvod_py.VIS_SEEN_THROUGH) & query
        return dict(moving=int((moving & seen).sum().item()), static=int((~moving & seen).sum().item()))
    flags = dict(moving_queries=int((moving & query).sum().item()), static_queries=int((~moving & query).sum().item()),
                 before=count_flags(before))
    stats = {}
    for name, kw in (("defaults", dict()), ("clear", dict(flags=scvod_py.TRKVIS_CLEAR)), ("window2", dict(window=2)),
                     ("window2_clear", dict(window=2, flags=scvod_py.TRKVIS_CLEAR))):
        call(scvod_py.track_visibility_params_default(**kw))
        stats[name] = ctx.track_visibility_stats()
        flags[name] = count_flags(out_bytes)
    out["flags"], out["stats"] = flags, stats
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
    head = ("The tracks' vote on the seen-through verdict (scvod_track_visibility_device, k_tv_* in csrc/scvod_trackvis.hip): cost on the\n"
            "bench-shaped jobs\n"
            f"written by tools/track_visibility_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --warmup {a.warmup}\n"
            + (a.note + "\n" if a.note else "") +
            "per job, one process, behind the whole recipe on one tracked batch, interleaved rounds:\n"
            "  whole     records + per-point bytes into a buffer of their own, default parameters\n"
            "  records   the two record tables only          paint     the per-point bytes only          window2   whole with window = 2\n"
            "  ov        yardstick 1: scvod_batch_object_visibility on the same batch, records + a separate d_verdict_out\n"
            "  copy      yardstick 2: one device-to-device hipMemcpyAsync of 3 bytes per input point (3 read + 3 written = the 6 bytes per\n"
            "            point k_tv_paint moves)\n"
            "ms = median of the stream-event times after the warm-up rounds, with minimum and maximum.  paint_kernel_ms = whole - records;\n"
            "paint_GBps and copy_GBps are 6 bytes per point over paint_kernel_ms and over the copy's ms.  The aims: whole_over_ov <= 1 and\n"
            "paint_over_copy_rate >= 0.6.  No hardware counters were taken.\n"
            "flags = the queries of the per-point vote by truth (moving: label & 0xFFFF in 252..259) that carry SCVOD_VIS_SEEN_THROUGH before\n"
            "the stage (after the objects' vote with its defaults) and after it with the defaults, with SCVOD_TRKVIS_CLEAR, with window = 2\n"
            "and with both; stats = scvod_track_visibility_stats of those calls.  Synthetic scans, untuned defaults: recorded, not asserted;\n"
            "they say nothing about real data.  --scale is the fraction of the bench job's scans.  A job that is missing below was not measured.\n\n")
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
