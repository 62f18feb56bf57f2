#!/usr/bin/env python3
"""Development tool: what the recognised map costs on the bench-shaped jobs -- scvod_batch_map_accumulate_classes (csrc/scvod_map.hip,
k_map_accumulate_labelled) next to scvod_batch_map_accumulate (k_map_accumulate) on the same tracked batch, with the same flags, into
maps of the same capacity, in the same process: the plain accumulate is the yardstick, never the new kernel against itself.
Four things are timed, in interleaved rounds (plain, classes, bytes, kernel, plain, ...), each into a map cleared just before the
first event:
  plain    scvod_batch_map_accumulate                       the yardstick
  classes  scvod_batch_map_accumulate_classes               the class bytes pass + the labelled kernel
  bytes    scvod_batch_point_classes alone                  the pass the batch form adds
  kernel   scvod_map_accumulate_labelled on the same cloud  the labelled kernel alone, on bytes computed beforehand
Stream-event times; the median, minimum and maximum of --reps rounds after --warmup rounds.  `spread` of a row is (max - min) / median.
Writes one block per job to profiles/class_map_cost.txt.
usage: python tools/class_map_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 7] [--warmup 2] [--flags 0]"""
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
OUT = os.path.join(ROOT, "profiles", "class_map_cost.txt")
LEAF = 0.2


def keep_table(flags):
    """the keep table scvod_batch_map_accumulate_classes states for flags without a part"""
    t = np.zeros(256, np.uint8)
    t[[3, 4, 5, 7]] = 1
    t[1] = 0 if flags & scvod_py.MAP_NO_GROUND else 1
    t[2] = 0 if flags & scvod_py.MAP_NO_REJECTED else 1
    t[6] = 1 if flags & scvod_py.MAP_IGNORE_DYNAMIC else 0
    return t


def summary(ms):
    med = float(np.median(ms))
    return dict(ms=round(med, 3), ms_min=round(float(min(ms)), 3), ms_max=round(float(max(ms)), 3),
                spread=round((max(ms) - min(ms)) / max(med, 1e-9), 3))


def run(kind, scale, reps, warmup, flags):
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
    ctx.set_region_growing(True)
    ctx.batch_cluster_types(stream=st, sync=False)
    ctx.batch_track(T, next_scan=nxt, stream=st, sync=False)
    torch.cuda.synchronize()
    cells = 1 << int(np.ceil(np.log2(max(n * 0.25, 1 << 22))))       # the benchmark's sizing
    plain = scvod_py.StaticMap(cells, leaf=LEAF)
    lab = scvod_py.StaticMap(cells, leaf=LEAF, kind=scvod_py.MAP_KIND_LABELLED)
    lab2 = scvod_py.StaticMap(cells, leaf=LEAF, kind=scvod_py.MAP_KIND_LABELLED)
    d_cls = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
    d_cls2 = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
    ctx.batch_point_classes(d_cls, stream=st)
    keep = keep_table(flags)
    arms = (("plain", plain, lambda: plain.accumulate(ctx, poses, flags=flags, stream=st)),
            ("classes", lab, lambda: lab.accumulate_classes(ctx, poses, flags=flags, stream=st)),
            ("bytes", None, lambda: ctx.batch_point_classes(d_cls2, stream=st)),
            ("kernel", lab2, lambda: lab2.accumulate_labelled(d, d_cls, offs, poses, keep=keep, stream=st)))
    ms = {name: [] for name, _, _ in arms}
    for r in range(warmup + reps):
        for name, m, fn in arms:
            if m is not None:
                m.clear(stream=st)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    out = dict(kind=kind, scans=count, points=n, flags=flags, map_cells=cells, leaf=LEAF)
    for name in ms:
        out[name] = summary(ms[name])
    n_plain, n_lab, n_lab2 = plain.count(), lab.count(), lab2.count()
    assert n_plain == n_lab == n_lab2, (n_plain, n_lab, n_lab2)       # the same cells, whichever way they were accumulated
    out["cells"] = n_plain
    out["scratch_bytes"] = lab.scratch_bytes()
    p, k, c, b = out["plain"], out["kernel"], out["classes"], out["bytes"]
    out["kernel_over_plain"] = round(k["ms"] / max(p["ms"], 1e-9), 3)
    out["classes_over_plain"] = round(c["ms"] / max(p["ms"], 1e-9), 3)
    noise = max(p["ms_max"] - p["ms_min"], k["ms_max"] - k["ms_min"])
    if k["ms"] - p["ms"] > noise:
        out["verdict"] = (f"the labelled kernel alone is slower than the plain one by {k['ms'] - p['ms']:.3f} ms, beyond the run-to-run spread "
                          f"({noise:.3f} ms): the time is in the kernel's own phase (stream + label byte + probes), not in the bytes pass")
    else:
        out["verdict"] = (f"the labelled kernel alone is not slower than the plain one beyond the run-to-run spread ({noise:.3f} ms); the batch "
                          f"call costs {c['ms'] - k['ms']:.3f} ms more than the kernel, the bytes pass alone takes {b['ms']:.3f} ms")
    for m in (plain, lab, lab2):
        m.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--flags", type=int, default=0, help="SCVOD_MAP_NO_GROUND | NO_REJECTED | IGNORE_DYNAMIC, the same for every arm")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    assert not a.flags & ~7, "no part flags here"
    scvod_py.load_lib()
    head = ("The recognised map (scvod_batch_map_accumulate_classes, k_map_accumulate_labelled in csrc/scvod_map.hip): cost on the bench-shaped jobs\n"
            f"written by tools/class_map_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --warmup {a.warmup} --flags {a.flags} on "
            f"{torch.cuda.get_device_name(0)}\n"
            "per job, on one tracked batch (region growing on) in one process, interleaved rounds, every map cleared before its timed call:\n"
            "  plain    scvod_batch_map_accumulate -- the yardstick\n"
            "  classes  scvod_batch_map_accumulate_classes (the class bytes pass + the labelled kernel)\n"
            "  bytes    scvod_batch_point_classes alone\n"
            "  kernel   scvod_map_accumulate_labelled on the same cloud with bytes computed beforehand (the labelled kernel alone)\n"
            "ms = median of the stream-event times after the warm-up rounds, with minimum, maximum and spread = (max - min) / median.\n"
            "--scale is the fraction of the bench job's scans.  A job that is missing below was not measured.\n\n")
    with open(a.out, "w") as f:
        f.write(head)
    for kind in a.jobs.split(","):
        r = run(kind, a.scale, a.reps, a.warmup, a.flags)
        line = json.dumps(r)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(f"{kind}: {line}\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
