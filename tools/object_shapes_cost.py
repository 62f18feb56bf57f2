#!/usr/bin/env python3
"""Development tool: what the eigenvalue descriptor costs on the bench-shaped jobs -- scvod_batch_object_shapes (k_obj_shape,
csrc/scvod_objects.hip) behind an object table with records and members, timed with stream events after a warm-up, next to that table
call and to the part of it that k_obj_reduce and k_obj_voxels add (records + members minus members only) in the same run.  With
--kernel-stats (the kernel_stats CSV of a run of this tool under rocprofv3 --kernel-trace --stats) the per-kernel averages of
k_obj_reduce and k_obj_shape are added.  Writes profiles/object_shapes_cost.txt.
usage: python tools/object_shapes_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 5] [--out FILE] [--kernel-stats CSV]"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scvod_py
import synth
from objects_cost import JOBS, timed


def run(kind, scale, reps):
    preset, seq, count, skip = JOBS[kind]
    count = max(skip + 1, int(count * scale))
    P = scvod_py.make_params(preset)
    scans = [synth.make_scan(seq, i, kind, device="cuda") for i in range(count)]
    d = torch.cat([s[0] for s in scans]).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(s[0]) for s in scans])]).astype(np.int32)
    del scans
    n = int(offs[-1])
    ctx = scvod_py.Ctx(P, max_points_total=n + 64, max_scans=count)
    st = torch.cuda.current_stream().cuda_stream
    ctx.batch_process(d, offs, stream=st, sync=False)
    ctx.batch_cluster(stream=st, sync=False)
    ctx.batch_cluster_types(stream=st, sync=False)
    d_off = torch.empty(count + 1, dtype=torch.int32, device="cuda")
    ctx.batch_objects(d_off, None, flags=scvod_py.OBJ_NO_TRACK, stream=st)
    s0 = ctx.batch_objects_stats()
    k, m = s0["objects"], s0["members"]
    rec = torch.empty((max(k, 1), 64), dtype=torch.uint8, device="cuda")
    mem = torch.empty(max(m, 1), dtype=torch.int32, device="cuda")
    shp = torch.empty((max(k, 1), 96), dtype=torch.uint8, device="cuda")
    cases = {
        "members_only": lambda: ctx.batch_objects(d_off, None, flags=scvod_py.OBJ_NO_TRACK, d_member_src=mem, stream=st),
        "records_members": lambda: ctx.batch_objects(d_off, rec, flags=scvod_py.OBJ_NO_TRACK, d_member_src=mem, stream=st),
        "shapes": lambda: ctx.batch_object_shapes(shp, stream=st),
    }
    out = dict(kind=kind, scans=count, points=n, objects=k, members=m)
    for name, fn in cases.items():
        med, lo, hi = timed(fn, reps)
        out[name] = dict(ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3))
    out["reduce_and_voxels_ms"] = round(out["records_members"]["ms"] - out["members_only"]["ms"], 3)
    s1 = ctx.batch_object_shapes_stats()
    assert s1["written"] == s1["objects"] == k
    out["not_finite"] = s1["not_finite"]
    h = rec.cpu().numpy().reshape(-1).view(scvod_py.OBJECT_DTYPE)[:k]
    out["largest_object_points"] = int(h["n_points"].max()) if k else 0
    ctx.close()
    return out


def kernel_lines(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if "k_obj_reduce" in r.get("Name", "") or "k_obj_shape" in r.get("Name", ""):
                name = "k_obj_reduce" if "k_obj_reduce" in r["Name"] else "k_obj_shape"
                rows.append(f"  {name}: calls {r.get('Calls')}, average {float(r.get('AverageNs', 'nan')) / 1e6:.3f} ms, "
                            f"min {float(r.get('MinNs', 'nan')) / 1e6:.3f} ms, max {float(r.get('MaxNs', 'nan')) / 1e6:.3f} ms")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_shapes_cost.txt"))
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats CSV of a rocprofv3 --kernel-trace --stats run of this tool")
    a = ap.parse_args()
    scvod_py.load_lib()
    lines = ["Eigenvalue descriptor of the object table (scvod_batch_object_shapes, k_obj_shape): cost on the bench-shaped jobs",
             "=" * 110, "",
             f"python tools/object_shapes_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} on {torch.cuda.get_device_name(0)}: ms per call "
             "from stream events,", "median (min .. max) after one warm-up call; the table is built with SCVOD_OBJ_NO_TRACK.", ""]
    for kind in a.jobs.split(","):
        r = run(kind, a.scale, a.reps)
        print(json.dumps(r), flush=True)
        f = lambda c: f"{r[c]['ms']:.3f} ({r[c]['ms_min']:.3f} .. {r[c]['ms_max']:.3f})"  # noqa: E731
        lines += [f"{kind}: {r['scans']} scans, {r['points']} points, {r['objects']} objects, {r['members']} member points, largest object "
                  f"{r['largest_object_points']} points, {r['not_finite']} objects with a feature that is not finite",
                  f"  scvod_batch_object_shapes            {f('shapes')}",
                  f"  scvod_batch_objects records+members  {f('records_members')}",
                  f"  scvod_batch_objects members only     {f('members_only')}",
                  f"  difference (k_obj_voxels + k_obj_reduce) {r['reduce_and_voxels_ms']:.3f}", ""]
        torch.cuda.empty_cache()
    if a.kernel_stats:
        lines += ["per kernel, from a run of this tool under rocprofv3 --kernel-trace --stats (all jobs and calls together):"] + kernel_lines(a.kernel_stats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
