#!/usr/bin/env python3
"""Development tool: what the ESF descriptor costs on the bench-shaped jobs -- scvod_batch_object_esf (k_esf, csrc/scvod_objesf.hip)
behind an object table with records and members, timed with stream events after a warm-up: at the defaults (20000 samples, every
class) with and without the 640-bin signatures, with cls_mask restricted to cars, next to scvod_batch_object_shapes on the same
table, and next to the CPU helper's single-thread loop (tests/helpers/object_esf_ref.cpp) on a sample of the same objects, scaled to
the table by valid-or-not sample count (every object draws the same number of samples).  Writes profiles/object_esf_cost.txt.
usage: python tools/object_esf_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--reps 3] [--cpu-objects 48] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import object_esf_ref as oer
import scvod_py
import synth
from objects_cost import JOBS, timed

CAR = 2  # scvod_object::cls of a car


def run(kind, scale, reps, cpu_objects, ref):
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
    ctx.batch_objects(d_off, rec, flags=scvod_py.OBJ_NO_TRACK, d_member_src=mem, stream=st)
    shp = torch.empty((max(k, 1), 96), dtype=torch.uint8, device="cuda")
    esf = torch.empty((max(k, 1), 64), dtype=torch.uint8, device="cuda")
    sig = torch.empty((max(k, 1), 640), dtype=torch.float32, device="cuda")
    p_all, p_car = scvod_py.esf_params_default(), scvod_py.esf_params_default(cls_mask=1 << CAR)
    cases = {
        "shapes": lambda: ctx.batch_object_shapes(shp, stream=st),
        "esf": lambda: ctx.batch_object_esf(esf, params=p_all, stream=st),
        "esf_sig": lambda: ctx.batch_object_esf(esf, sig, params=p_all, stream=st),
        "esf_cars": lambda: ctx.batch_object_esf(esf, params=p_car, stream=st),
    }
    out = dict(kind=kind, scans=count, points=n, objects=k, members=m)
    for name, fn in cases.items():
        med, lo, hi = timed(fn, reps)
        out[name] = dict(ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3))
        if name.startswith("esf"):
            out[name]["stats"] = ctx.esf_stats()
    out["scratch_bytes"] = ctx.esf_scratch_bytes()
    h = rec.cpu().numpy().reshape(-1).view(scvod_py.OBJECT_DTYPE)[:k]
    out["largest_object_points"] = int(h["n_points"].max()) if k else 0
    out["cars"] = int((h["cls"] == CAR).sum())
    # the CPU helper on every (k / cpu_objects)-th object, and the same objects' records from the device
    ctx.batch_object_esf(esf, params=p_all, stream=st)
    torch.cuda.synchronize()
    got = esf.cpu().numpy().reshape(-1).view(scvod_py.OBJECT_ESF_DTYPE)[:k]
    pick = np.unique(np.linspace(0, k - 1, min(cpu_objects, k)).astype(np.int64)) if k else []
    d_offs = torch.from_numpy(offs.astype(np.int64)).cuda()
    cpu_s, same = 0.0, 0
    for o in pick:
        r = h[o]
        idx = mem[int(r["point_begin"]):int(r["point_begin"]) + int(r["n_points"])].long() + d_offs[int(r["scan"])]
        xyz = d[idx][:, :3].cpu().numpy()
        t0 = time.perf_counter()
        w = oer.esf(ref, xyz, p_all.samples, p_all.seed, p_all.min_points)
        cpu_s += time.perf_counter() - t0
        same += int(w["record"].tobytes() == got[o].tobytes())
    out["cpu"] = dict(objects=len(pick), equal_records=same, ms_per_object=round(1e3 * cpu_s / max(len(pick), 1), 3),
                      ms_table=round(1e3 * cpu_s / max(len(pick), 1) * k, 1))
    out["speedup"] = round(out["cpu"]["ms_table"] / out["esf"]["ms"], 1) if out["esf"]["ms"] > 0 else None
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-objects", type=int, default=48, help="objects the CPU helper is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_esf_cost.txt"))
    a = ap.parse_args()
    scvod_py.load_lib()
    ref = oer.build(tempfile.mkdtemp(prefix="objesfref"))
    lines = ["ESF descriptor of the object table (scvod_batch_object_esf, k_esf): cost on the bench-shaped jobs",
             "=" * 110, "",
             f"python tools/object_esf_cost.py --jobs {a.jobs} --scale {a.scale} --reps {a.reps} --cpu-objects {a.cpu_objects} on "
             f"{torch.cuda.get_device_name(0)}: ms per call from stream events,",
             "median (min .. max) after one warm-up call; the table is built with SCVOD_OBJ_NO_TRACK; 20000 samples per object.", ""]
    for kind in a.jobs.split(","):
        r = run(kind, a.scale, a.reps, a.cpu_objects, ref)
        print(json.dumps(r), flush=True)
        f = lambda c: f"{r[c]['ms']:.3f} ({r[c]['ms_min']:.3f} .. {r[c]['ms_max']:.3f})"  # noqa: E731
        s, c = r["esf"]["stats"], r["esf_cars"]["stats"]
        lines += [f"{kind}: {r['scans']} scans, {r['points']} points, {r['objects']} objects ({r['cars']} cars), {r['members']} member points, "
                  f"largest object {r['largest_object_points']} points",
                  f"  scvod_batch_object_esf, defaults           {f('esf')}   {s['flagged']} flagged, {s['uncached']} objects beyond the "
                  f"on-chip cache, {s['valid_samples']} valid samples",
                  f"  ... with the 640-bin signatures            {f('esf_sig')}",
                  f"  ... cls_mask = cars alone                  {f('esf_cars')}   {c['masked']} objects left out",
                  f"  scvod_batch_object_shapes                  {f('shapes')}",
                  f"  CPU helper, one thread                     {r['cpu']['ms_per_object']:.3f} ms per object over {r['cpu']['objects']} objects "
                  f"spread over the table ({r['cpu']['equal_records']} records equal to the device's), {r['cpu']['ms_table']:.0f} ms for the table",
                  f"  speed-up over the CPU helper               {r['speedup']} x",
                  f"  scratch of the stage                       {r['scratch_bytes']} bytes", ""]
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
