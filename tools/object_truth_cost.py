#!/usr/bin/env python3
"""Development tool: what the truth label of the table's objects costs on the bench-shaped jobs -- scvod_batch_object_truth
(csrc/scvod_objtruth.hip) with a seeded label per input point, next to scvod_batch_object_shapes of the same table, both behind an
object table with records and members.  Timed with stream events after a warm-up call each, the two calls taking turns inside every
round (one process, interleaved), medians of the rounds.  Two labellings: `palette` draws every point's label from twelve values on its
own (no two neighbours agree: the most combining work a realistic label volume gives a wave), `runs` gives runs of 64 input points one
label (what a labelled scene looks like).  The fallback counter of the stats is reported.  Writes profiles/object_truth_cost.txt.
usage: python tools/object_truth_cost.py [--jobs K64,PARK,OS128] [--scale 1.0] [--rounds 7] [--out FILE]"""
import argparse
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
from objects_cost import JOBS

SEED = 20261019
PALETTE = [0, 40, 48, 70, (1 << 16) | 10, (2 << 16) | 10, (1 << 16) | 252, (2 << 16) | 252, (1 << 16) | 253, (3 << 16) | 259, (1 << 16) | 30,
           0xFFFFFFFF]


def labels(n, how):
    g = torch.Generator(device="cuda")
    g.manual_seed(SEED)
    pal = torch.tensor(np.array(PALETTE, np.uint32).view(np.int32), device="cuda")
    m = n if how == "palette" else (n + 63) // 64
    lab = pal[torch.randint(0, len(PALETTE), (m,), generator=g, device="cuda")]
    if how == "runs":
        lab = lab.repeat_interleave(64)[:n]
    return lab.contiguous()


def interleaved(fns, rounds):
    """{name: (median, min, max) ms}: one warm-up call each, then `rounds` rounds in which the calls take turns"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ms.items()}


def run(kind, scale, rounds):
    preset, seq, count, skip = JOBS[kind]
    count = max(skip + 1, int(count * scale))
    P = scvod_py.make_params(preset)
    scans = [synth.make_scan(seq, i, kind, device="cuda") for i in range(count)]
    d = torch.cat([s[0] for s in scans]).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(s[0]) for s in scans])]).astype(np.int32)
    del scans
    n = int(offs[-1])
    print(f"{kind}: {count} scans, {n} points", file=sys.stderr, flush=True)
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
    tru = torch.empty((max(k, 1), 32), dtype=torch.uint8, device="cuda")
    ctx.batch_objects(d_off, rec, flags=scvod_py.OBJ_NO_TRACK, d_member_src=mem, stream=st)
    gt = {how: labels(n, how) for how in ("palette", "runs")}

    def truth(how):
        ctx._chk(ctx.lib.scvod_batch_object_truth(ctx.h, gt[how].data_ptr(), None, tru.data_ptr(), k, st))

    t = interleaved({"shapes": lambda: ctx.batch_object_shapes(shp, stream=st), "truth_palette": lambda: truth("palette"),
                     "truth_runs": lambda: truth("runs")}, rounds)
    out = dict(kind=kind, scans=count, points=n, objects=k, members=m)
    for name, (med, lo, hi) in t.items():
        out[name] = dict(ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3))
    for how in ("palette", "runs"):
        truth(how)
        s1 = ctx.batch_object_truth_stats()
        assert s1["written"] == s1["objects"] == k
        out["stats_" + how] = s1
        out["ratio_" + how] = round(out["truth_" + how]["ms"] / out["shapes"]["ms"], 3)
    h = tru.cpu().numpy().reshape(-1).view(scvod_py.OBJECT_TRUTH_DTYPE)[:k]
    out["largest_object_points"] = int(h["n_points"].max()) if k else 0
    out["most_distinct_labels_runs"] = int(h["n_distinct"].max()) if k else 0
    out["scratch_bytes"] = ctx.batch_object_truth_scratch_bytes()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="K64,PARK,OS128")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_truth_cost.txt"))
    a = ap.parse_args()
    scvod_py.load_lib()
    lines = ["Truth label of the table's objects (scvod_batch_object_truth, csrc/scvod_objtruth.hip): cost on the bench-shaped jobs",
             "=" * 110, "",
             f"python tools/object_truth_cost.py --jobs {a.jobs} --scale {a.scale} --rounds {a.rounds} on {torch.cuda.get_device_name(0)}: ms per call "
             "from stream events,", f"median (min .. max) of {a.rounds} rounds in which the calls take turns, after one warm-up call each; the table is "
             "built with SCVOD_OBJ_NO_TRACK.", "palette: every point draws one of twelve labels on its own; runs: 64 consecutive input points share "
             "a label.", ""]
    for kind in a.jobs.split(","):
        r = run(kind, a.scale, a.rounds)
        print(json.dumps(r), flush=True)
        f = lambda c: f"{r[c]['ms']:.3f} ({r[c]['ms_min']:.3f} .. {r[c]['ms_max']:.3f})"  # noqa: E731
        lines += [f"{kind}: {r['scans']} scans, {r['points']} points, {r['objects']} objects, {r['members']} member points, largest object "
                  f"{r['largest_object_points']} points, scratch {r['scratch_bytes']} bytes",
                  f"  scvod_batch_object_shapes           {f('shapes')}",
                  f"  scvod_batch_object_truth, palette   {f('truth_palette')}   = {r['ratio_palette']:.3f} x shapes, fallback objects "
                  f"{r['stats_palette']['fallback_objects']}, moving points {r['stats_palette']['moving_points']}, in objects "
                  f"{r['stats_palette']['moving_members']}",
                  f"  scvod_batch_object_truth, runs      {f('truth_runs')}   = {r['ratio_runs']:.3f} x shapes, fallback objects "
                  f"{r['stats_runs']['fallback_objects']}, most distinct labels in one object {r['most_distinct_labels_runs']}", ""]
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
