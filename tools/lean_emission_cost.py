#!/usr/bin/env python3
"""Development tool: what the on-demand side of the lean emission costs.  A bench-shaped batch is processed in the default mode (lean
emission, lean voxel stage) with the per-kernel timing on; the first batch_fetch then runs k_apri_intensity ("emit_intensity"),
k_emit_lists ("emit_lists") and k_vx_descriptors for the whole batch.  Prints their hipEvent times next to the batch's own `emit`, and the same for a ctx forced eager.
usage: python tools/lean_emission_cost.py [--kind K64] [--scans 2761] [--reps 3]"""
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

JOBS = {"K64": ("semantickitti", 5), "PARK": ("parkinglot", 3), "OS128": ("os128_fine", 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="K64")
    ap.add_argument("--scans", type=int, default=2761)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    preset, seq = JOBS[a.kind]
    P = scvod_py.make_params(preset)
    scans = [synth.make_scan(seq, i, a.kind, device="cuda")[0] for i in range(a.scans)]
    d = torch.cat(scans).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    del scans
    out = dict(kind=a.kind, scans=a.scans, points=int(offs[-1]))
    for tag, mode in (("lean", 0), ("eager", 1)):
        ctx = scvod_py.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=a.scans)
        ctx.set_voxel_descriptors(mode)
        ctx.set_timing(True)
        rows = []
        for _ in range(a.reps + 1):
            ctx.batch_process(d, offs)
            ctx.batch_fetch(0)
            kt = {}
            for name, ms in ctx.timings():
                kt[name] = kt.get(name, 0.0) + ms
            rows.append(kt)
        rows = rows[1:]  # (the first pass warms up)
        out[tag] = {k: [round(r.get(k, 0.0), 3) for r in rows] for k in ("emit", "emit_intensity", "emit_lists", "vx_descriptors", "pw_fit_large", "pw_arrange")}
        out[tag]["binned_points"] = int(ctx.batch_counts()[:, 4].sum())
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
