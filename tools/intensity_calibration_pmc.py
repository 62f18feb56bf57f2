#!/usr/bin/env python3
"""Development tool: the workload of a counter run of k_cal_knn -- two calibrated scvod_batch_process calls on a K64 job cut to
--scans scans (the first is the warm-up dispatch set).  Run it under the profiler, counters only, one pass per counter group:
  rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS \\
      --kernel-include-regex k_cal_knn --output-format csv -d OUT -- python tools/intensity_calibration_pmc.py
  rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_SALU SQ_ACTIVE_INST_VMEM SQ_LDS_BANK_CONFLICT SQ_THREAD_CYCLES_VALU ... (same)
  rocprofv3 --pmc FETCH_SIZE ... ; rocprofv3 --pmc WRITE_SIZE ...   (raw x 1024 B; reads x 2: profiles/r06_pmc_calibration.md)
SCVOD_CALIB_FORCE_FALLBACK=1 in front gives the one-thread-per-query baseline.  tools/intensity_calibration_pmc.py --summary CSV...
prints the per-dispatch means of the second half of the dispatches of every CSV."""
import argparse
import collections
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))


def summary(paths):
    for p in paths:
        d = collections.defaultdict(list)
        for r in csv.DictReader(open(p)):
            if "k_cal_knn" in r["Kernel_Name"]:
                d[r["Counter_Name"]].append(float(r["Counter_Value"]))
        print(p)
        for k, v in sorted(d.items()):
            w = v[len(v) // 2:]   # the second call's dispatches
            print(f"  {k:28s} dispatches {len(w):4d}  sum {sum(w):.6e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=280)
    ap.add_argument("--summary", nargs="*")
    a = ap.parse_args()
    if a.summary:
        return summary(a.summary)
    import numpy as np
    import torch
    import scvod_py
    import synth
    scvod_py.load_lib()
    P = scvod_py.make_params("semantickitti")
    scans = [synth.make_scan(5, i, "K64", device="cuda")[0] for i in range(a.scans)]
    d = torch.cat(scans).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    ctx = scvod_py.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=a.scans)
    ctx.set_intensity_calibration(True, 10, 200.0)
    for _ in range(2):
        ctx.batch_process(d, offs)
    st = ctx.batch_intensity_calibration_stats()
    print("queries", st["points"], "fallback", st["fallback_queries"], "candidates", ctx.batch_intensity_calibration_candidates(), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
