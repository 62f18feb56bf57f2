#!/usr/bin/env python3
"""Development tool, CPU only: what the merge-path levels (csrc/scvod_mergepath.h) would save in the large Patchwork sort tiers.
Patch populations (oracle Patchwork, planes.n_pts) of synthetic scans go through tests/helpers/mergepath_replay.cpp in its count
mode, which replays the kernel's schedule on keys with many z ties and counts key comparisons (a compare-exchange of the network
is one: a v_min_f64 plus a v_max_f64 on the device) and LDS key accesses.  Per tier and hand-over run length R: both per key, for
the whole sort by the network (R = -) and for the network up to runs of R followed by merge levels.
usage: python tests/devtools/merge_sort_count.py [--kind K64] [--preset semantickitti] [--scans 4]"""
import argparse
import collections
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
TIERS = (2048, 4096, 8192)  # tier of capacity c sorts patches of c / 2 <= n < c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="K64")
    ap.add_argument("--preset", default="semantickitti")
    ap.add_argument("--scans", type=int, default=4)
    a = ap.parse_args()
    import oracle_py
    import scvod_py
    import synth
    orc = oracle_py.load()
    P = scvod_py.make_params(a.preset)
    patches = []
    for i in range(a.scans):
        x = synth.make_scan(5, i * 7, a.kind)[0].numpy()
        n = orc.patchwork(P, x, 1)["planes"]["n_pts"]
        patches += n[(n >= TIERS[0] // 2) & (n < TIERS[-1])].tolist()
    print(f"{a.kind} {a.preset}: {a.scans} scans, {len(patches)} patches of {TIERS[0] // 2} .. {TIERS[-1] - 1} points")
    if not patches:
        return
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mergepath_replay")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "helpers", "mergepath_replay.cpp")])
        out = subprocess.run([exe, "count", "1", *map(str, patches)], capture_output=True, text=True, check=True).stdout
    tot = collections.defaultdict(lambda: np.zeros(3, np.int64))  # (tier, R) -> keys, comparisons, accesses
    count = collections.Counter()
    for l in out.split("\n"):
        if l.startswith("count "):
            n, run, cmp_, acc = map(int, l.split()[1:])
            tier = next(c for c in TIERS if n < c)
            tot[(tier, run)] += (n, cmp_, acc)
            count[tier] += run == 0
    print("  tier  patches  mean n     R   comparisons / key   LDS accesses / key   (merge / network)")
    for tier in TIERS:
        if not count[tier]:
            continue
        net = tot[(tier, 0)]
        for run in (0, 16, 32, 64, 128, 256, 512, 1024):
            k, c, s = tot[(tier, run)]
            rel = "" if run == 0 else f"   {c / net[1]:.2f} / {s / net[2]:.2f}"
            print(f"  {tier:4d} {count[tier]:8d} {k / count[tier]:7.0f} {run if run else '-':>5} {c / k:19.1f} {s / k:20.1f}{rel}")


if __name__ == "__main__":
    main()
