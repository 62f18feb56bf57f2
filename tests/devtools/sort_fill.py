#!/usr/bin/env python3
"""Development tool, CPU only: how full the LDS sort tiers are.  Patch populations (oracle Patchwork, planes.n_pts) and
voxel key-bucket populations (oracle binning, bucket = (key + key_off) >> shift as in scvod_capi.hip) of synthetic scans,
summed per network size np2: real keys / slots sorted by the padded network, and the share the pad-free network still
touches (keys rounded up to whole runs of 16 resp. 8).
usage: python tests/devtools/sort_fill.py [--kind K64] [--preset semantickitti] [--scans 4]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def table(name, pops, run, lo=64):
    pops = np.asarray([p for p in pops if p >= lo], np.int64)
    np2 = 1 << np.ceil(np.log2(pops)).astype(np.int64)
    print(f" {name}: {len(pops)} items of >= {lo} keys")
    print("    np2    items   keys/slots   whole runs/slots")
    for c in sorted(set(np2.tolist()), reverse=True):
        p = pops[np2 == c]
        live = (p + run - 1) // run * run
        print(f"  {c:6d} {len(p):7d}   {p.sum() / (c * len(p)):10.2f}   {live.sum() / (c * len(p)):16.2f}")


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
    lib = scvod_py.load_lib()
    r, s, z, b = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    lib.scvod_grid_dims(C.byref(P), C.byref(r), C.byref(s), C.byref(z), C.byref(b))
    key_off = r.value * s.value + s.value + 1
    shift = 12
    while ((b.value + key_off + 1) >> shift) + 1 > 1024:
        shift += 1
    patches, buckets = [], []
    for i in range(a.scans):
        x = synth.make_scan(5, i * 7, a.kind)[0].numpy()
        o = orc.patchwork(P, x, 1)
        patches += o["planes"]["n_pts"][o["planes"]["n_pts"] > 0].tolist()
        apri = orc.bin(P, x[o["nonground_idx"]], True)["apri"]
        buckets += np.bincount((apri["voxel_idx"].astype(np.int64) + key_off) >> shift).tolist()
    print(f"{a.kind} {a.preset}: {a.scans} scans")
    table("Patchwork patches (16 keys per thread)", patches, 16)
    table("voxel key buckets (8 keys per thread)", [p for p in buckets if p > 0], 8)


if __name__ == "__main__":
    main()
