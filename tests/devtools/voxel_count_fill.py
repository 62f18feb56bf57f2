#!/usr/bin/env python3
"""Development tool, CPU only: what placing the points of a voxel bucket by key counting would cost, per tier of k_vx_bucket.
Voxel keys of synthetic scans (oracle Patchwork + binning), buckets as in scvod_capi.hip (bucket = (key + key_off) >> shift).  A bucket of
m points whose voxels hold c_1 .. c_v points costs the counting form sum(c^2) reads of its LDS list (a point looks through its own voxel's
segment) next to a handful of accesses per key; the network costs every key 2 x passes LDS accesses whatever the voxels are
(sortnet::merge_passes of scvod_sortnet.h, + 1 pass for the runs sorted in registers).  Per tier: buckets, voxels per bucket, mean points
per voxel, the size-biased mean sum(c^2) / sum(c), the largest c, the share of buckets whose largest voxel exceeds 64 / 256 / 1024
points, and the network's accesses per key.
usage: python tests/devtools/voxel_count_fill.py [--kind K64] [--preset semantickitti] [--scans 4]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

TIERS = ((256, 3), (1024, 3), (2048, 3), (4096, 3), (8192, 3))   # (capacity, keys per thread = 2^lge); a tier takes m < cap, the last m <= cap


def merge_passes(lg_np2, lge):
    """sortnet::merge_passes"""
    return sum((r + lge - 1) // lge for r in range(lge + 1, lg_np2 + 1))


def network_accesses_per_key(cap, lge):
    return 2 * (merge_passes(int(np.log2(cap)), lge) + 1)


def tier_of(m):
    for i, (cap, _) in enumerate(TIERS):
        if m < cap or (i == len(TIERS) - 1 and m <= cap):
            return i
    return len(TIERS)   # oversize: sorted in arena memory


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
    rows = [[] for _ in range(len(TIERS) + 1)]   # per tier: (m, voxels, sum c^2, max c) of every bucket
    for i in range(a.scans):
        x = synth.make_scan(5, i * 7, a.kind)[0].numpy()
        o = orc.patchwork(P, x, 1)
        key = orc.bin(P, x[o["nonground_idx"]], True)["apri"]["voxel_idx"].astype(np.int64) + key_off
        vox, c = np.unique(key, return_counts=True)
        bucket = vox >> shift
        for bk in np.unique(bucket):
            cb = c[bucket == bk]
            rows[tier_of(int(cb.sum()))].append((int(cb.sum()), len(cb), int((cb * cb).sum()), int(cb.max())))
    print(f"{a.kind} {a.preset}: {a.scans} scans, a bucket spans {1 << shift} keys")
    print("   tier  buckets   points  vox/bucket  pts/vox  sum c^2/sum c  max c   >64   >256  >1024  network accesses/key")
    for t, rs in enumerate(rows):
        if not rs:
            continue
        q = np.asarray(rs, np.int64)
        name = f"{TIERS[t][0]:6d}" if t < len(TIERS) else "  over"
        net = f"{network_accesses_per_key(*TIERS[t]):3d}" if t < len(TIERS) else "  -"
        share = [f"{(q[:, 3] > lim).mean():5.3f}" for lim in (64, 256, 1024)]
        print(f" {name} {len(q):8d} {q[:, 0].sum():8d} {q[:, 1].mean():11.1f} {q[:, 0].sum() / q[:, 1].sum():8.2f} "
              f"{q[:, 2].sum() / q[:, 0].sum():14.1f} {q[:, 3].max():6d} {share[0]} {share[1]}  {share[2]}  {net}")


if __name__ == "__main__":
    main()
