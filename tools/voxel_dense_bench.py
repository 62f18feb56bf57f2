#!/usr/bin/env python3
"""Development tool: what the 4096 tier of the voxel stage costs on buckets whose largest voxel holds c points -- the measurement behind
kVxCountDense (scvod_k_voxels.inc).  A scan of 24 buckets of 3000 points each (one voxel of c points, the others over 700 voxels; crafted as
in tests/test_gpu_voxel_counting.py), 128 copies of it as one batch, hipEvent time of vx_bucket_4096 of the third run.  Run it on builds with
-DSCVOD_VOX_COUNT=0 (network), -DSCVOD_VOX_COUNT_DENSE=100000 (every bucket counts) and -DSCVOD_VOX_COUNT_DENSE=0 (every bucket counts its
keys, then sorts: what a bucket above the threshold pays), chosen with SCVOD_LIB.
usage: SCVOD_LIB=.../libscvod_x.so python tools/voxel_dense_bench.py [--copies 128] [--c 35 128 256 512 1024 2700]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=128)
    ap.add_argument("--buckets", type=int, default=24)
    ap.add_argument("--c", type=int, nargs="+", default=[35, 128, 256, 512, 1024, 2700])
    ap.add_argument("--dry", action="store_true", help="build the scans only (no device)")
    a = ap.parse_args()
    import scvod_py
    import test_gpu_voxel_counting as T
    P = scvod_py.make_params("semantickitti")
    grid = T._Grid(scvod_py, P)
    print(f"lib {os.environ.get('SCVOD_LIB', 'default')}: {a.copies} copies of a scan of {a.buckets} buckets of 3000 points")
    for c in a.c:
        x, _ = T._scan(grid, [(T._spread(3000, c, 700), False)] * a.buckets, 11)
        if a.dry:
            print(f"  c = {c:5d}: {len(x)} points per scan")
            continue
        import torch
        offs = (np.arange(a.copies + 1, dtype=np.int64) * len(x)).astype(np.int32)
        d = torch.from_numpy(np.tile(x, (a.copies, 1))).cuda().contiguous()
        ctx = scvod_py.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=a.copies)
        ctx.set_timing(1)
        for _ in range(3):
            ctx.batch_process(d, offs)
        t = dict(ctx.timings())
        pop = ctx.batch_counts()[0]
        ctx.close()
        print(f"  c = {c:5d}: vx_bucket_4096 {t.get('vx_bucket_4096', float('nan')):7.3f} ms   (2048: {t.get('vx_bucket_2048', float('nan')):.3f}, "
              f"8192: {t.get('vx_bucket_8192', float('nan')):.3f}, 1024: {t.get('vx_bucket_1024', float('nan')):.3f}; binned points of a scan: {int(pop[4])})")


if __name__ == "__main__":
    main()
