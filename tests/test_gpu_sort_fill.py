"""The LDS sort tiers at partial fill: the pad-free network (csrc/scvod_sortnet.h) touches only the whole
runs below a patch's key count, so the sizes that matter are those around half, three quarters and all
of a tier's capacity, one run (16 or 8 keys) either side of a run boundary, and a small item that a
persistent workgroup sorts right after a large one.  Everything against the oracle, exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAPS = (256, 1024, 2048, 4096, 8192)


def _fill_sizes(c):
    return [c // 2 + 1, c // 2 + 15, c // 2 + 16, c // 2 + 17, 3 * c // 4 - 1, 3 * c // 4, 3 * c // 4 + 1,
            c - 17, c - 16, c - 15, c - 1]


def _check_pw(orc, P, x, r, tag):
    """ground and non-ground lists and planes of one scan, exact (the Patchwork part of test_gpu_parity._check_scan)"""
    o = orc.patchwork(P, x, 1)
    assert np.array_equal(r["cls"], o["cls"]), f"{tag} cls"
    assert np.array_equal(r["ground_idx"], o["ground_idx"]), f"{tag} ground order"
    assert np.array_equal(r["nonground_idx"], o["nonground_idx"]), f"{tag} nonground order"
    assert r["planes"].shape == o["planes"].shape
    for f in ("n_pts", "n_ground", "status"):
        assert np.array_equal(r["planes"][f], o["planes"][f]), f"{tag} planes.{f}"
    live = o["planes"]["status"] > 0
    for f in ("normal", "mean", "sv"):
        assert np.array_equal(r["planes"][f][live].view(np.uint32), o["planes"][f][live].view(np.uint32)), f"{tag} planes.{f}"
    return o


def _patch(rng, n, sector=0):
    """n points inside ring 0 of one sector of the innermost zone (16 sectors), with z ties and duplicated points"""
    ang = sector * (2 * np.pi / 16) + rng.uniform(0.02, 0.37, n)
    rad = rng.uniform(3.2, 6.8, n)
    z = np.round(rng.normal(-1.7, 0.04, n), 2)
    x = np.stack([rad * np.cos(ang), rad * np.sin(ang), z, rng.integers(0, 255, n)], 1).astype(np.float32)
    if n > 20:
        x[5:9] = x[4]
    return x


def test_patch_fill_of_every_tier(scvod, oracle):
    """one patch of exactly n points per scan for n around 1/2, 3/4 and 1 of every tier capacity (and 11 000 in the
    16 384 tier): once as a batch, once scan by scan"""
    import torch
    rng = np.random.default_rng(31)
    P = scvod.make_params("semantickitti")
    sizes = [n for c in CAPS for n in _fill_sizes(c)] + [11000]
    scans = [_patch(rng, n) for n in sizes]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in scans])]).astype(np.int32)
    allpts = np.concatenate(scans)
    ctx = scvod.Ctx(P, max_points_total=len(allpts) + 64, max_scans=len(scans))
    ctx.batch_process(torch.from_numpy(allpts).cuda(), offs)
    for s, x in enumerate(scans):
        o = _check_pw(oracle, P, x, ctx.batch_fetch(s), f"batch n={len(x)}")
        assert int((o["planes"]["n_pts"] > 0).sum()) == 1 and int(o["planes"]["n_pts"].max()) == len(x)   # really ONE patch
    for x in scans:
        _check_pw(oracle, P, x, ctx.process_scan(x), f"single n={len(x)}")
    ctx.close()


def test_small_patch_after_large_one_in_a_workgroup(scvod, oracle):
    """more items in the 4096 tier than it has workgroups, sizes 2049 / 4095 / 2050 / 3073 mixed: a persistent workgroup
    takes items blockIdx, blockIdx + grid, ... of the tier's list, so those that take a second item sort it in LDS that
    still holds the keys of the first.  The grid is kPersistCUs * 4 = 1024 workgroups (launch_process in
    scvod_kernels.hip): n_scans * per_scan has to stay above that, or no workgroup sorts twice and this checks nothing"""
    import torch
    rng = np.random.default_rng(32)
    P = scvod.make_params("semantickitti")
    cyc = (2049, 4095, 2050, 3073)
    n_scans, per_scan = 69, 16
    assert n_scans * per_scan >= 1024 + 64                     # at least 64 workgroups sort a second item
    scans = []
    for s in range(n_scans):
        scans.append(np.concatenate([_patch(rng, cyc[(s + k) % 4], k) for k in range(per_scan)]))
    offs = np.concatenate([[0], np.cumsum([len(x) for x in scans])]).astype(np.int32)
    allpts = np.concatenate(scans)
    ctx = scvod.Ctx(P, max_points_total=len(allpts) + 64, max_scans=n_scans)
    ctx.batch_process(torch.from_numpy(allpts).cuda(), offs)
    for s, x in enumerate(scans):
        o = _check_pw(oracle, P, x, ctx.batch_fetch(s), f"scan {s}")
        got = np.sort(o["planes"]["n_pts"][o["planes"]["n_pts"] > 0])
        assert np.array_equal(got, np.sort([cyc[(s + k) % 4] for k in range(per_scan)])), "sixteen patches of the sizes asked for"
    ctx.close()


def test_voxel_bucket_fill_of_every_tier(scvod, oracle):
    """one key bucket of exactly m points for m around 1/2, 3/4 and 1 of every tier capacity of the voxel-stage sorts,
    with many points per voxel and with single-point voxels"""
    rng = np.random.default_rng(33)
    P = scvod.make_params("semantickitti")
    sizes = [m for c in CAPS for m in _fill_sizes(c)]
    ctx = scvod.Ctx(P, max_points_total=max(sizes) + 64, max_scans=1)
    base_key = 4096 * 37                                       # one bucket of the 72 x 300 x 60 grid (shift 12)
    for m in sizes:
        for pattern in ("many per voxel", "single"):
            apri = np.zeros(m, scvod.APRI_DTYPE)
            if pattern == "single":
                apri["voxel_idx"] = base_key + rng.permutation(4096)[:m] if m <= 4096 else base_key + rng.integers(0, 4096, m)
            else:
                apri["voxel_idx"] = base_key + rng.integers(0, 40, m)
            apri["intensity"] = rng.integers(0, 255, m).astype(np.float32) * np.float32(0.37)
            apri["range_idx"] = apri["voxel_idx"] % 300        # any consistent-looking triple: the stage only uses the key
            r = ctx.voxelize(apri)
            v = oracle.voxelize(P, apri)
            tag = f"m={m} {pattern}"
            assert np.array_equal(r["vox_key"], v["vox_key"]), tag
            assert np.array_equal(r["vox_pt_begin"], v["vox_pt_begin"]) and np.array_equal(r["vox_pts"], v["vox_pts"]), tag
            assert np.array_equal(r["vox_av"].view(np.uint32), v["vox_av"].view(np.uint32)), tag
            assert np.array_equal(r["vox_cov"].view(np.uint32), v["vox_cov"].view(np.uint32)), tag
    ctx.close()


def test_filtered_scan_bucket_fill_of_every_tier(scvod, oracle):
    """the 32-bit key form of the voxel tiers (what a filtered scan or batch sorts: key relative to its bucket | point
    index): m points of ONE key bucket through bin_scan with the filter on, for m around 1/2, 3/4 and 1 of every tier
    capacity; odd m spread over the whole bucket (few points per voxel), even m packed into a few dozen voxels"""
    import ctypes as C
    rng = np.random.default_rng(34)
    P = scvod.make_params("semantickitti")
    r_, s_, z_, b_ = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    scvod.load_lib().scvod_grid_dims(C.byref(P), C.byref(r_), C.byref(s_), C.byref(z_), C.byref(b_))
    key_off = r_.value * s_.value + s_.value + 1               # bucket = (key + key_off) >> shift, as in scvod_capi.hip
    shift = 12
    while ((b_.value + key_off + 1) >> shift) + 1 > 1024:
        shift += 1

    def pool(n, d_lo, d_hi, a_lo, a_hi):
        """the points of n candidates on a cone of 5 degrees below the horizon that the filter keeps and that fall into
        the most populous key bucket"""
        dis, ang = rng.uniform(d_lo, d_hi, n), rng.uniform(a_lo, a_hi, n)
        x = np.stack([dis * np.cos(ang), dis * np.sin(ang), -dis * np.tan(np.deg2rad(5.0)), rng.integers(0, 255, n)], 1).astype(np.float32)
        b = oracle.bin(P, x, True)
        bucket = (b["apri"]["voxel_idx"].astype(np.int64) + key_off) >> shift
        return x[b["src"]][bucket == np.bincount(bucket).argmax()]

    spread, packed = pool(80000, 8.0, 20.0, 0.05, 6.2), pool(40000, 10.0, 10.4, 0.3, 1.1)
    assert len(spread) >= 8192 and len(packed) >= 8192
    ctx = scvod.Ctx(P, max_points_total=8192 + 64, max_scans=1)
    for m in [m for c in CAPS for m in _fill_sizes(c)]:
        x = (spread if m % 2 else packed)[:m]
        b = oracle.bin(P, x, True)
        bucket = (b["apri"]["voxel_idx"].astype(np.int64) + key_off) >> shift
        assert len(b["apri"]) == m and bucket.min() == bucket.max(), "really ONE bucket of m keys"
        r = ctx.bin_scan(x, apply_filter=True, with_voxels=True)
        v = oracle.voxelize(P, b["apri"])
        assert np.array_equal(r["apri"].view(np.uint8), b["apri"].view(np.uint8)), m
        assert np.array_equal(r["vox_key"], v["vox_key"]), m
        assert np.array_equal(r["vox_pt_begin"], v["vox_pt_begin"]) and np.array_equal(r["vox_pts"], v["vox_pts"]), m
        assert np.array_equal(r["vox_av"].view(np.uint32), v["vox_av"].view(np.uint32)), m
        assert np.array_equal(r["vox_cov"].view(np.uint32), v["vox_cov"].view(np.uint32)), m
    ctx.close()
