"""The per-voxel intensity descriptors (vox_av / vox_cov) of a batch, computed on demand.

A batch's voxel stage runs lean by default (scvod_set_voxel_descriptors mode 0): k_vx_bucket<..., DESC = false> leaves the descriptors
out, and k_vx_descriptors fills them from vox_pt_begin / vox_pts / apri_int when somebody asks -- the first batch_fetch, or the intensity
merge.  Mode 1 computes them inside the voxel stage of every batch, as the per-scan API always does.  Both forms call one routine
(vx_descriptor, scvod_k_voxels.inc), so every comparison here is bit for bit:

  a. lean + on demand == eager on a crafted scan whose buckets sit on both sides of every tier boundary of the voxel stage, with 32-bit
     and with 64-bit sort keys;
  b. the on-demand values == the oracle's av / cov on a 64-beam and a parking-lot scan;
  c. a fetch after clustering, types, tracking and the map == a fetch right after batch_process (the kernel's inputs survive the chain);
  d. the intensity merge gets its descriptors: merged names and counters are the same in both modes, whichever came first, the batch
     or scvod_set_intensity_merge;
  e. the chain enqueued on a side stream without synchronisation, then a fetch;
  f. changing batches on one ctx: every process call resets the flag, every fetch returns its own batch's values.

The 64-bit keys: every batch entry filters by range / FOV, so no out-of-grid bin reaches a lean voxel stage (scvod_bin_scan without the
filter is a per-scan call and keeps the fused form).  What does take a batch to 64-bit keys is a grid so fine that a bucket-relative
key and a scan-local index no longer share 32 bits (vb_shift + index bits > 32): the second case of (a) runs on such a grid."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_async_chain import MAP_CELLS, MERGE, _batch, _enqueue, _new_ctx, _stream, _track  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("vox_key", "vox_pt_begin", "vox_pts", "vox_av", "vox_cov")
# bucket populations on both sides of every tier boundary of k_vx_bucket (256 / 1024 / 2048 / 4096 / 8192 keys; the tiers take
# n < 256, < 1024, < 2048, < 4096, <= 8192), and one above the largest tier: the oversize path that sorts in arena memory
SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8192, 8193)
_EAGER = {}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _bucketing(scvod, P):
    """DevParams::key_off / vb_shift of the voxel stage (bucket = (voxel_idx + key_off) >> vb_shift, at most 1024 buckets)"""
    R, S, Az, bins = scvod.grid_dims(P)
    key_off = R * S + S + 1
    span = bins + key_off + 1
    shift = 12
    while (span >> shift) + 1 > 1024:
        shift += 1
    return R, S, key_off, shift


def _crafted_scan(scvod, P, seed=3):
    """One ring of the grid (an azimuth layer, a range ring: S consecutive voxel keys) per entry of SIZES, each ring inside one bucket
    of its own, at 4..12 m and 1..45 degrees above the sensor; a third of every larger ring's points in ONE voxel (several hundred to
    2700 points), the others spread over the ring (one-point voxels among them); ground under everything, so that Patchwork's planes
    are the ground and the rings stand clear of them.  Intensities log-uniform over 1e-3..255: fp32 summation order matters."""
    R, S, key_off, shift = _bucketing(scvod, P)
    rng = np.random.default_rng(seed)
    rings, used = [], set()
    a_lo, a_hi = int(np.ceil((1.0 - P.min_azimuth) / P.azimuth_res)), int((45.0 - P.min_azimuth) / P.azimuth_res)
    r_lo, r_hi = int(np.ceil((4.0 - P.min_dis) / P.range_res)), int((12.0 - P.min_dis) / P.range_res)
    for a in range(a_lo, a_hi):
        for r in range(r_lo, r_hi):
            k0 = a * R * S + r * S
            b = (k0 + key_off) >> shift
            if b == (k0 + S - 1 + key_off) >> shift and b not in used:
                used.add(b)
                rings.append((a, r))
    assert len(rings) >= len(SIZES)
    parts = []
    for (a, r), n in zip(rings, SIZES):
        dis = P.min_dis + (r + 0.5) * P.range_res
        phi = np.deg2rad(P.min_azimuth + (a + 0.5) * P.azimuth_res)
        sec = rng.integers(0, S, n)
        if n >= 1024:
            sec[:n // 3] = sec[0]
        th = np.deg2rad(P.min_angle + (sec + 0.5) * P.sector_res)
        parts.append(np.stack([dis * np.cos(th), dis * np.sin(th), np.full(n, dis * np.tan(phi)), np.zeros(n)], 1))
    gr, gt = np.meshgrid(np.arange(2.0, 30.0, 0.4), np.deg2rad(np.arange(0.0, 360.0, 3.0)))
    gr, gt = gr.ravel(), gt.ravel()
    parts.append(np.stack([gr * np.cos(gt), gr * np.sin(gt), np.full(gr.size, -P.sensor_height), np.zeros(gr.size)], 1))
    x = np.concatenate(parts).astype(np.float32)
    x[:, 3] = np.exp(rng.uniform(np.log(1e-3), np.log(255.0), len(x))).astype(np.float32)
    return x[rng.permutation(len(x))]


def _fetch(ctx, n):
    return [{k: np.asarray(v).copy() for k, v in ctx.batch_fetch(s).items() if k in KEYS} for s in range(n)]


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for s, (g, w) in enumerate(zip(got, want)):
        for k in KEYS:
            assert np.array_equal(_bits(g[k]), _bits(w[k])), f"{what}: scan {s}: {k} differs"


def _eager(scvod, b):
    """the batch in a fresh ctx at mode 1 (descriptors inside the voxel stage), fetched right after batch_process: computed once"""
    if b.name not in _EAGER:
        ctx = _new_ctx(scvod, [b], lambda c: c.set_voxel_descriptors(1))
        ctx.batch_process(b.d, b.offs)
        _EAGER[b.name] = _fetch(ctx, b.n)
        ctx.close()
    return _EAGER[b.name]


# ---- a. lean + on demand equals eager, bit for bit, on every tier -----------------------------------------------------------------------

@pytest.mark.parametrize("grid", ["32-bit keys", "64-bit keys"])
def test_on_demand_equals_eager_on_every_tier(scvod, grid):
    import synth
    import torch
    fine = dict(range_res=0.02, sector_res=0.06) if grid == "64-bit keys" else {}
    P = scvod.make_params("semantickitti", **fine)
    x = _crafted_scan(scvod, P)
    small = synth.make_scan(5, 300, "K64")[0].numpy()[::7]   # (a second, smaller scan: more than one scan per launch)
    offs = np.asarray([0, len(x), len(x) + len(small)], np.int32)
    d = torch.from_numpy(np.concatenate([x, small])).cuda().contiguous()
    R, S, key_off, shift = _bucketing(scvod, P)
    idx_bits = int(np.ceil(np.log2(len(x))))
    assert (shift + idx_bits <= 32) == (grid == "32-bit keys"), "the grid does not select the key type the case is named after"
    res = {}
    for mode in (0, 1):
        ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=2)
        ctx.set_voxel_descriptors(mode)
        ctx.batch_process(d, offs)
        res[mode] = _fetch(ctx, 2)
        ctx.close()
    _assert_same(res[0], res[1], grid)
    # the input does what it was crafted for: every population of SIZES is there, with one-point voxels (variance exactly 0) and a
    # voxel of several hundred points
    v = res[1][0]
    per_voxel = np.diff(v["vox_pt_begin"])
    per_bucket = np.bincount((v["vox_key"].astype(np.int64) + key_off) >> shift, weights=per_voxel).astype(np.int64)
    assert set(SIZES) <= set(per_bucket.tolist()), sorted(set(SIZES) - set(per_bucket.tolist()))
    assert per_voxel.max() >= 300 and (per_voxel == 1).sum() > 100
    assert (v["vox_cov"][per_voxel == 1] == 0).all() and (v["vox_cov"][per_voxel >= 300] > 0).all()


def test_the_mode_is_validated(scvod):
    ctx = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    for bad in (-1, 2):
        with pytest.raises(scvod.ScvodError):
            ctx.set_voxel_descriptors(bad)
    ctx.close()


# ---- b. the oracle still agrees ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,preset,scan", [("K64", "semantickitti", 1263), ("PARK", "parkinglot", 40)])
def test_on_demand_equals_the_oracle(scvod, oracle, kind, preset, scan):
    import synth
    P = scvod.make_params(preset)
    pts = synth.make_scan(5, scan, kind, device="cuda")[0].contiguous()
    offs = np.asarray([0, len(pts)], np.int32)
    ctx = scvod.Ctx(P, max_points_total=len(pts) + 64, max_scans=1)
    ctx.batch_process(pts, offs)
    r = ctx.batch_fetch(0)
    apri = np.asarray(r["apri"]).copy()
    got = {k: np.asarray(r[k]).copy() for k in KEYS}
    ctx.close()
    want = oracle.voxelize(P, apri)
    assert len(got["vox_av"]) > 1000
    for k in KEYS:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), f"{kind}: {k} differs from the oracle"


# ---- c. the inputs survive the chain ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["K6", "OS3"])
def test_a_fetch_after_the_whole_chain(scvod, name):
    b = _batch(scvod, name)
    first = _new_ctx(scvod, [b])
    first.batch_process(b.d, b.offs)
    at_once = _fetch(first, b.n)
    first.close()
    ctx, smap = _new_ctx(scvod, [b]), scvod.StaticMap(MAP_CELLS)
    ctx.batch_process(b.d, b.offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    _track(ctx, b, b.T, b.nxt, None, 1)
    smap.accumulate(ctx, b.poses)
    late = _fetch(ctx, b.n)
    smap.close()
    ctx.close()
    _assert_same(late, at_once, f"{name}: fetched after cluster, types, track and map")
    _assert_same(late, _eager(scvod, b), f"{name}: against the eager ctx")


# ---- d. the merge still gets its descriptors --------------------------------------------------------------------------------------------

def test_the_intensity_merge_reads_the_same_descriptors(scvod):
    b = _batch(scvod, "K6")
    got = {}
    # "late": the merge is turned on after the batch was processed lean, so the clustering itself asks for the descriptors
    for tag, mode, merge_first in (("eager", 1, True), ("on demand", 0, True), ("late", 0, False)):
        ctx = _new_ctx(scvod, [b])
        ctx.set_voxel_descriptors(mode)
        if merge_first:
            ctx.set_intensity_merge(*MERGE)
        ctx.batch_process(b.d, b.offs)
        if not merge_first:
            ctx.set_intensity_merge(*MERGE)
        ctx.batch_cluster()
        counts = ctx.batch_counts()
        got[tag] = ([ctx.batch_fetch_clusters(s, int(counts[s, 4])) for s in range(b.n)], ctx.batch_cluster_merge_stats())
        ctx.close()
    assert got["eager"][1]["fusions"] > 0
    for tag in ("on demand", "late"):
        assert got[tag][1] == got["eager"][1], f"{tag}: the merge's counters"
        for s in range(b.n):
            assert np.array_equal(got[tag][0][s], got["eager"][0][s]), f"{tag}: merged names of scan {s}"


# ---- e. stream order --------------------------------------------------------------------------------------------------------------------

def test_a_fetch_behind_the_chain_on_a_side_stream(scvod):
    b = _batch(scvod, "K6")
    stream = _stream()
    ctx, smap = _new_ctx(scvod, [b]), scvod.StaticMap(MAP_CELLS)
    _enqueue(ctx, smap, b, stream.cuda_stream)   # (nothing synchronises: the fetch orders its kernel behind the chain itself)
    got = _fetch(ctx, b.n)
    stream.synchronize()
    smap.close()
    ctx.close()
    _assert_same(got, _eager(scvod, b), "side stream, sync=False")


# ---- f. changing batches on one ctx -----------------------------------------------------------------------------------------------------

def test_every_process_call_resets_the_flag(scvod):
    a, b = _batch(scvod, "K6"), _batch(scvod, "R3")
    assert a.n != b.n and a.offs[-1] != b.offs[-1]
    ctx = _new_ctx(scvod, [a, b])
    ctx.batch_process(a.d, a.offs)
    _assert_same(_fetch(ctx, a.n), _eager(scvod, a), "A")
    ctx.batch_process(b.d, b.offs)
    _assert_same(_fetch(ctx, b.n), _eager(scvod, b), "B after A")
    ctx.batch_process(a.d, a.offs)               # (no fetch: A's descriptors are never computed)
    ctx.batch_process(b.d, b.offs)
    _assert_same(_fetch(ctx, b.n), _eager(scvod, b), "B after an unfetched A")
    ctx.batch_process(a.d, a.offs)
    _assert_same(_fetch(ctx, a.n), _eager(scvod, a), "A again")
    ctx.set_voxel_descriptors(1)                 # (the switch takes effect with the next batch)
    ctx.batch_process(b.d, b.offs)
    _assert_same(_fetch(ctx, b.n), _eager(scvod, b), "B, eager on the same ctx")
    ctx.close()
