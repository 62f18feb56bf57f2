"""The voxel stage's point lists against independent arithmetic: np.lexsort((apri index, voxel key)) of the oracle's apri keys.

k_vx_bucket places the points of a bucket whose keys span 2^12 voxels by key counting (an LDS counter per voxel, a prefix, a rank inside the
voxel's own segment) in the tiers of 2048, 4096 and 8192 keys, and by the comparison network everywhere else: the smaller tiers, a span of
2^14 keys (os128_fine), 64-bit keys, and any bucket whose largest voxel holds more than DENSE points.  Keys are unique (the index is part of
them), so ascending (voxel key, apri index) is ONE total order and every output must be bit-identical whichever path took the bucket.

The reference is not the other code path: the oracle's Patchwork and binning give the apri keys of the scan (compared with the device's
first), numpy's lexsort the order, and vox_key / vox_pt_begin / vox_pts follow from it.  With scvod_set_voxel_descriptors(ctx, 1) vox_av /
vox_cov are compared bit for bit with the oracle's voxelize as well.

Crafted scans, built the way test_gpu_voxel_descriptors.py::_crafted_scan builds its: points at voxel centres 4..16 m from the sensor and
1..45 degrees above it, every case in a bucket of its own, ground underneath, points permuted.  One scan holds a bucket population on both
sides of every tier boundary; a second one, per switching tier: one-point voxels only (every key of the span, the first and the last among
them, where the tier's population allows), ONE voxel, a largest voxel of exactly DENSE points and of DENSE + 1, and a voxel of 2700 points
beside one-point voxels (1700 in the 2048 tier, which holds fewer than 2048 points).  The first and the last key of a span (rel == 0,
rel == 2^vb_shift - 1) are taken in a bucket that counts and in the one that holds every key.

The first and the last bucket of the grid.  Last: a probe scan (every voxel centre of the top azimuth layer over the same ground) goes
through the oracle, and the highest bucket it fills -- the grid's last one, n_buckets - 1, in all three presets -- gets a case of 3000 points (a
counting tier where the span is 2^12) on keys the probe kept.  First: buckets 0 .. (key_off >> vb_shift) - 1 hold negative voxel indices only
and can never be occupied; the first bucket that can is the one of voxel key 0, the innermost rings of the lowest layer.  Patchwork's ground
swallows a part of whatever stands there (which part depends on the rest of the scan), so the case is a point in every 7th voxel of that bucket,
and the test asserts on the reference that the bucket is populated, that nothing lies below it and nothing above the last one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_voxel_descriptors import _bits, _bucketing  # noqa: E402

pytestmark = pytest.mark.gpu

DENSE = 256   # kVxCountDense (scvod_k_voxels.inc): a bucket whose largest voxel exceeds it takes the network
LIST_KEYS = ("vox_key", "vox_pt_begin", "vox_pts")
DESC_KEYS = ("vox_av", "vox_cov")
# bucket populations on both sides of every tier boundary (the tiers take n < 256, < 1024, < 2048, < 4096, <= 8192; above: arena memory)
SIZES = (255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8192, 8193)
# a population inside every tier that switches to counting on a span of 2^12 keys (m, and the largest one-point-voxel bucket: 4096 keys)
TIERS = {2048: 1500, 4096: 3000, 8192: 6000}
_MEMO = {}


class _Grid:
    """voxel key = azimuth layer * R * S + range ring * S + sector; bucket = (key + key_off) >> shift"""

    def __init__(self, scvod, P):
        self.P = P
        self.R, self.S, self.key_off, self.shift = _bucketing(scvod, P)
        self.Az = scvod.grid_dims(P)[2]
        self.span = 1 << self.shift
        a_lo, a_hi = int(np.ceil((1.0 - P.min_azimuth) / P.azimuth_res)), int((45.0 - P.min_azimuth) / P.azimuth_res)
        r_lo, r_hi = int(np.ceil((4.0 - P.min_dis) / P.range_res)), int((16.0 - P.min_dis) / P.range_res)
        # per bucket: which of its keys a point above the ground can stand in
        self.buckets = {}
        for a in range(a_lo, a_hi):
            keys = a * self.R * self.S + np.arange(r_lo * self.S, r_hi * self.S, dtype=np.int64)
            b = (keys + self.key_off) >> self.shift
            for bk in np.unique(b):
                self.buckets.setdefault(int(bk), []).append(keys[b == bk])
        self.buckets = {bk: np.concatenate(v) for bk, v in self.buckets.items()}

    def points(self, keys):
        """the centre of each voxel"""
        keys = np.asarray(keys, np.int64)
        P = self.P
        a, rs = np.divmod(keys, self.R * self.S)
        r, sec = np.divmod(rs, self.S)
        dis = P.min_dis + (r + 0.5) * P.range_res
        phi = np.deg2rad(P.min_azimuth + (a + 0.5) * P.azimuth_res)
        th = np.deg2rad(P.min_angle + (sec + 0.5) * P.sector_res)
        return np.stack([dis * np.cos(th), dis * np.sin(th), dis * np.tan(phi), np.zeros(len(keys))], 1)

    def ground(self):
        P = self.P
        gr, gt = np.meshgrid(np.arange(2.0, 30.0, 0.4), np.deg2rad(np.arange(0.0, 360.0, 3.0)))
        gr, gt = gr.ravel(), gt.ravel()
        return np.stack([gr * np.cos(gt), gr * np.sin(gt), np.full(gr.size, -P.sensor_height), np.zeros(gr.size)], 1)


def _extremes(oracle, grid):
    """the lowest and the highest bucket a point can occupy, with the keys the oracle keeps there: {"low": (bucket, keys), "top": ...}"""
    layer = grid.R * grid.S
    keys = np.concatenate([np.arange(0, layer, dtype=np.int64), (grid.Az - 1) * layer + np.arange(0, layer, dtype=np.int64)])
    x = np.concatenate([grid.points(keys), grid.ground()]).astype(np.float32)
    x[:, 3] = 1.0
    o = oracle.patchwork(grid.P, x, 1)
    kept = np.unique(oracle.bin(grid.P, x[o["nonground_idx"]], True)["apri"]["voxel_idx"].astype(np.int64))
    kept = kept[np.isin(kept, keys)]   # (a point that left its voxel is no evidence for the voxel it landed in)
    b = (kept + grid.key_off) >> grid.shift
    first = grid.key_off >> grid.shift   # the bucket of voxel key 0: every bucket below it holds negative keys only
    low = np.arange(0, ((first + 1) << grid.shift) - grid.key_off, 7, dtype=np.int64)   # (every 7th: a denser sheet becomes Patchwork's ground)
    return {"low": (first, low), "top": (int(b.max()), kept[b == b.max()])}


def _scan(grid, cases, seed):
    """cases: per bucket the voxel populations, largest first, as (counts, whole): whole = the bucket must offer every key of its span (the
    case then takes the first and the last key, rel == 0 and rel == span - 1, first).  Returns the scan and, per case, its bucket."""
    rng = np.random.default_rng(seed)
    free = sorted(grid.buckets, key=lambda b: (-len(grid.buckets[b]), b))
    parts, where = [], []
    for counts, whole in cases:
        counts = np.asarray(counts, np.int64)
        if whole in ("low", "top"):   # the extreme buckets: on the keys the probe kept
            b, keys = grid.extreme[whole]
            parts.append(grid.points(np.repeat(keys[rng.permutation(len(keys))[:len(counts)]], counts)))
            where.append(b)
            continue
        fit = [b for b in free if len(grid.buckets[b]) >= (grid.span if whole else len(counts))]
        assert fit, f"no bucket left that offers {len(counts)} voxels"
        b = fit[-1] if not whole else fit[0]   # (the emptiest bucket that still fits: the whole ones are few)
        free.remove(b)
        keys = grid.buckets[b]
        if whole:
            assert len(keys) == grid.span
            pick = np.concatenate([[0, grid.span - 1], 1 + rng.permutation(grid.span - 2)])[:len(counts)]
        else:
            pick = rng.permutation(len(keys))[:len(counts)]
        parts.append(grid.points(np.repeat(keys[pick], counts)))
        where.append(b)
    parts.append(grid.ground())
    x = np.concatenate(parts).astype(np.float32)
    x[:, 3] = np.exp(rng.uniform(np.log(1e-3), np.log(255.0), len(x))).astype(np.float32)   # (fp32 summation order matters)
    return x[rng.permutation(len(x))], where


def _spread(n, largest, voxels=None):
    """n points: one voxel of `largest`, the others over one-point voxels (voxels=None) or `voxels` voxels of nearly equal size"""
    rest = n - largest
    if voxels is None or rest <= voxels:
        return [largest] + [1] * rest
    q, r = divmod(rest, voxels)
    return [largest] + [q + 1] * r + [q] * (voxels - r)


def _boundary_cases(grid):
    # a voxel of 40 points and the others over n / 4 voxels: every bucket stays below DENSE, so the counting tiers count
    return [(_spread(n, 40, max(n // 4, 1)), False) for n in SIZES]


def _tier_cases(grid):
    cases = []
    for cap, m in TIERS.items():
        whole = grid.span <= 4096
        ones = m if cap < 8192 else min(grid.span, 8192)               # (the 8192 tier takes 4096 <= m: every key of a 2^12 span)
        cases.append(([1] * ones, whole and cap == 8192))              # one-point voxels only
        cases.append(([m], False))                                     # ONE voxel
        cases.append((_spread(m, DENSE, 900), False))                  # the largest voxel holds exactly the fallback threshold
        cases.append((_spread(m, DENSE + 1, 900), False))              # ... and one point more
        big = 2700 if cap > 2048 else 1700
        cases.append((_spread(big + 300 if cap < 8192 else big + 2000, big), False))   # a dense voxel beside one-point voxels
    cases.append((_spread(3000, 30, 700), grid.span <= 4096))          # rel == 0 and rel == span - 1 in a bucket that counts
    # the last bucket a point can occupy: 3000 points; the first: one point in every 7th voxel of its non-negative keys (the innermost rings
    # of the lowest layer; Patchwork takes a part of them for ground, which part depends on the rest of the scan)
    cases.append((_spread(3000, 30, min(700, len(grid.extreme["top"][1]) - 1)), "top"))
    cases.append(([1] * len(grid.extreme["low"][1]), "low"))
    return cases


def _reference(oracle, P, x):
    """apri keys by the oracle, the order by numpy"""
    o = oracle.patchwork(P, x, 1)
    apri = oracle.bin(P, x[o["nonground_idx"]], True)["apri"]
    key = apri["voxel_idx"].astype(np.int64)
    n = len(key)
    order = np.lexsort((np.arange(n), key))
    sk = key[order]
    heads = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]])) if n else np.zeros(0, np.int64)
    want = dict(vox_key=sk[heads].astype(np.int32), vox_pt_begin=np.concatenate([heads, [n]]).astype(np.int32), vox_pts=order.astype(np.int32))
    v = oracle.voxelize(P, apri)
    want.update(vox_av=v["vox_av"], vox_cov=v["vox_cov"])
    return apri, want


def _crafted(scvod, oracle, preset):
    """two crafted scans of a preset and their references: computed once"""
    if preset not in _MEMO:
        P = scvod.make_params(preset)
        grid = _Grid(scvod, P)
        grid.extreme = _extremes(oracle, grid)
        xa, wa = _scan(grid, _boundary_cases(grid), 3)
        xb, wb = _scan(grid, _tier_cases(grid), 4)
        _MEMO[preset] = (P, grid, [xa, xb], [_reference(oracle, P, x) for x in (xa, xb)], [wa, wb])
    return _MEMO[preset]


def _per_bucket(grid, want):
    """population and largest voxel of every bucket of a reference"""
    c = np.diff(want["vox_pt_begin"]).astype(np.int64)
    b = (want["vox_key"].astype(np.int64) + grid.key_off) >> grid.shift
    pop = np.bincount(b, weights=c).astype(np.int64)
    big = np.zeros(len(pop), np.int64)
    np.maximum.at(big, b, c)
    return pop, big


def _check(ctx, s, ref, keys, what):
    apri, want = ref
    r = ctx.batch_fetch(s)
    assert np.array_equal(np.asarray(r["apri"]).view(np.uint8), apri.view(np.uint8)), f"{what}: the device's apri_vec is not the oracle's"
    for k in keys:
        assert np.array_equal(_bits(np.asarray(r[k])), _bits(want[k])), f"{what}: scan {s}: {k} differs"


def _run(scvod, P, scans, refs, mode, what):
    import torch
    offs = np.concatenate([[0], np.cumsum([len(x) for x in scans])]).astype(np.int32)
    d = torch.from_numpy(np.concatenate(scans)).cuda().contiguous()
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=len(scans))
    ctx.set_voxel_descriptors(mode)
    ctx.batch_process(d, offs)
    for s, ref in enumerate(refs):
        _check(ctx, s, ref, LIST_KEYS + DESC_KEYS, f"{what}, mode {mode}")
    ctx.close()


# ---- the crafted inputs do what they were crafted for (the references only; no device) ------------------------------------------------

@pytest.mark.parametrize("preset", ["semantickitti", "parkinglot", "os128_fine"])
def test_the_crafted_scans_hold_their_cases(scvod, oracle, preset):
    P, grid, scans, refs, where = _crafted(scvod, oracle, preset)
    pop, big = _per_bucket(grid, refs[0][1])
    assert [int(pop[b]) for b in where[0]] == list(SIZES)
    assert all(big[b] == 40 for b in where[0])
    pop, big = _per_bucket(grid, refs[1][1])
    cases = _tier_cases(grid)
    assert [int(pop[b]) for b in where[1][:-2]] == [int(np.sum(c)) for c, _ in cases[:-2]]
    assert [int(big[b]) for b in where[1][:-2]] == [int(np.max(c)) for c, _ in cases[:-2]]
    assert {DENSE, DENSE + 1, 2700} <= set(big[where[1]].tolist())
    if grid.span == 4096:   # the first and the last key of a span, in a bucket that counts and in the one that holds every key
        rel = (refs[1][1]["vox_key"].astype(np.int64) + grid.key_off) & (grid.span - 1)
        b = (refs[1][1]["vox_key"].astype(np.int64) + grid.key_off) >> grid.shift
        for bk in (where[1][-3], where[1][10]):
            assert {0, grid.span - 1} <= set(rel[b == bk].tolist())
        assert pop[where[1][10]] == grid.span and big[where[1][10]] == 1
    # the extreme buckets: populated, nothing beyond them, and the top one is the grid's last where the binning keeps its rings
    top, low = where[1][-2], where[1][-1]
    filled = np.flatnonzero(pop)
    assert filled.min() == low and filled.max() == top and 0 < low < top
    # (Patchwork takes some of these points for ground, differently from scan to scan: what the reference holds there is what counts)
    assert 2048 <= pop[top] < 4096 and pop[low] >= 20, (pop[top], pop[low])
    n_buckets = ((scvod.grid_dims(P)[3] + grid.key_off + 1) >> grid.shift) + 1
    assert top == n_buckets - 1 and low == grid.key_off >> grid.shift
    idx_bits = int(np.ceil(np.log2(max(len(x) for x in scans))))
    assert grid.shift + idx_bits <= 32, "the scans must take the 32-bit keys"
    assert (grid.shift == 12) == (preset != "os128_fine")


# ---- every case, both forms of the voxel stage, all three presets ----------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("preset", ["semantickitti", "parkinglot", "os128_fine"])
def test_crafted_buckets_equal_the_lexsort(scvod, oracle, preset, mode):
    P, grid, scans, refs, where = _crafted(scvod, oracle, preset)
    _run(scvod, P, scans, refs, mode, preset)


# ---- the counters are reused across the buckets of a persistent workgroup: two different batches on one ctx in turn ---------------------

def test_two_batches_in_turn_on_one_ctx(scvod, oracle):
    import synth
    import torch
    P, grid, scans, refs, where = _crafted(scvod, oracle, "semantickitti")
    other = [synth.make_scan(5, 420, "K64")[0].numpy(), scans[0][::3].copy()]
    other_refs = [_reference(oracle, P, x) for x in other]
    batches = []
    for xs in (scans, other):
        offs = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
        batches.append((torch.from_numpy(np.concatenate(xs)).cuda().contiguous(), offs))
    ctx = scvod.Ctx(P, max_points_total=max(int(o[-1]) for _, o in batches) + 64, max_scans=2)
    for turn, (which, rr) in enumerate(((0, refs), (1, other_refs), (0, refs), (1, other_refs))):
        ctx.batch_process(*batches[which])
        for s, ref in enumerate(rr):
            _check(ctx, s, ref, LIST_KEYS, f"turn {turn}")
    ctx.close()


# ---- one seeded synthetic scan per kind against the oracle -----------------------------------------------------------------------------

@pytest.mark.parametrize("kind,preset,scan", [("K64", "semantickitti", 977), ("PARK", "parkinglot", 33), ("OS128", "os128_fine", 305)])
@pytest.mark.parametrize("mode", [0, 1])
def test_a_synthetic_scan_equals_the_lexsort(scvod, oracle, kind, preset, scan, mode):
    import synth
    P = scvod.make_params(preset)
    x = synth.make_scan(5, scan, kind)[0].numpy()
    ref = _reference(oracle, P, x)
    assert len(ref[1]["vox_key"]) > 1000
    _run(scvod, P, [x], [ref], mode, kind)
