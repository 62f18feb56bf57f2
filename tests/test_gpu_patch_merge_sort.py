"""The large Patchwork sort tiers where they merge sorted runs by merge path (csrc/scvod_mergepath.h): crafted single-sector
patches at the sizes where the code takes another way -- one key either side of a tier's capacity (the staged start at exactly
half of it, the register start above), one key either side of a whole run of 16 -- and the key orders a merge can get wrong:
all z equal (the index alone decides), z descending in input order (every merge takes all of the upper run first), z of both
signs with +0 and -0, a small patch sorted in LDS that still holds a large one's keys, two different batches in turn on one
ctx.  Ground and non-ground index lists of batch_fetch against the oracle's Patchwork, entry for entry."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _patch(rng, n, sector=0, z=None):
    """n points inside ring 0 of one sector of the innermost zone (16 sectors); z: ties around the ground height unless given"""
    ang = sector * (2 * np.pi / 16) + rng.uniform(0.02, 0.37, n)
    rad = rng.uniform(3.2, 6.8, n)
    if z is None:
        z = np.round(rng.normal(-1.7, 0.04, n), 2)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), z, rng.integers(0, 255, n)], 1).astype(np.float32)


def _scan(rng, sizes, z_of=None):
    return np.concatenate([_patch(rng, n, k, None if z_of is None else z_of(n)) for k, n in enumerate(sizes)])


def _run_batch(scvod, ctx, scans):
    import torch
    offs = np.concatenate([[0], np.cumsum([len(x) for x in scans])]).astype(np.int32)
    ctx.batch_process(torch.from_numpy(np.concatenate(scans)).cuda(), offs)


def _check(oracle, P, ctx, scans, sizes, tag):
    """index lists entry for entry, and the patches are the ones asked for"""
    for s, x in enumerate(scans):
        r, o = ctx.batch_fetch(s), oracle.patchwork(P, x, 1)
        assert np.array_equal(r["ground_idx"], o["ground_idx"]), f"{tag} scan {s}: ground order"
        assert np.array_equal(r["nonground_idx"], o["nonground_idx"]), f"{tag} scan {s}: non-ground order"
        assert np.array_equal(r["cls"], o["cls"]), f"{tag} scan {s}: cls"
        n_pts = o["planes"]["n_pts"]
        assert np.array_equal(np.sort(n_pts[n_pts > 0]), np.sort(sizes[s])), f"{tag} scan {s}: one patch per size asked for"


def _ctx(scvod, P, scans):
    return scvod.Ctx(P, max_points_total=sum(len(x) for x in scans) + 64, max_scans=len(scans))


def test_one_patch_either_side_of_every_capacity(scvod, oracle):
    """2047 / 2048 / 2049, 4095 / 4096 / 4097, 8191 / 8192: last patch of a tier, first of the next (np2 half the capacity: the
    staged start) and the first that fills the tier's network (register start); two scans of four sectors each"""
    rng = np.random.default_rng(41)
    P = scvod.make_params("semantickitti")
    sizes = [(2047, 2048, 2049, 4095), (4096, 4097, 8191, 8192)]
    scans = [_scan(rng, s) for s in sizes]
    ctx = _ctx(scvod, P, scans)
    _run_batch(scvod, ctx, scans)
    _check(oracle, P, ctx, scans, sizes, "capacity")
    ctx.close()


def _z_equal(n):
    return np.full(n, -1.7)


def _z_descending(n):
    return np.linspace(-1.5, -1.9, n)      # distinct in fp32: 0.4 m over at most 8191 steps


def _z_signed(n):
    """both signs around the sensor height, and a quarter of the points at +0 or -0 (equal as numbers)"""
    z = np.round(np.random.default_rng(n).normal(0.0, 0.05, n), 2)
    z[0::8] = 0.0
    z[1::8] = -0.0
    return z


@pytest.mark.parametrize("z_of", [_z_equal, _z_descending, _z_signed], ids=["all-z-equal", "z-descending", "signed-zeros"])
def test_key_orders_a_merge_can_get_wrong(scvod, oracle, z_of):
    """a patch in each merging tier (1500, 3000 and 7000 points; 2064 and 4112 are a run past half a capacity), two scans"""
    rng = np.random.default_rng(42)
    P = scvod.make_params("semantickitti")
    sizes = [(1500, 3000, 7000), (2064, 4112, 1039)]
    scans = [_scan(rng, s, z_of) for s in sizes]
    if z_of is _z_signed:
        assert np.signbit(scans[0][:, 2]).any() and (scans[0][:, 2] > 0).any()
        assert (np.signbit(scans[0][:, 2]) & (scans[0][:, 2] == 0)).any(), "-0 survives the conversion to fp32"
    ctx = _ctx(scvod, P, scans)
    _run_batch(scvod, ctx, scans)
    _check(oracle, P, ctx, scans, sizes, z_of.__name__)
    ctx.close()


def test_small_patch_after_a_large_one_in_the_8192_tier(scvod, oracle):
    """more items in the 8192 tier than it has workgroups (kPersistCUs * 2 = 512, launch_process in scvod_kernels.hip): a
    persistent workgroup takes items blockIdx, blockIdx + 512, ... of the list, which is ordered by descending size class, so
    the workgroups that take a second item merge a patch of 4097 .. 4113 keys in LDS that still holds 6145 .. 8191 sorted ones.
    n_scans * per_scan has to stay above 512, or no workgroup sorts twice and this checks nothing"""
    rng = np.random.default_rng(43)
    P = scvod.make_params("semantickitti")
    cyc = (8191, 4097, 6145, 4113)
    n_scans, per_scan = 36, 16
    assert n_scans * per_scan >= 512 + 64                      # at least 64 workgroups sort a second item
    sizes = [[cyc[(s + k) % 4] for k in range(per_scan)] for s in range(n_scans)]
    scans = [_scan(rng, s) for s in sizes]
    ctx = _ctx(scvod, P, scans)
    _run_batch(scvod, ctx, scans)
    _check(oracle, P, ctx, scans, sizes, "reuse")
    ctx.close()


def test_two_different_batches_in_turn_on_one_ctx(scvod, oracle):
    """a batch of three scans, then one of two with other sizes in other sectors, then the first again"""
    rng = np.random.default_rng(44)
    P = scvod.make_params("semantickitti")
    sizes_a = [(4095, 2049), (8191,), (3000, 1500, 5000)]
    sizes_b = [(2050, 6000, 4097), (7000, 2047)]
    a = [_scan(rng, s) for s in sizes_a]
    b = [np.roll(_scan(rng, s), 7, axis=0) for s in sizes_b]
    ctx = scvod.Ctx(P, max_points_total=max(sum(len(x) for x in a), sum(len(x) for x in b)) + 64, max_scans=3)
    for scans, sizes, tag in ((a, sizes_a, "first"), (b, sizes_b, "second"), (a, sizes_a, "first again")):
        _run_batch(scvod, ctx, scans)
        _check(oracle, P, ctx, scans, sizes, tag)
    ctx.close()
