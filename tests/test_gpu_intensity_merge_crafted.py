"""The intensity merge on the device (csrc/scvod_k_merge.inc) on the crafted scans of tests/helpers/merge_cases.py, whose preconditions
tests/test_intensity_merge_cases.py pins on the CPU: the hand cases with known answers (limits taken at equality, the far rule at
bins 43 / 44 of 72 and, where 0.6 R is an integer and `>` differs from `>=`, at bins 42 / 43 of 70, no sector wrap), clusters whose run of pairs ends before, on and after the walk's 64 lanes, pair counts on both sides of
the sort's and the unique's sizes, fusions of fusions over eight iterations, the scratch limit of 4 n + 256 pairs from both sides with
the error every reader then returns and the recovery of the ctx, the batch path against the single-scan path, scans whose clusters
share their smallest voxel key, and the refusal of a grid whose row table does not fit the LDS.  Everything is integer: no tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import intensity_merge_ref as imr  # noqa: E402
import merge_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

STAT_KEYS = ("clusters_before", "fusions", "clusters_after")


@pytest.fixture(scope="module")
def P(scvod):
    return scvod.make_params(mc.PRESET)


@pytest.fixture(scope="module")
def ctx(scvod, P):
    c = scvod.Ctx(P, max_points_total=4096, max_scans=1)
    yield c
    c.close()


@pytest.fixture
def new_ctx(scvod):
    """ctxs of a test's own, closed whether the test passes or not"""
    made = []

    def make(params, **kw):
        made.append(scvod.Ctx(params, **kw))
        return made[-1]
    yield make
    for c in made:
        c.close()


def _plain(ctx, oracle, P, apri):
    """the partition with the merge off: it must be the reference's"""
    ctx.set_intensity_merge(0, 2, 2.0, 1.0)
    pre = ctx.cluster(apri)
    assert np.array_equal(pre, imr.canonical(oracle.cluster(P, apri)[0]))
    return pre


def _merged(ctx, oracle, P, apri, pre, iterations, params, grid=mc.GRID):
    """one scan through voxelize / batch_cluster / batch_cluster_types (the finish reads A.apri) against the convention: partition,
    types, counters; the one-shot call gives the same"""
    n = len(apri)
    ctx.set_intensity_merge(iterations, *params)
    ctx.voxelize(apri)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    got = ctx.batch_fetch_clusters(0, n)
    types = ctx.batch_fetch_cluster_types(0, n, car_label=2, other_label=1)
    stats = ctx.batch_cluster_merge_stats()
    st = {}
    want = imr.convention(oracle.voxelize(P, apri), pre, grid, iterations, *params, stats=st)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {n} points differ"
    assert np.array_equal(types, oracle.cluster_types(P, apri, got, car_label=2, other_label=1))
    assert {k: stats[k] for k in STAT_KEYS} == {k: st[k] for k in STAT_KEYS}
    assert stats["scans_fused"] == (1 if st["fusions"] else 0)
    assert np.array_equal(ctx.cluster(apri), got)
    return got, types, st


def _apri(oracle, P, x):
    apri = oracle.bin(P, x, True)["apri"]
    assert len(apri) == len(x)
    return apri


@pytest.mark.parametrize("case", mc.HAND_CASES, ids=[c[0] for c in mc.HAND_CASES])
def test_hand_cases(ctx, oracle, P, case):
    name, voxels, iterations, params, groups = case
    apri = _apri(oracle, P, mc.scan(P, voxels))
    pre = _plain(ctx, oracle, P, apri)
    assert len(set(pre)) == len(voxels)
    got, _, _ = _merged(ctx, oracle, P, apri, pre, iterations, params)
    assert np.array_equal(got, mc.groups_to_names(voxels, groups))   # the answer the reference's text gives


@pytest.mark.parametrize("case", mc.FAR_CASES, ids=[c[0] for c in mc.FAR_CASES])
def test_far_rule_boundary(scvod, new_ctx, oracle, case):
    """R = 70: 0.6 R = 42.0 exactly, so bin 42 tells `>` from `>=` (on the preset's 72 bins no range bin does)"""
    name, voxels, iterations, params, groups = case
    far = scvod.make_params(mc.PRESET, **mc.FAR_GRID_KW)
    assert tuple(int(g) for g in oracle.grid_dims(far)[:3]) == mc.FAR_GRID
    c = new_ctx(far, max_points_total=64, max_scans=1)
    apri = _apri(oracle, far, mc.scan(far, voxels))
    pre = _plain(c, oracle, far, apri)
    assert len(set(pre)) == len(voxels)
    got, _, _ = _merged(c, oracle, far, apri, pre, iterations, params, grid=mc.FAR_GRID)
    assert np.array_equal(got, mc.groups_to_names(voxels, groups))


@pytest.mark.parametrize("m", [63, 64, 65, 128, 129])
def test_hub_run_of_m_pairs(ctx, oracle, P, m):
    """the hub's run of pairs is m long, all valid: it ends one lane before, on and one lane after the wave's last lane"""
    apri = _apri(oracle, P, mc.scan(P, mc.hub(m)))
    pre = _plain(ctx, oracle, P, apri)
    assert len(set(pre)) == m + 3
    for iterations in (1, 3):
        got, _, st = _merged(ctx, oracle, P, apri, pre, iterations, mc.YAML)
        assert st["fusions"] == 2 and st["clusters_after"] == 3
        h = 2 * (2 * m + 1)
        assert (got[:h] == 0).all() and (got[h:h + m] == h).all()      # the hub stays out of the fusion it records


SORT_SCANS = [("lines", c, n) for c, n in [(4, 128), (4, 130), (8, 128), (8, 130), (16, 128), (16, 130)]] + [("thick", 5, 120)]


@pytest.mark.parametrize("kind,count,length", SORT_SCANS)
def test_sort_and_unique_sizes(ctx, oracle, P, kind, count, length):
    """1016 / 1032, 2032 / 2064, 4064 / 4128 pairs, all different (one compare per thread of the sort, then several; one chunk of the
    unique, then more), and 1200 pairs of which 10 are different, a run of equal ones across index 1024.  Eight iterations halve a
    line seven times: names resolved through chains of several links"""
    voxels = mc.shuffled(mc.lines(count, length), 1) if kind == "lines" else mc.shuffled(mc.thick_lines(count, length), 2)
    apri = _apri(oracle, P, mc.scan(P, voxels))
    pre = _plain(ctx, oracle, P, apri)
    for iterations in (1, 8):
        got, _, st = _merged(ctx, oracle, P, apri, pre, iterations, mc.YAML)
    if kind == "lines":
        assert sum(f > 0 for f in st["fusions_per_iteration"]) >= 4
        assert st["clusters_after"] < st["clusters_before"] // 64
    else:
        assert st["fusions"] == count and st["clusters_after"] == count


@pytest.mark.parametrize("search_c", [2, 3])
def test_slack_lets_a_small_sparse_scan_through(ctx, oracle, P, search_c):
    """27 points, 316 pairs: 11.7 per point, within 4 * 27 + 256 = 364"""
    apri = _apri(oracle, P, mc.scan(P, mc.lattice(3, 3, 3)))
    pre = _plain(ctx, oracle, P, apri)
    for iterations in (1, 3):
        got, _, st = _merged(ctx, oracle, P, apri, pre, iterations, (search_c, 2.0, 1.0))
    assert len(set(got)) == 1 and st["fusions"] == 8


@pytest.mark.parametrize("dims", [(4, 4, 3), (6, 6, 4)])
def test_capacity_contract(scvod, new_ctx, oracle, P, dims):
    """652 pairs against 448, 2416 against 832: the clustering returns, every reader fails, and the next clustering starts clean"""
    c = new_ctx(P, max_points_total=1024, max_scans=1)
    apri = _apri(oracle, P, mc.scan(P, mc.lattice(*dims)))
    n = len(apri)
    c.set_intensity_merge(3, *mc.YAML)
    c.voxelize(apri)
    c.batch_cluster()
    with pytest.raises(scvod.ScvodError, match="outgrew"):
        c.batch_fetch_clusters(0, n)
    c.batch_cluster_types()
    with pytest.raises(scvod.ScvodError, match="outgrew"):
        c.batch_fetch_cluster_types(0, n)
    with pytest.raises(scvod.ScvodError, match="outgrew"):
        c.batch_track(np.zeros(12, np.float32))
    with pytest.raises(scvod.ScvodError, match="outgrew"):
        c.batch_cluster_merge_stats()
    with pytest.raises(scvod.ScvodError, match="outgrew"):
        c.cluster(apri)
    pre = _plain(c, oracle, P, apri)        # merge off, a new clustering: the plain partition
    assert len(set(pre)) == n
    assert c.batch_cluster_merge_stats() == dict(clusters_before=0, fusions=0, clusters_after=0, scans_fused=0)
    small = _apri(oracle, P, mc.scan(P, mc.lattice(3, 3, 3)))
    got, _, st = _merged(c, oracle, P, small, _plain(c, oracle, P, small), 3, mc.YAML)   # (counters of this scan alone)
    assert len(set(got)) == 1 and st["clusters_before"] == 27


def _batch(P, lists, seeds):
    """(the disc seeds are those tests/test_intensity_merge_cases.py::test_ground_disc_leaves_the_crafted_points pins per scan)"""
    import torch
    crafted = [mc.scan(P, v) for v in lists]
    scans = [mc.with_ground(x, k) for k, x in zip(seeds, crafted)]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in scans])]).astype(np.int32)
    return crafted, torch.from_numpy(np.concatenate(scans)).cuda().contiguous(), offs


def _batch_results(c, d, offs, with_types=True):
    c.batch_process(d, offs)
    c.batch_cluster()
    if with_types:
        c.batch_cluster_types()
    out = []
    for s in range(len(offs) - 1):
        r = c.batch_fetch(s)
        out.append((r, c.batch_fetch_clusters(s, r["n_apri"]),
                    c.batch_fetch_cluster_types(s, r["n_apri"], car_label=2, other_label=1) if with_types else None))
    return out


def test_batch_against_single_scans(scvod, new_ctx, ctx, oracle, P):
    """three crafted scans, each over a ground disc, through batch_process: scans at s > 0 have their pairs behind those of the scans
    before them, and the finish takes the boxes from the input points.  Against the convention on the batch's own apri, and against
    the same crafted points run alone (matched through apri_src: Patchwork hands the points on in the order of its patches)"""
    lists = [mc.hub(64), mc.shuffled(mc.lines(4, 128), 1), mc.lattice(3, 3, 3)]
    crafted, d, offs = _batch(P, lists, (0, 1, 2))
    over = list(lists)
    over[1] = mc.lattice(4, 4, 3)
    crafted_over, d_over, offs_over = _batch(P, over, (0, 3, 2))
    c = new_ctx(P, max_points_total=int(max(offs[-1], offs_over[-1])) + 64, max_scans=3)
    plain = _batch_results(c, d, offs, with_types=False)
    for s, (r, pre, _) in enumerate(plain):
        assert r["n_apri"] == len(crafted[s]) and (r["apri_src"] < len(crafted[s])).all()     # the disc went, the crafted points stayed
        assert np.array_equal(pre, imr.canonical(oracle.cluster(P, r["apri"])[0]))
    c.set_intensity_merge(3, *mc.YAML)

    def check():
        total = dict.fromkeys(STAT_KEYS, 0)
        fused = 0
        res = _batch_results(c, d, offs)
        stats = c.batch_cluster_merge_stats()
        for s, (r, got, types) in enumerate(res):
            st = {}
            want = imr.convention(oracle.voxelize(P, r["apri"]), plain[s][1], mc.GRID, 3, *mc.YAML, stats=st)
            assert np.array_equal(got, want), s
            assert np.array_equal(types, oracle.cluster_types(P, r["apri"], got, car_label=2, other_label=1)), s
            apri1 = _apri(oracle, P, crafted[s])
            got1, types1, st1 = _merged(ctx, oracle, P, apri1, _plain(ctx, oracle, P, apri1), 3, mc.YAML)
            src = r["apri_src"]
            assert np.array_equal(imr.canonical(got1[src]), got) and np.array_equal(types1[src], types), s
            assert {k: st[k] for k in STAT_KEYS} == {k: st1[k] for k in STAT_KEYS}
            for k in STAT_KEYS:
                total[k] += st[k]
            fused += st["fusions"] > 0
        assert {k: stats[k] for k in STAT_KEYS} == total and stats["scans_fused"] == fused == 3

    check()
    # the same batch with a scan in the middle whose pairs outgrow their scratch
    c.batch_process(d_over, offs_over)
    c.batch_cluster()
    c.batch_cluster_types()
    for s in range(3):
        assert c.batch_fetch(s)["n_apri"] == len(crafted_over[s])      # (the scan tables themselves stay readable)
        with pytest.raises(scvod.ScvodError, match="outgrew"):
            c.batch_fetch_clusters(s, 4096)
        with pytest.raises(scvod.ScvodError, match="outgrew"):
            c.batch_fetch_cluster_types(s, 4096)
    with pytest.raises(scvod.ScvodError, match="outgrew"):
        c.batch_track(np.zeros((3, 12), np.float32))
    with pytest.raises(scvod.ScvodError, match="outgrew"):
        c.batch_cluster_merge_stats()
    check()     # the first batch again: latch and counters cleared


@pytest.mark.parametrize("seed", [0, 2, 6])
def test_aliased_voxels_and_tied_keys(ctx, oracle, P, seed):
    """blobs with 5 % of their points on the x axis: voxels next to the -1 bins hold points of several clusters, and clusters share
    their smallest voxel key.  The kernel takes tied clusters in ascending name; the CPU file shows that the order does not matter
    for these seeds"""
    apri = oracle.bin(P, mc.blobs(seed), True)["apri"]
    assert (apri["sector_idx"] < 0).sum() > 0
    pre = _plain(ctx, oracle, P, apri)
    for params in (mc.YAML, mc.DEFAULTS):
        for iterations in (1, 3):
            _, _, st = _merged(ctx, oracle, P, apri, pre, iterations, params)
            assert st["key_ties"] >= 2 and st["fusions"] > 0


def test_grid_beyond_the_lds_is_refused(scvod, new_ctx, oracle):
    fine = scvod.make_params(mc.PRESET, range_res=0.05, azimuth_res=0.25)
    R, S, Az = oracle.grid_dims(fine)[:3]
    assert R * Az > 40960
    apri = oracle.bin(fine, mc.blobs(1, n_blobs=20, pts=30), True)["apri"]
    c = new_ctx(fine, max_points_total=len(apri) + 64, max_scans=1)
    c.set_intensity_merge(3, *mc.YAML)
    c.voxelize(apri)
    with pytest.raises(scvod.ScvodError, match="bytes of LDS"):
        c.batch_cluster()
    _plain(c, oracle, fine, apri)      # with the merge off the same ctx clusters the scan as the reference does
