"""The preconditions of tests/test_gpu_intensity_merge_crafted.py, on the CPU: the crafted scans of tests/helpers/merge_cases.py land in
their bins, cluster as designed, emit the number of neighbour pairs each case is about (on both sides of the sort's and the
scratch's limits), and the scans with tied smallest voxel keys have one answer whatever order the ties are visited in.  Not gpu."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import intensity_merge_ref as imr  # noqa: E402
import merge_cases as mc  # noqa: E402


@pytest.fixture(scope="module")
def P(scvod):
    return scvod.make_params(mc.PRESET)


def _tables(oracle, P, x):
    apri = oracle.bin(P, x, True)["apri"]
    running, n_clusters, _ = oracle.cluster(P, apri)
    return apri, oracle.voxelize(P, apri), running, imr.canonical(running), n_clusters


def test_grid_is_the_one_the_cases_are_written_for(oracle, P):
    assert tuple(int(g) for g in oracle.grid_dims(P)[:3]) == mc.GRID
    assert 0.6 * mc.GRID[0] == pytest.approx(43.2)      # bins 43 and 44 straddle the far rule


def test_hand_cases_have_their_literal_answer(oracle, P):
    for name, voxels, iterations, params, groups in mc.HAND_CASES:
        apri, vox, running, pre, n_clusters = _tables(oracle, P, mc.scan(P, voxels))   # (scan asserts the bins)
        assert n_clusters == len(voxels), name                                          # every voxel starts as a cluster of its own
        want = mc.groups_to_names(voxels, groups)
        assert np.array_equal(imr.convention(vox, pre, mc.GRID, iterations, *params), want), name
        assert np.array_equal(imr.canonical(imr.literal(vox, running, mc.GRID, iterations, *params)), want), name


def test_far_rule_boundary_on_a_grid_where_it_is_an_integer(oracle, scvod):
    far = scvod.make_params(mc.PRESET, **mc.FAR_GRID_KW)
    assert tuple(int(g) for g in oracle.grid_dims(far)[:3]) == mc.FAR_GRID
    assert mc.FAR_GRID[0] * 0.6 == 42.0      # exactly, as ssc.cpp:397 computes it: `>` and `>=` differ at bin 42
    for name, voxels, iterations, params, groups in mc.FAR_CASES:
        apri, vox, running, pre, n_clusters = _tables(oracle, far, mc.scan(far, voxels))
        assert n_clusters == len(voxels), name
        want = mc.groups_to_names(voxels, groups)
        assert np.array_equal(imr.convention(vox, pre, mc.FAR_GRID, iterations, *params), want), name
        assert np.array_equal(imr.canonical(imr.literal(vox, running, mc.FAR_GRID, iterations, *params)), want), name


@pytest.mark.parametrize("m", [63, 64, 65, 128, 129])
def test_hub_is_one_cluster_whose_set_holds_m_labels(oracle, P, m):
    voxels = mc.hub(m)
    apri, vox, running, pre, n_clusters = _tables(oracle, P, mc.scan(P, voxels))
    assert n_clusters == m + 3                     # the hub, m singles, the far pair
    assert (pre[:2 * (2 * m + 1)] == 0).all()      # the hub is cluster 0
    total, per = mc.emitted_pairs(vox, pre, mc.GRID, *mc.YAML)
    assert per[0] == m and total <= mc.pair_limit(len(apri))
    assert sorted(per.values())[-2] == 1           # (the far pair; a single sees nothing)
    st = {}
    got = imr.convention(vox, pre, mc.GRID, 1, *mc.YAML, stats=st)
    assert st["fusions"] == 2 and st["clusters_after"] == 3
    assert (got[:2 * (2 * m + 1)] == 0).all() and len(set(got[2 * (2 * m + 1):-2])) == 1   # the hub fuses the singles and stays out


def test_capacity_bracket(oracle, P):
    want = {(3, 3, 3): 316, (4, 4, 3): 652, (6, 6, 4): 2416}
    for dims, pairs in want.items():
        voxels = mc.lattice(*dims)
        apri, vox, running, pre, n_clusters = _tables(oracle, P, mc.scan(P, voxels))
        assert n_clusters == len(voxels) == len(apri)
        for search_c in ((2, 3) if dims == (3, 3, 3) else (2,)):
            total, per = mc.emitted_pairs(vox, pre, mc.GRID, search_c, 2.0, 1.0)
            assert total == pairs and max(per.values()) == 26   # (every label once per item: the count is exact)
    assert 4 * 27 < 316 <= mc.pair_limit(27) == 364             # fits through the per-scan slack only
    assert 652 > mc.pair_limit(48) == 448
    assert 2416 > mc.pair_limit(144) == 832


LINES = [(4, 128), (4, 130), (8, 128), (8, 130), (16, 128), (16, 130)]


def test_lines_sizes_straddle_the_sort_sizes(oracle, P):
    totals = []
    deep = 0
    for count, length in LINES:
        voxels = mc.shuffled(mc.lines(count, length), 1)
        apri, vox, running, pre, n_clusters = _tables(oracle, P, mc.scan(P, voxels))
        assert n_clusters == len(voxels)
        total, per = mc.emitted_pairs(vox, pre, mc.GRID, *mc.YAML)
        assert total == 2 * count * (length - 1) and max(per.values()) == 2 and total <= mc.pair_limit(len(apri))
        totals.append(total)
        if count == 4:
            st = {}
            imr.convention(vox, pre, mc.GRID, 8, *mc.YAML, stats=st)
            deep = max(deep, sum(f > 0 for f in st["fusions_per_iteration"]))
    assert totals[0] < 1024 < totals[1] and totals[2] < 2048 < totals[3] and totals[4] < 4096 < totals[5]
    assert deep >= 4      # fusions of fusions: the names of a line are chained through at least four iterations


def test_repeated_pairs_scan(oracle, P):
    voxels = mc.shuffled(mc.thick_lines(5, 120), 2)
    apri, vox, running, pre, n_clusters = _tables(oracle, P, mc.scan(P, voxels))
    assert n_clusters == 10
    total, per = mc.emitted_pairs(vox, pre, mc.GRID, *mc.YAML)
    assert total == 1200 > 1024 and total <= mc.pair_limit(len(apri))
    assert sum(per.values()) == 10      # what is left after the unique: runs of 120 equal pairs, one of them across index 1024


def test_ground_disc_leaves_the_crafted_points(oracle, P):
    for k, voxels in enumerate([mc.hub(64), mc.shuffled(mc.lines(4, 128), 1), mc.lattice(3, 3, 3), mc.lattice(4, 4, 3)]):
        x = mc.scan(P, voxels)
        ng = oracle.patchwork(P, mc.with_ground(x, k))["nonground_idx"]
        assert np.array_equal(np.sort(ng), np.arange(len(x))), k     # (in the order of Patchwork's patches)


BLOB_SEEDS = [0, 2, 6]   # (of seeds 0..7 the three with the most ties: 37, 11, 14)


@pytest.mark.parametrize("seed", BLOB_SEEDS)
def test_tied_smallest_keys_do_not_decide_the_partition(oracle, P, seed):
    apri, vox, running, pre, n_clusters = _tables(oracle, P, mc.blobs(seed))
    assert (apri["sector_idx"] < 0).sum() > 0
    for params in (mc.YAML, mc.DEFAULTS):
        for iterations in (1, 3):
            st = {}
            got = imr.convention(vox, pre, mc.GRID, iterations, *params, stats=st)
            assert st["key_ties"] >= 2 and st["fusions"] > 0
            assert np.array_equal(got, imr.convention(vox, pre, mc.GRID, iterations, *params, ties="asc"))
            assert np.array_equal(got, imr.convention(vox, pre, mc.GRID, iterations, *params, ties="desc"))
            if iterations == 1:
                assert np.array_equal(got, imr.canonical(imr.literal(vox, running, mc.GRID, 1, *params)))


def test_lds_refusal_grid(oracle, scvod):
    fine = scvod.make_params(mc.PRESET, range_res=0.05, azimuth_res=0.25)
    R, S, Az = oracle.grid_dims(fine)[:3]
    assert R * Az > 40960      # 160 KB of LDS hold 40 960 row starts
