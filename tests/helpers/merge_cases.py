"""Crafted scans for the intensity merge (csrc/scvod_k_merge.inc): points placed at the centres of chosen bins of the `semantickitti`
grid (72 x 300 x 60), so that the pre-merge clusters, the neighbour pairs the kernel emits and the fusions are known by construction.
tests/test_intensity_merge_cases.py pins those preconditions on the CPU, tests/test_gpu_intensity_merge_crafted.py runs the scans on
the device.  A voxel is (range bin, sector bin, azimuth bin, [intensities of its points]); the points of a scan follow the list.

The clustering joins voxels within radius 1, so voxels two bins apart are clusters of their own and consecutive bins are one cluster;
the merge (YAML search_c = 2) sees two bins out, below range bin 0.6 R = 43.2 only."""
import numpy as np

import intensity_merge_ref as imr

PRESET = "semantickitti"
GRID = (72, 300, 60)
YAML = (2, 2.0, 1.0)        # search_c, intensity_diff, intensity_cov of both shipped YAML files
DEFAULTS = (2, 50.0, 20.0)  # the reference's values when the YAML omits the keys
PAIRS_PER_POINT, PAIRS_PER_SCAN = 4, 256   # include/scvod.h: a scan of n points holds 4 n + 256 neighbour pairs


def _oracle():
    import oracle_py
    return oracle_py.load()


def pair_limit(n_points):
    return PAIRS_PER_POINT * n_points + PAIRS_PER_SCAN


def scan(P, voxels):
    """xyzi rows [n, 4] float32 of the voxels' points, each at the centre of its bin; asserts that the filtered binning keeps every
    point and puts it into the bin asked for"""
    rows, want = [], []
    for r, s, a, intensities in voxels:
        dis = P.min_dis + (r + .5) * P.range_res
        angle = np.deg2rad(P.min_angle + (s + .5) * P.sector_res)
        az = np.deg2rad(P.min_azimuth + (a + .5) * P.azimuth_res)
        for i in intensities:
            rows.append((dis * np.cos(angle), dis * np.sin(angle), dis * np.tan(az), i))
            want.append((r, s, a))
    x = np.asarray(rows, np.float32)
    apri = _oracle().bin(P, x, True)["apri"]
    assert len(apri) == len(x), f"the filter dropped {len(x) - len(apri)} of {len(x)} crafted points"
    got = np.stack([apri["range_idx"], apri["sector_idx"], apri["azimuth_idx"]], 1)
    assert np.array_equal(got, np.asarray(want)), "a crafted point left its bin"
    return x


def with_ground(x, seed):
    """x followed by a ground disc: 20 000 points at z = -1.73 +- 0.02 between 2 and 35 m.  Patchwork then removes the disc and keeps
    every crafted point (tests/test_intensity_merge_cases.py asserts it for the scans the batch tests use)"""
    rng = np.random.default_rng(seed)
    n = 20000
    rad = rng.uniform(2.0, 35.0, n)   # (uniform in radius: the small patches next to the sensor get their share)
    th = rng.uniform(0, 2 * np.pi, n)
    disc = np.stack([rad * np.cos(th), rad * np.sin(th), -1.73 + rng.uniform(-0.02, 0.02, n), rng.uniform(0, 60, n)], 1)
    return np.concatenate([x, disc.astype(np.float32)])


def shuffled(voxels, seed):
    """the same voxels in a seeded order: cluster names (smallest point index) stop following the bins"""
    order = np.random.default_rng(seed).permutation(len(voxels))
    return [voxels[i] for i in order]


def emitted_pairs(vox, names, grid, search_c, diff, cov):
    """(total, per_cluster): total = over every (voxel, cluster among its points) item, the number of distinct foreign labels among
    the voxel's kept neighbours; per_cluster[c] = foreign labels in the set S of cluster c.

    total equals the pair count the kernel reaches before sort and unique whenever no item meets more than four foreign labels, or
    meets every foreign label once only (one voxel per foreign cluster in its window): the kernel remembers the last four labels an
    item emitted and emits a label again when it comes back after four others.  Otherwise total is a LOWER bound of that count."""
    key, av, cv, idx3, slot, vlab, members, grid = imr._tables(vox, names, grid)
    total = 0
    per = {c: set() for c in members}
    for c, vs in members.items():
        for v in vs:
            seen = {int(vlab[u]) for u in imr._neighbour_set(v, key, av, cv, idx3, slot, grid, search_c, diff, cov)} - {c}
            total += len(seen)
            per[c] |= seen
    return total, {c: len(s) for c, s in per.items()}


# ---- generators --------------------------------------------------------------------------------------------------------------------
def lattice(nr, ns, na, r0=4, s0=20, a0=24, intensity=10.0):
    """nr x ns x na single-point voxels two bins apart in all three axes: one cluster each, every one sees all 26 around it"""
    return [(r0 + 2 * i, s0 + 2 * j, a0 + 2 * k, [intensity]) for k in range(na) for i in range(nr) for j in range(ns)]


def hub(m, r0=10, s0=10, a0=24):
    """2 m + 1 consecutive sector bins at one range and azimuth (one cluster, the hub), m single voxels two range bins out at every
    second sector, and a pair of single voxels far from both that fuse with each other.  A hub voxel holds two points of
    intensities 10 and 13: av 11.5, cov 2.25 -- above the YAML's 1.0, so nothing sees the hub, the hub itself included.  The singles
    alternate between 10 and 13: within 2.0 of the hub's 11.5, 3.0 from each other.  So a single's S is itself, and the hub's S is the
    m singles without the hub: the walk reads a run of exactly m pairs, every one valid, fuses the singles and leaves the hub alone.
    Hub points first: the hub is cluster 0 and its run stands first among the pairs, the far pair's behind it."""
    vs = [(r0, s0 + j, a0, [10.0, 13.0]) for j in range(2 * m + 1)]
    vs += [(r0 + 2, s0 + 1 + 2 * k, a0, [10.0 if k % 2 == 0 else 13.0]) for k in range(m)]
    vs += [(r0 + 20, s0, a0 + 6, [10.0]), (r0 + 20, s0 + 2, a0 + 6, [10.0])]
    return vs


def lines(count, length, intensity=10.0):
    """count rows of `length` single voxels two sector bins apart, the rows 7 bins from each other in range or azimuth.  A voxel sees
    the one before and the one after it: 2 (length - 1) pairs per row, all different"""
    assert length <= 150 and count <= 6 * 5
    out = []
    for c in range(count):
        r, a = 4 + 7 * (c % 6), 22 + 7 * (c // 6)   # (from 3.3 m: Patchwork drops what is nearer than 2.7 m)
        out += [(r, 2 * j, a, [intensity]) for j in range(length)]
    return out


def thick_lines(count, length):
    """count pairs of rows: `length` consecutive sector bins (one cluster) and the same two range bins out (another cluster).  Every
    voxel of a row sees the other row's label: 2 length pairs per pair of rows, of which 2 are different"""
    out = []
    for c in range(count):
        r, a = 4 + 7 * (c % 6), 22 + 7 * (c // 6)   # (from 3.3 m: Patchwork drops what is nearer than 2.7 m)
        out += [(r, 5 + j, a, [10.0]) for j in range(length)] + [(r + 2, 5 + j, a, [11.0]) for j in range(length)]
    return out


# the hand cases of tests/test_intensity_merge_ref.py on this grid, with the answer the reference's text gives (ssc.cpp:571-635):
# (name, voxels, iterations, (search_c, diff, cov), groups of voxel numbers that end in one cluster)
_A = 24
HAND_CASES = [
    ("gap_of_one_voxel_fuses", [(5, 5, _A, [10.0]), (5, 7, _A, [10.0])], 1, YAML, [[0, 1]]),
    ("gap_beyond_radius_one", [(5, 5, _A, [10.0]), (5, 7, _A, [10.0])], 1, (1, 2.0, 1.0), [[0], [1]]),
    ("cov_above_the_limit", [(5, 5, _A, [10.0]), (5, 7, _A, [8.5, 11.5])], 1, YAML, [[0], [1]]),           # cov 2.25 > 1.0
    ("cov_equal_to_the_limit", [(5, 5, _A, [10.0]), (5, 7, _A, [9.0, 11.0])], 1, YAML, [[0, 1]]),          # cov 1.0 <= 1.0
    ("cov_just_above_the_limit", [(5, 5, _A, [10.0]), (5, 7, _A, [9.0, 11.0])], 1, (2, 2.0, 0.999), [[0], [1]]),
    ("diff_above_the_limit", [(5, 5, _A, [10.0]), (5, 7, _A, [12.5])], 1, YAML, [[0], [1]]),
    ("diff_equal_to_the_limit", [(5, 5, _A, [10.0]), (5, 7, _A, [12.0])], 1, YAML, [[0, 1]]),              # 2.0 <= 2.0
    ("diff_just_above_the_limit", [(5, 5, _A, [10.0]), (5, 7, _A, [12.0])], 1, (2, 1.999, 1.0), [[0], [1]]),
    ("radius_two_below_0.6_R", [(40, 5, _A, [10.0]), (42, 5, _A, [10.0])], 1, YAML, [[0, 1]]),
    ("radius_two_at_bin_43", [(43, 5, _A, [10.0]), (45, 5, _A, [10.0])], 1, YAML, [[0, 1]]),               # 43 is not > 43.2
    ("radius_one_from_bin_44", [(44, 5, _A, [10.0]), (46, 5, _A, [10.0])], 1, YAML, [[0], [1]]),
    ("no_sector_wrap", [(5, 0, _A, [10.0]), (5, 299, _A, [10.0])], 1, YAML, [[0], [1]]),
    ("clipped_corner", [(0, 0, 0, [10.0]), (1, 2, 0, [10.0])], 1, YAML, [[0, 1]]),
    # the middle cluster's voxel fails the cov test: its S = {A, C} without itself; it records their fusion and stays
    ("cluster_outside_its_set", [(5, 2, _A, [10.0]), (5, 4, _A, [7.5, 12.5]), (5, 6, _A, [10.0])], 3, YAML, [[0, 2], [1]]),
    # the largest key goes first and fuses {B, C}; B is invalid when A is visited: A stays (ascending order would fuse {A, B})
    ("chain_first_iteration", [(5, 2, _A, [10.0]), (5, 4, _A, [10.0]), (5, 6, _A, [10.0])], 1, YAML, [[0], [1, 2]]),
    ("chain_second_iteration", [(5, 2, _A, [10.0]), (5, 4, _A, [10.0]), (5, 6, _A, [10.0])], 2, YAML, [[0, 1, 2]]),
]

# The far rule's own boundary.  On the preset's grid 0.6 R = 43.2 is no integer, so `>` and `>=` agree on every range bin and the
# cases above pin only WHERE the radius drops.  With max_dis = 29.5 the grid has R = 70 and 0.6 R = 42.0 exactly (in double): bin 42
# is not > 42 and still looks two bins out, bin 43 does not (tests/test_intensity_merge_ref.py does the same with R = 20, bin 12).
FAR_GRID_KW = dict(max_dis=29.5)
FAR_GRID = (70, 300, 60)
FAR_CASES = [
    ("radius_two_at_bin_42_of_70", [(42, 5, _A, [10.0]), (44, 5, _A, [10.0])], 1, YAML, [[0, 1]]),         # 42 is not > 42.0
    ("radius_one_from_bin_43_of_70", [(43, 5, _A, [10.0]), (45, 5, _A, [10.0])], 1, YAML, [[0], [1]]),
    ("radius_two_below_42_of_70", [(40, 5, _A, [10.0]), (42, 5, _A, [10.0])], 1, YAML, [[0, 1]]),
]


def groups_to_names(voxels, groups):
    """canonical name per point of the partition that puts the voxels of every group into one cluster"""
    first = np.concatenate([[0], np.cumsum([len(v[3]) for v in voxels])])
    names = np.zeros(first[-1], np.int64)
    for g in groups:
        t = min(first[v] for v in g)
        for v in g:
            names[first[v]:first[v + 1]] = t
    return names


def blobs(seed, n_blobs=60, pts=40, sigma=0.3, on_axis=0.05):
    """a seeded scan of Gaussian blobs all around the sensor, `on_axis` of the points moved onto the x axis.  On its positive half the
    polar angle is 0 and the sector index -1 under the filtered binning: such a point's voxel key is that of sector 299 one range bin
    below, whose voxel then holds points of several clusters -- clusters that can share their smallest voxel key"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(n_blobs):
        rad = rng.uniform(3.0, 25.0)
        th = rng.uniform(0, 2 * np.pi)
        c = np.array([rad * np.cos(th), rad * np.sin(th), rng.uniform(-0.5, 2.0)])
        p = c + rng.normal(0, sigma, (pts, 3))
        inten = rng.choice([10.0, 11.5, 13.0, 30.0]) + rng.normal(0, 0.8, pts)
        out.append(np.concatenate([p, inten[:, None]], 1))
    x = np.concatenate(out)
    x[rng.random(len(x)) < on_axis, 1] = 0.0
    return x[rng.permutation(len(x))].astype(np.float32)
