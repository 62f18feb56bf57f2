"""scvod_batch_track against CRAFTED successor tables at every size tier of csrc/scvod_track.hip.

Two parts of the tracking path switch on the size nv of the successor's voxel table: k_tk_probe stages the keys sampled every 2^shift
records (shift rises at nv = 8193, 16385, 32769, ...) and bisects the 2^shift records behind a sample, the last block cut at nv;
launch_track_batch runs k_tk_decide once per LDS bitset size (1024, 2560, 4096 words and words = max_scan_pts / 32 + 1 of the batch),
each launch taking the tables between the previous size and its own, the last one also those beyond `words` (by selection, without a
bitset).  Which launches exist depends on the LARGEST SCAN of the batch, not on the table.

An external table (include/scvod.h, scvod_batch_export_table) is a plain int32 [nv + 1, 4] device tensor, so a table of exactly the
size wanted is built with numpy: craft_table() below.  The scene is one scan of a few thousand car clusters (test_gpu_parity's post
field plus one wide thin plate that lands on more than 64 voxels); a second scan -- the scene again, padded with points beyond the range
gate -- sets max_scan_pts and has no successor.  Every result is compared exactly with tests/helpers/track_table_ref.py (numpy,
pinned against the oracle by tests/test_track_table_ref.py), never with another run of the device.

Mutations these tests were seen to catch: `nw < min_words` for `<=` in k_tk_decide (a table on a tier boundary is decided twice); the
4096-word launch skipped while the next one still starts above it; the probe's block end `a0 + (1 << shift) - 1` for the cut at nv;
`first.y != -1` dropped in tk_find_slot; and the ladder as it was before the last launch took the tables beyond `words`."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import track_table_ref as ttr

pytestmark = pytest.mark.gpu

K_SAMPLES = 8192                       # kTkSamples of scvod_track.hip
SIZES = (0, 1, 8192, 8193, 16384, 16385, 32768, 32769, 81920, 81921, 131072, 131073)
SPARE = 64                             # records behind a table, filled with a record that would be a hit: nothing may read them
# points of the second scan: the scene alone, ~100 000 and ~150 000 (multiples of 32) -> words in (1024, 2560], (2560, 4096], above
PAD_POINTS = (0, 100000, 150016)
FIELDS = ("cluster_root", "cluster_state", "n_unique", "pair_begin", "pair_label", "pair_count", "pt_dyn")


def sample_shift(nv):
    """the sampling of k_tk_probe: every 2^shift-th key, at most K_SAMPLES of them"""
    shift = 0
    while ((nv + (1 << shift) - 1) >> shift) > K_SAMPLES:
        shift += 1
    return shift


def boundary_records(nv):
    """the first record b of a sample block near the start, the middle and the end of a table: hits are wanted at b - 1 and b"""
    blk = 1 << sample_shift(nv)
    ns = (nv + blk - 1) // blk
    return sorted({b for b in (blk, (ns // 2) * blk, (ns - 1) * blk) if 2 <= b <= nv - 1})


def _ratio_pads(h, occ):
    """the fewest records f that put h hits of a cluster of h + f voxels BELOW the ratio (fp32, ssc.cpp:1336)"""
    f = 0
    while not (np.float32(h) / np.float32(h + f) < np.float32(occ)):
        f += 1
    return f


def _move(g, cap, lo, hi, amount):
    """adds `amount` fillers to (takes -amount from) the gaps lo .. hi - 1, nearest to hi first; returns what could not be placed"""
    for j in range(hi - 1, lo - 1, -1):
        if amount == 0:
            break
        d = min(amount, cap[j] - g[j]) if amount > 0 else -min(-amount, g[j])
        g[j] += d
        amount -= d
    return amount


def craft_table(landing_keys, nv, rng, occupancy=0.5):
    """A successor table of exactly nv records for a scan whose car cluster c lands on the keys landing_keys[c].

    A subset of the landing keys is present, the rest of the records are fillers no point lands on.  Labels are consistent (a label's
    size column counts its records, its type is one value) and arranged so that the scan's clusters meet every branch of the state
    rule: keys absent (no hit), records with label -1 under landing points (no hit), one car / one non-car label just below and
    exactly at the ratio, several labels, and -- the cluster with the most keys -- one label per key.  The three smallest and three
    largest landing keys stay absent, the next ones are records 0 and nv - 1, and the records on both sides of the sample-block
    boundaries of boundary_records(nv) are present keys with a label.
    -> keys, label, size, type (ascending key), and the records that were placed on purpose"""
    per = [np.unique(np.asarray(k, np.int64)) for k in landing_keys]
    L = np.unique(np.concatenate(per))
    empty = np.zeros(0, np.int32)
    if nv == 0:
        return empty, empty, empty, empty, []
    assert len(L) > 64
    cand = L[3:-3]
    if nv == 1:  # one record, a hit for whoever lands on it
        return np.array([cand[len(cand) // 2]], np.int32), np.array([9], np.int32), np.array([1], np.int32), np.array([ttr.TYPE_CAR], np.int32), [0]
    assert nv >= 4096, "sizes between 2 and 4095 are not laid out"
    owner = {}
    for c, ks in enumerate(per):
        for k in ks.tolist():
            owner.setdefault(k, c)
    names = iter(rng.permutation(4 * nv + 1024).tolist())  # label ids: distinct, unordered
    lab_of_key, typ_of_label, pads_of_label = {}, {}, {}
    forbidden = set(L[:3].tolist()) | set(L[-3:].tolist())
    budget = nv - 16
    used = 0

    def new_label(typ, pads=0):
        l = next(names)
        typ_of_label[l] = typ
        pads_of_label[l] = pads
        return l

    big = int(np.argmax([len(k) for k in per]))
    first = [big, owner[int(cand[0])], owner[int(cand[-1])]]
    order = first + [c for c in rng.permutation(len(per)).tolist() if c not in first]
    cats = rng.choice(7, len(per), p=[0.12, 0.10, 0.20, 0.20, 0.13, 0.13, 0.12])
    cats[first[1]] = cats[first[2]] = 2
    cats[big] = 6
    for c in order:
        ks = [k for k in per[c].tolist() if k not in forbidden and k not in lab_of_key]
        cat, h = int(cats[c]), len(ks)
        if h == 0 or cat == 0:
            continue  # its keys stay absent
        if c == big:
            if used + h > budget:
                continue
            for k in ks:
                lab_of_key[k] = new_label(ttr.TYPE_CAR)  # more labels than the chain's 64-entry table, one voxel each
            used += h
            continue
        if cat == 6 and h < 2:
            cat = 3
        below = _ratio_pads(h, occupancy)
        pads = {1: 0, 2: below, 3: below - 1, 4: below, 5: below - 1, 6: 0}[cat]
        if used + h + pads > budget:
            continue
        used += h + pads
        if cat == 1:
            for k in ks:
                lab_of_key[k] = -1
        elif cat == 6:
            two = [new_label(ttr.TYPE_CAR), new_label(ttr.TYPE_OTHER if h % 2 else ttr.TYPE_CAR)]
            for n, k in enumerate(ks):
                lab_of_key[k] = two[n % 2]
        else:
            l = new_label(ttr.TYPE_CAR if cat in (2, 3) else ttr.TYPE_OTHER, pads)
            for k in ks:
                lab_of_key[k] = l
    S = np.array(sorted(lab_of_key), np.int64)
    assert S[0] == cand[0] and S[-1] == cand[-1] and lab_of_key[int(S[0])] != -1 and lab_of_key[int(S[-1])] != -1
    n_fill = nv - len(S)
    assert n_fill > 0
    # free keys (no point lands on them) between consecutive present keys, and how many of them each gap takes
    span = np.arange(S[0], S[-1] + 1)
    free = np.ones(len(span), bool)
    free[L[(L >= S[0]) & (L <= S[-1])] - S[0]] = False
    before = np.cumsum(free) - free            # free keys below a position
    at_S = before[S - S[0]]
    cap = np.diff(at_S)
    assert cap.sum() >= n_fill, f"{int(cap.sum())} free keys between the landing keys, {n_fill} fillers wanted"
    g = (cap * (n_fill / cap.sum())).astype(np.int64)
    assert _move(g, cap, 0, len(g), n_fill - int(g.sum())) == 0
    # two present keys side by side at the records b - 1 and b, both with a label (a fresh one where the draw left them erased)
    placed, lo = [0, nv - 1], 0
    for b in boundary_records(nv):
        pos = np.arange(len(S)) + np.concatenate([[0], np.cumsum(g)])
        ok = np.arange(lo + 1, len(S) - 1)  # (a gap below i is needed to move it; the present keys on either side must fit)
        ok = ok[(ok <= b - 1) & (len(S) - 2 - ok <= nv - 1 - b) & ((ok + 2 < len(S)) | (b == nv - 1))]
        for i in ok[np.argsort(np.abs(pos[ok] - (b - 1)), kind="stable")][:256].tolist():  # the nearest pair the gaps have room for
            g2 = g.copy()
            g2[i] = 0
            need = (b - 1) - int(pos[i])
            if _move(g2, cap, lo, i, need) == 0 and _move(g2, cap, i + 1, len(g), int(g[i]) - need) == 0:
                break
        else:
            raise AssertionError(f"no room to move a present key onto record {b - 1} of {nv}")
        g = g2
        for k in (int(S[i]), int(S[i + 1])):
            if lab_of_key[k] == -1:
                lab_of_key[k] = new_label(ttr.TYPE_CAR)
        placed += [b - 1, b]
        lo = i + 1
    assert int(g.sum()) == n_fill and (g >= 0).all() and (g <= cap).all()
    gap = np.searchsorted(S, span, "right") - 1
    gap_c = np.minimum(gap, len(g) - 1)
    fillers = span[free & (before - at_S[gap_c] < g[gap_c])]
    assert len(fillers) == n_fill
    # filler labels: the pads of the ratio clusters first, then clusters of their own and erased records
    flab = []
    for l, p in pads_of_label.items():
        flab += [l] * p
    while len(flab) < n_fill:
        n = int(min(rng.integers(1, 60), n_fill - len(flab)))
        flab += [-1] * n if rng.random() < 0.3 else [new_label(int(rng.integers(1, 3)))] * n
    flab = np.array(flab, np.int64)[rng.permutation(n_fill)]
    keys = np.concatenate([S, fillers])
    label = np.concatenate([np.array([lab_of_key[int(k)] for k in S], np.int64), flab])
    o = np.argsort(keys)
    keys, label = keys[o], label[o]
    u, inv, cnt = np.unique(label, return_inverse=True, return_counts=True)
    size = np.where(label == -1, 0, cnt[inv])
    typ = np.array([ttr.TYPE_ERASED if l == -1 else typ_of_label[l] for l in label.tolist()], np.int64)
    assert len(keys) == nv and (np.diff(keys) > 0).all()
    assert not np.isin(fillers, L).any() and (label[placed] != -1).all() and np.isin(keys[placed], L).all()
    assert keys[0] > L[2] and keys[-1] < L[-3]
    return keys.astype(np.int32), label.astype(np.int32), size.astype(np.int32), typ.astype(np.int32), placed


def _scene():
    """test_gpu_parity's field of thin posts and a flat plate 6 m wide and 1 m high across the x axis (a `car` by the box rules: the
    footprint of its bounding box is small) whose points land on more than 64 voxels; a multiple of 32 points"""
    from test_gpu_parity import _post_field
    x = _post_field(0.0, [])[0]
    yy, zz = np.meshgrid(np.arange(-3.0, 3.0, 0.04), np.arange(-1.5, -0.5, 0.05))
    plate = np.stack([np.full(yy.size, 8.37), yy.ravel(), zz.ravel(), np.full(yy.size, 0.5)], 1).astype(np.float32)
    x = np.concatenate([x, plate])
    return np.ascontiguousarray(x[len(x) % 32:])


def _far(n, rng):
    """points beyond the range gate: the binning rejects them"""
    a = rng.uniform(0, 2 * np.pi, n)
    r = rng.uniform(100.0, 120.0, n)
    return np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-1.0, 1.0, n), np.full(n, 0.3)], 1).astype(np.float32)


class _Geometry:
    """the scene and its padded copy segmented on the device, the helper's view of the scene scan, and one tracking call per table"""

    def __init__(self, scvod, oracle, pad_points, landing_cache):
        import torch
        self.torch = torch
        self.P = scvod.make_params("semantickitti")
        scene = _scene()
        rng = np.random.default_rng(5)
        second = np.concatenate([scene, _far(max(pad_points - len(scene), 0), rng)])
        offs = np.array([0, len(scene), len(scene) + len(second)], np.int32)
        self.max_scan_pts = int(np.diff(offs).max())
        assert self.max_scan_pts % 32 == 0 and self.max_scan_pts == max(pad_points, len(scene))
        self.words = self.max_scan_pts // 32 + 1  # of the last launch of launch_track_batch
        self.ctx = ctx = scvod.Ctx(self.P, max_points_total=int(offs[-1]) + 64, max_scans=2)
        self.d = torch.from_numpy(np.concatenate([scene, second])).cuda()
        ctx.batch_process(self.d, offs)
        ctx.batch_cluster()
        ctx.batch_cluster_types()
        r = ctx.batch_fetch(0)
        self.n_apri = r["n_apri"]
        assert ctx.batch_fetch(1)["n_apri"] == self.n_apri, "the padding must not survive the binning"
        names = ctx.batch_fetch_clusters(0, self.n_apri)
        self.types = ctx.batch_fetch_cluster_types(0, self.n_apri, car_label=2, other_label=1)
        self.clusters, self.roots = ttr.car_clusters(names, self.types)
        self.T = np.zeros((2, 12), np.float32)
        self.T[0] = oracle.pose_delta([0, 0, 0, 0, 0, 0], [0.4, 0.1, 0, 0, 0, 0.01])
        car = np.concatenate(self.clusters)
        a = r["apri"][car]
        xyzi = np.stack([a["x"], a["y"], a["z"], a["intensity"]], 1).astype(np.float32)
        key = xyzi.tobytes()
        if key not in landing_cache:  # (the scene scan is the same in every geometry)
            landing_cache.clear()
            landing_cache[key] = ttr.landing_keys(oracle, self.P, xyzi, self.T[0], 0, oracle.grid_dims(self.P)[3])
        self.landing = np.full(self.n_apri, ttr.NO_KEY, np.int32)
        self.landing[car] = landing_cache[key]
        self.per_cluster = [self.landing[m] for m in self.clusters]
        self.poison = (int(np.max(self.landing[car])), 7, 1, ttr.TYPE_CAR)  # the largest landing key: never part of a table

    def table(self, nv, seed):
        return craft_table(self.per_cluster, nv, np.random.default_rng(seed), self.P.occupancy)

    def track(self, tab, chain=False, spare=SPARE):
        keys, label, size, typ = tab[:4]
        host = ttr.pack_table(keys, label, size, typ, spare_records=spare)
        host[1 + len(keys):] = self.poison
        dev = self.torch.from_numpy(host).cuda()
        self.ctx.set_track_mode(chain=chain)
        self.ctx.batch_track(self.T, next_scan=np.array([-2, -1], np.int32), ext_tables=[dev])
        got = [self.ctx.batch_fetch_track(s) for s in range(2)]
        stats = self.ctx.batch_track_stats()
        want = ttr.decide(self.clusters, self.roots, self.landing, keys, label, size, typ, self.P.occupancy, n_apri=self.n_apri, pt_type=self.types)
        return got, want, stats

    def check(self, tab, chain=False, spare=SPARE):
        nv = len(tab[0])
        got, want, stats = self.track(tab, chain, spare)
        for k in FIELDS:
            assert np.array_equal(got[0][k], want[k]), (nv, k, int((got[0][k] != want[k]).sum()) if got[0][k].shape == want[k].shape else "shape")
        assert got[0]["n_dynamic_clusters"] == want["n_dynamic_clusters"] and got[0]["n_dynamic_points"] == want["n_dynamic_points"], nv
        # the padded copy of the scene has no successor: as many car clusters, nothing decided
        assert got[1]["n_clusters"] == len(self.roots) and (got[1]["cluster_state"] == -1).all() and not (got[1]["pt_dyn"] == 1).any()
        assert got[1]["n_dynamic_clusters"] == 0 and got[1]["n_dynamic_points"] == 0
        assert stats["error_bits"] == 0
        return want


@pytest.fixture(scope="module")
def geometries(scvod, oracle):
    made, landing_cache = {}, {}

    def get(pad_points):
        if pad_points not in made:
            made[pad_points] = _Geometry(scvod, oracle, pad_points, landing_cache)
        return made[pad_points]
    yield get
    for g in made.values():
        g.ctx.close()


def _assert_every_branch(want, tab, per_cluster, occupancy):
    keys, label, size, typ, placed = tab
    st, npairs = want["cluster_state"], np.diff(want["pair_begin"])
    one = np.nonzero(npairs == 1)[0]
    rec = np.array([want["uniq"][c][0] for c in one])
    below = np.array([np.float32(want["n_unique"][c]) / np.float32(size[r]) < np.float32(occupancy) for c, r in zip(one, rec)])
    car = typ[rec] == ttr.TYPE_CAR
    assert (st[npairs == 0] == 1).all() and (npairs == 0).sum() > 0                                   # no hit: dynamic
    assert (st[one[car & below]] == 1).all() and (car & below).sum() > 0                              # one car label below: dynamic
    assert (st[one[car & ~below]] == 0).all() and (car & ~below).sum() > 0                            # at or above: static
    assert (st[one[~car & below]] == 0).all() and (~car & below).sum() > 0                            # one non-car label below: static
    assert (st[one[~car & ~below]] == -1).all() and (~car & ~below).sum() > 0                         # at or above: untouched
    assert (st[npairs > 1] == 0).all() and (npairs > 1).sum() > 0                                     # several labels: static
    assert npairs.max() > 64                                                                          # more labels than the chain's fast table
    hit = np.unique(np.concatenate(want["uniq"]))
    assert np.isin(placed, hit).all(), "records 0, nv - 1 and both sides of the sample boundaries must be hit"
    # records with label -1 under landing points, landing keys below the first and above the last key
    land = np.unique(np.concatenate(per_cluster))
    assert (label[np.isin(keys, land)] == -1).any() and land[0] < keys[0] and land[-1] > keys[-1]


@pytest.mark.parametrize("pad_points", PAD_POINTS)
def test_first_order_decision_against_crafted_tables(geometries, pad_points):
    """every size of SIZES, the largest table the last launch's bitset holds (32 * words) and the first it does not (32 * words + 1:
    decided by selection in that launch), in a batch whose launch ladder ends in each of the three ranges"""
    g = geometries(pad_points)
    lo, hi = {0: (1024, 2560), 100000: (2560, 4096), 150016: (4096, 16385)}[pad_points]
    assert lo < g.words <= hi, (g.max_scan_pts, g.words)
    assert len(g.roots) > 1536
    for n, nv in enumerate(sorted(set(SIZES) | {32 * g.words, 32 * g.words + 1})):
        tab = g.table(nv, 100 + n)
        want = g.check(tab, spare=1 if nv == 0 else SPARE)
        if nv == 0:
            assert (want["cluster_state"] == 1).all() and want["n_dynamic_points"] == sum(len(m) for m in g.clusters)
        elif nv == 1:
            assert want["n_unique"].sum() >= 1 and (want["cluster_state"] != -1).all()
        else:
            _assert_every_branch(want, tab, g.per_cluster, g.P.occupancy)


def test_chain_mode_decides_an_external_table_the_same(geometries):
    """the default mode: an external table ends a chain, so the decision is the first-order one -- one table per launch of the ladder"""
    g = geometries(PAD_POINTS[2])
    for n, nv in enumerate((20000, 50000, 100000, 32 * g.words - 7, 32 * g.words + 33)):
        g.check(g.table(nv, 200 + n), chain=True)


@pytest.mark.parametrize("pad_points", PAD_POINTS[1:])
def test_a_smaller_table_after_a_larger_one(geometries, pad_points):
    """two calls back to back on one ctx, the larger table first: what a tier left in its bitset, in tk_uniq or in the kernel's
    dynamic-LDS attribute must not reach the next call"""
    g = geometries(pad_points)
    for n, nv in enumerate((32 * g.words + 1, 90000, 32 * g.words, 9000, 70000, 0, 33000)):
        g.check(g.table(nv, 300 + n), spare=1 if nv == 0 else SPARE)
