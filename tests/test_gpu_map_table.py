"""The static map's hash table, its exports and its accumulation kernel (csrc/scvod_map.hip) on inputs built to go wrong.

Part 1 drives the table alone through records made in numpy (merge / export / count / export_parts / export_parts_padded / points /
clear): load up to 0.95 with probe chains of up to 383 slots, chains that wrap round the end of the table, 300 keys on one home slot,
a table that overflows, output buffers that are too small.  The reference of every case is the definition: per distinct key the
smallest value, padding keys ignored (tests/helpers/map_ref.py).

Part 2 drives k_map_accumulate with controlled geometry through batch_process + SCVOD_MAP_IGNORE_DYNAMIC.  The kept set is the set of
points the ORACLE's Patchwork does not drop; keys and values are the fp32 definition (map_ref.encode_points).  The last test closes the
loop with tests/test_pose_matrix.py: what points() hands out against the input points moved in fp64 by the elementary-rotation matrix."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import map_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu

ERR_CAPACITY = -4                       # SCVOD_ERR_CAPACITY
SENT = 0x5555555555555555               # pre-fill of output buffers: neither a record the tests make nor padding
BARRIER = 384                           # every BARRIER-th slot stays empty in the load cases: no run longer than 383 < 400 < 512


def _status(excinfo):
    m = re.match(r"status (-?\d+)", str(excinfo.value))
    assert m, str(excinfo.value)
    return int(m.group(1))


def _raw_export(m, rows, cap=None):
    """scvod_map_export through the C ABI into a sentinel-filled buffer of `rows` records: (status, n_out, buffer as uint64 [rows, 2])"""
    import torch
    buf = torch.full((rows, 2), SENT, dtype=torch.int64, device="cuda")
    n = C.c_int64(-1)
    rc = m.lib.scvod_map_export(m.h, C.c_void_p(buf.data_ptr()), rows if cap is None else cap, C.byref(n), None)
    return rc, int(n.value), buf.cpu().numpy().view(np.uint64)


def _keys_behind_barriers(rng, capacity, n, first_barrier=0):
    """n distinct keys whose linear-probing table leaves every slot first_barrier + i * BARRIER empty (keys that would land there are
    left out), so its runs of occupied slots are at most BARRIER - 1 long whatever the load"""
    barrier = np.zeros(capacity, bool)
    barrier[first_barrier::BARRIER] = True
    occ = bytearray(capacity)
    cand = mr.random_keys(rng, 4 * n + 4096)
    out = []
    for k, h in zip(cand.tolist(), mr.home(cand, capacity).tolist()):
        while occ[h]:
            h = (h + 1) & (capacity - 1)
        if barrier[h]:
            continue
        occ[h] = 1
        out.append(k)
        if len(out) == n:
            break
    assert len(out) == n
    return np.asarray(out, np.uint64)


def _keys_with_home(rng, capacity, n, lo, hi):
    """n distinct keys whose home slot lies in [lo, hi)"""
    out = np.zeros(0, np.uint64)
    while len(out) < n:
        cand = mr.random_keys(rng, 1 << 18)
        h = mr.home(cand, capacity)
        out = np.unique(np.concatenate([out, cand[(h >= lo) & (h < hi)]]))
    return rng.permutation(out)[:n]


def _records(rng, keys, max_rep=8, pad_share=0.15):
    """every key 1 to max_rep times with different values, shuffled, padding records (key ~0, any value) in between"""
    rep = rng.integers(1, max_rep + 1, len(keys))
    k = np.repeat(keys, rep)
    v = mr.random_keys(rng, len(k))                       # distinct 63-bit values
    n_pad = int(len(k) * pad_share) + 3
    k = np.concatenate([k, np.full(n_pad, mr.PAD, np.uint64)])
    v = np.concatenate([v, rng.integers(0, 1 << 63, n_pad, dtype=np.uint64)])
    v[-1] = mr.PAD                                        # (what a gathered, memset list holds)
    o = rng.permutation(len(k))
    return k[o], v[o]


def _merge_and_check(scvod, capacity, keys, rng, chunks=1):
    occ = mr.simulate_table(keys, capacity)
    run, wraps = mr.longest_run(occ)
    assert run <= 400, "precondition: no insertion may need 512 probes in any order"
    k, v = _records(rng, keys)
    ek, ev = mr.reduce_records(k, v)
    assert np.array_equal(ek, np.sort(keys))
    m = scvod.StaticMap(capacity)
    assert m.lib.scvod_map_capacity(m.h) == capacity
    rec = mr.to_device(k, v)
    for part in np.array_split(np.arange(len(k)), chunks):
        m.merge(rec[int(part[0]):int(part[-1]) + 1])
    assert m.count() == len(ek)                           # (raises if anything was dropped)
    gk, gv = mr.sorted_records(m)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    m.merge(rec)                                          # idempotent
    gk, gv = mr.sorted_records(m)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    m.close()
    return run, wraps


# ---------------------------------------------------------------- part 1: the table alone

@pytest.mark.parametrize("capacity", [1024, 4096])
@pytest.mark.parametrize("load", [0.5, 0.9, 0.95])
def test_table_under_load(scvod, capacity, load):
    rng = np.random.default_rng(1000 + capacity + int(load * 100))
    keys = _keys_behind_barriers(rng, capacity, int(capacity * load))
    run, _ = _merge_and_check(scvod, capacity, keys, rng, chunks=3)
    if load >= 0.9:
        assert run >= 100                                 # the case is about long probe chains


def test_probe_chain_wraps_round_the_end_of_the_table(scvod):
    capacity = 1024
    rng = np.random.default_rng(11)
    # (a) 300 keys at home in the last 24 slots: one run, from slot >= 1000 over the end to slot ~275
    keys = _keys_with_home(rng, capacity, 300, 1000, 1024)
    run, wraps = _merge_and_check(scvod, capacity, keys, rng)
    assert wraps and run >= 300
    # (b) 300 keys on ONE home slot, 50 slots before the end: the last of them probes 300 slots, 250 of them behind the wrap
    keys = _keys_with_home(rng, capacity, 300, capacity - 50, capacity - 49)
    assert (mr.home(keys, capacity) == capacity - 50).all()
    run, wraps = _merge_and_check(scvod, capacity, keys, rng)
    assert wraps and run == 300
    # (c) the same with unrelated keys around: the run only grows inside the bound
    more = np.concatenate([keys, _keys_with_home(rng, capacity, 60, 300, 900)])
    run, wraps = _merge_and_check(scvod, capacity, more, rng)
    assert wraps


def test_overflow_is_reported_bounded_and_cleared(scvod):
    capacity = 1024
    rng = np.random.default_rng(12)
    keys = mr.random_keys(rng, 2000)
    k, v = _records(rng, keys, max_rep=3)
    ek, ev = mr.reduce_records(k, v)
    m = scvod.StaticMap(capacity)
    m.merge(mr.to_device(k, v))
    with pytest.raises(scvod.ScvodError) as e:
        m.count()
    assert _status(e) == ERR_CAPACITY
    rc, n, buf = _raw_export(m, capacity + 8)
    assert rc == ERR_CAPACITY and 512 <= n <= capacity    # (an insertion is only dropped behind 512 occupied slots)
    gk, gv = buf[:n, 0], buf[:n, 1]
    assert (buf[n:] == np.uint64(SENT)).all()
    assert len(np.unique(gk)) == n
    pos = np.searchsorted(ek, gk)
    assert (pos < len(ek)).all() and np.array_equal(ek[np.minimum(pos, len(ek) - 1)], gk)   # a subset of the input ...
    assert np.array_equal(ev[pos], gv)                                                      # ... each with its smallest value
    m.clear()
    assert m.count() == 0                                 # empty, and the error is gone
    rc, n, buf = _raw_export(m, 16)
    assert rc == 0 and n == 0 and (buf == np.uint64(SENT)).all()
    keys = mr.random_keys(rng, 400)
    k, v = _records(rng, keys)
    ek, ev = mr.reduce_records(k, v)
    m.merge(mr.to_device(k, v))
    assert m.count() == 400
    gk, gv = mr.sorted_records(m)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    m.close()


def test_export_into_a_buffer_that_is_too_small(scvod):
    rng = np.random.default_rng(13)
    keys = mr.random_keys(rng, 3000)
    vals = mr.random_keys(rng, 3000)
    m = scvod.StaticMap(8192)
    m.merge(mr.to_device(keys, vals))
    n = m.count()
    assert n == 3000
    ek, ev = mr.reduce_records(keys, vals)
    cap = n - 5
    rc, n_out, buf = _raw_export(m, n + 64, cap=cap)
    assert rc == ERR_CAPACITY
    assert n_out == n                                     # the true count, so the caller can size the next buffer
    assert (buf[cap:] == np.uint64(SENT)).all()           # nothing at or behind cap
    gk, gv = buf[:cap, 0], buf[:cap, 1]
    assert len(np.unique(gk)) == cap and np.isin(gk, ek).all()
    assert np.array_equal(ev[np.searchsorted(ek, gk)], gv)
    # the map itself is intact, and the error belonged to that call alone
    gk, gv = mr.sorted_records(m)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    rc, n_out, buf = _raw_export(m, n + 64, cap=n)
    assert rc == 0 and n_out == n and (buf[n:] == np.uint64(SENT)).all()
    m.close()


@pytest.mark.parametrize("n_parts", [1, 3, 64])
def test_parts_partition_the_map(scvod, n_parts):
    import torch
    rng = np.random.default_rng(14 + n_parts)
    n = 3000
    keys, vals = mr.random_keys(rng, n), mr.random_keys(rng, n)
    ek, ev = mr.reduce_records(keys, vals)
    m = scvod.StaticMap(8192)
    m.merge(mr.to_device(keys, vals))
    g, counts = m.export_parts(n_parts)
    g = g.cpu().numpy().view(np.uint64)
    assert len(counts) == n_parts and sum(counts) == n and g.shape[0] == n
    o = np.argsort(g[:, 0])
    assert np.array_equal(g[o, 0], ek) and np.array_equal(g[o, 1], ev)          # the groups partition the records
    off = np.concatenate([[0], np.cumsum(counts)])
    owner = dict(zip(g[:, 0].tolist(), np.repeat(np.arange(n_parts), counts).tolist()))
    if n_parts > 1:
        assert min(counts) > 0 and max(counts) < 3 * n // n_parts               # an owner hash, not a constant
    # the padded form: same keys in the same groups, counts on the device, padding behind every group, guards untouched
    cap, guard = max(counts) + 3, 16
    flat = torch.full((n_parts * cap + 2 * guard, 2), SENT, dtype=torch.int64, device="cuda")
    d_counts = torch.full((n_parts,), -7, dtype=torch.int64, device="cuda")
    m.export_parts_padded(n_parts, flat[guard:guard + n_parts * cap].view(n_parts, cap, 2), d_counts)
    assert m.count() == n                                                        # (synchronises; nothing overflowed)
    h = flat.cpu().numpy().view(np.uint64)
    assert (h[:guard] == np.uint64(SENT)).all() and (h[guard + n_parts * cap:] == np.uint64(SENT)).all()
    slots = h[guard:guard + n_parts * cap].reshape(n_parts, cap, 2)
    assert d_counts.cpu().tolist() == counts
    for p in range(n_parts):
        a, b = slots[p, :counts[p]], g[off[p]:off[p + 1]]
        assert (slots[p, counts[p]:] == mr.PAD).all()
        oa, ob = np.argsort(a[:, 0]), np.argsort(b[:, 0])
        assert np.array_equal(a[oa], b[ob])
    # merging the groups (padding included) into n_parts fresh maps reproduces the whole
    allk, allv = [], []
    for p in range(n_parts):
        q = scvod.StaticMap(max(1024, 2 * counts[p]))
        q.merge(flat[guard + p * cap:guard + (p + 1) * cap])
        assert q.count() == counts[p]
        k, v = mr.sorted_records(q)
        allk.append(k[:counts[p]])
        allv.append(v[:counts[p]])
        q.close()
    allk, allv = np.concatenate(allk), np.concatenate(allv)
    o = np.argsort(allk)
    assert np.array_equal(allk[o], ek) and np.array_equal(allv[o], ev)
    # a slot one below the largest group: reported by the next count(), true sizes in d_counts, nothing outside a group's slot
    cap = max(counts) - 1
    flat.fill_(SENT)
    d_counts.fill_(-7)
    m.export_parts_padded(n_parts, flat[guard:guard + n_parts * cap].view(n_parts, cap, 2), d_counts)
    with pytest.raises(scvod.ScvodError) as e:
        m.count()
    assert _status(e) == ERR_CAPACITY
    assert d_counts.cpu().tolist() == counts
    h = flat.cpu().numpy().view(np.uint64)
    assert (h[:guard] == np.uint64(SENT)).all() and (h[guard + n_parts * cap:] == np.uint64(SENT)).all()
    slots = h[guard:guard + n_parts * cap].reshape(n_parts, cap, 2)
    for p in range(n_parts):
        fill = min(counts[p], cap)
        a = slots[p, :fill]
        assert (slots[p, fill:] == mr.PAD).all()
        assert len(np.unique(a[:, 0])) == fill and all(owner.get(kk, -1) == p for kk in a[:, 0].tolist())
        assert np.array_equal(ev[np.searchsorted(ek, a[:, 0])], a[:, 1])
    m.close()


@pytest.mark.parametrize("leaf", [0.2, 0.25])
def test_points_decode_every_axis(scvod, leaf):
    rng = np.random.default_rng(15)
    edge = np.array([-(1 << 20), -1, 0, (1 << 20) - 1, 1000, -777], np.int64)
    offs = np.array([0, 65535, 1, 32768, 12345, 54321, 65534], np.int64)
    ix, iy, iz = [a.ravel() for a in np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij")]
    cx, cy, cz = edge[ix], edge[iy], edge[iz]
    n0 = len(cx)
    # an axis' offset is picked by the cells of the other two (u + 2 v mod 7 takes every value for u, v in 0..5): every cell of an
    # axis meets every offset on that axis, and the three axes never run in step
    qx, qy, qz = offs[(iy + 2 * iz) % 7], offs[(iz + 2 * ix + 1) % 7], offs[(ix + 2 * iy + 3) % 7]
    qi = rng.integers(0, 65536, n0)
    qi[:4] = [0, 65535, 1, 256]
    n1 = 2000
    rc = rng.integers(-(1 << 20), 1 << 20, (3, n1))
    rq = rng.integers(0, 65536, (4, n1))
    keys = np.concatenate([mr.pack_key(cx, cy, cz), mr.pack_key(rc[0], rc[1], rc[2])])
    vals = np.concatenate([mr.pack_val(qx, qy, qz, qi), mr.pack_val(rq[0], rq[1], rq[2], rq[3])])
    keys, first = np.unique(keys, return_index=True)
    vals = vals[first]
    assert len(keys) >= n0 and (keys != mr.PAD).all()
    # the offsets 0 and 65535 meet all four edge cells, on every axis, and the axes differ
    c, q = mr.unpack_key(keys), mr.unpack_val(vals)
    for ax in range(3):
        for cell in edge[:4]:
            assert ((c[ax] == cell) & (q[ax] == 0)).any() and ((c[ax] == cell) & (q[ax] == 65535)).any()
    assert (q[1] != q[2]).sum() > len(keys) // 2 and (q[0] != q[1]).sum() > len(keys) // 2
    m = scvod.StaticMap(8192, leaf=leaf)
    m.merge(mr.to_device(keys, vals))
    xyzi, rec = m.points()
    xyzi, rec = xyzi.cpu().numpy(), rec.cpu().numpy().view(np.uint64)
    assert xyzi.shape == (len(keys), 4) and rec.shape == (len(keys), 2)
    o = np.argsort(rec[:, 0])
    assert np.array_equal(rec[o, 0], keys) and np.array_equal(rec[o, 1], vals)
    # row i of xyzi is record i
    want, want_i = mr.decode_points(rec[:, 0], rec[:, 1], leaf)
    got = xyzi[:, :3]
    ulp = np.spacing(np.abs(got)).astype(np.float64)
    for ax in range(3):
        assert (np.abs(got[:, ax].astype(np.float64) - want[:, ax]) <= 2 * ulp[:, ax]).all(), f"axis {ax}"
    assert np.array_equal(xyzi[:, 3].astype(np.float64), want_i)
    m.close()


# ---------------------------------------------------------------- part 2: accumulation with controlled geometry

SIZES = [255, 256, 257, 8191, 8192, 8193, 8192 + 65]     # wave tails, the kMapPts stride, a run cut by the end of a scan


def _scan(rng, n, sensor_height=1.73):
    """n points in INPUT ORDER made of runs that share one 0.2 m cell under the identity pose: single points, short runs, whole waves
    (64, 65, 130), stretches that alternate between two cells, box columns (one x/y cell, z spread), points Patchwork drops for sure
    (inside its 2.7 m gate) in the middle of runs; the last 40 points are one run that ends with the scan.  Flat ground ring from 3 m
    to 12 / 25 m over an arc that grows with n, so that patches exceed num_min_pts."""
    arc = min(2 * np.pi, n / 255.0 * (np.pi / 8))
    rmax = 12.0 if n < 3000 else 25.0

    def anchor(dropped=False):
        r = rng.uniform(0.3, 2.4) if dropped else np.sqrt(rng.uniform(3.2 ** 2, rmax ** 2))
        a = rng.uniform(0, arc)
        return (np.floor(r * np.cos(a) / 0.2) + 0.5) * 0.2, (np.floor(r * np.sin(a) / 0.2) + 0.5) * 0.2

    xs, ys, zs = [], [], []
    left = n - 40
    forced = [10, 0, 1, 4]                                 # every scan holds a dropped run, an alternating stretch and a box column
    while left > 0:
        L = min(int(rng.choice([1, 1, 1, 2, 3, 7, 31, 64, 65, 130])), left)
        kind = forced.pop(0) if forced else rng.integers(0, 20)
        a0, a1 = anchor(dropped=kind == 0), anchor()
        pick = (np.arange(L) % 2 == 1) if kind in (1, 2, 3) else np.zeros(L, bool)      # alternating cells
        xs.append(np.where(pick, a1[0], a0[0]))
        ys.append(np.where(pick, a1[1], a0[1]))
        zs.append(rng.uniform(-sensor_height, 0.5, L) if kind in (4, 5, 6) else np.full(L, -sensor_height))   # a box column
        left -= L
    a0 = anchor()
    xs.append(np.full(40, a0[0]))
    ys.append(np.full(40, a0[1]))
    zs.append(np.full(40, -sensor_height))
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = np.concatenate(xs) + rng.uniform(-0.08, 0.08, n)
    p[:, 1] = np.concatenate(ys) + rng.uniform(-0.08, 0.08, n)
    p[:, 2] = np.concatenate(zs) + rng.uniform(-0.02, 0.02, n)
    p[:, 3] = rng.uniform(0.0, 255.0, n)
    return p


def _oracle_kept(oracle, P, scan):
    r = oracle.patchwork(P, scan)
    keep = np.zeros(len(scan), bool)
    keep[r["ground_idx"]] = True
    keep[r["nonground_idx"]] = True
    return keep


class _Batch:
    """scans through batch_process once; the kept set from the oracle's Patchwork"""

    def __init__(self, scvod, oracle, scans):
        import torch
        self.scvod = scvod
        self.P = scvod.make_params("semantickitti")
        self.x = np.concatenate(scans)
        self.offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
        self.n_scans = len(scans)
        self.kept = [_oracle_kept(oracle, self.P, s) for s in scans]
        self.ctx = scvod.Ctx(self.P, max_points_total=int(self.offs[-1]) + 64, max_scans=self.n_scans)
        self.d = torch.from_numpy(self.x).cuda()
        self.ctx.batch_process(self.d, self.offs)

    def points(self, s):
        return self.x[self.offs[s]:self.offs[s + 1]][self.kept[s]]

    def definition(self, poses, leaf, scans=None):
        """(keys, values, points out of range) of the scans under the fp32 definition"""
        ks, vs, out = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint64)], 0
        for s in (range(self.n_scans) if scans is None else scans):
            k, v, ok = mr.encode_points(self.scvod.pose_matrix(poses[s]), self.points(s), leaf)
            ks.append(k[ok])
            vs.append(v[ok])
            out += int((~ok).sum())
        k, v = mr.reduce_records(np.concatenate(ks), np.concatenate(vs))
        return k, v, out

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def sized(scvod, oracle):
    rng = np.random.default_rng(2024)
    b = _Batch(scvod, oracle, [_scan(rng, n) for n in SIZES])
    assert int(b.offs[-1]) <= 40000
    yield b
    b.close()


def _moving_poses(n):
    return np.asarray([[0.7 * s, 0.1 * s, 0.01 * s, 0.002 * s, -0.003 * s, 0.01 * s] for s in range(n)], np.float32)


def _accumulated(scvod, b, poses, leaf, capacity=1 << 17):
    m = scvod.StaticMap(capacity, leaf=leaf)
    m.accumulate(b.ctx, poses, flags=scvod.MAP_IGNORE_DYNAMIC)
    return m


def test_the_scans_hold_the_runs_they_are_meant_to(scvod, sized):
    """the geometry the cases below rely on, stated on the definition's own keys (identity pose, leaf 0.2)"""
    ident = np.zeros((sized.n_scans, 6), np.float32)
    for s in range(sized.n_scans):
        n = SIZES[s]
        k, _, ok = mr.encode_points(scvod.pose_matrix(ident[s]), sized.x[sized.offs[s]:sized.offs[s + 1]], 0.2)
        assert ok.all()
        keep = sized.kept[s]
        assert 0 < (~keep).sum() < n // 2                                  # Patchwork dropped some, kept most
        k = np.where(keep, k, mr.PAD)                                      # what a lane holds
        assert keep[-40:].all() and (k[-40:] == k[-1]).all()               # a run cut by the end of the scan
        change = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1], [True]]))
        runs = np.diff(change)
        assert runs.max() >= 40
        if n > 8000:
            assert runs.max() >= 130 and (runs == 1).sum() >= 64           # whole waves in one cell, and single points
            alt = (k[2:] == k[:-2]) & (k[1:-1] != k[2:]) & (k[2:] != mr.PAD) & (k[1:-1] != mr.PAD)
            assert alt.sum() >= 64                                         # alternating cells


@pytest.mark.parametrize("leaf", [50.0, 0.2, 0.01])
def test_leaf_drives_the_contention(scvod, sized, leaf):
    """leaf 50: whole waves in one cell, thousands of atomicMin on one record; leaf 0.01: runs of length 1"""
    poses = _moving_poses(sized.n_scans)
    ek, ev, out = sized.definition(poses, leaf)
    assert out == 0
    n_kept = sum(int(k.sum()) for k in sized.kept)
    if leaf == 50.0:
        assert len(ek) <= 8
    if leaf == 0.01:
        assert len(ek) > n_kept // 2
    m = _accumulated(scvod, sized, poses, leaf)
    assert m.count() == len(ek)
    gk, gv = mr.sorted_records(m)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    m.accumulate(sized.ctx, poses, flags=scvod.MAP_IGNORE_DYNAMIC)     # every record is there already: the test-before-atomic path
    gk, gv = mr.sorted_records(m)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    m.close()


def test_every_scan_size_on_its_own(scvod, sized):
    ident = np.zeros((sized.n_scans, 6), np.float32)
    m = scvod.StaticMap(1 << 15, leaf=0.2)
    for s in range(sized.n_scans):
        m.clear()
        m.accumulate_range(sized.ctx, ident, s, 1, flags=scvod.MAP_IGNORE_DYNAMIC)
        ek, ev, out = sized.definition(ident, 0.2, scans=[s])
        assert out == 0 and len(ek) > 0
        gk, gv = mr.sorted_records(m)
        assert np.array_equal(gk, ek) and np.array_equal(gv, ev), f"scan of {SIZES[s]} points"
    m.close()


def test_order_of_accumulation_and_rotated_poses(scvod, sized):
    h = np.float32(np.pi / 2)
    poses = np.asarray([[3.0 * s, -2.0 * s, 0.5 * s, 0.0, 0.1 * (s % 2), h * (s % 3 - 1)] for s in range(sized.n_scans)], np.float32)
    poses[0, 3:] = [0.0, 0.1, h]                                          # yaw pi/2 and pitch 0.1 together
    ek, ev, out = sized.definition(poses, 0.2)
    assert out == 0
    one = _accumulated(scvod, sized, poses, 0.2)
    gk, gv = mr.sorted_records(one)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    rev = scvod.StaticMap(1 << 17, leaf=0.2)
    for _ in range(2):
        for s in reversed(range(sized.n_scans)):
            rev.accumulate_range(sized.ctx, poses, s, 1, flags=scvod.MAP_IGNORE_DYNAMIC)
    rk, rv = mr.sorted_records(rev)
    assert np.array_equal(rk, ek) and np.array_equal(rv, ev)
    one.close()
    rev.close()


def test_far_and_out_of_range_poses(scvod, sized):
    n = sized.n_scans
    # cells near -2**20 on every axis (leaf 0.2: -2.0e5 m is cell -1.0e6 > -1 048 576)
    far = np.asarray([[-2.0e5 - 3 * s, -2.0e5 + 2 * s, -2.0e5, 0.0, 0.02, 0.3 * s] for s in range(n)], np.float32)
    ek, ev, out = sized.definition(far, 0.2)
    assert out == 0 and mr.unpack_key(ek)[0].max() < -990000
    m = _accumulated(scvod, sized, far, 0.2)
    assert m.count() == len(ek)
    gk, gv = mr.sorted_records(m)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    # every point out of range: reported, and no record at all (nothing aliased into a valid key)
    m.clear()
    gone = np.asarray([[3.0e5, 0, 0, 0, 0, 0.1 * s] for s in range(n)], np.float32)
    ek, ev, out = sized.definition(gone, 0.2)
    n_kept = sum(int(k.sum()) for k in sized.kept)
    assert len(ek) == 0 and out == n_kept
    m.accumulate(sized.ctx, gone, flags=scvod.MAP_IGNORE_DYNAMIC)
    with pytest.raises(scvod.ScvodError) as e:
        m.count()
    assert _status(e) == ERR_CAPACITY
    assert int(re.search(r"(\d+) points did not fit", str(e.value)).group(1)) == n_kept
    rc, cnt, buf = _raw_export(m, 64)
    assert rc == ERR_CAPACITY and cnt == 0 and (buf == np.uint64(SENT)).all()
    # mixed: scans out of range on either side of any axis between scans in range
    m.clear()
    mixed = _moving_poses(n)
    mixed[1, 0] = 3.0e5
    mixed[3, 1] = -3.0e5
    mixed[4, 2] = 3.0e5
    mixed[6, :3] = [-3.0e5, 3.0e5, -3.0e5]
    inside = [0, 2, 5]
    ek, ev, out = sized.definition(mixed, 0.2)
    ik, iv, _ = sized.definition(mixed, 0.2, scans=inside)
    assert np.array_equal(ek, ik) and out == sum(int(sized.kept[s].sum()) for s in (1, 3, 4, 6))
    m.accumulate(sized.ctx, mixed, flags=scvod.MAP_IGNORE_DYNAMIC)
    rc, cnt, buf = _raw_export(m, len(ek) + 64)
    assert rc == ERR_CAPACITY and cnt == len(ek)
    o = np.argsort(buf[:cnt, 0])
    assert np.array_equal(buf[:cnt][o, 0], ek) and np.array_equal(buf[:cnt][o, 1], ev)
    assert (buf[cnt:] == np.uint64(SENT)).all()
    assert int(re.search(r"(\d+) points did not fit", m.lib.scvod_map_last_error(m.h).decode()).group(1)) == out
    m.close()


def test_points_on_cell_faces(scvod, oracle):
    """identity rotation, leaf 0.25, every coordinate and every translation an exact multiple of 0.25 (both signs, -0.0 too): the world
    coordinate is exact in fp32, so the offset is 0 and the cell is the one floor gives"""
    g = np.arange(-100, 101, 2) * 0.25
    X, Y = np.meshgrid(g, g, indexing="ij")
    r = np.hypot(X, Y)
    ring = (r > 3.0) & (r < 24.0)
    x, y = X[ring], Y[ring]
    x = np.where(x == 0.0, -0.0, x)                                        # x = -0.0 down the y axis
    scans, rng = [], np.random.default_rng(5)
    for z_levels in ([-1.75], [-1.75, -1.5, -0.0, 0.25], [-1.75, 0.0]):
        z = rng.choice(z_levels, len(x))
        scans.append(np.stack([x, y, z, rng.uniform(0, 255, len(x))], axis=1).astype(np.float32))
    assert np.signbit(scans[0][:, 0]).any() and (scans[0][:, 0] == 0).any()
    b = _Batch(scvod, oracle, scans)
    poses = np.zeros((3, 6), np.float32)
    poses[0, :3] = [-0.0, -0.0, -0.0]
    poses[1, :3] = [12.25, -7.5, 0.25]
    poses[2, :3] = [-100.75, 3.0, -0.5]
    leaf = 0.25
    ks = []
    for s in range(3):
        p = b.points(s).astype(np.float64)
        assert len(p) > 1000
        c = [np.rint((p[:, i] + np.float64(poses[s, i])) * 4.0).astype(np.int64) for i in range(3)]     # exact: the cell floor gives
        ks.append(mr.pack_key(*c))
    want = np.unique(np.concatenate(ks))
    ek, ev, out = b.definition(poses, leaf)
    assert out == 0 and np.array_equal(ek, want)
    assert all((q == 0).all() for q in mr.unpack_val(ev)[:3])
    m = _accumulated(scvod, b, poses, leaf)
    gk, gv = mr.sorted_records(m)
    assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
    xyzi, rec = m.points()
    xyzi, rec = xyzi.cpu().numpy().astype(np.float64), rec.cpu().numpy().view(np.uint64)
    c = mr.unpack_key(rec[:, 0])
    for ax in range(3):
        assert ((xyzi[:, ax] >= c[ax] * leaf) & (xyzi[:, ax] < (c[ax] + 1) * leaf)).all()
    assert min(cc.min() for cc in c) < 0 < max(cc.max() for cc in c)
    m.close()
    b.close()


def test_intensity_is_clamped(scvod, oracle):
    """map_encode clamps intensity * 256 to [0, 65535] and truncates: -5 -> 0, 0 -> 0, 255.99 -> 65533, 300 and 1e9 -> 65535.
    NaN intensity is out of scope: the conversion is undefined and include/scvod.h says so."""
    rng = np.random.default_rng(6)
    special = np.array([-5.0, 0.0, 255.99, 300.0, 1e9, 17.5], np.float32)
    stored = {-5.0: 0, 0.0: 0, 255.99: 65533, 300.0: 65535, 1e9: 65535, 17.5: 4480}
    scans = []
    for n in (1500, 2100):
        p = _scan(rng, n)
        p[:, 3] = special[np.arange(n) % len(special)]
        scans.append(p)
    b = _Batch(scvod, oracle, scans)
    poses = _moving_poses(2)
    leaf = 0.01
    ek, ev, out = b.definition(poses, leaf)
    m = _accumulated(scvod, b, poses, leaf)
    gk, gv = mr.sorted_records(m)
    assert out == 0 and np.array_equal(gk, ek) and np.array_equal(gv, ev)
    # cells that hold one point: the stored intensity is that point's, clamped as stated (not through the definition's own clip)
    seen = set()
    for s in range(2):
        p = b.points(s)
        k, _, _ = mr.encode_points(scvod.pose_matrix(poses[s]), p, leaf)
        uk, idx, cnt = np.unique(k, return_index=True, return_counts=True)
        other = b.definition(poses, leaf, scans=[1 - s])[0]
        alone = (cnt == 1) & ~np.isin(uk, other)
        got = mr.unpack_val(gv[np.searchsorted(gk, uk[alone])])[3]
        for inten, q in zip(p[idx[alone], 3].tolist(), got.tolist()):
            key = min(stored, key=lambda t: abs(t - inten))
            assert q == stored[key], (inten, q)
            seen.add(key)
    assert seen == set(stored)
    xyzi, _ = m.points()
    inten = xyzi[:, 3].cpu().numpy()
    assert inten.min() == 0.0 and inten.max() == np.float32(65535 / 256.0)
    m.close()
    b.close()


def test_points_against_fp64_transform_of_the_input(scvod, sized):
    """closes the loop with tests/test_pose_matrix.py: every point points() returns lies, per axis, within
    leaf / 65536 + 8 * 2**-24 * (|x| + |y| + |z| + |t|_max) of an oracle-kept input point (x, y, z) moved in fp64 by the
    elementary-rotation matrix, and carries that point's intensity to within 1/256"""
    leaf = 0.2
    scans = [0, 1, 2, 3]
    poses = np.zeros((sized.n_scans, 6), np.float32)
    for s in scans:
        poses[s] = [812.5 + 1.5 * s, -903.25 + 0.4 * s, 41.0 - 0.1 * s, 0.03, -0.08 + 0.01 * s, 2.1 + 0.05 * s]
    m = scvod.StaticMap(1 << 15, leaf=leaf)
    m.accumulate_range(sized.ctx, poses, 0, len(scans), flags=scvod.MAP_IGNORE_DYNAMIC)
    xyzi, _ = m.points()
    got = xyzi.cpu().numpy().astype(np.float64)
    assert 500 < len(got) < 9000
    W, I, tol = [], [], []
    for s in scans:
        p = sized.points(s).astype(np.float64)
        M = mr.pose64(poses[s])
        W.append(p[:, :3] @ M[:3, :3].T + M[:3, 3])
        I.append(p[:, 3])
        tol.append(leaf / 65536 + 8 * 2.0 ** -24 * (np.abs(p[:, :3]).sum(axis=1) + np.abs(M[:3, 3]).max()))
    W, I, tol = np.concatenate(W), np.concatenate(I), np.concatenate(tol)
    worst = 0.0
    for a in range(0, len(got), 256):
        d = np.abs(got[a:a + 256, None, :3] - W[None, :, :]).max(axis=2)           # [chunk, inputs], the largest axis distance
        j = np.argmin(d, axis=1)
        dj = d[np.arange(len(j)), j]
        worst = max(worst, float((dj / tol[j]).max()))
        assert (dj <= tol[j]).all()
        di = I[j] - got[a:a + 256, 3]
        assert ((di >= 0) & (di <= 1.0 / 256)).all()                               # truncated to 1/256, never above
    print(f"worst distance / bound {worst:.3f}")
    m.close()
