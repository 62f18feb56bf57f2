"""The labelled static map (SCVOD_MAP_KIND_LABELLED) on the device: k_map_accumulate_labelled through the ctx-free call on crafted
clouds, scvod_map_points_labelled, the kind errors, and the batch form scvod_batch_map_accumulate_classes on batch "R3" of
tests/test_gpu_class_score.py with the region growing on.

The yardstick is tests/helpers/class_map_ref.py on top of tests/helpers/map_ref.py: `encode_points` gives key and plain value, the
labelled value is (val & ~0xFFFF) | label << 8 | qi8, `reduce_records` is the definition of the map.  Device records, sorted by key,
must equal it bit for bit: every comparison is np.array_equal."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import class_map_ref as cmr  # noqa: E402
import class_score_ref as csr  # noqa: E402
import map_ref as mr  # noqa: E402
from test_gpu_async_chain import _new_ctx, _track  # noqa: E402
from test_gpu_class_score import _assert_result, _classes, _cuda, _r3_with  # noqa: E402

pytestmark = pytest.mark.gpu

LEAF = 0.5
ERR_INVALID, ERR_CAPACITY, ERR_STATE = -1, -4, -5
SENT = 0x5555555555555555
SIZES = [1, 63, 64, 65, 0, 255, 257, 8191, 8193]      # wave tails, the 256-thread round, the 8192-point tile; the empty scan in the middle
DROP = 250                                            # the label the keep tables of the run cases leave out
U16 = np.uint64(16)


def _status(excinfo):
    m = re.match(r"status (-?\d+)", str(excinfo.value))
    assert m, str(excinfo.value)
    return int(m.group(1))


def _lmap(scvod, cells=1 << 16, leaf=LEAF):
    m = scvod.StaticMap(cells, leaf=leaf, kind=scvod.MAP_KIND_LABELLED)
    assert m.lib.scvod_map_kind(m.h) == 1
    return m


def _dev(x, lab):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(lab, np.uint8)).cuda()


def _same(m, ek, ev, what=""):
    gk, gv = mr.sorted_records(m)
    assert np.array_equal(gk, ek), f"{what}: {len(gk)} cells, expected {len(ek)}"
    bad = np.flatnonzero(gv != ev)
    assert len(bad) == 0, f"{what}: {len(bad)} values differ, first {[hex(int(v)) for v in (gv[bad[0]], ev[bad[0]])]}"


class _Sized:
    def __init__(self):
        rng = np.random.default_rng(20261018)
        n = sum(SIZES)
        self.x = np.concatenate([rng.uniform(-3.0, 3.0, (n, 3)), rng.uniform(-5.0, 300.0, (n, 1))], axis=1).astype(np.float32)
        self.lab = rng.integers(0, 256, n).astype(np.uint8)
        self.offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
        self.n_scans = len(SIZES)
        self.poses = np.asarray([[0.3 * s, -0.2 * s, 0.05 * s, 0.01 * s, -0.02 * s, 0.4 * s] for s in range(self.n_scans)], np.float32)
        self.d_x, self.d_lab = _dev(self.x, self.lab)


@pytest.fixture(scope="module")
def sized():
    return _Sized()


# ---------------------------------------------------------------- part 1: crafted clouds through the ctx-free call

def test_scan_sizes_in_one_call_and_one_scan_per_call(scvod, sized):
    ek, ev, out = cmr.definition(scvod, sized.x, sized.lab, sized.offs, sized.poses, LEAF)
    assert out == 0 and 500 < len(ek) < sum(SIZES) // 2, "the cells are meant to collide"
    assert len(np.unique(cmr.unpack_labelled(ev)[3])) > 100 and (cmr.unpack_labelled(ev)[4] == 255).any() and (cmr.unpack_labelled(ev)[4] == 0).any()
    m = _lmap(scvod)
    m.accumulate_labelled(sized.d_x, sized.d_lab, sized.offs, sized.poses)
    assert m.count() == len(ek)
    _same(m, ek, ev, "one call")
    m.accumulate_labelled(sized.d_x, sized.d_lab, sized.offs, sized.poses)      # every record is there already
    _same(m, ek, ev, "the same call again")
    m.clear()
    for s in range(sized.n_scans):                                             # offsets that start anywhere, one pose
        m.accumulate_labelled(sized.d_x, sized.d_lab, sized.offs[s:s + 2], sized.poses[s:s + 1])
    _same(m, ek, ev, "one scan per call")
    for s in (3, 8):
        m.clear()
        m.accumulate_labelled(sized.d_x, sized.d_lab, sized.offs[s:s + 2], sized.poses[s:s + 1])
        k1, v1, _ = cmr.definition(scvod, sized.x, sized.lab, sized.offs, sized.poses, LEAF, scans=[s])
        _same(m, k1, v1, f"scan of {SIZES[s]} points alone")
    # no poses = the zero pose through the same expression
    ik, iv, _ = cmr.definition(scvod, sized.x, sized.lab, sized.offs, None, LEAF)
    for poses in (None, np.zeros((sized.n_scans, 6), np.float32)):
        m.clear()
        m.accumulate_labelled(sized.d_x, sized.d_lab, sized.offs, poses)
        _same(m, ik, iv, "identity")
    m.close()


# (first point, length, positions inside the run whose label is DROP, cell index along x); the cells of the runs lie on the line
# y, z in [0, 0.5); every other point lies at y >= 1 in a cell of its own choosing
RUNS = [(60, 8, [0], 0),                    # straddles lanes 63 | 64, its first point removed
        (120, 130, [64], 1),                # longer than a wave, a middle point removed
        (250, 12, [11], 2),                 # straddles threads 255 | 256, its last point removed
        (300, 2, [0, 1], 3),                # removed entirely: no cell
        (400, 70, [], 4),
        (500, 5, [2], 4),                   # the cell of the run before, from another wave
        (8185, 20, [0, 7], 5),              # straddles the 8192-point tile: two workgroups
        (8300, 64, list(range(64)), 6),     # a whole aligned-sized run removed
        (8400, 3, [1], 7),                  # a removed middle point splits the run in two
        (8489, 11, [10], 8)]                # ends with the scan, its last point removed


def _run_scan():
    rng = np.random.default_rng(77)
    n = 8500
    x = np.zeros((n, 4), np.float32)
    x[:, 0] = rng.uniform(-3.0, 3.0, n)
    x[:, 1] = rng.uniform(1.0, 4.0, n)
    x[:, 2] = rng.uniform(-1.0, 1.0, n)
    x[:, 3] = rng.uniform(-5.0, 300.0, n)
    lab = rng.integers(0, 200, n).astype(np.uint8)
    for first, length, gone, cell in RUNS:
        sl = slice(first, first + length)
        x[sl, 0] = cell * 0.5 + rng.uniform(0.01, 0.49, length)
        x[sl, 1] = rng.uniform(0.01, 0.49, length)
        x[sl, 2] = rng.uniform(0.01, 0.49, length)
        lab[sl] = rng.integers(0, 200, length)
        at = first + np.asarray(gone, np.int64)
        lab[at] = DROP
        x[at, 0] = cell * 0.5 + rng.uniform(0.001, 0.009, len(at))     # the removed points would win their cells: the smallest offsets
    return x, lab


def test_runs_of_one_cell_and_the_keep_table(scvod):
    x, lab = _run_scan()
    offs = np.array([0, len(x)], np.int32)
    keep = cmr.table256(range(200))
    assert keep[DROP] == 0
    k, v, ok, bad = cmr.encode_scan(scvod.pose_matrix(np.zeros(6, np.float32)), x, lab, LEAF, keep)
    assert not bad.any()
    for first, length, gone, cell in RUNS:     # the layout is what the comment says
        assert 2 <= length <= 130 and len(set(k[first:first + length].tolist())) == 1
        assert mr.unpack_key(k[first:first + 1])[0][0] == cell and k[first - 1] != k[first]
        assert len(set(cmr.qi8(x[first:first + length, 3]).tolist())) > 1
        assert len(set(lab[first:first + length].tolist())) > 1 or len(gone) == length
        assert (lab[first:first + length] == DROP).sum() == len(gone)
    ek, ev = mr.reduce_records(k[ok], v[ok])
    gone_cells = {int(k[300]), int(k[8300])}
    assert not gone_cells & set(ek.tolist()), "a run that is removed entirely leaves no cell"
    assert not (cmr.unpack_labelled(ev)[3] == DROP).any()
    d_x, d_lab = _dev(x, lab)
    m = _lmap(scvod)
    m.accumulate_labelled(d_x, d_lab, offs, keep=keep)
    _same(m, ek, ev, "runs")
    assert not np.isin(mr.sorted_records(m)[0], list(gone_cells)).any()
    # the removed points did matter: without the table some cell's representative is one of them
    m.clear()
    m.accumulate_labelled(d_x, d_lab, offs)
    ak, av = mr.reduce_records(k, v)
    _same(m, ak, av, "runs, every label kept")
    assert len(ak) == len(ek) + 2 and (cmr.unpack_labelled(av)[3] == DROP).sum() == 9 and (av[np.isin(ak, ek)] != ev).sum() == 7
    m.close()


@pytest.mark.parametrize("together", [True, False])
def test_tie_order(scvod, together):
    """equal offset: the smallest label wins; equal offset and label: the smallest intensity; a smaller label on a larger offset
    loses -- in both input orders, with the rivals side by side in one wave (the run reduction) or in two calls (the atomicMin)"""
    a = [0.25, 0.25, 0.25]
    pts = np.array([a + [10.0], a + [10.0],                               # cell (0, 0, 0): labels 9 and 4
                    [0.75, 0.25, 0.25, 50.0], [0.75, 0.25, 0.25, 20.0],   # cell (1, 0, 0): label 3 twice
                    [1.375, 0.25, 0.25, 0.0], [1.25, 0.25, 0.25, 99.0]],  # cell (2, 0, 0): label 1 at offset 0.75, label 200 at 0.5
                   np.float32)
    lab = np.array([9, 4, 3, 3, 1, 200], np.uint8)
    want = {0: (4, 10), 1: (3, 20), 2: (200, 99)}
    for order in ([0, 1, 2, 3, 4, 5], [1, 0, 3, 2, 5, 4]):
        x, ls = pts[order], lab[order]
        d_x, d_lab = _dev(x, ls)
        m = _lmap(scvod, 1024)
        if together:
            m.accumulate_labelled(d_x, d_lab, np.array([0, 6], np.int32))
        else:
            for i in range(6):
                m.accumulate_labelled(d_x, d_lab, np.array([i, i + 1], np.int32))
        gk, gv = mr.sorted_records(m)
        cx = mr.unpack_key(gk)[0].tolist()
        q = cmr.unpack_labelled(gv)
        assert cx == [0, 1, 2]
        assert {c: (int(q[3][i]), int(q[4][i])) for i, c in enumerate(cx)} == want
        assert q[0].tolist() == [32768, 32768, 32768]
        ek, ev, _ = cmr.definition(scvod, x, ls, np.array([0, 6], np.int32), None, LEAF)
        assert np.array_equal(gk, ek) and np.array_equal(gv, ev)
        m.close()


def test_intensity_packing(scvod):
    inten = np.array([-1.0, 0.99, 254.5, 255.0, 1e9], np.float32)
    x = np.stack([0.5 * np.arange(5) + 0.25, np.full(5, 0.25), np.full(5, 0.25), inten], axis=1).astype(np.float32)
    lab = np.array([0, 255, 7, 128, 64], np.uint8)
    d_x, d_lab = _dev(x, lab)
    m = _lmap(scvod, 1024)
    m.accumulate_labelled(d_x, d_lab, np.array([0, 5], np.int32))
    gk, gv = mr.sorted_records(m)
    q = cmr.unpack_labelled(gv)
    assert mr.unpack_key(gk)[0].tolist() == [0, 1, 2, 3, 4]
    assert q[4].tolist() == [0, 0, 254, 255, 255] and q[3].tolist() == [0, 255, 7, 128, 64]
    xyzi, pl, rec = m.points_labelled()
    o = np.argsort(rec.cpu().numpy().view(np.uint64)[:, 0])
    assert xyzi.cpu().numpy()[o, 3].tolist() == [0.0, 0.0, 254.0, 255.0, 255.0] and pl.cpu().numpy()[o].tolist() == [0, 255, 7, 128, 64]
    pxyzi, _ = m.points()                                                 # scvod_map_points on a labelled map: the low 8 bits
    assert sorted(pxyzi.cpu().numpy()[:, 3].tolist()) == [0.0, 0.0, 254.0, 255.0, 255.0]
    m.close()


def test_order_and_merge(scvod, sized):
    ek, ev, _ = cmr.definition(scvod, sized.x, sized.lab, sized.offs, sized.poses, LEAF)
    rev = _lmap(scvod)
    for s in reversed(range(sized.n_scans)):
        rev.accumulate_labelled(sized.d_x, sized.d_lab, sized.offs[s:s + 2], sized.poses[s:s + 1])
    _same(rev, ek, ev, "scans in reverse order")
    h = 7                                                                  # the last two scans hold half of the points
    a, b, c = _lmap(scvod), _lmap(scvod), _lmap(scvod, 1 << 13)
    a.accumulate_labelled(sized.d_x, sized.d_lab, sized.offs[:h + 1], sized.poses[:h])
    b.accumulate_labelled(sized.d_x, sized.d_lab, sized.offs[h:], sized.poses[h:])
    ka, _ = mr.sorted_records(a)
    kb, _ = mr.sorted_records(b)
    assert len(np.intersect1d(ka, kb)) > 100 and len(ka) < len(ek) and len(kb) < len(ek)
    c.merge(a.export())
    c.merge(b.export())
    _same(c, ek, ev, "two halves merged")
    g, counts = rev.export_parts(3)
    assert sum(counts) == len(ek) and min(counts) > 0
    d = _lmap(scvod, 1 << 13)
    off = np.concatenate([[0], np.cumsum(counts)])
    for p in (2, 0, 1):
        d.merge(g[int(off[p]):int(off[p + 1])])
    _same(d, ek, ev, "export_parts(3) merged")
    for q in (rev, a, b, c, d):
        q.close()


def test_bad_points_are_left_out_and_counted(scvod, sized):
    import torch
    x, lab = sized.x[:300].copy(), sized.lab[:300].copy()
    x[17, 0] = np.nan
    x[200, 1] = 0.5 * (1 << 20) + 10.0                                     # cell 2^20 + 20 on y
    offs = np.array([0, 300], np.int32)
    ek, ev, out = cmr.definition(scvod, x, lab, offs, None, LEAF)
    assert out == 2 and len(ek) > 100
    d_x, d_lab = _dev(x, lab)
    m = _lmap(scvod, 4096)
    m.accumulate_labelled(d_x, d_lab, offs)
    with pytest.raises(scvod.ScvodError) as e:
        m.count()
    assert _status(e) == ERR_CAPACITY
    assert int(re.search(r"(\d+) points did not fit", str(e.value)).group(1)) == 2
    buf = torch.full((len(ek) + 16, 2), SENT, dtype=torch.int64, device="cuda")
    n = C.c_int64(-1)
    assert m.lib.scvod_map_export(m.h, C.c_void_p(buf.data_ptr()), len(ek) + 16, C.byref(n), None) == ERR_CAPACITY
    h = buf.cpu().numpy().view(np.uint64)
    assert n.value == len(ek) and (h[len(ek):] == np.uint64(SENT)).all()
    o = np.argsort(h[:len(ek), 0])
    assert np.array_equal(h[:len(ek)][o, 0], ek) and np.array_equal(h[:len(ek)][o, 1], ev)      # the other cells are intact
    m.clear()
    assert m.count() == 0                                                 # empty, and the error is gone
    m.accumulate_labelled(d_x[:17], d_lab[:17], np.array([0, 17], np.int32))
    k1, v1, _ = cmr.definition(scvod, x, lab, np.array([0, 17], np.int32), None, LEAF)
    _same(m, k1, v1, "after clear")
    m.close()


def test_points_labelled(scvod, sized):
    import torch
    ek, ev, _ = cmr.definition(scvod, sized.x, sized.lab, sized.offs, sized.poses, LEAF)
    n = len(ek)
    m = _lmap(scvod)
    m.accumulate_labelled(sized.d_x, sized.d_lab, sized.offs, sized.poses)
    xyzi, lab, rec = m.points_labelled()
    xyzi, lab, rec = xyzi.cpu().numpy(), lab.cpu().numpy(), rec.cpu().numpy().view(np.uint64)
    assert xyzi.shape == (n, 4) and lab.shape == (n,) and rec.shape == (n, 2)
    o = np.argsort(rec[:, 0])
    assert np.array_equal(rec[o, 0], ek) and np.array_equal(rec[o, 1], ev)
    # row i of every output is record i: xyz the way test_points_decode_every_axis compares it, label and intensity the record's
    want, want_lab, want_i = cmr.decode_points(rec[:, 0], rec[:, 1], LEAF)
    got = xyzi[:, :3]
    ulp = np.spacing(np.abs(got)).astype(np.float64)
    for ax in range(3):
        assert (np.abs(got[:, ax].astype(np.float64) - want[:, ax]) <= 2 * ulp[:, ax]).all(), f"axis {ax}"
    assert np.array_equal(lab, want_lab) and np.array_equal(xyzi[:, 3].astype(np.float64), want_i)
    assert len(np.unique(lab)) > 100
    # "label L" and "not L" partition the map
    L = int(np.bincount(lab, minlength=256).argmax())
    n_L = int((lab == L).sum())
    assert 0 < n_L < n
    _, lab_a, rec_a = m.points_labelled(select=[L])
    _, lab_b, rec_b = m.points_labelled(select=[v for v in range(256) if v != L])
    lab_a, lab_b = lab_a.cpu().numpy(), lab_b.cpu().numpy()
    rec_a, rec_b = rec_a.cpu().numpy().view(np.uint64), rec_b.cpu().numpy().view(np.uint64)
    assert len(rec_a) == n_L and (lab_a == L).all() and len(rec_b) == n - n_L and not (lab_b == L).any()
    both = np.concatenate([rec_a, rec_b])
    o = np.argsort(both[:, 0])
    assert np.array_equal(both[o, 0], ek) and np.array_equal(both[o, 1], ev)
    assert np.array_equal(np.concatenate([lab_a, lab_b])[o], cmr.unpack_labelled(ev)[3].astype(np.uint8))
    # a buffer that is too short: the true count, and nothing at or behind cap
    guard, cap = 64, n_L - 3
    bx = torch.full((n_L + guard, 4), -7.0, dtype=torch.float32, device="cuda")
    bl = torch.full((n_L + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    br = torch.full((n_L + guard, 2), SENT, dtype=torch.int64, device="cuda")
    sel = cmr.table256([L])
    cnt = C.c_int64(-1)
    call = lambda c: m.lib.scvod_map_points_labelled(m.h, C.c_void_p(bx.data_ptr()), C.c_void_p(bl.data_ptr()), C.c_void_p(br.data_ptr()), c,  # noqa: E731
                                                     sel.ctypes.data_as(C.c_void_p), C.byref(cnt), None)
    assert call(cap) == ERR_CAPACITY and cnt.value == n_L
    assert (bx.cpu().numpy()[cap:] == -7.0).all() and (bl.cpu().numpy()[cap:] == 0xA5).all() and (br.cpu().numpy().view(np.uint64)[cap:] == np.uint64(SENT)).all()
    got_r = br.cpu().numpy().view(np.uint64)[:cap]
    assert len(np.unique(got_r[:, 0])) == cap and np.isin(got_r[:, 0], rec_a[:, 0]).all() and (bl.cpu().numpy()[:cap] == L).all()
    assert call(n_L) == 0 and cnt.value == n_L
    assert (bl.cpu().numpy()[n_L:] == 0xA5).all() and (bl.cpu().numpy()[:n_L] == L).all()
    # the map itself is intact
    _same(m, ek, ev, "after the short buffer")
    m.close()


def test_kind_errors_leave_the_table_untouched(scvod, sized):
    rng = np.random.default_rng(5)
    keys, vals = mr.random_keys(rng, 300), mr.random_keys(rng, 300)
    ek, ev = mr.reduce_records(keys, vals)
    offs = np.array([0, 300], np.int32)
    po = offs.ctypes.data_as(C.c_void_p)
    px, pl = C.c_void_p(sized.d_x.data_ptr()), C.c_void_p(sized.d_lab.data_ptr())
    plain = scvod.StaticMap(4096, leaf=LEAF)
    assert plain.lib.scvod_map_kind(plain.h) == 0 and plain.scratch_bytes() == 0
    plain.merge(mr.to_device(keys, vals))
    lib = plain.lib
    assert lib.scvod_map_accumulate_labelled(plain.h, px, pl, po, 1, None, None, None) == ERR_INVALID            # a plain map
    n = C.c_int64(-1)
    assert lib.scvod_map_points_labelled(plain.h, None, None, None, 0, None, C.byref(n), None) == ERR_INVALID
    _same(plain, ek, ev, "plain map after the refused calls")
    plain.close()
    lm = _lmap(scvod, 4096)
    lm.merge(mr.to_device(keys, vals))
    ctx = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    poses = np.zeros((1, 6), np.float32)
    pp = poses.ctypes.data_as(C.c_void_p)
    assert lib.scvod_batch_map_accumulate(ctx.h, lm.h, pp, 0, None) == ERR_INVALID                               # a labelled map
    assert lib.scvod_batch_map_accumulate_range(ctx.h, lm.h, pp, 4, 0, -1, None) == ERR_INVALID
    assert lib.scvod_batch_map_accumulate_classes(ctx.h, lm.h, pp, 0, 0, -1, None) == ERR_STATE                  # no batch
    assert lib.scvod_batch_map_accumulate_classes(ctx.h, lm.h, pp, 32, 0, -1, None) == ERR_INVALID               # an unknown flag
    assert lib.scvod_batch_map_accumulate_classes(ctx.h, lm.h, pp, 8 | 16, 0, -1, None) == ERR_INVALID           # both parts
    assert lib.scvod_map_accumulate_labelled(lm.h, C.c_void_p(sized.d_x.data_ptr() + 4), pl, po, 1, None, None, None) == ERR_INVALID   # misaligned
    assert lib.scvod_map_accumulate_labelled(lm.h, None, pl, po, 1, None, None, None) == ERR_INVALID
    assert lib.scvod_map_accumulate_labelled(lm.h, px, None, po, 1, None, None, None) == ERR_INVALID
    assert lib.scvod_map_accumulate_labelled(lm.h, px, pl, None, 1, None, None, None) == ERR_INVALID
    assert lib.scvod_map_accumulate_labelled(lm.h, px, pl, po, -1, None, None, None) == ERR_INVALID
    down = np.array([0, 200, 100], np.int32)
    assert lib.scvod_map_accumulate_labelled(lm.h, px, pl, down.ctypes.data_as(C.c_void_p), 2, None, None, None) == ERR_INVALID        # offsets decrease
    assert lib.scvod_map_accumulate_labelled(lm.h, None, None, np.array([5, 5, 5], np.int32).ctypes.data_as(C.c_void_p), 2, None, None, None) == 0   # empty
    assert lm.scratch_bytes() == 0
    _same(lm, ek, ev, "labelled map after the refused calls")
    ctx.close()
    lm.close()


# ---------------------------------------------------------------- part 2: the recognised map of a batch

BLEAF = 0.2
CELLS = 1 << 20
NO_GROUND, NO_REJECTED, IGNORE_DYNAMIC, PART_UNTRACKED, PART_TRACKED = 1, 2, 4, 8, 16


def _r3(scvod):
    k = _r3_with(scvod, True)
    if "cls_tracked" not in k:
        k["cls_tracked"] = _classes(k, 0)[0].copy()      # the device's own bytes, with the tracking result
    return k


def _labels_of(vals):
    return cmr.unpack_labelled(vals)[3]


@pytest.mark.parametrize("flags", [0, NO_GROUND, NO_REJECTED, NO_GROUND | NO_REJECTED, IGNORE_DYNAMIC])
def test_batch_against_the_helper_and_the_plain_map(scvod, flags):
    k = _r3(scvod)
    ctx, b = k["ctx"], k["b"]
    cls = k["cls_tracked"]
    ek, ev, out = cmr.definition(scvod, b.x, cls, b.offs, b.poses, BLEAF, cmr.batch_keep_table(flags))
    assert out == 0 and len(ek) > 10000
    m = _lmap(scvod, CELLS, BLEAF)
    m.accumulate_classes(ctx, b.poses, flags)
    assert m.scratch_bytes() == k["n"]
    _same(m, ek, ev, f"flags {flags}")
    # not vacuous
    got = np.bincount(_labels_of(ev), minlength=256)
    print(f"flags {flags}: {len(ek)} cells, per label {got[:8].tolist()}")
    assert got[8:].sum() == 0 and got[0] == 0
    assert got[7] > 0 and (got[5] > 0 or got[6] > 0)
    assert (got[1] > 0) == (not flags & NO_GROUND) and (got[2] == 0 or not flags & NO_REJECTED)
    if flags & IGNORE_DYNAMIC:
        assert got[6] > 0, "the raw map is meant to hold dynamic cells"
    else:
        assert got[6] == 0
    # the cells and the leading 48 bits are the plain map's
    p = scvod.StaticMap(CELLS, leaf=BLEAF)
    p.accumulate(ctx, b.poses, flags=flags)
    pk, pv = mr.sorted_records(p)
    assert np.array_equal(pk, ek) and np.array_equal(pv >> U16, ev >> U16)
    p.close()
    m.close()


def test_batch_ranges(scvod):
    k = _r3(scvod)
    ctx, b = k["ctx"], k["b"]
    keep = cmr.batch_keep_table(0)
    m = _lmap(scvod, CELLS, BLEAF)
    for first, count in ((0, 1), (1, 2), (2, 1), (1, -1), (3, 0)):
        m.clear()
        m.accumulate_classes(ctx, b.poses, 0, first, count)
        scans = range(first, b.n if count < 0 else first + count)
        ek, ev, _ = cmr.definition(scvod, b.x, k["cls_tracked"], b.offs, b.poses, BLEAF, keep, scans=scans)
        assert (len(ek) > 10000) == (len(scans) > 0)
        _same(m, ek, ev, f"range ({first}, {count})")
    pp = b.poses.ctypes.data_as(C.c_void_p)
    for first, count in ((-1, 1), (0, 4), (4, 0), (2, 2)):
        assert m.lib.scvod_batch_map_accumulate_classes(ctx.h, m.h, pp, 0, first, count, None) == ERR_INVALID
    assert m.count() == 0
    m.close()


def test_batch_parts_and_state_errors(scvod):
    import torch
    k = _r3(scvod)
    b, n = k["b"], k["n"]
    ctx = _new_ctx(scvod, [b])
    lib = ctx.lib
    buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    pb, pp = C.c_void_p(buf.data_ptr()), b.poses.ctypes.data_as(C.c_void_p)
    m = _lmap(scvod, CELLS, BLEAF)
    ALL = (0, NO_GROUND, IGNORE_DYNAMIC, PART_UNTRACKED, PART_TRACKED, PART_TRACKED | IGNORE_DYNAMIC)

    def states(what):
        """every flag combination answers what scvod_batch_point_classes answers for the bytes it needs"""
        got = {}
        for f in ALL:
            want = lib.scvod_batch_point_classes(ctx.h, pb, n, IGNORE_DYNAMIC if f & PART_UNTRACKED else 0, None)
            got[f] = lib.scvod_batch_map_accumulate_classes(ctx.h, m.h, pp, f, 0, -1, None)
            assert got[f] == want, f"{what}: flags {f}: {got[f]} != {want}"
        return got

    assert set(states("no batch").values()) == {ERR_STATE}
    ctx.batch_process(b.d, b.offs)
    assert set(states("no clustering").values()) == {ERR_STATE}
    ctx.batch_cluster()
    assert set(states("no types").values()) == {ERR_STATE}
    assert m.count() == 0
    ctx.set_region_growing(True)
    ctx.batch_cluster_types()
    got = states("no tracking result")
    assert got[PART_UNTRACKED] == 0 and all(v == ERR_INVALID for f, v in got.items() if f != PART_UNTRACKED)
    # part UNTRACKED ran before any scvod_batch_track: everything that is not a member of a car cluster
    uk, uv = mr.sorted_records(m)
    cls0 = ctx.batch_point_classes(flags=IGNORE_DYNAMIC).cpu().numpy()[:n]
    ek, ev, _ = cmr.definition(scvod, b.x, cls0, b.offs, b.poses, BLEAF, cmr.batch_keep_table(PART_UNTRACKED))
    assert np.array_equal(uk, ek) and np.array_equal(uv, ev) and not np.isin(_labels_of(uv), [5, 6]).any()
    _track(ctx, b, b.T, b.nxt, None, 1)
    cls = ctx.batch_point_classes().cpu().numpy()[:n]
    assert np.array_equal(cls, k["cls_tracked"])
    for extra in (0, IGNORE_DYNAMIC, NO_GROUND):
        m.clear()
        m.accumulate_classes(ctx, b.poses, PART_UNTRACKED | extra)
        m.accumulate_classes(ctx, b.poses, PART_TRACKED | extra)
        whole = _lmap(scvod, CELLS, BLEAF)
        whole.accumulate_classes(ctx, b.poses, extra)
        wk, wv = mr.sorted_records(whole)
        _same(m, wk, wv, f"two parts, flags {extra}")
        ek, ev, _ = cmr.definition(scvod, b.x, cls, b.offs, b.poses, BLEAF, cmr.batch_keep_table(extra))
        assert np.array_equal(wk, ek) and np.array_equal(wv, ev)
        m.clear()
        m.accumulate_classes(ctx, b.poses, PART_TRACKED | extra)
        tk, tv = mr.sorted_records(m)
        assert len(tk) > 0 and np.isin(_labels_of(tv), [5, 6] if extra & IGNORE_DYNAMIC else [5]).all()
        whole.close()
    ctx.batch_cluster_types()                                            # the tracking result is stale now
    got = states("stale tracking result")
    assert got[PART_UNTRACKED] == 0 and all(v == ERR_INVALID for f, v in got.items() if f != PART_UNTRACKED)
    m.close()
    ctx.close()


def test_batch_end_to_end_and_nothing_else_moves(scvod):
    import quality
    k = _r3(scvod)
    ctx, b, n = k["ctx"], k["b"], k["n"]

    def snapshot():
        p = scvod.StaticMap(CELLS, leaf=BLEAF)
        p.accumulate(ctx, b.poses)
        rec = mr.sorted_records(p)
        p.close()
        return ctx.arena_bytes(), rec[0], rec[1], ctx.batch_point_labels().cpu().numpy()[:n].copy(), _classes(k, 0)[0].copy()

    before = snapshot()
    m = _lmap(scvod, CELLS, BLEAF)
    assert m.scratch_bytes() == 0
    m.accumulate_classes(ctx, b.poses, 0)
    xyzi, lab, rec = m.points_labelled()
    assert m.scratch_bytes() == n
    # the map's points under their labels as the estimate of the class scores
    w = quality.world_points(scvod, b.x, b.offs, b.poses)
    est = xyzi[:, :3].contiguous()
    ctx.score_classes_device(_cuda(w, np.float32), k["d_gt"], est, lab.contiguous())
    got = ctx.score_classes_stats()
    want = csr.score(w, k["gt"], est.cpu().numpy(), lab.cpu().numpy(), nn_fn=csr.tree_nn)
    _assert_result(got, None, want, "the labelled map as the estimate")
    conf = np.asarray(want["conf"])
    assert int(conf.sum()) == n and conf[0, 1] > 0 and conf[1, 2] > 0
    after = snapshot()
    for x, y in zip(before, after):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    m.close()
