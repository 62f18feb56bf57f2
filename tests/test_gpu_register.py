"""scvod_map_register / scvod_batch_map_register / scvod_register_device on the device, through the C-ABI: poses (fp64) and 64-byte
records per scan against the CPU helper (tests/helpers/register_ref.py: the library's reg_* functions in a sequential C++ loop with an
exhaustive search).  The sums are integers and the solve is IEEE-basic operations in a stated order, so every comparison with the
helper is on the raw bytes.  Guard regions lie behind every output."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import map_ref as mr  # noqa: E402
import register_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 4
LEAF, R_MAP, R_CLOUD = 0.1, 0.099, 0.2
EYE = np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
STARTS = ((0.003, 0.04), (0.002, 0.03), (0.001, 0.05))
ALL64 = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("registerref"))


@pytest.fixture(scope="module")
def cloud():
    xyzi, world, normals = rr.corner_cloud()
    return dict(xyzi=xyzi, world=world, normals=normals, n=len(xyzi))


@pytest.fixture(scope="module")
def ctx(scvod):
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=8192, max_scans=4)
    yield c
    c.close()


def _start6(scvod, d_rot, d_trans):
    """the start pose as the {x, y, z, roll, pitch, yaw} the calls take, and the fp32 matrix the device makes of it"""
    p6 = scvod.pose_from_matrix(rr.start_matrix(d_rot, d_trans))
    return p6, scvod.pose_matrix(p6)


class Out:
    """pose and record buffers of one call with guard regions of GUARD rows before the first row and behind row n_scans"""

    def __init__(self, n_scans):
        import torch
        self.n = n_scans
        self.pose = torch.full(((n_scans + 2 * GUARD) * 96,), 0xA5, dtype=torch.uint8, device="cuda")
        self.rec = torch.full(((n_scans + 2 * GUARD) * 64,), 0xA5, dtype=torch.uint8, device="cuda")

    def ptrs(self):
        """(GUARD rows into the buffers: 384 and 256 bytes, so both stay 8-byte aligned)"""
        assert self.pose.data_ptr() % 8 == 0 and self.rec.data_ptr() % 8 == 0
        return C.c_void_p(self.pose.data_ptr() + GUARD * 96), C.c_void_p(self.rec.data_ptr() + GUARD * 64)

    def _rows(self):
        pose, rec = self.pose.cpu().numpy(), self.rec.cpu().numpy()
        for a, w, what in ((pose, 96, "poses"), (rec, 64, "records")):
            assert (a[:GUARD * w] == 0xA5).all(), f"{what} were written before the first row"
            assert (a[(GUARD + self.n) * w:] == 0xA5).all(), f"{what} were written behind n_scans"
        return pose[GUARD * 96:(GUARD + self.n) * 96], rec[GUARD * 64:(GUARD + self.n) * 64]

    def host(self):
        pose, rec = self._rows()
        return dict(pose=pose.copy().view(np.float64).reshape(-1, 12), records=rec.copy().view(rr.RECORD_DTYPE))

    def untouched(self):
        """a refused call wrote nothing at all"""
        pose, rec = self._rows()
        return bool((pose == 0xA5).all() and (rec == 0xA5).all())


def _params(scvod, p):
    return scvod.register_params_default(use256=p["use256"], max_iterations=p["max_iterations"], min_corr=p["min_corr"], mode=p["mode"],
                                         max_dist=p["max_dist"], max_range=p["max_range"], eps_rot=p["eps_rot"], eps_trans=p["eps_trans"],
                                         lam=p["lam"], pivot_eps=p["pivot_eps"])


def _dev(a, dtype=F):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _on_cloud(scvod, ctx, src, offs, poses6, tgt, p, labels=None, normals=None):
    out = Out(len(offs) - 1)
    d_src, d_tgt = _dev(np.asarray(src, F).reshape(-1, 4)), _dev(np.asarray(tgt, F).reshape(-1, 3))
    d_lab = None if labels is None else _dev(labels, np.uint8)
    d_nrm = None if normals is None else _dev(np.asarray(normals, F).reshape(-1, 3))
    off = np.ascontiguousarray(offs, np.int32)
    p6 = np.ascontiguousarray(poses6, F).reshape(-1, 6)
    q = _params(scvod, p)
    rc = ctx.lib.scvod_register_device(ctx.h, C.c_void_p(d_src.data_ptr()), off.ctypes.data_as(C.c_void_p), len(off) - 1,
                                       p6.ctypes.data_as(C.c_void_p), None if d_lab is None else C.c_void_p(d_lab.data_ptr()),
                                       C.c_void_p(d_tgt.data_ptr()) if len(d_tgt) else None,
                                       None if d_nrm is None else C.c_void_p(d_nrm.data_ptr()), len(d_tgt), C.byref(q), *out.ptrs(), None)
    assert rc == 0, ctx.lib.scvod_last_error(ctx.h)
    return out.host()


def _on_map(scvod, m, src, offs, poses6, p, labels=None, select=None):
    out = Out(len(offs) - 1)
    d_src = _dev(np.asarray(src, F).reshape(-1, 4))
    d_lab = None if labels is None else _dev(labels, np.uint8)
    off = np.ascontiguousarray(offs, np.int32)
    p6 = np.ascontiguousarray(poses6, F).reshape(-1, 6)
    q = _params(scvod, p)
    k, pk = m._table256(select)
    rc = m.lib.scvod_map_register(m.h, C.c_void_p(d_src.data_ptr()), off.ctypes.data_as(C.c_void_p), len(off) - 1, p6.ctypes.data_as(C.c_void_p),
                                  None if d_lab is None else C.c_void_p(d_lab.data_ptr()), C.byref(q), pk, *out.ptrs(), None)
    assert rc == 0, m.lib.scvod_map_last_error(m.h)
    return out.host()


def _same(dev, hlp, what=""):
    assert dev["records"].tobytes() == hlp["records"].tobytes(), (what, dev["records"], hlp["records"])
    assert dev["pose"].tobytes() == hlp["pose"].tobytes(), (what, np.abs(dev["pose"] - hlp["pose"]).max())


def _plain_map(scvod, world):
    """a plain map that holds exactly the points `world` (zero pose), and its decoded points with their keys"""
    w4 = np.concatenate([np.asarray(world, F), np.ones((len(world), 1), F)], 1)
    keys, vals, ok = mr.encode_points(EYE, w4, LEAF)
    assert ok.all()
    m = scvod.StaticMap(1 << 13, leaf=LEAF)
    m.merge(mr.to_device(*mr.reduce_records(keys, vals)))
    return m


def _labelled_map(scvod, world, labels):
    m = scvod.StaticMap(1 << 13, leaf=LEAF, kind=scvod.MAP_KIND_LABELLED)
    w4 = np.concatenate([np.asarray(world, F), np.ones((len(world), 1), F)], 1)
    m.accumulate_labelled(_dev(w4), _dev(labels, np.uint8), [0, len(w4)], None, None)
    return m


def _map_target(m, select=None):
    """the helper's target for a map: scvod_map_points' decoded output and the keys"""
    if select is None:
        xyzi, rec = m.points()
    else:
        xyzi, _, rec = m.points_labelled(select)
    return xyzi.cpu().numpy()[:, :3].copy(), rec.cpu().numpy().view(np.uint64)[:, 0].copy()


def _own_image(tgt_xyz, world):
    """for every source point the index of the target point that is its own image (the target's order is unspecified)"""
    d = np.linalg.norm(tgt_xyz.astype(np.float64)[None, :, :] - world.astype(np.float64)[:, None, :], axis=2)
    own = d.argmin(axis=1)
    assert d[np.arange(len(world)), own].max() < 2e-5 and len(np.unique(own)) == len(world)
    return own


# ---------------------------------------------------------------- equality with the helper on the crafted cloud

@pytest.mark.parametrize("iters", [1, 2, 10])
@pytest.mark.parametrize("target", ["cloud-point", "cloud-plane", "map-plain", "map-labelled"])
def test_crafted_cloud_equals_the_helper(scvod, ctx, ref, cloud, target, iters):
    p6, T0 = _start6(scvod, *STARTS[0])
    offs = [0, cloud["n"]]
    if target.startswith("cloud"):
        mode = rr.PLANE if target == "cloud-plane" else rr.POINT
        p = rr.params(mode=mode, max_iterations=iters, max_dist=R_CLOUD)
        h = rr.run(ref, cloud["xyzi"], offs, T0, cloud["world"], p, tgt_nrm=cloud["normals"])
        assert np.array_equal(h["match0"], np.arange(cloud["n"])), "the condition of the test: every point matches its own image"
        d = _on_cloud(scvod, ctx, cloud["xyzi"], offs, p6, cloud["world"], p, normals=cloud["normals"])
        stats = ctx.register_stats()
    else:
        m = _plain_map(scvod, cloud["world"]) if target == "map-plain" else _labelled_map(scvod, cloud["world"], np.full(cloud["n"], 3, np.uint8))
        assert m.count() == cloud["n"], "a cell of the map holds more than one point of the crafted cloud"
        tgt, keys = _map_target(m)
        p = rr.params(max_iterations=iters, max_dist=R_MAP)
        h = rr.run(ref, cloud["xyzi"], offs, T0, tgt, p, tgt_key=keys)
        assert np.array_equal(h["match0"], _own_image(tgt, cloud["world"])), "the condition of the test: every point matches its own image"
        d = _on_map(scvod, m, cloud["xyzi"], offs, p6, p)
        stats = m.register_stats()
        m.close()
    _same(d, h, target)
    e0, eh, ed = rr.pose_error(T0, cloud["xyzi"]), rr.pose_error(h["pose"][0], cloud["xyzi"]), rr.pose_error(d["pose"][0], cloud["xyzi"])
    rec = d["records"][0]
    print(f"{target} x{iters}: start {e0:.3e} m, helper {eh:.6e} m, device {ed:.6e} m, status {rec['status']}, iterations {rec['iterations']}")
    assert ed == eh and ed < e0
    assert rec["n_corr"] == cloud["n"]
    assert stats["scans"] == 1 and stats["points"] == cloud["n"] and stats["correspondences"] == rec["n_corr"]
    assert stats["iterations"] == rec["iterations"] and stats["skipped"] == 0
    assert [stats["max_iterations"], stats["converged"], stats["degenerate"]] == [int(rec["status"] == v) for v in (0, 1, 2)]


# ---------------------------------------------------------------- against the query of the parent commit

def test_correspondences_are_the_querys_hits(scvod, ref, cloud):
    """max_iterations 1: a scan's correspondences are its points whose d_nn_key != ~0 in scvod_map_query (same poses, radius, select)"""
    import torch
    rng = np.random.default_rng(11)
    m = _labelled_map(scvod, cloud["world"], np.where(np.arange(cloud["n"]) < 484, 5, 3).astype(np.uint8))
    noisy = cloud["xyzi"].copy()
    noisy[:, :3] += rng.normal(scale=0.04, size=(cloud["n"], 3)).astype(F)
    src = np.concatenate([cloud["xyzi"], noisy, cloud["xyzi"][::3]])
    offs = np.asarray([0, cloud["n"], 2 * cloud["n"], len(src)], np.int32)
    poses = np.stack([_start6(scvod, *s)[0] for s in STARTS])
    for select in (None, [3]):
        p = rr.params(max_iterations=1, max_dist=R_MAP, max_range=float("inf"))
        d = _on_map(scvod, m, src, offs, poses, p, select=select)
        q = m.query(torch.from_numpy(src).cuda(), offs, poses, R_MAP, select, ("nn_key",))["nn_key"].cpu().numpy().view(np.uint64)
        hits = [int((q[offs[s]:offs[s + 1]] != np.uint64(ALL64)).sum()) for s in range(3)]
        assert d["records"]["n_corr"].tolist() == hits and min(hits) > 100
        assert (d["records"]["n_corr"] + d["records"]["skip_no_corr"]).tolist() == np.diff(offs).tolist()
        tgt, keys = _map_target(m, select)
        _same(d, rr.run(ref, src, offs, [scvod.pose_matrix(x) for x in poses], tgt, p, tgt_key=keys), f"select {select}")
    m.close()


# ---------------------------------------------------------------- shapes where the kernel can go wrong

SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2049)


@pytest.mark.parametrize("target", ["cloud", "map"])
def test_scan_sizes_in_one_call_and_alone(scvod, ctx, ref, cloud, target):
    rng = np.random.default_rng(3)
    pick = [rng.integers(0, cloud["n"], n) for n in SIZES]
    src = np.concatenate([cloud["xyzi"][i] for i in pick])
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    poses = np.stack([_start6(scvod, *STARTS[s % 3])[0] for s in range(len(SIZES))])
    T0 = [scvod.pose_matrix(x) for x in poses]
    m = _plain_map(scvod, cloud["world"]) if target == "map" else None
    tgt, keys = _map_target(m) if m else (cloud["world"], None)
    p = rr.params(max_iterations=4, max_dist=R_MAP if m else R_CLOUD, min_corr=6)

    def run(s, o, q):
        return _on_map(scvod, m, s, o, q, p) if m else _on_cloud(scvod, ctx, s, o, q, cloud["world"], p)

    d = run(src, offs, poses)
    _same(d, rr.run(ref, src, offs, T0, tgt, p, tgt_key=keys), target)
    st = d["records"]["status"]
    assert (st[:3] == rr.DEGENERATE).all() and (st[3:] != rr.DEGENERATE).all()
    for s, n in enumerate(SIZES):
        solo = run(src[offs[s]:offs[s + 1]], [0, n], poses[s:s + 1])
        assert solo["pose"].tobytes() == d["pose"][s:s + 1].tobytes() and solo["records"].tobytes() == d["records"][s:s + 1].tobytes(), n
    if m:
        m.close()


def test_three_start_errors_and_an_empty_scan_in_one_call(scvod, ctx, ref, cloud):
    src = np.concatenate([cloud["xyzi"]] * 3)
    n = cloud["n"]
    offs = [0, n, n, 2 * n, 3 * n]  # (scan 1 is empty)
    poses = np.stack([_start6(scvod, *STARTS[i])[0] for i in (0, 1, 1, 2)])
    p = rr.params(max_dist=R_CLOUD)
    d = _on_cloud(scvod, ctx, src, offs, poses, cloud["world"], p)
    st = ctx.register_stats()
    _same(d, rr.run(ref, src, offs, [scvod.pose_matrix(x) for x in poses], cloud["world"], p))
    assert d["records"]["status"].tolist() == [rr.CONVERGED, rr.DEGENERATE, rr.CONVERGED, rr.CONVERGED]
    assert d["pose"][1].tobytes() == scvod.pose_matrix(poses[1]).astype(np.float64).tobytes()
    for s in (0, 2, 3):
        solo = _on_cloud(scvod, ctx, cloud["xyzi"], [0, n], poses[s:s + 1], cloud["world"], p)
        assert solo["pose"].tobytes() == d["pose"][s:s + 1].tobytes() and solo["records"].tobytes() == d["records"][s:s + 1].tobytes(), s
    assert (st["scans"], st["converged"], st["degenerate"], st["max_iterations"], st["points"]) == (4, 3, 1, 0, 3 * n)
    assert st["iterations"] == int(d["records"]["iterations"].sum()) and st["correspondences"] == 3 * n


def test_launch_geometry_and_point_order_do_not_matter(scvod, ctx, ref, cloud):
    rng = np.random.default_rng(8)
    pick = rng.integers(0, cloud["n"], 2049)
    src = cloud["xyzi"][pick]
    p6, T0 = _start6(scvod, *STARTS[0])
    m = _plain_map(scvod, cloud["world"])
    pc, pm = rr.params(max_dist=R_CLOUD, mode=rr.PLANE), rr.params(max_dist=R_MAP)
    base_c = _on_cloud(scvod, ctx, src, [0, 2049], p6, cloud["world"], pc, normals=cloud["normals"])
    base_m = _on_map(scvod, m, src, [0, 2049], p6, pm)
    try:
        for blocks in (1, 3, 40):
            ctx.lib.scvod__debug_register_blocks(blocks)
            _same(_on_cloud(scvod, ctx, src, [0, 2049], p6, cloud["world"], pc, normals=cloud["normals"]), base_c, f"{blocks} workgroups")
            _same(_on_map(scvod, m, src, [0, 2049], p6, pm), base_m, f"{blocks} workgroups")
    finally:
        ctx.lib.scvod__debug_register_blocks(0)
    o = rng.permutation(2049)
    _same(_on_cloud(scvod, ctx, src[o], [0, 2049], p6, cloud["world"], pc, normals=cloud["normals"]), base_c, "shuffled")
    _same(_on_map(scvod, m, src[o], [0, 2049], p6, pm), base_m, "shuffled")
    tgt, keys = _map_target(m)
    a, b = rr.run(ref, src, [0, 2049], T0, tgt, pm, tgt_key=keys), rr.run(ref, src[o], [0, 2049], T0, tgt, pm, tgt_key=keys)
    assert np.array_equal(a["sums"], b["sums"])
    _same(base_m, a)
    m.close()


@pytest.mark.parametrize("target", ["cloud", "map"])
def test_the_latch(scvod, ctx, cloud, target):
    """max_iterations 16 gives the bytes of stopping at the iteration the record reports (each target has a kernel of its own)"""
    p6, _ = _start6(scvod, *STARTS[0])
    m = _plain_map(scvod, cloud["world"]) if target == "map" else None

    def run(iters):
        if m:
            return _on_map(scvod, m, cloud["xyzi"], [0, cloud["n"]], p6, rr.params(max_iterations=iters, max_dist=R_MAP))
        return _on_cloud(scvod, ctx, cloud["xyzi"], [0, cloud["n"]], p6, cloud["world"], rr.params(max_iterations=iters, max_dist=R_CLOUD))

    long = run(16)
    it = int(long["records"]["iterations"][0])
    assert long["records"]["status"][0] == rr.CONVERGED and 2 <= it <= 5
    _same(run(it), long)
    short = run(it - 1)
    assert short["records"]["status"][0] == rr.MAX_ITERATIONS and short["pose"].tobytes() != long["pose"].tobytes()
    if m:
        m.close()


# ---------------------------------------------------------------- gates

def test_the_label_gate_keeps_dynamic_points_out(scvod, ctx, ref, cloud):
    DYN = scvod.PT_DYNAMIC
    moved = cloud["xyzi"][:300].copy()
    moved[:, 0] += F(0.08)  # a block of points that moved since the target was taken
    src = np.concatenate([cloud["xyzi"][300:], moved])
    labels = np.concatenate([np.full(cloud["n"] - 300, 4, np.uint8), np.full(300, DYN, np.uint8)])
    use = np.ones(256, np.uint8)
    use[DYN] = 0
    p6, T0 = _start6(scvod, *STARTS[1])
    free, gated = rr.params(max_dist=R_CLOUD), rr.params(max_dist=R_CLOUD, use256=use)
    a = _on_cloud(scvod, ctx, src, [0, len(src)], p6, cloud["world"], free, labels=labels)
    b = _on_cloud(scvod, ctx, src, [0, len(src)], p6, cloud["world"], gated, labels=labels)
    c = _on_cloud(scvod, ctx, src[:-300], [0, len(src) - 300], p6, cloud["world"], free)
    _same(b, rr.run(ref, src, [0, len(src)], T0, cloud["world"], gated, labels=labels))
    assert a["pose"].tobytes() != b["pose"].tobytes() and b["pose"].tobytes() == c["pose"].tobytes()
    assert b["records"]["skip_label"][0] == 300 and a["records"]["skip_label"][0] == 0
    assert b["records"]["n_corr"][0] == c["records"]["n_corr"][0] == cloud["n"] - 300
    assert rr.pose_error(b["pose"][0], cloud["xyzi"]) < rr.pose_error(a["pose"][0], cloud["xyzi"])


def test_nan_range_and_normal_skips_are_counted(scvod, ctx, ref, cloud):
    src = cloud["xyzi"].copy()
    src[5::97, 1] = np.nan
    nrm = cloud["normals"].copy()
    nrm[::50] = 0
    nrm[7::61, 2] = np.nan
    p6, T0 = _start6(scvod, *STARTS[2])
    for mode in (rr.POINT, rr.PLANE):
        p = rr.params(mode=mode, max_dist=R_CLOUD, max_range=9.0)
        d = _on_cloud(scvod, ctx, src, [0, cloud["n"]], p6, cloud["world"], p, normals=nrm)
        _same(d, rr.run(ref, src, [0, cloud["n"]], T0, cloud["world"], p, tgt_nrm=nrm), f"mode {mode}")
        r = d["records"][0]
        far = int((np.linalg.norm(src[:, :3].astype(np.float64), axis=1) > 9.0).sum())
        assert r["skip_nan"] == len(src[5::97]) and abs(int(r["skip_range"]) - far) <= 2 and far > 50
        assert (r["skip_normal"] > 5) == (mode == rr.PLANE) and (mode == rr.PLANE or r["skip_normal"] == 0)
        assert r["n_corr"] + r["skip_nan"] + r["skip_range"] + r["skip_no_corr"] + r["skip_normal"] == cloud["n"]
        assert r["status"] == rr.CONVERGED


def test_select_table_on_a_labelled_map(scvod, ref, cloud):
    """face 0 of the corner carries label 5, the other two label 3: with select {3} the points of face 0 find nothing"""
    labels = np.where(np.arange(cloud["n"]) < 484, 5, 3).astype(np.uint8)
    m = _labelled_map(scvod, cloud["world"], labels)
    p6, T0 = _start6(scvod, *STARTS[0])
    p = rr.params(max_dist=R_MAP)
    for select, n_corr in ((None, cloud["n"]), ([3], cloud["n"] - 484), ([5], 484)):
        d = _on_map(scvod, m, cloud["xyzi"], [0, cloud["n"]], p6, p, select=select)
        tgt, keys = _map_target(m, select)
        _same(d, rr.run(ref, cloud["xyzi"], [0, cloud["n"]], T0, tgt, p, tgt_key=keys), f"select {select}")
        assert d["records"]["n_corr"][0] == n_corr and d["records"]["skip_no_corr"][0] == cloud["n"] - n_corr
    m.close()
    plain = _plain_map(scvod, cloud["world"])
    out = Out(1)
    off, q6 = np.asarray([0, cloud["n"]], np.int32), np.ascontiguousarray(p6, F)
    sel = np.ones(256, np.uint8)
    rc = plain.lib.scvod_map_register(plain.h, C.c_void_p(_dev(cloud["xyzi"]).data_ptr()), off.ctypes.data_as(C.c_void_p), 1,
                                      q6.ctypes.data_as(C.c_void_p), None, C.byref(_params(scvod, p)), sel.ctypes.data_as(C.c_void_p), *out.ptrs(),
                                      None)
    assert rc == -1 and b"select table" in plain.lib.scvod_map_last_error(plain.h)
    assert out.untouched()
    plain.close()


def test_the_calls_refuse_and_write_nothing(scvod, ctx, cloud):
    """the refusals of scvod_register_check through the entry points themselves: status SCVOD_ERR_INVALID, outputs and guards untouched,
    nothing allocated"""
    m = _plain_map(scvod, cloud["world"])
    fresh = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=4096, max_scans=1)
    d_src, d_tgt = _dev(cloud["xyzi"]), _dev(cloud["world"])
    off = np.asarray([0, cloud["n"]], np.int32)
    p6 = np.ascontiguousarray(_start6(scvod, *STARTS[0])[0], F)
    po, pp = off.ctypes.data_as(C.c_void_p), p6.ctypes.data_as(C.c_void_p)

    def on_map(q, src=None):
        out = Out(1)
        rc = m.lib.scvod_map_register(m.h, C.c_void_p(src or d_src.data_ptr()), po, 1, pp, None, C.byref(q), None, *out.ptrs(), None)
        return rc, out.untouched()

    def on_cloud(q, src=None, nrm=None):
        out = Out(1)
        rc = fresh.lib.scvod_register_device(fresh.h, C.c_void_p(src or d_src.data_ptr()), po, 1, pp, None, C.c_void_p(d_tgt.data_ptr()), nrm,
                                             cloud["n"], C.byref(q), *out.ptrs(), None)
        return rc, out.untouched()

    d = scvod.register_params_default
    for bad in (dict(max_iterations=0), dict(max_iterations=65), dict(min_corr=5), dict(mode=2), dict(max_range=0.0)):
        assert on_map(d(**dict(dict(max_dist=R_MAP), **bad))) == (-1, True), bad
        assert on_cloud(d(**dict(dict(max_dist=R_CLOUD), **bad))) == (-1, True), bad
    assert on_map(d(max_dist=float(F(0.995) * F(LEAF)))) == (-1, True) and b"0.99" in m.lib.scvod_map_last_error(m.h)
    assert on_map(d(max_dist=R_MAP, mode=scvod.REG_PLANE)) == (-1, True)
    assert on_cloud(d(max_dist=R_CLOUD, mode=scvod.REG_PLANE)) == (-1, True) and b"normals" in fresh.lib.scvod_last_error(fresh.h)
    assert on_map(d(max_dist=R_MAP), src=d_src.data_ptr() + 4) == (-1, True) and b"aligned" in m.lib.scvod_map_last_error(m.h)
    assert on_cloud(d(max_dist=R_CLOUD), src=d_src.data_ptr() + 8) == (-1, True)
    out = Out(1)
    rc = m.lib.scvod_map_register(m.h, C.c_void_p(d_src.data_ptr()), po, 1, pp, None, C.byref(d(max_dist=R_MAP)), None,
                                  C.c_void_p(out.ptrs()[0].value + 4), out.ptrs()[1], None)
    assert rc == -1 and out.untouched()  # a d_pose_out that is not 8-byte aligned
    assert m.register_scratch_bytes() == 0 and fresh.register_scratch_bytes() == 0
    assert m.lib.scvod_map_register_stats(m.h, (C.c_int64 * 8)()) == -5  # SCVOD_ERR_STATE: no call ran
    fresh.close()
    m.close()


# ---------------------------------------------------------------- degenerate scans

def test_degenerate_scans_keep_their_pose(scvod, ctx, ref, cloud):
    n = cloud["n"]
    src = np.concatenate([cloud["xyzi"], cloud["xyzi"], cloud["xyzi"][:10], cloud["xyzi"][:484]])
    offs = [0, n, 2 * n, 2 * n + 10, 2 * n + 494]
    good, _ = _start6(scvod, *STARTS[0])
    away = good.copy()
    away[0] += F(50.0)  # no correspondence at all (a shift inside the faces' extent would find the lattice again)
    poses = np.stack([good, away, good, good])
    T0 = [scvod.pose_matrix(x) for x in poses]
    for mode in (rr.POINT, rr.PLANE):
        p = rr.params(mode=mode, max_dist=R_CLOUD)
        d = _on_cloud(scvod, ctx, src, offs, poses, cloud["world"], p, normals=cloud["normals"])
        _same(d, rr.run(ref, src, offs, T0, cloud["world"], p, tgt_nrm=cloud["normals"]), f"mode {mode}")
        want = [rr.CONVERGED, rr.DEGENERATE, rr.DEGENERATE, rr.DEGENERATE if mode == rr.PLANE else rr.CONVERGED]
        assert d["records"]["status"].tolist() == want
        assert d["records"]["n_corr"].tolist() == [n, 0, 10, 484]
        for s in range(4):
            if want[s] == rr.DEGENERATE:
                assert d["pose"][s].tobytes() == T0[s].astype(np.float64).tobytes(), s
        solo = _on_cloud(scvod, ctx, cloud["xyzi"], [0, n], good, cloud["world"], p, normals=cloud["normals"])
        assert solo["pose"].tobytes() == d["pose"][:1].tobytes() and solo["records"].tobytes() == d["records"][:1].tobytes()
    empty = _on_cloud(scvod, ctx, cloud["xyzi"], [0, n], good, np.zeros((0, 3), F), rr.params(max_dist=R_CLOUD))
    assert empty["records"]["status"][0] == rr.DEGENERATE and empty["records"]["skip_no_corr"][0] == n


# ---------------------------------------------------------------- state, and the batch form

def test_batch_and_ctx_free_calls_alternate_on_one_map(scvod, ref, cloud):
    """a batch call of 4 scans between two ctx-free calls of 2 scans with the same offsets and poses: the 4-scan sums lie where the
    2-scan call staged its offsets, so the second ctx-free call has to stage them again"""
    import torch
    m = _plain_map(scvod, cloud["world"])
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=4096, max_scans=4)
    d = torch.from_numpy(cloud["xyzi"]).cuda()
    off4, off2 = np.asarray([0, 300, 700, 1000, cloud["n"]], np.int32), [0, 700, cloud["n"]]
    c.batch_process(d, off4)
    p6 = _start6(scvod, *STARTS[0])[0]
    q = scvod.register_params_default(max_dist=R_MAP)
    p = rr.params(max_dist=R_MAP)
    tgt, keys = _map_target(m)
    want4 = rr.run(ref, cloud["xyzi"], off4, [scvod.pose_matrix(p6)] * 4, tgt, p, tgt_key=keys)
    want2 = rr.run(ref, cloud["xyzi"], off2, [scvod.pose_matrix(p6)] * 2, tgt, p, tgt_key=keys)
    for _ in range(2):
        b = scvod.register_result(*m.register_batch(c, np.stack([p6] * 4), params=q))
        assert b["matrices"].tobytes() == want4["pose"].tobytes() and b["records"].tobytes() == want4["records"].tobytes()
        assert m.register_stats()["points"] == cloud["n"]
        _same(_on_map(scvod, m, cloud["xyzi"], off2, np.stack([p6] * 2), p), want2, "ctx-free behind a batch call")
        st = m.register_stats()
        assert st["points"] == cloud["n"] and st["scans"] == 2 and st["degenerate"] == 0
    c.close()
    m.close()


def test_a_register_call_moves_nothing_else(scvod, cloud):
    import torch
    m = _labelled_map(scvod, cloud["world"], np.full(cloud["n"], 3, np.uint8))
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=4096, max_scans=2)
    d = torch.from_numpy(cloud["xyzi"]).cuda()
    c.batch_process(d, np.asarray([0, 700, cloud["n"]], np.int32))
    p6 = np.stack([_start6(scvod, *STARTS[0])[0]] * 2)
    m.query_batch(c, p6, R_MAP, None, ("result",))
    before = (c.arena_bytes(), m.scratch_bytes(), m.query_scratch_bytes(), m.filter_scratch_bytes(), m.count(), *mr.sorted_records(m))
    assert m.register_scratch_bytes() == 0 and c.register_scratch_bytes() == 0  # nothing is allocated before the first call
    q = scvod.register_params_default(max_dist=R_MAP)
    pose, rec = m.register_batch(c, p6, params=q)
    batch = scvod.register_result(pose, rec)
    free = scvod.register_result(*m.register(d, [0, 700, cloud["n"]], p6, params=q))
    assert batch["matrices"].tobytes() == free["matrices"].tobytes() and batch["records"].tobytes() == free["records"].tobytes()
    assert (batch["records"]["status"] == scvod.REG_CONVERGED).all() and batch["poses"].shape == (2, 6)
    lab = torch.full((cloud["n"],), 6, dtype=torch.uint8, device="cuda")
    gated = scvod.register_result(*m.register_batch(c, p6, labels=lab, params=scvod.register_params_default(max_dist=R_MAP, use256=[1, 2, 3])))
    assert gated["records"]["skip_label"].tolist() == [700, cloud["n"] - 700] and (gated["records"]["status"] == scvod.REG_DEGENERATE).all()
    c.register_device(d, [0, cloud["n"]], torch.from_numpy(cloud["world"]).cuda(), p6[:1])
    st = m.register_stats()
    after = (c.arena_bytes(), m.scratch_bytes(), m.query_scratch_bytes(), m.filter_scratch_bytes(), m.count(), *mr.sorted_records(m))
    assert before[:5] == after[:5] and np.array_equal(before[5], after[5]) and np.array_equal(before[6], after[6])
    assert 0 < m.register_scratch_bytes() <= 4096 and c.register_scratch_bytes() > 0
    assert st["scans"] == 2 and st["degenerate"] == 2 and st["skipped"] == cloud["n"]
    assert c.register_stats()["converged"] == 1
    c.close()
    m.close()
