"""The pose refinement's step on the CPU (include/scvod.h: scvod_map_register, scvod_register_device).  Not gpu.

The C++ helper (tests/helpers/register_ref.cpp: the library's reg_* functions of scvod_math.h in a sequential loop with an exhaustive
search) against the independent numpy statement of tests/helpers/register_ref.py, which does not read that header: int64 sums equal,
poses and records bit for bit -- every operation of the step is an IEEE-basic one in a stated order, which numpy and Python floats
mirror, so no tolerance is needed.  Then hand-worked cases, the crafted cloud of the device tests, and the refusals that need no
device (scvod_register_check)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dr-using-scv-od_amd", "pyshim"))
import register_ref as rr  # noqa: E402
import scvod_py  # noqa: E402

F = np.float32
IDENTITY = np.asarray([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
S = 1 << 20


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rr.build(tmp_path_factory.mktemp("registerref"))


def _same(a, b):
    assert np.array_equal(a["sums"], b["sums"]), (a["sums"] - b["sums"])
    assert np.array_equal(a["match0"], b["match0"])
    assert a["pose"].tobytes() == b["pose"].tobytes(), np.abs(a["pose"] - b["pose"]).max()
    assert a["records"].tobytes() == b["records"].tobytes(), (a["records"], b["records"])


@pytest.mark.parametrize("mode", [rr.POINT, rr.PLANE])
@pytest.mark.parametrize("iters", [1, 2, 10])
def test_helper_equals_numpy_on_the_crafted_cloud(ref, mode, iters):
    xyzi, world, normals = rr.corner_cloud()
    p = rr.params(mode=mode, max_iterations=iters, max_dist=0.2)
    args = (xyzi, [0, len(xyzi)], rr.start_matrix(), world, p)
    h = rr.run(ref, *args, tgt_nrm=normals)
    _same(h, rr.run_numpy(*args, tgt_nrm=normals))
    assert np.array_equal(h["match0"], np.arange(len(xyzi))), "a point of the crafted cloud does not match its own image"
    assert h["records"]["n_corr"][0] == len(xyzi) == 1452


@pytest.mark.parametrize("mode", [rr.POINT, rr.PLANE])
@pytest.mark.parametrize("start", [(0.003, 0.04), (0.002, 0.03), (0.001, 0.05)])
def test_crafted_cloud_converges(ref, mode, start):
    """Every point matches its own image from iteration 0, so the step solves a fixed least-squares problem: it converges in a few
    iterations.  The bound on the final error comes from the inputs, not from the code: a target coordinate near 128 m is an fp32
    with half an ulp (3.8e-6 m) of rounding, 6.6e-6 m per point in norm; the fit over 1452 such points cannot be off by more than the
    largest of them plus the fixed-point rounding (2^-21 per term), so 1e-5 m holds with room."""
    xyzi, world, normals = rr.corner_cloud()
    T0 = rr.start_matrix(*start)
    h = rr.run(ref, xyzi, [0, len(xyzi)], T0, world, rr.params(mode=mode, max_dist=0.2), tgt_nrm=normals)
    assert np.array_equal(h["match0"], np.arange(len(xyzi)))
    rec = h["records"][0]
    e0, e1 = rr.pose_error(T0, xyzi), rr.pose_error(h["pose"][0], xyzi)
    print(f"mode {mode} start {start}: {rec['iterations']} iterations, error {e0:.3e} -> {e1:.3e} m, status {rec['status']}")
    assert rec["status"] == rr.CONVERGED and 2 <= rec["iterations"] <= 5
    assert e1 < 1e-5 < e0
    R = h["pose"][0].reshape(3, 4)[:, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6  # as orthonormal as the fp32 start


def test_helper_equals_numpy_on_a_rough_cloud(ref):
    """three scans (one empty) with NaN points, points beyond max_range, gated labels, bad normals, ties and misses, both modes"""
    rng = np.random.default_rng(5)
    tgt = (rng.integers(-12, 12, (700, 3)) * 0.25).astype(F)  # a lattice with repeated points: ties go to the lowest index
    nrm = rng.normal(size=(700, 3)).astype(F)
    nrm[::17] = 0
    nrm[5::31, 1] = np.nan
    src = np.concatenate([tgt[rng.integers(0, 700, 900)] + rng.normal(scale=0.05, size=(900, 3)).astype(F), np.ones((900, 1), F)], 1).astype(F)
    src[::41, 0] = np.nan
    src[7::53] *= F(40)
    labels = rng.integers(0, 8, 900).astype(np.uint8)
    use = np.ones(256, np.uint8)
    use[6] = 0
    pose = np.stack([IDENTITY, IDENTITY, rr.start_matrix()])
    pose[0, 3] = 0.03
    for mode in (rr.POINT, rr.PLANE):
        p = rr.params(mode=mode, max_iterations=4, max_dist=0.3, max_range=9.0, use256=use, min_corr=6)
        args = (src, [0, 500, 500, 900], pose, tgt, p)
        h = rr.run(ref, *args, labels=labels, tgt_nrm=nrm)
        _same(h, rr.run_numpy(*args, labels=labels, tgt_nrm=nrm))
        r = h["records"]
        assert r["skip_nan"].sum() > 0 and r["skip_range"].sum() > 0 and r["skip_label"].sum() > 0 and r["skip_no_corr"].sum() > 0
        assert (r["skip_normal"].sum() > 0) == (mode == rr.PLANE)
        assert r["status"][1] == rr.DEGENERATE and h["pose"][1].tobytes() == IDENTITY.astype(np.float64).tobytes()


def test_map_tie_goes_to_the_smaller_key(ref):
    tgt = np.asarray([[1, 0, 0], [-1, 0, 0]], F)
    src = np.asarray([[0, 0, 0, 1]], F)
    for keys, want in (([7, 3], 1), ([3, 7], 0)):
        args = (src, [0, 1], IDENTITY, tgt, rr.params(max_dist=1.5, min_corr=6))
        h = rr.run(ref, *args, tgt_key=np.asarray(keys, np.uint64))
        assert h["match0"][0] == want
        _same(h, rr.run_numpy(*args, tgt_key=np.asarray(keys, np.uint64)))
    assert rr.run(ref, src, [0, 1], IDENTITY, tgt, rr.params(max_dist=1.5))["match0"][0] == 0  # a cloud: the lowest index


def test_one_correspondence_by_hand(ref):
    """p = (1, 2, 3) under the identity, q = (1.5, 2, 3): r = p - q = (-0.5, 0, 0); J = [ -[p]x , I ] row by row"""
    h = rr.run(ref, [[1, 2, 3, 0]], [0, 1], IDENTITY, [[1.5, 2, 3]], rr.params(max_dist=0.75, min_corr=6))
    J = np.asarray([[0, 3, -2, 1, 0, 0], [-3, 0, 1, 0, 1, 0], [2, -1, 0, 0, 0, 1]], np.int64)
    r = np.asarray([-0.5, 0, 0])
    H = J.T @ J
    want = [int(H[i, j]) * S for i in range(6) for j in range(i, 6)] + [int(v * S) for v in J.T @ r] + [S // 4, 1, 0, 0, 0, 0, 0]
    assert h["sums"][0].tolist() == want
    rec = h["records"][0]
    assert rec["status"] == rr.DEGENERATE and rec["iterations"] == 1 and rec["n_corr"] == 1 and rec["sum_r2"] == 0.25
    assert h["pose"][0].tobytes() == IDENTITY.astype(np.float64).tobytes()  # fewer than min_corr: the pose is kept


def test_pure_translation_by_hand(ref):
    """a 3 x 3 x 3 lattice against itself moved by (1/16, -1/32, 1/64): the problem is linear in v and omega = 0 solves it, so ONE step
    lands on the translation (all numbers are dyadic: the sums are exact) and the second reports convergence"""
    g = np.arange(3, dtype=np.float64) - 1.0
    p = np.stack([c.reshape(-1) for c in np.meshgrid(g, g, g, indexing="ij")], 1)
    t = np.asarray([1 / 16, -1 / 32, 1 / 64])
    src = np.concatenate([p, np.zeros((27, 1))], 1)
    h1 = rr.run(ref, src, [0, 27], IDENTITY, p + t, rr.params(max_iterations=1, max_dist=0.2, min_corr=6))
    M = h1["pose"][0].reshape(3, 4)
    assert np.abs(M[:, :3] - np.eye(3)).max() < 1e-15 and np.abs(M[:, 3] - t).max() < 1e-15
    assert h1["records"]["status"][0] == rr.MAX_ITERATIONS and h1["records"]["n_corr"][0] == 27
    assert h1["sums"][0][27] == int(27 * (t @ t) * S)  # sum r^2 of the first accumulation
    h2 = rr.run(ref, src, [0, 27], IDENTITY, p + t, rr.params(max_dist=0.2, min_corr=6))
    assert h2["records"]["status"][0] == rr.CONVERGED and h2["records"]["iterations"][0] == 2
    _same(h2, rr.run_numpy(src, [0, 27], IDENTITY, p + t, rr.params(max_dist=0.2, min_corr=6)))


def test_point_mode_sums_that_the_kernel_derives(ref):
    """k_reg_accumulate folds 16 of the 28 point-mode sums and derives the rest: the omega-v block is [p]x summed (each of x, y, z once
    with either sign; the rounding is odd), three of its entries and the v-v off-diagonal are 0, the v-v diagonal is the count * 2^20"""
    xyzi, world, _ = rr.corner_cloud()
    src = xyzi.copy()
    src[:, :3] += np.random.default_rng(1).normal(scale=0.03, size=(len(src), 3)).astype(F)
    s = rr.run(ref, src, [0, len(src)], rr.start_matrix(), world, rr.params(max_iterations=1, max_dist=0.2))["sums"][0].tolist()
    assert s[4] == -s[8] != 0 and s[5] == -s[12] != 0 and s[13] == -s[10] != 0
    assert [s[i] for i in (3, 9, 14, 16, 17, 19)] == [0] * 6 and s[15] == s[18] == s[20] == s[28] * S and s[28] > 1000


def test_degenerate_plane_by_hand(ref):
    """a single plane in plane mode leaves three directions (two translations, one rotation) free: rank 3, DEGENERATE, pose kept"""
    g = np.arange(8, dtype=np.float64) * 0.5
    u, v = (c.reshape(-1) for c in np.meshgrid(g, g, indexing="ij"))
    p = np.stack([u, v, np.zeros_like(u)], 1)
    n = np.tile([0.0, 0.0, 1.0], (64, 1))
    src = np.concatenate([p, np.zeros((64, 1))], 1)
    args = (src, [0, 64], IDENTITY, p + [0, 0, 0.0625], rr.params(mode=rr.PLANE, max_dist=0.2, min_corr=6))
    h = rr.run(ref, *args, tgt_nrm=n)
    assert h["records"]["status"][0] == rr.DEGENERATE and h["records"]["n_corr"][0] == 64
    assert h["pose"][0].tobytes() == IDENTITY.astype(np.float64).tobytes()
    _same(h, rr.run_numpy(*args, tgt_nrm=n))
    # the same points in point mode are well posed
    assert rr.run(ref, *args[:4], rr.params(max_dist=0.2, min_corr=6))["records"]["status"][0] == rr.CONVERGED


def test_defaults_and_sizes():
    p = scvod_py.register_params_default()
    assert C.sizeof(scvod_py.RegisterParams) == 64 and scvod_py.REGISTER_RECORD_DTYPE.itemsize == 64
    assert scvod_py.REGISTER_RECORD_DTYPE == rr.RECORD_DTYPE
    assert (p.max_iterations, p.min_corr, p.mode, p.reserved, p.use256) == (10, 30, scvod_py.REG_POINT, 0, None)
    assert (p.max_dist, p.max_range) == (F(0.19), F(80))
    assert (p.eps_rot, p.eps_trans, p.lam, p.pivot_eps) == (1e-6, 1e-5, 0.0, 1e-9)
    q = scvod_py.register_params_default(use256=[1, 2, 3])
    assert q.use256 and q._use_bytes.sum() == 3


def test_refusals_that_need_no_device():
    d = scvod_py.register_params_default
    ok = scvod_py.register_check
    assert ok(None, 0.2) == 0 and ok(d(), 0.0) == 0 and ok(d(max_iterations=64, min_corr=6), 0.2, d_src_xyzi=4096) == 0
    for bad in (dict(max_iterations=0), dict(max_iterations=65), dict(min_corr=5), dict(mode=2), dict(reserved=1), dict(max_dist=0.0),
                dict(max_dist=float("nan")), dict(max_dist=300.0), dict(max_range=0.0), dict(eps_rot=-1.0), dict(eps_trans=float("nan")),
                dict(lam=-0.5), dict(pivot_eps=-1e-3)):
        assert ok(d(**bad), 0.0) == -1, bad
    assert ok(d(max_dist=float(F(0.99) * F(0.2))), 0.2) == 0
    assert ok(d(max_dist=0.1981), 0.2) == -1        # above 0.99 * leaf
    assert ok(d(max_dist=0.1981), 0.0) == 0         # a cloud target has no leaf
    assert ok(d(mode=scvod_py.REG_PLANE), 0.2, has_normals=True) == -1  # the map is point-to-point only
    assert ok(d(mode=scvod_py.REG_PLANE), 0.0, has_normals=False) == -1
    assert ok(d(mode=scvod_py.REG_PLANE), 0.0, has_normals=True) == 0
    assert ok(d(), 0.2, d_src_xyzi=4096 + 8) == -1  # not 16-byte aligned
    assert ok(d(max_range=float("inf")), 0.2) == 0  # no range gate
    lib = scvod_py.load_lib()
    assert lib.scvod_map_register(None, None, None, 0, None, None, None, None, None, None, None) == -1
    assert lib.scvod_register_device(None, None, None, 0, None, None, None, None, 0, None, None, None, None) == -1
    assert lib.scvod_map_register_scratch_bytes(None) == 0 and lib.scvod_register_scratch_bytes(None) == 0
