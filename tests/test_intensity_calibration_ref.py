"""SSC::intensityCalibrationByCurvature (src/ssc.cpp:98-153) on the CPU (tests/helpers/intensity_calibration_ref.cpp): known answers,
the spec function calibrated_intensity_f32 against a plain fp32 transcription of ssc.cpp:140-151, and the (d^2, position) order of
the neighbour lists on duplicated points and on a lattice.  Not gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F03 = np.float32(0.3)


def build_ic(out_dir):
    src = os.path.join(ROOT, "tests", "helpers", "intensity_calibration_ref.cpp")
    so = os.path.join(str(out_dir), "libicref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", so, src])
    lib = C.CDLL(so)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    lib.ic_run.argtypes = [fp, C.c_int, C.c_int, C.c_float, fp, fp, ip, C.POINTER(C.c_long), C.c_int]
    lib.ic_spec.restype = C.c_float
    lib.ic_spec.argtypes = [C.c_float, C.c_float, fp, fp]
    return lib


STAT_KEYS = ("points", "clamped_before", "cos_floored", "capped_after", "nan_normals")


def run(lib, xyzi, k=10, max_int=200.0, threads=16):
    """one non-ground cloud [n, 4]: (normal_curv [n, 4], intensity [n], neighbours [n, k_eff], stats)"""
    xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    n = len(xyzi)
    keff = min(k, n)
    nc = np.zeros((max(n, 1), 4), np.float32)
    inten = np.zeros(max(n, 1), np.float32)
    nbr = np.zeros((max(n, 1), max(keff, 1)), np.int32)
    st = (C.c_long * 8)()
    fp = C.POINTER(C.c_float)
    got = lib.ic_run(xyzi.ctypes.data_as(fp), n, k, C.c_float(max_int), nc.ctypes.data_as(fp), inten.ctypes.data_as(fp),
                     nbr.ctypes.data_as(C.POINTER(C.c_int)), st, threads)
    assert got == keff
    return nc[:n], inten[:n], nbr[:n, :keff], dict(zip(STAT_KEYS, [int(v) for v in st[:5]]))


@pytest.fixture(scope="module")
def ic(tmp_path_factory):
    return build_ic(tmp_path_factory.mktemp("icref"))


def _plane(origin, u, v, m=5, step=0.25, intensity=40.0):
    """(2m+1)^2 lattice points origin + a u + b v; the first row of the result is the origin"""
    a, b = np.meshgrid(np.arange(-m, m + 1), np.arange(-m, m + 1), indexing="ij")
    ab = np.stack([a.ravel(), b.ravel()], -1).astype(np.float64) * step
    order = np.argsort((ab ** 2).sum(1), kind="stable")
    p = np.asarray(origin, np.float64) + ab[order, :1] * np.asarray(u, np.float64) + ab[order, 1:] * np.asarray(v, np.float64)
    return np.concatenate([p, np.full((len(p), 1), intensity)], 1).astype(np.float32)


def test_head_on_plane_keeps_the_intensity(ic):
    x = _plane([8, 0, 0], [0, 1, 0], [0, 0, 1])
    nc, inten, _, st = run(ic, x, max_int=200.0)
    assert abs(abs(nc[0, 0]) - 1.0) <= 1e-6 and inten[0] == np.float32(40.0)
    assert st["points"] == len(x) and st["nan_normals"] == 0 and st["clamped_before"] == 0


def test_plane_at_sixty_degrees_doubles_it(ic):
    # the normal (1, 0, 0) and the ray to (4, 0, 4 sqrt 3) enclose 60 degrees: cos = 1/2
    z = 4.0 * np.sqrt(3.0)
    x = _plane([4, 0, z], [0, 1, 0], [0, 0, 1])
    _, inten, _, _ = run(ic, x, max_int=200.0)
    assert abs(float(inten[0]) - 80.0) <= 80.0 * 4 * 2.0 ** -24   # fp32: the rounding of z, of the norm and of the quotient


def test_grazing_plane_hits_the_floor(ic):
    x = _plane([0.5, 30, 0], [0, 1, 0], [0, 0, 1])    # cos about 1/60
    _, inten, _, st = run(ic, x, max_int=200.0)
    assert inten[0] == np.float32(40.0) / F03 and st["cos_floored"] >= 1
    in_plane = _plane([0, 30, 0], [0, 1, 0], [0, 0, 1])  # the ray lies in the plane: cos = 0
    _, inten, _, _ = run(ic, in_plane, max_int=200.0)
    assert inten[0] == np.float32(40.0) / F03


def test_max_intensity_clamps_before_and_after(ic):
    x = _plane([8, 0, 0], [0, 1, 0], [0, 0, 1], intensity=300.0)
    _, inten, _, st = run(ic, x, max_int=255.0)
    assert np.all(inten == np.float32(255.0)) and st["clamped_before"] == len(x)
    y = _plane([0.5, 30, 0], [0, 1, 0], [0, 0, 1], intensity=100.0)   # 100 / 0.3 > 255
    _, inten, _, st = run(ic, y, max_int=255.0)
    assert inten[0] == np.float32(255.0) and st["capped_after"] >= 1 and st["clamped_before"] == 0


def test_fewer_than_three_points_give_nan(ic):
    for n in (1, 2):
        x = np.asarray([[1, 2, 3, 10], [2, 2, 3, 20]], np.float32)[:n]
        nc, inten, nbr, st = run(ic, x)
        assert np.isnan(nc).all() and np.isnan(inten).all() and st["nan_normals"] == n and nbr.shape == (n, n)
    nc, inten, nbr, st = run(ic, np.zeros((0, 4), np.float32))
    assert len(inten) == 0 and st["points"] == 0


def test_fewer_points_than_k_use_them_all(ic):
    x = _plane([8, 0, 0], [0, 1, 0], [0, 0, 1], m=1)   # 9 points, k = 16
    nc, inten, nbr, _ = run(ic, x, k=16)
    assert nbr.shape == (9, 9) and all(sorted(r) == list(range(9)) for r in nbr.tolist())
    assert not np.isnan(nc[:, :3]).any() and inten[0] == np.float32(40.0)   # (the first point is the one seen head-on)


def _literal(inten, mx, n, p):
    """ssc.cpp:101-105, 140-151 in plain fp32 (numpy float32 operations round once each; Eigen's 3-term sums as a0 + (a1 + a2))"""
    f = np.float32
    i0 = np.where(inten > mx, mx, inten).astype(f)
    dot = (n[:, 0] * p[:, 0] + (n[:, 1] * p[:, 1] + n[:, 2] * p[:, 2])).astype(f)
    nn = np.sqrt((n[:, 0] * n[:, 0] + (n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])).astype(f)).astype(f)
    pn = np.sqrt((p[:, 0] * p[:, 0] + (p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2])).astype(f)).astype(f)
    with np.errstate(all="ignore"):
        c = np.abs((dot / (nn * pn).astype(f)).astype(f))
        c = np.where(c < F03, F03, c).astype(f)
        v = (i0 / c).astype(f)
    return np.where(v > mx, mx, v).astype(f)


def test_spec_function_equals_the_plain_transcription(ic):
    rng = np.random.default_rng(11)
    m = 20000
    n = rng.normal(size=(m, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True).astype(np.float32)
    p = (rng.normal(size=(m, 3)) * rng.choice([0.5, 5.0, 50.0], (m, 1))).astype(np.float32)
    p[::7] -= (n[::7] * (p[::7] * n[::7]).sum(1, keepdims=True)).astype(np.float32)   # nearly grazing
    n[::501] = np.nan
    n[1::503] = 0.0
    inten = rng.uniform(0, 300, m).astype(np.float32)
    mx = np.float32(255.0)
    want = _literal(inten, mx, n, p)
    fp = C.POINTER(C.c_float)
    got = np.asarray([ic.ic_spec(C.c_float(inten[i]), C.c_float(mx), n[i].ctypes.data_as(fp), p[i].ctypes.data_as(fp)) for i in range(m)], np.float32)
    assert np.array_equal(got.view(np.uint32) & np.where(np.isnan(got), 0x7FC00000, 0xFFFFFFFF).astype(np.uint32),
                          want.view(np.uint32) & np.where(np.isnan(want), 0x7FC00000, 0xFFFFFFFF).astype(np.uint32))
    assert np.isnan(got).sum() >= m // 503 and (got == mx).any() and (want < mx).any()


def _order(x, k):
    d = x[:, None, :3].astype(np.float32) - x[None, :, :3].astype(np.float32)
    d2 = ((d[..., 0] * d[..., 0]).astype(np.float32) + (d[..., 1] * d[..., 1]).astype(np.float32)).astype(np.float32)
    d2 = (d2 + (d[..., 2] * d[..., 2]).astype(np.float32)).astype(np.float32).T   # [i, j] = d^2(j - i) as the helper forms it
    return np.stack([np.lexsort((np.arange(len(x)), d2[i]))[:k] for i in range(len(x))])


def test_ties_follow_distance_then_position(ic):
    rng = np.random.default_rng(5)
    base = rng.uniform(-2, 2, (40, 3)).astype(np.float32)
    dups = np.concatenate([base, base[rng.integers(0, 40, 80)]])
    dups = np.concatenate([dups[rng.permutation(len(dups))], np.ones((len(dups), 1), np.float32)], 1)
    a, b, c = np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij")
    lattice = np.stack([a.ravel() + 3, b.ravel(), c.ravel(), np.ones(a.size)], -1).astype(np.float32)
    lattice = lattice[rng.permutation(len(lattice))]
    for x in (dups, lattice):
        for k in (3, 10, 16):
            _, _, nbr, _ = run(ic, x, k=k)
            assert np.array_equal(nbr, _order(x, k))
    nc, inten, _, st = run(ic, np.tile(np.asarray([[1, 2, 3, 9]], np.float32), (30, 1)))
    assert np.isnan(nc[:, :3]).all() and np.isnan(inten).all() and st["nan_normals"] == 30
