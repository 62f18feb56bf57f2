"""The host-only part of the scan stacking (include/scvod.h: scvod_stack_offsets, scvod_pose_from_matrix).  Not gpu.

scvod_stack_offsets against the literal loop of tests/helpers/stack_ref.py for every n_in 0..40, interval 1..5, window 1 / 3 / 5 and both
flag values on ragged scans with empty ones; the reference bound with (3, 3) against `for (i = 0; i < n - 3; i += 3)`; argument errors;
count-only calls.  scvod_pose_from_matrix bit for bit against a small C++ restatement compiled here (tests/helpers/
pose_from_matrix_ref.cpp, -ffp-contract=off), the singular branch on crafted matrices, and the round trip through scvod_pose_matrix."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import stack_ref  # noqa: E402

INVALID, CAPACITY = -1, -4


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw(scvod, off, n_in, window, interval, flags, out=None, mid=None, cap=0, largest=None):
    return scvod.load_lib().scvod_stack_offsets(_vp(off), n_in, window, interval, flags, _vp(out), _vp(mid), cap, _vp(largest))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("pose_ref")), "libposeref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so,
                           os.path.join(HERE, "helpers", "pose_from_matrix_ref.cpp")])
    lib = C.CDLL(so)
    lib.ref_atan2f.restype = C.c_float
    lib.ref_atan2f.argtypes = [C.c_float, C.c_float]
    lib.ref_sqrtf.restype = C.c_float
    lib.ref_sqrtf.argtypes = [C.c_float]
    return lib


def _ref_pose(ref, M):
    m = np.ascontiguousarray(M, np.float32).reshape(12)
    out = np.zeros(6, np.float32)
    ref.ref_pose_from_matrix(_vp(m), _vp(out))
    return out


def _ragged_offsets(n_in, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 50, n_in)
    sizes[rng.random(n_in) < 0.25] = 0          # empty scans anywhere
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def test_offsets_against_the_literal_loop(scvod):
    for n_in in range(0, 41):
        off = _ragged_offsets(n_in, 1000 + n_in)
        for interval in range(1, 6):
            for window in (1, 3, 5):
                for bound in (False, True):
                    want_off, want_mid, want_largest = stack_ref.offsets(off, window, interval, bound)
                    n_out = len(want_mid)
                    got_off = np.full(n_out + 2, -7, np.int32)
                    got_mid = np.full(n_out + 1, -7, np.int32)
                    largest = np.full(1, -7, np.int32)
                    rc = _raw(scvod, off, n_in, window, interval, int(bound), got_off, got_mid, n_out, largest)
                    tag = (n_in, interval, window, bound)
                    assert rc == n_out, tag
                    assert np.array_equal(got_off[:n_out + 1], want_off) and got_off[n_out + 1] == -7, tag
                    assert np.array_equal(got_mid[:n_out], want_mid) and got_mid[n_out] == -7, tag
                    assert largest[0] == want_largest, tag
                    if n_in < window:
                        assert n_out == 0, tag
                    # the Python wrapper hands out the same
                    w_off, w_mid = scvod.stack_offsets(off, window, interval, bound)
                    assert np.array_equal(w_off, want_off) and np.array_equal(w_mid, want_mid), tag


def test_reference_bound_is_the_stackers_loop(scvod):
    """window 3, interval 3: exactly the iterations of `for (i = 0; i < n - 3; i += 3)`, n >= 3: a multiple of 3 loses its last group"""
    for n in range(3, 41):
        off = np.arange(n + 1, dtype=np.int32) * 5
        iters = list(range(0, n - 3, 3))
        _, mid = scvod.stack_offsets(off, 3, 3, reference_bound=True)
        assert list(mid) == [i + 1 for i in iters], n
        _, mid_all = scvod.stack_offsets(off, 3, 3)
        assert len(mid_all) == n // 3
        assert len(mid_all) - len(mid) == (1 if n % 3 == 0 else 0), n


def test_count_only_calls(scvod):
    off = _ragged_offsets(17, 5)
    want_off, want_mid, want_largest = stack_ref.offsets(off, 3, 2)
    n_out = len(want_mid)
    assert _raw(scvod, off, 17, 3, 2, 0) == n_out
    assert _raw(scvod, None, 17, 3, 2, 0) == n_out                      # the count needs no offsets
    largest = np.zeros(1, np.int32)
    assert _raw(scvod, off, 17, 3, 2, 0, largest=largest) == n_out and largest[0] == want_largest
    mid = np.zeros(n_out, np.int32)
    assert _raw(scvod, None, 17, 3, 2, 0, mid=mid, cap=n_out) == n_out and np.array_equal(mid, want_mid)
    out = np.zeros(n_out + 1, np.int32)
    assert _raw(scvod, off, 17, 3, 2, 0, out=out, cap=n_out) == n_out and np.array_equal(out, want_off)
    assert _raw(scvod, off, 0, 3, 3, 0) == 0
    assert _raw(scvod, off, 2, 3, 3, 0) == 0 and _raw(scvod, off, 2, 3, 3, 1) == 0


def test_argument_errors(scvod):
    off = _ragged_offsets(12, 9)
    for window in (-1, 0, 2, 4, 8, 10, 11):
        assert _raw(scvod, off, 12, window, 3, 0) == INVALID, window
    assert _raw(scvod, off, 12, 9, 3, 0) == 2
    for interval in (0, -1):
        assert _raw(scvod, off, 12, 3, interval, 0) == INVALID
    for flags in (2, 3, -1):
        assert _raw(scvod, off, 12, 3, 3, flags) == INVALID
    assert _raw(scvod, off, -1, 3, 3, 0) == INVALID
    bad = off.copy()
    bad[5] = bad[4] - 1
    assert _raw(scvod, bad, 12, 3, 3, 0) == INVALID
    out = np.full(8, -7, np.int32)
    assert _raw(scvod, None, 12, 3, 3, 0, out=out, cap=7) == INVALID            # sizes without offsets
    assert _raw(scvod, None, 12, 3, 3, 0, largest=out) == INVALID
    mid = np.full(8, -7, np.int32)
    assert _raw(scvod, off, 12, 3, 3, 0, out=out, cap=3) == CAPACITY and (out == -7).all()
    assert _raw(scvod, off, 12, 3, 3, 0, mid=mid, cap=3) == CAPACITY and (mid == -7).all()
    assert _raw(scvod, off, 12, 3, 3, 0, out=out, mid=mid, cap=4) == 4
    # overlapping windows can stack more points than int32 offsets hold
    big = (np.arange(6, dtype=np.int64) * 400_000_000).astype(np.int32)
    assert _raw(scvod, big, 5, 3, 3, 0, largest=np.zeros(1, np.int32)) == 1
    assert _raw(scvod, big, 5, 3, 1, 0, largest=np.zeros(1, np.int32)) == CAPACITY
    with pytest.raises(scvod.ScvodError):
        scvod.stack_offsets(off, 4, 3)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _seeded_poses(n, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 6), np.float32)
    p[:, :3] = rng.uniform(-500, 500, (n, 3))
    p[:, 3] = rng.uniform(-np.pi, np.pi, n)
    p[:, 4] = rng.uniform(-1.5, 1.5, n)       # |pitch| below 1.5: away from the singular branch
    p[:, 5] = rng.uniform(-np.pi, np.pi, n)
    return p


def test_pose_from_matrix_equals_the_restatement(scvod, ref):
    rng = np.random.default_rng(77)
    mats = [scvod.pose_matrix(p) for p in _seeded_poses(300, 3)]
    mats += list(rng.uniform(-2, 2, (200, 12)).astype(np.float32))          # not rotations at all: the function is plain arithmetic
    mats += [np.asarray([1, 0, 0, 1, 0, 1, 0, 2, 0, 0, 1, 3], np.float32), np.zeros(12, np.float32)]
    for M in mats:
        assert np.array_equal(_bits(scvod.pose_from_matrix(M)), _bits(_ref_pose(ref, M)))
    assert np.array_equal(scvod.pose_from_matrix(mats[-2]), np.asarray([1, 2, 3, 0, 0, 0], np.float32))
    # a 3x4 array is taken row by row
    assert np.array_equal(_bits(scvod.pose_from_matrix(mats[0].reshape(3, 4))), _bits(scvod.pose_from_matrix(mats[0])))


def test_pose_from_matrix_singular_branch(scvod, ref):
    """sy < 1e-6 (compared in double): roll from the second and third column, yaw exactly 0"""
    def M(r00, r10, r20, r11, r12):
        return np.asarray([r00, 0.3, 0.4, 7, r10, r11, r12, 8, r20, 0.6, 0.7, 9], np.float32)
    for r00, r10, singular in ((0.0, 0.0, True), (9e-7, 0.0, True), (0.0, -9.9e-7, True), (6e-7, 6e-7, True), (1.1e-6, 0.0, False),
                               (8e-7, 8e-7, False), (0.0, 1.0, False)):
        for r20 in (-1.0, 1.0, 0.25):
            m = M(r00, r10, r20, 0.8, -0.6)
            got = scvod.pose_from_matrix(m)
            assert np.array_equal(_bits(got), _bits(_ref_pose(ref, m))), (r00, r10, r20)
            sy = ref.ref_sqrtf(C.c_float(np.float32(r00) * np.float32(r00) + np.float32(r10) * np.float32(r10)))
            assert (float(sy) < 1e-6) == singular
            assert np.array_equal(got[:3], np.asarray([7, 8, 9], np.float32))
            if singular:
                assert _bits(got[5:6])[0] == 0                                                    # +0.0
                assert got[3] == np.float32(ref.ref_atan2f(C.c_float(0.6), C.c_float(0.8)))       # atan2(-r12, r11)
            else:
                assert got[3] == np.float32(ref.ref_atan2f(C.c_float(0.6), C.c_float(0.7)))       # atan2(r21, r22)
                assert got[5] == np.float32(ref.ref_atan2f(C.c_float(r10), C.c_float(r00)))
            assert got[4] == np.float32(ref.ref_atan2f(C.c_float(-r20), sy))
    # pitch of +-90 degrees exactly: the matrix scvod_pose_matrix cannot produce in fp32, written by hand
    down = np.asarray([0, 0, 1, 0, 0, 1, 0, 0, -1, 0, 0, 0], np.float32)
    got = scvod.pose_from_matrix(down)
    assert got[5] == 0 and got[4] == np.float32(np.pi / 2) and got[3] == np.float32(ref.ref_atan2f(C.c_float(-0.0), C.c_float(1.0)))


def test_pose_round_trip(scvod, ref):
    """scvod_pose_matrix -> scvod_pose_from_matrix on 400 seeded poses with |pitch| < 1.5, against the fp64 evaluation of the same atan2
    expressions on the same float32 matrix entries (sy in fp64 too).  The allowed distance is twice the worst distance of this image's
    atan2f from the fp64 atan2 on the arguments the extraction really passes (the fp32 sy among them), measured by the test itself before
    it asserts: 2.247e-07 rad on this image (about an ulp of an angle in [2, 4)), so the bound is 4.493e-07 rad; the worst distance of the
    round trip measured with it was 2.247e-07 rad."""
    poses = _seeded_poses(400, 11)
    worst_atan2f, worst = 0.0, 0.0
    dist = []
    for p in poses:
        M = scvod.pose_matrix(p)
        got = scvod.pose_from_matrix(M)
        assert np.array_equal(_bits(got[:3]), _bits(p[:3]))
        m = M.astype(np.float64)
        sy64 = np.sqrt(m[0] * m[0] + m[4] * m[4])
        want = np.asarray([np.arctan2(m[9], m[10]), np.arctan2(-m[8], sy64), np.arctan2(m[4], m[0])])
        sy32 = np.float32(ref.ref_sqrtf(C.c_float(M[0] * M[0] + M[4] * M[4])))
        for (a, b) in ((M[9], M[10]), (-M[8], sy32), (M[4], M[0])):
            f = float(ref.ref_atan2f(C.c_float(a), C.c_float(b)))
            worst_atan2f = max(worst_atan2f, abs(f - float(np.arctan2(np.float64(a), np.float64(b)))))
        d = np.abs(got[3:].astype(np.float64) - want)
        dist.append(d)
        worst = max(worst, float(d.max()))
        # and the angles come back: |pitch| < 1.5 keeps the extraction on the branch that inverts scvod_pose_matrix.  An entry of M
        # carries a few fp32 roundings (6e-8 each) and roll / yaw divide them by cos(pitch) >= cos(1.5) = 0.07: below 1e-5, 2e-5 allowed
        back = np.abs(got[3:].astype(np.float64) - p[3:].astype(np.float64))
        back = np.minimum(back, 2 * np.pi - back)
        assert (back < 2e-5).all(), (p, got)
    print(f"atan2f vs fp64 worst {worst_atan2f:.3e} rad, round trip worst {worst:.3e} rad, allowed {2 * worst_atan2f:.3e} rad")
    assert worst_atan2f > 0
    assert worst <= 2 * worst_atan2f
