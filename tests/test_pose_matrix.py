"""scvod_pose_matrix, scvod_pose_delta and oracle_pose_delta against fp64 arithmetic the project did not write: the rotation is the
product of the three ELEMENTARY rotations, R = Rz(yaw) @ Ry(pitch) @ Rx(roll) (what pcl::getTransformation means through Eigen's
AngleAxis product), not the closed form the library and the oracle both restate.  A wrong Euler order or a wrong sign in both
places passes every library-against-oracle comparison; it does not pass here.  Host functions only: not gpu."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import map_ref as mr  # noqa: E402

SEED = 20240917
N_POSES = 20000
# per rotation entry: every magnitude is at most 1; up to three sinf / cosf values of at most 1 ulp each, up to three rounded
# products, one rounded sum
ROT_TOL = 8 * 2.0 ** -24
# pose delta, scaled by 1 + |t_pre| + |t_next|: twice the worst scaled error of oracle_pose_delta against inv(M_next) @ M_pre in
# fp64 on the poses of SEED = 20240917 (measured on the CPU: 1.0169e-07 = 1.71 * 2**-24, the cancellation of two translations
# of up to 1000 m in fp32; the library gives the same figure, being bit-identical to the oracle)
DELTA_MEASURED = 1.0169e-07
DELTA_TOL = 2 * DELTA_MEASURED


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def poses():
    rng = np.random.default_rng(SEED)
    n = N_POSES
    p = np.zeros((n, 6), np.float64)
    p[:, :3] = rng.uniform(-1000.0, 1000.0, (n, 3))
    p[:, 3:5] = rng.uniform(-0.2, 0.2, (n, 2))
    wide = rng.random(n) < 0.2
    p[wide, 3:5] = rng.uniform(-1.5, 1.5, (int(wide.sum()), 2))
    p[:, 5] = -rng.uniform(-np.pi, np.pi, n)            # (-pi, pi]
    special = np.array([np.pi, -np.pi, np.pi / 2, -np.pi / 2, 0.0])
    p[:5 * 40, 5] = np.tile(special, 40)                # the special yaws with random rolls, pitches and translations
    p[200:205, 3:5] = 0.0                               # ... and alone
    p[200:205, 5] = special
    p[205:210] = 0.0
    p[205:210, :3] = [[0, 0, 0], [1000, -1000, 1000], [-1000, 1000, -1000], [0.1, 0, 0], [0, 0, -0.0]]
    return p.astype(np.float32)


@pytest.fixture(scope="module")
def pose_pairs(poses):
    """(pre, next): next = pre moved by 0 to 3 m and by 0 to 0.1 rad per angle, as a sequence moves"""
    rng = np.random.default_rng(SEED + 1)
    n = len(poses)
    d = rng.normal(size=(n, 3))
    d *= (rng.uniform(0.0, 3.0, n) / np.linalg.norm(d, axis=1))[:, None]
    a = rng.uniform(0.0, 0.1, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    step = np.concatenate([d, a], axis=1)
    step[::50] = 0.0                                    # a sensor that stands still
    step[1::50, 3:] = 0.0                               # pure translation
    step[2::50, :3] = 0.0                               # pure rotation
    nxt = (poses.astype(np.float64) + step).astype(np.float32)
    return poses, nxt


@pytest.fixture(scope="module")
def matrices(scvod, poses):
    lib = scvod.load_lib()
    T = np.zeros((len(poses), 12), np.float32)
    for i in range(len(poses)):
        lib.scvod_pose_matrix(_p(poses[i]), _p(T[i]))
    return T.reshape(-1, 3, 4)


def test_translation_column_is_the_input_bit_for_bit(poses, matrices):
    assert np.array_equal(matrices[:, :, 3].view(np.uint32), poses[:, :3].view(np.uint32))


def test_rotation_equals_the_fp64_product_of_elementary_rotations(poses, matrices):
    ref = mr.poses64(poses)
    err = np.abs(matrices[:, :, :3].astype(np.float64) - ref[:, :3, :3])
    worst = float(err.max())
    i = int(np.argmax(err.max(axis=(1, 2))))
    print(f"worst rotation entry error {worst:.4e} = {worst * 2 ** 24:.3f} * 2**-24 at pose {poses[i].tolist()}")
    assert worst <= ROT_TOL
    # the vectorised reference is the plain one
    for k in (0, 7, 203, len(poses) - 1):
        assert np.array_equal(ref[k], mr.pose64(poses[k]))


def test_rotation_is_orthonormal_and_proper(matrices):
    R = matrices[:, :, :3].astype(np.float64)
    G = np.transpose(R, (0, 2, 1)) @ R
    # entries off by at most e = ROT_TOL, rows and columns of norm 1: |sum (a + da)(b + db) - sum a b| <= 2 sqrt(3) e + 3 e^2 < 4 e
    assert float(np.abs(G - np.eye(3)).max()) <= 4 * ROT_TOL
    det = np.linalg.det(R)
    # multilinear in three columns of norm 1, each off by at most sqrt(3) e: |det - 1| <= 3 sqrt(3) e + O(e^2) < 6 e
    assert (det > 0).all() and float(np.abs(det - 1.0).max()) <= 6 * ROT_TOL


def _matrix(scvod, pose):
    return scvod.pose_matrix(np.asarray(pose, np.float32)).reshape(3, 4).astype(np.float64)


def test_hand_checkable_rotations(scvod):
    h = np.float32(np.pi / 2)
    M = _matrix(scvod, [0, 0, 0, 0, 0, h])                      # yaw: x -> y, y -> -x
    assert np.abs(M[:, :3] @ [1, 0, 0] - [0, 1, 0]).max() <= ROT_TOL
    assert np.abs(M[:, :3] @ [0, 1, 0] - [-1, 0, 0]).max() <= ROT_TOL
    assert np.abs(M[:, :3] @ [0, 0, 1] - [0, 0, 1]).max() <= ROT_TOL
    M = _matrix(scvod, [0, 0, 0, 0, h, 0])                      # pitch about y: x -> -z (nose down), z -> x
    assert np.abs(M[:, :3] @ [1, 0, 0] - [0, 0, -1]).max() <= ROT_TOL
    assert np.abs(M[:, :3] @ [0, 0, 1] - [1, 0, 0]).max() <= ROT_TOL
    assert np.abs(M[:, :3] @ [0, 1, 0] - [0, 1, 0]).max() <= ROT_TOL
    M = _matrix(scvod, [0, 0, 0, h, 0, 0])                      # roll about x: y -> z, z -> -y
    assert np.abs(M[:, :3] @ [0, 1, 0] - [0, 0, 1]).max() <= ROT_TOL
    assert np.abs(M[:, :3] @ [0, 0, 1] - [0, -1, 0]).max() <= ROT_TOL
    assert np.abs(M[:, :3] @ [1, 0, 0] - [1, 0, 0]).max() <= ROT_TOL
    a = 0.3
    c, s = np.cos(np.float64(np.float32(a))), np.sin(np.float64(np.float32(a)))
    assert np.abs(_matrix(scvod, [0, 0, 0, 0, 0, a])[:, :3] - [[c, -s, 0], [s, c, 0], [0, 0, 1]]).max() <= ROT_TOL
    assert np.abs(_matrix(scvod, [0, 0, 0, 0, a, 0])[:, :3] - [[c, 0, s], [0, 1, 0], [-s, 0, c]]).max() <= ROT_TOL
    assert np.abs(_matrix(scvod, [0, 0, 0, a, 0, 0])[:, :3] - [[1, 0, 0], [0, c, -s], [0, s, c]]).max() <= ROT_TOL
    # the order: yaw is applied last (about the world's z), roll first (about the body's x)
    M = _matrix(scvod, [0, 0, 0, h, 0, h])
    assert np.abs(M[:, :3] @ [0, 1, 0] - [0, 0, 1]).max() <= ROT_TOL    # roll takes y to z, yaw leaves z alone
    assert np.abs(M[:, :3] @ [0, 0, 1] - [1, 0, 0]).max() <= ROT_TOL    # roll takes z to -y, yaw takes -y to x


def _scaled_errors(fn, pre, nxt):
    want = np.linalg.inv(mr.poses64(nxt)) @ mr.poses64(pre)
    got = np.stack([fn(pre[i], nxt[i]) for i in range(len(pre))]).reshape(-1, 3, 4).astype(np.float64)
    scale = 1.0 + np.linalg.norm(pre[:, :3].astype(np.float64), axis=1) + np.linalg.norm(nxt[:, :3].astype(np.float64), axis=1)
    return np.abs(got - want[:, :3, :]).max(axis=(1, 2)) / scale, got


def test_pose_delta_of_library_and_oracle_against_fp64(scvod, oracle, pose_pairs):
    pre, nxt = pose_pairs
    lib = scvod.load_lib()

    def library(a, b):
        T = np.zeros(12, np.float32)
        lib.scvod_pose_delta(_p(a), _p(b), _p(T))
        return T

    e_or, T_or = _scaled_errors(oracle.pose_delta, pre, nxt)
    e_lib, T_lib = _scaled_errors(library, pre, nxt)
    print(f"worst scaled pose-delta error: oracle {e_or.max():.4e}, library {e_lib.max():.4e} (seed {SEED})")
    assert float(e_or.max()) <= DELTA_TOL
    assert float(e_lib.max()) <= DELTA_TOL
    # the library against the oracle stays bit-exact
    assert np.array_equal(T_lib.astype(np.float32).view(np.uint32), T_or.astype(np.float32).view(np.uint32))
    # a sensor that stands still: the identity, to the same scaled bound
    still = np.flatnonzero((pre == nxt).all(axis=1))
    assert len(still) >= N_POSES // 50
    eye = np.eye(4)[:3]
    scale = 1.0 + 2.0 * np.linalg.norm(pre[still, :3].astype(np.float64), axis=1)
    assert float((np.abs(T_lib[still] - eye).max(axis=(1, 2)) / scale).max()) <= DELTA_TOL
