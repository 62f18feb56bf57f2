"""Reference statement of the cloud vote (include/scvod.h: scvod_cloud_visibility_device) -- test infrastructure only.

`run` is the brute-force C++ loop of cloud_visibility_ref.cpp: the library's arithmetic (scvod_math.h) for every (point, scan) pair, no
sort and no skipped scan.  `matrices` builds the world -> viewer matrices as the library does (scvod_pose_delta, host only).  The grid
tuple and the pair classes are visibility_ref's."""
import ctypes as C
import os
import subprocess

import numpy as np

from visibility_ref import AGREE, EMPTY, OCCLUDED, OUTSIDE, ROOT, THROUGH, grid_of  # noqa: F401

STATS = ("points", "finite", "seen_through", "keep", "untested", "through", "agree", "occluded", "empty")


def build(out_dir):
    src = os.path.join(ROOT, "tests", "helpers", "cloud_visibility_ref.cpp")
    so = os.path.join(str(out_dir), "libcloudvisibilityref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.cvis_ref.argtypes = [C.c_void_p] * 3 + [C.c_longlong] + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 6
    lib.cvis_ref.restype = None
    return lib


def matrices(scvod, poses, n_scans=None):
    """[n_scans, 12]: scvod_pose_delta(zero pose, pose_s) -- trans_s^-1, host only; poses None: the zero pose for n_scans scans"""
    lib = scvod.load_lib()
    p = np.zeros((int(n_scans), 6), np.float32) if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
    zero = np.zeros(6, np.float32)
    T = np.zeros((len(p), 12), np.float32)
    for s in range(len(p)):
        b = np.ascontiguousarray(p[s])
        lib.scvod_pose_delta(zero.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), T[s].ctypes.data_as(C.c_void_p))
    return T


def params_tuple(prm):
    return (np.asarray([prm.halo, prm.min_through, prm.vote_num, prm.vote_den], np.int32),
            np.asarray([prm.gap_abs, prm.gap_rel, prm.max_range], np.float32))


def run(lib, scvod, P, xyzi, images, T, prm, pair_classes=False):
    """the vote of the world-frame records `xyzi` [n, 4] against `images` [n_scans, A, S] with the matrices `T` [n_scans, 12]:
    dict(votes uint16 [n, 4], verdict uint8 [n], stats int64 [9], and with pair_classes: pair_class uint8 [n_scans, n])"""
    x = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    g9, dims3 = grid_of(scvod, P)
    S, A = int(dims3[1]), int(dims3[2])
    T = np.ascontiguousarray(T, np.float32).reshape(-1, 12)
    n_scans = len(T)
    img = np.ascontiguousarray(images, np.float32).reshape(n_scans, A * S)
    ip, fp = params_tuple(prm)
    n = len(x)
    votes = np.zeros((n, 4), np.uint16)
    verdict = np.zeros(n, np.uint8)
    stats = np.zeros(9, np.int64)
    pc = np.zeros((n_scans, n), np.uint8) if pair_classes else None

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)
    lib.cvis_ref(ptr(g9), ptr(dims3), ptr(x), n, ptr(img), ptr(T), n_scans, ptr(ip), ptr(fp), ptr(votes), ptr(verdict), ptr(stats), ptr(pc))
    out = dict(votes=votes, verdict=verdict, stats=stats)
    if pair_classes:
        out["pair_class"] = pc
    return out
