"""Reference statement of scvod_batch_objects (include/scvod.h) in numpy -- test infrastructure only.

Per scan, from the arrays a caller can fetch (or the oracle's own stage outputs): the apri records (coordinates and voxel_idx), the
canonical cluster name of every apri point, the segmentation's type (-1 erased, `car`, anything else), optionally the class byte
(1 tree / other, 2 car, 3 building), the tracking byte pt_dyn and the state of every car cluster.  The table lists the clusters that
are not erased in ascending name; members are in ascending apri index.

The arithmetic that has to be the library's (the polar angle of the box corners) and the C++ form of the sequential centre sum come
from objects_ref.cpp, built by `build`."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OBJECT_DTYPE = np.dtype([("scan", "i4"), ("name", "i4"), ("n_points", "i4"), ("n_voxels", "i4"), ("box_min", "f4", 3),
                         ("box_max", "f4", 3), ("center", "f4", 3), ("angle_diff", "f4"), ("cls", "i1"), ("state", "i1"),
                         ("dynamic", "u1"), ("reserved", "u1"), ("point_begin", "i4")])
OBJ_NO_TRACK = 1
DYN_DYNAMIC = 1


def build(out_dir):
    src = os.path.join(ROOT, "tests", "helpers", "objects_ref.cpp")
    so = os.path.join(str(out_dir), "libobjref.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.obj_center.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.obj_center.restype = None
    lib.obj_angle_diff.argtypes = [C.c_float] * 4
    lib.obj_angle_diff.restype = C.c_float
    return lib


def _ord(f):
    """order-preserving integer image of a float (the library's float_sort_key): -0 orders below +0"""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _unord(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def cpp_center(lib, xyz):
    xyz = np.ascontiguousarray(xyz, np.float32)
    out = np.zeros(3, np.float32)
    lib.obj_center(xyz.ctypes.data_as(C.c_void_p), len(xyz), out.ctypes.data_as(C.c_void_p))
    return out


def seq_center(xyz):
    """three sequential float32 sums in the order given (np.add.accumulate adds one element after the other), divided by (float)n"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    return (np.add.accumulate(xyz, axis=0, dtype=np.float32)[-1] / np.float32(len(xyz))).astype(np.float32)


def cluster_boxes(apri, pt_cluster):
    """every cluster of the scan, the erased ones included: (names ascending, member apri indices grouped by name in ascending index,
    first slot of each group [+ end], box_min [k, 3], box_max [k, 3], n_voxels)"""
    cl = np.asarray(pt_cluster, np.int64)
    order = np.argsort(cl, kind="stable")
    names, first, counts = np.unique(cl[order], return_index=True, return_counts=True)
    begin = np.concatenate([first, [len(cl)]]).astype(np.int64)
    if len(names) == 0:
        z = np.zeros((0, 3), np.float32)
        return names, order, begin, z, z, np.zeros(0, np.int64)
    xyz = np.stack([apri["x"], apri["y"], apri["z"]], axis=1).astype(np.float32)[order]
    keys = _ord(xyz)
    mn = _unord(np.minimum.reduceat(keys, first, axis=0))
    mx = _unord(np.maximum.reduceat(keys, first, axis=0))
    # occupy_voxels after sampleVec: the distinct voxel_idx among the cluster's points (ssc.cpp:365, 383)
    pairs = np.unique(np.stack([cl, np.asarray(apri["voxel_idx"], np.int64)], axis=1), axis=0)
    nv_names, nvox = np.unique(pairs[:, 0], return_counts=True)
    assert np.array_equal(nv_names, names)
    return names, order, begin, mn, mx, nvox


def box_types(P, mn, mx, counts, car=2, other=1):
    """refineClusterByBoundingBox (ssc.cpp:437-467) and the box part of recognize (ssc.cpp:849-872) on boxes and point counts:
    -1 erased, car, other"""
    mn, mx = np.asarray(mn, np.float32), np.asarray(mx, np.float32)
    diff_z = (mx[:, 2] - mn[:, 2]).astype(np.float32)
    erased = (mn[:, 2] > np.float32(0.0)) | (np.asarray(counts) < int(P.toBeClass)) | (diff_z.astype(np.float64) < 0.2)
    square = (mx[:, 0] - mn[:, 0]).astype(np.float32).astype(np.float64) * (mx[:, 1] - mn[:, 1]).astype(np.float32).astype(np.float64)
    car_sq, min_z, max_z = float(np.float32(P.car_square)), float(np.float32(P.min_z)), float(np.float32(P.max_z))
    is_car = ~(square > car_sq) & (mn[:, 2].astype(np.float64) < min_z) & (square < car_sq) & (mx[:, 2].astype(np.float64) < max_z)
    return np.where(erased, -1, np.where(is_car, car, other)).astype(np.int32)


def scan_objects(lib, s, apri, pt_cluster, types, classes=None, pt_dyn=None, car_state=None, car=2):
    """the objects of one scan: (records with point_begin counted from 0 inside the scan, member apri indices, per apri point the
    scan-local object index or -1).  classes: per apri point 1 / 2 / 3 (None: 2 for car, 1 otherwise); pt_dyn None and car_state None:
    the SCVOD_OBJ_NO_TRACK form.  car_state: {canonical name: Cluster::state} of the car clusters"""
    types = np.asarray(types)
    n = len(types)
    names, order, begin, mn, mx, nvox = cluster_boxes(apri, pt_cluster)
    keep = np.asarray([types[order[begin[k]]] != -1 for k in range(len(names))], bool)
    rec = np.zeros(int(keep.sum()), OBJECT_DTYPE)
    members = []
    point_obj = np.full(n, -1, np.int32)
    xyz = np.stack([apri["x"], apri["y"], apri["z"]], axis=1).astype(np.float32) if n else np.zeros((0, 3), np.float32)
    o, slot = 0, 0
    for k in np.nonzero(keep)[0]:
        m = order[begin[k]:begin[k + 1]]
        assert m[0] == names[k] and (np.diff(m) > 0).all(), "a canonical name is the smallest apri index of its cluster"
        assert (types[m] == types[m[0]]).all(), "the type is a property of the cluster"
        r = rec[o]
        r["scan"], r["name"], r["n_points"], r["n_voxels"] = s, names[k], len(m), nvox[k]
        r["box_min"], r["box_max"] = mn[k], mx[k]
        r["center"] = seq_center(xyz[m])
        r["angle_diff"] = lib.obj_angle_diff(float(mn[k][0]), float(mn[k][1]), float(mx[k][0]), float(mx[k][1]))
        r["cls"] = (2 if types[m[0]] == car else 1) if classes is None else classes[m[0]]
        r["state"] = -1
        if car_state is not None and types[m[0]] == car:
            r["state"] = car_state[int(names[k])]
        if pt_dyn is not None:
            d = np.asarray(pt_dyn)[m] == DYN_DYNAMIC
            assert d.all() or not d.any(), "the tracking byte is a property of the cluster"
            r["dynamic"] = int(d[0])
        r["point_begin"] = slot
        point_obj[m] = o
        members.append(m)
        slot += len(m)
        o += 1
    return rec, (np.concatenate(members).astype(np.int32) if members else np.zeros(0, np.int32)), point_obj


def batch_table(per_scan):
    """[(records, members as INPUT indices, per input point the scan-local object or -1)] per scan -> the batch's table: records with
    point_begin counted over the batch, offsets [n_scans + 1], member list, per input point the object index in the table"""
    recs, mems, pobj, offs, slot = [], [], [], [0], 0
    for rec, m_src, po in per_scan:
        rec = rec.copy()
        rec["point_begin"] += slot
        slot += len(m_src)
        po = np.where(po >= 0, po + offs[-1], -1).astype(np.int32)
        offs.append(offs[-1] + len(rec))
        recs.append(rec)
        mems.append(m_src)
        pobj.append(po)
    cat = lambda a, dt: np.concatenate(a) if a else np.zeros(0, dt)  # noqa: E731
    return cat(recs, OBJECT_DTYPE), np.asarray(offs, np.int32), cat(mems, np.int32).astype(np.int32), cat(pobj, np.int32)


def to_input(n_points, apri_src, members, point_obj_apri):
    """apri indices -> INPUT indices of the scan: the member list as apri_src, the per-point object scattered to the input points"""
    apri_src = np.asarray(apri_src, np.int64)
    po = np.full(n_points, -1, np.int32)
    po[apri_src] = point_obj_apri
    return apri_src[members].astype(np.int32), po
