"""numpy statement of the labelled static map (include/scvod.h, SCVOD_MAP_KIND_LABELLED) -- test infrastructure only, built on
tests/helpers/map_ref.py, which it imports and does not change.

A record of the labelled kind is the plain record with its low 16 bits replaced: val = (plain & ~0xFFFF) | label << 8 | qi8, qi8 =
(int)clamp(intensity, 0, 255) in fp32.  The map is `map_ref.reduce_records` of the kept points' records: per cell the smallest value."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_ref as mr  # noqa: E402

_U = np.uint64
NO_GROUND, NO_REJECTED, IGNORE_DYNAMIC, PART_UNTRACKED, PART_TRACKED = 1, 2, 4, 8, 16
PT_DROPPED, PT_GROUND, PT_REJECTED, PT_UNCLUSTERED, PT_OTHER, PT_CAR, PT_DYNAMIC, PT_BUILDING = range(8)


def table256(labels=None):
    """a keep / select table: None -> every label, otherwise the listed labels"""
    t = np.zeros(256, np.uint8)
    if labels is None:
        t[:] = 1
    else:
        t[np.asarray(list(labels), np.int64)] = 1
    return t


def qi8(intensity):
    """(int)clamp(intensity, 0.f, 255.f): truncation, no scaling"""
    with np.errstate(invalid="ignore"):
        return np.clip(np.asarray(intensity, np.float32), np.float32(0), np.float32(255)).astype(np.int64)


def labelled_vals(plain_vals, labels, intensity):
    lab = np.asarray(labels, np.uint8).astype(np.uint64)
    return (np.asarray(plain_vals, np.uint64) & ~_U(0xFFFF)) | (lab << _U(8)) | qi8(intensity).astype(np.uint64)


def unpack_labelled(vals):
    """qx, qy, qz, label, qi8"""
    v = np.asarray(vals, np.uint64)
    return [((v >> _U(s)) & _U(m)).astype(np.int64) for s, m in ((48, 0xFFFF), (32, 0xFFFF), (16, 0xFFFF), (8, 0xFF), (0, 0xFF))]


def encode_scan(T, p, labels, leaf, keep=None):
    """(keys, vals, kept and in range, kept but out of range) of one scan's points p [n, 4] with their label bytes under the row-major
    3x4 matrix T; keep: a 256-entry table or None"""
    k, v, ok = mr.encode_points(T, p, leaf)
    labels = np.asarray(labels, np.uint8)
    kept = np.ones(len(labels), bool) if keep is None else np.asarray(keep)[labels] != 0
    return k, labelled_vals(v, labels, np.asarray(p, np.float32)[:, 3]), kept & ok, kept & ~ok


def definition(scvod_py, x, labels, offs, poses, leaf, keep=None, scans=None):
    """the labelled map of the scans (all, or the listed ones) of the cloud x [n, 4] / labels [n] cut by offs: (keys, vals, points left
    out because they are out of range or NaN); poses [n_scans][6] or None for the zero pose"""
    ks, vs, out = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint64)], 0
    for s in (range(len(offs) - 1) if scans is None else scans):
        a, b = int(offs[s]), int(offs[s + 1])
        T = scvod_py.pose_matrix(np.zeros(6, np.float32) if poses is None else poses[s])
        k, v, ok, bad = encode_scan(T, x[a:b], labels[a:b], leaf, keep)
        ks.append(k[ok])
        vs.append(v[ok])
        out += int(bad.sum())
    k, v = mr.reduce_records(np.concatenate(ks), np.concatenate(vs))
    return k, v, out


def batch_keep_table(flags):
    """the keep table scvod_batch_map_accumulate_classes states for its flags"""
    t = np.zeros(256, np.uint8)
    if not flags & PART_TRACKED:
        t[[PT_UNCLUSTERED, PT_OTHER, PT_BUILDING]] = 1
        t[PT_GROUND] = 0 if flags & NO_GROUND else 1
        t[PT_REJECTED] = 0 if flags & NO_REJECTED else 1
    if not flags & PART_UNTRACKED:
        t[PT_CAR] = 1
        t[PT_DYNAMIC] = 1 if flags & IGNORE_DYNAMIC else 0
    return t


def decode_points(keys, vals, leaf):
    """fp64 statement of scvod_map_points_labelled: map_ref.decode_points' xyz, the label byte, the intensity = the low 8 bits"""
    xyz, _ = mr.decode_points(keys, vals, leaf)
    q = unpack_labelled(vals)
    return xyz, q[3].astype(np.uint8), q[4].astype(np.float64)
