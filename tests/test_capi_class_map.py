"""The labelled static map (SCVOD_MAP_KIND_LABELLED) without a GPU: the symbols in the header, the library and the shim, the argument
errors that are answered before a device is looked for, and the numpy statement tests/helpers/class_map_ref.py against answers worked
out by hand.  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import class_map_ref as cmr  # noqa: E402
import map_ref as mr  # noqa: E402

NEW = ("scvod_map_create_kind", "scvod_map_kind", "scvod_map_scratch_bytes", "scvod_map_accumulate_labelled",
       "scvod_batch_map_accumulate_classes", "scvod_map_points_labelled")
INVALID, NO_DEVICE = -1, -2


def test_symbols_declared_exported_and_in_the_shim(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("accumulate_labelled", "accumulate_classes", "points_labelled", "scratch_bytes"):
        assert callable(getattr(scvod.StaticMap, m))
    assert re.search(r"#define\s+SCVOD_MAP_KIND_PLAIN\s+0\b", hdr) and scvod.MAP_KIND_PLAIN == 0
    assert re.search(r"#define\s+SCVOD_MAP_KIND_LABELLED\s+1\b", hdr) and scvod.MAP_KIND_LABELLED == 1
    assert (scvod.MAP_PART_UNTRACKED, scvod.MAP_PART_TRACKED) == (cmr.PART_UNTRACKED, cmr.PART_TRACKED) == (8, 16)


def test_argument_errors_come_before_the_device(scvod):
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data_as(C.c_void_p)
    offs = np.array([0, 4], np.int32).ctypes.data_as(C.c_void_p)
    h = C.c_void_p(0x1234)
    # an unknown kind, and the argument errors scvod_map_create has always had, are INVALID whatever the machine holds
    for kind in (2, -1, 255):
        assert lib.scvod_map_create_kind(0, 4096, 0.2, kind, C.byref(h)) == INVALID
        assert h.value is None, "the handle of a refused create is NULL"
        h = C.c_void_p(0x1234)
    for kind in (0, 1):
        assert lib.scvod_map_create_kind(0, 4096, 0.2, kind, None) == INVALID
        assert lib.scvod_map_create_kind(0, 16, 0.2, kind, C.byref(h)) == INVALID
        assert lib.scvod_map_create_kind(0, 4096, 0.0, kind, C.byref(h)) == INVALID
        assert lib.scvod_map_create_kind(-1, 4096, 0.2, kind, C.byref(h)) == NO_DEVICE      # (a device that cannot exist)
    # a NULL map
    assert lib.scvod_map_kind(None) == INVALID
    assert lib.scvod_map_scratch_bytes(None) == 0
    n = C.c_int64(-7)
    assert lib.scvod_map_accumulate_labelled(None, p, p, offs, 1, None, None, None) == INVALID
    assert lib.scvod_batch_map_accumulate_classes(None, None, p, 0, 0, -1, None) == INVALID
    assert lib.scvod_batch_map_accumulate_classes(p, None, p, 0, 0, -1, None) == INVALID
    assert lib.scvod_map_points_labelled(None, p, p, p, 4, None, C.byref(n), None) == INVALID
    assert n.value == -7 and not buf.any()


def test_helper_packing_known_answers():
    # intensities -1, 0.99, 254.5, 255, 1e9 pack to 0, 0, 254, 255, 255
    assert cmr.qi8([-1.0, 0.99, 254.5, 255.0, 1e9]).tolist() == [0, 0, 254, 255, 255]
    plain = mr.pack_val(1, 2, 3, 0xABCD)
    v = cmr.labelled_vals([plain], [0x7F], [17.9])
    assert int(v[0]) == (1 << 48) | (2 << 32) | (3 << 16) | (0x7F << 8) | 17
    assert [int(q[0]) for q in cmr.unpack_labelled(v)] == [1, 2, 3, 0x7F, 17]
    # one cell (leaf 0.5, identity): equal offsets -> the smallest label; equal offset and label -> the smallest intensity; a smaller
    # label on a larger offset loses
    ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    p = np.array([[0.25, 0.25, 0.25, 9.0], [0.25, 0.25, 0.25, 3.0], [0.25, 0.25, 0.25, 200.0], [0.375, 0.25, 0.25, 0.0]], np.float32)
    k, v, ok, bad = cmr.encode_scan(ident, p, [5, 5, 4, 1], 0.5)
    assert ok.all() and not bad.any() and len(set(k.tolist())) == 1
    rk, rv = mr.reduce_records(k, v)
    assert [int(q[0]) for q in cmr.unpack_labelled(rv)] == [32768, 32768, 32768, 4, 200]
    rk, rv = mr.reduce_records(k[:2], v[:2])
    assert [int(q[0]) for q in cmr.unpack_labelled(rv)][3:] == [5, 3]
    # the keep table removes the winner: the next one takes the cell; all removed: no cell
    k, v, ok, _ = cmr.encode_scan(ident, p, [5, 5, 4, 1], 0.5, keep=cmr.table256([5, 1]))
    rk, rv = mr.reduce_records(k[ok], v[ok])
    assert [int(q[0]) for q in cmr.unpack_labelled(rv)][3:] == [5, 3]
    k, v, ok, _ = cmr.encode_scan(ident, p, [5, 5, 4, 1], 0.5, keep=cmr.table256([]))
    assert not ok.any()
    # the leading 48 bits are the plain map's
    pk, pv, _ = mr.encode_points(ident, p, 0.5)
    assert np.array_equal(v >> np.uint64(16), pv >> np.uint64(16))


def test_helper_batch_keep_tables():
    def kept(flags):
        return np.flatnonzero(cmr.batch_keep_table(flags)).tolist()
    assert kept(0) == [1, 2, 3, 4, 5, 7]
    assert kept(cmr.NO_GROUND) == [2, 3, 4, 5, 7]
    assert kept(cmr.NO_REJECTED) == [1, 3, 4, 5, 7]
    assert kept(cmr.NO_GROUND | cmr.NO_REJECTED) == [3, 4, 5, 7]
    assert kept(cmr.IGNORE_DYNAMIC) == [1, 2, 3, 4, 5, 6, 7]
    assert kept(cmr.PART_UNTRACKED) == [1, 2, 3, 4, 7]
    assert kept(cmr.PART_UNTRACKED | cmr.NO_GROUND) == [2, 3, 4, 7]
    assert kept(cmr.PART_TRACKED) == [5]
    assert kept(cmr.PART_TRACKED | cmr.IGNORE_DYNAMIC) == [5, 6]
    for f in (0, cmr.NO_GROUND, cmr.IGNORE_DYNAMIC, cmr.NO_REJECTED | cmr.IGNORE_DYNAMIC):
        both = cmr.batch_keep_table(f | cmr.PART_UNTRACKED) | cmr.batch_keep_table(f | cmr.PART_TRACKED)
        assert np.array_equal(both, cmr.batch_keep_table(f))
