"""scvod_batch_objects / scvod_batch_objects_stats / scvod_batch_objects_scratch_bytes without a GPU: the symbols and the record's
layout, the argument errors that come before a device is looked for, and the numpy statement of the object table
(tests/helpers/objects_ref.py) against the oracle: fed the oracle's stage outputs, its boxes and counts must reproduce
oracle.cluster_types through the reference's rules, its dynamic flags the chain's per-point bytes.  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import objects_ref as obr  # noqa: E402

NEW = ("scvod_batch_objects", "scvod_batch_objects_stats", "scvod_batch_objects_scratch_bytes")
CAR, OTHER = 2, 1
FIELDS = (("scan", 0), ("name", 4), ("n_points", 8), ("n_voxels", 12), ("box_min", 16), ("box_max", 28), ("center", 40),
          ("angle_diff", 52), ("cls", 56), ("state", 57), ("dynamic", 58), ("reserved", 59), ("point_begin", 60))


@pytest.fixture(scope="module")
def objlib(tmp_path_factory):
    return obr.build(tmp_path_factory.mktemp("objref"))


def test_symbols_declared_and_exported_and_the_record_layout(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    m = re.search(r"#define SCVOD_OBJ_NO_TRACK (\d+)", hdr)
    assert m and int(m.group(1)) == 1 == scvod.OBJ_NO_TRACK == obr.OBJ_NO_TRACK
    assert "typedef struct scvod_object {" in hdr and "cc_box_square" in hdr
    assert C.sizeof(scvod.Object) == 64 == scvod.OBJECT_DTYPE.itemsize == obr.OBJECT_DTYPE.itemsize
    for name, off in FIELDS:
        assert getattr(scvod.Object, name).offset == off, name
        assert scvod.OBJECT_DTYPE.fields[name][1] == off == obr.OBJECT_DTYPE.fields[name][1], name
    assert scvod.OBJECT_DTYPE == obr.OBJECT_DTYPE
    # the struct of the header, field by field in this order
    body = hdr[hdr.index("typedef struct scvod_object {"):hdr.index("} scvod_object;")]
    assert re.findall(r"^\s*(?:u?int\d+_t|float)\s+(\w+)", body, re.M) == [f for f, _ in FIELDS]


def test_argument_errors_come_before_the_device(scvod):
    """a NULL ctx is SCVOD_ERR_INVALID whatever else is passed -- a negative capacity, an unknown flag bit: no device is touched and
    nothing is written"""
    lib = scvod.load_lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.scvod_batch_objects(None, 0, p, 4, p, p, 4, p, None) == -1
    assert lib.scvod_batch_objects(None, 0, p, -1, p, p, 4, p, None) == -1
    assert lib.scvod_batch_objects(None, 0, p, 4, p, p, -1, p, None) == -1
    assert lib.scvod_batch_objects(None, 2, p, 4, p, None, 0, None, None) == -1
    assert lib.scvod_batch_objects(None, scvod.OBJ_NO_TRACK, None, 0, p, None, 0, None, None) == -1
    assert lib.scvod_batch_objects_stats(None, p) == -1
    assert lib.scvod_batch_objects_scratch_bytes(None) == 0
    assert not buf.any()


def oracle_stages(oracle, P, x, offs, poses, sort_mode=0):
    """the oracle's stages the way oracle_time_sequence chains them, kept per scan (as tests/test_capi_export.py feeds them):
    Patchwork -> binning of the non-ground cloud -> clustering (canonical names) -> box rules -> the literal tracking chain.
    sort_mode is Patchwork's (oracle/patchwork_oracle.cpp): 0 is the reference's std::sort on z, whose order among points of equal z
    inside a patch is implementation-defined; 1 breaks those ties by input index, the canonical order the device implements.  The
    order of the non-ground cloud is the apri order, so the member ORDER inside an object (and nothing else of the table on these
    scans) depends on it: a comparison with the device's member list needs 1"""
    res, names, types = [], [], []
    for s in range(len(offs) - 1):
        p = x[offs[s]:offs[s + 1]]
        pw = oracle.patchwork(P, p, sort_mode)
        b = oracle.bin(P, p[pw["nonground_idx"]], True)
        cl, _, _ = oracle.cluster(P, b["apri"])
        _, first = np.unique(cl, return_index=True)
        canon = np.zeros(int(cl.max()) + 1 if len(cl) else 1, np.int32)
        canon[cl[first]] = first
        cl = canon[cl] if len(cl) else cl
        ty = oracle.cluster_types(P, b["apri"], cl, CAR, OTHER)
        res.append(dict(n_points=len(p), cls=pw["cls"], ground_idx=pw["ground_idx"], apri=b["apri"], n_apri=len(b["apri"]),
                        apri_src=pw["nonground_idx"][b["src"]], rejected_src=pw["nonground_idx"][b["rejected"]]))
        names.append(cl)
        types.append(ty)
    dyn, _ = oracle.reference_chain(P, res, names, types, poses)
    ao = np.concatenate([[0], np.cumsum([r["n_apri"] for r in res])])
    return res, names, types, [dyn[ao[s]:ao[s + 1]] for s in range(len(res))]


def oracle_table(objlib, res, names, types, dyn):
    """the batch's table from the oracle's stage outputs alone (no cluster states: the oracle's chain reports per-point bytes)"""
    per_scan = []
    for s, r in enumerate(res):
        rec, mem, po = obr.scan_objects(objlib, s, r["apri"], names[s], types[s], pt_dyn=dyn[s], car=CAR)
        per_scan.append((rec,) + obr.to_input(r["n_points"], r["apri_src"], mem, po))
    return obr.batch_table(per_scan)


def six_scans(scvod):
    import synth
    P = scvod.make_params("semantickitti")
    scans = [synth.make_scan(5, 300 + 5 * k, "K64") for k in range(6)]
    x = np.concatenate([sc[0].numpy() for sc in scans])
    offs = np.concatenate([[0], np.cumsum([len(sc[0]) for sc in scans])]).astype(np.int32)
    poses = np.asarray([sc[2] for sc in scans], np.float32)
    return P, x, offs, poses


def test_helper_against_the_oracle(scvod, oracle, objlib):
    P, x, offs, poses = six_scans(scvod)
    res, names, types, dyn = oracle_stages(oracle, P, x, offs, poses)
    table, t_offs, members, pobj = oracle_table(objlib, res, names, types, dyn)
    scans_with_erased = 0
    for s, r in enumerate(res):
        apri, cl, ty, d = r["apri"], names[s], types[s], dyn[s]
        rec = table[t_offs[s]:t_offs[s + 1]]
        roots = np.nonzero(cl == np.arange(len(cl)))[0]
        # the listed clusters are exactly the non-erased ones, in ascending name
        assert np.array_equal(rec["name"], roots[ty[roots] != -1]), f"scan {s}"
        assert (rec["scan"] == s).all() and (rec["reserved"] == 0).all() and (rec["state"] == -1).all()
        scans_with_erased += int((ty[roots] == -1).any())
        # the reference's rules on the helper's own boxes and counts reproduce the oracle's types, the erased clusters included
        all_names, order, begin, mn, mx, nvox = obr.cluster_boxes(apri, cl)
        assert np.array_equal(all_names, roots)
        want = obr.box_types(P, mn, mx, np.diff(begin), car=CAR, other=OTHER)
        assert np.array_equal(want, ty[roots]), f"scan {s}: the helper's boxes do not give the oracle's types"
        kept = ty[roots] != -1
        assert np.array_equal(rec["box_min"].view(np.uint32), mn[kept].view(np.uint32))
        assert np.array_equal(rec["box_max"].view(np.uint32), mx[kept].view(np.uint32))
        assert np.array_equal(rec["n_points"], np.diff(begin)[kept]) and np.array_equal(rec["n_voxels"], nvox[kept])
        assert np.array_equal(rec["cls"], np.where(ty[rec["name"]] == CAR, 2, 1))
        # dynamic agrees with the chain's per-point bytes, which are uniform inside every cluster (scan_objects asserts that)
        assert np.array_equal(rec["dynamic"], (d[rec["name"]] == 1).astype(np.uint8))
        po_a = pobj[offs[s]:offs[s + 1]][r["apri_src"]]
        assert np.array_equal(d == 1, (po_a >= 0) & (table["dynamic"][np.maximum(po_a, 0)] == 1))
        assert int(rec["n_points"].sum()) == int((ty != -1).sum())
        assert ((rec["n_voxels"] >= 1) & (rec["n_voxels"] <= rec["n_points"])).all()
        # centre: inside the box; the helper's sequential float32 sum is the C++ loop's, bit for bit
        assert (rec["center"] >= rec["box_min"]).all() and (rec["center"] <= rec["box_max"]).all()
        xyz = np.stack([apri["x"], apri["y"], apri["z"]], axis=1)
        inv = np.full(r["n_points"], -1, np.int64)
        inv[r["apri_src"]] = np.arange(len(apri))
        for k, o in enumerate(rec):
            m = members[o["point_begin"]:o["point_begin"] + o["n_points"]]
            idx = inv[m]
            assert idx[0] == o["name"] and (np.diff(idx) > 0).all()
            assert np.array_equal(obr.cpp_center(objlib, xyz[idx]).view(np.uint32), o["center"].view(np.uint32)), f"scan {s} object {k}"
            assert np.array_equal(x[offs[s]:offs[s + 1]][m][:, :3].view(np.uint32), xyz[idx].view(np.uint32))
        assert (rec["angle_diff"] >= 0).all() and (rec["angle_diff"] < 360).all()
        # the per-point object composed with the table is the cluster name; the points of no object are the others
        po = pobj[offs[s]:offs[s + 1]]
        assert np.array_equal(table["name"][po[r["apri_src"]][ty != -1]], cl[ty != -1]) and (po[r["apri_src"]][ty == -1] == -1).all()
        assert int((po >= 0).sum()) == int((ty != -1).sum())
    assert np.array_equal(table["point_begin"], np.concatenate([[0], np.cumsum(table["n_points"])[:-1]]))
    # the condition the cases rest on
    assert (table["cls"] == 2).any() and (table["cls"] == 1).any() and (table["dynamic"] == 1).any(), "no car, no other or no dynamic object"
    assert scans_with_erased > 0, "no scan has an erased cluster"
    assert (table["dynamic"][table["cls"] != 2] == 0).all()
