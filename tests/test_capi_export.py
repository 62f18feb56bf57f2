"""scvod_batch_point_labels / scvod_batch_export_points / scvod_batch_export_stats without a GPU: the symbols, the argument errors
that come before a device is looked for, and the numpy statement of the label table (tests/helpers/point_labels_ref.py) against the
oracle's own chain: fed the oracle's stage outputs, its labels must collapse to oracle_time_sequence's per-point labels everywhere.
Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import point_labels_ref as plr  # noqa: E402

NEW = ("scvod_batch_point_labels", "scvod_batch_export_points", "scvod_batch_export_stats")
CAR, OTHER = 2, 1


def test_symbols_declared_and_exported(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for k, name in enumerate(("DROPPED", "GROUND", "REJECTED", "UNCLUSTERED", "STATIC_OTHER", "STATIC_CAR", "DYNAMIC")):
        m = re.search(rf"#define SCVOD_PT_{name} (\d+)", hdr)
        assert m and int(m.group(1)) == k == getattr(scvod, "PT_" + name) == getattr(plr, "PT_" + name)
    assert len({getattr(scvod, "PT_" + n) for n in ("DROPPED", "GROUND", "REJECTED", "UNCLUSTERED", "STATIC_OTHER", "STATIC_CAR", "DYNAMIC")}) == 7


def test_argument_errors_come_before_the_device(scvod):
    """a NULL ctx is SCVOD_ERR_INVALID whatever else is passed: no device is touched"""
    lib = scvod.load_lib()
    buf = np.zeros(16, np.int64)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.scvod_batch_point_labels(None, p, 16, 0, None) == -1
    assert lib.scvod_batch_point_labels(None, p, -1, 0, None) == -1
    assert lib.scvod_batch_export_points(None, 0, None, None, p, None, None, 4, p, None) == -1
    assert lib.scvod_batch_export_points(None, 0, None, None, p, None, None, -1, p, None) == -1
    assert lib.scvod_batch_export_stats(None, p) == -1
    assert not buf.any()


def _oracle_stages(oracle, P, x, offs, poses):
    """the oracle's stages the way oracle_time_sequence chains them, kept per scan: Patchwork -> binning of the non-ground cloud ->
    clustering (canonical names) -> box rules -> the literal tracking chain"""
    res, names, types = [], [], []
    for s in range(len(offs) - 1):
        p = x[offs[s]:offs[s + 1]]
        pw = oracle.patchwork(P, p, 0)
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
    return res, types, dyn


def test_label_table_against_the_oracle_chain(scvod, oracle):
    import synth
    P = scvod.make_params("semantickitti")
    count = 6
    scans = [synth.make_scan(5, 300 + 5 * k, "K64") for k in range(count)]
    x = np.concatenate([sc[0].numpy() for sc in scans])
    offs = np.concatenate([[0], np.cumsum([len(sc[0]) for sc in scans])]).astype(np.int32)
    poses = np.asarray([sc[2] for sc in scans], np.float32)
    _, want, _ = oracle.time_sequence(P, x, offs, poses, car=CAR, other=OTHER)
    res, types, dyn = _oracle_stages(oracle, P, x, offs, poses)
    ao = np.concatenate([[0], np.cumsum([r["n_apri"] for r in res])])
    seen = set()
    for s, r in enumerate(res):
        d = dyn[ao[s]:ao[s + 1]]
        lab = plr.scan_labels(r["n_points"], r["cls"], r["ground_idx"], r["rejected_src"], r["apri_src"], types[s], d, car=CAR)
        assert np.array_equal(plr.collapse(lab), want[offs[s]:offs[s + 1]]), f"scan {s}"
        seen |= set(np.unique(lab).tolist())
        # the keep rule, flag by flag, is the map's: dropped never, dynamic unless ignored, the two lists unless switched off
        raw = plr.scan_labels(r["n_points"], r["cls"], r["ground_idx"], r["rejected_src"], r["apri_src"], types[s], None, car=CAR)
        assert not (raw == plr.PT_DYNAMIC).any() and np.array_equal(raw[lab != plr.PT_DYNAMIC], lab[lab != plr.PT_DYNAMIC])
        assert (raw[lab == plr.PT_DYNAMIC] == plr.PT_STATIC_CAR).all()
        for flags in (0, 1, 2, 3, 4):
            keep = plr.keep_of(lab if not flags & 4 else raw, flags)
            n = int((r["cls"] != 2).sum())
            n -= int((d == 1).sum()) if not flags & 4 else 0
            n -= len(r["ground_idx"]) if flags & 1 else 0
            n -= len(r["rejected_src"]) if flags & 2 else 0
            assert int(keep.sum()) == n
    assert seen == set(range(7)), f"the sequence does not exercise every label: {sorted(seen)}"
