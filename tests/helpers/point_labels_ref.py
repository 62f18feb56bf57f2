"""Reference statement of scvod_batch_point_labels / scvod_batch_export_points (include/scvod.h) in numpy -- test infrastructure only.

Per scan, from the arrays a caller can fetch (or the oracle's own stage outputs): which of the three clouds an INPUT point went to
(`ground_idx`, `rejected_src`, `apri_src`; a point in none of them was dropped by Patchwork, `cls == 2`), the segmentation's type of
every apri point's cluster (-1 erased, `car`, anything else) and the tracking byte `pt_dyn` (0 static, 1 dynamic, 2 in no cluster)."""
import numpy as np

PT_DROPPED, PT_GROUND, PT_REJECTED, PT_UNCLUSTERED, PT_STATIC_OTHER, PT_STATIC_CAR, PT_DYNAMIC = range(7)
MAP_NO_GROUND, MAP_NO_REJECTED, MAP_IGNORE_DYNAMIC = 1, 2, 4
DYN_DYNAMIC = 1
# the oracle's four values (pyshim/quality.py): 0 static, 1 dynamic, 2 in no cluster, 3 dropped
COLLAPSE = np.array([3, 0, 0, 2, 0, 0, 1], np.uint8)


def scan_labels(n_points, cls, ground_idx, rejected_src, apri_src, types, pt_dyn=None, car=2):
    """the label table.  pt_dyn None: the SCVOD_MAP_IGNORE_DYNAMIC form (no point is labelled DYNAMIC)"""
    lab = np.full(n_points, PT_DROPPED, np.uint8)
    lab[np.asarray(ground_idx, np.int64)] = PT_GROUND
    lab[np.asarray(rejected_src, np.int64)] = PT_REJECTED
    types = np.asarray(types)
    a = np.where(types == -1, PT_UNCLUSTERED, np.where(types == car, PT_STATIC_CAR, PT_STATIC_OTHER)).astype(np.uint8)
    if pt_dyn is not None:
        a[np.asarray(pt_dyn) == DYN_DYNAMIC] = PT_DYNAMIC
    lab[np.asarray(apri_src, np.int64)] = a
    # the three lists partition what Patchwork kept: nothing it dropped is in one of them, nothing it kept is in none
    assert np.array_equal(lab == PT_DROPPED, np.asarray(cls) == 2), "the lists and cls disagree about the dropped points"
    assert len(ground_idx) + len(rejected_src) + len(apri_src) == int((lab != PT_DROPPED).sum()), "the lists overlap"
    return lab


def keep_of(labels, flags):
    """the keep rule of k_map_accumulate as a function of the label byte alone"""
    labels = np.asarray(labels)
    keep = labels != PT_DROPPED
    if not flags & MAP_IGNORE_DYNAMIC:
        keep &= labels != PT_DYNAMIC
    if flags & MAP_NO_GROUND:
        keep &= labels != PT_GROUND
    if flags & MAP_NO_REJECTED:
        keep &= labels != PT_REJECTED
    return keep


def collapse(labels):
    return COLLAPSE[np.asarray(labels)]
