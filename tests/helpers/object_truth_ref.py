"""Reference statement of scvod_batch_object_truth / scvod_object_truth_finish (include/scvod.h) in numpy and plain Python -- the
yardstick of tests/test_capi_object_truth.py and tests/test_gpu_object_truth.py.  Nothing of the library is used here.

record    np.unique over the 32-bit labels of one object's members: the label with the largest count wins, equal counts go to the
          SMALLEST label value (np.unique returns the labels ascending and np.argmax the first maximum); n_class the members of the
          winner's class (label & 0xFFFF), n_moving the members of a class in `dynamic`, n_distinct the distinct labels
records   the same per object of a table: the members are the run [point_begin, point_begin + n_points) of the member list, whose
          entries are INPUT indices inside the object's scan
finish    the object rule: this project's convention (the reference's tools hold hard-coded numbers only)
"""
import numpy as np

DTYPE = np.dtype([("label", "<u4"), ("n_label", "<i4"), ("n_class", "<i4"), ("n_moving", "<i4"), ("n_distinct", "<i4"), ("n_points", "<i4"),
                  ("reserved", "<i4", 2)])
DYNAMIC = tuple(range(252, 260))
COUNTS = ("moving_objects", "moving_dynamic", "moving_car_static", "moving_car_untracked", "moving_not_car", "static_objects",
          "static_dynamic", "mixed_objects", "skipped")
RATES = ("precision", "recall")


def moving_mask(labels, dynamic=DYNAMIC):
    sem = np.asarray(labels).astype(np.uint32) & np.uint32(0xFFFF)
    return np.isin(sem, np.asarray(list(dynamic), np.uint32)) if len(dynamic) else np.zeros(sem.shape, bool)


def record(labels, dynamic=DYNAMIC):
    """the record of one object from the labels of its members (any order)"""
    lab = np.asarray(labels).astype(np.uint32).reshape(-1)
    r = np.zeros((), DTYPE)
    r["n_points"] = len(lab)
    if len(lab) == 0:
        r["label"] = 0xFFFFFFFF
        return r
    uniq, cnt = np.unique(lab, return_counts=True)
    w = int(np.argmax(cnt))
    r["label"], r["n_label"] = uniq[w], cnt[w]
    r["n_class"] = int(((lab & np.uint32(0xFFFF)) == (uniq[w] & np.uint32(0xFFFF))).sum())
    r["n_moving"] = int(moving_mask(lab, dynamic).sum())
    r["n_distinct"] = len(uniq)
    return r


def records(objects, members, scan_offsets, gt_label, dynamic=DYNAMIC):
    """one record per object of a table (its OBJECT_DTYPE records, its member list, the batch's scan offsets) for the labels gt_label
    of the batch's input points"""
    gt = np.asarray(gt_label).astype(np.uint32).reshape(-1)
    out = np.zeros(len(objects), DTYPE)
    for o, rec in enumerate(objects):
        m = np.asarray(members[int(rec["point_begin"]):int(rec["point_begin"]) + int(rec["n_points"])], np.int64)
        out[o] = record(gt[int(scan_offsets[int(rec["scan"])]) + m], dynamic)
    return out


def finish(objects, truth, moving_from=0.5, pure_from=0.5, min_points=1):
    r = dict.fromkeys(COUNTS, 0)
    for o, t in zip(objects, np.asarray(truth, DTYPE).reshape(-1)):
        n, n_label, n_moving = int(t["n_points"]), int(t["n_label"]), int(t["n_moving"])
        cls, state, dyn = int(o["cls"]), int(o["state"]), int(o["dynamic"]) == 1
        if n < min_points:
            r["skipped"] += 1
            continue
        r["mixed_objects"] += float(n_label) < pure_from * float(n)
        if float(n_moving) >= moving_from * float(n):
            r["moving_objects"] += 1
            if dyn:
                r["moving_dynamic"] += 1
            elif cls != 2:
                r["moving_not_car"] += 1
            elif state == 0:
                r["moving_car_static"] += 1
            else:
                r["moving_car_untracked"] += 1
        else:
            r["static_objects"] += 1
            r["static_dynamic"] += dyn
    r = {k: int(v) for k, v in r.items()}
    alarms = r["moving_dynamic"] + r["static_dynamic"]
    r["precision"] = 100.0 * r["moving_dynamic"] / alarms if alarms else float("nan")
    r["recall"] = 100.0 * r["moving_dynamic"] / r["moving_objects"] if r["moving_objects"] else float("nan")
    return r
