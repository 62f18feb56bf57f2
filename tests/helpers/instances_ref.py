"""Reference statement of scvod_score_instances_device / scvod_instance_finish / scvod_instance_merge (include/scvod.h) in numpy and plain
Python -- the yardstick of tests/test_capi_instances.py and tests/test_gpu_instances.py.  Nothing of the library is used here.

table     np.unique on the keys; np.add.at for the three counts, np.minimum.at for the first index.  Result byte: bit 0 inlier, bit 1
          truth dynamic, bit 2 estimate dynamic at the neighbour; a point is preserved iff bit 0 is set and bit 1 == bit 2
          (analysis.py's num_static_preserved + num_dynamic_preserved); the bits above are ignored
finish    the HD / LD object rule: this project's convention (tool/plotIoU.py:70-84 holds hard-coded numbers only)
merge     two tables ascending by key -> one
"""
import numpy as np

DTYPE = np.dtype([("label", "<u4"), ("first_point", "<i4"), ("n_points", "<i8"), ("n_inlier", "<i8"), ("n_preserved", "<i8")])
DYNAMIC = tuple(range(252, 260))
STATIC = (10, 31, 30, 32, 16, 13, 18, 20)   # the SemanticKITTI static counterparts of 252..259, in that order
COUNTS = ("hd_gt", "hd_removed", "ld_gt", "ld_retained", "hd_points", "hd_points_preserved", "ld_points", "ld_points_preserved", "skipped")


def table(keys, point_result):
    keys = np.asarray(keys).astype(np.uint32).reshape(-1)
    res = np.asarray(point_result).astype(np.uint8).reshape(-1)
    assert keys.shape == res.shape
    uniq, inv = np.unique(keys, return_inverse=True)
    out = np.zeros(len(uniq), DTYPE)
    out["label"] = uniq
    inl = (res & 1) != 0
    pre = inl & (((res >> 1) & 1) == ((res >> 2) & 1))
    n_points, n_inlier, n_preserved = (np.zeros(len(uniq), np.int64) for _ in range(3))
    first = np.full(len(uniq), np.iinfo(np.int32).max, np.int64)
    np.add.at(n_points, inv, 1)
    np.add.at(n_inlier, inv, inl.astype(np.int64))
    np.add.at(n_preserved, inv, pre.astype(np.int64))
    np.minimum.at(first, inv, np.arange(len(keys), dtype=np.int64))
    out["n_points"], out["n_inlier"], out["n_preserved"], out["first_point"] = n_points, n_inlier, n_preserved, first
    return out


def finish(tab, dynamic=DYNAMIC, static=STATIC, removed_below=0.5, retained_from=0.5, min_points=1):
    r = dict.fromkeys(COUNTS, 0)
    for rec in np.asarray(tab, DTYPE).reshape(-1):
        label, n, pre = int(rec["label"]), int(rec["n_points"]), int(rec["n_preserved"])
        sem = label & 0xFFFF
        if (label >> 16) == 0 or n < min_points or not (sem in dynamic or sem in static):
            r["skipped"] += 1
        elif sem in dynamic:
            r["hd_gt"] += 1
            r["hd_points"] += n
            r["hd_points_preserved"] += pre
            r["hd_removed"] += float(pre) < removed_below * float(n)
        else:
            r["ld_gt"] += 1
            r["ld_points"] += n
            r["ld_points_preserved"] += pre
            r["ld_retained"] += float(pre) >= retained_from * float(n)
    r = {k: int(v) for k, v in r.items()}
    r["hd_removed_rate"] = 100.0 * r["hd_removed"] / r["hd_gt"] if r["hd_gt"] else float("nan")
    r["ld_retained_rate"] = 100.0 * r["ld_retained"] / r["ld_gt"] if r["ld_gt"] else float("nan")
    return r


def merge(a, b):
    acc = {}
    for rec in list(np.asarray(a, DTYPE).reshape(-1)) + list(np.asarray(b, DTYPE).reshape(-1)):
        k = int(rec["label"])
        if k in acc:
            o = acc[k]
            acc[k] = (k, min(o[1], int(rec["first_point"])), o[2] + int(rec["n_points"]), o[3] + int(rec["n_inlier"]),
                      o[4] + int(rec["n_preserved"]))
        else:
            acc[k] = (k, int(rec["first_point"]), int(rec["n_points"]), int(rec["n_inlier"]), int(rec["n_preserved"]))
    return np.array([acc[k] for k in sorted(acc)], DTYPE)
