"""numpy statement of the first-order tracking decision of ONE scan against a successor TABLE (scvod_batch_track with an external
table, include/scvod.h): what csrc/scvod_track.hip's k_tk_probe / k_tk_decide / k_tk_dyn must give, field for field.

Inputs are plain arrays: the car clusters of the scan as per-cluster lists of apri indices (roots -- the smallest index of each --
ascending), the key every apri point lands on in the successor's grid, and the table in the layout scvod_batch_export_table documents:
ascending unique keys and per record {label, |occupy_voxels| of the label's cluster, type (0 erased, 1 other, 2 car)}.  The rule is
SSC::tracking's (ssc.cpp:1304-1397) as the header of scvod_track.hip restates it.  Nothing here calls the library.

The landing keys are NOT worked out here: the fp32 transform and the unfiltered re-bin are restated once, in the oracle's
oracle_track_probe; landing_keys() below reads them off it by probing a table that holds every key of a range."""
import numpy as np

DYN_STATIC, DYN_DYNAMIC, DYN_UNCLUSTERED = 0, 1, 2  # SCVOD_DYN_*
TYPE_ERASED, TYPE_OTHER, TYPE_CAR = 0, 1, 2           # the table's type column
NO_KEY = np.iinfo(np.int32).min                       # a landing key nobody asked for (points of no car cluster)


def landing_keys(oracle, P, xyzi, T, lo=None, hi=None):
    """the voxel key every point of xyzi [n, 4] lands on after T, from oracle.track_probe against the table of ALL keys lo .. hi - 1
    with every label set (slot + lo is then the key).  Default range: three times the grid, centred on it; a point that leaves it
    is an error (choose a wider range), never a silent miss"""
    bins = oracle.grid_dims(P)[3]
    lo = -bins if lo is None else lo
    hi = 2 * bins if hi is None else hi
    keys = np.arange(lo, hi, dtype=np.int32)
    x = np.ascontiguousarray(xyzi, np.float32)
    hit, _, _ = oracle.track_probe(P, x, [0, len(x)], T, keys, np.zeros(len(keys), np.int32))
    if (hit < 0).any():
        raise ValueError(f"{int((hit < 0).sum())} points land outside the keys {lo} .. {hi - 1}")
    return (hit + lo).astype(np.int32)


def car_clusters(names, types, car=2):
    """per-cluster point lists of a segmentation (names: canonical cluster of every apri point, types: its cluster's type), the car
    clusters only, roots ascending"""
    names, types = np.asarray(names), np.asarray(types)
    idx = np.nonzero(types == car)[0]
    order = np.argsort(names[idx], kind="stable")
    idx = idx[order]
    roots, start = np.unique(names[idx], return_index=True)
    return [idx[a:b] for a, b in zip(start, list(start[1:]) + [len(idx)])], roots.astype(np.int32)


def table_of_segmentation(vox_key, vox_first_pt, names, types, car=2):
    """the table scvod_batch_export_table documents for a segmented scan: per voxel (ascending key) the label of its points' cluster
    (-1 where the bounding-box refine erased it), the number of voxels that carry the label, the cluster's type"""
    names, types = np.asarray(names), np.asarray(types)
    f = np.asarray(vox_first_pt)
    erased = types[f] == -1
    label = np.where(erased, -1, names[f]).astype(np.int32)
    size = np.zeros(len(label), np.int32)
    if (~erased).any():
        u, inv, cnt = np.unique(label[~erased], return_inverse=True, return_counts=True)
        size[~erased] = cnt[inv]
    typ = np.where(erased, TYPE_ERASED, np.where(types[f] == car, TYPE_CAR, TYPE_OTHER)).astype(np.int32)
    return np.asarray(vox_key, np.int32), label, size, typ


def pack_table(keys, label, size, typ, spare_records=0, spare_fill=0):
    """int32 [1 + nv + spare, 4]: header {records, n_voxels, 0, 0}, then the records; `spare` records of `spare_fill` behind them"""
    nv = len(keys)
    t = np.full((1 + nv + spare_records, 4), spare_fill, np.int32)
    t[0] = (nv, nv, 0, 0)
    t[1:1 + nv] = np.stack([keys, label, size, typ], 1) if nv else np.zeros((0, 4), np.int32)
    return t


def decide(clusters, roots, landing, keys, label, size, typ, occupancy, n_apri=None, pt_type=None):
    """-> dict with the fields of scvod_batch_fetch_track for the scan (cluster_root, cluster_state, n_unique, pair_begin, pair_label,
    pair_count, n_dynamic_clusters, n_dynamic_points and -- given n_apri and the per-point type (-1 erased, else its cluster's) --
    pt_dyn), plus `uniq`: the sorted unique hit slots per cluster"""
    keys, label, size, typ = (np.asarray(a, np.int64) for a in (keys, label, size, typ))
    assert (np.diff(keys) > 0).all(), "a table's keys ascend strictly"
    landing = np.asarray(landing, np.int64)
    occ = np.float32(occupancy)
    state, n_unique, uniq_all = [], [], []
    pair_begin, pair_label, pair_count = [0], [], []
    for members in clusters:
        k = landing[members]
        slot = np.searchsorted(keys, k)
        ok = slot < len(keys)
        ok[ok] = keys[slot[ok]] == k[ok]
        ok[ok] = label[slot[ok]] != -1          # ssc.cpp:1304-1305: the voxel exists and carries a label
        uniq = np.unique(slot[ok])              # sampleVec over all labels: sorted, de-duplicated
        labs, cnt = np.unique(label[uniq], return_counts=True)  # remap_name: ascending label, unique voxels each
        if len(labs) == 0:
            st = 1                              # ssc.cpp:1323-1326
        elif len(labs) == 1:
            rec = uniq[0]
            below = np.float32(cnt[0]) / np.float32(size[rec]) < occ  # ssc.cpp:1336
            car = typ[rec] == TYPE_CAR
            st = (1 if car else 0) if below else (0 if car else -1)    # ssc.cpp:1337-1352, 1377-1380
        else:
            st = 0                              # ssc.cpp:1396-1397
        state.append(st)
        n_unique.append(len(uniq))
        uniq_all.append(uniq.astype(np.int32))
        pair_label += labs.tolist()
        pair_count += cnt.tolist()
        pair_begin.append(len(pair_label))
    state = np.asarray(state, np.int32).reshape(-1)
    out = dict(cluster_root=np.asarray(roots, np.int32), cluster_state=state, n_unique=np.asarray(n_unique, np.int32).reshape(-1),
               pair_begin=np.asarray(pair_begin, np.int32), pair_label=np.asarray(pair_label, np.int32).reshape(-1),
               pair_count=np.asarray(pair_count, np.int32).reshape(-1), uniq=uniq_all,
               n_dynamic_clusters=int((state == 1).sum()),
               n_dynamic_points=int(sum(len(m) for m, s in zip(clusters, state) if s == 1)))
    if n_apri is not None:
        dyn = np.where(np.asarray(pt_type) == -1, DYN_UNCLUSTERED, DYN_STATIC).astype(np.uint8)
        for m, s in zip(clusters, state):
            if s == 1:
                dyn[m] = DYN_DYNAMIC
        assert len(dyn) == n_apri
        out["pt_dyn"] = dyn
    return out
