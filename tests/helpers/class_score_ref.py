"""Reference statement of scvod_batch_point_classes / scvod_score_classes_device / scvod_batch_score_classes (include/scvod.h) in numpy --
test infrastructure only.

Written from the rules of the header (which restate src/plotObject.cpp:87-146 of the reference with two stated departures: the
estimate's y is y, and a neighbour counts only inside max_dist).  No golden file from the reference stands behind it: plotObject.cpp needs
PCL, which cannot be built here, so the known answers of tests/test_capi_class_score.py are worked out by hand instead.

The look-up is a brute force over every estimate point: fp32 d = (dx*dx + dy*dy) + dz*dz, the lowest index among equal distances
(`brute_nn`).  A whole batch is too large for it: `tree_nn` gives the same answer wherever the rules look at it (inside max_dist) and is
checked against the brute force in tests/test_capi_class_score.py."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "..", "..", "dr-using-scv-od_amd", "pyshim"))
sys.path.insert(0, _HERE)
import point_labels_ref as plr  # noqa: E402

GROUND, BUILDING, TREE = (40, 44, 48, 49, 71, 72), (50, 51, 52, 60), (70, 80, 81)   # the defaults of scvod_class_params_default
T_GROUND, T_BUILDING, T_TREE, T_PD = range(4)
E_OTHER, E_GROUND, E_BUILDING, E_TREE, E_NONE = range(5)
P_BIT = 32
PT_STATIC_BUILDING = 7
# estimate class of a SCVOD_PT_* byte: GROUND -> ground, STATIC_BUILDING -> building, STATIC_OTHER -> tree, everything else -> other
_EST_OF_PT = np.zeros(256, np.uint8)
_EST_OF_PT[plr.PT_GROUND] = E_GROUND
_EST_OF_PT[PT_STATIC_BUILDING] = E_BUILDING
_EST_OF_PT[plr.PT_STATIC_OTHER] = E_TREE


def truth_class(label, ground=GROUND, building=BUILDING, tree=TREE):
    """the lists in the order of check(): ground first, then building, then tree; in no list: pd"""
    sem = np.asarray(label).astype(np.uint32) & np.uint32(0xFFFF)
    out = np.full(sem.shape, T_PD, np.uint8)
    out[np.isin(sem, np.asarray(list(tree), np.uint32))] = T_TREE
    out[np.isin(sem, np.asarray(list(building), np.uint32))] = T_BUILDING
    out[np.isin(sem, np.asarray(list(ground), np.uint32))] = T_GROUND
    return out


def estimate_class(pt_bytes):
    return _EST_OF_PT[np.asarray(pt_bytes, np.uint8)]


def brute_nn(est_xyz, q_xyz, chunk=256):
    m = np.asarray(est_xyz, np.float32).reshape(-1, 3)
    q = np.asarray(q_xyz, np.float32).reshape(-1, 3)
    idx = np.full(len(q), -1, np.int64)
    sq = np.full(len(q), np.inf, np.float32)
    if len(m):
        for a in range(0, len(q), chunk):
            e = m[None, :, :] - q[a:a + chunk, None, :]
            d = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            i = d.argmin(axis=1)  # (the first of equal minima: the lowest index)
            idx[a:a + chunk] = i
            sq[a:a + chunk] = d[np.arange(len(i)), i]
    return idx, sq


def tree_nn(est_xyz, q_xyz, reach=0.75):
    """brute_nn's answer for every query with an estimate point inside `reach` (idx -1 / +inf or a farther point otherwise), at the scale
    of a batch: scipy's kd-tree (float64 on the fp32 coordinates) names the four nearest candidates, the fp32 expression and the tie rule
    decide among those within 1e-5 of the nearest; a query whose fourth candidate is still that close goes to the brute force"""
    from scipy.spatial import cKDTree
    m = np.asarray(est_xyz, np.float32).reshape(-1, 3)
    q = np.asarray(q_xyz, np.float32).reshape(-1, 3)
    idx = np.full(len(q), -1, np.int64)
    sq = np.full(len(q), np.inf, np.float32)
    if not len(m) or not len(q):
        return idx, sq
    k = min(4, len(m))
    dd, ii = cKDTree(m.astype(np.float64)).query(q.astype(np.float64), k=k, distance_upper_bound=float(reach) * 1.01)
    dd, ii = dd.reshape(len(q), k), ii.reshape(len(q), k)
    found = np.isfinite(dd[:, 0])
    close = np.isfinite(dd) & (dd <= dd[:, :1] * (1 + 1e-5) + 1e-7)
    e = m[np.minimum(ii, len(m) - 1)] - q[:, None, :]
    d = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(np.float32)
    d[~close] = np.inf
    key = np.where(close, (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ii.astype(np.uint64), np.uint64(0xFFFFFFFFFFFFFFFF))
    best = key.min(axis=1)
    idx[found] = (best[found] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    sq[found] = (best[found] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    crowd = np.nonzero(found & close[:, k - 1] & (len(m) > k))[0]
    if len(crowd):
        idx[crowd], sq[crowd] = brute_nn(m, q[crowd])
    return idx, sq


def finish(conf, pd_far):
    """num, P and the fp32 rates of scvod_class_finish (NaN where num == 0)"""
    conf = np.asarray(conf, np.int64).reshape(4, 5)
    num = conf.sum(1)
    P = np.array([conf[0, E_GROUND], conf[1, E_BUILDING] + conf[1, E_TREE], conf[2, E_BUILDING] + conf[2, E_TREE],
                  conf[3, E_OTHER] + conf[3, E_NONE] + int(pd_far)], np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rate_P = P.astype(np.float32) / num.astype(np.float32)
        rate_N = (num - P).astype(np.float32) / num.astype(np.float32)
    return num, P, rate_P.astype(np.float32), rate_N.astype(np.float32)


def score(gt_xyz, gt_label, est_xyz, est_pt, max_dist=0.75, ground=GROUND, building=BUILDING, tree=TREE, nn_fn=brute_nn):
    """dict(conf [4][5], pd_far, num, P, rate_P, rate_N, point_result)"""
    gt_xyz = np.asarray(gt_xyz, np.float32).reshape(-1, 3)
    t = truth_class(np.asarray(gt_label, np.uint32).reshape(-1), ground, building, tree)
    idx, d = nn_fn(est_xyz, gt_xyz)
    max2 = np.float32(max_dist) * np.float32(max_dist)
    assert max2 > np.float32(0.5)
    has = (idx >= 0) & (d < max2)
    e = np.full(len(t), E_NONE, np.uint8)
    e[has] = estimate_class(np.asarray(est_pt, np.uint8).reshape(-1)[idx[has]])
    far = (idx >= 0) & (d > np.float32(0.5))
    P = np.where(t == T_GROUND, e == E_GROUND,
                 np.where(t == T_PD, (e == E_OTHER) | (e == E_NONE) | far, (e == E_BUILDING) | (e == E_TREE)))
    conf = np.zeros((4, 5), np.int64)
    np.add.at(conf, (t.astype(np.int64), e.astype(np.int64)), 1)
    pd_far = int(((t == T_PD) & has & (e != E_OTHER) & far).sum())
    num, Pn, rate_P, rate_N = finish(conf, pd_far)
    assert np.array_equal(Pn, np.bincount(t[P], minlength=4)), "P per class and the P bits disagree"
    return dict(conf=conf.tolist(), pd_far=pd_far, num=num.tolist(), P=Pn.tolist(), rate_P=rate_P, rate_N=rate_N,
                point_result=(t | (e << 2) | (P * P_BIT)).astype(np.uint8), nn_idx=idx, nn_sq=d)


def batch_point_classes(ctx, offs, flags=0):
    """the class byte of every input point of the ctx's last batch, from outputs that exist without scvod_batch_point_classes: the
    bytes of batch_point_labels, with a STATIC_OTHER point set to 7 where batch_fetch_cluster_classes reports building (0) for its apri
    point; the input index of an apri point is the `apri_src` of batch_fetch"""
    n = int(offs[-1])
    lab = ctx.batch_point_labels(flags=flags & plr.MAP_IGNORE_DYNAMIC).cpu().numpy()[:n].copy()
    for s in range(len(offs) - 1):
        r = ctx.batch_fetch(s)
        cls = ctx.batch_fetch_cluster_classes(s, r["n_apri"], car_label=2, building_label=0, tree_label=1)
        src = int(offs[s]) + np.asarray(r["apri_src"], np.int64)[:r["n_apri"]]
        hit = src[(cls == 0) & (lab[src] == plr.PT_STATIC_OTHER)]
        lab[hit] = PT_STATIC_BUILDING
    return lab


def keep_of(classes, flags):
    """the export's keep rule on class bytes: a building point is kept as the STATIC_OTHER point it is for the export"""
    c = np.asarray(classes, np.uint8)
    return plr.keep_of(np.where(c == PT_STATIC_BUILDING, plr.PT_STATIC_OTHER, c), flags)


def batch_score(scvod_py, x, offs, poses, classes, gt_label, flags=0, **kw):
    """truth = every input point in the world frame (quality.world_points' expression) with its label; estimate = the kept points, in
    input order, with their class bytes"""
    import quality
    w = quality.world_points(scvod_py, np.asarray(x, np.float32), offs, poses)
    keep = keep_of(classes, flags)
    kw.setdefault("nn_fn", tree_nn)
    out = score(w, gt_label, w[keep], np.asarray(classes, np.uint8)[keep], **kw)
    out["world"], out["keep"] = w, keep
    return out
