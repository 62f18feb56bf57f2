"""tests/helpers/track_table_ref.py -- the numpy statement tests/test_gpu_track_tables.py holds the device to -- pinned against the
oracle's restatement of SSC::tracking (oracle_track_decide) on one synthetic K64 pair: the successor's table is built from the oracle's
clustering and box types the way scvod_batch_export_table documents it, the landing keys come from oracle_track_probe, and clusters,
remap_name pairs and states must agree field for field.  Not gpu."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import track_table_ref as ttr


def _segment(oracle, P, x):
    ng = oracle.patchwork(P, x, 1)["nonground_idx"]
    apri = oracle.bin(P, x[ng], True)["apri"]
    names, _, _ = oracle.cluster(P, apri)
    types = oracle.cluster_types(P, apri, names, car_label=2, other_label=1)
    vox = oracle.voxelize(P, apri)
    return apri, names, types, vox


def _xyzi(apri):
    return np.stack([apri["x"], apri["y"], apri["z"], apri["intensity"]], 1).astype(np.float32)


def test_helper_equals_the_oracle_decision(oracle, scvod):
    import synth
    P = scvod.make_params("semantickitti")
    a, _, pose_a = synth.make_scan(5, 420, "K64")
    b, _, pose_b = synth.make_scan(5, 421, "K64")
    T = oracle.pose_delta(pose_a, pose_b)
    apri_a, names_a, types_a, _ = _segment(oracle, P, a.numpy())
    apri_b, names_b, types_b, vox_b = _segment(oracle, P, b.numpy())
    want = oracle.track_decide(P, apri_a, names_a, types_a, apri_b, names_b, types_b, T)

    keys, label, size, typ = ttr.table_of_segmentation(vox_b["vox_key"], vox_b["vox_pts"][vox_b["vox_pt_begin"][:-1]], names_b, types_b)
    assert (label == -1).any() and (typ == ttr.TYPE_CAR).any() and (typ == ttr.TYPE_OTHER).any()
    clusters, roots = ttr.car_clusters(names_a, types_a)
    landing = np.full(len(apri_a), ttr.NO_KEY, np.int32)
    car = np.concatenate(clusters)
    landing[car] = ttr.landing_keys(oracle, P, _xyzi(apri_a[car]), T)
    got = ttr.decide(clusters, roots, landing, keys, label, size, typ, P.occupancy, n_apri=len(apri_a), pt_type=types_a)

    assert len(roots) >= 10, "the pair must hold a handful of car clusters"
    assert np.array_equal(got["cluster_root"], want["clusters"][:, 0])
    assert np.array_equal(got["cluster_state"], want["clusters"][:, 1])
    assert np.array_equal(got["n_unique"], want["clusters"][:, 2])
    assert np.array_equal(np.diff(got["pair_begin"]), want["clusters"][:, 3])
    assert np.array_equal(got["pair_begin"], want["pair_begin"])
    assert np.array_equal(got["pair_label"], want["pairs"][:, 0])
    assert np.array_equal(got["pair_count"], want["pairs"][:, 1])
    assert set(np.unique(got["cluster_state"])) >= {0, 1}, "the pair must decide static and dynamic clusters"
    # the unique slots are the oracle's probe of the same clusters against the same table
    offs = np.concatenate([[0], np.cumsum([len(m) for m in clusters])])
    _, ouq, oub = oracle.track_probe(P, _xyzi(apri_a[car]), offs, T, keys, label)
    assert np.array_equal(np.concatenate(got["uniq"]), ouq) and np.array_equal(np.cumsum([0] + [len(u) for u in got["uniq"]]), oub)
    # the per-point bytes against the sequence-level oracle in its per-cluster mode (the second scan has no successor: all static)
    apri = np.concatenate([apri_a, apri_b])
    ao = np.array([0, len(apri_a), len(apri)], np.int32)
    dyn, nd = oracle.sequence_tracking(P, apri, ao, np.concatenate([names_a, names_b]), np.concatenate([types_a, types_b]),
                                       np.asarray([pose_a, pose_b], np.float32), chain=2)
    assert np.array_equal(got["pt_dyn"], dyn[:len(apri_a)]) and got["n_dynamic_clusters"] == nd
    assert got["n_dynamic_points"] == int((dyn[:len(apri_a)] == 1).sum())


def test_the_state_rule_on_a_hand_made_table():
    """every branch of ssc.cpp:1323-1397 on six one-point clusters and a table of nine records, worked out by hand"""
    keys = [10, 20, 30, 31, 40, 50, 60, 61, 70]
    label = [5, 5, 6, 6, 7, 8, -1, 9, 9]
    size = [4, 4, 2, 2, 4, 1, 0, 2, 2]                # occupancy 0.5: one hit of label 5 is 0.25 (below), of label 6 is 0.5 (at)
    typ = [2, 2, 2, 2, 1, 1, 0, 1, 1]
    clusters = [np.array([0]), np.array([1]), np.array([2, 3]), np.array([4]), np.array([5]), np.array([6, 7]), np.array([8, 9])]
    landing = [15, 10, 30, 30, 40, 50, 10, 40, 60, 71]
    r = ttr.decide(clusters, [0, 1, 2, 4, 5, 6, 8], landing, keys, label, size, typ, 0.5, n_apri=11, pt_type=[2] * 10 + [-1])
    #   no key -> dynamic; car below -> dynamic; car at the ratio (duplicates count once) -> static; other below -> static;
    #   other at or above -> untouched; two labels -> static; an erased record and a key past the last -> no hit -> dynamic
    assert r["cluster_state"].tolist() == [1, 1, 0, 0, -1, 0, 1]
    assert r["n_unique"].tolist() == [0, 1, 1, 1, 1, 2, 0]
    assert r["pair_begin"].tolist() == [0, 0, 1, 2, 3, 4, 6, 6]
    assert r["pair_label"].tolist() == [5, 6, 7, 8, 5, 7] and r["pair_count"].tolist() == [1, 1, 1, 1, 1, 1]
    assert [u.tolist() for u in r["uniq"]] == [[], [0], [2], [4], [5], [0, 4], []]
    assert r["pt_dyn"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 2]
    assert (r["n_dynamic_clusters"], r["n_dynamic_points"]) == (3, 4)
