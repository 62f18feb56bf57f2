"""The intensity merge on the device (csrc/scvod_k_merge.inc, scvod_set_intensity_merge) against the convention restatement of
SSC::refineClusterByIntensity (tests/helpers/intensity_merge_ref.py) on K64, PARK and OS128 batches: the post-merge partition,
its types against the oracle's box rules, the stage's counters, the tracking chain on the fused partition against the oracle's chains,
and the merge switched off leaving every output as it was."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import intensity_merge_ref as imr  # noqa: E402

pytestmark = pytest.mark.gpu

YAML = (2, 2.0, 1.0)
DEFAULTS = (2, 50.0, 20.0)
JOBS = {"K64": ("semantickitti", 5, 300, 3, 7), "PARK": ("parkinglot", 3, 30, 3, 3), "OS128": ("os128_fine", 5, 302, 3, 1)}  # (OS128: scan 303 goes through k_cc_exact)


def _batch(scvod, kind):
    import synth
    import torch
    preset, seq, first, count, stride = JOBS[kind]
    P = scvod.make_params(preset)
    scans = [synth.make_scan(seq, first + k * stride, kind, device="cuda") for k in range(count)]
    d = torch.cat([sc[0] for sc in scans]).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(sc[0]) for sc in scans])]).astype(np.int32)
    return P, d, offs, count


def _cluster(scvod, P, d, offs, count, merge=None):
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=count)
    if merge is not None:
        ctx.set_intensity_merge(*merge)
    ctx.batch_process(d, offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    out = []
    for s in range(count):
        r = ctx.batch_fetch(s)
        out.append((r, ctx.batch_fetch_clusters(s, r["n_apri"]), ctx.batch_fetch_cluster_types(s, r["n_apri"])))
    return ctx, out


@pytest.mark.parametrize("kind", ["K64", "PARK", "OS128"])
def test_merge_off_is_identical(scvod, kind):
    P, d, offs, count = _batch(scvod, kind)
    a, ra = _cluster(scvod, P, d, offs, count)
    b, rb = _cluster(scvod, P, d, offs, count, merge=(0, 2, 2.0, 1.0))
    for (r1, n1, t1), (r2, n2, t2) in zip(ra, rb):
        assert np.array_equal(n1, n2) and np.array_equal(t1, t2)
    T = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(-1), count)
    maps = []
    for ctx in (a, b):
        ctx.batch_track(T)
        m = scvod.StaticMap(1 << 21, leaf=0.2)
        m.accumulate(ctx, np.zeros((count, 6), np.float32))
        maps.append(np.sort(m.export().cpu().numpy().view(np.uint64).reshape(-1)))
        m.close()
    assert np.array_equal(maps[0], maps[1])
    for s in range(count):
        x, y = a.batch_fetch_track(s), b.batch_fetch_track(s)
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), (s, k)
    assert b.batch_cluster_merge_stats() == dict(clusters_before=0, fusions=0, clusters_after=0, scans_fused=0)
    a.close()
    b.close()


@pytest.mark.parametrize("kind,params,iterations", [("K64", YAML, 1), ("K64", YAML, 3), ("K64", DEFAULTS, 2), ("K64", (1, 2.0, 1.0), 3),
                                                    ("PARK", YAML, 3), ("PARK", DEFAULTS, 1), ("OS128", YAML, 3), ("OS128", (1, 50.0, 20.0), 2),
                                                    ("K64", (3, 50.0, 20.0), 2), ("OS128", (3, 50.0, 20.0), 1)])
def test_partition_and_types_equal_the_convention(scvod, oracle, kind, params, iterations):
    P, d, offs, count = _batch(scvod, kind)
    base, rb = _cluster(scvod, P, d, offs, count)
    base.close()
    ctx, rm = _cluster(scvod, P, d, offs, count, merge=(iterations,) + params)
    grid = tuple(int(g) for g in oracle.grid_dims(P)[:3])
    want_stats = dict(clusters_before=0, fusions=0, clusters_after=0)
    for (r, pre, _), (_, got, types) in zip(rb, rm):
        vox = oracle.voxelize(P, r["apri"])
        st = {}
        want = imr.convention(vox, pre, grid, iterations, params[0], params[1], params[2], stats=st)
        assert np.array_equal(got, want)
        assert np.array_equal(types, oracle.cluster_types(P, r["apri"], got, car_label=2, other_label=1))
        for k in want_stats:
            want_stats[k] += st[k]
    if kind == "OS128":
        assert ctx.batch_cluster_stats()["runs_clustered_again"] > 0   # the batch holds a scan of k_cc_exact
    got_stats = ctx.batch_cluster_merge_stats()
    assert {k: got_stats[k] for k in want_stats} == want_stats
    assert got_stats["clusters_before"] - got_stats["clusters_after"] >= got_stats["fusions"]
    if kind == "K64" and params == YAML:
        assert got_stats["fusions"] > 0 and got_stats["scans_fused"] > 0
    ctx.close()


def test_one_shot_cluster_applies_the_setting(scvod, oracle):
    P, d, offs, count = _batch(scvod, "PARK")
    ctx, rm = _cluster(scvod, P, d, offs, count, merge=(3,) + YAML)
    r, got, _ = rm[0]
    assert np.array_equal(ctx.cluster(r["apri"]), got)
    ctx.close()


def _sequence(scvod, kind, preset, first, count, skip):
    import synth
    import torch
    P = scvod.make_params(preset)
    scans = [synth.make_scan(5, first + k * skip, kind, device="cuda") for k in range(count)]
    d = torch.cat([sc[0] for sc in scans]).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(sc[0]) for sc in scans])]).astype(np.int32)
    poses = np.asarray([sc[2] for sc in scans], np.float32)
    return P, d, offs, poses


@pytest.mark.parametrize("kind,preset,skip,count,first", [("K64", "semantickitti", 5, 40, 300), ("PARK", "parkinglot", 1, 60, 30)])
def test_chain_on_the_fused_partition(scvod, oracle, kind, preset, skip, count, first):
    """the successor tables, car lists, max_name carrier and per-point dynamic bytes follow the fused clusters: the device chain equals
    the oracle's chains run on the fused names and types -- the literal max_name with the oracle's carrier mapped to its fusion, and
    fresh numbers with the literal reading off"""
    P, d, offs, poses = _sequence(scvod, kind, preset, first, count, skip)
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=count)
    ctx.set_intensity_merge(*((3,) + YAML))
    ctx.batch_process(d, offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    res = [ctx.batch_fetch(s) for s in range(count)]
    names = [ctx.batch_fetch_clusters(s, r["n_apri"]) for s, r in enumerate(res)]
    types = [ctx.batch_fetch_cluster_types(s, r["n_apri"], car_label=2, other_label=1) for s, r in enumerate(res)]
    assert ctx.batch_cluster_merge_stats()["fusions"] > 0
    ln, _ = ctx.batch_cluster_last_name(count)
    T = np.zeros((count, 12), np.float32)
    for s in range(count - 1):
        T[s] = ctx.pose_delta(poses[s], poses[s + 1])
    ctx.batch_track(T)
    assert ctx.batch_track_stats()["error_bits"] == 0
    got = np.concatenate([ctx.batch_fetch_track(s)["pt_dyn"] for s in range(count)])
    apri = np.concatenate([r["apri"] for r in res])
    ao = np.concatenate([[0], np.cumsum([r["n_apri"] for r in res])]).astype(np.int32)
    nm, ty = np.concatenate(names), np.concatenate(types)
    collide = np.asarray([oracle.cluster_last_name(P, r["apri"])[0] for r in res], np.int32)
    collide = np.asarray([names[s][c] if c >= 0 else -1 for s, c in enumerate(collide)], np.int32)   # the carrier's fusion
    known = ln[:, 2] == 0
    for s in np.nonzero(known)[0]:
        assert ln[s, 0] == collide[s] or (ln[s, 0] == -1 and collide[s] >= 0 and types[s][collide[s]] == -1)
    collide[~known] = -1
    dynL, ndL, _ = oracle.sequence_tracking_literal(P, apri, ao, nm, ty, collide, poses, chain=3)
    assert np.array_equal(got, dynL), f"{int((got != dynL).sum())} of {len(dynL)} per-point bytes differ from the literal chain"
    assert int(got.sum()) > 0
    ctx.set_max_name_literal(False)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    ctx.batch_track(T)
    got0 = np.concatenate([ctx.batch_fetch_track(s)["pt_dyn"] for s in range(count)])
    dyn3, _ = oracle.sequence_tracking(P, apri, ao, nm, ty, poses, chain=3)
    assert np.array_equal(got0, dyn3), f"{int((got0 != dyn3).sum())} bytes differ from the chain with fresh numbers"
    ctx.close()
