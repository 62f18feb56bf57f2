"""The region growing on the device (csrc/scvod_k_rgrow.inc, scvod_set_region_growing) against the CPU restatement of
SSC::regionGrowing (tests/helpers/region_growing_ref.cpp): hand-built scenes, K64 / PARK / OS128 batches (normals and curvatures
bit for bit, segments, classes, counters), the fused partition of the intensity merge, a cluster on the HBM path, and the stage
switched on leaving every existing output as it was."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_region_growing_ref import build_rg, run  # noqa: E402

pytestmark = pytest.mark.gpu

CAR, BUILDING, TREE = 2, 0, 1
JOBS = {"K64": ("semantickitti", 5, 300, 3, 7), "PARK": ("parkinglot", 3, 30, 3, 3), "OS128": ("os128_fine", 5, 302, 3, 1)}


@pytest.fixture(scope="module")
def rg(tmp_path_factory):
    return build_rg(tmp_path_factory.mktemp("rgref"))


def _canon(nc):
    a = nc.copy()
    a[np.isnan(a)] = np.nan
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def expected(rg, P, xyz, names, types, curv=1.2):
    """per apri point of one scan: classes, normal_curv, segments, and the scan's counters"""
    n = len(names)
    cls = np.where(types == -1, -1, np.where(types == CAR, CAR, TREE)).astype(np.int32)
    nc = np.full((n, 4), np.nan, np.float32)
    seg = np.full(n, -1, np.int32)
    st = dict(candidate_clusters=0, building_clusters=0, candidate_points=0, kept_edges=0, hbm_clusters=0, tail_points=0)
    for nm in np.unique(names[types == 1]):
        idx = np.nonzero(names == nm)[0]
        x = xyz[idx]
        sq = np.float64(np.float32(x[:, 0].max() - x[:, 0].min())) * np.float64(np.float32(x[:, 1].max() - x[:, 1].min()))
        if not sq > np.float64(np.float32(P.car_square)):
            continue
        c, cnc, cseg, cst = run(rg, x, "min-key", curv=curv)
        cls[idx] = BUILDING if c == 3 else TREE
        nc[idx] = cnc
        seg[idx] = idx[cseg]
        st["candidate_clusters"] += 1
        st["building_clusters"] += c == 3
        st["candidate_points"] += len(idx)
        st["kept_edges"] += cst["edges"]
        st["hbm_clusters"] += len(idx) > 8192
        st["tail_points"] += cst["tail"]
    return cls, nc, seg, st


def _xyz(apri):
    return np.stack([apri["x"], apri["y"], apri["z"]], -1).astype(np.float32)


def _check_scan(ctx, rg, P, s, apri, curv=1.2):
    n = len(apri)
    names = ctx.batch_fetch_clusters(s, n)
    types = ctx.batch_fetch_cluster_types(s, n, car_label=CAR, other_label=1)
    cls, nc, seg, st = expected(rg, P, _xyz(apri), names, types, curv)
    got_nc, got_seg = ctx.batch_fetch_region_growing(s, n)
    assert np.array_equal(_canon(got_nc), _canon(nc)), int((_canon(got_nc) != _canon(nc)).any(1).sum())
    assert np.array_equal(got_seg, seg), int((got_seg != seg).sum())
    assert np.array_equal(ctx.batch_fetch_cluster_classes(s, n, CAR, BUILDING, TREE), cls)
    return st


def _add(a, b):
    for k in b:
        a[k] = a.get(k, 0) + b[k]


def _batch(scvod, kind):
    import synth
    import torch
    preset, seq, first, count, stride = JOBS[kind]
    P = scvod.make_params(preset)
    scans = [synth.make_scan(seq, first + k * stride, kind, device="cuda") for k in range(count)]
    d = torch.cat([sc[0] for sc in scans]).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(sc[0]) for sc in scans])]).astype(np.int32)
    return P, d, offs, count


def _run(scvod, P, d, offs, count, rgrow=None, merge=None):
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=count)
    if merge is not None:
        ctx.set_intensity_merge(*merge)
    if rgrow is not None:
        ctx.set_region_growing(*rgrow)
    ctx.batch_process(d, offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    return ctx


@pytest.mark.parametrize("kind", ["K64", "PARK", "OS128"])
def test_real_batches_equal_the_helper(scvod, rg, kind):
    P, d, offs, count = _batch(scvod, kind)
    ctx = _run(scvod, P, d, offs, count, rgrow=(True,))
    want = {}
    for s in range(count):
        _add(want, _check_scan(ctx, rg, P, s, ctx.batch_fetch(s)["apri"]))
    got = ctx.batch_region_growing_stats()
    assert {k: got[k] for k in want} == want, (got, want)
    assert got["candidate_clusters"] > 0 and got["max_rounds"] >= 1
    ctx.close()


def test_low_curvature_threshold_takes_the_tail(scvod, rg):
    P, d, offs, count = _batch(scvod, "PARK")
    ctx = _run(scvod, P, d, offs, count, rgrow=(True, 10, 20, 10.0, 0.02, 0.2))
    want = {}
    for s in range(count):
        _add(want, _check_scan(ctx, rg, P, s, ctx.batch_fetch(s)["apri"], curv=0.02))
    got = ctx.batch_region_growing_stats()
    assert {k: got[k] for k in want} == want and got["tail_points"] > 0
    ctx.close()


def test_merge_and_region_growing_together(scvod, rg):
    P, d, offs, count = _batch(scvod, "K64")
    ctx = _run(scvod, P, d, offs, count, rgrow=(True,), merge=(3, 2, 2.0, 1.0))
    assert ctx.batch_cluster_merge_stats()["fusions"] > 0
    want = {}
    for s in range(count):
        _add(want, _check_scan(ctx, rg, P, s, ctx.batch_fetch(s)["apri"]))
    got = ctx.batch_region_growing_stats()
    assert {k: got[k] for k in want} == want
    ctx.close()


@pytest.mark.parametrize("kind", ["K64", "PARK"])
def test_stage_on_leaves_every_output_as_it_was(scvod, kind):
    P, d, offs, count = _batch(scvod, kind)
    a = _run(scvod, P, d, offs, count)
    b = _run(scvod, P, d, offs, count, rgrow=(True,))
    a.set_timing(True)
    a.batch_cluster_types()
    assert not any(nm.startswith("rg_") for nm, _ in a.timings())
    a.set_timing(False)
    for s in range(count):
        n = a.batch_fetch(s)["n_apri"]
        assert np.array_equal(a.batch_fetch_clusters(s, n), b.batch_fetch_clusters(s, n))
        ta = a.batch_fetch_cluster_types(s, n)
        assert np.array_equal(ta, b.batch_fetch_cluster_types(s, n))
        ca = a.batch_fetch_cluster_classes(s, n, CAR, BUILDING, TREE)
        assert np.array_equal(ca, np.where(ta == 1, TREE, ta))             # off: other -> tree, never building
        cb = b.batch_fetch_cluster_classes(s, n, CAR, BUILDING, TREE)
        assert np.array_equal(ca == TREE, (cb == TREE) | (cb == BUILDING))
    assert a.batch_region_growing_stats()["candidate_clusters"] == 0
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
    a.close()
    b.close()


def _scene(rng, parts):
    pts = np.concatenate(parts).astype(np.float32)
    return np.concatenate([pts, rng.uniform(0, 50, (len(pts), 1)).astype(np.float32)], 1)


def _wall(rng, n, length, height, at=(6.0, 6.0)):
    t = rng.uniform(0, length, n)
    return np.stack([at[0] + t * 0.7071, at[1] + t * 0.7071, rng.uniform(-1.6, -1.6 + height, n)], -1)


def _hand_built(scvod, oracle, rg, pts):
    P = scvod.make_params("semantickitti")
    apri = oracle.bin(P, pts, True)["apri"]
    ctx = scvod.Ctx(P, max_points_total=len(pts) + 64, max_scans=1)
    ctx.set_region_growing(True)
    ctx.cluster(apri)
    ctx.batch_cluster_types()
    st = _check_scan(ctx, rg, P, 0, apri)
    got = ctx.batch_region_growing_stats()
    assert {k: got[k] for k in st} == st
    names = ctx.batch_fetch_clusters(0, len(apri))
    cls = ctx.batch_fetch_cluster_classes(0, len(apri), CAR, BUILDING, TREE)
    ctx.close()
    return apri, names, cls, got


def test_hand_built_scenes(scvod, oracle, rg):
    rng = np.random.default_rng(5)
    wall = _wall(rng, 3000, 8.0, 3.0)
    bush = rng.normal(0, 0.8, (1500, 3)) * [1.5, 1.5, 0.8] + [-8.0, 7.0, -0.8]
    bush = bush[rng.random(len(bush)) < 0.6]
    sparse = np.stack([np.linspace(-8, -5.5, 15), np.linspace(-8, -5.5, 15), np.linspace(-1.6, -0.8, 15)], -1)  # large box, < 20 points
    dup = np.repeat(_wall(rng, 200, 4.0, 2.0, at=(-6.0, -12.0)), 4, axis=0)
    apri, names, cls, st = _hand_built(scvod, oracle, rg, _scene(rng, [wall, bush, sparse, dup]))
    xyz = _xyz(apri)
    def cls_near(c):
        i = np.argmin(((xyz - np.asarray(c, np.float32)) ** 2).sum(1))
        return cls[i]
    assert cls_near([6.0 + 4 * 0.7071, 6.0 + 4 * 0.7071, -0.5]) == BUILDING
    assert cls_near([-8.0, 7.0, -0.8]) == TREE
    assert st["candidate_clusters"] >= 2 and st["building_clusters"] >= 1


def test_cluster_beyond_the_lds_path(scvod, oracle, rg):
    rng = np.random.default_rng(9)
    facade = _wall(rng, 70000, 20.0, 5.0, at=(4.0, 4.0))
    apri, names, cls, st = _hand_built(scvod, oracle, rg, _scene(rng, [facade]))
    assert st["hbm_clusters"] >= 1 and st["candidate_points"] >= 60000
    assert (cls == BUILDING).sum() >= 60000


def test_invalid_arguments(scvod):
    P = scvod.make_params("semantickitti")
    ctx = scvod.Ctx(P, max_points_total=1024, max_scans=1)
    for bad in [(True, 0), (True, 17), (True, 10, 0), (True, 10, 20, 0.0), (True, 10, 20, 90.5), (True, 10, 20, 10.0, 1.2, -0.1),
                (True, 10, 20, 10.0, 1.2, 1.5)]:
        with pytest.raises(Exception):
            ctx.set_region_growing(*bad)
    ctx.set_region_growing(True, 16, 1, 90.0, 0.0, 1.0)
    ctx.set_region_growing(False)
    ctx.close()


def test_facade_reports_a_building_on_the_wall_scene(scvod, tmp_path):
    """the facade's SSC::segDF with ssc/device_region_growing_: 1 (host/scvod_sequence): the wall is a building cluster"""
    import importlib.util
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("sequence_demo", os.path.join(root, "tools", "sequence_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    exe = os.path.join(root, "dr-using-scv-od_amd", "host", "scvod_sequence")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    rng = np.random.default_rng(2)
    P = scvod.PRESETS["semantickitti"]
    os.makedirs(tmp_path / "velodyne")
    os.makedirs(tmp_path / "labels")
    with open(tmp_path / "poses.txt", "w") as pf:
        for k in range(2):
            r, a = rng.uniform(3, 30, 20000), rng.uniform(0, 2 * np.pi, 20000)
            ground = np.stack([r * np.cos(a), r * np.sin(a), np.full(20000, -P["sensor_height"])], -1)
            wall = _wall(rng, 6000, 10.0, 3.5)
            x = np.concatenate([ground, wall]).astype(np.float32)
            x = np.concatenate([x, rng.uniform(0, 1, (len(x), 1)).astype(np.float32)], 1)
            x.tofile(tmp_path / "velodyne" / f"{k:06d}.bin")
            np.concatenate([np.full(20000, 40), np.full(6000, 50)]).astype(np.uint32).tofile(tmp_path / "labels" / f"{k:06d}.label")
            pf.write(" ".join(repr(float(v)) for v in [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]) + "\n")
    cfg = tmp_path / "cfg.yaml"
    text = demo.YAML.format(skip=1, count=2, data=str(tmp_path / "velodyne"), labels=str(tmp_path / "labels"),
                            poses=str(tmp_path / "poses.txt"), **P)
    cfg.write_text(text + "  device_region_growing_: 1\n")
    res = subprocess.run([exe, str(cfg), str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    frames = [l.split() for l in res.stdout.splitlines() if l.startswith("frame ")]
    assert len(frames) == 2
    for f in frames:
        assert int(f[f.index("buildings") + 1]) >= 1, res.stdout
