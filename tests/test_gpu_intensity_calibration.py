"""The intensity calibration on the device (csrc/scvod_k_calib.inc, scvod_set_intensity_calibration) against the CPU restatement of
SSC::intensityCalibrationByCurvature (tests/helpers/intensity_calibration_ref.cpp), bit for bit: normals, curvatures and calibrated
intensities on K64 / PARK / OS128 batches, on hand-built scenes and across the chunks of a large uneven batch; the apri records and
voxel descriptors that follow; the intensity merge on the calibrated descriptors; the stage off leaving every output as it was; the
stage on leaving everything that does not read an intensity as it was; the settings it refuses; the facade key.
NaNs are compared as NaNs (every NaN pattern is mapped to one: the sign of 0/0 differs between the host and the device)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import intensity_merge_ref as imr  # noqa: E402
from test_intensity_calibration_ref import STAT_KEYS, build_ic, run  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dr-using-scv-od_amd", "host")
JOBS = {"K64": ("semantickitti", 5, 300, 3, 7), "PARK": ("parkinglot", 3, 30, 3, 3), "OS128": ("os128_fine", 5, 302, 2, 1)}
CAL = (True, 10, 200.0)


@pytest.fixture(scope="module")
def ic(tmp_path_factory):
    return build_ic(tmp_path_factory.mktemp("icref"))


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def _batch(scvod, kind):
    import synth
    import torch
    preset, seq, first, count, stride = JOBS[kind]
    P = scvod.make_params(preset)
    scans = [synth.make_scan(seq, first + k * stride, kind, device="cuda") for k in range(count)]
    d = torch.cat([sc[0] for sc in scans]).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(sc[0]) for sc in scans])]).astype(np.int32)
    return P, d, offs, count


def _ground(seed=0, n=6000):
    rng = np.random.default_rng(seed)
    r = rng.uniform(3, 45, n)
    a = rng.uniform(0, 2 * np.pi, n)
    return np.stack([r * np.cos(a), r * np.sin(a), -1.73 + rng.normal(0, 0.01, n), np.full(n, 5.0)], -1).astype(np.float32)


def _wall(x0, y0, y1, z0, z1, step, inten):
    y, z = np.meshgrid(np.arange(y0, y1, step), np.arange(z0, z1, step), indexing="ij")
    return np.stack([np.full(y.size, x0), y.ravel(), z.ravel(), np.full(y.size, inten)], -1).astype(np.float32)


def _scenes():
    """hand-built scans (a flat ground that Patchwork takes away, and what stands on it) and the size of their non-ground clouds"""
    g = _ground()
    rng = np.random.default_rng(3)
    a, b, c = np.meshgrid(np.arange(12), np.arange(12), np.arange(8), indexing="ij")
    lat = np.stack([6 + a.ravel() * 0.25, -1.5 + b.ravel() * 0.25, -1.0 + c.ravel() * 0.25, 50 + (a.ravel() % 5) * 60], -1).astype(np.float32)
    cat = lambda *p: np.concatenate([np.asarray(q, np.float32).reshape(-1, 4) for q in p]).astype(np.float32)
    return [("empty", g, 0),
            ("one_point", cat(g, [[5, 0, 1, 10]]), 1),
            ("two_points", cat(g, [[5, 0, 1, 10], [5.05, 0.02, 1.4, 250]]), 2),
            ("dense_near_wall", cat(g, _wall(3.5, -3, 3, -1.6, 2.0, 0.02, 120.0)), 51300),
            ("sparse_far_wall", cat(g, _wall(38.0, -20, 20, -1.5, 3.0, 0.9, 60.0), _wall(3.5, -1, 1, -1.6, 1.0, 0.05, 230.0)), 2193),
            ("duplicates", cat(g, np.tile([[6, 1, 0.5, 33]], (500, 1)), np.tile([[6.5, 1, 0.5, 300]], (40, 1))), 540),
            ("lattice", cat(g, lat[rng.permutation(len(lat))]), 1152)]


def _check_scan(ctx, ic, oracle, P, s, x, cal, want_stats, vox=True):
    """scan s (input cloud x) of a calibrated batch against the helper; returns (fetch result, helper intensities per apri point)"""
    r = ctx.batch_fetch(s)
    ng = r["nonground_idx"]
    nc, inten, _, st = run(ic, x[ng], k=cal[1], max_int=cal[2])
    got_nc, got_int = ctx.batch_fetch_intensity_calibration(s, len(ng))
    print(f"scan {s}: {len(ng)} non-ground points, normal/curvature words that differ {int((_bits(got_nc) != _bits(nc)).sum())}, "
          f"intensities that differ {int((_bits(got_int) != _bits(inten)).sum())}")
    assert np.array_equal(_bits(got_nc), _bits(nc))
    assert np.array_equal(_bits(got_int), _bits(inten))
    for k in STAT_KEYS:
        want_stats[k] = want_stats.get(k, 0) + st[k]
    pos = np.full(len(x), -1, np.int64)
    pos[ng] = np.arange(len(ng))
    src = r["apri_src"]
    assert (pos[src] >= 0).all()
    apri = r["apri"]
    assert np.array_equal(np.stack([apri["x"], apri["y"], apri["z"]], -1).view(np.uint32), x[src, :3].view(np.uint32))
    want_int = inten[pos[src]]
    assert np.array_equal(_bits(apri["intensity"]), _bits(want_int))
    if vox:
        fed = apri.copy()
        fed["intensity"] = want_int
        v = oracle.voxelize(P, fed)
        assert np.array_equal(r["vox_key"], v["vox_key"]) and np.array_equal(r["vox_pts"], v["vox_pts"])
        assert np.array_equal(_bits(r["vox_av"]), _bits(v["vox_av"]))
        assert np.array_equal(_bits(r["vox_cov"]), _bits(v["vox_cov"]))
    return r, want_int


@pytest.mark.parametrize("kind", ["K64", "PARK", "OS128"])
def test_batches_equal_the_helper(scvod, oracle, ic, kind):
    P, d, offs, count = _batch(scvod, kind)
    x = d.cpu().numpy()
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=count)
    ctx.set_intensity_calibration(*CAL)
    ctx.batch_process(d, offs)
    want = {}
    for s in range(count):
        _check_scan(ctx, ic, oracle, P, s, x[offs[s]:offs[s + 1]], CAL, want)
    got = ctx.batch_intensity_calibration_stats()
    assert {k: got[k] for k in want} == want, (got, want)
    assert got["points"] > 0 and got["cos_floored"] > 0 and ctx.batch_intensity_calibration_candidates() >= got["points"]
    if kind == "K64":  # both readers of a run (the staged tile, the sorted copy) and a ring beyond the tile were exercised
        assert 0 < got["fallback_queries"] < got["points"] and got["max_ring"] >= 2, got
    ctx.close()


@pytest.mark.parametrize("cal", [(True, 10, 200.0), (True, 3, 255.0), (True, 16, 100.0)])
def test_hand_built_scenes_equal_the_helper(scvod, oracle, ic, cal):
    import torch
    P = scvod.make_params("semantickitti")
    scenes = _scenes()
    xs = [sc[1] for sc in scenes]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
    d = torch.from_numpy(np.concatenate(xs)).cuda().contiguous()
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=len(xs))
    ctx.set_intensity_calibration(*cal)
    ctx.batch_process(d, offs)
    want = {}
    for s, (name, x, n_ng) in enumerate(scenes):
        r, _ = _check_scan(ctx, ic, oracle, P, s, x, cal, want)
        assert r["n_nonground"] == n_ng, (name, r["n_nonground"])
    got = ctx.batch_intensity_calibration_stats()
    assert {k: got[k] for k in want} == want, (got, want)
    assert got["nan_normals"] >= 1 + 2 + 540   # one point, two points, the duplicates
    ctx.close()
    # the per-scan entry point honours the setting too
    one = scvod.Ctx(P, max_points_total=len(xs[6]) + 16, max_scans=1)
    one.set_intensity_calibration(*cal)
    r1 = one.process_scan(xs[6])
    ng = r1["nonground_idx"]
    _, inten, _, _ = run(ic, xs[6][ng], k=cal[1], max_int=cal[2])
    pos = np.full(len(xs[6]), -1, np.int64)
    pos[ng] = np.arange(len(ng))
    assert np.array_equal(_bits(r1["apri"]["intensity"]), _bits(inten[pos[r1["apri_src"]]]))
    one.close()


def test_uneven_batch_across_the_chunks(scvod, oracle, ic):
    """more than 2^22 points (the chunk of the stage's scratch) in scans of very different sizes, the small ones at the chunk borders"""
    import synth
    import torch
    P = scvod.make_params("semantickitti")
    small = [sc[1] for sc in _scenes() if sc[0] in ("empty", "one_point", "two_points", "lattice")]
    big = [synth.make_scan(5, 400 + 3 * k, "K64", device="cuda")[0] for k in range(38)]
    parts = []
    for k, b in enumerate(big):
        parts.append(b)
        if k % 9 == 0:
            parts.extend(torch.from_numpy(x).cuda() for x in small)
    d = torch.cat(parts).contiguous()
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
    assert offs[-1] > (1 << 22) + 200000
    x = d.cpu().numpy()
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=len(parts))
    ctx.set_intensity_calibration(*CAL)
    ctx.batch_process(d, offs)
    want = {}
    for s in range(len(parts)):
        _check_scan(ctx, ic, oracle, P, s, x[offs[s]:offs[s + 1]], CAL, want)
    got = ctx.batch_intensity_calibration_stats()
    assert {k: got[k] for k in want} == want, (got, want)
    ctx.close()


@pytest.mark.parametrize("kind", ["K64", "OS128"])
def test_merge_reads_the_calibrated_descriptors(scvod, oracle, kind):
    P, d, offs, count = _batch(scvod, kind)
    grid = tuple(int(g) for g in oracle.grid_dims(P)[:3])
    pre = []
    base = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=count)
    base.set_intensity_calibration(*CAL)
    base.batch_process(d, offs)
    base.batch_cluster()
    for s in range(count):
        pre.append(base.batch_fetch_clusters(s, base.batch_fetch(s)["n_apri"]))
    base.close()
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=count)
    ctx.set_intensity_calibration(*CAL)
    ctx.set_intensity_merge(3, 2, 2.0, 1.0)
    ctx.batch_process(d, offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    raw = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=count)
    raw.set_intensity_merge(3, 2, 2.0, 1.0)
    raw.batch_process(d, offs)
    raw.batch_cluster()
    differs = 0
    for s in range(count):
        r = ctx.batch_fetch(s)   # (its intensities equal the helper's: test_batches_equal_the_helper)
        vox = oracle.voxelize(P, r["apri"])
        want = imr.convention(vox, pre[s], grid, 3, 2, 2.0, 1.0, stats={})
        got = ctx.batch_fetch_clusters(s, r["n_apri"])
        assert np.array_equal(got, want)
        differs += int((got != raw.batch_fetch_clusters(s, r["n_apri"])).sum())
    print("points whose fused cluster differs from the merge on raw intensities:", differs)
    ctx.close()
    raw.close()


def _everything(scvod, P, d, offs, count, setup):
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=count)
    setup(ctx)
    ctx.batch_process(d, offs)
    ctx.batch_cluster()
    ctx.batch_cluster_types()
    T = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(-1), count)
    ctx.batch_track(T)
    out = []
    for s in range(count):
        r = ctx.batch_fetch(s)
        n = r["n_apri"]
        tr = ctx.batch_fetch_track(s)
        out.append(dict(r=r, names=ctx.batch_fetch_clusters(s, n), types=ctx.batch_fetch_cluster_types(s, n), track={k: np.asarray(v) for k, v in tr.items()}))
    return ctx, ctx.batch_counts(), out


INTENSITY_FIELDS = ("apri", "vox_av", "vox_cov")


def _same(a, b, skip=()):
    for k in a["r"]:
        if k in skip:
            continue
        va, vb = a["r"][k], b["r"][k]
        if isinstance(va, np.ndarray):
            assert np.array_equal(np.ascontiguousarray(va).view(np.uint8), np.ascontiguousarray(vb).view(np.uint8)), k
        else:
            assert va == vb, k
    assert np.array_equal(a["names"], b["names"]) and np.array_equal(a["types"], b["types"])
    for k in a["track"]:
        assert np.array_equal(a["track"][k], b["track"][k]), k


@pytest.mark.parametrize("kind", ["K64", "PARK"])
def test_stage_off_is_identical(scvod, kind):
    P, d, offs, count = _batch(scvod, kind)
    never, c0, a = _everything(scvod, P, d, offs, count, lambda c: None)
    off, c1, b = _everything(scvod, P, d, offs, count, lambda c: c.set_intensity_calibration(False, 10, 200.0))

    def on_then_off(c):
        c.set_intensity_calibration(*CAL)
        c.set_intensity_calibration(False, 10, 200.0)
    unset, c2, e = _everything(scvod, P, d, offs, count, on_then_off)
    zeros = dict(points=0, clamped_before=0, cos_floored=0, capped_after=0, nan_normals=0, fallback_queries=0, max_ring=0)
    for ctx, other in ((off, b), (unset, e)):
        for s in range(count):
            _same(a[s], other[s])
        assert ctx.batch_intensity_calibration_stats() == zeros and ctx.batch_intensity_calibration_candidates() == 0
        assert ctx.arena_bytes() == never.arena_bytes()   # (nothing was allocated)
        with pytest.raises(Exception):
            ctx.batch_fetch_intensity_calibration(0, 1 << 20)
    assert never.batch_intensity_calibration_stats() == zeros
    assert np.array_equal(np.asarray(c0), np.asarray(c1)) and np.array_equal(np.asarray(c0), np.asarray(c2))
    for c in (never, off, unset):
        c.close()


@pytest.mark.parametrize("kind", ["K64", "PARK"])
def test_stage_on_moves_nothing_but_intensities(scvod, kind):
    P, d, offs, count = _batch(scvod, kind)
    off, c0, a = _everything(scvod, P, d, offs, count, lambda c: None)
    on, c1, b = _everything(scvod, P, d, offs, count, lambda c: c.set_intensity_calibration(*CAL))
    assert np.array_equal(np.asarray(c0), np.asarray(c1))
    moved = 0
    for s in range(count):
        _same(a[s], b[s], skip=INTENSITY_FIELDS)
        pa, pb = a[s]["r"]["apri"], b[s]["r"]["apri"]
        for f in pa.dtype.names:
            if f != "intensity":
                assert np.array_equal(pa[f].view(np.uint32), pb[f].view(np.uint32)), f
        moved += int((_bits(pa["intensity"]) != _bits(pb["intensity"])).sum())
    assert moved > 0
    assert on.batch_intensity_calibration_stats()["points"] > 0
    off.close()
    on.close()


def test_invalid_settings_are_refused_and_change_nothing(scvod, oracle, ic):
    P, d, offs, count = _batch(scvod, "PARK")
    x = d.cpu().numpy()
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=count)
    cal = (True, 7, 180.0)
    ctx.set_intensity_calibration(*cal)
    for bad in ((True, 2, 200.0), (True, 17, 200.0), (True, 10, 0.0), (True, 10, -1.0), (True, 10, float("nan")), (False, 2, 200.0)):
        assert ctx.lib.scvod_set_intensity_calibration(ctx.h, int(bad[0]), bad[1], bad[2]) == -1   # SCVOD_ERR_INVALID
        with pytest.raises(Exception):
            ctx.set_intensity_calibration(*bad)
    ctx.batch_process(d, offs)
    _check_scan(ctx, ic, oracle, P, 0, x[offs[0]:offs[1]], cal, {})
    ctx.close()


def test_facade_key_yields_the_same_voxel_descriptors(scvod, tmp_path):
    import synth
    from test_gpu_facade import YAML
    exe = os.path.join(HOST, "facade_check")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST])
    P = scvod.make_params("semantickitti")
    cfg = tmp_path / "semantickitti.yaml"
    cfg.write_text(YAML.format(**scvod.PRESETS["semantickitti"]) + "  search_num_: 8\n  device_intensity_calibration_: 1\n")
    scans = []
    for k, idx in enumerate((120, 121)):
        x = synth.make_scan(5, idx, "K64")[0].numpy()
        x.tofile(tmp_path / f"s{k}.f32")
        scans.append(x)
    pre = str(tmp_path / "out")
    res = subprocess.run([exe, str(cfg), str(tmp_path / "s0.f32"), str(tmp_path / "s1.f32"), pre], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    ctx = scvod.Ctx(P, max_points_total=max(len(x) for x in scans) + 16, max_scans=1)
    ctx.set_intensity_calibration(True, 8, 255.0)
    plain = scvod.Ctx(P, max_points_total=max(len(x) for x in scans) + 16, max_scans=1)
    for tag, x in zip(("a", "b"), scans):
        r = ctx.process_scan(x)
        apri = np.fromfile(f"{pre}_{tag}_apri.bin", scvod.APRI_DTYPE)
        assert np.array_equal(apri.view(np.uint8), r["apri"].view(np.uint8))
        rows = [l.split() for l in open(f"{pre}_{tag}_hash.txt")]
        assert [int(q[0]) for q in rows] == r["vox_key"].tolist()
        assert [int(q[5]) for q in rows] == r["vox_av"].view(np.uint32).tolist()
        assert [int(q[6]) for q in rows] == r["vox_cov"].view(np.uint32).tolist()
        use = np.fromfile(f"{pre}_{tag}_cloud_use.f32", np.float32).reshape(-1, 4)
        assert np.array_equal(use[:, 3].view(np.uint32), r["apri"]["intensity"].view(np.uint32))
        assert not np.array_equal(plain.process_scan(x)["vox_av"].view(np.uint32), r["vox_av"].view(np.uint32))
    ctx.close()
    plain.close()


def test_batch_of_empty_scans_is_a_calibrated_batch_of_no_points(scvod):
    import torch
    P = scvod.make_params("semantickitti")
    ctx = scvod.Ctx(P, max_points_total=64, max_scans=3)
    ctx.set_intensity_calibration(*CAL)
    ctx.batch_process(torch.zeros((1, 4), dtype=torch.float32, device="cuda"), np.zeros(4, np.int32))   # three scans of no points
    nc, inten = ctx.batch_fetch_intensity_calibration(1, 0)
    assert len(nc) == 0 and len(inten) == 0
    assert ctx.batch_intensity_calibration_stats()["points"] == 0 and ctx.batch_intensity_calibration_candidates() == 0
    ctx.close()


def test_sequence_driver_with_the_key_equals_a_batch_ctx(scvod, ic, tmp_path):
    """the facade's SSC::segDF (host/scvod_sequence: one process() per frame) with ssc/device_intensity_calibration_: 1 against
    scvod_batch_process on the frames the driver loaded: cloud_use = the kept points with the batch's calibrated intensities"""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("sequence_demo", os.path.join(ROOT, "tools", "sequence_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    exe = os.path.join(HOST, "scvod_sequence")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", HOST])
    rng = np.random.default_rng(2)
    PR = scvod.PRESETS["semantickitti"]
    os.makedirs(tmp_path / "velodyne")
    os.makedirs(tmp_path / "labels")
    os.makedirs(tmp_path / "out")
    with open(tmp_path / "poses.txt", "w") as pf:
        for k in range(2):
            g = _ground(seed=10 + k, n=20000)
            w = _wall(9.0 + k, -4, 4, -1.6, 2.4, 0.07, 0.0)
            x = np.concatenate([g, w]).astype(np.float32)
            x[:, 3] = rng.uniform(0, 1, len(x)).astype(np.float32)
            x.tofile(tmp_path / "velodyne" / f"{k:06d}.bin")
            np.concatenate([np.full(len(g), 40), np.full(len(w), 50)]).astype(np.uint32).tofile(tmp_path / "labels" / f"{k:06d}.label")
            pf.write(" ".join(repr(float(v)) for v in [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]) + "\n")
    cfg = tmp_path / "cfg.yaml"
    text = demo.YAML.format(skip=1, count=2, data=str(tmp_path / "velodyne"), labels=str(tmp_path / "labels"), poses=str(tmp_path / "poses.txt"), **PR)
    cfg.write_text(text + "  search_num_: 12\n  device_intensity_calibration_: 1\n")
    res = subprocess.run([exe, str(cfg), str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    frames = [l.split() for l in res.stdout.splitlines() if l.startswith("frame ")]
    assert len(frames) == 2 and "intensity_calibration search_num 12" in res.stdout
    mx = float([l for l in res.stdout.splitlines() if l.startswith("intensity_calibration")][0].split()[-1])
    clouds = [np.fromfile(tmp_path / "out" / f"{f[1]}_cloud.f32", np.float32).reshape(-1, 4) for f in frames]
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    P = scvod.make_params("semantickitti")
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=2)
    ctx.set_intensity_calibration(True, 12, mx)
    ctx.batch_process(torch.from_numpy(np.concatenate(clouds)).cuda().contiguous(), offs)
    moved = 0
    for s, f in enumerate(frames):
        r = ctx.batch_fetch(s)
        use = np.fromfile(tmp_path / "out" / f"{f[1]}_cloud_use.f32", np.float32).reshape(-1, 4)
        assert len(use) == r["n_apri"] > 1000
        assert np.array_equal(use[:, :3].view(np.uint32), clouds[s][r["apri_src"], :3].view(np.uint32))
        assert np.array_equal(_bits(use[:, 3]), _bits(r["apri"]["intensity"]))
        ng = r["nonground_idx"]
        _, inten, _, _ = run(ic, clouds[s][ng], k=12, max_int=mx)
        pos = np.full(len(clouds[s]), -1, np.int64)
        pos[ng] = np.arange(len(ng))
        assert np.array_equal(_bits(use[:, 3]), _bits(inten[pos[r["apri_src"]]]))
        moved += int((_bits(use[:, 3]) != _bits(clouds[s][r["apri_src"], 3])).sum())
    assert moved > 0
    ctx.close()
