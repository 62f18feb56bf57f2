"""The lean emission of a batch: the arrange pass bins the kept non-ground points, k_emit only compacts.

By default a batch entry runs k_pw_fit_coop / k_pw_arrange in their LEAN form: a point that passed the range/FOV test gets its packed
index triple (pack_idx3) staged next to its seg word, and k_emit<true> compacts the staged words -- no gather from the input cloud, no
apri_int.  The intensities are filled by k_apri_intensity when somebody needs them (ensure_intensities: the on-demand descriptors).  A
ctx that computes its descriptors in the voxel stage (scvod_set_voxel_descriptors(1)), calibrates or merges by intensity when the batch
is processed, and a grid beyond the packed triple's limits keep the eager form (k_emit<false>, the gather).  Both forms must agree bit
for bit in everything a caller can fetch:

  1. lean == eager on 12 scans (k_pw_fit_coop<16>) and on 3 scans (k_pw_fit_coop<64>) whose patches cover the three arrange variants,
     and the default ctx's PointAPRI records == the oracle's;
  2. the same on a scan with crafted points: next to sector / azimuth edges, y == +-0, z == 0, dis == min_dis (range index -1), a tilted
     patch (status 2) and an elevated rough one (status 3);
  3. the intensities on demand: descriptors, a calibration turned on afterwards, a merge turned on between process and cluster, and no
     second intensity pass for a second fetch;
  4. a grid with more than 2044 sectors takes the gather form and equals the oracle;
  5. (not gpu) the bound behind the lean form: the key recomputed from the packed triple is apri_of_point's voxel_idx.

The compact arrays apri_key / apri_idx3 and the irregular list (scan_irr, irr_list) have no fetch of their own; they are compared through
everything computed from them: apri_key per point is rebuilt from the fetched voxel arrays (vox_key of the voxel that lists the point),
apri_idx3 / scan_irr / irr_list feed the clustering and its max_name pass, whose names, counters and last names are compared."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGE = (3, 2, 2.0, 1.0)
CAL = (True, 10, 200.0)
FETCHED = ("cls", "ground_idx", "nonground_idx", "planes", "apri", "apri_src", "rejected_src", "vox_key", "vox_pt_begin", "vox_pts",
           "vox_av", "vox_cov")
CLUSTER_RESULTS = ("scans_approximated", "nodes_concerned", "exact", "scans_on_hbm_forest", "runs_settled_by_rule", "runs_clustered_again")
_CACHE = {}


# ---- input ------------------------------------------------------------------------------------------------------------------------------

def _ground(rng, n, r0, r1, t0, t1, h, noise=0.02):
    r, t = rng.uniform(r0, r1, n), rng.uniform(t0, t1, n)
    return np.stack([r * np.cos(t), r * np.sin(t), -h + rng.normal(0, noise, n)], 1)


def _scan(P, seed, n_sparse, crafted=None, clear=()):
    """A K64-like scan of 4-8 k points: sparse ground all around (patches of a few to a few dozen points), one patch of the first ring
    with 600-900 ground points (>= 512: the cooperative fit), one with 150-300 (64..511), walls and boxes standing on the ground --
    some inside the two dense patches, so that both hold a non-ground part -- and clutter above.  Intensities log-uniform."""
    rng = np.random.default_rng(seed)
    h = P.sensor_height
    sparse = _ground(rng, n_sparse, 2.8, 45.0, 0.0, 2 * np.pi, h)
    for t0, t1 in clear:                                                                # (sectors a crafted patch has to itself)
        t = np.arctan2(sparse[:, 1], sparse[:, 0]) % (2 * np.pi)
        sparse = sparse[~((t >= t0) & (t < t1) & (np.hypot(sparse[:, 0], sparse[:, 1]) < 7.6))]
    parts = [sparse,
             _ground(rng, int(rng.integers(600, 900)), 3.0, 7.0, 0.05, 0.35, h),       # zone 0, ring 0, sector 0
             _ground(rng, int(rng.integers(150, 300)), 3.0, 7.0, 0.83, 1.13, h)]       # zone 0, ring 0, sector 2
    for t0 in (0.2, 0.98):                                                              # a wall in each dense patch
        m = 120
        r, z = rng.uniform(5.0, 5.3, m), rng.uniform(-h + 0.3, 1.0, m)
        t = t0 + rng.uniform(-0.05, 0.05, m)
        parts.append(np.stack([r * np.cos(t), r * np.sin(t), z], 1))
    for _ in range(14):                                                                 # boxes
        m = int(rng.integers(60, 160))
        c = rng.uniform(-28, 28, 2)
        if np.hypot(*c) < 4.0:
            c = c + 6.0
        parts.append(np.stack([c[0] + rng.uniform(-1, 1, m), c[1] + rng.uniform(-0.6, 0.6, m), rng.uniform(-h + 0.2, 0.6, m)], 1))
    m = 300                                                                             # clutter above, some beyond the FOV / range
    r, t = rng.uniform(2.8, 34.0, m), rng.uniform(0, 2 * np.pi, m)
    parts.append(np.stack([r * np.cos(t), r * np.sin(t), rng.uniform(-1.0, 9.0, m)], 1))
    if crafted is not None:
        parts.append(crafted)
    xyz = np.concatenate(parts)
    x = np.zeros((len(xyz), 4), np.float32)
    x[:, :3] = xyz
    x[:, 3] = np.exp(rng.uniform(np.log(1e-3), np.log(255.0), len(x)))
    order = rng.permutation(len(x))
    return np.ascontiguousarray(x[order])


def _batch(P, seeds):
    scans = [_scan(P, s, 1500 + 250 * (s % 11)) for s in seeds]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    return np.concatenate(scans), offs


def _crafted_points(P):
    """points the guarded estimate must leave to the reference arithmetic, the signed zeros, and the lower range limit"""
    rng = np.random.default_rng(77)
    pts = []
    for k in range(40):                                     # within 1e-3 degrees of a sector edge
        r, z = rng.uniform(4, 12), rng.uniform(-0.8, 1.5)
        t = np.deg2rad(P.min_angle + int(rng.integers(1, 299)) * P.sector_res + rng.uniform(-1e-3, 1e-3))
        pts.append([r * np.cos(t), r * np.sin(t), z])
    for k in range(40):                                     # ... of an azimuth edge
        r, t = rng.uniform(4, 12), rng.uniform(0, 2 * np.pi)
        az = np.deg2rad(P.min_azimuth + int(rng.integers(18, 24)) * P.azimuth_res + rng.uniform(-1e-3, 1e-3))
        pts.append([r * np.cos(t), r * np.sin(t), r * np.tan(az)])
    for xx in (6.0, -6.0, 4.5, -4.5, 9.0, -9.0):
        pts.append([xx, 0.0, 0.4])                          # y == +0
        pts.append([xx, -0.0, 0.7])                         # y == -0
    for k in range(8):                                      # z == 0
        r, t = rng.uniform(4, 12), rng.uniform(0, 2 * np.pi)
        pts.append([r * np.cos(t), r * np.sin(t), 0.0])
    d = float(P.min_dis)                                    # dis == min_dis exactly (sqrt(d * d) == d): range index -1
    for z in (0.2, 0.5, 0.8):
        pts += [[0.0, d, z], [0.0, -d, z + 0.1], [d, 0.0, z], [-d, -0.0, z + 0.1]]
    return np.asarray(pts, np.float64)


def _crafted_scan(P):
    """the scan of _scan() plus the crafted points, a steep slope filling one patch (normal far from upright: status 2) and a rough,
    elevated pile filling another patch of the first ring (status 3)"""
    rng = np.random.default_rng(78)
    h = P.sensor_height
    m = 400
    r, t = rng.uniform(3.2, 7.0, m), rng.uniform(1.62, 1.9, m)                       # zone 0, ring 0, sector 4: 60 degrees of slope
    slope = np.stack([r * np.cos(t), r * np.sin(t), -h + 1.75 * (r - 3.2) + rng.normal(0, 0.01, m)], 1)
    r, t = rng.uniform(3.2, 7.0, m), rng.uniform(2.4, 2.7, m)                        # zone 0, ring 0, sector 6: half a metre up, rough
    pile = np.stack([r * np.cos(t), r * np.sin(t), -h + 0.9 + rng.uniform(-0.25, 0.25, m)], 1)
    return _scan(P, 5, 3000, crafted=np.concatenate([_crafted_points(P), slope, pile]), clear=((1.571, 1.963), (2.357, 2.748)))


# ---- running a batch --------------------------------------------------------------------------------------------------------------------

def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        return a.view(np.uint8)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _keys_per_point(r):
    """apri_key of every apri point, rebuilt from the voxel stage's output: the key of the voxel that lists the point"""
    key = np.full(r["n_apri"], np.iinfo(np.int32).min, np.int64)
    per = np.diff(r["vox_pt_begin"])
    key[r["vox_pts"]] = np.repeat(r["vox_key"].astype(np.int64), per)
    return key


def _run(scvod, P, x, offs, setup=None, after_process=None, cluster=True):
    """everything a caller can fetch of the batch, and the names of the timed launches up to the second fetch of scan 0"""
    import torch
    n = len(offs) - 1
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=n)
    if setup is not None:
        setup(ctx)
    ctx.set_timing(True)
    d = torch.from_numpy(x).cuda().contiguous()
    ctx.batch_process(d, offs)
    if after_process is not None:
        after_process(ctx)
    out = {"counts": ctx.batch_counts()}
    res = []
    for s in range(n):
        r = ctx.batch_fetch(s)
        res.append(r)
        for k in FETCHED:
            out[f"{k}[{s}]"] = np.asarray(r[k]).copy()
        out[f"apri_key[{s}]"] = _keys_per_point(r)
    first = [name for name, _ in ctx.timings()]
    ctx.batch_fetch(0)
    second = [name for name, _ in ctx.timings()]
    if cluster:
        ctx.batch_cluster()
        for s in range(n):
            out[f"clusters[{s}]"] = ctx.batch_fetch_clusters(s, res[s]["n_apri"])
        cs = ctx.batch_cluster_stats()
        out["cluster_stats"] = np.asarray([int(cs[k]) for k in CLUSTER_RESULTS])
        ln, lst = ctx.batch_cluster_last_name(n)
        out["last_name"] = ln
        out["last_name_stats"] = np.asarray([lst["unknown_too_large"], lst["unknown_irregular"]])
        ms = ctx.batch_cluster_merge_stats()
        out["merge_stats"] = np.asarray([ms[k] for k in sorted(ms)])
    ctx.close()
    torch.cuda.synchronize()
    return out, res, first, second


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), f"{what}: {k} differs"


def _case(scvod, name):
    """the two synthetic batches and the crafted scan, each run once in the default (lean) and once in the eager ctx"""
    if name not in _CACHE:
        kw = dict(min_dis=3.0) if name == "crafted" else {}    # (Patchwork drops everything nearer than 2.7 m: min_dis has to lie beyond)
        P = scvod.make_params("semantickitti", **kw)
        if name == "crafted":
            x = _crafted_scan(P)
            offs = np.asarray([0, len(x)], np.int32)
        else:
            x, offs = _batch(P, range(12) if name == "B12" else range(20, 23))
        lean = _run(scvod, P, x, offs)
        eager = _run(scvod, P, x, offs, setup=lambda c: c.set_voxel_descriptors(1))
        _CACHE[name] = (P, x, offs, lean, eager)
    return _CACHE[name]


def _check_forms(lean, eager, n):
    """the default ctx emitted lean (its first fetch ran the intensity pass, once), the mode-1 ctx eagerly"""
    assert lean[2].count("emit") == 1 and eager[2].count("emit") == 1
    assert lean[2].count("emit_intensity") == 1 and lean[2].count("vx_descriptors") == 1
    assert lean[3].count("emit_intensity") == 1 and lean[3].count("vx_descriptors") == 1, "a second fetch ran the passes again"
    assert "emit_intensity" not in eager[3] and "vx_descriptors" not in eager[3]


def _check_oracle(oracle, P, x, offs, res):
    for s, r in enumerate(res):
        xs = x[offs[s]:offs[s + 1]]
        o = oracle.patchwork(P, xs, 1)
        assert np.array_equal(r["nonground_idx"], o["nonground_idx"]) and np.array_equal(r["ground_idx"], o["ground_idx"])
        b = oracle.bin(P, xs[o["nonground_idx"]], True)
        assert np.array_equal(r["apri"].view(np.uint8), b["apri"].view(np.uint8)), f"scan {s}: PointAPRI records differ from the oracle"
        assert np.array_equal(r["apri_src"], o["nonground_idx"][b["src"]])
        v = oracle.voxelize(P, b["apri"])
        for k in ("vox_key", "vox_pt_begin", "vox_pts", "vox_av", "vox_cov"):
            assert np.array_equal(_bits(r[k]), _bits(v[k])), f"scan {s}: {k} differs from the oracle"


# ---- 1. lean against eager, bit for bit ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["B12", "B3"])
def test_lean_equals_eager_and_the_oracle(scvod, oracle, name):
    P, x, offs, lean, eager = _case(scvod, name)
    n = len(offs) - 1
    assert (n > 8) == (name == "B12"), "B > 8 selects k_pw_fit_coop<16>, a handful of scans k_pw_fit_coop<64>"
    sizes = np.concatenate([r["planes"]["n_pts"] for r in lean[1]])
    npts = np.diff(offs)
    assert npts.min() >= 4000 and npts.max() <= 8000
    assert ((sizes > 0) & (sizes < 64)).sum() > 50 and ((sizes >= 64) & (sizes < 512)).sum() >= n and (sizes >= 512).sum() >= n
    assert lean[0]["counts"][:, 4].min() > 500 and lean[0]["counts"][:, 5].min() > 0      # kept and rejected points in every scan
    _check_forms(lean, eager, n)
    _same(lean[0], eager[0], name)
    _check_oracle(oracle, P, x, offs, lean[1])
    for s, r in enumerate(lean[1]):                             # the rebuilt keys are the records' voxel_idx
        assert np.array_equal(lean[0][f"apri_key[{s}]"], r["apri"]["voxel_idx"].astype(np.int64))


# ---- 2. crafted points ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_crafted_points_and_rejected_patches(scvod, oracle, spec_lean):
    P, x, offs, lean, eager = _case(scvod, "crafted")
    # the input holds what it was crafted for: checked on the CPU first
    o = oracle.patchwork(P, x, 1)
    status = o["planes"]["status"]
    assert (status == 2).sum() >= 1 and (status == 3).sum() >= 1 and (status == 1).sum() > 50, np.bincount(status)
    b = oracle.bin(P, x[o["nonground_idx"]], True)
    a = b["apri"]
    R, S, Az, _ = scvod.grid_dims(P)
    outside = (a["range_idx"] < 0) | (a["range_idx"] >= R) | (a["sector_idx"] < 0) | (a["sector_idx"] >= S) | (a["azimuth_idx"] < 0) | (a["azimuth_idx"] >= Az)
    assert (a["range_idx"] == -1).sum() >= 4 and outside.sum() >= 4, "no kept point with an out-of-grid triple in the input"
    kept = x[o["nonground_idx"]][b["src"]]
    assert ((kept[:, 1] == 0) & ~np.signbit(kept[:, 1])).sum() >= 3 and ((kept[:, 1] == 0) & np.signbit(kept[:, 1])).sum() >= 3
    assert (kept[:, 2] == 0).sum() >= 6
    st = _spec_compare(spec_lean, scvod, P, kept[:, :3])
    assert st[10] >= 60, "the points next to the bin edges were decided by the estimate after all"
    # a rejected patch's ground part joins the non-ground stream: more non-ground points than the final plane test alone leaves
    rej = np.isin(status, (2, 3))
    assert lean[1][0]["n_nonground"] >= int(o["planes"]["n_pts"][rej].sum()) > 500
    _check_forms(lean, eager, 1)
    _same(lean[0], eager[0], "crafted")
    _check_oracle(oracle, P, x, offs, lean[1])
    # the irregular points reached the clustering's max_name pass in both forms alike (same last names above); and there are some
    assert (lean[1][0]["apri"]["range_idx"] == -1).sum() == (a["range_idx"] == -1).sum()


# ---- 3. intensities on demand -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_intensities_on_demand(scvod):
    import torch
    P, x, offs, lean, eager = _case(scvod, "B3")
    n = len(offs) - 1
    # descriptors fetched on demand == the eager ctx's bits, one intensity pass (test 1 compared vox_av / vox_cov; here: that they vary)
    for s in range(n):
        assert np.array_equal(_bits(lean[0][f"vox_av[{s}]"]), _bits(eager[0][f"vox_av[{s}]"]))
        assert len(np.unique(lean[0][f"vox_av[{s}]"])) > 100 and (lean[0][f"vox_cov[{s}]"] > 0).sum() > 50
    assert lean[3].count("emit_intensity") == 1
    # the merge turned on between process and cluster: the clustering asks for descriptors, hence intensities, itself
    want = _run(scvod, P, x, offs, setup=lambda c: (c.set_voxel_descriptors(1), c.set_intensity_merge(*MERGE)))
    late = _run(scvod, P, x, offs, after_process=lambda c: c.set_intensity_merge(*MERGE))
    assert late[2].count("emit_intensity") == 1 and "emit_intensity" not in want[3]
    assert want[0]["merge_stats"].tolist() != eager[0]["merge_stats"].tolist(), "the merge fused nothing: the case decides nothing"
    _same(late[0], want[0], "merge turned on after a lean process")
    # ... without any fetch in between
    d = torch.from_numpy(x).cuda().contiguous()
    ctx = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=n)
    ctx.set_timing(True)
    ctx.batch_process(d, offs)
    ctx.set_intensity_merge(*MERGE)
    ctx.batch_cluster()
    for s in range(n):
        assert np.array_equal(ctx.batch_fetch_clusters(s, lean[1][s]["n_apri"]), want[0][f"clusters[{s}]"])
    # a calibration turned on after a lean batch: the next batch on the same ctx calibrates, and equals a ctx that always did
    ctx.set_intensity_merge(0, *MERGE[1:])
    ctx.set_intensity_calibration(*CAL)
    ctx.batch_process(d, offs)
    got = [ctx.batch_fetch(s) for s in range(n)]
    names = [name for name, _ in ctx.timings()]
    assert "emit_intensity" not in names, "a calibrating ctx emits eagerly"
    got_cal = [ctx.batch_fetch_intensity_calibration(s, got[s]["n_nonground"]) for s in range(n)]
    got_stats = ctx.batch_intensity_calibration_stats()
    ctx.close()
    ref = scvod.Ctx(P, max_points_total=int(offs[-1]) + 64, max_scans=n)
    ref.set_voxel_descriptors(1)
    ref.set_intensity_calibration(*CAL)
    ref.batch_process(d, offs)
    for s in range(n):
        r = ref.batch_fetch(s)
        for k in FETCHED:
            assert np.array_equal(_bits(got[s][k]), _bits(r[k])), f"calibrated, scan {s}: {k}"
        nc, inten = ref.batch_fetch_intensity_calibration(s, r["n_nonground"])
        assert np.array_equal(_bits(got_cal[s][0]), _bits(nc)) and np.array_equal(_bits(got_cal[s][1]), _bits(inten))
        assert not np.array_equal(_bits(r["apri"]["intensity"]), _bits(lean[1][s]["apri"]["intensity"])), "the calibration changed nothing"
    assert got_stats == ref.batch_intensity_calibration_stats() and got_stats["points"] > 0
    ref.close()
    torch.cuda.synchronize()


# ---- 4. a grid beyond the pack limits -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_grid_beyond_the_pack_limits_keeps_the_gather_form(scvod, oracle):
    P = scvod.make_params("semantickitti", sector_res=0.17)
    R, S, Az, _ = scvod.grid_dims(P)
    assert S > 2044 and R <= 2044 and Az <= 1020
    x = _scan(P, 31, 3000)
    offs = np.asarray([0, len(x)], np.int32)
    out, res, first, second = _run(scvod, P, x, offs, cluster=False)
    assert first.count("emit") == 1 and "emit_intensity" not in second, "the ctx emitted lean on a grid the packed triple cannot hold"
    assert second.count("vx_descriptors") == 1                  # (the voxel stage itself stays lean)
    assert res[0]["apri"]["sector_idx"].max() > 2045            # ... and the scan has points out there
    _check_oracle(oracle, P, x, offs, res)
    assert np.array_equal(out["apri_key[0]"], res[0]["apri"]["voxel_idx"].astype(np.int64))


# ---- 5. the bound, on the CPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def spec_lean(tmp_path_factory):
    """tests/helpers/lean_emission_spec.cpp: scvod_math.h compiled for the CPU, as the spec fixture does"""
    out = str(tmp_path_factory.mktemp("lean_emission") / "liblean_emission_spec.so")
    src = os.path.join(ROOT, "tests", "helpers", "lean_emission_spec.cpp")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, src])
    lib = C.CDLL(out)
    lib.lean_key_compare.restype = C.c_int
    return lib


def _spec_compare(lib, scvod, P, xyz, dims=None):
    g = np.array([P.min_dis, P.max_dis, P.min_angle, P.max_angle, P.min_azimuth, P.max_azimuth, P.range_res, P.sector_res, P.azimuth_res],
                 np.float32)
    d = np.asarray(dims if dims is not None else scvod.grid_dims(P)[:3], np.int32)
    xyz = np.ascontiguousarray(xyz, np.float32)
    out = np.zeros(12, np.int64)
    ok = lib.lean_key_compare(g.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), xyz.ctypes.data_as(C.c_void_p), C.c_long(len(xyz)),
                              out.ctypes.data_as(C.c_void_p))
    out = out.tolist()
    out.append(ok)
    return out


def _edge_cloud(P, rng, n):
    """n points: a third uniform over (and beyond) the range / FOV box, the others clustered -- down to single ulps -- around the range
    limits, the azimuth limits, the sector edges with the 0 / 360 seam, and the azimuth bin edges"""
    f32 = np.float32
    r = rng.uniform(0.5 * P.min_dis, 1.1 * P.max_dis, n)
    th = rng.uniform(0, 2 * np.pi, n)
    az = np.deg2rad(rng.uniform(P.min_azimuth - 5, P.max_azimuth + 5, n))
    k = n // 6
    lim = rng.choice([P.min_dis, P.max_dis], k)
    r[k:2 * k] = lim * (1 + rng.choice([-1, 0, 1], k) * 10.0 ** rng.uniform(-8, -3, k))
    lim = np.deg2rad(rng.choice([P.min_azimuth, P.max_azimuth], k))
    az[2 * k:3 * k] = lim + rng.choice([-1, 1], k) * 10.0 ** rng.uniform(-8, -3, k)
    S = int(np.ceil((P.max_angle - P.min_angle) / P.sector_res))
    th[3 * k:4 * k] = np.deg2rad(P.min_angle + rng.integers(0, S + 1, k) * float(P.sector_res) + rng.normal(0, 1, k) * rng.choice([1e-6, 1e-4, 2e-3], k))
    A = int(np.ceil((P.max_azimuth - P.min_azimuth) / P.azimuth_res))
    az[4 * k:5 * k] = np.deg2rad(P.min_azimuth + rng.integers(0, A + 1, k) * float(P.azimuth_res) + rng.normal(0, 1, k) * rng.choice([1e-6, 1e-4, 2e-3], k))
    xyz = np.stack([r * np.cos(th), r * np.sin(th), r * np.tan(az)], 1).astype(f32)
    # exact limits: dis == min_dis / max_dis on the axes (sqrt(d * d) == d), the seam from below, signed zeros, z == 0
    m = 2000
    d = rng.choice([f32(P.min_dis), f32(P.max_dis), np.nextafter(f32(P.max_dis), f32(0)), np.nextafter(f32(P.min_dis), f32(1e9))], m).astype(f32)
    ax = rng.integers(0, 4, m)
    xyz[:m, 0] = np.where(ax == 0, d, np.where(ax == 1, -d, 0.0))
    xyz[:m, 1] = np.where(ax == 2, d, np.where(ax == 3, -d, rng.choice([0.0, -0.0], m)))
    xyz[m:2 * m, 1] = -np.abs(xyz[m:2 * m, 1]) * f32(1e-7)
    xyz[m:2 * m, 0] = np.abs(xyz[m:2 * m, 0])
    xyz[2 * m:3 * m, 2] = 0.0
    return xyz


def test_the_key_recomputed_from_the_packed_triple_is_the_reference_key(spec_lean, scvod):
    """pack_idx3 clamps range / sector to [-2, 2045] and azimuth to [-2, 1021].  A point that passed the range / FOV test has
    0 <= (v - min) / res <= (max - min) / res in fp32 (subtraction and division by a positive number are monotone), and the grid's
    dimension is the ceiling of that same fp32 quotient: every index lies in [-1, dim - 1], so the clamp never bites while
    dim <= 2044 (1020) -- the limit the ctx tests (idx3_roundtrip_ok).  Counted here, not assumed: the shipped presets and parameter
    sets that put one dimension AT its limit, their upper limits an exact multiple of the resolution or an ulp off it."""
    rng = np.random.default_rng(91)
    f32 = np.float32
    sets = [scvod.make_params(p) for p in ("semantickitti", "parkinglot", "os128_fine", "semantickitti_seq05")]
    for dim, num in (("range", 2044), ("sector", 2044), ("azimuth", 1020), ("range", 700), ("sector", 1333), ("azimuth", 333)):
        for nudge in (0, 1, -1):
            if dim == "range":
                res = f32(rng.uniform(0.01, 0.02))
                mn = f32(rng.uniform(0.5, 3.0))
                mx = f32(mn + f32(num) * res)
                for _ in range(abs(nudge)):
                    mx = np.nextafter(mx, f32(1e9) if nudge > 0 else f32(0))
                kw = dict(min_dis=float(mn), max_dis=float(mx), range_res=float(res))
            elif dim == "sector":
                res = f32(360.0) / f32(num)
                for _ in range(abs(nudge)):
                    res = np.nextafter(res, f32(1e9) if nudge < 0 else f32(0))
                kw = dict(sector_res=float(res))
            else:
                res = f32(rng.uniform(0.05, 0.11))
                mn = f32(rng.uniform(-45.0, -20.0))
                mx = f32(mn + f32(num) * res)
                for _ in range(abs(nudge)):
                    mx = np.nextafter(mx, f32(1e9) if nudge > 0 else f32(-1e9))
                kw = dict(min_azimuth=float(mn), max_azimuth=float(mx), azimuth_res=float(res))
            P = scvod.make_params("semantickitti", **kw)
            R, S, Az, _ = scvod.grid_dims(P)
            if R <= 2044 and S <= 2044 and Az <= 1020:          # (a nudge may push the ceiling one over: not a lean grid then)
                sets.append(P)
    assert len(sets) >= 16
    at_limit = set()
    total = 0
    for P in sets:
        R, S, Az, _ = scvod.grid_dims(P)
        assert R * S * Az < 2 ** 31
        st = _spec_compare(spec_lean, scvod, P, _edge_cloud(P, rng, 300_000))
        kept, bad_key, bad_triple = st[0], st[1], st[2]
        assert st[12] == 1, "idx3_roundtrip_ok refuses a grid within the limits"
        assert st[11] == 0, "keep_of_point (the arrange pass's verdict) disagrees with apri_of_point's range / FOV test"
        assert kept > 100_000 and bad_key == 0 and bad_triple == 0, (R, S, Az, st)
        assert st[3] == -1 and st[5] >= -1 and st[7] >= -1 and st[4] <= R and st[6] <= S and st[8] <= Az, (R, S, Az, st)
        assert st[4] >= R - 1 and st[6] >= S - 1 and st[8] >= Az - 1, "the cloud does not reach the grid's last bins"
        assert st[9] > 0 and st[10] > 1000                      # out-of-grid triples and undecided estimates are among the kept points
        at_limit |= {k for k, v, lim in (("R", R, 2044), ("S", S, 2044), ("A", Az, 1020)) if v == lim}
        total += kept
    assert at_limit == {"R", "S", "A"} and total > 3_000_000
    # beyond the limits the clamp does bite, and the ctx's test says so
    P = scvod.make_params("semantickitti", sector_res=0.17)
    st = _spec_compare(spec_lean, scvod, P, _edge_cloud(P, rng, 200_000))
    assert st[12] == 0 and st[1] > 0
