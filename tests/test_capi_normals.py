"""The surface normals' definition on the CPU (include/scvod.h: scvod_normals_device).  Not gpu.

The C++ helper (tests/helpers/normals_ref.cpp: the library's nrm_* / normal_* functions of scvod_math.h over an exhaustive neighbour
loop) against the independent numpy statement of tests/helpers/normals_ref.py, which does not read that header: the count and the ten
int64 sums of every query are equal, not close.  Then the reused fp32 eigen solver against numpy.linalg.eigh, and the refusals that need
no device (scvod_normals_check)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dr-using-scv-od_amd", "pyshim"))
import normals_ref as nr  # noqa: E402
import scvod_py  # noqa: E402

F = np.float32
CRAFTED = nr.crafted()
MEASURED_ANGLE = 1.279e-7  # rad: the largest angle of test_normal_against_eigh as measured (tilt 2; 1.026e-8 and 7.502e-8 at tilts 0, 1)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return nr.build(tmp_path_factory.mktemp("normalsref"))


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_helper_sums_equal_numpy(ref, name):
    c = CRAFTED[name]
    h = nr.run(ref, c["cloud"], c["query"], c["radius"], c["min_neighbours"])
    pick = list(range(len(h["count"]))) if c["numpy_pick"] is None else list(c["numpy_pick"])
    want = nr.sums_numpy(c["cloud"], c["query"], c["radius"], pick)
    got = [[int(v) for v in h["sums"][i]] for i in pick]
    assert got == want
    assert [int(h["count"][i]) for i in pick] == [w[0] for w in want]


def test_the_crafted_clouds_are_what_their_names_say(ref):
    """the conditions the device tests rest on, from the exhaustive loop"""
    run = {k: nr.run(ref, c["cloud"], c["query"], c["radius"], c["min_neighbours"]) for k, c in CRAFTED.items()}
    assert run["k4_k5"]["count"].tolist() == [4] * 4 + [5] * 5
    assert np.isnan(run["k4_k5"]["normals"][:4]).all() and np.isfinite(run["k4_k5"]["normals"][4:]).all()
    assert np.isnan(run["k4_k5"]["curvature"][:4]).all() and np.isfinite(run["k4_k5"]["curvature"][4:]).all()
    assert run["k4_k5"]["stats"]["below_min"] == 4 and run["k4_k5"]["stats"]["finite"] == 5
    # (0.5, 0, 0) and (-0.5, 0, 0) are out, the float below 0.5 is in
    assert run["radius_edge"]["count"].tolist() == [4]
    assert run["radius_edge"]["sums"][0, 1] == int(np.rint(float(np.nextafter(F(0.5), F(0))) * 2 ** 30)) + int(np.rint(float(F(0.1)) * 2 ** 30))
    assert run["alias"]["count"].tolist() == [5] and run["alias_self"]["count"].tolist() == [2, 2, 2, 2, 5]
    assert [run[f"points{n}"]["count"].tolist() for n in (1, 2, 3)] == [[1], [2, 2], [3, 3, 3]]
    assert np.isfinite(run["points3"]["normals"]).all() and np.isnan(run["points2"]["normals"]).all()
    assert run["faces"]["count"][-2:].tolist() == [1, 1] and run["faces_queries"]["count"][-2:].tolist() == [0, 0]
    assert run["faces"]["count"].max() > 8
    sizes = (63, 64, 65, 129)
    assert run["groups"]["count"].tolist() == [n for n in sizes for _ in range(n)]
    assert (run["blob"]["count"] == 5000).all()
    assert np.abs(run["blob"]["sums"][:, 4:]).max() > 5000 * 2 ** 30 * 3.5  # second-order sums beyond 2^44.1: the fixed-point range
    d = run["dirty"]
    bad = ~nr.usable(CRAFTED["dirty"]["cloud"])
    assert d["stats"]["cloud_left_out"] == d["stats"]["nonfinite_queries"] == int(bad.sum()) > 20
    assert np.isnan(d["normals"][bad]).all() and (d["count"][bad] == 0).all() and (d["count"][~bad] > 0).all()
    clean = nr.run(ref, CRAFTED["dirty"]["cloud"][~bad], None, 0.2, 5)
    assert clean["sums"].tobytes() == d["sums"][~bad].tobytes() and clean["normals"].tobytes() == d["normals"][~bad].tobytes()
    dq = run["dirty_queries"]
    assert dq["stats"]["nonfinite_queries"] == int((~nr.usable(CRAFTED["dirty_queries"]["query"])).sum()) > 10


def test_segments_flip_towards_the_viewpoint(ref):
    cloud, n = nr.plane_cloud(1)
    seg = [0, 200, 200, len(cloud)]
    above, below = 30.0 * n, -30.0 * n
    h0 = nr.run(ref, cloud, None, 0.5, 5)
    h = nr.run(ref, cloud, None, 0.5, 5, seg=seg, view=[above, below, below])
    assert h["sums"].tobytes() == h0["sums"].tobytes() and h["curvature"].tobytes() == h0["curvature"].tobytes()
    dots = h["normals"].astype(np.float64) @ n
    assert (dots[:200] > 0.9).all() and (dots[200:] < -0.9).all()
    assert np.array_equal(np.abs(h["normals"]), np.abs(h0["normals"]))  # only signs move
    signs0 = np.sign(h0["normals"].astype(np.float64) @ n)
    assert np.array_equal(h["normals"][:200], h0["normals"][:200] * signs0[:200, None].astype(F))


def _angles(ref, tilt):
    """per query: the angle (rad) between the helper's normal and eigh's smallest eigenvector of the fp64 covariance of the same
    neighbours, and the gap of the two smallest eigenvalues over the largest"""
    cloud, _ = nr.plane_cloud(tilt)
    h = nr.run(ref, cloud, None, 0.5, 5)
    P = cloud.astype(np.float64)
    r2 = F(0.5) * F(0.5)
    ang, gap = [], []
    for i in range(len(cloud)):
        E = cloud - cloud[i][None, :]
        d = (E[:, 0] * E[:, 0] + E[:, 1] * E[:, 1]) + E[:, 2] * E[:, 2]
        nb = P[d < r2]
        assert len(nb) == h["count"][i]
        w, v = np.linalg.eigh(np.cov(nb.T, bias=True))
        gap.append((w[1] - w[0]) / w[2])
        n = h["normals"][i].astype(np.float64)
        ang.append(float(np.arctan2(np.linalg.norm(np.cross(v[:, 0], n)), abs(float(v[:, 0] @ n)))))  # (does not see the fp32 length)
    return np.asarray(ang), np.asarray(gap)


@pytest.mark.parametrize("tilt", [0, 1, 2])
def test_normal_against_eigh(ref, tilt):
    """Watches the reused fp32 solver (eigen33_min_f32) only.  Lattice planes at three tilts (0, 14 and 29 degrees) with 1 cm of fp32
    noise, radius 0.5: the largest angle to numpy.linalg.eigh's eigenvector measured here is 1.279e-7 rad (MEASURED_ANGLE; DESIGN.md
    section 2 quotes it), about one fp32 epsilon; the bound is eight times that, a margin for libm and BLAS differences between machines and nothing more.
    Queries whose two smallest eigenvalues differ by less than 5 % of the largest would be left out; the clouds are built so that none
    is."""
    ang, gap = _angles(ref, tilt)
    left_out = int((gap < 0.05).sum())
    print(f"tilt {tilt}: largest angle {ang.max():.3e} rad over {len(ang)} queries, smallest gap {gap.min():.3f}, left out {left_out}")
    assert left_out == 0
    assert ang.max() <= 8 * MEASURED_ANGLE


def test_normals_check_refuses_and_accepts_the_limits():
    d = scvod_py.normal_params_default
    chk = scvod_py.normals_check
    p = d()
    assert (p.radius, p.min_neighbours, p.flags, p.reserved) == (0.5, 5, 0, 0)
    assert chk() == 0 and chk(p, 4, 100, 3, 7) == 0
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float(np.nextafter(F(4), F(5)))), dict(min_neighbours=2),
                dict(flags=1), dict(reserved=1)):
        assert chk(d(**bad), 3, 10) == -1, bad
    assert chk(d(radius=4.0), 3, 10) == 0 and chk(d(min_neighbours=3), 3, 10) == 0  # the limits at equality
    for stride in (0, 1, 2, 5):
        assert chk(p, stride, 10) == -1
    for stride in (1, 2, 5):
        assert chk(p, 3, 10, stride, 10) == -1
    assert chk(p, 3, 1 << 28) == 0 and chk(p, 3, (1 << 28) + 1) == -1 and chk(p, 3, -1) == -1 and chk(p, 3, 1 << 40) == -1
    assert chk(p, 3, 10, 3, -1) == -1
    view = np.zeros((2, 3), F)
    assert chk(p, 3, 10, 0, 10, [0, 4, 10], view) == 0 and chk(p, 3, 10, 0, 10, [0, 10, 10], view) == 0
    assert chk(p, 3, 10, 0, 10, [0, 5, 4], view) == -1       # decrease
    assert chk(p, 3, 10, 0, 10, [0, 4, 9], view) == -1       # do not end at n_query
    assert chk(p, 3, 10, 0, 10, [1, 4, 10], view) == -1      # do not start at 0
    assert chk(p, 3, 10, 0, 10, None, view, n_segments=2) == -1  # viewpoints without offsets
    assert chk(p, 3, 10, 0, 10, [0, 4, 10], None) == -1
    assert chk(p, 3, 10, 0, 10, None, view, n_segments=0) == -1
