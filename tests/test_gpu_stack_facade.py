"""The scan stacking through the C++ facade and its driver (dr-using-scv-od_amd/host: SSC::stackScans inside SSC::segDF, scvod_sequence
--stack-window W --stack-interval I) on the small KITTI-layout sample test_gpu_facade.py writes for its driver test: the stacked run's
frames are the numpy statement's stack (tests/helpers/stack_ref.py) of the plain run's frames under the poses of --poses-only, there are
stack_offsets' n_out of them, and the plain run is what it was: the loader's clouds (the oracle's VoxelGrid of the files), the same
lines, and byte for byte what the keys 1 / 1 give."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import stack_ref  # noqa: E402

COUNT = 6


def _run(exe, *args):
    res = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    return res.stdout


def _clouds(d, n):
    return [np.fromfile(os.path.join(d, f"{k}_cloud.f32"), np.float32).reshape(-1, 4) for k in range(n)]


@pytest.fixture(scope="module")
def sample(scvod, tmp_path_factory):
    spec = importlib.util.spec_from_file_location("sequence_demo", os.path.join(ROOT, "tools", "sequence_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    exe = os.path.join(ROOT, "dr-using-scv-od_amd", "host", "scvod_sequence")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)])
    d = str(tmp_path_factory.mktemp("stack_facade"))
    seq = os.path.join(d, "seq")
    os.makedirs(seq)
    scans, labels = demo.write_kitti_sequence(seq, 3, 0, COUNT, "PARK")
    cfg = os.path.join(d, "cfg.yaml")
    open(cfg, "w").write(demo.YAML.format(skip=1, count=COUNT, data=os.path.join(seq, "velodyne"), labels=os.path.join(seq, "labels"),
                                          poses=os.path.join(seq, "poses.txt"), **scvod.PRESETS["parkinglot"]))
    plain = os.path.join(d, "plain")
    os.makedirs(plain)
    log = _run(exe, cfg, plain)
    poses = np.asarray([[np.float32(v) for v in line.split()] for line in _run(exe, "--poses-only", cfg).strip().splitlines()], np.float32)
    assert poses.shape == (COUNT, 6)
    return dict(exe=exe, d=d, seq=seq, cfg=cfg, plain=plain, log=log, poses=poses, scans=scans, labels=labels)


def test_stacked_run_is_the_stack_of_the_plain_run(scvod, oracle, sample):
    out = os.path.join(sample["d"], "stacked")
    os.makedirs(out)
    log = _run(sample["exe"], sample["cfg"], out, "--stack-window", "3", "--stack-interval", "3")
    plain = _clouds(sample["plain"], COUNT)
    off = np.concatenate([[0], np.cumsum([len(c) for c in plain])]).astype(np.int32)
    want = stack_ref.stack(oracle, np.concatenate(plain), off, sample["poses"], 3, 3)
    out_off, mid = scvod.stack_offsets(off, 3, 3)
    n_out = len(mid)
    assert n_out == 2 and np.array_equal(out_off, want["out_offsets"])
    assert re.search(r"^frames (\d+) ", log, re.M).group(1) == str(n_out)
    assert sorted(f for f in os.listdir(out) if f.endswith("_cloud.f32")) == [f"{g}_cloud.f32" for g in range(n_out)]
    got = _clouds(out, n_out)
    assert not np.isnan(want["xyzi"]).any()
    for g in range(n_out):
        w = want["xyzi"][out_off[g]:out_off[g + 1]]
        assert got[g].shape == w.shape, g
        assert np.array_equal(got[g].view(np.uint32), w.view(np.uint32)), g
        assert np.array_equal(got[g][:len(plain[mid[g]])].view(np.uint32), plain[mid[g]].view(np.uint32))   # the middle scan first, untouched
    # the frames were moved: the sample's poses are a metre apart
    assert np.abs(want["xyzi"][want["moved"]][:, :3] - np.concatenate(plain)[want["src"][want["moved"]]][:, :3]).max() > 0.5


def test_plain_run_is_unchanged(scvod, oracle, sample):
    lines = sample["log"].strip().splitlines()
    assert len(lines) == COUNT + 1
    for k, line in enumerate(lines[:-1]):
        assert re.fullmatch(rf"frame {k} points \d+ clusters \d+ tracked \d+ dynamic \d+", line), line
    assert re.fullmatch(rf"frames {COUNT} dynamic_total \d+", lines[-1])
    # the frames are the loader's: label filter, intensity scaling and VoxelGrid 0.08 m of the files (SSC::getCloud), nothing stacked
    for k, got in enumerate(_clouds(sample["plain"], COUNT)):
        x = np.fromfile(os.path.join(sample["seq"], "velodyne", f"{k:06d}.bin"), np.float32).reshape(-1, 4)
        lab = np.fromfile(os.path.join(sample["seq"], "labels", f"{k:06d}.label"), np.uint32)
        ref, _ = oracle.voxelgrid(x, (0.08, 0.08, 0.08), labels=lab, max_intensity=255.0)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), k
    # the keys 1 / 1 are off: byte for byte the run without them
    out = os.path.join(sample["d"], "one_one")
    os.makedirs(out)
    log = _run(sample["exe"], sample["cfg"], out, "--stack-window", "1", "--stack-interval", "1")
    assert log == sample["log"]
    assert sorted(os.listdir(out)) == sorted(os.listdir(sample["plain"]))
    for f in os.listdir(out):
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(sample["plain"], f), "rb").read(), f
