"""The N > 1 job of bench.py on ONE device.
(1) two ranks (gloo, device buffers staged through the host) share a job of two sequences -- whole sequences per rank, the
    sequential tracking chain inside each, the static maps reduce-scattered as padded slots: per-scan dynamic counts and
    the merged map must equal the single-rank run of the same job bit for bit;
(2) the RCCL leg the driver will run at 8 ranks, executed at ONE rank: torch.distributed initialised with backend nccl,
    the step's device collectives (all_to_all_single of the padded map slots, all_reduce of the summary) really run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp, name, extra, backend="gloo"):
    out = os.path.join(tmp, name + ".npz")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--no-cpu", "--no-extras", "--backend", backend,
           "--kind", "PARK", "--preset", "parkinglot", "--dump-map", out] + extra
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line), np.load(out)


def test_two_ranks_reproduce_the_single_rank_job(tmp_path):
    one, m1 = _run(str(tmp_path), "one", ["--gpus", "1", "--scans", "24", "--sequences", "2"])
    two, m2 = _run(str(tmp_path), "two", ["--gpus", "2", "--scans", "24", "--same-device", "--replicate"])
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2 and two["config"]["rccl_ranks"] == 2
    assert one["config"]["tracking_chain"]["chain"] and two["config"]["tracking_chain"]["chain"]
    assert np.array_equal(m1["scans"], m2["scans"]) and len(m1["scans"]) == 48
    assert np.array_equal(m1["dynamic_points"], m2["dynamic_points"])
    assert m1["dynamic_points"].sum() > 0
    assert np.array_equal(m1["keys"], m2["keys"]) and np.array_equal(m1["vals"], m2["vals"])
    assert len(m1["keys"]) == one["config"]["static_map_cells"] == two["config"]["static_map_cells"]
    assert two["config"]["map_records_sent_per_rank"] > 0


def test_rccl_leg_at_one_rank(tmp_path):
    plain, m0 = _run(str(tmp_path), "plain", ["--gpus", "1", "--scans", "20"])
    rccl, m1 = _run(str(tmp_path), "rccl", ["--gpus", "1", "--scans", "20", "--force-dist", "--split-sequence", "--full"], backend="nccl")
    assert rccl["config"]["backend"] == "nccl" and rccl["config"]["rccl_ranks"] == 1
    assert rccl["config"]["map_slot_records"] > 0                       # the padded all_to_all_single ran
    # the boundary exchange of a cut sequence on the device: export kernels into padded records, one RCCL point-to-point exchange
    # (rank 0 -> rank 0 here), the compare kernel, the all_reduce of the verdict -- and nothing for the slow path to do
    b = rccl["config"]["split"]
    assert b["boundary"]["path"].startswith("device") and b["boundary"]["record_bytes"] >= 65536 and b["boundary_slow_path_steps_rank0"] == 0
    assert "tk_boundary_exchange" in rccl["kernels"]
    assert np.array_equal(m0["dynamic_points"], m1["dynamic_points"])
    assert np.array_equal(m0["keys"], m1["keys"]) and np.array_equal(m0["vals"], m1["vals"])
    assert plain["config"]["static_map_cells"] == rccl["config"]["static_map_cells"]


@pytest.mark.parametrize("halo", [2, 12])
def test_one_sequence_split_over_two_ranks(tmp_path, halo):
    """bench.py at N = 2 (one sequence is cut over the ranks by default): one PARK sequence (one chain, stride 1) in two blocks
    on two gloo ranks of one device.  A halo of two steps cannot rebuild the carried clouds, so the second rank has to walk its
    chain again from the state the first one sends (the one-after-the-other phase of resolve_chain_boundaries); with twelve the
    warm-up reproduces it and the comparison round is all there is.  Either way the per-scan results and the merged map are
    those of the single-rank run, bit for bit."""
    one, m1 = _run(str(tmp_path), "one", ["--gpus", "1", "--scans", "60"])
    two, m2 = _run(str(tmp_path), "two", ["--gpus", "2", "--scans", "60", "--same-device", "--split-halo", str(halo)])
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["config"]["split"]["own"] == 30
    assert np.array_equal(m1["scans"], m2["scans"]) and len(m2["scans"]) == 60
    assert m1["dynamic_points"].sum() > 0
    assert np.array_equal(m1["dynamic_points"], m2["dynamic_points"])
    assert np.array_equal(m1["keys"], m2["keys"]) and np.array_equal(m1["vals"], m2["vals"])


def test_two_sequences_cut_over_three_ranks(tmp_path):
    """plan_job_split through the device path: two sequences of 40 scans dealt as three runs of 26 / 27 / 27 scans -- the first is
    cut once, the second once; rank 1 receives the end of sequence A from rank 0, holds the start of sequence B and sends ITS end to
    rank 2.  Per-scan results and the merged map equal the run with whole sequences on one rank."""
    one, m1 = _run(str(tmp_path), "one", ["--gpus", "1", "--scans", "40", "--sequences", "2"])
    cut, m2 = _run(str(tmp_path), "cut", ["--gpus", "3", "--scans", "40", "--sequences", "2", "--same-device", "--split-sequence", "--split-halo", "3"])
    assert cut["n_gpus"] == 3 and cut["scaling"] == "strong" and len(cut["config"]["split"]["pieces_rank0"]) == 1
    assert np.array_equal(m1["scans"], m2["scans"]) and len(m2["scans"]) == 80
    assert m1["dynamic_points"].sum() > 0
    assert np.array_equal(m1["dynamic_points"], m2["dynamic_points"])
    assert np.array_equal(m1["keys"], m2["keys"]) and np.array_equal(m1["vals"], m2["vals"])


def test_k64_sequence_over_two_ranks_with_the_default_halo(tmp_path):
    """the KITTI stride (five interleaved chains) cut in two with the default halo of 10 steps: the warm-up reproduces every
    chain's boundary state (nothing is walked again: the ranks' comparison round is the whole exchange) and the job equals
    the one-rank run"""
    one, m1 = _run(str(tmp_path), "one", ["--gpus", "1", "--scans", "170", "--kind", "K64", "--preset", "semantickitti"])
    two, m2 = _run(str(tmp_path), "two", ["--gpus", "2", "--scans", "170", "--kind", "K64", "--preset", "semantickitti", "--same-device"])
    assert two["scaling"] == "strong" and two["config"]["split"]["chains_rewalked_at_boundary_all_ranks"] == 0
    assert np.array_equal(m1["scans"], m2["scans"]) and len(m2["scans"]) == 170
    assert m1["dynamic_points"].sum() > 0
    assert np.array_equal(m1["dynamic_points"], m2["dynamic_points"])
    assert np.array_equal(m1["keys"], m2["keys"]) and np.array_equal(m1["vals"], m2["vals"])


def _run_k64(tmp, name, extra, timeout=1500):
    out = os.path.join(tmp, name + ".npz")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--no-cpu", "--no-extras", "--backend", "gloo",
           "--kind", "K64", "--preset", "semantickitti", "--dump-map", out] + extra
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line), np.load(out)


def test_one_k64_sequence_over_four_ranks(tmp_path):
    """The driver's `bench.py --gpus N` job (ONE sequence cut over the ranks, default halo of 10 steps, the KITTI stride of five
    interleaved chains) driven through the device path: four gloo ranks on one device (with the launcher and the test's own
    process that is all a shared device may have open at once), 60 own scans each + a halo of 60 + one successor per chain.  The
    cuts at scans 60 / 120 / 180 are three of the seven cuts of the eight-rank job.  Per-scan dynamic points and the merged map
    equal the one-rank run bit for bit; the line reports how many chains were walked again at a cut (none with the full halo)."""
    one, m1 = _run_k64(str(tmp_path), "one", ["--gpus", "1", "--scans", "240"])
    four, m4 = _run_k64(str(tmp_path), "four", ["--gpus", "4", "--scans", "240", "--same-device"])
    sp = four["config"]["split"]
    assert four["n_gpus"] == 4 and four["scaling"] == "strong" and sp["own"] == 60 and four["config"]["rccl_ranks"] == 4
    assert sp["chains_rewalked_at_boundary_all_ranks"] == 0
    assert np.array_equal(m1["scans"], m4["scans"]) and len(m4["scans"]) == 240
    assert m1["dynamic_points"].sum() > 0
    assert np.array_equal(m1["dynamic_points"], m4["dynamic_points"])
    assert np.array_equal(m1["keys"], m4["keys"]) and np.array_equal(m1["vals"], m4["vals"])
    assert len(m1["keys"]) == one["config"]["static_map_cells"] == four["config"]["static_map_cells"]


def test_kitti_job_scaled_down_over_four_ranks(tmp_path):
    """BASELINE configs[3] -- SemanticKITTI seq 00-10, the sequences cut where the load says (shard.plan_job_split) -- with every
    sequence at 1/32 of its real length (86, 142, 146, 127, 50, 38, 34, 34, 34, 25 and 8 scans in job order: 724 in all), four gloo ranks on one
    device: cuts fall inside sequences, ranks hold the end of one sequence and the start of the next, the shortest sequence is
    shorter than the tracking stride's warm-up.  Results equal the run with whole sequences on one rank."""
    one, m1 = _run_k64(str(tmp_path), "one", ["--gpus", "1", "--kitti", "--kitti-scale", "1/32"])
    four, m4 = _run_k64(str(tmp_path), "four", ["--gpus", "4", "--kitti", "--kitti-scale", "1/32", "--split-sequence", "--same-device"])
    assert four["n_gpus"] == 4 and four["scaling"] == "strong"
    n = len(m1["scans"])
    assert n == len(m4["scans"]) and n > 700 and np.array_equal(m1["scans"], m4["scans"])
    assert len(np.unique(m1["scans"][:, 0])) == 11
    assert m1["dynamic_points"].sum() > 0
    assert np.array_equal(m1["dynamic_points"], m4["dynamic_points"])
    assert np.array_equal(m1["keys"], m4["keys"]) and np.array_equal(m1["vals"], m4["vals"])
    assert four["config"]["split"]["chains_rewalked_at_boundary_all_ranks"] is not None


def test_os128_sequence_over_four_ranks(tmp_path):
    """BASELINE configs[4]'s multi-GPU leg as a dry run: a 128-beam sequence (258 k returns per scan, the 2x finer grid: the generic
    clustering variant, the max_name passes beyond the LDS tables) cut over four gloo ranks of one device with a short halo -- a
    rank whose warm-up misses the state at its cut walks its chains again from the state it receives.  Per-scan dynamic points
    and the merged map equal the one-rank run."""
    common = ["--kind", "OS128", "--preset", "os128_fine", "--scans", "64"]
    one, m1 = _run_k64(str(tmp_path), "one", ["--gpus", "1"] + common)
    four, m4 = _run_k64(str(tmp_path), "four", ["--gpus", "4", "--same-device", "--split-halo", "3"] + common)
    assert four["n_gpus"] == 4 and four["scaling"] == "strong" and four["config"]["split"]["own"] == 16
    assert np.array_equal(m1["scans"], m4["scans"]) and len(m4["scans"]) == 64
    assert m1["dynamic_points"].sum() > 0
    assert np.array_equal(m1["dynamic_points"], m4["dynamic_points"])
    assert np.array_equal(m1["keys"], m4["keys"]) and np.array_equal(m1["vals"], m4["vals"])


@pytest.mark.parametrize("halo", [2, 12])
def test_device_boundary_step_logic_with_a_real_neighbour(tmp_path, halo):
    """bench.py's nccl-path step on two ranks of ONE device (round-5 verdict, missing #1): `--boundary device` on gloo runs
    shard.DeviceBoundary -- padded rows exported without a host read, the pinned pointer table, the compare kernel, the verdict word
    copied behind an event and read when the NEXT step starts (or at the final barrier) -- with the rows and the verdict staged
    through the host where RCCL would move them.  Halo 12: the verdict is 0, no slow path.  Halo 2: the warm-up cannot rebuild the
    carried clouds, the verdict sends every step through resolve_chain_boundaries and the step's map is accumulated again from the
    corrected labels.  Either way the job equals the one-rank run bit for bit."""
    one, m1 = _run_k64(str(tmp_path), "one", ["--gpus", "1", "--scans", "170"])
    two, m2 = _run_k64(str(tmp_path), "two", ["--gpus", "2", "--scans", "170", "--same-device", "--boundary", "device", "--split-halo", str(halo), "--steps", "2", "--full"])
    sp = two["config"]["split"]
    assert two["n_gpus"] == 2 and sp["boundary"]["path"].startswith("device rows") and sp["boundary"]["record_bytes"] >= 65536
    assert "tk_boundary_exchange" in two["kernels"]
    if halo == 12:
        assert sp["boundary_slow_path_steps_rank0"] == 0 and sp["chains_rewalked_at_boundary_all_ranks"] == 0
    else:  # warm-up + 2 timed + 2 attributed steps: each one's verdict sent the job down the host-driven protocol
        assert sp["boundary_slow_path_steps_rank0"] >= 4 and sp["chains_rewalked_at_boundary_all_ranks"] > 0
    assert np.array_equal(m1["scans"], m2["scans"]) and len(m2["scans"]) == 170
    assert m1["dynamic_points"].sum() > 0
    assert np.array_equal(m1["dynamic_points"], m2["dynamic_points"])
    assert np.array_equal(m1["keys"], m2["keys"]) and np.array_equal(m1["vals"], m2["vals"])
