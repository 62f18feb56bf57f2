"""The box-grid kNN search that the region growing and the intensity calibration share (csrc/scvod_boxgrid.h), replayed on the
CPU: tests/helpers/boxgrid_replay.cpp calls the header's own shape rule, cell rule, ring walk, top-k insertion and stop rule
(the CSR table is filled serially there, in the header's convention: the header's build needs a workgroup).
Checked: for grids with an axis of one cell, 1 x 1 x 1 and three dozen seeded grids of up to 12 cells per axis, and every query
cell, the runs of rings 0 .. R visit every cell exactly once, each at its ring's Chebyshev distance and in the row the walk names,
and the bound reports "the whole grid is probed" at exactly ring R; the search returns the brute-force (d^2, index)-sorted k nearest,
bit for bit, for k 3, 10 and 16 with both stages' shape constants on clouds of 1, 2 and 7 points, 500 copies of one point, a lattice
of exact ties, a plane, a line, and clouds around +-80 m; the shape rule equals a transcription of the two code blocks it replaced
(h as a bit pattern, the three cell counts) on those clouds and on zero, tiny and huge boxes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "boxgrid_replay.cpp")


def _build(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", *flags, "-o", exe, SRC])
    return exe


def test_rings_partition_the_grid_and_the_search_equals_brute_force(tmp_path):
    exe = _build(tmp_path, "boxgrid_replay", ["-O2"])
    p = subprocess.run([exe, "full", "20262"], capture_output=True, text=True)
    assert p.returncode == 0 and "FAIL" not in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
    assert any(l.startswith("ok ") for l in p.stdout.split("\n"))


def test_replay_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program, a reduced set of cases, built with -fsanitize=address,undefined and run once, stand-alone"""
    exe = _build(tmp_path, "boxgrid_replay_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    p = subprocess.run([exe, "quick", "3"], capture_output=True, text=True)
    assert p.returncode == 0 and "FAIL" not in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "ok " in p.stdout
