"""The schedule of the pad-free LDS sorts (csrc/scvod_sortnet.h), replayed on the CPU: tests/helpers/sortnet_replay.cpp
runs every pass thread by thread through the templates the kernels call, on an array that records every access.
Covered: every n from 1 to 1100 with 8 and 16 keys per thread; for the 2048, 4096, 8192 and 16 384 networks every n within
17 of 1/2, 3/4 and 1 of np2, n within 1 of a seeded sample of multiples of the thread count, and 200 seeded random n.
Checked per sort: the output is std::sort of the input (unique 64-bit keys; 32-bit keys with repeats), no slot at or above
n' (n rounded up to whole runs) is read or written (they are poisoned and compared afterwards), no slot is touched by two
threads between two barriers, and the number of passes is that of the padded network."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "sortnet_replay.cpp")


def _padded_passes(lg_np2, lge):
    """passes of block_bitonic_merge_stages (scvod_kernels.hip) for np2 = 2^lg_np2: stage k = 2^r, r = lge + 1 .. lg_np2,
    takes a leading pass of r mod lge levels (lge when that is 0) and then full passes of lge levels"""
    total = 0
    for r in range(lge + 1, lg_np2 + 1):
        first = r % lge or lge
        total += 1 + (r - first) // lge
    return total


def _build(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, "-o", exe, SRC])
    return exe


def test_schedule_sorts_and_stays_below_the_live_prefix(tmp_path):
    exe = _build(tmp_path, "sortnet_replay", ["-O2"])
    p = subprocess.run([exe, "full", "20261"], capture_output=True, text=True)
    assert p.returncode == 0 and "FAIL" not in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
    lines = p.stdout.split("\n")
    assert any(l.startswith("ok ") for l in lines)
    passes = {}
    for l in lines:
        if l.startswith("passes "):
            _, lge, np2, cnt = l.split()
            passes[(int(lge), int(np2))] = int(cnt)
    assert _padded_passes(12, 4) == 20 and _padded_passes(13, 4) == 24
    for lge in (3, 4):
        for lg in range(lge, 15):
            assert passes[(lge, 1 << lg)] == _padded_passes(lg, lge), (lge, lg)


def test_replay_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program, a reduced set of sizes, built with -fsanitize=address,undefined and run once, stand-alone"""
    exe = _build(tmp_path, "sortnet_replay_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    p = subprocess.run([exe, "quick", "3"], capture_output=True, text=True)
    assert p.returncode == 0 and "FAIL" not in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "ok " in p.stdout
