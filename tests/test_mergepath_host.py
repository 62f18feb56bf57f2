"""The merge-path schedule of the large Patchwork sort tiers (csrc/scvod_mergepath.h), replayed on the CPU:
tests/helpers/mergepath_replay.cpp runs the register runs, the network's stages up to the hand-over run length R and every merge
level thread by thread and barrier by barrier through the templates the kernel calls, on an array that records every access.
Covered: n = 1, 15, 16, 17, 31, 33, 255, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192; R = 16, 64, 256; keys ascending,
descending, all z equal (the index decides), two z values interleaved, runs already merged, random with many z ties.
Checked per sort: the result is std::sort of the keys; no slot at or beyond n' (n rounded up to whole runs of 16) is read or
written (guard words, poisoned and compared afterwards); between the barriers of a merge level nothing is written while threads
read and no slot is stored twice; every thread's split agrees with its neighbours', so the 16-output windows tile [0, n') exactly:
a window's outputs are the merge of the input ranges between its own split and the next thread's, a last run without a partner
is left alone, threads at or beyond n' touch nothing."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "mergepath_replay.cpp")
SIZES = (1, 15, 16, 17, 31, 33, 255, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192)
RUNS = (16, 64, 256)
PATTERNS = 6


def _build(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, "-o", exe, SRC])
    return exe


def _levels(n, run):
    """merge levels from runs of `run` keys over the live prefix: the run length doubles while it is below n'"""
    nlive = (n + 15) // 16 * 16
    c = 0
    while run < nlive:
        run *= 2
        c += 1
    return c


def _check(p):
    assert p.returncode == 0 and "FAIL" not in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    lines = p.stdout.split("\n")
    assert f"ok {len(SIZES) * len(RUNS) * PATTERNS}" in lines
    levels = {}
    for l in lines:
        if l.startswith("levels "):
            _, run, n, cnt = l.split()
            levels[(int(run), int(n))] = int(cnt)
    for n in SIZES:
        for run in RUNS:
            assert levels[(run, n)] == _levels(n, run), (n, run)
    assert levels[(16, 4096)] == 8 and levels[(16, 8192)] == 9 and levels[(256, 4097)] == 5 and levels[(16, 16)] == 0


def test_merge_levels_sort_tile_the_live_prefix_and_stay_below_it(tmp_path):
    exe = _build(tmp_path, "mergepath_replay", ["-O2"])
    _check(subprocess.run([exe, "test", "20262"], capture_output=True, text=True))


def test_replay_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same stand-alone program with the same cases, built with -fsanitize=address,undefined and run once"""
    exe = _build(tmp_path, "mergepath_replay_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    _check(subprocess.run([exe, "test", "3"], capture_output=True, text=True))
