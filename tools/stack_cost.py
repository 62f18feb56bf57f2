#!/usr/bin/env python3
"""Development tool: what scvod_batch_stack_scans (csrc/scvod_stack.hip) costs on the K64 bench-shaped job, or on as many of its scans
as fit next to their output -- window 3 / interval 3 (the reference's stacker) and window 3 / interval 1 (overlapping windows: three
times the output), xyzi alone and with payload and source index carried.  Per case: ms per call (stream events around the call after
a warm-up call, median of the repetitions) and GB/s over the bytes the pass has to move: 32 B per output point (16 read, 16 written),
+ 8 B with the payload (4 read, 4 written), + 4 B with the source index (written).  Next to each case a device-to-device copy that
moves the same number of bytes (half of them read, half written), timed the same way in the same run, and the ratio of the two rates.
Writes profiles/stack_cost.txt (--out).
usage: python tools/stack_cost.py [--scale 1.0] [--reps 7] [--out profiles/stack_cost.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dr-using-scv-od_amd", "pyshim"))
import scvod_py
import synth

PRESET, SEQ, COUNT = "semantickitti", 5, 2761   # the K64 bench job (bench.py)
AIM = 0.8


def timed(fn, reps, front=None):
    """median / min / max ms of fn between two stream events.  front: work enqueued in front of the first event, so that the device is
    busy while the host prepares fn's launches and the events bracket fn's device time alone"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if front is not None:
            front()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the bench job's scans")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stack_cost.txt"))
    a = ap.parse_args()
    scvod_py.load_lib()
    count = max(9, int(COUNT * a.scale))
    free, _ = torch.cuda.mem_get_info()
    scans, n = [], 0
    for i in range(count):
        pts, lab, pose = synth.make_scan(SEQ, i, "K64", device="cuda")
        # per input point: 20 B of input, 3 x 24 B of interval-1 output, and the two buffers of the largest copy (3 x 44 B together)
        if (n + len(pts)) * (20 + 72 + 132) > 0.8 * free:
            break
        scans.append((pts, lab.to(torch.int32), pose))
        n += len(pts)
    count = len(scans)
    d = torch.cat([s[0] for s in scans]).contiguous()
    pay = torch.cat([s[1] for s in scans]).contiguous()
    off = np.concatenate([[0], np.cumsum([len(s[0]) for s in scans])]).astype(np.int32)
    poses = np.asarray([s[2] for s in scans], np.float32)
    del scans
    ctx = scvod_py.Ctx(scvod_py.make_params(PRESET), max_points_total=1024, max_scans=1)   # the stage needs no arena
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"job: K64 bench-shaped, {count} of {COUNT} scans, {n} input points ({16 * n / 1e9:.2f} GB of xyzi); {a.reps} repetitions, median (min .. max)",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    worst = None
    for window, interval in ((3, 3), (3, 1)):
        out_off, mid = scvod_py.stack_offsets(off, window, interval)
        m = int(out_off[-1])
        xyzi = torch.empty((m, 4), dtype=torch.float32, device="cuda")
        pay_out = torch.empty(m, dtype=torch.int32, device="cuda")
        src = torch.empty(m, dtype=torch.int32, device="cuda")
        for name, kw, per_point in (("xyzi", {}, 32), ("xyzi + payload + src", dict(d_payload_in=pay, d_payload_out=pay_out, d_src_out=src), 44)):
            nbytes = per_point * m
            a_buf = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            b_buf = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")

            def call():
                ctx.batch_stack_scans(d, off, poses, xyzi, window=window, interval=interval, stream=st, **kw)

            def copy():
                b_buf.copy_(a_buf)
            imed, ilo, ihi = timed(call, a.reps)                 # an idle stream: the device waits while the host builds the tables
            med, lo, hi = timed(call, a.reps, front=copy)        # behind queued work: the table upload and the kernel alone
            cmed, clo, chi = timed(copy, a.reps, front=copy)
            del a_buf, b_buf
            rate, crate = nbytes / med / 1e6, nbytes / cmed / 1e6
            ratio = rate / crate
            worst = ratio if worst is None else min(worst, ratio)
            lines.append(f"window {window} / interval {interval}, {name}: {len(mid)} stacked scans, {m} output points, {nbytes / 1e9:.2f} GB moved")
            lines.append(f"    stack  {med:8.3f} ms ({lo:.3f} .. {hi:.3f})   {rate:7.0f} GB/s   (behind queued work: table upload + kernel)")
            lines.append(f"    stack  {imed:8.3f} ms ({ilo:.3f} .. {ihi:.3f})   {nbytes / imed / 1e6:7.0f} GB/s   (the call on an idle stream, the host's table building included)")
            lines.append(f"    copy   {cmed:8.3f} ms ({clo:.3f} .. {chi:.3f})   {crate:7.0f} GB/s   (device-to-device, {nbytes // 2} bytes)")
            lines.append(f"    ratio  {ratio:.3f}   (aim: at least {AIM})")
        del xyzi, pay_out, src
        torch.cuda.empty_cache()
    lines += ["", f"lowest ratio {worst:.3f}: " + ("the aim is met" if worst >= AIM else "BELOW the aim -- see the counters (a run of their own)")]
    lines.append(f"scratch of the stage after these calls: {ctx.stack_scratch_bytes()} bytes")
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(HEADER + text)


HEADER = """Cost of scvod_batch_stack_scans (csrc/scvod_stack.hip) on the K64 bench-shaped job
====================================================================================

How to measure: `python tools/stack_cost.py --reps 7` on the MI355X (stream events around each call after a warm-up call, median of the
repetitions).  Bytes moved: 32 B per output point (16 read, 16 written), + 8 B with the payload, + 4 B with the source index.  The copy
next to each case is a device-to-device copy of half those bytes (it reads and writes them once each), timed the same way in the same
run.  The stacking call is timed twice: behind a queued copy (the device is busy while the host builds the segment / tile table, so the
events bracket the table upload and the kernel alone; the ratio is taken from this figure) and on an idle stream (the device waits for
the host's table building: what a caller with nothing else in flight sees).  The aim is at least 0.8 x the copy's GB/s.

"""


if __name__ == "__main__":
    main()
