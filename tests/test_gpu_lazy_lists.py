"""The three index lists of a batch -- ground_idx, nonground_idx, rejected_src -- on demand.

A lean emission (k_emit<true>, the default of scvod_batch_process) writes none of them: no kernel of process -> cluster -> types -> track
-> map accumulate reads them.  Their first reader runs k_emit_lists ("emit_lists") once for the whole batch (ensure_lists); a ctx with
scvod_set_voxel_descriptors(1) keeps the eager emission, which writes them as it always did.  Both must hand every reader the same bits:

  1. default ctx == mode-1 ctx for every reader (batch_fetch: the lists and cls; point labels, point classes, exported scans; a map
     without the ground, without the rejects, without both), in three call orders, with the timing labels each order must show;
  2. the shapes where the walk can go wrong, against the oracle's two lists and mode 1;
  3. the max_name pass with its tables in arena scratch: it takes seg when the lists are written and the scan's slice of ground_idx while
     they are pending -- lists, clusters and last_name equal mode 1 in both orders;
  4. a second batch on the same ctx decides the flag again."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_async_chain import MAP_CELLS, Batch, _sorted_records, _track, _transforms  # noqa: E402
from test_gpu_lean_emission import _bits, _crafted_scan, _scan  # noqa: E402

pytestmark = pytest.mark.gpu

NO_GROUND, NO_REJECTED, IGNORE_DYNAMIC = 1, 2, 4
LISTS = ("cls", "ground_idx", "nonground_idx", "rejected_src")
MAP_FLAGS = (NO_GROUND, NO_REJECTED, NO_GROUND | NO_REJECTED)
ORDERS = ("readers_first", "chain_first", "fetch_cluster_fetch")


# ---- input ------------------------------------------------------------------------------------------------------------------------------

def _make_batch(scvod, name, P, scans):
    import torch
    n = len(scans)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    x = np.concatenate(scans).astype(np.float32) if n else np.zeros((0, 4), np.float32)
    poses = np.zeros((n, 6), np.float32)
    poses[:, 0] = 0.4 * np.arange(n)
    poses[:, 5] = 0.01 * np.arange(n)
    nxt = np.asarray([s + 1 if s + 1 < n else -1 for s in range(n)], np.int32)
    d = torch.from_numpy(np.ascontiguousarray(x)).cuda().contiguous()
    return Batch(name=name, P=P, d=d, x=x, offs=offs, poses=poses, nxt=nxt, T=_transforms(scvod, poses, nxt), n=n, ext=None)


def _new(scvod, b, eager, timing=True):
    ctx = scvod.Ctx(b.P, max_points_total=int(b.offs[-1]) + 64, max_scans=max(b.n, 1))
    if eager:
        ctx.set_voxel_descriptors(1)
    ctx.set_timing(timing)
    return ctx


# ---- the readers ------------------------------------------------------------------------------------------------------------------------

def _names(ctx):
    return [name for name, _ in ctx.timings(256)]


def _fetch_lists(ctx, b, out, tag=""):
    for s in range(b.n):
        r = ctx.batch_fetch(s)
        for k in LISTS:
            out[f"{tag}{k}[{s}]"] = np.asarray(r[k]).copy()
        assert len(r["ground_idx"]) == r["n_ground"] and len(r["nonground_idx"]) == r["n_nonground"] and len(r["rejected_src"]) == r["n_rejected"]


def _maps(scvod, ctx, b, out, extra, tag):
    for f in MAP_FLAGS:
        smap = scvod.StaticMap(MAP_CELLS)
        smap.accumulate(ctx, b.poses, flags=f | extra)
        out[f"{tag}map[{f}]"] = _sorted_records(smap, None)
        smap.close()


def _exports(scvod, ctx, b, out):
    """the readers that need the clustering, its types and the tracking result"""
    import torch
    n = int(b.offs[-1])
    for f in (0, IGNORE_DYNAMIC):
        out[f"labels[{f}]"] = ctx.batch_point_labels(flags=f).cpu().numpy()[:n].copy()
        out[f"classes[{f}]"] = ctx.batch_point_classes(flags=f).cpu().numpy()[:n].copy()
    for f in (0,) + MAP_FLAGS:
        offs = torch.zeros(b.n + 1, dtype=torch.int32, device="cuda")
        xyzi = torch.zeros((max(n, 1), 4), dtype=torch.float32, device="cuda")
        src = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
        ctx.batch_export_points(offs, xyzi, flags=f, d_src_out=src)
        kept = ctx.batch_export_stats()["kept"]
        out[f"export[{f}].offs"] = offs.cpu().numpy()
        out[f"export[{f}].xyzi"] = xyzi.cpu().numpy()[:kept].copy()
        out[f"export[{f}].src"] = src.cpu().numpy()[:kept].copy()
    _maps(scvod, ctx, b, out, 0, "tracked.")


def _chain(ctx, b, seen):
    """cluster -> types -> track -> a plain map accumulate: the step; the labels of every stage go to `seen`"""
    ctx.batch_cluster()
    seen += _names(ctx)
    ctx.batch_cluster_types()
    seen += _names(ctx)
    _track(ctx, b, b.T, b.nxt, None, 1)
    seen += _names(ctx)


def _run(scvod, b, order, eager):
    """every reader's output in one call order, and the labels: of the step itself, after the first reader, after all readers of that
    stretch"""
    ctx = _new(scvod, b, eager)
    out, step, first, after = {}, [], [], []
    ctx.batch_process(b.d, b.offs)
    step += _names(ctx)
    if order == "readers_first":
        ctx.batch_fetch(0)
        first = _names(ctx)
        _fetch_lists(ctx, b, out)
        _maps(scvod, ctx, b, out, IGNORE_DYNAMIC, "early.")
        after = _names(ctx)
        _chain(ctx, b, step)
        _exports(scvod, ctx, b, out)
        step += _names(ctx)                                      # (the lists were there: nothing runs again behind the chain)
    elif order == "chain_first":
        _chain(ctx, b, step)
        smap = scvod.StaticMap(MAP_CELLS)
        smap.accumulate(ctx, b.poses)
        out["plain_map"] = _sorted_records(smap, None)
        smap.close()
        step += _names(ctx)
        ctx.batch_point_labels(flags=0)
        first = _names(ctx)
        _exports(scvod, ctx, b, out)
        _fetch_lists(ctx, b, out)
        _maps(scvod, ctx, b, out, IGNORE_DYNAMIC, "early.")
        after = _names(ctx)
    else:
        ctx.batch_fetch(b.n - 1)
        first = _names(ctx)
        _fetch_lists(ctx, b, out, "before.")
        after = _names(ctx)
        ctx.batch_cluster()
        step += _names(ctx)
        _fetch_lists(ctx, b, out)
        step += _names(ctx)
        ctx.batch_cluster_types()
        _track(ctx, b, b.T, b.nxt, None, 1)
        step += _names(ctx)
        _exports(scvod, ctx, b, out)
        _maps(scvod, ctx, b, out, IGNORE_DYNAMIC, "early.")
        step += _names(ctx)
        for s in range(b.n):
            for k in LISTS:
                assert np.array_equal(out[f"before.{k}[{s}]"], out[f"{k}[{s}]"]), f"{k}[{s}] changed across the clustering"
    out["counts"] = ctx.batch_counts()
    ln, _ = ctx.batch_cluster_last_name(b.n)
    out["last_name"] = ln
    for s in range(b.n):
        out[f"clusters[{s}]"] = ctx.batch_fetch_clusters(s, int(out["counts"][s, 4]))
    ctx.close()
    return out, step, first, after


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), f"{what}: {k} differs from the ctx that emitted the lists eagerly"


def _check_lists_against_oracle(oracle, b, out):
    for s in range(b.n):
        xs = b.x[b.offs[s]:b.offs[s + 1]]
        if len(xs) == 0:
            assert len(out[f"ground_idx[{s}]"]) == 0 and len(out[f"nonground_idx[{s}]"]) == 0 and len(out[f"rejected_src[{s}]"]) == 0
            continue
        o = oracle.patchwork(b.P, xs, 1)
        assert np.array_equal(out[f"ground_idx[{s}]"], o["ground_idx"]), f"scan {s}: ground_idx differs from the oracle"
        assert np.array_equal(out[f"nonground_idx[{s}]"], o["nonground_idx"]), f"scan {s}: nonground_idx differs from the oracle"
        assert np.array_equal(out[f"cls[{s}]"], o["cls"]), f"scan {s}: cls differs from the oracle"
        bn = oracle.bin(b.P, xs[o["nonground_idx"]], True)
        kept = np.zeros(len(o["nonground_idx"]), bool)
        kept[bn["src"]] = True
        assert np.array_equal(out[f"rejected_src[{s}]"], o["nonground_idx"][~kept]), f"scan {s}: rejected_src is not the stream's unkept points in order"


# ---- 1. every reader, three call orders -------------------------------------------------------------------------------------------------

_B9 = {}


def _b9(scvod):
    if "b" not in _B9:
        P = scvod.make_params("semantickitti")
        _B9["b"] = _make_batch(scvod, "B9", P, [_scan(P, 40 + s, 1500 + 250 * (s % 5)) for s in range(9)])   # > 8 scans: k_pw_fit_coop<16>
    return _B9["b"]


@pytest.mark.parametrize("order", ORDERS)
def test_every_reader_equals_the_eager_ctx_in_each_call_order(scvod, oracle, order):
    b = _b9(scvod)
    got, step, first, after = _run(scvod, b, order, eager=False)
    want, estep, efirst, eafter = _run(scvod, b, order, eager=True)
    _same(got, want, order)
    assert got["counts"][:, 1].min() > 500 and got["counts"][:, 2].min() > 500 and got["counts"][:, 5].min() > 0
    if order == ORDERS[0]:
        _check_lists_against_oracle(oracle, b, got)
    # the labels: the step never pays the pass, the first reader runs it once, no later reader runs it again, the eager ctx never
    assert step.count("emit") == 1 and estep.count("emit") == 1
    assert "emit_lists" not in step, "a stage of the step, or a reader behind the first, ran k_emit_lists"
    assert first.count("emit_lists") == 1, "the first reader did not run k_emit_lists"
    assert after.count("emit_lists") == 1, "a second reader ran k_emit_lists again"
    assert "emit_lists" not in estep + efirst + eafter, "the eager ctx ran k_emit_lists"


# ---- 2. the shapes where the walk can go wrong ------------------------------------------------------------------------------------------

def _dropped_scan():
    """six points more than the range Patchwork starts at, each alone in its patch: every patch is skipped, every point dropped"""
    t = np.linspace(0.3, 5.8, 6)
    x = np.zeros((6, 4), np.float32)
    x[:, 0], x[:, 1], x[:, 2], x[:, 3] = 20.0 * np.cos(t), 20.0 * np.sin(t), -1.7, 10.0
    return x


def test_shapes_where_the_walk_can_go_wrong(scvod, oracle):
    P = scvod.make_params("semantickitti", min_dis=3.0)          # (as the crafted scan of test_gpu_lean_emission.py wants it)
    pw = scvod.PwParams()
    scvod.load_lib().scvod_pw_params_default(C.byref(pw))
    empty = np.zeros((0, 4), np.float32)
    scans = [_crafted_scan(P), _scan(P, 61, 1500), empty, _scan(P, 62, 2500), _dropped_scan(), _scan(P, 63, 2000)]
    b = _make_batch(scvod, "shapes", P, scans)
    assert b.n <= 8, "a handful of scans: k_pw_fit_coop<64>"
    got, step, first, after = _run(scvod, b, "readers_first", eager=False)
    want = _run(scvod, b, "readers_first", eager=True)[0]
    # the input holds what it was made for
    ctx = _new(scvod, b, eager=True, timing=False)
    ctx.batch_process(b.d, b.offs)
    planes = [np.asarray(ctx.batch_fetch(s)["planes"]).copy() for s in range(b.n)]
    ctx.close()
    pl = np.concatenate(planes)
    size, n_g, status = pl["n_pts"], pl["n_ground"], pl["status"]
    assert (np.isin(planes[0]["status"], (2, 3))).sum() >= 2, "no rejected patch in the crafted scan"
    assert got["counts"][0, 5] > 0 and got["counts"][0, 2] > got["counts"][0, 4]
    assert ((status == 1) & (n_g == size) & (size > pw.num_min_pts)).sum() >= 1, "no kept patch that is all ground"
    assert ((status >= 2) | ((status == 1) & (n_g == 0))).sum() >= 1, "no patch whose points all join the non-ground stream"
    assert ((size > 0) & (size <= pw.num_min_pts)).sum() >= 1, "no patch of at most num_min_pts points"
    for lo, hi in ((1, 64), (64, 512), (512, 1 << 30)):          # the three arrange variants
        assert ((status >= 1) & (size >= max(lo, pw.num_min_pts + 1)) & (size < hi)).sum() >= 1, (lo, hi)
    assert tuple(got["counts"][2]) == (0, 0, 0, 0, 0, 0, 0, got["counts"][2, 7]), "the empty scan"
    assert got["counts"][4, 0] == 6 and got["counts"][4, 3] == 6 and got["counts"][4, 1] == 0 and got["counts"][4, 2] == 0, "the scan Patchwork drops"
    _same(got, want, "shapes")
    _check_lists_against_oracle(oracle, b, got)
    assert first.count("emit_lists") == 1 and after.count("emit_lists") == 1 and "emit_lists" not in step


# ---- 3. the scratch of the max_name pass ------------------------------------------------------------------------------------------------

def _os128(scvod):
    import synth
    import torch
    P = scvod.make_params("os128_fine")
    sc = synth.make_scan(5, OS128_SCAN, "OS128", device="cuda")
    d = sc[0].contiguous()
    offs = np.asarray([0, len(d)], np.int32)
    x = d.cpu().numpy()
    torch.cuda.synchronize()
    return Batch(name="OS1", P=P, d=d, x=x, offs=offs, n=1)


OS128_SCAN = 734        # of the OS128 window of test_gpu_lastname.py (700 + 17 k): the one whose set outgrows the LDS tables


def test_the_max_name_pass_takes_its_scratch_from_the_side_that_is_not_needed(scvod, capfd):
    b = _os128(scvod)

    def run(eager, fetch_first):
        ctx = _new(scvod, b, eager, timing=False)                # (untimed: the pass runs on its own streams, beside the readers)
        ctx.batch_process(b.d, b.offs)
        out = {}
        if fetch_first:
            _fetch_lists(ctx, b, out, "first.")                  # lists materialised before the pass: its scratch is seg
            ctx.batch_cluster(sync=False)
        else:
            ctx.batch_cluster(sync=False)                        # lists pending during the pass: its scratch is ground_idx
        _fetch_lists(ctx, b, out)                                # ... which this fetch rewrites, behind the pass
        out["clusters"] = ctx.batch_fetch_clusters(0, int(ctx.batch_counts()[0, 4]))
        os.environ["SCVOD_LN_PROF"] = "1"                        # (development print of the pass each scan took: the precondition below)
        try:
            capfd.readouterr()
            ln, st = ctx.batch_cluster_last_name(1)
            err = capfd.readouterr().err
        finally:
            del os.environ["SCVOD_LN_PROF"]
        out["last_name"] = ln
        ctx.close()
        cap = [int(m) for m in re.findall(r"ln_prof scan 0: .* cap (-?\d+)", err)]
        return out, ln, cap

    want, ln, cap = run(True, False)
    # the precondition: the scan's set went through the pass whose tables live in arena scratch (32 767 nodes), and was determined.
    # (The fourth word of scvod_batch_cluster_last_name holds the set's size only for a set beyond that pass; the development print
    # names the pass.)
    assert cap == [32767], f"scan {OS128_SCAN} does not take the pass with its tables in arena scratch (table capacity {cap})"
    assert ln[0, 2] == 0, "the pass left the scan undetermined"
    for fetch_first in (False, True):
        got, _, cap = run(False, fetch_first)
        assert cap == [32767]
        for k in want:
            assert np.array_equal(got[k], want[k]), f"lists {'materialised before' if fetch_first else 'pending during'} the pass: {k} differs"
        if fetch_first:
            for k in LISTS:
                assert np.array_equal(got[f"first.{k}[0]"], got[f"{k}[0]"])


# ---- 4. a second batch on the same ctx --------------------------------------------------------------------------------------------------

def test_a_second_batch_decides_the_flag_again(scvod):
    P = scvod.make_params("semantickitti")
    b1 = _make_batch(scvod, "one", P, [_scan(P, 70 + s, 2000) for s in range(3)])
    b2 = _make_batch(scvod, "two", P, [_scan(P, 80 + s, 1500 + 500 * s) for s in range(3)])
    cap = max(int(b1.offs[-1]), int(b2.offs[-1])) + 64
    want = {}
    ref = _new(scvod, b2, eager=True)
    ref.batch_process(b2.d, b2.offs)
    _fetch_lists(ref, b2, want)
    ref.close()
    ctx = scvod.Ctx(P, max_points_total=cap, max_scans=3)
    ctx.set_timing(True)
    ctx.batch_process(b1.d, b1.offs)
    one = {}
    _fetch_lists(ctx, b1, one)
    assert _names(ctx).count("emit_lists") == 1
    ctx.batch_process(b2.d, b2.offs)
    assert "emit_lists" not in _names(ctx)
    got = {}
    _fetch_lists(ctx, b2, got)
    assert _names(ctx).count("emit_lists") == 1, "the second batch's lists were taken for written"
    _same(got, want, "second batch")
    assert any(not np.array_equal(one[k], got[k]) for k in got), "the two batches hold the same lists: the case decides nothing"
    # ... and a batch whose lists nobody fetched leaves nothing behind for the next one
    ctx.batch_process(b1.d, b1.offs)
    ctx.batch_process(b2.d, b2.offs)
    again = {}
    _fetch_lists(ctx, b2, again)
    _same(again, want, "third batch")
    ctx.close()
