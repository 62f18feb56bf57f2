"""scvod_map_split_device / scvod_map_split_stats / scvod_map_split_scratch_bytes without a GPU: the symbols, the struct and its
defaults, the constants, the argument errors that come before a device is looked for, the numpy statement
(tests/helpers/map_split_ref.py) against the oracle's exhaustive look-up and against answers worked out by hand, and the host tool's
usage line.  Not gpu."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import map_split_ref as msr  # noqa: E402

NEW = ("scvod_split_params_default", "scvod_map_split_device", "scvod_map_split_stats", "scvod_map_split_scratch_bytes", "scvod_map_split")
INVALID = -1
TOOL = os.path.join(ROOT, "dr-using-scv-od_amd", "host", "scvod_map_split")

# the 6-point base of the hand-written case (also used on the device, tests/test_gpu_map_split.py)
HAND_BASE = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0], [5, 0, 0]], np.float32)
HAND_LABEL = np.array([40, 252 | (7 << 16), 252, 70, 40, 10], np.uint32)
HAND_QUERY = np.array([[0.75, 0, 0], [1.25, 0, 0], [3.5, 0, 0]], np.float32)   # two choose point 1; the third is 0.5 from 3 and from 4
HAND_PAYLOAD = np.array([0xFFFFFFFF, 0x80000001, 2, 0x7FC00003, 4, 0xDEADBEEF], np.uint32)
HAND = {
    (): dict(mark=[0, 1, 0, 1, 0, 0], order=[1, 3, 0, 2, 4, 5], seg4=[0, 2, 6, 6], counts=(2, 4, 0)),
    (252,): dict(mark=[0, 2, 0, 1, 0, 0], order=[3, 0, 2, 4, 5, 1], seg4=[0, 1, 5, 6], counts=(1, 4, 1)),
}
HAND_NN = ([1, 1, 3], [0.0625, 0.0625, 0.25])


def test_symbols_declared_and_exported_and_the_struct(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("map_split_device", "map_split_stats", "map_split_scratch_bytes"):
        assert callable(getattr(scvod.Ctx, m))
    for name, value in (("MISS", 0), ("HIT", 1), ("GATED", 2)):
        assert re.search(r"#define\s+SCVOD_SPLIT_%s\s+%d\b" % (name, value), hdr)
        assert getattr(scvod, "SPLIT_" + name) == value == getattr(msr, name)
    P = scvod.SplitParams
    assert C.sizeof(P) == 52
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("cell", 0), ("max_rings", 4), ("base_stride", 8), ("query_stride", 12),
                                                                 ("n_reject_classes", 16), ("reject_classes", 20)]
    body = hdr[hdr.index("typedef struct scvod_split_params {"):hdr.index("} scvod_split_params;")]
    assert re.findall(r"\b(cell|max_rings|base_stride|query_stride|n_reject_classes|reject_classes)\b(?=[\[,;])", body) == \
        ["cell", "max_rings", "base_stride", "query_stride", "n_reject_classes", "reject_classes"]


def test_params_default(scvod):
    p = scvod.split_params_default()
    assert np.float32(p.cell).view(np.uint32) == np.float32(0.2).view(np.uint32)
    assert (p.max_rings, p.base_stride, p.query_stride, p.n_reject_classes) == (3, 3, 3, 0) and not any(p.reject_classes)
    q = scvod.split_params_default(cell=1.0, max_rings=8, base_stride=4, reject_classes=(252, 253))
    assert q.cell == 1.0 and (q.max_rings, q.base_stride, q.query_stride, q.n_reject_classes) == (8, 4, 3, 2)
    assert tuple(q.reject_classes[:3]) == (252, 253, 0)


def test_argument_errors_come_before_the_device(scvod):
    """a NULL ctx is SCVOD_ERR_INVALID whatever else is passed: no device is touched and nothing is written"""
    lib = scvod.load_lib()
    buf = np.zeros(256, np.int64)
    p = C.c_void_p(buf.ctypes.data)
    assert buf.ctypes.data % 16 == 0
    odd = C.c_void_p(buf.ctypes.data + 8)            # not 16-byte aligned
    out = C.c_void_p(buf.ctypes.data + 1024)
    par = scvod.split_params_default()

    def call(base=p, label=None, n_base=4, query=p, n_query=4, params=par, mark=out, order=out, seg4=out, base_out=out, pay_in=None,
             pay_out=None):
        return lib.scvod_map_split_device(None, base, label, n_base, query, n_query, C.byref(params), mark, order, seg4, base_out, pay_in,
                                          pay_out, out, out, None)

    assert call() == INVALID                                             # a NULL ctx
    assert call(n_base=-1) == INVALID and call(n_query=-1) == INVALID    # negative sizes
    assert call(base=None) == INVALID and call(query=None) == INVALID    # a NULL array of a non-empty cloud
    for field in ("base_stride", "query_stride"):
        for v in (0, 2, 5, -3):
            assert call(params=scvod.split_params_default(**{field: v})) == INVALID
    assert call(base=odd, params=scvod.split_params_default(base_stride=4)) == INVALID
    assert call(query=odd, params=scvod.split_params_default(query_stride=4)) == INVALID
    assert call(pay_out=out) == INVALID                                  # d_payload_out without d_payload_in
    assert call(base_out=C.c_void_p(buf.ctypes.data + 16)) == INVALID    # d_base_out overlapping d_base
    many = scvod.split_params_default()
    many.n_reject_classes = 17
    assert call(params=many, label=p) == INVALID
    assert call(params=scvod.split_params_default(reject_classes=(252,))) == INVALID   # a reject list with NULL labels
    for v in (0.0, -0.2, float("inf"), float("nan")):
        assert call(params=scvod.split_params_default(cell=v)) == INVALID
    for v in (0, -1, 9):
        assert call(params=scvod.split_params_default(max_rings=v)) == INVALID
    assert lib.scvod_map_split_stats(None, out) == INVALID
    assert lib.scvod_map_split_scratch_bytes(None) == 0
    assert lib.scvod_map_split(None, p, None, 4, p, 4, C.byref(par), out, out, out, out) == INVALID
    assert not buf.any()


def test_the_helper_lookup_equals_the_oracle(oracle):
    for seed, n, m in ((1, 2500, 1800), (2, 3000, 2200), (3, 1200, 4000)):
        rng = np.random.default_rng(seed)
        base = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
        base[50:60] = base[7]                                            # coincident points: ties at every distance
        k = min(m // 3, n)
        query = np.concatenate([base[:k], base[:k] + rng.normal(0, 0.05, (k, 3)), rng.uniform(-6, 6, (m - 2 * k, 3))]).astype(np.float32)
        idx, sq = msr.nn(base, query)
        o_idx, o_sq, _ = oracle.nn_search(base, query, 1.0)
        assert np.array_equal(idx, o_idx) and np.array_equal(sq.view(np.uint32), o_sq.view(np.uint32)), seed
        assert idx[7] == 7 and (idx[50:60] == 7).all()
    idx, sq = msr.nn(np.zeros((0, 3), np.float32), np.zeros((5, 3), np.float32))
    assert (idx == -1).all() and np.isposinf(sq).all()


def test_the_helper_against_answers_by_hand():
    for reject, want in HAND.items():
        r = msr.split(HAND_BASE, HAND_QUERY, HAND_LABEL, reject, HAND_PAYLOAD)
        assert r["nn_idx"].tolist() == HAND_NN[0] and r["nn_sqdist"].tolist() == HAND_NN[1]
        assert r["mark"].tolist() == want["mark"] and r["order"].tolist() == want["order"] and r["seg4"].tolist() == want["seg4"]
        assert (r["n_hit"], r["n_miss"], r["n_gated"]) == want["counts"]
        assert np.array_equal(r["base_out"], HAND_BASE[want["order"]]) and r["payload_out"].tolist() == HAND_PAYLOAD[want["order"]].tolist()
    # no query: everything is MISS, in base order
    r = msr.split(HAND_BASE, np.zeros((0, 3), np.float32), HAND_LABEL, (252,))
    assert not r["mark"].any() and r["order"].tolist() == list(range(6)) and r["seg4"].tolist() == [0, 0, 6, 6]


def test_the_host_tool_is_built_and_prints_its_usage():
    assert os.access(TOOL, os.X_OK), "build() did not build scvod_map_split"
    r = subprocess.run([TOOL], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "usage: scvod_map_split <original.pcd> <static.pcd> <out_prefix>" in r.stderr
