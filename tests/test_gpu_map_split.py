"""scvod_map_split_device on the device, through the C-ABI: the neighbour of every query, the mark bytes, the stable three-way partition,
the records and the payload in its order, the segment bounds and the stats against the numpy statement tests/helpers/map_split_ref.py
(an exhaustive look-up, no grid).  Every comparison is bit for bit."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import evaluate_ref as evr  # noqa: E402
import map_split_ref as msr  # noqa: E402
from test_capi_map_split import HAND, HAND_BASE, HAND_LABEL, HAND_NN, HAND_PAYLOAD, HAND_QUERY, TOOL  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
ERR_INVALID, ERR_STATE = -1, -5
OUTPUTS = ("mark", "order", "seg4", "base_out", "payload_out", "nn_idx", "nn_sqdist")
CENTRES = [(0.0, 0.0, 0.0), (-7.0, -3.0, -1.0), (2000.0, -2000.0, 3.0)]


@pytest.fixture(scope="module")
def ctx(scvod):
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    yield c
    c.close()


def _cuda(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


class _Call:
    """one enqueued split: the device buffers (each with a guard behind it) and how to read them back"""

    def __init__(self, scvod, ctx, base, query, label=None, reject=(), payload=None, outputs=OUTPUTS, stream=None, defer=False, **par):
        import torch
        self.ctx = ctx
        base, query = np.ascontiguousarray(base, np.float32), np.ascontiguousarray(query, np.float32)
        self.n, self.m, self.stride = len(base), len(query), base.shape[1]
        self.d_base, self.d_query = _cuda(base), _cuda(query)
        d_label = _cuda(np.asarray(label, np.uint32)) if label is not None else None
        d_pay = _cuda(np.asarray(payload, np.uint32)) if payload is not None else None
        size = dict(mark=(self.n, torch.uint8), order=(self.n, torch.int32), seg4=(4, torch.int64), base_out=(self.n * self.stride, torch.float32),
                    payload_out=(self.n, torch.int32), nn_idx=(self.m, torch.int32), nn_sqdist=(self.m, torch.float32))
        self.size = {k: v[0] for k, v in size.items()}
        self.buf = {}
        for k in outputs:
            if k == "payload_out" and payload is None:
                continue
            t = torch.zeros(size[k][0] + GUARD, dtype=size[k][1], device="cuda")
            t.view(torch.uint8).fill_(0xA5)
            self.buf[k] = t
        self.args = dict(params=scvod.split_params_default(reject_classes=reject, **par), d_base_label=d_label, d_payload_in=d_pay, stream=stream)
        if not defer:
            torch.cuda.synchronize()
            self.go()

    def go(self):
        """enqueue the call; nothing here synchronises"""
        self.ctx.map_split_device(self.d_base, self.d_query, **self.args, **{"d_" + k: v for k, v in self.buf.items()})

    def read(self):
        self.ctx.map_split_stats()   # (waits for the stream of the ctx's last split: this call or a later one in the same stream)
        out = {}
        for k, t in self.buf.items():
            h = t.cpu().numpy()
            assert (h[self.size[k]:].view(np.uint8) == 0xA5).all(), f"{k} was written behind its last entry"
            out[k] = h[:self.size[k]]
        if "base_out" in out:
            out["base_out"] = out["base_out"].reshape(self.n, self.stride)
        if "payload_out" in out:
            out["payload_out"] = out["payload_out"].view(np.uint32)
        return out


def _same(got, want, what):
    for k, v in got.items():
        w = np.asarray(want[k])
        if v.dtype == np.float32:
            v, w = v.view(np.uint32), np.ascontiguousarray(w, np.float32).view(np.uint32)
        assert v.shape == w.shape and np.array_equal(v, w), f"{what}: {k} differs in {int((v != w).sum())} of {v.size} entries"


def _run(scvod, ctx, base, query, label=None, reject=(), payload=None, want=None, what="", **par):
    """the split with every output, compared with the helper; returns (helper's answer, stats)"""
    call = _Call(scvod, ctx, base, query, label, reject, payload, **par)
    st = ctx.map_split_stats()
    got = call.read()
    if want is None:
        want = msr.split(base, query, label, reject, payload)
    _same(got, want, what)
    assert (st["n_hit"], st["n_miss"], st["n_gated"]) == (want["n_hit"], want["n_miss"], want["n_gated"]), what
    assert st["pass1_queries"] + st["ring_queries"] + st["exhaustive_queries"] == len(query), what
    return want, st


# ---- 1. by hand --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reject", [(), (252,)])
def test_by_hand(scvod, ctx, reject):
    call = _Call(scvod, ctx, HAND_BASE, HAND_QUERY, HAND_LABEL, reject, HAND_PAYLOAD)
    st = ctx.map_split_stats()
    got = call.read()
    want = HAND[reject]
    assert got["mark"].tolist() == want["mark"] and got["order"].tolist() == want["order"] and got["seg4"].tolist() == want["seg4"]
    assert np.array_equal(got["base_out"].view(np.uint32), HAND_BASE[want["order"]].view(np.uint32))
    assert got["payload_out"].tolist() == HAND_PAYLOAD[want["order"]].tolist()
    assert got["nn_idx"].tolist() == HAND_NN[0] and got["nn_sqdist"].tolist() == HAND_NN[1]
    assert (st["n_hit"], st["n_miss"], st["n_gated"]) == want["counts"]
    assert (st["pass1_queries"], st["ring_queries"], st["exhaustive_queries"]) == (0, 3, 0)   # 0.25 m and 0.5 m: beyond 0.99 cells of 0.2


# ---- 2. / 8. the normal use, around three centres -----------------------------------------------------------------------------------

def _normal_case(centre):
    rng = np.random.default_rng(20261018)
    base = (rng.uniform(-10, 10, (3000, 3)) + np.asarray(centre)).astype(np.float32)
    half = rng.permutation(3000)[:1500]
    moved = base[rng.permutation(3000)[:200]] + rng.uniform(-0.05, 0.05, (200, 3)).astype(np.float32)
    query = np.concatenate([base[half], moved]).astype(np.float32)
    label = rng.choice([40, 70, 252, 253], 3000).astype(np.uint32) | (rng.integers(0, 1 << 16, 3000).astype(np.uint32) << np.uint32(16))
    return base, query, label


@pytest.mark.parametrize("centre", CENTRES)
def test_the_normal_use(scvod, ctx, centre):
    base, query, label = _normal_case(centre)
    want, st = _run(scvod, ctx, base, query, label, (), label, what=f"normal {centre}")
    assert 1500 <= want["n_hit"] <= 1700 and want["n_gated"] == 0
    assert (st["pass1_queries"], st["ring_queries"], st["exhaustive_queries"]) == (1700, 0, 0), "a cleaned map left the 27-cell pass"
    want, st = _run(scvod, ctx, base, query, label, (252,), label, what=f"normal gated {centre}")
    assert want["n_gated"] > 0 and st["ring_queries"] == 0 and st["exhaustive_queries"] == 0


# ---- 3. / 4. the traps between the passes ----------------------------------------------------------------------------------------------

def _mirrors():
    for axis in range(3):
        for sign in (1.0, -1.0):
            yield axis, sign, (lambda p, axis=axis, sign=sign: (np.roll(np.asarray(p, np.float32), axis, axis=-1) * np.float32(sign)).astype(np.float32))


@pytest.mark.parametrize("b_first", [False, True])
def test_trap_between_the_27_cells_and_the_rings(scvod, ctx, b_first):
    for axis, sign, f in _mirrors():
        q = f([[0.1, 0.1, 0.1]])
        A, B = f([0.39, 0.39, 0.1]), f([0.41, 0.1, 0.1])      # A: inside the 27 cells at 0.41; B: in ring 2 at 0.31
        base = np.array([B, A] if b_first else [A, B], np.float32)
        cq, cb = np.floor(q * np.float32(5)), np.floor(base * np.float32(5))
        assert np.abs(cb - cq).max(axis=1).tolist() == ([2, 1] if b_first else [1, 2])
        call = _Call(scvod, ctx, base, q, cell=0.2)
        st, got = ctx.map_split_stats(), call.read()
        want = msr.split(base, q)
        _same(got, want, f"trap 1 axis {axis} sign {sign}")
        assert got["nn_idx"].tolist() == [0 if b_first else 1]
        assert (st["pass1_queries"], st["ring_queries"], st["exhaustive_queries"]) == (0, 1, 0)


@pytest.mark.parametrize("b_first", [False, True])
def test_trap_between_the_rings_and_the_exhaustive_pass(scvod, ctx, b_first):
    for axis, sign, f in _mirrors():
        q = f([[0.19, 0.1, 0.1]])
        A, B = f([-0.35, 0.1, 0.1]), f([0.61, 0.1, 0.1])      # A': in ring 2 at 0.54; B': in ring 3 at 0.42
        base = np.array([B, A] if b_first else [A, B], np.float32)
        cq, cb = np.floor(q * np.float32(5)), np.floor(base * np.float32(5))
        assert np.abs(cb - cq).max(axis=1).tolist() == ([3, 2] if b_first else [2, 3])
        call = _Call(scvod, ctx, base, q, cell=0.2, max_rings=2)
        st, got = ctx.map_split_stats(), call.read()
        _same(got, msr.split(base, q), f"trap 2 axis {axis} sign {sign}")
        assert got["nn_idx"].tolist() == [0 if b_first else 1]
        assert (st["pass1_queries"], st["ring_queries"], st["exhaustive_queries"]) == (0, 0, 1)


# ---- 5. ties ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("which", ["pass1", "rings", "exhaustive"])
def test_ties_go_to_the_lowest_base_index(scvod, ctx, which, swap):
    # two base points at exactly the same representable distance on either side of the query (1, 0, 0)
    half, n, at = {"pass1": (0.0625, 2, (0, 1)), "rings": (0.3125, 2, (0, 1)), "exhaustive": (2.5, 1500, (70, 1300))}[which]
    rng = np.random.default_rng(5)
    base = rng.uniform(100, 200, (n, 3)).astype(np.float32)            # (the others are far away)
    pair = np.array([[1 - half, 0, 0], [1 + half, 0, 0]], np.float32)
    base[list(at)] = pair[::-1] if swap else pair
    q = np.array([[1.0, 0, 0]], np.float32)
    d = (base[list(at)] - q)
    assert (d[0] ** 2).sum() == (d[1] ** 2).sum() == np.float32(half * half)
    if which == "exhaustive":
        assert (at[0] % 256) // 64 != (at[1] % 256) // 64 and at[0] // 256 != at[1] // 256    # another wave, another stride of the scan
    call = _Call(scvod, ctx, base, q)
    st, got = ctx.map_split_stats(), call.read()
    _same(got, msr.split(base, q), f"tie {which} swap {swap}")
    assert got["nn_idx"].tolist() == [at[0]] and got["nn_sqdist"].tolist() == [half * half]
    assert (st["pass1_queries"], st["ring_queries"], st["exhaustive_queries"]) == {"pass1": (1, 0, 0), "rings": (0, 1, 0), "exhaustive": (0, 0, 1)}[which]


# ---- 6. / 8. independence from the parameters -----------------------------------------------------------------------------------------

def _spread_case(centre):
    rng = np.random.default_rng(6)
    base = np.concatenate([rng.uniform(-5, 5, (2000, 2)), rng.uniform(0, 1, (2000, 1))], axis=1)      # a slab: z in 0..1
    lifted = base[rng.permutation(2000)[:500]].copy()
    lifted[:, 2] = 1.0 + rng.uniform(0.3, 2.7, 500)                                                    # 0.3 .. 3 m from the slab
    far = np.array([40.0, 0, 0]) + rng.normal(0, 0.5, (50, 3))
    query = np.concatenate([base[:450], base[450:950] + rng.normal(0, 0.03, (500, 3)), lifted, far])
    label = rng.choice([40, 252], 2000).astype(np.uint32)
    c = np.asarray(centre)
    return (base + c).astype(np.float32), (query + c).astype(np.float32), label


@pytest.mark.parametrize("centre", CENTRES)
def test_independence_from_cell_and_max_rings(scvod, ctx, centre):
    base, query, label = _spread_case(centre)
    want = msr.split(base, query, label, (252,), label)
    gap = np.sqrt(want["nn_sqdist"][950:1450].astype(np.float64))
    assert gap.min() > 0.25 and gap.max() < 3.2 and np.sqrt(want["nn_sqdist"][1450:].astype(np.float64)).min() > 30
    for cell in (0.1, 0.2, 1.0):
        for rings in (1, 2, 3, 8):
            _, st = _run(scvod, ctx, base, query, label, (252,), label, want=want, what=f"cell {cell} rings {rings} at {centre}", cell=cell,
                         max_rings=rings)
            assert st["exhaustive_queries"] >= 50      # the far ones: no ring of 8 cells of 1 m reaches 30 m
            if rings == 1:
                assert st["ring_queries"] == 0 and st["exhaustive_queries"] > 50
            if cell == 1.0 and rings == 8:
                assert st["exhaustive_queries"] == 50 and st["ring_queries"] > 0


# ---- 7. sizes --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_query", [0, 1, 63, 64, 65, 255, 256, 257])
def test_query_sizes(scvod, ctx, n_query):
    rng = np.random.default_rng(700 + n_query)
    base = rng.uniform(-2, 2, (1000, 3)).astype(np.float32)
    query = rng.uniform(-2.5, 2.5, (n_query, 3)).astype(np.float32)
    want, st = _run(scvod, ctx, base, query, payload=np.arange(1000, dtype=np.uint32), what=f"n_query {n_query}")
    if n_query == 0:
        assert (st["n_hit"], st["n_miss"], st["n_gated"]) == (0, 1000, 0) and want["order"].tolist() == list(range(1000))


@pytest.mark.parametrize("n_base", [0, 1, 2047, 2048, 2049, 4097])
def test_base_sizes(scvod, ctx, n_base):
    rng = np.random.default_rng(800 + n_base)
    base = rng.uniform(-2, 2, (n_base, 3)).astype(np.float32)
    query = rng.uniform(-2.5, 2.5, (300, 3)).astype(np.float32)
    label = rng.choice([40, 252], n_base).astype(np.uint32)
    want, st = _run(scvod, ctx, base, query, label, (252,), label if n_base else None, what=f"n_base {n_base}")
    if n_base == 0:
        assert (want["nn_idx"] == -1).all() and np.isposinf(want["nn_sqdist"]).all() and want["seg4"].tolist() == [0, 0, 0, 0]
        assert (st["pass1_queries"], st["ring_queries"], st["exhaustive_queries"]) == (300, 0, 0)
    else:
        assert want["n_hit"] + want["n_gated"] > 0


# ---- 8. aliased buckets ------------------------------------------------------------------------------------------------------------------

def test_aliased_buckets(scvod, ctx):
    rng = np.random.default_rng(12)
    base = rng.uniform(-250, 250, (40, 3)).astype(np.float32)       # 40 points: 1024 buckets for 2500^3 cells
    query = np.concatenate([base + rng.normal(0, 0.05, (40, 3)), base + rng.normal(0, 0.12, (40, 3)), rng.uniform(-250, 250, (1500, 3))]).astype(np.float32)
    c = np.floor(query[:, None, :] * np.float32(5)).astype(np.int64) + np.asarray([[dx, dy, dz] for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])[None]
    c = c.astype(np.uint32)
    b = (c[..., 0] * np.uint32(73856093) ^ c[..., 1] * np.uint32(19349663) ^ c[..., 2] * np.uint32(83492791)) & np.uint32(1023)
    assert any(len(set(row.tolist())) < 27 for row in b), "no query probes a bucket twice"
    for rings in (1, 3, 8):
        want, st = _run(scvod, ctx, base, query, what=f"aliased rings {rings}", max_rings=rings)
        assert st["exhaustive_queries"] > 1000 and st["pass1_queries"] >= 30


def test_base_cells_that_collide_in_the_hash(scvod, ctx):
    # 30 occupied cells, far from each other, that all hash to ONE of the 1024 buckets: every probe of that bucket meets all 30 points
    g = np.arange(-60, 60, dtype=np.int64)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[::7]
    u = cells.astype(np.uint32)
    bucket = (u[:, 0] * np.uint32(73856093) ^ u[:, 1] * np.uint32(19349663) ^ u[:, 2] * np.uint32(83492791)) & np.uint32(1023)
    same = cells[bucket == bucket[0]]
    rng = np.random.default_rng(8)
    same = same[rng.permutation(len(same))[:30]]
    assert len(same) == 30
    base = ((same + 0.5) * 0.2).astype(np.float32)                    # the cells' centres
    assert np.array_equal(np.floor(base * np.float32(5)).astype(np.int64), same)
    query = np.concatenate([base + rng.uniform(-0.09, 0.09, (30, 3)), base + rng.uniform(-0.5, 0.5, (30, 3)), rng.uniform(-12, 12, (300, 3))]).astype(np.float32)
    want, st = _run(scvod, ctx, base, query, payload=np.arange(30, dtype=np.uint32), what="one bucket")
    assert want["nn_idx"][:30].tolist() == list(range(30)) and st["pass1_queries"] >= 30


# ---- 9. the gate -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reject", [(252,), tuple(range(100, 116))])
def test_the_gate(scvod, ctx, reject):
    rng = np.random.default_rng(len(reject))
    pool = np.asarray(list(reject) + [40, 70, 99, 116, 251], np.uint32)
    base = rng.uniform(-3, 3, (1500, 3)).astype(np.float32)
    label = rng.choice(pool, 1500).astype(np.uint32) | (rng.integers(1, 1 << 16, 1500).astype(np.uint32) << np.uint32(16))   # instance bits
    label[:4] = [reject[0] << 16, reject[0], reject[-1] | 0xFFFF0000, 40]       # the class in the upper half alone is not rejected
    chosen = np.concatenate([np.arange(4), rng.permutation(np.arange(4, 1500))[:700]])
    query = np.concatenate([base[chosen], base[chosen[:300]], base[chosen[:300]] + rng.normal(0, 0.005, (300, 3))]).astype(np.float32)
    want, st = _run(scvod, ctx, base, query, label, reject, label, what=f"gate {reject}")
    rejected = np.isin(label & np.uint32(0xFFFF), reject)
    picks = np.bincount(want["nn_idx"], minlength=1500)
    assert (picks[rejected] > 1).any(), "no rejected point was chosen by several queries"
    assert (want["mark"][rejected & (picks > 0)] == msr.GATED).all() and (want["mark"][rejected & (picks == 0)] == msr.MISS).all()
    assert (rejected & (picks == 0)).any() and want["mark"][:4].tolist() == [1, 2, 2, 1]
    assert not rejected[want["order"][:want["n_hit"]]].any()


# ---- 10. strides ------------------------------------------------------------------------------------------------------------------------

def test_strides(scvod, ctx):
    rng = np.random.default_rng(10)
    base4 = np.concatenate([rng.uniform(-3, 3, (2500, 3)), rng.uniform(0, 255, (2500, 1))], axis=1).astype(np.float32)
    bits = base4.view(np.uint32)
    bits[0, 3], bits[1, 3], bits[2, 3], bits[3, 3] = 0x7FC12345, 0xFFA00001, 0x80000000, 0x7F800000   # NaNs with payloads, -0.0, +inf
    query3 = np.concatenate([base4[::2, :3], base4[1::5, :3] + np.float32(0.01)]).astype(np.float32)
    query4 = np.concatenate([query3, np.full((len(query3), 1), np.nan, np.float32)], axis=1)
    payload = rng.integers(0, 1 << 32, 2500, dtype=np.uint64).astype(np.uint32)
    payload[:3] = [0xFFFFFFFF, 0x80000000, 0x7FC00000]
    want3 = msr.split(base4[:, :3], query4[:, :3], payload=payload)
    for sb, sq in itertools.product((3, 4), repeat=2):
        base = np.ascontiguousarray(base4[:, :sb])
        want = dict(want3)
        if sb == 4:
            want["base_out"] = bits[want3["order"]].view(np.float32)       # the whole records, the intensity word included
        got, _ = _run(scvod, ctx, base, np.ascontiguousarray(query4[:, :sq]), payload=payload, want=want, what=f"strides {sb} / {sq}")
    assert want3["order"][:want3["n_hit"]].min() == 0 and set(bits[want["order"], 3][:50].tolist()) & {0x7FC12345, 0x80000000}


# ---- 11. optional outputs ---------------------------------------------------------------------------------------------------------------

def test_every_subset_of_optional_outputs(scvod, ctx):
    rng = np.random.default_rng(11)
    base = rng.uniform(-1, 1, (2300, 3)).astype(np.float32)
    query = np.concatenate([base[::3], rng.uniform(-1.5, 1.5, (150, 3))]).astype(np.float32)
    label = rng.choice([40, 252], 2300).astype(np.uint32)
    want = msr.split(base, query, label, (252,), label)
    for r in range(len(OUTPUTS) + 1):
        for subset in itertools.combinations(OUTPUTS, r):
            call = _Call(scvod, ctx, base, query, label, (252,), label, outputs=subset)
            st = ctx.map_split_stats()
            got = call.read()
            assert set(got) == set(subset)
            _same(got, want, f"outputs {subset}")
            assert (st["n_hit"], st["n_miss"], st["n_gated"]) == (want["n_hit"], want["n_miss"], want["n_gated"]), subset


# ---- 12. repeatability and stream order -------------------------------------------------------------------------------------------------

def test_repeatable_and_stream_ordered(scvod):
    import torch
    from test_gpu_async_chain import _stream
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    base, query, label = _spread_case((0.0, 0.0, 0.0))
    small = (base[:300], query[:200], label[:300])
    big = (base, query, label)
    runs = [_Call(scvod, c, *big, (252,), label).read() for _ in range(2)]
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    # back to back on a side stream, nothing synchronises in between: small then big (the scratch grows under the first), then small again
    c2 = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    s = _stream()
    calls = [_Call(scvod, c2, b, q, lab, (252,), lab, stream=s.cuda_stream, defer=True) for b, q, lab in (small, big, small)]
    torch.cuda.synchronize()
    for call in calls:
        call.go()
    st = c2.map_split_stats()
    s.synchronize()
    for call, (b, q, lab) in zip(calls, (small, big, small)):
        _same(call.read(), msr.split(b, q, lab, (252,), lab), f"back to back, {len(b)} base points")
    w = msr.split(*small[:2], small[2], (252,), small[2])
    assert (st["n_hit"], st["n_miss"], st["n_gated"]) == (w["n_hit"], w["n_miss"], w["n_gated"])      # the stats are the last call's
    c.close()
    c2.close()


# ---- 13. side effects -------------------------------------------------------------------------------------------------------------------

def test_stats_before_the_first_split_and_argument_errors_of_a_live_ctx(scvod):
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    out = np.zeros(8, np.int64)
    assert c.map_split_scratch_bytes() == 0
    assert c.lib.scvod_map_split_stats(c.h, out.ctypes.data_as(C.c_void_p)) == ERR_STATE
    z = np.zeros(64, np.int64).ctypes.data_as(C.c_void_p)
    bad = scvod.split_params_default(max_rings=9)
    assert c.lib.scvod_map_split_device(c.h, z, None, 1, z, 1, C.byref(bad), None, None, None, None, None, None, None, None, None) == ERR_INVALID
    assert c.lib.scvod_map_split_device(c.h, z, None, -1, z, 1, None, None, None, None, None, None, None, None, None, None) == ERR_INVALID
    assert c.lib.scvod_map_split_device(c.h, None, None, 1, z, 1, None, None, None, None, None, None, None, None, None, None) == ERR_INVALID
    assert c.map_split_scratch_bytes() == 0 and c.arena_bytes() > 0 and not out.any()
    c.close()


def test_side_effects_on_a_tracked_batch(scvod):
    import torch
    from test_gpu_evaluate import _k6
    k = _k6(scvod)
    b, ctx = k["b"], k["ctx"]
    n = int(b.offs[-1])
    rng = np.random.default_rng(13)
    gt = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    glab = rng.choice([40, 252], 500).astype(np.uint32)
    ctx.evaluate_device(_cuda(gt), _cuda(glab), _cuda(gt[::2]), _cuda(glab[::2]))
    ev0 = ctx.evaluate_stats()
    before = (ctx.arena_bytes(), ctx.evaluate_scratch_bytes(), ctx.score_classes_scratch_bytes())
    lab0 = ctx.batch_point_labels().cpu().numpy()[:n].copy()
    grown = [ctx.map_split_scratch_bytes()]
    assert grown[0] == 0
    base, query, label = _normal_case((0.0, 0.0, 0.0))
    for nb in (500, 3000, 1000):
        _run(scvod, ctx, base[:nb], query[:nb // 2], label[:nb], (252,), label[:nb], what=f"after the batch, {nb} base points")
        grown.append(ctx.map_split_scratch_bytes())
    assert 0 < grown[1] < grown[2] == grown[3]
    assert (ctx.arena_bytes(), ctx.evaluate_scratch_bytes(), ctx.score_classes_scratch_bytes()) == before
    ev1 = ctx.evaluate_stats()
    assert all(ev0[key] == ev1[key] for key in evr.COUNTS)
    assert np.array_equal(ctx.batch_point_labels().cpu().numpy()[:n], lab0)
    torch.cuda.synchronize()


# ---- 14. into the consumer ---------------------------------------------------------------------------------------------------------------

def test_the_split_feeds_classify_map_device(scvod, ctx):
    import torch
    base, query, label = _normal_case((0.0, 0.0, 0.0))
    rng = np.random.default_rng(14)
    query = np.concatenate([query, base[:400] + rng.normal(0, 0.08, (400, 3))]).astype(np.float32)
    call = _Call(scvod, ctx, base, query, label, (252,))
    ctx.map_split_stats()
    # on the device: mark == 1 is the predicted-static byte, the HIT segment the static cloud, the MISS segment the dynamic cloud
    seg = [int(v) for v in call.buf["seg4"][:4].cpu().numpy()]
    pred = (call.buf["mark"][:len(base)] == scvod.SPLIT_HIT).to(torch.uint8).contiguous()
    rec = call.buf["base_out"][:3 * len(base)].view(-1, 3)
    static, dynamic = rec[seg[0]:seg[1]].contiguous(), rec[seg[1]:seg[2]].contiguous()
    cls = torch.full((len(base) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.classify_map_device(call.d_base, pred, static, dynamic, d_class=cls)
    st = ctx.classify_map_stats()
    want = msr.split(base, query, label, (252,))
    o = want["order"]
    w_cls, w_counts = evr.classify(base, want["mark"] == msr.HIT, base[o[:want["n_hit"]]], base[o[want["n_hit"]:want["n_hit"] + want["n_miss"]]],
                                   nn_fn=evr.brute_nn)
    h = cls.cpu().numpy()
    assert np.array_equal(h[:len(base)], w_cls) and (h[len(base):] == 0xA5).all()
    assert [st[key] for key in evr.CLASS_NAMES] == w_counts.tolist()
    assert w_counts[1] == want["n_hit"] and w_counts[3] >= want["n_miss"] and want["n_gated"] > 0


# ---- the host tool -----------------------------------------------------------------------------------------------------------------------

def _write_pcd(path, xyzi):
    with open(path, "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
                f"WIDTH {len(xyzi)}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {len(xyzi)}\nDATA ascii\n")
        for p in xyzi:
            f.write(" ".join(repr(float(v)) for v in p) + "\n")


def _read_pcd(path):
    lines = open(path).read().splitlines()
    at = lines.index("DATA ascii")
    return np.array([[float(v) for v in ln.split()] for ln in lines[at + 1:] if ln], np.float32).reshape(-1, 4)


def test_the_host_tool_writes_the_dynamic_cloud(tmp_path):
    rng = np.random.default_rng(15)
    grid = np.unique(rng.integers(-40, 40, (400, 3)), axis=0)
    grid = grid[rng.permutation(len(grid))] / 8.0                       # (multiples of 1/8 and 1/64: exact in the 8 digits an ASCII file keeps)
    ori = np.concatenate([grid, rng.choice([40.0, 252.0, 70.0], (len(grid), 1))], axis=1).astype(np.float32)
    stat = ori[rng.random(len(ori)) < 0.6].copy()
    stat[:, :3] += np.float32(1 / 64)
    _write_pcd(tmp_path / "ori.pcd", ori)
    _write_pcd(tmp_path / "static.pcd", stat)
    prefix = str(tmp_path / "out_")
    r = subprocess.run([TOOL, str(tmp_path / "ori.pcd"), str(tmp_path / "static.pcd"), prefix], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = msr.split(ori, stat)
    got = _read_pcd(prefix + "dynamic_cloud.pcd")
    assert 0 < want["n_miss"] < len(ori)
    assert np.array_equal(got.view(np.uint32), want["base_out"][want["n_hit"]:want["n_hit"] + want["n_miss"]].view(np.uint32))
    # segDF's evaluation block: the hit points whose label (the intensity field) is not 252
    r = subprocess.run([TOOL, str(tmp_path / "ori.pcd"), str(tmp_path / "static.pcd"), prefix, "--reject", "252", "--static-out",
                        str(tmp_path / "eva_static.pcd")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = msr.split(ori, stat, ori[:, 3].astype(np.uint32), (252,))
    got = _read_pcd(tmp_path / "eva_static.pcd")
    assert want["n_gated"] > 0 and np.array_equal(got.view(np.uint32), want["base_out"][:want["n_hit"]].view(np.uint32))
    assert not (got[:, 3] == 252).any()
