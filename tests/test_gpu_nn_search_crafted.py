"""The correspondence search (A7) on the crafted clouds of tests/helpers/nn_search_cases.py: every case through scvod_nn_search,
scvod_nn_radius_search (where the radius is positive) and scvod_nn_search_device, against the brute-force oracle.  idx, the bits of
sqdist and within / found are compared with np.array_equal; every output array has guard words before and after it.
tests/test_nn_search_cases.py holds the cases themselves to the properties they are named for."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import nn_search_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 16       # elements before and after every output array
CSRC = os.path.join(os.path.dirname(HERE), "dr-using-scv-od_amd", "csrc")


@pytest.fixture(scope="module")
def ctx(scvod):
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    yield c
    c.close()


# ---- the three entry points, with guards ----------------------------------------------------------------------------------------------------

def _host_out(n, dtype):
    a = np.empty(n + 2 * GUARD, dtype)
    a.view(np.uint8)[:] = 0xA5
    return a


def _host_read(a, n, what):
    b, g = a.view(np.uint8), GUARD * a.itemsize
    assert (b[:g] == 0xA5).all() and (b[g + n * a.itemsize:] == 0xA5).all(), f"{what}: written outside its {n} entries"
    return a[GUARD:GUARD + n].copy()


def _hp(a, guarded=True):
    return C.c_void_p(a.ctypes.data + (GUARD * a.itemsize if guarded else 0)) if a.size else None


def host_search(ctx, m, q, radius, bounded=False):
    """scvod_nn_search / scvod_nn_radius_search -> (idx, sqdist, within or None)"""
    m, q = np.ascontiguousarray(m, F), np.ascontiguousarray(q, F)
    n = len(q)
    idx, sq, w = _host_out(n, np.int32), _host_out(n, F), _host_out(n, np.uint8)
    if bounded:
        rc = ctx.lib.scvod_nn_radius_search(ctx.h, _hp(m, False), len(m), _hp(q, False), n, float(radius), _hp(idx), _hp(sq))
    else:
        rc = ctx.lib.scvod_nn_search(ctx.h, _hp(m, False), len(m), _hp(q, False), n, float(radius), _hp(idx), _hp(sq), _hp(w))
    assert rc == 0, ctx.last_error() if hasattr(ctx, "last_error") else rc
    return _host_read(idx, n, "idx"), _host_read(sq, n, "sqdist"), _host_read(w, n, "within") if not bounded else None


class DeviceCall:
    """scvod_nn_search_device: the buffers of one call; go() only enqueues, read() waits for the whole device"""

    def __init__(self, ctx, m, q, radius, stream=None):
        import torch
        self.ctx, self.n, self.radius, self.stream = ctx, len(q), float(radius), stream
        self.d_m = torch.from_numpy(np.ascontiguousarray(m, F).copy()).cuda()
        self.d_q = torch.from_numpy(np.ascontiguousarray(q, F).copy()).cuda()
        self.out = {}
        for k, dt in (("idx", torch.int32), ("sq", torch.float32), ("w", torch.uint8)):
            t = torch.empty(self.n + 2 * GUARD, dtype=dt, device="cuda")
            t.view(torch.uint8).fill_(0xA5)
            self.out[k] = t
        torch.cuda.synchronize()

    def _p(self, t, guarded=True):
        return C.c_void_p(t.data_ptr() + (GUARD * t.element_size() if guarded else 0)) if t.numel() else None

    def go(self):
        o = self.out
        rc = self.ctx.lib.scvod_nn_search_device(self.ctx.h, self._p(self.d_m, False), int(self.d_m.shape[0]), self._p(self.d_q, False), self.n,
                                                 self.radius, self._p(o["idx"]), self._p(o["sq"]), self._p(o["w"]),
                                                 C.c_void_p(self.stream) if self.stream else None)
        assert rc == 0, rc
        return self

    def read(self):
        import torch
        torch.cuda.synchronize()
        got = []
        for k in ("idx", "sq", "w"):
            h = self.out[k].cpu().numpy()
            got.append(_host_read(h, self.n, "device " + k))
        return tuple(got)


def _same(got, want, what):
    (gi, gs, gw), (wi, ws, ww) = got, want
    bad = np.flatnonzero((gi != wi) | (gs.view(np.uint32) != np.ascontiguousarray(ws, F).view(np.uint32)))
    detail = [(int(k), int(gi[k]), float(gs[k]), int(wi[k]), float(ws[k])) for k in bad[:8]]
    assert np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), np.ascontiguousarray(ws, F).view(np.uint32)), \
        f"{what}: {len(bad)} of {len(wi)} queries differ; (query, idx, sqdist, oracle's idx, sqdist) {detail}"
    if gw is not None:
        assert np.array_equal(gw, ww), f"{what}: within differs at {np.flatnonzero(gw != ww)[:8].tolist()}"


def check(ctx, oracle, case, reverse=False, stream=None):
    """the case through the three forms against the oracle"""
    m = case.map[::-1] if reverse else case.map
    want = nc.expected(oracle, case, reverse)
    what = case.name + (" (map reversed)" if reverse else "")
    _same(host_search(ctx, m, case.query, case.radius), want, what + ": nn_search")
    _same(DeviceCall(ctx, m, case.query, case.radius, stream).go().read(), want, what + ": nn_search_device")
    if case.radius > 0:
        bi, bs, bw = nc.bounded(*want)
        gi, gs, _ = host_search(ctx, m, case.query, case.radius, bounded=True)
        _same((gi, gs, (gi >= 0).astype(np.uint8)), (bi, bs, bw), what + ": nn_radius_search")
    return want


# ---- the radius sliver ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", range(3))
@pytest.mark.parametrize("radius", nc.SLIVER_RADII)
def test_radius_sliver(scvod, oracle, ctx, radius, axis):
    """A neighbour inside the radius, but so close to its rim that fp32 cell coordinates put it two cells from the query when the cell edge
    is the radius; and the same with a candidate inside the 27 cells that is slightly farther.  The map's first point sets the host form's
    grid origin (the min corner) to the one the pairs were found for."""
    case = nc.sliver_case(radius, axis)
    idx, sq, within = check(ctx, oracle, case)
    assert all(idx[q] == p for q, p, _ in case.meta["nearer"]) and all(within[q] for q, _ in case.meta["pairs"])


# ---- the radius edge and the acceptance edge -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("threshold,radius", nc.EDGE_CALLS)
def test_threshold_edges(scvod, oracle, ctx, threshold, radius):
    """d^2 bit-equal to fl(r * r) (strictly below is inside, equal is not) or to launch_nn's h2 (at or below: the grid's answer; above: the
    brute-force list's), and one ulp on either side"""
    for axis in range(3):
        case = nc.edge_case(threshold, radius, axis)
        idx, sq, within = check(ctx, oracle, case)
        T = case.meta["threshold"]
        assert {int(np.sign(int(sq[q].view(np.uint32)) - int(T.view(np.uint32)))) for q, _, _ in case.meta["edges"]} == {-1, 0, 1}


@pytest.mark.parametrize("first", ["outside", "inside"])
def test_tie_between_the_27_cells_and_the_list(scvod, oracle, ctx, first):
    for axis in range(3):
        case = nc.list_tie_case(axis, first)
        idx, sq, within = check(ctx, oracle, case)
        assert idx.tolist() == [1] and sq.tolist() == [0.0625]


# ---- ties -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reverse", [False, True])
def test_ties_go_to_the_lowest_index(scvod, oracle, ctx, reverse):
    for case in nc.tie_cases():
        idx, sq, within = check(ctx, oracle, case, reverse)
        n = len(case.map)
        for q, tied in case.meta["tie"]:
            assert idx[q] == (min(n - 1 - t for t in tied) if reverse else min(tied)), case.name


# ---- cell faces -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", [0.15, 0.3])
def test_points_on_cell_faces(scvod, oracle, ctx, radius):
    for axis in range(3):
        check(ctx, oracle, nc.face_case(radius, axis))


# ---- the hash ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", nc.hash_cases(), ids=lambda c: c.name)
def test_hash(scvod, oracle, ctx, case):
    idx, sq, within = check(ctx, oracle, case)
    assert 0 < within.sum() < len(case.query)


# ---- the brute-force list -----------------------------------------------------------------------------------------------------------------

def _source_int(name):
    for f in sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".inc", ".h"))):
        m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, f)).read())
        if m:
            return int(m.group(1))
    raise AssertionError(name + " not found in the source")


@pytest.mark.parametrize("n_map", nc.LIST_MAP_SIZES)
def test_list_sizes(scvod, oracle, ctx, n_map):
    assert _source_int("kNnTile") == 2048 and _source_int("kNnThreads") == 256, "the sizes of this test are set around these"
    for n_query in nc.LIST_LENGTHS:
        idx, sq, within = check(ctx, oracle, nc.list_case(n_map, n_query))
        assert sq.min() >= 400 and (idx[0] == 0)


def test_list_longer_than_one_round_of_the_grid(scvod, oracle, ctx):
    """k_nn_brute_list runs 2 * kPersistCUs workgroups of kNnThreads queries: one query more than twice that, so the grid-stride loop
    comes round a second time and its last round is a single query"""
    n_query = 2 * _source_int("kPersistCUs") * _source_int("kNnThreads") + 1
    case = nc.list_case(2049, n_query)
    idx, sq, within = check(ctx, oracle, case)
    assert len(idx) == n_query > 100000 and sq.min() >= 400


# ---- far coordinates ----------------------------------------------------------------------------------------------------------------------

def test_far_coordinates(scvod, oracle, ctx):
    idx, sq, within = check(ctx, oracle, nc.far_case())
    assert 0 < within.sum() < len(within)


# ---- call sequences on one ctx --------------------------------------------------------------------------------------------------------------

def test_sizes_grow_then_shrink_and_empty_calls(scvod, oracle):
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    empty = np.zeros((0, 3), F)
    big = nc.near_case(6000, 4000)
    seq = [nc.near_case(40, 30), nc.list_case(2049, 700), big, nc.near_case(300, 200, radius=0.3), nc.list_case(1, 1), nc.near_case(40, 30)]
    for case in seq:            # the scratch grows, then serves smaller calls; a long list is followed by short ones (the count restarts at 0)
        check(c, oracle, case)
    assert (nc.expected(oracle, big)[1] > F(0.0392)).sum() > 400 and (nc.expected(oracle, seq[-1])[1] <= F(0.0392)).sum() > 10
    for m, q in ((big.map, empty), (empty, big.query[:300]), (empty, empty)):
        case = nc.Case(f"empty {len(m)} x {len(q)}", m, q, 0.25, {})
        idx, sq, within = check(c, oracle, case)
        assert len(idx) == len(q) and (idx == -1).all() and not within.any()
    check(c, oracle, seq[0])
    c.close()


def test_device_form_on_a_stream_that_is_not_the_current_one(scvod, oracle):
    import torch
    c = scvod.Ctx(scvod.make_params("semantickitti"), max_points_total=1024, max_scans=1)
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    cases = [nc.near_case(300, 200), nc.near_case(5000, 3000), nc.list_case(2049, 257), nc.near_case(300, 200)]
    calls = [DeviceCall(c, k.map, k.query, k.radius, stream=s.cuda_stream) for k in cases]
    for call in calls:          # back to back, nothing synchronises in between: the scratch grows under the first
        call.go()
    s.synchronize()
    for call, k in zip(calls, cases):
        _same(call.read(), nc.expected(oracle, k), k.name + ": back to back on a side stream")
    c.close()
