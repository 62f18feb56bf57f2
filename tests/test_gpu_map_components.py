"""scvod_map_components and scvod_map_component_visibility on the device (csrc/scvod_mapcomp.hip) against the plain statement of
tests/helpers/map_components_ref.py, byte for byte, with guard regions around every output.  The lists are the crafted ones of
tests/helpers/map_components_cases.py; the maps are filled through merge, as tests/test_gpu_map_table.py fills its tables."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import map_components_cases as mk  # noqa: E402
import map_components_ref as mc  # noqa: E402
import map_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, ERR_CAPACITY = -1, -4
G = 16                                  # guard elements on either side of an output
SENT32, SENT8 = 0x55555555, 0x55
CASES = {c["id"]: c for c in mk.gpu_cases()}
SMALL = [c["id"] for c in mk.hand_worked()]
EVERY_CONN = SMALL + ["random_01", "random_03"]
PAIRS = [(cid, conn) for cid in CASES for conn in ((6, 18, 26) if cid in EVERY_CONN else (6, 26))]


def _status(excinfo):
    m = re.match(r"status (-?\d+)", str(excinfo.value))
    assert m, str(excinfo.value)
    return int(m.group(1))


@functools.lru_cache(maxsize=None)
def _ref(cid, conn):
    c = CASES[cid]
    return mc.components(c["list"], c["map"], conn)


def _pow2(n):
    c = 1024
    while c < n:
        c <<= 1
    return c


def _map_of(scvod, keys, capacity=None, order=None, chunks=1, kind=None, vals=None):
    keys = np.asarray(keys, np.uint64)
    m = scvod.StaticMap(capacity or _pow2(2 * len(keys)), kind=scvod.MAP_KIND_PLAIN if kind is None else kind)
    if len(keys):
        v = (keys * np.uint64(2654435761)) >> np.uint64(1) if vals is None else np.asarray(vals, np.uint64)
        o = np.arange(len(keys)) if order is None else order
        rec = mr.to_device(keys[o], v[o])
        for part in np.array_split(np.arange(len(keys)), chunks):
            if len(part):
                m.merge(rec[int(part[0]):int(part[-1]) + 1])
        assert m.count() == len(np.unique(keys))
    return m


def _guarded(torch, n, dtype, fill):
    t = torch.full((n + 2 * G,), fill, dtype=dtype, device="cuda")
    return t, t[G:G + n] if n else t[G:G]


def _run(scvod, m, list_keys, conn, cap=None, stream=None):
    """scvod_map_components through the C ABI into guarded outputs: (status, component, table, n, guards untouched)"""
    import torch
    k = np.asarray(list_keys, np.uint64)
    n = len(k)
    rec = mr.to_device(k, k ^ np.uint64(0x1234)) if n else None
    cap = n if cap is None else cap
    comp_all, comp = _guarded(torch, n, torch.int32, SENT32)
    tab_all = torch.full(((cap + 2 * G) * 48,), SENT8, dtype=torch.uint8, device="cuda")
    n_all, d_n = _guarded(torch, 1, torch.int64, SENT32)
    rc = m.lib.scvod_map_components(m.h, C.c_void_p(rec.data_ptr()) if n else None, n, conn, C.c_void_p(comp_all.data_ptr() + 4 * G) if n else None,
                                    C.c_void_p(tab_all.data_ptr() + 48 * G), cap, C.c_void_p(n_all.data_ptr() + 8 * G), C.c_void_p(stream or 0))
    torch.cuda.synchronize()
    hc, ht, hn = comp_all.cpu().numpy(), tab_all.cpu().numpy(), n_all.cpu().numpy()
    clean = (hc[:G] == SENT32).all() and (hc[G + n:] == SENT32).all() and (ht[:48 * G] == SENT8).all() and (ht[48 * (G + cap):] == SENT8).all() and \
        (hn[:G] == SENT32).all() and (hn[G + 1:] == SENT32).all()
    return rc, hc[G:G + n].copy(), ht[48 * G:48 * (G + cap)].copy(), int(hn[G]), clean


def _check(scvod, m, case, conn, ref=None, what=""):
    ref = _ref(case["id"], conn) if ref is None else ref
    rc, comp, tab, n, clean = _run(scvod, m, case["list"], conn)
    assert rc == 0 and clean, what
    nc = len(ref["table"])
    assert n == nc, (what, n, nc)
    assert np.array_equal(comp, ref["component"]), what
    assert tab[:48 * nc].tobytes() == ref["table"].tobytes(), what
    assert (tab[48 * nc:] == SENT8).all(), what                    # nothing behind the components either
    assert list(m.components_stats().values()) == ref["stats"], what
    return comp, tab[:48 * nc]


@pytest.mark.parametrize("cid,conn", PAIRS, ids=["%s-%d" % p for p in PAIRS])
def test_device_equals_the_helper(scvod, cid, conn):
    case = CASES[cid]
    m = _map_of(scvod, case["map"])
    _check(scvod, m, case, conn, what=cid)
    if case["count"]:
        assert m.components_stats()["components"] == case["count"][conn]
    m.close()


def test_an_empty_list(scvod):
    m = _map_of(scvod, CASES["snake"]["map"])
    rc, comp, tab, n, clean = _run(scvod, m, np.zeros(0, np.uint64), 26, cap=4)
    assert rc == 0 and clean and n == 0 and len(comp) == 0 and (tab == SENT8).all()
    assert list(m.components_stats().values()) == [0] * 8
    out = m.components(mr.to_device(np.zeros(0, np.uint64), np.zeros(0, np.uint64)).reshape(0, 2))
    assert out["n"].cpu().tolist() == [0] and out["component"].numel() == 0
    m.close()


def test_a_table_at_load_095_with_wrapping_chains(scvod):
    """972 neighbouring cells in a table of 1024 slots: a box is moved until the table's longest run of occupied slots crosses the end
    of the table (and stays below the probe bound), so own-cell walks and neighbour walks wrap"""
    capacity, n = 1024, 972
    rng = np.random.default_rng(21)
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij"), axis=-1).reshape(-1, 3)
    g = g[rng.permutation(len(g))[:n]]
    for shift in range(4000):
        keys = mr.pack_key(g[:, 0] + shift, g[:, 1] - 3 * shift, g[:, 2] + 7)
        run, wraps = mr.longest_run(mr.simulate_table(keys, capacity))
        if wraps and 100 <= run <= 400:
            break
    assert wraps and 100 <= run <= 400, "no shift gives a wrapping run inside the probe bound"
    m = _map_of(scvod, keys, capacity=capacity, chunks=3)
    assert m.lib.scvod_map_capacity(m.h) == capacity
    lk = keys[rng.permutation(n)]
    for conn in (6, 26):
        case = {"id": "load95", "list": lk, "map": keys}
        ref = mc.components(lk, keys, conn)
        assert 1 <= len(ref["table"]) < n
        _check(scvod, m, case, conn, ref=ref, what="load 0.95, %d" % conn)
    m.close()


def test_invariance_under_order_capacity_insertion_and_run(scvod):
    case = CASES["random_01"]
    conn = 18
    ref = _ref("random_01", conn)
    m = _map_of(scvod, case["map"])
    comp, tab = _check(scvod, m, case, conn)
    comp2, tab2 = _check(scvod, m, case, conn, what="the call run twice")
    assert np.array_equal(comp, comp2) and tab.tobytes() == tab2.tobytes()
    # the list permuted: the same table but for first_record, d_component permuted accordingly
    rng = np.random.default_rng(31)
    perm = rng.permutation(len(case["list"]))
    rc, pcomp, ptab, n, clean = _run(scvod, m, case["list"][perm], conn)
    assert rc == 0 and clean and n == len(ref["table"])
    assert np.array_equal(pcomp, comp[perm])
    a, b = np.frombuffer(tab.tobytes(), mc.COMPONENT_DTYPE), np.frombuffer(ptab[:48 * n].tobytes(), mc.COMPONENT_DTYPE)
    for f in ("key", "n_records", "cell_min", "cell_max", "reserved"):
        assert np.array_equal(a[f], b[f]), f
    inv = np.argsort(perm)
    assert np.array_equal(b["first_record"], np.array([inv[comp == c].min() for c in range(n)]))
    pref = mc.components(case["list"][perm], case["map"], conn)
    assert ptab[:48 * n].tobytes() == pref["table"].tobytes()
    m.close()
    # the same cells in maps of two capacities and two insertion orders
    for capacity, order, chunks in ((1 << 15, None, 1), (1 << 17, rng.permutation(len(case["map"])), 5)):
        q = _map_of(scvod, case["map"], capacity=capacity, order=order, chunks=chunks)
        c3, t3 = _check(scvod, q, case, conn, what="capacity %d" % capacity)
        assert np.array_equal(c3, comp) and t3.tobytes() == tab.tobytes()
        q.close()


def test_a_table_one_record_short(scvod):
    case = CASES["random_01"]
    ref = _ref("random_01", 26)
    nc = len(ref["table"])
    m = _map_of(scvod, case["map"])
    rc, comp, tab, n, clean = _run(scvod, m, case["list"], 26, cap=nc - 1)
    assert rc == 0 and clean                                          # (nothing at or behind cap_table: the guard begins there)
    assert n == nc and np.array_equal(comp, ref["component"])         # d_component and d_n are complete all the same
    assert tab.tobytes() == ref["table"][:nc - 1].tobytes()
    o = (C.c_int64 * 8)()
    assert m.lib.scvod_map_components_stats(m.h, o) == ERR_CAPACITY
    assert list(o) == ref["stats"][:6] + [nc - 1, 1]
    with pytest.raises(scvod.ScvodError) as e:
        m.components_stats()
    assert _status(e) == ERR_CAPACITY
    _check(scvod, m, case, 26, what="the next call with a table that is big enough")
    # no table at all is no overflow
    out = m.components(mr.to_device(case["list"], case["list"]), want=("component", "n"))
    assert out["n"].cpu().tolist() == [nc] and np.array_equal(out["component"].cpu().numpy(), ref["component"])
    assert m.components_stats()["overflow"] == 0 and m.components_stats()["written"] == 0
    m.close()


def test_a_labelled_map_joins_through_ground_only_when_ground_is_listed(scvod):
    """two 3 x 3 x 3 blocks of label 4 standing on a strip of label-1 cells: one component with every label selected, two without 1"""
    a = [(x, y, z) for x in range(3) for y in range(3) for z in range(1, 4)]
    b = [(x + 10, y, z) for (x, y, z) in a]
    ground = [(x, y, 0) for x in range(-2, 15) for y in range(3)]
    cells = np.array(a + b + ground, np.int64)
    keys = mr.pack_key(cells[:, 0], cells[:, 1], cells[:, 2])
    label = np.array([4] * (len(a) + len(b)) + [1] * len(ground), np.uint64)
    vals = mr.pack_val(100, 200, 300, 0) | (label << np.uint64(8)) | np.uint64(9)
    m = _map_of(scvod, keys, kind=scvod.MAP_KIND_LABELLED, vals=vals)
    for select, want in ((None, 1), ([v for v in range(256) if v != 1], 2)):
        pts, lab, recs = m.points_labelled(select=select)
        lk = recs.cpu().numpy().view(np.uint64)[:, 0]
        assert len(lk) == (len(keys) if select is None else len(a) + len(b))
        out = m.components(recs.contiguous())
        ref = mc.components(lk, keys, 26)
        assert len(ref["table"]) == want
        assert out["n"].cpu().tolist() == [want]
        assert np.array_equal(out["component"].cpu().numpy(), ref["component"])
        assert out["table"].cpu().numpy()[:want].tobytes() == ref["table"].tobytes()
        assert list(m.components_stats().values()) == ref["stats"]
    m.close()


def test_no_other_stage_moves(scvod):
    import torch
    case = CASES["mixed"]
    m = _map_of(scvod, case["map"])
    pts, recs = m.points()
    q = m.query(pts.contiguous(), [0, len(pts)], radius=0.1, want=("result",))
    f = m.filter(pts.contiguous(), [0, len(pts)], want=("side",))
    torch.cuda.synchronize()
    before = (m.query_stats(), m.query_scratch_bytes(), m.filter_stats(), m.filter_scratch_bytes(), m.scratch_bytes(), m.count(),
              mr.sorted_records(m)[0].tobytes(), mr.sorted_records(m)[1].tobytes())
    assert m.components_scratch_bytes() == 0                          # nothing is allocated before the first call
    _check(scvod, m, case, 26)
    comp = m.components(mr.to_device(case["list"], case["list"]))
    ver = torch.randint(0, 3, (len(case["list"]),), dtype=torch.uint8, device="cuda")
    m.component_visibility(comp, ver)
    m.component_visibility_stats()
    s0 = m.components_scratch_bytes()
    assert s0 > 0
    _check(scvod, m, case, 6)
    assert m.components_scratch_bytes() == s0                         # grow-only: the same list needs no more
    after = (m.query_stats(), m.query_scratch_bytes(), m.filter_stats(), m.filter_scratch_bytes(), m.scratch_bytes(), m.count(),
             mr.sorted_records(m)[0].tobytes(), mr.sorted_records(m)[1].tobytes())
    assert before == after
    m.close()


def test_bad_arguments_on_a_live_map(scvod):
    import torch
    m = _map_of(scvod, CASES["snake"]["map"])
    lib, h = m.lib, m.h
    n = 64
    rec = mr.to_device(CASES["snake"]["list"][:n], CASES["snake"]["list"][:n])
    buf = torch.zeros(8192, dtype=torch.int64, device="cuda")
    r, b = rec.data_ptr(), buf.data_ptr()
    P = C.c_void_p
    comp, tab, dn = b, b + 1024, b + 8192
    good = lambda: [h, P(r), n, 26, P(comp), P(tab), n, P(dn), None]   # noqa: E731

    def bad(i, v):
        a = good()
        a[i] = v
        return lib.scvod_map_components(*a)

    assert bad(2, -1) == INVALID and bad(2, 1 << 31) == INVALID        # n
    assert bad(1, None) == INVALID                                     # NULL records with n > 0
    for conn in (0, 4, 8, 27, -6):
        assert bad(3, conn) == INVALID
    assert bad(1, P(r + 4)) == INVALID and bad(4, P(comp + 2)) == INVALID and bad(5, P(tab + 4)) == INVALID and bad(7, P(dn + 4)) == INVALID
    assert bad(6, -1) == INVALID                                       # cap_table
    assert bad(7, None) == INVALID                                     # a table without d_n
    assert bad(4, P(r)) == INVALID and bad(5, P(r + 512)) == INVALID and bad(7, P(r + 8)) == INVALID     # an output over the records
    assert bad(5, P(comp + 8)) == INVALID and bad(7, P(comp)) == INVALID and bad(7, P(tab + 48)) == INVALID   # outputs over each other
    assert m.components_scratch_bytes() == 0                           # refused before anything was allocated
    o = (C.c_int64 * 8)()
    assert lib.scvod_map_components_stats(h, o) == -5                  # SCVOD_ERR_STATE: no call yet
    assert lib.scvod_map_component_visibility_stats(h, o) == -5
    assert lib.scvod_map_components(*good()) == 0
    # the vote
    ver = torch.zeros(n, dtype=torch.uint8, device="cuda")
    votes = torch.zeros((n, 4), dtype=torch.int16, device="cuda")
    recs = torch.zeros(n * 8 + 8, dtype=torch.int64, device="cuda")
    outv = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    prm = scvod.component_visibility_params_default()
    vgood = lambda p=prm: [h, P(comp), n, P(dn), n, P(ver.data_ptr()), P(votes.data_ptr()), C.byref(p), P(recs.data_ptr()), n,  # noqa: E731
                           P(outv.data_ptr()), None]

    def vbad(i, v, p=prm):
        a = vgood(p)
        a[i] = v
        return lib.scvod_map_component_visibility(*a)

    assert vbad(2, -1) == INVALID and vbad(2, 1 << 31) == INVALID and vbad(3, None) == INVALID
    assert vbad(1, None) == INVALID and vbad(5, None) == INVALID
    assert vbad(4, -1) == INVALID and vbad(9, -1) == INVALID
    assert vbad(1, P(comp + 2)) == INVALID and vbad(3, P(dn + 4)) == INVALID and vbad(6, P(votes.data_ptr() + 2)) == INVALID
    assert vbad(8, P(recs.data_ptr() + 4)) == INVALID
    assert vbad(10, P(ver.data_ptr() + 1)) == INVALID                  # overlaps d_verdict without being equal to it
    assert vbad(10, P(votes.data_ptr())) == INVALID and vbad(10, P(recs.data_ptr())) == INVALID and vbad(10, P(comp)) == INVALID
    for kw in (dict(flags=2), dict(min_cells=0), dict(max_cells=-1), dict(min_tested=0), dict(vote_den=0), dict(vote_den=4097),
               dict(vote_num=-1), dict(vote_num=4097)):
        assert vbad(0, h, scvod.component_visibility_params_default(**kw)) == INVALID, kw
    p = scvod.component_visibility_params_default()
    p.reserved = 1
    assert vbad(0, h, p) == INVALID
    assert vbad(6, None, scvod.component_visibility_params_default(flags=scvod.CMPVIS_POOL_PAIRS)) == INVALID
    assert lib.scvod_map_component_visibility_stats(h, o) == -5        # still no call
    assert lib.scvod_map_component_visibility(*vgood()) == 0
    assert vbad(10, P(ver.data_ptr())) == 0                            # in place is fine
    torch.cuda.synchronize()
    m.close()


# ---------------------------------------------------------------- the vote

def _vote_inputs(rng, n):
    ver = rng.integers(0, 256, n).astype(np.uint8)
    pick = rng.random(n) < 0.7
    ver[pick] = rng.integers(0, 3, int(pick.sum())).astype(np.uint8)  # mostly the three verdicts, the rest any byte
    votes = rng.integers(0, 65536, (n, 4)).astype(np.uint16)
    return ver, votes


def _vote(scvod, m, comp, n_comp, ver, votes, prm_kw, cap_components=None, cap=None, in_place=False):
    """scvod_map_component_visibility through the C ABI into guarded outputs"""
    import torch
    n = len(comp)
    cap = n if cap is None else cap
    cap_components = n if cap_components is None else cap_components
    d_comp = torch.from_numpy(np.ascontiguousarray(comp, np.int32)).cuda()
    d_n = torch.tensor([n_comp], dtype=torch.int64, device="cuda")
    ver_all, d_ver = _guarded(torch, n, torch.uint8, SENT8)
    d_ver.copy_(torch.from_numpy(ver))
    d_votes = None if votes is None else torch.from_numpy(votes.view(np.int16)).cuda()
    out_all, d_out = (ver_all, d_ver) if in_place else _guarded(torch, n, torch.uint8, SENT8)
    rec_all = torch.full(((cap + 2 * G) * 64,), SENT8, dtype=torch.uint8, device="cuda")
    prm = scvod.component_visibility_params_default(**prm_kw)
    rc = m.lib.scvod_map_component_visibility(m.h, C.c_void_p(d_comp.data_ptr()), n, C.c_void_p(d_n.data_ptr()), cap_components,
                                              C.c_void_p(d_ver.data_ptr()), None if votes is None else C.c_void_p(d_votes.data_ptr()), C.byref(prm),
                                              C.c_void_p(rec_all.data_ptr() + 64 * G), cap, C.c_void_p(d_out.data_ptr()), None)
    torch.cuda.synchronize()
    ho, hr = out_all.cpu().numpy(), rec_all.cpu().numpy()
    clean = (ho[:G] == SENT8).all() and (ho[G + n:] == SENT8).all() and (hr[:64 * G] == SENT8).all() and (hr[64 * (G + cap):] == SENT8).all()
    if not in_place:
        assert np.array_equal(ver_all.cpu().numpy()[G:G + n], ver)    # the input is only read
    return rc, ho[G:G + n].copy(), hr[64 * G:64 * (G + cap)].copy(), clean


def _check_vote(scvod, m, comp, n_comp, ver, votes, prm_kw, what="", **kw):
    want = mc.vote(comp, n_comp, ver, votes, prm_kw, cap_components=kw.get("cap_components"))
    rc, out, rec, clean = _vote(scvod, m, comp, n_comp, ver, votes, prm_kw, **kw)
    assert rc == 0 and clean, what
    assert np.array_equal(out, want["verdict"]), what
    nr = len(want["records"])
    assert rec[:64 * nr].tobytes() == want["records"].tobytes(), what
    assert (rec[64 * nr:] == SENT8).all(), what
    assert list(m.component_visibility_stats().values()) == want["stats"], what
    return want


@pytest.mark.parametrize("cid,conn", [("random_01", 26), ("random_03", 6), ("block", 26), ("mixed", 18)])
def test_vote_equals_the_helper(scvod, cid, conn):
    case, ref = CASES[cid], _ref(cid, conn)
    rng = np.random.default_rng(41 + conn)
    n = len(case["list"])
    ver, votes = _vote_inputs(rng, n)
    m = _map_of(scvod, case["map"][:16])                              # (the vote reads no cell: any map will do)
    nc = len(ref["table"])
    for prm_kw, v in ((dict(), None), (dict(), votes), (dict(flags=1), votes), (dict(flags=1, vote_num=2049, vote_den=4096, min_through=5), votes),
                      (dict(min_cells=3, vote_num=1, vote_den=3), votes)):
        for in_place in (False, True):
            w = _check_vote(scvod, m, ref["component"], nc, ver, v, prm_kw, what="%s %s in_place=%s" % (cid, prm_kw, in_place), in_place=in_place)
    assert w["stats"][1] > 0
    m.close()


def test_vote_gates_on_both_sides_of_equality(scvod):
    case, ref = CASES["random_01"], _ref("random_01", 26)
    comp, nc = ref["component"], len(ref["table"])
    sizes = ref["table"]["n_records"]
    s = int(np.sort(sizes)[len(sizes) * 3 // 4])                      # a size that some components have, some exceed, some miss
    assert (sizes == s).any() and (sizes > s).any() and (sizes < s).any()
    rng = np.random.default_rng(43)
    ver, votes = _vote_inputs(rng, len(comp))
    m = _map_of(scvod, case["map"][:16])
    hows = {}
    for kw in (dict(max_cells=s), dict(max_cells=s - 1), dict(min_cells=s), dict(min_cells=s + 1)):
        w = _check_vote(scvod, m, comp, nc, ver, votes, kw, what=str(kw))
        hows[tuple(kw.items())] = w["records"]["how"]
    at = sizes == s
    assert hows[(("max_cells", s),)][at].any() and not hows[(("max_cells", s - 1),)][at].any()
    assert hows[(("min_cells", s),)][at].any() and not hows[(("min_cells", s + 1),)][at].any()
    tested = np.array([int(np.isin(ver[comp == c], (1, 2)).sum()) for c in range(nc)])
    t = int(np.sort(tested)[len(tested) // 2]) or 1
    assert (tested == t).any() and (tested == t - 1).any()
    a = _check_vote(scvod, m, comp, nc, ver, votes, dict(min_tested=t))["records"]["how"]
    b = _check_vote(scvod, m, comp, nc, ver, votes, dict(min_tested=t + 1))["records"]["how"]
    assert a[tested == t].all() and not b[tested == t].any() and not a[tested == t - 1].any()
    m.close()


def test_vote_capacities(scvod):
    case, ref = CASES["random_01"], _ref("random_01", 26)
    comp, nc = ref["component"], len(ref["table"])
    rng = np.random.default_rng(44)
    ver, votes = _vote_inputs(rng, len(comp))
    m = _map_of(scvod, case["map"][:16])
    # components at or beyond cap_components keep their bytes
    capc = nc // 2
    w = _check_vote(scvod, m, comp, nc, ver, votes, dict(), cap_components=capc, what="cap_components")
    beyond = comp >= capc
    assert beyond.any() and np.array_equal(w["verdict"][beyond], ver[beyond]) and w["stats"][6] == nc - capc
    # records one short: nothing at or behind cap_records, the overflow latched, the bytes complete
    full = mc.vote(comp, nc, ver, votes, {})
    rc, out, rec, clean = _vote(scvod, m, comp, nc, ver, votes, {}, cap=nc - 1)
    assert rc == 0 and clean and np.array_equal(out, full["verdict"])
    assert rec.tobytes() == full["records"][:nc - 1].tobytes()
    o = (C.c_int64 * 8)()
    assert m.lib.scvod_map_component_visibility_stats(m.h, o) == ERR_CAPACITY
    assert list(o) == full["stats"][:5] + [nc - 1, 0, 1]
    _check_vote(scvod, m, comp, nc, ver, votes, dict(), what="the next call is clean")
    m.close()


def test_pooled_sums_beyond_32_bits_on_the_device(scvod):
    """one component of 40 000 members with counters of 65 535: sum_through = 2 621 400 000 > 2^31"""
    n = 40000
    votes = np.zeros((n, 4), np.uint16)
    votes[:, 0] = 65535
    votes[:, 1] = 65535
    votes[n // 2:, 1] = 65534
    votes[:, 3] = 65535
    comp = np.zeros(n, np.int32)
    ver = np.full(n, mc.KEEP, np.uint8)
    m = _map_of(scvod, CASES["snake"]["map"][:16])
    w = _check_vote(scvod, m, comp, 1, ver, votes, dict(flags=1, vote_num=2048, vote_den=4096))
    assert w["records"]["sum_through"][0] == n * 65535 > 1 << 31 and w["records"]["verdict"][0] == mc.SEEN_THROUGH
    assert (w["verdict"] == mc.SEEN_THROUGH).all()
    m.close()


def test_the_recipe_on_one_stream_without_a_host_read(scvod):
    """cloud_visibility -> components -> component_visibility -> accumulate_labelled on one stream, no synchronisation in between,
    against the same calls with a synchronisation after each"""
    import torch
    P = scvod.make_params("semantickitti")
    rng = np.random.default_rng(51)
    scans = []
    for s in range(3):
        a = rng.uniform(0, 2 * np.pi, 6000)
        wall = np.stack([14.0 * np.cos(a), 14.0 * np.sin(a), rng.uniform(-1.5, 1.0, len(a))], axis=1)
        a = rng.uniform(0, 2 * np.pi, 600)
        r = rng.uniform(5.5, 6.5, len(a))
        thing = np.stack([r * np.cos(a[0] + 0.2 * s) + 0 * a, r * np.sin(a[0] + 0.2 * s) + 0 * a, rng.uniform(-1.2, 0.2, len(a))], axis=1)
        p = np.concatenate([wall, thing])
        scans.append(np.concatenate([p, rng.uniform(0, 100, (len(p), 1))], axis=1).astype(np.float32))
    x = np.concatenate(scans)
    off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    poses = np.zeros((3, 6), np.float32)
    poses[:, 0] = 0.3 * np.arange(3)
    ctx = scvod.Ctx(P, max_points_total=len(x) + 64, max_scans=3)
    d = torch.from_numpy(x).cuda()
    imgs = ctx.visibility_device(d, off, None, None, scvod.visibility_params_default(before=0, after=1), None, want=("images",))["images"]
    raw = scvod.StaticMap(1 << 16, kind=scvod.MAP_KIND_LABELLED)
    raw.accumulate_labelled(d, torch.full((len(x),), 4, dtype=torch.uint8, device="cuda"), off, poses)
    pts, lab, recs = raw.points_labelled(select=[v for v in range(256) if v != 1])
    pts, recs = pts.contiguous(), recs.contiguous()
    keep = [v for v in range(256) if v != scvod.VIS_SEEN_THROUGH]
    torch.cuda.synchronize()
    results = []
    for sync in (False, True):
        st = torch.cuda.Stream()
        clean = scvod.StaticMap(1 << 16, kind=scvod.MAP_KIND_LABELLED)
        wait = torch.cuda.synchronize if sync else (lambda: None)
        with torch.cuda.stream(st):
            out = ctx.cloud_visibility(pts, imgs, poses, stream=st.cuda_stream)
            wait()
            comp = raw.components(recs, stream=st.cuda_stream)
            wait()
            fin = raw.component_visibility(comp, out["verdict"], out["votes"], stream=st.cuda_stream)
            wait()
            clean.accumulate_labelled(pts, fin["verdict"], [0, len(pts)], None, keep=keep, stream=st.cuda_stream)
        torch.cuda.synchronize()
        results.append((out["verdict"].cpu().numpy(), out["votes"].cpu().numpy(), comp["component"].cpu().numpy(), int(comp["n"].cpu()[0]),
                        comp["table"].cpu().numpy(), fin["verdict"].cpu().numpy(), fin["records"].cpu().numpy(), mr.sorted_records(clean)))
        clean.close()
    a, b = results
    nc = a[3]
    assert nc == b[3] and nc > 1
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[4][:nc], b[4][:nc]) and np.array_equal(a[5], b[5]) and np.array_equal(a[6][:nc], b[6][:nc])
    assert np.array_equal(a[7][0], b[7][0]) and np.array_equal(a[7][1], b[7][1])
    # and it is the helper's answer
    lk = recs.cpu().numpy().view(np.uint64)[:, 0]
    ref = mc.components(lk, lk, 26)
    assert np.array_equal(a[2], ref["component"]) and a[4][:nc].tobytes() == ref["table"].tobytes()
    want = mc.vote(a[2], nc, a[0], a[1].view(np.uint16))
    assert np.array_equal(a[5], want["verdict"]) and a[6][:nc].tobytes() == want["records"].tobytes()
    assert 0 < len(a[7][0]) <= len(lk)
    raw.close()
    ctx.close()
