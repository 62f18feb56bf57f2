"""scvod_map_components / scvod_map_component_visibility without a GPU: the symbols, struct sizes and defaults, every refusal that is
made before a device is looked for, and the plain statement (tests/helpers/map_components_ref.py) on cases worked out by hand -- what
makes the device's byte-for-byte comparison against it in tests/test_gpu_map_components.py meaningful.  A map cannot exist without a
device, so here the refusals are those of a NULL map; the same calls with bad arguments on a live map are in the gpu file.  Not gpu."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import map_components_cases as mk  # noqa: E402
import map_components_ref as mc  # noqa: E402
import map_ref as mr  # noqa: E402

NEW = ("scvod_map_components", "scvod_map_components_stats", "scvod_map_components_scratch_bytes", "scvod_map_component_visibility",
       "scvod_map_component_visibility_stats", "scvod_component_visibility_params_default")
INVALID = -1


def test_symbols_declared_exported_and_listed(scvod):
    lib = scvod.load_lib()
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    declared = set(re.findall(r"\b(scvod_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/scvod.h"
        assert hasattr(lib, name), f"{name} is not exported by libscvod.so"
        assert name in scvod.EXPORTED_SYMBOLS
    for m in ("components", "components_stats", "components_scratch_bytes", "component_visibility", "component_visibility_stats"):
        assert callable(getattr(scvod.StaticMap, m))
    assert re.search(r"#define\s+SCVOD_CMPVIS_POOL_PAIRS\s+1\b", hdr) and scvod.CMPVIS_POOL_PAIRS == 1 == mc.POOL_PAIRS
    assert len(scvod.MAP_COMPONENTS_STATS) == 8 and len(scvod.CMPVIS_STATS) == 8
    assert "scvod_mapcomp" in open(os.path.join(ROOT, "dr-using-scv-od_amd", "csrc", "Makefile")).read()
    # the header says whose rule this is
    sec = hdr[hdr.index("connected components of the map's cells"):]
    assert "NOT from real data" in sec and "Reference analogue: none" in sec


def test_struct_sizes_and_defaults(scvod):
    assert C.sizeof(scvod.ComponentVisibilityParams) == 32
    assert scvod.MAP_COMPONENT_DTYPE.itemsize == 48 and scvod.COMPONENT_VISIBILITY_DTYPE.itemsize == 64
    assert scvod.MAP_COMPONENT_DTYPE == mc.COMPONENT_DTYPE and scvod.COMPONENT_VISIBILITY_DTYPE == mc.VISIBILITY_DTYPE
    hdr = open(os.path.join(ROOT, "include", "scvod.h")).read()
    assert re.search(r"typedef struct scvod_map_component \{ /\* 48 bytes", hdr)
    assert re.search(r"typedef struct scvod_component_visibility \{ /\* 64 bytes", hdr)
    assert re.search(r"typedef struct scvod_component_visibility_params \{ /\* 32 bytes", hdr)
    p = scvod.component_visibility_params_default()
    got = [getattr(p, f[0]) for f in scvod.ComponentVisibilityParams._fields_]
    assert got == [0, 1, 0, 1, 2, 1, 2, 0]
    assert [mc.DEFAULTS[k] for k in ("flags", "min_cells", "max_cells", "min_tested", "min_through", "vote_num", "vote_den")] == got[:7]
    scvod.load_lib().scvod_component_visibility_params_default(None)       # NULL: nothing happens
    assert scvod.component_visibility_params_default(max_cells=4096, flags=1).max_cells == 4096


def test_a_null_map_is_invalid(scvod):
    lib = scvod.load_lib()
    buf = np.zeros(256, np.int64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.scvod_map_components(None, p, 4, 26, p, p, 4, p, None) == INVALID
    assert lib.scvod_map_components(None, None, 0, 26, None, None, 0, None, None) == INVALID
    assert lib.scvod_map_components_stats(None, p) == INVALID
    assert lib.scvod_map_components_scratch_bytes(None) == 0
    assert lib.scvod_map_component_visibility(None, p, 4, p, 4, p, None, None, None, 0, p, None) == INVALID
    assert lib.scvod_map_component_visibility_stats(None, p) == INVALID
    assert not buf.any()


# ---- the statement on cases worked out by hand

@pytest.mark.parametrize("case", mk.hand_worked() + [mk.snake(), mk.u_shape(), mk.axis_chain(0), mk.axis_chain(1), mk.axis_chain(2)],
                         ids=lambda c: c["id"])
def test_helper_counts_components_as_worked_out_by_hand(case):
    for conn in (6, 18, 26):
        r = mc.components(case["list"], case["map"], conn)
        assert r["stats"][5] == len(r["table"]) == case["count"][conn], (case["id"], conn)
        assert int(r["table"]["n_records"].sum()) == r["stats"][1] == int((r["component"] >= 0).sum())
        assert (np.diff(r["table"]["key"].astype(np.uint64)) > 0).all()                    # ascending by smallest key


def test_helper_pairs_in_detail():
    a, b = (5, -7, 3), (6, -8, 3)
    k = mr.pack_key([a[0], b[0]], [a[1], b[1]], [a[2], b[2]])
    r = mc.components(k, k, 6)
    assert r["component"].tolist() == [0, 1] and r["table"]["first_record"].tolist() == [0, 1]
    r = mc.components(k[::-1], k, 6)                                   # numbering follows the key, not the list
    assert r["component"].tolist() == [1, 0] and r["table"]["first_record"].tolist() == [1, 0]
    r = mc.components(k, k, 18)
    t = r["table"][0]
    assert r["component"].tolist() == [0, 0] and int(t["key"]) == int(k.min()) and t["n_records"] == 2
    assert t["cell_min"].tolist() == [5, -8, 3] and t["cell_max"].tolist() == [6, -7, 3] and t["reserved"].tolist() == [0, 0]


def test_helper_border_cell_has_no_neighbour_across_a_field():
    top = (1 << 20) - 1
    a, b = int(mr.pack_key(0, 0, top)), int(mr.pack_key(0, 1, -(1 << 20)))
    assert b == a + 1                                                   # what a carry out of the z field would reach
    for conn in (6, 18, 26):
        r = mc.components([a, b], [a, b], conn)
        assert r["component"].tolist() == [0, 1]
    assert mc.cell_of(a) == (0, 0, top) and mc.key_of(*mc.cell_of(b)) == b


def test_helper_duplicates_padding_and_absent_keys():
    cases = {c["id"]: c for c in mk.hand_worked()}
    r = mc.components(cases["duplicate"]["list"], cases["duplicate"]["map"], 26)
    # list = [c, a, b, a, c, c] with a - b joined: {a, b} has the smaller key
    assert r["component"].tolist() == [1, 0, 0, 0, 1, 1] and r["stats"] == [6, 6, 0, 0, 3, 2, 2, 0]
    assert r["table"]["n_records"].tolist() == [3, 3] and r["table"]["first_record"].tolist() == [1, 0]
    r = mc.components(cases["padding"]["list"], cases["padding"]["map"], 26)
    assert r["component"].tolist() == [-1, 0, -1, 0, 1, -1] and r["stats"] == [6, 3, 3, 0, 0, 2, 2, 0]
    r = mc.components(cases["absent"]["list"], cases["absent"]["map"], 26)
    assert r["component"].tolist() == [0, -1, 1] and r["stats"] == [3, 2, 0, 1, 0, 2, 2, 0]
    r = mc.components(cases["bridge_left_out"]["list"], cases["bridge_left_out"]["map"], 26)
    assert r["component"].tolist() == [0, 1]                           # the cell between them is in the map, not in the list


def test_helper_vote_at_equality_of_every_threshold():
    K, S, U = mc.KEEP, mc.SEEN_THROUGH, mc.UNTESTED
    d = mc.decide
    # min_cells / max_cells / min_tested: equality votes, one short does not
    assert d(5, 2, 3, 0, 0, dict(min_cells=5)) == (S, 1) and d(4, 2, 2, 0, 0, dict(min_cells=5)) == (-1, 0)
    assert d(5, 2, 3, 0, 0, dict(max_cells=5)) == (S, 1) and d(6, 3, 3, 0, 0, dict(max_cells=5)) == (-1, 0)
    assert d(6, 3, 3, 0, 0, dict(max_cells=0)) == (S, 1)
    assert d(9, 1, 2, 0, 0, dict(min_tested=3)) == (S, 1) and d(9, 1, 1, 0, 0, dict(min_tested=3)) == (-1, 0)
    # min_through: t == min_through passes, one below keeps
    assert d(9, 0, 2, 0, 0, {}) == (S, 1) and d(9, 0, 1, 0, 0, {}) == (K, 1)
    # the ratio: t * den >= num * (t + a) at equality, and one member short of it
    assert d(6, 3, 3, 0, 0, {}) == (S, 1) and d(7, 4, 3, 0, 0, {}) == (K, 1)
    assert d(10, 3, 7, 0, 0, dict(vote_num=7, vote_den=10)) == (S, 1) and d(10, 4, 6, 0, 0, dict(vote_num=7, vote_den=10)) == (K, 1)
    assert d(3, 3, 0, 0, 0, dict(vote_num=0, min_through=0)) == (S, 1)            # 0 >= 0 on both tests
    # pooled pairs read the sums, the gates still read the bytes
    pool = dict(flags=mc.POOL_PAIRS)
    assert d(4, 4, 0, 50, 50, pool) == (S, 1) and d(4, 4, 0, 49, 50, pool) == (K, 1) and d(4, 0, 0, 50, 0, pool) == (-1, 0)
    # the members: everyone of a component that voted moves, UNTESTED included; a component that did not vote keeps its bytes
    comp = [0, 0, 0, 1, 1, -1, 2]
    ver = [S, S, U, K, 7, S, U]
    r = mc.vote(comp, 3, ver)
    assert r["verdict"].tolist() == [S, S, S, K, K, S, U]
    assert r["records"]["verdict"].tolist() == [S, K, -1] and r["records"]["how"].tolist() == [1, 1, 0]
    assert r["records"]["n_untested"].tolist() == [1, 1, 1]
    assert r["stats"] == [3, 2, 1, 1, 1, 3, 0, 0]
    r = mc.vote(comp, 3, ver, cap_components=1)                        # components 1 and 2 are beyond the cap: their bytes stay
    assert r["verdict"].tolist() == [S, S, S, K, 7, S, U] and r["stats"] == [3, 1, 1, 1, 0, 1, 2, 0]


def test_helper_sums_and_products_beyond_32_bits():
    """40 000 members with counters of 65 535: the pooled sums pass 2^31, and t * vote_den passes 2^32 -- a 32-bit sum or product gives
    the other verdict"""
    n = 40000
    votes = np.zeros((n, 4), np.uint16)
    votes[:, 0] = 65535                                                # through
    votes[:, 1] = 65535                                                # agree
    votes[n // 2:, 1] = 65534                                          # ... a little less: through > agree in the true sums
    comp = np.zeros(n, np.int32)
    ver = np.full(n, mc.KEEP, np.uint8)
    p = dict(flags=mc.POOL_PAIRS, vote_num=2048, vote_den=4096)
    r = mc.vote(comp, 1, ver, votes, p)
    t, a = int(r["records"]["sum_through"][0]), int(r["records"]["sum_agree"][0])
    assert t == n * 65535 > 1 << 31 and a == t - n // 2
    assert t * 4096 > 1 << 32 and r["records"]["verdict"][0] == mc.SEEN_THROUGH
    # sums truncated to int32 turn negative: t >= min_through fails and the verdict would be KEEP
    as_i32 = lambda v: (v & 0xFFFFFFFF) - (1 << 32) if (v & 0xFFFFFFFF) >> 31 else (v & 0xFFFFFFFF)   # noqa: E731
    assert mc.decide(n, n, 0, as_i32(t), as_i32(a), p) != mc.decide(n, n, 0, t, a, p)
    # a product beyond 2^32 with sums that fit 32 bits: t * 4096 lies just below 3 * 2^32, 4095 * (t + a) just above it
    tt, aa = 3145727, 770
    q = dict(flags=mc.POOL_PAIRS, vote_num=4095, vote_den=4096)
    assert tt * 4096 == 3 * (1 << 32) - 4096 and 4095 * (tt + aa) == 3 * (1 << 32) + 3327
    assert mc.decide(5, 5, 0, tt, aa, q)[0] == mc.KEEP
    assert ((tt * 4096) & 0xFFFFFFFF) >= ((4095 * (tt + aa)) & 0xFFFFFFFF)                   # the truncated products say SEEN_THROUGH
