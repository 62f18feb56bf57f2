"""The crafted lists of the component tests.  A case is a dict: id, list (uint64 keys in list order: padding, absent keys and duplicates
where the case is about them), map (the distinct keys the map holds) and, where it was worked out by hand, count: {connectivity:
components}."""
import numpy as np

import map_ref as mr

TOP = (1 << 20) - 1      # the last cell of an axis
LOW = -(1 << 20)         # the first


def _keys(cells):
    c = np.asarray(cells, np.int64).reshape(-1, 3)
    return mr.pack_key(c[:, 0], c[:, 1], c[:, 2])


def _case(cid, cells, count=None, rng=None, list_keys=None):
    k = _keys(cells)
    assert len(np.unique(k)) == len(k), cid
    lk = k if list_keys is None else np.asarray(list_keys, np.uint64)
    if rng is not None:
        lk = lk[rng.permutation(len(lk))]
    return {"id": cid, "list": lk, "map": k, "count": count}


def hand_worked():
    """pairs, the border cell, a field carry, a checkerboard, a duplicate, padding, an absent key"""
    out = []
    for name, d, cnt in (("face", (1, 0, 0), {6: 1, 18: 1, 26: 1}), ("face_z", (0, 0, -1), {6: 1, 18: 1, 26: 1}),
                         ("edge", (1, -1, 0), {6: 2, 18: 1, 26: 1}), ("edge_yz", (0, 1, 1), {6: 2, 18: 1, 26: 1}),
                         ("corner", (1, 1, 1), {6: 2, 18: 2, 26: 1}), ("corner_mixed", (-1, 1, -1), {6: 2, 18: 2, 26: 1}),
                         ("apart", (2, 0, 0), {6: 2, 18: 2, 26: 2})):
        out.append(_case("pair_" + name, [(5, -7, 3), (5 + d[0], -7 + d[1], 3 + d[2])], cnt))
    # the last cell of z: it has no +z neighbour.  (0, 1, LOW) is the cell whose key is key(0, 0, TOP) + 1: a carry would join them
    out.append(_case("border_top_z", [(0, 0, TOP), (0, 1, LOW)], {6: 2, 18: 2, 26: 2}))
    out.append(_case("border_top_y", [(3, TOP, 7), (4, LOW, 7)], {6: 2, 18: 2, 26: 2}))
    out.append(_case("border_low_z", [(0, 1, LOW), (0, 0, TOP), (0, 1, LOW + 1)], {6: 2, 18: 2, 26: 2}))
    out.append(_case("border_corner", [(TOP, TOP, TOP), (TOP - 1, TOP - 1, TOP - 1), (LOW, LOW, LOW), (LOW + 1, LOW, LOW)], {6: 3, 18: 3, 26: 2}))
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), axis=-1).reshape(-1, 3)
    board = g[g.sum(axis=1) % 2 == 0] + np.array([-3, 10, -2])
    out.append(_case("checkerboard", board, {6: len(board), 18: 1, 26: 1}, rng=np.random.default_rng(1)))
    three = _keys([(1, 1, 1), (2, 1, 1), (9, 9, 9)])
    out.append(_case("duplicate", [(1, 1, 1), (2, 1, 1), (9, 9, 9)], {6: 2, 18: 2, 26: 2}, list_keys=three[[2, 0, 1, 0, 2, 2]]))
    pad = np.uint64(mr.PAD)
    out.append(_case("padding", [(1, 1, 1), (2, 1, 1), (9, 9, 9)], {6: 2, 18: 2, 26: 2}, list_keys=np.array([pad, three[1], pad, three[0], three[2], pad])))
    # (2, 1, 1) is in the map but not in the list: no node, so it joins nothing; (3, 1, 1) is not in the map at all
    lk = np.array([three[0], _keys([(3, 1, 1)])[0], three[2]], np.uint64)
    c = _case("absent", [(1, 1, 1), (2, 1, 1), (9, 9, 9), (4, 1, 1)], {6: 2, 18: 2, 26: 2}, list_keys=lk)
    out.append(c)
    # a bridge the list leaves out: (1,1,1) - [(2,1,1)] - (3,1,1)
    lk = _keys([(1, 1, 1), (3, 1, 1)])
    out.append(_case("bridge_left_out", [(1, 1, 1), (2, 1, 1), (3, 1, 1)], {6: 2, 18: 2, 26: 2}, list_keys=lk))
    return out


def snake(n=5000, row=50, seed=2):
    """one face-connected path: rows of `row` cells along x at every other y, joined at alternating ends; random list order"""
    cells, y = [], 0
    while len(cells) < n:
        xs = range(row) if (y // 2) % 2 == 0 else range(row - 1, -1, -1)
        cells += [(x, y, 4) for x in xs]
        cells.append((cells[-1][0], y + 1, 4))
        y += 2
    return _case("snake", cells[:n], {6: 1, 18: 1, 26: 1}, rng=np.random.default_rng(seed))


def u_shape(arm=700):
    """two arms three cells apart that meet only at the far end, listed from the open ends inwards"""
    a = [(x, 0, 0) for x in range(arm)]
    b = [(x, 3, 0) for x in range(arm)]
    cells = [c for pair in zip(a, b) for c in pair] + [(arm - 1, 1, 0), (arm - 1, 2, 0)]
    return _case("u_shape", cells, {6: 1, 18: 1, 26: 1})


def block(side=40):
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 3) - side // 2
    return _case("block", g, {6: 1, 18: 1, 26: 1}, rng=np.random.default_rng(3))


def random_box(fill, n=20000, side=30, seed=4):
    """cells of a side^3 box at the given fill, topped up to n cells with copies of the box far away"""
    rng = np.random.default_rng(seed + int(fill * 10))
    cells = []
    shift = 0
    while len(cells) < n:
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 3)
        g = g[rng.random(len(g)) < fill] + np.array([shift, -500, 77])
        cells += g.tolist()
        shift += side + 5
    return _case("random_%02d" % int(fill * 10), cells[:n], None, rng=rng)


def axis_chain(axis):
    """a chain along one axis through cell 0 and up to both borders of the range, the other two coordinates at borders of their own"""
    other = {0: (TOP, LOW), 1: (LOW, TOP), 2: (TOP, TOP)}[axis]
    cells = []
    for v in list(range(-40, 41)) + list(range(LOW, LOW + 30)) + list(range(TOP - 29, TOP + 1)):
        c = list(other)
        c.insert(axis, v)
        cells.append(tuple(c))
    return _case("chain_axis%d" % axis, cells, {6: 3, 18: 3, 26: 3}, rng=np.random.default_rng(5 + axis))


def mixed(seed=6):
    """a list with absent keys, padding and duplicates mixed into random cells"""
    rng = np.random.default_rng(seed)
    base = random_box(0.3, n=3000, side=16, seed=seed)
    k = base["map"]
    held = k[: len(k) * 4 // 5]                            # the map holds four fifths ...
    lk = np.concatenate([k, k[rng.integers(0, len(k), 900)], np.full(300, mr.PAD, np.uint64), mr.random_keys(rng, 200)])
    return {"id": "mixed", "list": lk[rng.permutation(len(lk))], "map": held, "count": None}


def gpu_cases():
    return hand_worked() + [snake(), u_shape(), block(), random_box(0.1), random_box(0.3), axis_chain(0), axis_chain(1), axis_chain(2), mixed()]
