"""Finds the `radius sliver' pairs of tests/helpers/nn_search_cases.py: a query q and a map point p on one axis whose fp32 squared distance
is below fl(r * r) while the fp32 cell rule of csrc/scvod_grid.h puts them TWO cells apart when the cell edge is the radius itself.

The model is the grid's arithmetic restated in numpy float32 (unfused, as the library is built with -ffp-contract=off):
    cell(x) = floor(fl(fl(x - origin) * fl(1 / cell)))          d^2 = fl(fl(p - q) * fl(p - q))   (the other two axes are equal)
Such a pair needs the query a hair above a cell face (its product rounds up onto the face) and the map point a hair below the face one cell
down (its product rounds down), so the search walks the fp32 values around every face instead of sampling at random.

    python tests/devtools/nn_sliver_model.py            # prints the literals (value, bit pattern) that the helper commits
Not part of the suite; nothing here touches a GPU.
"""
import sys

import numpy as np

F = np.float32
ORIGIN = F(-37.123)          # the map's min corner on every axis (an anchor point of the case sits there)
SPAN = 6                     # fp32 neighbours walked on either side of a face


def cell_of(x, origin, cell):
    inv = F(1) / F(cell)
    return np.floor((np.asarray(x, F) - F(origin)) * inv)


def sqdist_1d(p, q):
    d = np.asarray(p, F) - np.asarray(q, F)
    return d * d


def _around(x, span):
    out = [F(x)]
    lo = hi = F(x)
    for _ in range(span):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return np.sort(np.asarray(out, F))


def sliver_pairs(radius, origin=ORIGIN, faces=range(200, 700), span=SPAN):
    """[(q, p)] with cell(q) - cell(p) == 2, fl(d^2) < fl(r * r) and p < q, for the cell edge == radius"""
    r = F(radius)
    r2 = r * r
    found = []
    for n in faces:
        face = F(np.float64(origin) + n * np.float64(r))
        q = _around(face, span)
        for qv in q:
            p = _around(qv - r, span)
            ok = (cell_of(qv, origin, r) - cell_of(p, origin, r) == 2) & (sqdist_1d(p, qv) < r2)
            found += [(qv, pv) for pv in p[ok]]
    return found


def nearer_variant(q, p, radius):
    """a: the offset on another axis of a second map point A = q + (0, a, 0) with d^2(p) < d^2(A) < fl(r * r): A is the candidate inside the
    27 cells, p the nearer point two cells away.  The query's other coordinates are 0, so a is A's coordinate itself.  None if the window
    between the two squared distances holds no fp32 value"""
    r = F(radius)
    r2, dp = r * r, sqdist_1d(p, q)
    a = r
    for _ in range(64):
        a = np.nextafter(a, F(0))
        if a * a < r2:
            return a if a * a > dp else None
    return None


def offsets_for(target):
    """(s, t) with fl(fl(s * s) + fl(t * t)) bit-equal to `target`: a map point at query + (s, t, 0) has exactly that fp32 d^2.  t is about
    a tenth of the distance, so one fp32 step of t moves t * t by far less than an ulp of the target and the walk cannot step over it"""
    T = F(target)
    t = F(0.1) * np.sqrt(T)
    s = np.sqrt(T - t * t)
    for _ in range(100000):
        d = s * s + t * t
        if d == T:
            return s, t
        t = np.nextafter(t, F(np.inf) if d < T else F(0))
    raise RuntimeError(f"no offsets for {T!r}")


def thresholds():
    """name -> fp32 value: fl(r * r) of the radius edge, and launch_nn's acceptance bound (0.99f * cell) * (0.99f * cell)"""
    out = {}
    for r in (0.25, 0.15):
        out[f"r2 of radius {r}"] = F(r) * F(r)
    for cell in (0.2, 0.3):
        out[f"h2 of cell {cell}"] = (F(0.99) * F(cell)) * (F(0.99) * F(cell))
    return out


def main():
    for name, T in thresholds().items():
        print(f"{name}: {T!r} ({T.view(np.uint32):#010x})")
        for what, v in (("below", np.nextafter(T, F(0))), ("equal", T), ("above", np.nextafter(T, F(np.inf)))):
            s, t = offsets_for(v)
            print(f"    {what!r}: ({v.view(np.uint32):#010x}, {s.view(np.uint32):#010x}, {t.view(np.uint32):#010x}),   # d2 {v!r} s {s!r} t {t!r}")
    for radius in (0.2, 0.3, 0.35, 1.0):
        pairs = sliver_pairs(radius)
        print(f"radius {radius}: {len(pairs)} pairs, origin {ORIGIN!r} ({ORIGIN.view(np.uint32):#010x})")
        if "--all" not in sys.argv:          # per cell face the pair with the smallest d^2 (the helper's literals are some of these)
            best = {}
            for q, p in pairs:
                face = int(cell_of(q, ORIGIN, F(radius)))
                if face not in best or sqdist_1d(p, q) < sqdist_1d(best[face][1], best[face][0]):
                    best[face] = (q, p)
            pairs = [best[k] for k in sorted(best)]
        for q, p in pairs:
            a = nearer_variant(q, p, radius)
            sep = (np.float64(q) - np.float64(p)) / np.float64(F(radius))
            print(f"    ({q.view(np.uint32):#010x}, {p.view(np.uint32):#010x}),   # q {q!r} p {p!r} sep/r {sep:.8f} d2 {sqdist_1d(p, q)!r}"
                  + (f" A {a.view(np.uint32):#010x}" if a is not None else " (no A)"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
