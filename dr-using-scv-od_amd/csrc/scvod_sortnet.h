// Schedule of the pad-free LDS bitonic sorts, as plain host/device C++ (no intrinsics), so that the
// whole network can be replayed thread by thread on the CPU (tests/test_sortnet_host.py).
//
// The network is the all-ascending ("normalised") bitonic sort on np2 = 2^q logical slots: stage
// k = 2^r is a mirror step inside every k-block (i <-> i ^ (k - 1)) followed by the butterfly levels
// with distances k/4 .. 1.  Every comparator puts the minimum at the lower index, so slots that hold
// +inf never move: with n' = n rounded up to a multiple of the run length 2^LGE, the logical slots
// >= n' are +inf for the whole sort and are never read, written or compared.  A patch then costs what
// its keys cost, not what its tier's capacity costs.
//
// Register blocking is that of the padded network: runs of 2^LGE are sorted in registers, and every
// later stage takes its r levels in ceil(r / LGE) passes, a leading partial pass and full LGE-level
// passes.  The mirror level is folded into the stage's first pass: a work item takes the lower half
// of its registers at residue t0 from the lower half of the k-block and the upper half at residue
// jl - 1 - t0 from the upper half of the k-block, a set closed under the mirror and under the
// butterfly levels that follow it in the pass.
#pragma once

#if defined(__HIPCC__)
#define SORTNET_HD __host__ __device__ __forceinline__
#else
#define SORTNET_HD inline
#endif

namespace sortnet {

// padded LDS layout: one spare slot after every 8 elements
SORTNET_HD constexpr int slot(bool pad, int i) { return pad ? i + (i >> 3) : i; }

// n': the live prefix, n rounded up to whole runs (the < 2^LGE filler pads count as keys)
SORTNET_HD constexpr int live_end(int n, int lge) { return ((n + (1 << lge) - 1) >> lge) << lge; }

// levels of the leading pass of a stage with r levels; the passes after it take lge levels each
SORTNET_HD constexpr int first_levels(int r, int lge) { return (r % lge) ? (r % lge) : lge; }

// passes (= barriers) of the merge stages k = 2^(lge+1) .. np2 = 2^lg_np2
SORTNET_HD constexpr int merge_passes(int lg_np2, int lge) {
    int p = 0;
    for (int r = lge + 1; r <= lg_np2; ++r) p += (r + lge - 1) / lge;
    return p;
}

// calls f(r, lt, mirror) for every pass of the merge stages, in order: the pass does the levels with
// distances 2^(r-1) .. 2^(r-lt); mirror = the first of them is the mirror step of the 2^r-blocks
template <int LGE, typename F>
SORTNET_HD void for_each_pass(int np2, F f) {
    int lgk = LGE + 1;
    for (int k = 2 << LGE; k <= np2; k <<= 1, ++lgk) {
        int r = lgk;
        const int first = first_levels(r, LGE);
        f(r, first, true);
        r -= first;
        while (r > 0) {
            f(r, LGE, false);
            r -= LGE;
        }
    }
}

// work items t of a pass are the np2 >> lt groups of 2^lt elements; items [0, pass_items) are those
// whose 2^r-block starts below nlive, all later ones hold nothing live
SORTNET_HD constexpr int pass_items(int np2, int nlive, int r, int lt) {
    const int all = np2 >> lt;
    const int some = ((nlive + (1 << r) - 1) >> r) << (r - lt);
    return some < all ? some : all;
}

// lowest logical index of item t: bits [r-lt, r) are zero
SORTNET_HD constexpr int item_base(int t, int r, int lt) {
    return ((t >> (r - lt)) << r) | (t & ((1 << (r - lt)) - 1));
}

// logical index held in register m of the item with base b; monotone in m
SORTNET_HD constexpr int item_elem(int b, int m, int r, int lt, bool mirror) {
    const int jl = 1 << (r - lt);
    return ((mirror && m >= (1 << lt) / 2) ? (b ^ (jl - 1)) : b) + m * jl;
}

// the compare-exchanges of a pass on the registers of one item; cx(lo, hi) leaves min in lo
template <int LT, bool MIRROR, typename T, typename CX>
SORTNET_HD void pass_network(T (&e)[1 << LT], CX cx) {
    constexpr int E = 1 << LT;
    if (MIRROR) {
#pragma unroll
        for (int m = 0; m < E / 2; ++m) cx(e[m], e[E - 1 - m]);
    }
#pragma unroll
    for (int d = MIRROR ? E / 4 : E / 2; d >= 1; d >>= 1) {
#pragma unroll
        for (int m = 0; m < E; ++m)
            if ((m & d) == 0) cx(e[m], e[m + d]);
    }
}

// stages k = 2 .. 2^LGE on a run held in registers: ascending sort of the run
template <int LGE, typename T, typename CX>
SORTNET_HD void run_network(T (&e)[1 << LGE], CX cx) {
    constexpr int E = 1 << LGE;
#pragma unroll
    for (int kk = 2; kk <= E; kk <<= 1) {
#pragma unroll
        for (int d = kk >> 1; d >= 1; d >>= 1) {
#pragma unroll
            for (int m = 0; m < E; ++m)
                if ((m & d) == 0) {
                    if (kk == E || (m & kk) == 0)
                        cx(e[m], e[m + d]);
                    else
                        cx(e[m + d], e[m]);
                }
        }
    }
}

// one work item of a pass on the array a (LDS on the device; anything with operator[] on the host).
// Registers of logical slots >= nlive hold padv (>= every key) and are neither loaded nor stored; a
// comparator never moves them because they sit at the upper index of every pair they are in.
template <int LT, bool MIRROR, bool PAD, typename T, typename Arr, typename CX>
SORTNET_HD void pass_item(Arr a, int t, int r, int nlive, T padv, CX cx) {
    constexpr int E = 1 << LT;
    const int b = item_base(t, r, LT);
    if (b >= nlive) return;
    T e[E];
    if (item_elem(b, E - 1, r, LT, MIRROR) < nlive) {  // wholly live: no predicates
#pragma unroll
        for (int m = 0; m < E; ++m) e[m] = a[slot(PAD, item_elem(b, m, r, LT, MIRROR))];
        pass_network<LT, MIRROR>(e, cx);
#pragma unroll
        for (int m = 0; m < E; ++m) a[slot(PAD, item_elem(b, m, r, LT, MIRROR))] = e[m];
    } else {
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int i = item_elem(b, m, r, LT, MIRROR);
            e[m] = padv;
            if (i < nlive) e[m] = a[slot(PAD, i)];
        }
        pass_network<LT, MIRROR>(e, cx);
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int i = item_elem(b, m, r, LT, MIRROR);
            if (i < nlive) a[slot(PAD, i)] = e[m];
        }
    }
}

// run g (logical slots [g << LGE, (g + 1) << LGE), all live) sorted in registers and stored
template <int LGE, bool PAD, typename T, typename Arr, typename CX>
SORTNET_HD void run_store(T (&e)[1 << LGE], Arr a, int g, CX cx) {
    run_network<LGE>(e, cx);
#pragma unroll
    for (int m = 0; m < (1 << LGE); ++m) a[slot(PAD, (g << LGE) + m)] = e[m];
}

// register start: the it-th load of active thread t (of T' = nlive >> LGE) is key it * T' + t
SORTNET_HD constexpr int start_key(int it, int t, int nlive, int lge) { return it * (nlive >> lge) + t; }

}  // namespace sortnet
