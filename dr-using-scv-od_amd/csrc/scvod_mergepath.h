// Schedule of the merge-path levels of the large Patchwork sort tiers, as plain host/device C++ (no
// intrinsics), so that every level can be replayed thread by thread on the CPU
// (tests/test_mergepath_host.py).  Companion of scvod_sortnet.h: same LDS layout (sortnet::slot), same
// live prefix n' (sortnet::live_end), same runs of E = 2^LGE keys sorted in registers.
//
// One level merges the sorted runs of length L pairwise into runs of 2L over the live prefix n'.  The
// pads (the largest key) lie at the end of the last run, so they sort to the end and nothing at or
// beyond n' is ever read, written or compared.  Thread t owns the output positions [E t, E t + E):
//   - its pair of runs is the one that holds position E t; a last run without a partner is left in place;
//   - its split is a binary search on the diagonal d = E t - (start of the pair): i keys of the window's
//     predecessors come from the lower run and d - i from the upper one (merge path; equal keys go to the
//     lower run first, so the splits of neighbouring threads agree);
//   - it then merges E keys serially into registers.  The heads of both runs stay in registers, a step
//     costs one comparison and one new read;
//   - the level is in place: all threads read, barrier, all threads store their E outputs, barrier.
// n' is a multiple of E and so is every run start, so a window never straddles two pairs and is
// either whole or absent.
#pragma once

#include "scvod_sortnet.h"

namespace mergepath {

// the pair of runs that holds output position p at run length L, cut at the live prefix
struct Pair {
    int a0, a1;  // lower run: logical slots [a0, a1)
    int b0, b1;  // upper run: [b0, b1); b0 == b1: the lower run has no partner
    int d;       // diagonal: p - a0
};
SORTNET_HD constexpr int imin(int x, int y) { return x < y ? x : y; }
SORTNET_HD constexpr int imax(int x, int y) { return x > y ? x : y; }

SORTNET_HD constexpr Pair pair_of(int p, int L, int nlive) {
    const int a0 = p & ~(2 * L - 1);
    const int b0 = imin(a0 + L, nlive);
    return Pair{a0, b0, b0, imin(a0 + 2 * L, nlive), p - a0};
}

// levels of a sort that starts from runs of length run0: L = run0, 2 run0, ... while L < nlive
SORTNET_HD constexpr int levels(int run0, int nlive) {
    int c = 0;
    for (int L = run0; L < nlive; L <<= 1) ++c;
    return c;
}

// merge-path split on diagonal q.d: the number of keys the first q.d outputs of the pair take from the lower run
template <bool PAD, typename T, typename Arr>
SORTNET_HD int split(Arr a, const Pair& q) {
    int lo = imax(0, q.d - (q.b1 - q.b0)), hi = imin(q.d, q.a1 - q.a0);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const T ka = a[sortnet::slot(PAD, q.a0 + mid)];
        const T kb = a[sortnet::slot(PAD, q.b0 + q.d - 1 - mid)];
        if (kb < ka)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// the E outputs of thread t at run length L, merged into out[]; false: the thread has nothing to do at this
// level (its window is at or beyond nlive, or in a run without a partner).  sent is larger than every key and
// every pad: it stands for the head of a run that is used up.  *ia: the thread's split (slots of the lower run
// before its window), for the replay.
template <int LGE, bool PAD, typename T, typename Arr>
SORTNET_HD bool merge_window(Arr a, int t, int L, int nlive, T (&out)[1 << LGE], T sent, int* ia = nullptr) {
    constexpr int E = 1 << LGE;
    const int p = t << LGE;
    if (p >= nlive) return false;
    const Pair q = pair_of(p, L, nlive);
    if (q.b0 == q.b1) return false;
    const int i = split<PAD, T>(a, q);
    if (ia) *ia = i;
    int xa = q.a0 + i, xb = q.b0 + (q.d - i);  // next unread slot of either run
    T ha = sent, hb = sent;
    if (xa < q.a1) ha = a[sortnet::slot(PAD, xa)];
    if (xb < q.b1) hb = a[sortnet::slot(PAD, xb)];
#pragma unroll
    for (int s = 0; s < E; ++s) {
        const bool take_a = !(hb < ha);
        out[s] = take_a ? ha : hb;
        if (s + 1 < E) {
            if (take_a) ++xa; else ++xb;
            const int x = take_a ? xa : xb;
            T v = sent;
            if (x < (take_a ? q.a1 : q.b1)) v = a[sortnet::slot(PAD, x)];
            if (take_a) ha = v; else hb = v;
        }
    }
    return true;
}

// after the barrier: the window's outputs to logical slots [E t, E t + E)
template <int LGE, bool PAD, typename T, typename Arr>
SORTNET_HD void store_window(Arr a, int t, const T (&out)[1 << LGE]) {
#pragma unroll
    for (int m = 0; m < (1 << LGE); ++m) a[sortnet::slot(PAD, (t << LGE) + m)] = out[m];
}

}  // namespace mergepath
