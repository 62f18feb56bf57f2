// scvod_k_cluster.inc -- curved-voxel clustering, boxes, type rules, successor tables (SURVEY 8(f)-1/2): k_cc_scan.
// Part of the kernels translation unit: included by scvod_kernels.hip (inside namespace scvod), never compiled on its own.
// ------------------------------------------------------------------------------------------
// Curved-voxel clustering (SSC::clusterAndCreateFrame, src/ssc.cpp:299-352; SURVEY 8(f)-1).
// The reference walks the points in order; point i looks its index triple's 3x3x3 neighbourhood up in hash_cloud
// (findVoxelNeighbors, ssc.cpp:395-411: clipped to the grid, no sector wrap-around) and is merged with EVERY point of the
// occupied voxels it finds (ssc.cpp:316-345); a point that finds nothing opens a cluster of its own (ssc.cpp:347-353).
// The resulting partition does not depend on the order: it is the set of connected components of that relation.
//
// One workgroup per scan, the whole union-find in LDS.  Nodes are VOXELS, not points: a voxel that appears in anybody's
// neighbourhood ("touched") has all its points merged, so it is one node, named after its first point; the points of a
// voxel are walked as RUNS of equal index triples (a run's points share one neighbourhood) and a run that does not start
// its voxel -- only possible when different triples alias onto one voxel_idx, i.e. next to the -1 bins -- is an extra
// node.  Per scan: ~10 k voxels x 9 binary searches (the three sector neighbours of one (range, azimuth) pair are
// adjacent keys) + lock-free unions, all on a 64 KB key table and a 64 KB parent array in LDS; the canonical cluster name
// is the smallest apri index of the component.  Scans with more than kCcNodes voxels or kCcSlots points (128-beam scans on a
// fine grid) run the generic variant: nodes (keys, parents, bits) on arena scratch in HBM; its search still runs in LDS, one
// window of whole z-planes of the node list at a time (cc_search_windows), the few out-of-grid points of such a scan are
// listed by the regularity pass so that run detection and the regular bits look at their voxels only.
// ------------------------------------------------------------------------------------------
constexpr int kCcNodes = 14336;  // voxels + extra run openers per scan held in LDS
constexpr int kCcSlots = 65536;  // apri points per scan whose run / voxel start bits are held in LDS
#ifndef SCVOD_CC_THREADS
#define SCVOD_CC_THREADS 1024
#endif
constexpr int kCcThreads = SCVOD_CC_THREADS;
constexpr int kCcCounts = 256 + 1;  // per-(chunk, wave) root counts of the all-in-LDS variant (kCcNodes / 64 + kCcThreads / 64 <= 256) + the total
constexpr int kCcBoxes = 2048;   // bounding boxes per scan held in LDS (7 words each, in the key table once the search is over)
constexpr int kCcBuckets = 8192; // entries of the key-bucket index (uint16 node numbers; the generic variant: kCcNodes 32-bit entries)
constexpr int kCcExactMaxNodes = 4096;  // generic variant: nodes in components with irregular runs that are re-clustered exactly
constexpr int kCcBad = 256;          // generic variant: apri points outside the grid that are listed (more: every slot / node is looked at)
constexpr int kCcBadVoxel = 4096;    // ... and the largest voxel whose slots one thread walks for them
constexpr int kCcSlotsBig = 262144;  // generic variant: the nodes live in HBM, which leaves LDS for the bit arrays of this many points

static_assert(7 * kCcBoxes <= kCcNodes, "box records must fit the released key table");
constexpr size_t kCcLdsBytes = (size_t)(2 * kCcNodes + 3 * (kCcSlots / 32) + 3 * (kCcNodes / 32) + kCcBuckets / 2 + 32) * 4;
static_assert(kCcLdsBytes <= 160 * 1024, "one workgroup per CU: all of its LDS");
static_assert((size_t)(kCcNodes + 3 * (kCcSlotsBig / 32)) * 4 <= kCcLdsBytes, "generic layout inside the same LDS");

__device__ __forceinline__ int cc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t cc_ldu(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_find(int* parent, int x) {
    int p = cc_ld(&parent[x]);
    while (p != x) {
        const int gp = cc_ld(&parent[p]);
        if (gp != p) atomicMin(&parent[x], gp);  // path halving (only ever moves towards smaller ancestors)
        x = p;
        p = gp;
    }
    return x;
}
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(&parent[a], a, b) == a) return;  // a was still a root: now hangs under the smaller b
    }
}
__device__ __forceinline__ int cc_lower_bound(const int* keys, int nv, int key) {
    int lo = 0, hi = nv;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
__device__ __forceinline__ bool cc_bit(const int* bits, int i) { return (cc_ld(&bits[i >> 5]) >> (i & 31)) & 1; }
__device__ __forceinline__ void cc_set(int* bits, int i) { atomicOr(&bits[i >> 5], 1 << (i & 31)); }

// sorted voxel keys of the scan (`k`: LDS in the FAST variant, HBM otherwise) + bucket index in LDS: tab[b] = first node whose
// key is >= b << bshift, for the keys a search can ask for (0 .. R*S*Az - 1).  A lower bound then costs two table reads and a
// search among the few keys of one bucket instead of log2(nv) dependent reads.
template <typename TabT>
struct CcKeys {
    const int* k;
    int nv;
    const TabT* tab;
    int bshift;
    int first = 0;  // searches start at this node or later (a window of the node list: cc_search_windows)
};
template <typename TabT>
__device__ __forceinline__ int cc_lower_bound2(const CcKeys<TabT>& K, int key) {  // key >= 0
    const int b = key >> K.bshift;
    int lo = (int)K.tab[b], hi = (int)K.tab[b + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (K.k[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// neighbourhood of triple t for node `me`: unions with every occupied voxel found, marks them touched
template <typename TabT>
__device__ __forceinline__ bool cc_search(const CcKeys<TabT>& K, int* parent, int* touched, int me, int32_t t, int R, int S, int Az) {
    const int ri = (t & 2047) - 2, si = ((t >> 11) & 2047) - 2, ai = ((t >> 22) & 1023) - 2;
    const int ylo = max(si - 1, 0), yhi = min(si + 1, S - 1);
    bool found = false;
    if (ylo > yhi) return false;
    for (int z = ai - 1; z <= ai + 1; ++z) {
        if (z > Az - 1 || z < 0) continue;
        for (int x = ri - 1; x <= ri + 1; ++x) {
            if (x > R - 1 || x < 0) continue;
            const int k0 = x * S + ylo + z * R * S, k1 = k0 + (yhi - ylo);
            for (int u = cc_lower_bound2(K, k0); u < K.nv && K.k[u] <= k1; ++u) {
                cc_set(touched, u);  // every point of u joins (ssc.cpp:316)
                if (u != me) cc_union(parent, me, u);
                found = true;
            }
        }
    }
    return found;
}

// union that hands back the surviving root (the caller keeps it as its next starting point)
__device__ __forceinline__ int cc_union_r(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return a;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(&parent[a], a, b) == a) return b;
    }
}
// A REGULAR node is a voxel whose opener's triple is in range and encodes to the voxel's own key: it finds itself (so it is
// touched and found), and two regular voxels find each other, so such a pair is joined once, by the one with the larger
// index looking backwards (cc_search_half).  The few irregular nodes (-1 bins, extra runs) run the full search around their
// own triple, and an irregular VOXEL also looks around its key's own triple on behalf of the regular voxels that find it there.
template <typename TabT>
__device__ __forceinline__ void cc_search_canon(const CcKeys<TabT>& K, int* parent, int* touched, const int* regular, int me, int key, int R,
                                                int S, int Az) {
    const int RS = R * S;
    const int ai = key / RS, rem = key - ai * RS;
    const int ri = rem / S, si = rem - ri * S;
    const int ylo = max(si - 1, 0), yhi = min(si + 1, S - 1);
    for (int z = max(ai - 1, 0); z <= min(ai + 1, Az - 1); ++z)
        for (int x = max(ri - 1, 0); x <= min(ri + 1, R - 1); ++x) {
            const int k0 = x * S + ylo + z * RS, k1 = k0 + (yhi - ylo);
            for (int u = cc_lower_bound2(K, k0); u < K.nv && K.k[u] <= k1; ++u) {
                if (u == me || !cc_bit(regular, u)) continue;
                cc_set(touched, me);  // the regular voxel u finds me here (ssc.cpp:316)
                cc_union(parent, me, u);
            }
        }
}

// Regular voxels find themselves and each other mutually, so a regular node only looks BACKWARDS in key order (z-major, then
// range, then sector): the row (z, x-1) and the three rows of plane z-1 -- four lower bounds, taken in lockstep so that their
// reads overlap, instead of nine one after the other.
//   Consecutive occupied sectors of a row form a RUN; its nodes start out pointing at the run's head (cc_link_runs: no
// atomics, flat trees).  Two runs of neighbouring rows that touch are joined as soon as ONE touching pair is, and the pair
// where the node or the candidate is the HEAD of its run always exists (the head of the run that starts later touches the
// other run): a node in the middle of a run skips the candidates in the middle of theirs -- the unions left are one or two per
// run, every find is a step or two.  Irregular voxels do not search like this: they are runs of their own (always heads).
//   RUNS (parents in LDS, runs linked up front): a candidate that continues the run of the candidate before it is in that one's
// component already and is skipped, as is the predecessor of a node inside a run -- four or five unions instead of thirteen.
template <bool RUNS = false, typename TabT>
__device__ __forceinline__ void cc_search_half(const CcKeys<TabT>& K, int* parent, const int* heads, int me, int ri, int si, int ai, int R,
                                               int S, int Az) {
    const int ylo = max(si - 1, 0), yhi = min(si + 1, S - 1);
    int k0[4], k1[4], lo[4], hi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int x = (q == 3) ? ri - 1 : ri - 1 + q;
        const int z = (q == 3) ? ai : ai - 1;
        const bool valid = z >= 0 && x >= 0 && x <= R - 1;
        k0[q] = valid ? x * S + ylo + z * R * S : -1;
        k1[q] = k0[q] + (yhi - ylo);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int b = max(k0[q], 0) >> K.bshift;
        lo[q] = max((int)K.tab[b], K.first);
        hi[q] = max((int)K.tab[b + 1], K.first);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (k0[q] < 0) lo[q] = hi[q] = K.first;
    bool more = true;
    while (more) {
        more = false;
        int kq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) kq[q] = K.k[min((lo[q] + hi[q]) >> 1, K.nv - 1)];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (lo[q] < hi[q]) {
                const int mid = (lo[q] + hi[q]) >> 1;
                if (kq[q] < k0[q])
                    lo[q] = mid + 1;
                else
                    hi[q] = mid;
                more |= lo[q] < hi[q];
            }
        }
    }
    int cand[12], hw[12], pu[12];  // a range holds at most three keys (sectors y-1 .. y+1), distinct and ascending
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int u = min(lo[q] + e, K.nv - 1);
            cand[q * 3 + e] = K.k[u];
            hw[q * 3 + e] = heads ? heads[u >> 5] : -1;
            pu[q * 3 + e] = cc_ld(&parent[u]);  // read together: a candidate that hangs under my root already costs nothing more
        }
    const int prev = K.k[max(me - 1, 0)];
    // heads == nullptr (parents in LDS, where a union is cheap): every node is treated as a head -- all pairs are joined
    const bool me_head = heads ? ((heads[me >> 5] >> (me & 31)) & 1) : true;
    int ra = me;
    // the predecessor in the row is found too (ssc.cpp:316); inside a linked run it is the parent already
    if (me_head && me > 0 && si >= 1 && prev == K.k[me] - 1) ra = cc_union_r(parent, ra, me - 1);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int u = lo[q] + e;
            if (!(k0[q] >= 0 && u < K.nv && cand[q * 3 + e] <= k1[q])) continue;
            if (pu[q * 3 + e] == ra) continue;  // (a parent link is for good: u is in ra's component)
            const bool u_head = (hw[q * 3 + e] >> (u & 31)) & 1;
            if (RUNS) {
                if (e == 0 || u_head) ra = cc_union_r(parent, ra, u);
                continue;
            }
            if (me_head || u_head) ra = cc_union_r(parent, ra, u);
        }
    // I am a candidate of the nodes of the next row and plane: hanging straight under the root I ended at keeps their finds at a
    // step and lets most of their candidates pass the test above
    if (ra < me) atomicMin(&parent[me], ra);
}

// The occupied voxels around triple t in the order findVoxelNeighbors lists them (ssc.cpp:395-411: range outermost, azimuth
// innermost); f(u) returns false to stop
template <typename TabT, typename Fn>
__device__ __forceinline__ void cc_for_each_listed(const CcKeys<TabT>& K, int32_t t, int R, int S, int Az, Fn f) {
    const int ri = (t & 2047) - 2, si = ((t >> 11) & 2047) - 2, ai = ((t >> 22) & 1023) - 2;
    for (int x = max(ri - 1, 0); x <= min(ri + 1, R - 1); ++x)
        for (int y = max(si - 1, 0); y <= min(si + 1, S - 1); ++y)
            for (int z = max(ai - 1, 0); z <= min(ai + 1, Az - 1); ++z) {
                const int key = x * S + y + z * R * S;
                const int u = cc_lower_bound2(K, key);
                if (u < K.nv && K.k[u] == key)
                    if (!f(u)) return;
            }
}

// cc_for_each_listed's list of triple t into lst[] (same voxels, same order), the searches in LOCKSTEP: the three sectors of a (range,
// azimuth) pair are consecutive keys, so the 27 cells are 9 lower bounds whose table reads and key reads are issued together, then
// three keys behind each -- a handful of dependent round trips to the key table instead of a hundred (round 6: the rows of the exact
// re-clustering of a 40 k-node component took 4-5 ms to build one search after the other).  Returns the number of entries.
template <typename TabT>
__device__ __forceinline__ int cc_list27(const CcKeys<TabT>& K, int32_t t, int R, int S, int Az, int (&lst)[27]) {
    const int ri = (t & 2047) - 2, si = ((t >> 11) & 2047) - 2, ai = ((t >> 22) & 1023) - 2;
    const int ylo = max(si - 1, 0), yhi = min(si + 1, S - 1);
    int lo[9], hi[9], k0[9];
    bool on[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int x = ri + r / 3 - 1, z = ai + r % 3 - 1;
        on[r] = ylo <= yhi && x >= 0 && x <= R - 1 && z >= 0 && z <= Az - 1;
        k0[r] = on[r] ? x * S + ylo + z * R * S : 0;
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int b = k0[r] >> K.bshift;
        lo[r] = on[r] ? (int)K.tab[b] : 0;
        hi[r] = on[r] ? (int)K.tab[b + 1] : 0;
    }
    for (;;) {
        bool more = false;
        int mid[9], km[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            mid[r] = (lo[r] + hi[r]) >> 1;
            km[r] = lo[r] < hi[r] ? K.k[mid[r]] : 0;
        }
#pragma unroll
        for (int r = 0; r < 9; ++r)
            if (lo[r] < hi[r]) {
                if (km[r] < k0[r])
                    lo[r] = mid[r] + 1;
                else
                    hi[r] = mid[r];
                more |= lo[r] < hi[r];
            }
        if (!more) break;
    }
    int kk[9][3];
#pragma unroll
    for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int e = 0; e < 3; ++e) kk[r][e] = (on[r] && lo[r] + e < K.nv) ? K.k[lo[r] + e] : 0x7fffffff;
    int n = 0;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int y = si - 1 + dy;
#pragma unroll
            for (int dz = 0; dz < 3; ++dz) {
                const int r = dx * 3 + dz;
                if (!on[r] || y < ylo || y > yhi) continue;
                const int key = k0[r] + (y - ylo);
                // (the keys behind the lower bound ascend: key k0 + d can only sit at offset <= d)
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    if (kk[r][e] == key) lst[n++] = lo[r] + e;
            }
        }
    return n;
}

// Run heads of the voxel list + flat initial forest: head(v) = v starts a run (v == 0, or its key does not continue the
// predecessor's inside the row, or one of the two is irregular); parent[v] = the head of v's run (the latest head at or
// before v: ballots inside a wave, one LDS word per wave across the workgroup, a carry across the 1024-node chunks).
// `regular` = nullptr: every voxel is regular.  Extra-run nodes (>= nv) are their own parents.
__device__ __forceinline__ void cc_link_runs(const int* keys, int nv, int nn, int S, const int* regular, int* heads, int* parent, int* wlast,
                                             int off = 0) {  // off: the node number of entry 0 (a window of the node list)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;  // latest head before this chunk
    for (int j0 = 0; j0 < nv; j0 += kCcThreads) {
        const int j = j0 + tid;
        bool head = false;
        if (j < nv) {
            const int key = keys[j], pk = keys[max(j - 1, 0)];
            head = j == 0 || pk != key - 1 || key < 0 || (key % S) == 0;
            if (regular && !head) head = !cc_bit(regular, j) || !cc_bit(regular, j - 1);
            if (regular && !cc_bit(regular, j)) head = true;
        }
        const unsigned long long b = __ballot(head);
        if ((tid & 31) == 0 && j0 + (tid & ~31) < nv) heads[j >> 5] = (int)(unsigned)((tid & 32) ? (b >> 32) : b);
        if (lane == 0) wlast[wave] = b ? j0 + (wave << 6) + 63 - __clzll((long long)b) : -1;
        __syncthreads();
        int before = carry;  // latest head in the waves before mine
        for (int w = 0; w < wave; ++w) before = max(before, wlast[w]);
        const unsigned long long upto = b & ((2ull << lane) - 1ull);
        const int mine = upto ? j0 + (wave << 6) + 63 - __clzll((long long)upto) : before;
        if (j < nv) parent[j] = mine + off;
        int last = carry;
        for (int w = 0; w < kCcThreads / 64; ++w) last = max(last, wlast[w]);
        carry = last;
        __syncthreads();
    }
    for (int j = nv + tid; j < nn; j += kCcThreads) parent[j] = j;
}

// Generic variant (nodes in HBM): the backward search of the regular nodes, one WINDOW of whole z-planes at a time with the
// window's keys and parents in LDS.  A regular node only joins nodes of its own plane and of the plane before it, so a window
// holds the plane before its first one as well; a window's forest is flattened into the scan's parent array when it is done
// (parents are global node numbers throughout: the LDS arrays are addressed through pointers shifted by the window's start),
// and what the window joined among the nodes of that earlier plane -- which belong to the window before -- is joined in HBM,
// a few unions per window.  Returns false, with nothing changed, when two consecutive planes do not fit `cap` nodes.
//   regular == nullptr: every node is regular.  Nodes outside the grid's key range (negative keys, extra runs) are left as
// their own parents for the caller's pass over the irregular nodes.
// the same for a window of the node list held in LDS: the head bits first, then every node looks its head up in the words at
// and before its own (no barrier per chunk; entry 0 is a head); parents are node numbers, entry i is node off + i
__device__ __forceinline__ void cc_link_runs_lds(const int* keys, int count, int S, const int* regular, int* heads, int* parent, int off) {
    const int tid = threadIdx.x;
    for (int j0 = 0; j0 < count; j0 += kCcThreads) {
        const int j = j0 + tid;
        bool head = false;
        if (j < count) {
            const int key = keys[j], pk = keys[max(j - 1, 0)];
            head = j == 0 || pk != key - 1 || key < 0 || (key % S) == 0;
            if (regular && !head) head = !cc_bit(regular, j) || !cc_bit(regular, j - 1);
        }
        const unsigned long long b = __ballot(head);
        if ((tid & 31) == 0 && j0 + (tid & ~31) < count) heads[j >> 5] = (int)(unsigned)((tid & 32) ? (b >> 32) : b);
    }
    __syncthreads();
    for (int j = tid; j < count; j += kCcThreads) {
        int w = j >> 5;
        unsigned m = (unsigned)heads[w] & (0xffffffffu >> (31 - (j & 31)));
        while (!m) m = (unsigned)heads[--w];
        parent[j] = off + (w << 5) + 31 - __clz(m);
    }
}

#ifdef SCVOD_PROFILE
#define CCW_PROF_PARAM , unsigned long long& t_prev
#define CCW_PROF_ARG , t_prev
#else
#define CCW_PROF_PARAM
#define CCW_PROF_ARG
#endif
template <typename TabT>
__device__ __forceinline__ bool cc_search_windows(const CcKeys<TabT>& K, int* parent_g, const int* regular, int nn, int R, int S, int Az, int* lds,
                                                  int lds_words, int* wlast CCW_PROF_PARAM) {
    const int tid = threadIdx.x, RS = R * S;
    // LDS: [plane starts Az + 1][regular bits of the window][keys cap + 1][parents cap + 1]
    if (Az + 1 + 64 > lds_words / 4) return false;
    int* pstart = lds;
    const int cap = ((lds_words - (Az + 1)) * 32 / 66) - 40;  // 2 words + 2 bits per node
    int* reg_l = pstart + Az + 1;                              // [cap / 32 + 2]
    int* heads_l = reg_l + (cap >> 5) + 2;                     // [cap / 32 + 2]
    int* keys_l = heads_l + (cap >> 5) + 2;                    // [cap + 1]
    int* par_l = keys_l + cap + 1;                             // [cap + 1]
    for (int z = tid; z <= Az; z += kCcThreads) pstart[z] = z >= Az ? K.nv : cc_lower_bound2(K, z * RS);
    __syncthreads();
    bool too_big = false;
    for (int z = tid; z < Az; z += kCcThreads) too_big |= pstart[z + 1] - (max(pstart[max(z - 1, 0)] - 1, 0) & ~31) > cap;
    if (__syncthreads_or(too_big ? 1 : 0)) return false;
    for (int j = tid; j < nn; j += kCcThreads) parent_g[j] = j;
    CCW_MARK(1);
    int z = 0;
    while (z < Az) {
        __syncthreads();
        if (tid == 0) {
            const int p0 = pstart[max(z - 1, 0)];
            const int w0 = max(p0 - 1, 0) & ~31;  // (the predecessor read of the window's first node; whole words of the regular bits)
            int lo = z + 1, hi = Az;              // the last plane end that still fits
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pstart[mid] - w0 <= cap)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            wlast[0] = w0;
            wlast[1] = p0;
            wlast[2] = pstart[z];
            wlast[3] = pstart[lo];
            wlast[4] = lo;
        }
        __syncthreads();
        const int w0 = wlast[0], p0 = wlast[1], c0 = wlast[2], c1 = wlast[3], z_end = wlast[4];
        CCW_MARK(2);
        for (int i = w0 + tid; i < c1; i += kCcThreads) keys_l[i - w0] = K.k[i];
        if (regular)
            for (int w = (w0 >> 5) + tid; w <= ((c1 - 1) >> 5); w += kCcThreads) reg_l[w - (w0 >> 5)] = regular[w];
        __syncthreads();
        cc_link_runs_lds(keys_l, c1 - w0, S, regular ? reg_l : (const int*)nullptr, heads_l, par_l, w0);
        __syncthreads();
        CCW_MARK(3);
        CcKeys<TabT> KL = K;
        KL.k = keys_l - w0;
        KL.nv = c1;
        KL.first = w0;
        int* par = par_l - w0;
        for (int j = c0 + tid; j < c1; j += kCcThreads) {
            if (regular && !((reg_l[(j - w0) >> 5] >> (j & 31)) & 1)) continue;
            const int key = KL.k[j];
            const int ai = key / RS, rem = key - ai * RS;
            const int ri = rem / S, si = rem - ri * S;
            cc_search_half<true>(KL, par, heads_l - (w0 >> 5), j, ri, si, ai, R, S, Az);
        }
        __syncthreads();
        CCW_MARK(4);
        for (int g = c0 + tid; g < c1; g += kCcThreads) parent_g[g] = cc_find(par, g);
        for (int g = p0 + tid; g < c0; g += kCcThreads) {
            const int r = cc_find(par, g);
            // (the window before left both under its own root when it had them in one component: the usual case)
            if (r != g && cc_ld(&parent_g[g]) != cc_ld(&parent_g[r])) cc_union(parent_g, g, r);
        }
        z = z_end;
        CCW_MARK(5);
    }
    __syncthreads();
    return true;
}

// box area of a cluster (getDescriptorByEigenValue's f_11(0, 7)): float extents, double product
__device__ __forceinline__ double cc_box_square(float mnx, float mny, float mxx, float mxy) { return (double)(mxx - mnx) * (double)(mxy - mny); }
// type of a cluster from its box and member count: refineClusterByBoundingBox (ssc.cpp:437-467) + the box part of recognize
// (ssc.cpp:849-872).  0 erased, 1 other, 2 car.  Shared by the clustering and the intensity merge (scvod_k_merge.inc).
__device__ __forceinline__ uint32_t cc_type_rule(const DevParams& P, float mnx, float mny, float mnz, float mxx, float mxy, float mxz, int cnt) {
    const float diff_zf = mxz - mnz;
    if (mnz > 0.f || cnt < P.to_be_class || diff_zf < 0.2f) return 0;
    const double square = cc_box_square(mnx, mny, mxx, mxy);
    if (square > (double)P.car_square) return 1;
    if ((double)mnz < (double)P.min_z && square < (double)P.car_square && (double)mxz < (double)P.max_z) return 2;
    return 1;
}
// a cluster of type 1 that recognize hands to regionGrowing (ssc.cpp:849): the `square > car_square` branch of cc_type_rule
__device__ __forceinline__ bool cc_rg_candidate(const DevParams& P, float mnx, float mny, float mxx, float mxy) {
    return cc_box_square(mnx, mny, mxx, mxy) > (double)P.car_square;
}
__device__ __forceinline__ uint32_t f2ord(float f) { return float_sort_key(f); }
__device__ __forceinline__ float ord2f(uint32_t u) { return u2f((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}

// ---- generic variant: does an irregular run need the visiting order at all?  (one WAVE per run, wave-uniform answer)
// "Everything found is joined" differs from clusterAndCreateFrame (ssc.cpp:303-350) only where a find is one-sided and is
// never repeated the other way round: voxels that hold a point with its triple inside the grid ("proper" voxels) that list
// each other always end up together (the later of their first visits sees a visited point in the other), so only the
// finds around an irregular run can be lost -- (1) the voxels the run lists, (2) the run's home voxel and whoever lists
// that.  Both are settled by what stands in the 3x3x3 cells around the run's triple and around its key's own cell:
//  (1) a visiting point i is joined with listed voxel k for sure when k holds a visited point (first point < i, or a lister
//      of k had its third visit -- second, if k sits behind that lister's own cell -- before i) or when every listed voxel
//      behind k is still untouched at time i (nobody around it, regular or not, was visited before i: then i opens a
//      cluster with all of them or was labelled itself); the listed voxels must be proper and every group of them that
//      find each other must hold one that is joined for sure;
//  (2) the home voxel: with two regular points (its second regular visit joins its own cell) or one that comes after the
//      run's first point nothing can be lost; otherwise a lister of the home cell must join it for sure -- three regular
//      points, two if the cell sits behind its own, or a regular point after the home voxel's first point (which is visited
//      by then) -- one such lister when the home voxel has a regular point of its own (that one finds the others), one per
//      group of listers that find each other when it has none; a home voxel nobody lists is alone in both readings.
// false = not proven: the run's component is clustered again with the visiting order (cc_scan_impl below).  The rule is
// pinned on the CPU against the oracle's loop by tests/test_irregular_runs_rule.py (same statement in numpy).
struct CcRunRule {
    CcKeys<uint32_t> K;
    const int32_t* vbeg;
    const int32_t* vpts;
    const int32_t* idx3;
    const int* triple;   // [nn] opener triples
    const int* irrl;     // [n_irr] the irregular nodes
    const int* extras;   // opener slots of the extra runs
    const int* vstart;   // bit per slot: starts a voxel
    const int* prefix;
    int nv, n_irr, R, S, Az, kspan;
};
struct CcVoxInfo {
    int first, nreg, r1, r2, r3, lastreg;  // first point; regular points: how many of the first 32 (capped at 3), the first three, the last
};
__device__ __forceinline__ bool cc_point_regular(const CcRunRule& Q, int pt, int key) {
    const int t = Q.idx3[pt];
    const int ri = (t & 2047) - 2, si = ((t >> 11) & 2047) - 2, ai = ((t >> 22) & 1023) - 2;
    return ri >= 0 && ri < Q.R && si >= 0 && si < Q.S && ai >= 0 && ai < Q.Az && ri * Q.S + si + ai * Q.R * Q.S == key;
}
__device__ __forceinline__ CcVoxInfo cc_vox_info(const CcRunRule& Q, int u) {
    CcVoxInfo f;
    const int b = Q.vbeg[u], e = Q.vbeg[u + 1], key = Q.K.k[u];
    f.nreg = 0;
    f.r1 = f.r2 = f.r3 = 0x7fffffff;
    f.lastreg = -1;
    // the first four slots and the last one together (two round trips: points, then their triples); more only for a voxel
    // that holds irregular points among its first four
    int pt[5];
    bool rg[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) pt[k] = Q.vpts[k < 4 ? min(b + k, e - 1) : e - 1];
#pragma unroll
    for (int k = 0; k < 5; ++k) rg[k] = cc_point_regular(Q, pt[k], key);
    f.first = pt[0];
    auto take = [&](int p) {
        ++f.nreg;
        if (f.nreg == 1) f.r1 = p;
        if (f.nreg == 2) f.r2 = p;
        if (f.nreg == 3) f.r3 = p;
        f.lastreg = p;
    };
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (b + k < e && rg[k] && f.nreg < 3) take(pt[k]);
    for (int k = b + 4; k < min(e, b + 32) && f.nreg < 3; ++k) {
        const int p = Q.vpts[k];
        if (cc_point_regular(Q, p, key)) take(p);
    }
    if (rg[4])
        f.lastreg = max(f.lastreg, pt[4]);
    else
        for (int k = e - 2; k >= max(b, e - 8); --k) {  // (a lower bound of the last regular point is all the rule needs)
            const int p = Q.vpts[k];
            if (p <= f.lastreg) break;
            if (cc_point_regular(Q, p, key)) {
                f.lastreg = p;
                break;
            }
        }
    return f;
}
__device__ __forceinline__ int cc_cell_voxel(const CcRunRule& Q, int x, int y, int z) {  // voxel of a cell, -1 = none / outside the grid
    if (x < 0 || x >= Q.R || y < 0 || y >= Q.S || z < 0 || z >= Q.Az) return -1;
    const int key = x * Q.S + y + z * Q.R * Q.S;
    const int u = cc_lower_bound2(Q.K, key);
    return (u < Q.K.nv && Q.K.k[u] == key) ? u : -1;
}
// Each half of the wave (lanes 0-26 and 32-58) holds the cells of a 3x3x3 block in list order (range outermost, azimuth
// innermost, ssc.cpp:395-411): smallest position (0-26) of the group of `on` cells a lane's cell hangs together with
// (adjacent cells list each other); the two halves are independent blocks
__device__ __forceinline__ int cc_cell_groups(bool on, int lane) {
    const int base = lane & 32, l = lane & 31;
    const unsigned m = (unsigned)(__ballot(on) >> base);
    const int ax = l / 9, ay = (l / 3) % 3, az = l % 3;
    int lab = l;
    for (;;) {
        int best = lab;
        for (int b = 0; b < 27; ++b) {
            const int lb = __shfl(lab, base + b);
            if (on && ((m >> b) & 1) && abs(ax - b / 9) <= 1 && abs(ay - (b / 3) % 3) <= 1 && abs(az - b % 3) <= 1) best = min(best, lb);
        }
        const bool changed = best != lab;
        lab = best;
        if (!__any(changed)) break;
    }
    return lab;
}
__device__ __forceinline__ unsigned cc_group_mask(bool flag, int lab, int lane) {  // bit g: a lane of my half with `flag` has group label g
    const int base = lane & 32;
    const unsigned m = (unsigned)(__ballot(flag) >> base);
    unsigned gm = 0;
    for (int b = 0; b < 27; ++b) {
        const int lb = __shfl(lab, base + b);
        if ((m >> b) & 1) gm |= 1u << lb;
    }
    return gm;
}
__device__ __noinline__ bool cc_run_is_plain(const CcRunRule& Q, int j, int lane) {
    const int nv = Q.nv, R = Q.R, S = Q.S, Az = Q.Az, RS = R * S;
    const int o = (j < nv) ? Q.vbeg[j] : Q.extras[j - nv];
    int v = j;
    if (j >= nv) {
        const unsigned m = (unsigned)Q.vstart[o >> 5] & (0xffffffffu >> (31 - (o & 31)));
        v = Q.prefix[o >> 5] + __popc(m) - 1;
    }
    const int i = Q.vpts[o], t = Q.triple[j], kv = Q.K.k[v];
    const int ri = (t & 2047) - 2, si = ((t >> 11) & 2047) - 2, ai = ((t >> 22) & 1023) - 2;
    if (ri >= 0 && ri < R && si >= 0 && si < S && ai >= 0 && ai < Az && ri * S + si + ai * RS == kv) return true;  // a regular run behind an irregular opener
    // lanes 0-26: the cells around the triple (1); lanes 32-58: the cells around the key's own cell (2); lane 63: the home voxel
    const int half = lane >> 5, l = lane & 31;
    const int lx = l / 9 - 1, ly = (l / 3) % 3 - 1, lz = l % 3 - 1;
    const bool home_cell = kv >= 0 && kv < Q.kspan;
    const int hz = home_cell ? kv / RS : 0, hrem = kv - hz * RS;
    const int hx = home_cell ? hrem / S : 0, hy = home_cell ? hrem - hx * S : 0;
    int u = -1;
    if (l < 27) {
        if (half == 0)
            u = cc_cell_voxel(Q, ri + lx, si + ly, ai + lz);
        else if (home_cell && l != 13)
            u = cc_cell_voxel(Q, hx + lx, hy + ly, hz + lz);
    }
    if (lane == 63) u = v;
    CcVoxInfo f;
    f.first = 0x7fffffff;
    f.nreg = 0;
    f.r1 = f.r2 = f.r3 = 0x7fffffff;
    f.lastreg = -1;
    if (u >= 0) f = cc_vox_info(Q, u);
    const bool behind = lx < 0 || (lx == 0 && (ly < 0 || (ly == 0 && lz < 0)));  // the block's centre sits behind this lane's own cell in the lane's list
    // (1) the listed voxels
    {
        const bool occ = half == 0 && l < 27 && u >= 0;
        if (__any(occ && f.nreg == 0)) return false;
        const unsigned m = (unsigned)__ballot(occ);  // (lanes 0-26)
        if (m) {
            const int lab = cc_cell_groups(occ, lane);
            const int last = 31 - __clz((int)m);
            unsigned gm = cc_group_mask(occ && (f.first < i || lane == last), lab, lane);
            if (__any(occ && !((gm >> lab) & 1))) {
                // the look around every listed voxel (rare: a group of listed voxels that is not settled by the first points alone)
                unsigned untouched = 0, labelled = 0;
                for (int b = 0; b < 27; ++b) {
                    if (!((m >> b) & 1)) continue;
                    const int bx = ri + b / 9 - 1, by = si + (b / 3) % 3 - 1, bz = ai + b % 3 - 1;
                    const int w = lane < 27 ? cc_cell_voxel(Q, bx + lx, by + ly, bz + lz) : -1;
                    CcVoxInfo g;
                    g.first = 0x7fffffff;
                    g.nreg = 0;
                    g.r2 = g.r3 = 0x7fffffff;
                    if (w >= 0) g = cc_vox_info(Q, w);
                    bool early = w >= 0 && g.first < i;  // (lane 13 is the listed voxel itself)
                    if (Q.n_irr > kCcBad) early = true;  // (too many irregular runs to ask each of them)
                    for (int y = lane; y < Q.n_irr && !early; y += 64) {
                        const int q = Q.irrl[y];
                        const int oq = (q < nv) ? Q.vbeg[q] : Q.extras[q - nv];
                        const int tq = Q.triple[q];
                        const int qr = (tq & 2047) - 2, qs = ((tq >> 11) & 2047) - 2, qa = ((tq >> 22) & 1023) - 2;
                        if (Q.vpts[oq] < i && abs(qr - bx) <= 1 && abs(qs - by) <= 1 && abs(qa - bz) <= 1) early = true;
                    }
                    if (!__any(early)) untouched |= 1u << b;
                    const bool sl = w >= 0 && lane != 13 && ((g.nreg >= 3 && g.r3 < i) || (g.nreg >= 2 && g.r2 < i && behind));
                    if (__shfl(f.first, b) < i || __any(sl)) labelled |= 1u << b;
                }
                const unsigned later = lane < 27 ? (m & ~((2u << lane) - 1u)) : 0u;
                const bool sure = occ && (((labelled >> lane) & 1) || (later & ~untouched) == 0);
                gm = cc_group_mask(sure, lab, lane);
                if (__any(occ && !((gm >> lab) & 1))) return false;
            }
        }
    }
    // (2) the home voxel
    const int h_nreg = __shfl(f.nreg, 63), h_r1 = __shfl(f.r1, 63), h_first = __shfl(f.first, 63);
    if (h_nreg >= 2 || (h_nreg == 1 && i < h_r1) || !home_cell) return true;
    const bool around = half == 1 && l < 27 && u >= 0;
    const bool fin = around && f.nreg > 0;
    const bool strong = fin && (f.nreg >= 3 || (f.nreg >= 2 && behind) || f.lastreg > h_first);
    if (h_nreg == 1) return !__any(around) || __any(strong);
    if (!__any(fin)) return true;
    const int lab = cc_cell_groups(fin, lane);
    const unsigned gm = cc_group_mask(strong, lab, lane);
    return !__any(fin && !((gm >> lab) & 1));
}

// FAST: every table of the scan in LDS, the pointers are LDS pointers at compile time (ds_* instead of flat_* accesses);
// gives up (returns false, nothing published yet) when the extra runs push the node count over kCcNodes.  The generic
// variant picks LDS or arena scratch per table at run time.
extern __shared__ int cc_smem[];

// A wave adds 1 to the LDS cell of `key` (key < 0: nothing) with ONE atomic per RUN of equal keys among consecutive lanes -- the points
// and voxels of a scan arrive cluster after cluster, so most waves add to a single address (measured: k_cc_scan 3.27 -> 3.20 ms).
// Returns what atomicAdd(cell, 1) would have returned for some order of the lanes.  Wave-uniform call (shuffles, ballot).
__device__ __forceinline__ uint32_t cc_run_add(uint32_t* cell, int key) {
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(key, 1);
    const bool head = (lane == 0) || (prev != key);
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = (2ull << lane) - 1ull;  // lanes 0 .. lane (lane 63: all)
    const int head_lane = 63 - __clzll((long long)(heads & upto));
    const unsigned long long after = heads & ~upto;
    const int run_end = after ? (__ffsll((long long)after) - 1) : 64;
    uint32_t old = 0;
    if (head && key >= 0) old = atomicAdd(cell, (uint32_t)(run_end - lane));
    return __shfl(old, head_lane) + (uint32_t)(lane - head_lane);
}
// ---- the exact re-clustering of LARGE components, shared between workgroups (round 6) -------------------------------------------
// A component of tens of thousands of nodes around an irregular run (a return at polar angle exactly 0 on a facade of a 128-beam
// scan) needs a dozen or more Jacobi rounds over all of its nodes; on the scan's one workgroup that is 15-50 ms, which a batch waits
// for (round 5: off by default, 32 of 1000 OS128 scans kept "everything found is joined").  The rounds are data-parallel over the
// listed nodes and read / write global memory only, so the scan's workgroup (the LEADER) publishes them on a board and whoever has
// nothing else to do takes chunks of 1024 nodes: k_cc_scan is launched with extra blocks behind the scans' (HELPERS: they come up
// when the scans have all been handed out, i.e. on the CUs that the short scans vacate while the slow ones still run).  The leader
// takes chunks itself and never waits for anybody who has not already claimed a chunk: without a single helper it does all the work
// (no assumption about dispatch order or residency; a helper leaves once every scan is past this phase, and after a bounded spin
// in any case).  Hand-off per round (cdna_hip_programming.md section 6, guideline 16): the leader's stores -> agent-scope release ->
// the slot's 64-bit claim word (round number << 32 | next chunk) -> a helper's claim (an atomic add: it learns the round its chunk
// belongs to from the value it gets back) -> agent-scope acquire -> plain loads; the helpers' results are atomicMin's on the next
// round's times (performed at the memory side) -> release -> the slot's done counter -> the leader's acquire.
constexpr int kCcHelpMinNodes = 6144;  // listed nodes from which a leader asks (below: a round is a few chunks, the hand-off would cost more than it saves)
// (kCcHelpSlots / kCcHelpHdr / kCcHelpSlotWords / kCcHelpWords: scvod_kernels.h -- the ctx allocates the board)

constexpr int kCcAggSlots = 8192;  // a helper block's LDS table per chunk: [tag = listed number | minimum sent to the next times | current time], direct-mapped
struct CcExactTabs {
    const int4* runs;        // [na] {first slot, home voxel, len | regular << 31, triple}
    const uint16_t* nbr16;   // [na][32] listed voxels, 0xffff none
    const int* Tg;           // [nv] labelling times of the last round
    const int* P1g;          // [nv] first point of a voxel
    int* Tng;                // [nv] next round's times (atomicMin)
    const int32_t* vpts;
    const int* La;           // [na] listed number -> node
    int* qnode;              // [na] position in a node's list from which its last point joins
    int* parent;             // [nn] the scan's forest
    int* touched;            // [nn bits]
    int* found;              // [nn bits]
    const int* keys;         // [nvox] the scan's sorted voxel keys
    const uint32_t* tabg;    // the leader's bucket index of the keys, copied to global memory (cc_lower_bound2)
    const int* loc;          // [nvox] voxel -> listed number, 0xffff not listed
    int nvox, R, S, Az, bshift;
    int* agg;                // LDS [2 * kCcAggSlots] or nullptr: a helper block's table of the minima a chunk sends to Tng (cc_exact_agg_*)
    bool remote;             // a helper block: what the leader rewrites between phases (Tg, qnode) is read / written past the caches (see cc_help_loop)
};
// labelling time of listed voxel i as the round sees it.  A helper block first brings the times of its chunk's targets into LDS ONCE each (a chunk
// of 1024 consecutive nodes names ~3 k targets ~25 times each: agent-scope look-ups are the device-wide bound of this kernel, see below)
__device__ __forceinline__ int cc_exact_time(const CcExactTabs& E, int i) {
    if (E.agg) {
        const int sl = i & (kCcAggSlots - 1);
        if (E.agg[sl] == i) return E.agg[2 * kCcAggSlots + sl];
        return cc_ld(&E.Tg[i]);
    }
    return E.remote ? cc_ld(&E.Tg[i]) : E.Tg[i];
}
// The rounds' traffic is what bounds them chip-wide: 27 agent-scope look-ups + up to 27 atomicMin per node and event triple, all served at the
// memory side (~25 G/s for the whole device: 11 ms of it per 1000 128-beam scans, whoever issues them).  A helper block has the LDS of its
// CU to itself, so it first reduces a chunk's minima there -- direct-mapped by listed number, 8192 slots, a conflicting target goes
// straight to memory -- and sends ONE atomicMin per distinct target (a chunk of 1024 consecutive nodes names ~3 k targets ~25 times each).
__device__ __forceinline__ void cc_exact_load_row(const uint16_t* nbr16, int x, uint32_t (&u)[28]) {  // 0xffffffff = no entry
    const uint4* row = reinterpret_cast<const uint4*>(nbr16 + (size_t)x * 32);
    uint4 r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = row[k];
    const uint32_t w[16] = {r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, r[1].z, r[1].w, r[2].x, r[2].y, r[2].z, r[2].w, r[3].x, r[3].y, r[3].z, r[3].w};
#pragma unroll
    for (int e = 0; e < 28; ++e) {
        const uint32_t v16 = (w[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
        u[e] = v16 == 0xffffu ? 0xffffffffu : v16;
    }
}

__device__ __forceinline__ void cc_exact_agg_clear(int* agg, int tid) {
    for (int i = tid; i < kCcAggSlots; i += kCcThreads) {
        agg[i] = -1;
        agg[kCcAggSlots + i] = 0x7fffffff;
    }
}
__device__ __forceinline__ void cc_exact_agg_flush(int* agg, int* Tng, int tid) {
    for (int i = tid; i < kCcAggSlots; i += kCcThreads) {
        const int u = agg[i];
        if (u < 0) continue;
        const int te = agg[kCcAggSlots + i];
        if (te != 0x7fffffff) atomicMin(&Tng[u], te);
    }
}
// the targets of listed node x (its listed voxels and its home voxel) claim their slots of the chunk's table
__device__ __forceinline__ void cc_exact_tags16(const CcExactTabs& E, int x) {
    const int4 c = E.runs[x];
    uint32_t u[28];
    cc_exact_load_row(E.nbr16, x, u);
    atomicCAS(&E.agg[c.y & (kCcAggSlots - 1)], -1, c.y);
#pragma unroll
    for (int k = 0; k < 27; ++k)
        if (u[k] != 0xffffffffu) atomicCAS(&E.agg[u[k] & (kCcAggSlots - 1)], -1, (int)u[k]);
}
__device__ __forceinline__ void cc_exact_agg_times(const CcExactTabs& E, int tid) {
    for (int i = tid; i < kCcAggSlots; i += kCcThreads) {
        const int u = E.agg[i];
        if (u >= 0) E.agg[2 * kCcAggSlots + i] = cc_ld(&E.Tg[u]);
    }
}
enum : int { kCcPhaseRound0 = 1, kCcPhaseRound = 2, kCcPhaseQ = 3, kCcPhaseUnion = 4, kCcPhaseRows = 5 };

// the visits of listed node x in one Jacobi round (DESIGN.md section 2, the state machine of clusterAndCreateFrame): the row in
// registers, the times / first points of its voxels gathered nine at a time (loads in flight together: a walk is a handful of round
// trips to HBM instead of two per listed voxel)
__device__ __noinline__ void cc_exact_visit16(const CcExactTabs& E, int x, bool round0) {
    const int4 c = E.runs[x];
    const int nev = c.z < 0 ? min(c.z & 0x7fffffff, 3) : c.z;
    uint32_t u[28];
    cc_exact_load_row(E.nbr16, x, u);
    const int tv = cc_exact_time(E, c.y);
    for (int p0 = 0; p0 < nev; p0 += 3) {
        int ie[3], qe[3], pq[3], st[3];
        bool on[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            on[e] = p0 + e < nev;
            ie[e] = on[e] ? E.vpts[c.x + p0 + e] : 0x7fffffff;
            qe[e] = -1;
            pq[e] = 0x7fffffff;
        }
#pragma unroll
        for (int c0 = 0; c0 < 27; c0 += 9) {
            int ta[9], pa[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const bool ok = u[c0 + k] != 0xffffffffu;
                const int idx = ok ? (int)u[c0 + k] : c.y;
                ta[k] = cc_exact_time(E, idx);
                pa[k] = E.P1g[idx];
                if (!ok) ta[k] = pa[k] = 0x7fffffff;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k)
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    if (on[e] && qe[e] < 0 && min(ta[k], pa[k]) < ie[e]) {
                        qe[e] = c0 + k;
                        pq[e] = pa[k];
                    }
        }
        // event e labels the listed voxels from position st[e] on
#pragma unroll
        for (int e = 0; e < 3; ++e) st[e] = !on[e] ? 1000 : ((round0 || tv < ie[e] || qe[e] < 0) ? 0 : (pq[e] < ie[e] ? qe[e] : qe[e] + 1));
        if (E.agg) {  // (a helper block: through the LDS table)
#pragma unroll
            for (int k = 0; k < 27; ++k) {
                if (u[k] == 0xffffffffu) continue;
                int te = 0x7fffffff;
#pragma unroll
                for (int e = 2; e >= 0; --e)
                    if (k >= st[e]) te = ie[e];
                if (te == 0x7fffffff) continue;
                const int slot = (int)(u[k] & (kCcAggSlots - 1));
                const int t = atomicCAS(&E.agg[slot], -1, (int)u[k]);
                if (t == -1 || t == (int)u[k])
                    atomicMin(&E.agg[kCcAggSlots + slot], te);
                else
                    atomicMin(&E.Tng[u[k]], te);
            }
            continue;
        }
#pragma unroll
        for (int c0 = 0; c0 < 27; c0 += 9) {
            int tn[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) tn[k] = u[c0 + k] != 0xffffffffu ? cc_ld(&E.Tng[u[c0 + k]]) : 0;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                int te = 0x7fffffff;
#pragma unroll
                for (int e = 2; e >= 0; --e)
                    if (c0 + k >= st[e]) te = ie[e];
                if (te < tn[k]) atomicMin(&E.Tng[u[c0 + k]], te);
            }
        }
    }
}

// q of listed node x at its LAST point: the first listed voxel that holds a labelled point by then (0 when the node's own voxel is fully
// labelled or none does: everything it lists joins)
__device__ __noinline__ void cc_exact_q16(const CcExactTabs& E, int x) {
    const int4 c = E.runs[x];
    const int i = E.vpts[c.x + (c.z & 0x7fffffff) - 1];
    int q = -1;
    if (!(cc_exact_time(E, c.y) < i)) {
        uint32_t u[28];
        cc_exact_load_row(E.nbr16, x, u);
#pragma unroll
        for (int c0 = 0; c0 < 27; c0 += 9) {
            int ta[9], pa[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const bool ok = u[c0 + k] != 0xffffffffu;
                const int idx = ok ? (int)u[c0 + k] : c.y;
                ta[k] = cc_exact_time(E, idx);
                pa[k] = E.P1g[idx];
                if (!ok) ta[k] = pa[k] = 0x7fffffff;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k)
                if (q < 0 && min(ta[k], pa[k]) < i) q = c0 + k;
        }
    }
    __hip_atomic_store(&E.qnode[x], max(q, 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (written through: another workgroup reads it in the union pass)
}

// the unions of listed node x: everything from position q of its list on joins it (the rows hold listed numbers)
__device__ __noinline__ void cc_exact_union16(const CcExactTabs& E, int x) {
    const int j = E.La[x];
    const int q = cc_ld(&E.qnode[x]);
    uint32_t u[28];
    cc_exact_load_row(E.nbr16, x, u);
    int nodes[27];
#pragma unroll
    for (int e = 0; e < 27; ++e) nodes[e] = u[e] != 0xffffffffu ? E.La[u[e]] : -1;  // (gathers in flight together)
    int r = j;
    bool any = false;
#pragma unroll
    for (int e = 0; e < 27; ++e) {
        if (nodes[e] < 0) continue;
        any = true;
        if (e >= q) {
            cc_set(E.touched, nodes[e]);
            if (nodes[e] != j) r = cc_union_r(E.parent, r, nodes[e]);  // (from the root the last union returned: its find is a step or two)
        }
    }
    if (any) cc_set(E.found, j);
}

// the row of listed node x: the voxels its triple lists (cc_list27: same voxels, same order as findVoxelNeighbors), as listed numbers.  Written
// THROUGH (agent-scope stores): whoever runs this -- the leader after its first publication, a helper block -- other workgroups read the row
// with plain loads in the passes that follow, and nobody has read it before
__device__ __noinline__ void cc_exact_rows16(const CcExactTabs& E, int x) {
    CcKeys<uint32_t> Kg;
    Kg.k = E.keys;
    Kg.nv = E.nvox;
    Kg.tab = E.tabg;
    Kg.bshift = E.bshift;
    int lst[27];
    const int jj = cc_list27(Kg, E.runs[x].w, E.R, E.S, E.Az, lst);
    uint32_t lv[28];
#pragma unroll
    for (int k = 0; k < 27; ++k) lv[k] = k < jj ? (uint32_t)E.loc[lst[k]] : 0xffffu;  // (the gathers in flight together)
    lv[27] = 0xffffu;
    uint32_t* row = reinterpret_cast<uint32_t*>(const_cast<uint16_t*>(E.nbr16) + (size_t)x * 32);
#pragma unroll
    for (int k = 0; k < 14; ++k) __hip_atomic_store(&row[k], (lv[2 * k] & 0xffffu) | (lv[2 * k + 1] << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&row[14], 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&row[15], 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned long long* cc_help_claim_word(int32_t* slot) { return reinterpret_cast<unsigned long long*>(slot); }

// a helper block of k_cc_scan: takes chunks of the rounds that leaders publish until every scan is past its exact phase
__device__ __forceinline__ void cc_help_loop(const Arena& A, int* bc /* LDS [4] */, int n_leading) {
    int32_t* H = A.cc_help;
    const int tid = threadIdx.x;
    long long t_idle = wall_clock64();  // (the last time this helper had work)
    int rr = blockIdx.x & 63;  // the slot this helper served last (at first: spread over the slots)
    for (;;) {
        if (tid < 64) {  // the first wave looks at 64 slots at a time, one per lane (a look is a round trip to the memory side: one after the other they were the round's latency)
            int got = -1, seq = 0, idx = 0;
            const int cnt = min(__hip_atomic_load(&H[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), kCcHelpSlots);
            for (int k0 = 0; k0 < cnt && got < 0; k0 += 64) {
                const int k = k0 + tid;
                bool open = false;
                int nch = 0;
                if (k < cnt) {
                    int32_t* slot = H + kCcHelpHdr + (size_t)k * kCcHelpSlotWords;
                    const unsigned long long peek = __hip_atomic_load(cc_help_claim_word(slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    nch = __hip_atomic_load(&slot[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    open = (peek >> 32) != 0 && (int)(peek & 0xffffffffu) < nch;  // a phase is published and chunks of it are left
                }
                unsigned long long m = __ballot(open);
                // (start behind the slot this helper served last: helpers spread over the open slots instead of all taking the first)
                const int rot = (rr + 1 - k0) & 63;
                m = rot ? ((m >> rot) | (m << (64 - rot))) : m;
                while (m && got < 0) {
                    const int lane = ((__ffsll((long long)m) - 1) + rot) & 63;
                    m &= m - 1;
                    unsigned long long old = 0;
                    if (tid == lane) {
                        int32_t* slot = H + kCcHelpHdr + (size_t)(k0 + lane) * kCcHelpSlotWords;
                        old = __hip_atomic_fetch_add(cc_help_claim_word(slot), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    old = __shfl(old, lane);
                    const int nl = __shfl(nch, lane);
                    if ((old >> 32) != 0 && (int)(old & 0xffffffffu) < nl) {
                        got = k0 + lane;
                        seq = (int)(old >> 32);
                        idx = (int)(old & 0xffffffffu);
                    }
                }
            }
            if (got < 0) {
                const int passed = __hip_atomic_load(&H[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // (every scan is past its exact phase: nothing will be published any more; or this helper has idled for 20 ms: leaders never depend on it)
                if (passed >= n_leading || wall_clock64() - t_idle > 2000000ll) got = -2;
            }
            if (tid == 0) {
                bc[0] = got;
                bc[1] = seq;
                bc[2] = idx;
            }
        }
        __syncthreads();
        const int got = bc[0], seq = bc[1], idx = bc[2];
        __syncthreads();
        if (got == -2) return;
        if (got < 0) {
            __builtin_amdgcn_s_sleep(16);
            continue;
        }
        rr = got & 63;
        t_idle = wall_clock64();
        // NO agent-scope fence here (round 6, second form): an acquire invalidates the whole L2 of this XCD and a release writes it back,
        // once per chunk and helper that slowed every scan of the batch by a third.  Instead: what never changes after the leader's first
        // publication (rows, run records, first points, the node list: private, 128-byte aligned regions that nobody read earlier in this
        // launch, behind the leader's one release) is read with plain loads; what the leader rewrites between phases (the times, the
        // q's) and the board itself are read and written past the caches (agent-scope atomic accesses), results are atomics.
        int32_t* slot = H + kCcHelpHdr + (size_t)got * kCcHelpSlotWords;
        auto fld = [&](int w) -> void* {
            const unsigned long long lo = (unsigned)__hip_atomic_load(&slot[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long hi = (unsigned)__hip_atomic_load(&slot[w + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return reinterpret_cast<void*>(lo | (hi << 32));
        };
        CcExactTabs E;
        const int na = __hip_atomic_load(&slot[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        E.runs = (const int4*)fld(6);
        E.nbr16 = (const uint16_t*)fld(8);
        E.Tg = (const int*)fld(10);
        E.P1g = (const int*)fld(12);
        E.Tng = (int*)fld(14);
        E.vpts = (const int32_t*)fld(16);
        E.La = (const int*)fld(26);
        E.qnode = (int*)fld(28);
        E.parent = (int*)fld(30);
        E.touched = (int*)fld(32);
        E.found = (int*)fld(34);
        E.keys = (const int*)fld(48);
        E.tabg = (const uint32_t*)fld(50);
        E.loc = (const int*)fld(52);
        E.nvox = __hip_atomic_load(&slot[36], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        E.R = __hip_atomic_load(&slot[37], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        E.S = __hip_atomic_load(&slot[44], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        E.Az = __hip_atomic_load(&slot[45], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        E.bshift = __hip_atomic_load(&slot[46], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        E.remote = true;
        const int x = idx * kCcThreads + tid;
        const int kind = seq & 7;
        E.agg = nullptr;
        if (kind == kCcPhaseRound0 || kind == kCcPhaseRound) {
            E.agg = cc_smem;  // (a helper block has the dynamic LDS of k_cc_scan to itself)
            cc_exact_agg_clear(E.agg, tid);
            __syncthreads();
            if (x < na) cc_exact_tags16(E, x);
            __syncthreads();
            cc_exact_agg_times(E, tid);
            __syncthreads();
            if (x < na) cc_exact_visit16(E, x, kind == kCcPhaseRound0);
            __syncthreads();
            cc_exact_agg_flush(E.agg, E.Tng, tid);
        } else if (x < na) {
            if (kind == kCcPhaseQ)
                cc_exact_q16(E, x);
            else if (kind == kCcPhaseUnion)
                cc_exact_union16(E, x);
            else if (kind == kCcPhaseRows)
                cc_exact_rows16(E, x);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // (every wave: its atomics and written-through stores have left -- no cache is written back)
        __syncthreads();
        if (tid == 0) {
            __hip_atomic_fetch_add(&slot[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicAdd(&A.cc_stats[6], 1);  // chunks done by helpers (development counter)
        }
    }
}

// SHARED (round 6): the instantiation of k_cc_exact -- the exact re-clustering of the components that hold an unsettled irregular run, its
// passes shared with helper blocks.  k_cc_scan's instantiations (SHARED = false) hand such a scan over (cc_again) instead: the code stays
// out of the kernel every scan runs (with it inside, k_cc_scan needed 2.5 KB of scratch per lane instead of 1 KB and ran 12-45 % slower
// on scans that never reach it).
template <bool FAST, bool SHARED = false>
__device__ __forceinline__ bool cc_scan_impl(const DevParams& P, const Arena& A, int from_apri, int* wsum, int* wcnt, int* wlast, int& n_extra_s, int* bad_s, int s,
                                             int base, int n, int nv) {
    PROF_BEGIN();
    const int tid = threadIdx.x;
#ifdef SCVOD_CC_DEVCLK
    const long long t_entry = wall_clock64();
#endif
    if (!FAST) {  // bad_s: [kCcBad] listed points (then their voxels), [kCcBad] = how many there are
        if (tid == 0) bad_s[kCcBad] = 0;
        __syncthreads();
    }
    const int32_t* vbeg = A.vox_pt_begin + base + s;
    const int32_t* vpts = A.vox_pts + base;
    const int32_t* idx3 = A.apri_idx3 + base;
    const int R = P.bin.range_num, S = P.bin.sector_num, Az = P.bin.azimuth_num;
    const long long span = (long long)R * S * Az;
    // A scan is REGULAR when every apri point's index triple lies inside the grid and encodes to its voxel key (no -1 bins:
    // the usual case, the range / FOV verdict keeps such points out of apri_vec).  Then equal keys mean equal triples -- no
    // extra runs --, every voxel finds itself and every neighbour pair is mutual (cc_search_half).  One coalesced pass decides.
    bool bad = !(span > 0 && span < 0x7fffffffLL);
    for (int i0 = 0; i0 < n; i0 += kCcThreads * 4) {
        int tv[4], kv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = min(i0 + u * kCcThreads + tid, n - 1);
            tv[u] = idx3[i];
            kv[u] = from_apri ? A.apri_key[(size_t)base + i] : 0;  // k_emit / k_bin_direct encode the key from the triple themselves
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = tv[u];
            const int ri = (t & 2047) - 2, si = ((t >> 11) & 2047) - 2, ai = ((t >> 22) & 1023) - 2;
            bool b = ri < 0 || ri >= R || si < 0 || si >= S || ai < 0 || ai >= Az;
            if (from_apri) b |= kv[u] != ri * S + si + ai * R * S;
            bad |= b;
            // the generic variant lists the offenders (a handful of returns at polar angle exactly 0 per 128-beam scan): only
            // their voxels can hold a second run or be irregular, so two passes over every slot / node shrink to these voxels
            const int i = i0 + u * kCcThreads + tid;
            if (!FAST && b && i < n) {
                const int x = atomicAdd(&bad_s[kCcBad], 1);
                if (x < kCcBad) bad_s[x] = i;
            }
        }
    }
    const bool allreg = !__syncthreads_or(bad ? 1 : 0);
    if (!allreg && tid == 0) A.scan_irr[s] = 1;  // (the binning kernels' flag is a hint; this is the verdict: the max_name pass reads it)
    const int n_bad = FAST ? 0 : bad_s[kCcBad];
    bool sparse = !FAST && !allreg && span > 0 && span < 0x7fffffffLL && n_bad <= kCcBad;
    const int nw = (n + 31) >> 5;             // words of the per-slot bit arrays
    // storage.  FAST: everything in LDS -- [keys N][parents N][vstart][rstart][prefix][touched][found][bucket index][regular].
    // Generic: nodes (keys, parents, touched / found) in HBM, LDS = [bucket index, 32-bit][vstart][rstart][prefix] for up to
    // kCcSlotsBig points; beyond that the bit arrays move to the arena's per-point scratch (nothing of it is live here).
    const bool slots_lds = FAST || n <= kCcSlotsBig;
    constexpr int kSlotWords = FAST ? kCcSlots / 32 : kCcSlotsBig / 32;
    int* vstart = FAST ? cc_smem + 2 * kCcNodes : (slots_lds ? cc_smem + kCcNodes : A.pt_voxel + base);
    int* rstart = slots_lds ? vstart + kSlotWords : A.tk_members + base;
    int* prefix = slots_lds ? rstart + kSlotWords : A.tk_clusters + base;
    int* extras = A.tk_uniq + base;            // slots of the extra run openers (rare: global scratch in both modes)
    int* extra_of_slot = A.tk_mbegin + base;   // slot -> index in extras
    if (tid == 0) n_extra_s = 0;
    for (int w = tid; w < nw; w += kCcThreads) {
        vstart[w] = 0;
        rstart[w] = 0;
    }
    __syncthreads();
    for (int v = tid; v < nv; v += kCcThreads) {
        const int k = vbeg[v];
        cc_set(vstart, k);
        if (!allreg) cc_set(rstart, k);
    }
    __syncthreads();
    CC_MARK(0);
    // runs inside a voxel: a slot whose triple differs from the previous slot's opens one (ssc.cpp:306-330 walks the
    // voxel's points with their own triples; equal triples have equal neighbourhoods)
    if (sparse) {
        const int* vkey = A.vox_key + base;
        bool fail = false;
        for (int x = tid; x < n_bad; x += kCcThreads) {
            const int i = bad_s[x];
            const int key = A.apri_key[(size_t)base + i];
            const int v = cc_lower_bound(vkey, nv, key);
            if (v >= nv || vkey[v] != key || vbeg[v + 1] - vbeg[v] > kCcBadVoxel) {
                fail = true;
                continue;
            }
            bad_s[x] = v;  // (from here on: the voxel)
            int t_prev = idx3[vpts[vbeg[v]]];
            for (int k = vbeg[v] + 1; k < vbeg[v + 1]; ++k) {
                const int t = idx3[vpts[k]];
                if (t != t_prev && !((atomicOr(&rstart[k >> 5], 1 << (k & 31)) >> (k & 31)) & 1)) {  // (two listed points of one voxel)
                    const int e = atomicAdd(&n_extra_s, 1);
                    extras[e] = k;
                    extra_of_slot[k] = e;
                }
                t_prev = t;
            }
        }
        if (__syncthreads_or(fail ? 1 : 0)) sparse = false;  // (what was found stays: the pass below skips the slots that are marked)
    }
    if (!allreg && !sparse) {
        for (int k0 = 0; k0 < n; k0 += kCcThreads * 4) {
            int pa[4], pb[4], ta[4], tb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // the two dependent gathers of four slots in flight together
                const int k = min(k0 + u * kCcThreads + tid, n - 1);
                pa[u] = vpts[k];
                pb[u] = vpts[max(k - 1, 0)];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                ta[u] = idx3[pa[u]];
                tb[u] = idx3[pb[u]];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + u * kCcThreads + tid;
                if (k >= n || cc_bit(vstart, k)) continue;
                if (ta[u] != tb[u] && !((atomicOr(&rstart[k >> 5], 1 << (k & 31)) >> (k & 31)) & 1)) {
                    const int e = atomicAdd(&n_extra_s, 1);
                    extras[e] = k;
                    extra_of_slot[k] = e;
                }
            }
        }
    }
    CC_MARK(1);
    // prefix[w] = voxel starts in the words before w: voxel of slot k = prefix[k >> 5] + popc(vstart word up to k) - 1
    {
        int run = 0;
        for (int w0 = 0; w0 < nw; w0 += kCcThreads) {
            const int w = w0 + tid;
            const int c = (w < nw) ? __popc((unsigned)vstart[w]) : 0;
            int total;
            const int ex = block_excl_scan<kCcThreads>(c, total, wsum);
            if (w < nw) prefix[w] = run + ex;
            run += total;
        }
    }
    __syncthreads();
    const int n_extra = n_extra_s;
    const int nn = nv + n_extra;
    if (FAST && nn > kCcNodes) return false;
    int* lkeys = cc_smem;  // FAST only
    int* parent = FAST ? cc_smem + kCcNodes : A.cc_parent + base;
    int* touched = FAST ? cc_smem + 2 * kCcNodes + 3 * (kCcSlots / 32) : A.tk_npairs + base;
    int* found = FAST ? touched + kCcNodes / 32 : A.tk_hit + base;
    using TabT = typename std::conditional<FAST, uint16_t, uint32_t>::type;
    constexpr int kTabEntries = FAST ? kCcBuckets : kCcNodes;
    TabT* tab = FAST ? (TabT*)(cc_smem + 2 * kCcNodes + 3 * (kCcSlots / 32) + 2 * (kCcNodes / 32)) : (TabT*)cc_smem;
    CcKeys<TabT> K;
    K.nv = nv;
    K.k = FAST ? lkeys : A.vox_key + base;
    K.tab = tab;
    K.bshift = 0;
    const int kspan = (span > 0 && span < 0x7fffffffLL) ? (int)span : 0x7ffffffe;  // (an overflowing grid: all int keys searchable)
    while (((kspan - 1) >> K.bshift) + 2 > kTabEntries) ++K.bshift;
    const int nb = ((kspan - 1) >> K.bshift) + 1;
    if (FAST)
        for (int v = tid; v < nv; v += kCcThreads) lkeys[v] = A.vox_key[(size_t)base + v];
    __syncthreads();
    if (FAST) {
        for (int b = tid; b <= nb; b += kCcThreads) tab[b] = (TabT)cc_lower_bound(lkeys, nv, (int)min((long long)b << K.bshift, 0x7fffffffLL));
    } else {
        // keys in HBM: the nodes fill the table -- node v owns the buckets after its predecessor's up to its own
        auto bucket_of = [&](int key) -> int { return key < 0 ? -1 : min(key >> K.bshift, nb); };
        for (int v = tid; v < nv; v += kCcThreads) {
            const int bc = bucket_of(K.k[v]);
            const int bp = (v > 0) ? bucket_of(K.k[v - 1]) : -1;
            for (int b = bp + 1; b <= bc; ++b) tab[b] = (TabT)v;
            if (v == nv - 1)
                for (int b = bc + 1; b <= nb; ++b) tab[b] = (TabT)nv;
        }
    }
    __syncthreads();
    CC_MARK(2);
    auto voxel_of_slot = [&](int k) -> int {
        const unsigned m = (unsigned)vstart[k >> 5] & (0xffffffffu >> (31 - (k & 31)));
        return prefix[k >> 5] + __popc(m) - 1;
    };
    // the run that starts a voxel is node v, an extra run is node nv + e
    // parents in HBM (generic variant): runs linked up front and the head rule, so that few unions with short finds remain;
    // parents in LDS: plain forest, every neighbour pair joined (measured: the rule costs more than LDS unions save)
    int* heads = FAST ? nullptr : A.cl_count + base;  // [nv bits]
    if (FAST) {
        for (int j = tid; j < nn; j += kCcThreads) parent[j] = j;
        __syncthreads();
    }
    // generic variant: the bit arrays of the slots leave the LDS for the search (they are not read by it) and the regular
    // nodes are joined window by window on LDS copies of their keys and parents (cc_search_windows)
    constexpr int kWinWords = (int)(kCcLdsBytes / 4) - kCcNodes - 64;
    int* spill[3] = {A.pt_voxel + base, A.tk_members + base, A.tk_clusters + base};
    auto windows = [&](const int* regular) -> bool {
        if (FAST || kspan != (int)span) return false;
        if (slots_lds) {
            for (int w = tid; w < nw; w += kCcThreads) {
                spill[0][w] = vstart[w];
                spill[1][w] = rstart[w];
                spill[2][w] = prefix[w];
            }
            __syncthreads();
        }
        const bool done = cc_search_windows(K, parent, regular, nn, R, S, Az, cc_smem + kCcNodes, kWinWords, wlast CCW_PROF_ARG);
        if (slots_lds) {
            __syncthreads();
            for (int w = tid; w < nw; w += kCcThreads) {
                vstart[w] = spill[0][w];
                rstart[w] = spill[1][w];
                prefix[w] = spill[2][w];
            }
            __syncthreads();
        }
        return done;
    };
    if (allreg) {
        const bool windowed = windows(nullptr);
        if (!FAST && !windowed && tid == 0) atomicAdd(&A.cc_stats[3], 1);  // planes too large for a window: forest in HBM
        if (!FAST && !windowed) {
            cc_link_runs(K.k, nv, nn, S, (const int*)nullptr, heads, parent, wlast);
            __syncthreads();
        }
        if (FAST) {  // runs linked in LDS, their head bits in the (unused: every voxel is touched) touched words
            cc_link_runs_lds(lkeys, nv, S, (const int*)nullptr, touched, parent, 0);
            __syncthreads();
        }
        const int RS = R * S;
        int k_next = K.k[min(tid, nv - 1)];
        for (int j = tid; j < nv && !windowed; j += kCcThreads) {
            const int key = k_next;
            k_next = K.k[min(j + kCcThreads, nv - 1)];
            const int ai = key / RS, rem = key - ai * RS;  // the triple IS the key's decomposition
            const int ri = rem / S, si = rem - ri * S;
            if (FAST)
                cc_search_half<true>(K, parent, touched, j, ri, si, ai, R, S, Az);
            else
                cc_search_half(K, parent, heads, j, ri, si, ai, R, S, Az);
        }
    } else if (FAST && n <= 65535) {
        // ---- a scan with index triples outside the grid, all tables in LDS: the visiting order of clusterAndCreateFrame
        // (ssc.cpp:303-350) decides which of the asymmetric "finds" stick, so it is modelled exactly (DESIGN.md section 2).
        // The loop reduces to a voxel-level state machine: a point is labelled once it was visited or once its voxel became
        // FULLY labelled at time T(k).  Visiting point i of voxel v with the listed voxels k1 .. km: if T(v) < i every kj joins
        // i and becomes fully labelled; otherwise with q = the first kj holding a labelled point (T(kj) < i or its first point
        // < i) the voxels kq .. km join i (kq becomes fully labelled only through a visited first point), the ones before q are
        // left alone; without any q all of them join.  T is well-founded in visiting order: Jacobi sweeps over all points
        // reach its fixed point in a handful of rounds; then one pass takes q per point and one pass does the unions.
        uint16_t* T16 = (uint16_t*)(cc_smem + kCcNodes);  // [nv] (the parents' LDS until the unions start), 0xffff = never
        uint16_t* P1 = T16 + kCcNodes;                    // [nv] first point of every voxel
        for (int v = tid; v < nv; v += kCcThreads) {
            T16[v] = 0xffffu;
            P1[v] = (uint16_t)vpts[vbeg[v]];
        }
        __syncthreads();
        auto labelled_voxel = [&](int u, int i) -> bool { return T16[u] != 0xffffu && (int)T16[u] < i; };
        // Work goes by RUN (node): the points of a run share their list.  Of a regular run (triple in the grid, encoding to the
        // voxel's key: its own voxel is in its list) only the first three points are events -- the second visit at the latest
        // labels the voxel fully, the third labels the whole list, later ones change nothing; an irregular run visits with
        // every point.  Up to three events share one walk over the list (their q's are found together).
        struct Run {
            int o, v, len;
            int32_t t;
            bool regular;
        };
        auto run_of_node = [&](int j) -> Run {
            Run r;
            r.o = (j < nv) ? vbeg[j] : extras[j - nv];
            r.v = (j < nv) ? j : voxel_of_slot(r.o);
            int w = (r.o + 1) >> 5;
            unsigned m = (w < nw) ? ((unsigned)rstart[w] & ~((1u << ((r.o + 1) & 31)) - 1u)) : 0u;
            while (!m && ++w < nw) m = (unsigned)rstart[w];
            r.len = (m ? min((w << 5) + __ffs((int)m) - 1, n) : n) - r.o;
            r.t = idx3[vpts[r.o]];
            const int ri = (r.t & 2047) - 2, si = ((r.t >> 11) & 2047) - 2, ai = ((r.t >> 22) & 1023) - 2;
            r.regular = kspan == (int)span && ri >= 0 && ri < R && si >= 0 && si < S && ai >= 0 && ai < Az && (ri * S + si + ai * R * S == K.k[r.v]);
            return r;
        };
        // the listed voxels of every node, looked up once: 27 uint16 per node in the box scratch of the scan (free until the
        // boxes are built) when it is large enough -- the rounds then walk the table instead of repeating 27 searches
        // (rows of 32 entries = 64 bytes, 16-byte aligned: a row is four wide loads in flight, then registers)
        uint16_t* nbr = (uint16_t*)(((uintptr_t)(A.cl_bbox + 7 * (size_t)base) + 15) & ~(uintptr_t)15);
        const bool tabled = (size_t)nn * 64 + 16 <= (size_t)n * 7 * sizeof(float);
        if (tabled) {
            for (int j = tid; j < nn; j += kCcThreads) {
                const int o = (j < nv) ? vbeg[j] : extras[j - nv];
                uint16_t* row = nbr + (size_t)j * 32;
                int jj = 0;
                cc_for_each_listed(K, idx3[vpts[o]], R, S, Az, [&](int u) -> bool {
                    row[jj++] = (uint16_t)u;
                    return true;
                });
                for (; jj < 32; ++jj) row[jj] = 0xffffu;
            }
            __syncthreads();
        }
        CC_MARK(10);
        auto walk = [&](int j, int32_t t, auto f) {  // f(u) in list order; false stops
            if (tabled) {
                const uint4* row = reinterpret_cast<const uint4*>(nbr + (size_t)j * 32);
                const uint4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
                const unsigned w[16] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
#pragma unroll
                for (int e = 0; e < 27; ++e) {
                    const int u = (int)((w[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
                    if (u == 0xffff || !f(u)) return;
                }
            } else {
                cc_for_each_listed(K, t, R, S, Az, f);
            }
        };
        // what a round needs of a run, gathered once (arena scratch): opener slot, voxel, length (bit 31: regular), triple
        int4* runs = (int4*)A.tk_pairs + ((size_t)base + 1) / 2;  // [nn] (16-byte aligned inside the scan's 8 n bytes; nn <= n / 2 ... checked)
        const bool runs_cached = (size_t)nn * 2 + 2 <= (size_t)n;
        if (runs_cached) {
            for (int j = tid; j < nn; j += kCcThreads) {
                const Run r = run_of_node(j);
                runs[j] = make_int4(r.o, r.v, r.len | (r.regular ? (int)0x80000000u : 0), r.t);
            }
            __syncthreads();
        }
        auto cached_run = [&](int j) -> Run {
            if (!runs_cached) return run_of_node(j);
            const int4 c = runs[j];
            Run r;
            r.o = c.x;
            r.v = c.y;
            r.len = c.z & 0x7fffffff;
            r.regular = c.z < 0;
            r.t = c.w;
            return r;
        };
        // the next round's times: in the key table's LDS once the lists are tabled (no search needs the keys any more)
        int* Tn = tabled && runs_cached ? lkeys : A.cc_parent + base;  // [nv]
        for (int round = 0; round < 1024; ++round) {  // (about seven in practice; the fixed point exists after at most one round per visit)
            for (int v = tid; v < nv; v += kCcThreads) Tn[v] = 0x7fffffff;
            __syncthreads();
            for (int j = tid; j < nn; j += kCcThreads) {
                const Run r = cached_run(j);
                const int nev = r.regular ? min(r.len, 3) : r.len;
                for (int p0 = 0; p0 < nev; p0 += 3) {
                    int ie[3], qe[3];
                    bool cs[3];
#pragma unroll
                    for (int e = 0; e < 3; ++e) {
                        ie[e] = (p0 + e < nev) ? vpts[r.o + p0 + e] : 0x7fffffff;  // (an absent event never sets anything)
                        // round 0 starts the iteration from the optimistic end (every visit labels its whole list): any start
                        // reaches the same fixed point, this one in fewer rounds than "nothing is ever labelled"
                        cs[e] = p0 + e < nev && (round == 0 || labelled_voxel(r.v, ie[e]));
                        qe[e] = -1;
                    }
                    int jj = 0;
                    walk(j, r.t, [&](int u) -> bool {
                        const int p1 = P1[u];
#pragma unroll
                        for (int e = 0; e < 3; ++e)
                            if (qe[e] < 0 && ie[e] != 0x7fffffff && (labelled_voxel(u, ie[e]) || p1 < ie[e])) qe[e] = jj;
                        ++jj;
                        return true;
                    });
                    jj = 0;
                    walk(j, r.t, [&](int u) -> bool {
                        const int p1 = P1[u];
                        int te = 0x7fffffff;  // the earliest of the events that labels u fully
#pragma unroll
                        for (int e = 2; e >= 0; --e)
                            if (ie[e] != 0x7fffffff && (cs[e] || qe[e] < 0 || jj > qe[e] || (jj == qe[e] && p1 < ie[e]))) te = ie[e];
                        if (te != 0x7fffffff && te < cc_ld(&Tn[u])) atomicMin(&Tn[u], te);
                        ++jj;
                        return true;
                    });
                }
            }
            __syncthreads();
            bool changed = false;
            for (int v = tid; v < nv; v += kCcThreads) {
                const int tv = cc_ld(&Tn[v]);  // (written by atomics: read past the L1)
                const uint16_t t16 = tv == 0x7fffffff ? (uint16_t)0xffffu : (uint16_t)tv;
                changed |= t16 != T16[v];
                T16[v] = t16;
            }
            CC_MARK(13);
#ifdef SCVOD_PROFILE
            if (tid == 0) atomicAdd(&g_prof[0][14], 100ull);  // rounds x 100 (prints as "us": 1.0 per round and scan)
#endif
            if (!__syncthreads_or(changed ? 1 : 0)) break;
        }
        CC_MARK(11);
        // the unions: what a run's LAST point joins contains what its earlier points joined (q only moves forward in time)
        int* qnode = A.cc_parent + base;  // [nn] q of every node
        for (int j = tid; j < nn; j += kCcThreads) {
            const Run r = cached_run(j);
            const int i = vpts[r.o + r.len - 1];
            int q = -1, jj = 0;
            if (!labelled_voxel(r.v, i))
                walk(j, r.t, [&](int u) -> bool {
                    if (labelled_voxel(u, i) || (int)P1[u] < i) {
                        q = jj;
                        return false;
                    }
                    ++jj;
                    return true;
                });
            qnode[j] = max(q, 0);
        }
        __syncthreads();
        for (int j = tid; j < nn; j += kCcThreads) parent[j] = j;  // (T16 / P1 are used up)
        for (int w = tid; w < ((nn + 31) >> 5); w += kCcThreads) {
            touched[w] = 0;
            found[w] = 0;
        }
        __syncthreads();
        for (int j = tid; j < nn; j += kCcThreads) {
            const int o = (j < nv) ? vbeg[j] : extras[j - nv];
            const int q = qnode[j];
            int jj = 0;
            walk(j, idx3[vpts[o]], [&](int u) -> bool {
                if (jj >= q) {
                    cc_set(touched, u);  // all of u's points join
                    if (u != j) cc_union(parent, j, u);
                }
                ++jj;
                return true;
            });
            if (jj > 0) cc_set(found, j);
        }
        CC_MARK(12);
    } else {
        int* regular = FAST ? cc_smem + 2 * kCcNodes + 3 * (kCcSlots / 32) + 2 * (kCcNodes / 32) + kCcBuckets / 2 : A.pt_cluster + base;
        int* triple = (int*)(A.tk_pairs + base);  // [nn] opener triples (arena scratch, free until the naming pass)
        const int nwords = (nn + 31) >> 5;
        constexpr int kG = FAST ? 4 : 8;
        if (sparse) {
            // every voxel is regular except the listed ones whose OPENER is outside the grid (or does not encode to the key);
            // only irregular nodes need their triple (a regular one's is its key's decomposition: triple_of)
            for (int w = tid; w < nwords; w += kCcThreads) {
                const int c = min(max(nv - (w << 5), 0), 32);
                const int word = c >= 32 ? -1 : (int)((1u << c) - 1u);
                regular[w] = word;
                touched[w] = word;  // a regular voxel finds itself
                found[w] = word;
            }
            __syncthreads();
            for (int x = tid; x < n_bad; x += kCcThreads) {
                const int v = bad_s[x];
                const int t = idx3[vpts[vbeg[v]]];
                const int ri = (t & 2047) - 2, si = ((t >> 11) & 2047) - 2, ai = ((t >> 22) & 1023) - 2;
                const bool reg = ri >= 0 && ri < R && si >= 0 && si < S && ai >= 0 && ai < Az && (ri * S + si + ai * R * S == K.k[v]);
                if (!reg) {
                    const int m = ~(1 << (v & 31));
                    atomicAnd(&regular[v >> 5], m);
                    atomicAnd(&touched[v >> 5], m);
                    atomicAnd(&found[v >> 5], m);
                    triple[v] = t;
                }
            }
            for (int e = tid; e < n_extra; e += kCcThreads) triple[nv + e] = idx3[vpts[extras[e]]];
        }
        for (int j0 = 0; j0 < nn && !sparse; j0 += kCcThreads * kG) {  // the three dependent gathers of kG nodes per thread in flight together
            int tc[kG];
#pragma unroll
            for (int u = 0; u < kG; ++u) {
                const int j = j0 + u * kCcThreads + tid;
                tc[u] = (j < nn) ? ((j < nv) ? vbeg[j] : extras[j - nv]) : 0;
            }
#pragma unroll
            for (int u = 0; u < kG; ++u) tc[u] = vpts[tc[u]];
#pragma unroll
            for (int u = 0; u < kG; ++u) tc[u] = idx3[tc[u]];
#pragma unroll
            for (int u = 0; u < kG; ++u) {
                const int j = j0 + u * kCcThreads + tid;
                const int t = tc[u];
                const int ri = (t & 2047) - 2, si = ((t >> 11) & 2047) - 2, ai = ((t >> 22) & 1023) - 2;
                const bool reg = kspan == (int)span && j < nv && ri >= 0 && ri < R && si >= 0 && si < S && ai >= 0 && ai < Az && (ri * S + si + ai * R * S == K.k[min(j, nv - 1)]);
                const unsigned long long b = __ballot(reg);
                if ((tid & 31) == 0 && (j >> 5) < nwords) {
                    const int word = (int)(unsigned)((tid & 32) ? (b >> 32) : b);
                    regular[j >> 5] = word;
                    touched[j >> 5] = word;  // a regular voxel finds itself
                    found[j >> 5] = word;
                }
                if (j < nn) triple[j] = t;
            }
        }
        __syncthreads();
        CCW_MARK(0);
        const bool windowed = windows(regular);
        if (!FAST && !windowed && tid == 0) atomicAdd(&A.cc_stats[3], 1);
        if (!FAST && !windowed) {
            cc_link_runs(K.k, nv, nn, S, regular, heads, parent, wlast);
            __syncthreads();
        }
        if (windowed) {
            // the regular nodes are done: only the irregular ones (a handful per scan) search, straight from the bit words
            // listed, then one WAVE per node: the nine (azimuth, range) rows around its triple on lanes 0-8 (cc_search), the nine
            // around its key's own triple on lanes 16-24 (cc_search_canon) -- a thread alone walks 18 searches in HBM one
            // after the other
            int* irr = heads;  // [nn] (the run heads are not used by the windowed search)
            if (tid == 0) wlast[8] = 0;
            __syncthreads();
            for (int w = tid; w < nwords; w += kCcThreads) {
                unsigned m = ~(unsigned)regular[w];
                if (w == nwords - 1 && (nn & 31)) m &= (1u << (nn & 31)) - 1u;
                while (m) {
                    irr[atomicAdd(&wlast[8], 1)] = (w << 5) + __ffs((int)m) - 1;
                    m &= m - 1;
                }
            }
            __syncthreads();
            const int n_irr = wlast[8], lane = tid & 63, RS = R * S;
            for (int x = tid >> 6; x < n_irr; x += kCcThreads / 64) {
                const int j = cc_ld(&irr[x]);
                const int q = lane & 15, canon = lane >> 4;  // canon: 0 = around the triple, 1 = around the key's triple
                int ri, si, ai;
                bool on = q < 9 && canon < 2;
                if (canon == 0) {
                    const int t = triple[j];
                    ri = (t & 2047) - 2, si = ((t >> 11) & 2047) - 2, ai = ((t >> 22) & 1023) - 2;
                } else {
                    const int key = (j < nv) ? K.k[j] : -1;
                    on = on && key >= 0 && key < kspan;
                    ai = key / RS;
                    const int rem = key - ai * RS;
                    ri = rem / S, si = rem - ri * S;
                }
                const int z = ai - 1 + q / 3, xx = ri - 1 + q % 3;
                const int ylo = max(si - 1, 0), yhi = min(si + 1, S - 1);
                on = on && ylo <= yhi && z >= 0 && z <= Az - 1 && xx >= 0 && xx <= R - 1;
                bool hit = false;
                if (on) {
                    const int k0 = xx * S + ylo + z * RS, k1 = k0 + (yhi - ylo);
                    for (int u = cc_lower_bound2(K, k0); u < K.nv && K.k[u] <= k1; ++u) {
                        if (canon == 0) {
                            cc_set(touched, u);  // every point of u joins (ssc.cpp:316)
                            if (u != j) cc_union(parent, j, u);
                            hit = true;
                        } else if (u != j && cc_bit(regular, u)) {
                            cc_set(touched, j);  // the regular voxel u finds me here (ssc.cpp:316)
                            cc_union(parent, j, u);
                        }
                    }
                }
                if (__any(hit) && lane == 0) cc_set(found, j);
            }
        }
        for (int j = tid; j < nn && !windowed; j += kCcThreads) {
            if (cc_bit(regular, j)) {
                const int RS = R * S, key = K.k[j];  // (a regular node's triple is its key's decomposition)
                const int ai = key / RS, rem = key - ai * RS;
                cc_search_half(K, parent, heads, j, rem / S, rem % S, ai, R, S, Az);
            } else {
                const int t = triple[j];
                if (cc_search(K, parent, touched, j, t, R, S, Az)) cc_set(found, j);
                if (j < nv) {
                    const int key = K.k[j];
                    if (key >= 0 && key < kspan) cc_search_canon(K, parent, touched, regular, j, key, R, S, Az);
                }
            }
        }
    }
    __syncthreads();
    CC_MARK(3);
    // every point of a touched voxel is merged with the voxel (ssc.cpp:316-345): the extra runs inside one join it
    for (int e = tid; e < n_extra; e += kCcThreads) {
        const int v = voxel_of_slot(extras[e]);
        if (cc_bit(touched, v)) cc_union(parent, nv + e, v);
    }
    __syncthreads();
    if (!FAST) CCW_MARK(6);
    if (!FAST && !allreg && slots_lds && kspan == (int)span) {
        // ---- generic variant, scan with irregular triples: what stands now is "everything found is joined".  The visiting
        // order (the model of the all-in-LDS variant above, DESIGN.md section 2) can only SPLIT components that hold an
        // irregular run, and its state machine never looks outside such a component (a listed voxel is in the lister's
        // component; a voxel's labelling time depends on its finders only): those components are clustered again, exactly,
        // with the times / first points / next times of their voxels in arena scratch.
        int* regular = A.pt_cluster + base;
        const int* triple = (const int*)(A.tk_pairs + base);  // [nn] opener triples (written by the search above: the irregular nodes' at least)
        auto triple_of = [&](int j) -> int32_t {
            if (j >= nv || !cc_bit(regular, j)) return triple[j];
            const int RS = R * S, key = K.k[j];
            const int ai = key / RS, rem = key - ai * RS;
            return (int32_t)((rem / S + 2) | ((rem % S + 2) << 11) | ((ai + 2) << 22));
        };
        int* aff = A.tk_members + base;                       // [nn] root flag: the component holds an irregular run
        // (regions that helper blocks read start on a 128-byte line of their own: nothing another scan's workgroup touches shares a line with them)
        const int base_al = (base + 31) & ~31;
        const bool al_ok = !FAST && nn + 64 <= n;
        int* La = A.tk_clusters + (al_ok ? base_al : base);   // [na] the nodes of those components
        int* Tg = A.cl_count + base;                          // [nv] labelling times (run heads are used up)
        int* P1g = A.tk_nuniq + base;                         // [nv] first point of a voxel
        int* Tng = A.tk_cursor + base;                        // [nv] next round's times, then [na] q per listed node
        for (int j = tid; j < nn; j += kCcThreads) aff[j] = 0;
        if (tid == 0) wlast[8] = 0;
        __syncthreads();
        int* irrl = Tng;  // [n_irr] (free until the rounds)
        for (int w = tid; w < ((nn + 31) >> 5); w += kCcThreads) {  // the irregular nodes, straight from the bit words (extra runs have no bit set)
            unsigned m = ~(unsigned)regular[w];
            if (w == ((nn + 31) >> 5) - 1 && (nn & 31)) m &= (1u << (nn & 31)) - 1u;
            while (m) {
                irrl[atomicAdd(&wlast[8], 1)] = (w << 5) + __ffs((int)m) - 1;
                m &= m - 1;
            }
        }
        __syncthreads();
        bool any_left = true;
        if constexpr (!FAST) {
            // most of them change nothing (cc_run_is_plain: settled by the cells around the run); only the components of the
            // others are clustered again.  A.cc_plain_rule == 0 (scvod_set_cluster_exact(ctx, 2): tests) skips the rule.
            CcRunRule Q;
            Q.K = K;
            Q.vbeg = vbeg;
            Q.vpts = vpts;
            Q.idx3 = idx3;
            Q.triple = triple;
            Q.irrl = irrl;
            Q.extras = extras;
            Q.vstart = vstart;
            Q.prefix = prefix;
            Q.nv = nv;
            Q.n_irr = wlast[8];
            Q.R = R;
            Q.S = S;
            Q.Az = Az;
            Q.kspan = kspan;
            int settled = 0;
            for (int x = tid >> 6; x < Q.n_irr; x += kCcThreads / 64) {
                const int j = cc_ld(&irrl[x]);
                if (A.cc_plain_rule && cc_run_is_plain(Q, j, tid & 63))
                    ++settled;
                else if ((tid & 63) == 0) {
                    aff[cc_find(parent, j)] = 1;
                    if constexpr (!SHARED) atomicAdd(&A.cc_stats[5], 1);  // (k_cc_exact evaluates the rule again for the scans handed over: counted once)
                }
            }
            if constexpr (!SHARED)
                if ((tid & 63) == 0 && settled) atomicAdd(&A.cc_stats[4], settled);
            any_left = settled < (Q.n_irr - (tid >> 6) + kCcThreads / 64 - 1) / (kCcThreads / 64);  // (wave-uniform: this wave left a run unsettled)
        }
        any_left = __syncthreads_or(any_left ? 1 : 0);
        if constexpr (!SHARED) {
            // a run the rule does not settle: the scan is clustered again by k_cc_exact, from scratch (nothing it needs was changed here)
            if (any_left) {
                if (tid == 0) A.cc_again[1 + atomicAdd(&A.cc_again[0], 1)] = s;
                return true;
            }
        }
        if constexpr (SHARED) {
#ifdef SCVOD_CC_DEVCLK
        const long long t_rule = wall_clock64();  // (development clocks of the help board)
#endif
        // closure: the state machine of an affected component reads the labelling time of the HOME voxel of each of its irregular
        // runs (a visitor whose voxel is fully labelled joins all it lists), and a run that nobody has merged with its home voxel
        // sits in another component than that voxel: that component is clustered again as well, and so on
        if (any_left) {
            const int n_irr = wlast[8];
            for (int it = 0; it < 64; ++it) {
                bool changed = false;
                for (int x = tid; x < n_irr; x += kCcThreads) {
                    const int j = cc_ld(&irrl[x]);
                    if (j < nv) continue;  // (the run that opens a voxel IS its home voxel's node)
                    const int v = voxel_of_slot(extras[j - nv]);
                    const int rj = cc_find(parent, j), rv = cc_find(parent, v);
                    if (rj != rv && cc_ld(&aff[rj]) != 0 && cc_ld(&aff[rv]) == 0) {
                        aff[rv] = 1;
                        changed = true;
                    }
                }
                if (!__syncthreads_or(changed ? 1 : 0)) break;
            }
        }
        // (a sample of every eighth node first: components far beyond the bound are not even listed -- when there is a bound)
        int sampled = 0;
        const int exact_max = A.cc_exact_max;
        const bool bounded = exact_max < 0x3fffffff;
        for (int j0 = 0; j0 < nn && any_left && bounded; j0 += kCcThreads * 8) {
            const int j = j0 + tid * 8;
            sampled += __syncthreads_count(j < nn && aff[cc_find(parent, j)] != 0);
        }
        int na = 0;
        const bool listed = !bounded || (long long)sampled * 8 <= 2ll * exact_max;
        if (listed && any_left) {
            // the nodes of the affected components in ascending order.  Their roots first, four walks per thread in flight together (read-only:
            // 75 k dependent walks one at a time were most of the 2 ms this took on a 128-beam scan), kept in scratch that is free until the
            // tables are built; then the places by block scans as before
            int* rootj = P1g;  // [nn]
            for (int j0 = 0; j0 < nn; j0 += kCcThreads * 4) {
                int rr[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u * kCcThreads + tid;
                    rr[u] = j < nn ? cc_ld(&parent[j]) : 0;
                }
                for (int hop = 0; hop < 4096; ++hop) {  // (bounded: a forest's walk ends at a root long before)
                    int pp[4];
                    bool more = false;
#pragma unroll
                    for (int u = 0; u < 4; ++u) pp[u] = cc_ld(&parent[rr[u]]);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (pp[u] != rr[u]) {
                            rr[u] = pp[u];
                            more = true;
                        }
                    if (!more) break;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u * kCcThreads + tid;
                    if (j < nn) rootj[j] = rr[u];
                }
            }
            __syncthreads();
            for (int j0 = 0; j0 < nn; j0 += kCcThreads) {
                const int j = j0 + tid;
                const bool a = j < nn && aff[rootj[j]] != 0;
                int total;
                const int ex = block_excl_scan<kCcThreads>(a ? 1 : 0, total, wsum);
                if (a) La[na + ex] = j;
                na += total;
            }
        }
        __syncthreads();
        // (components of tens of thousands of nodes -- an irregular return on a facade of a 128-beam scan -- are left as they
        // are: the rounds would cost milliseconds in HBM, and around such a point every voxel has finders with three or
        // more points, whose third visit joins all they list; DESIGN.md section 2)
        if (tid == 0 && ((!listed && sampled > 0) || na > exact_max || (na > 0 && n_extra + na > n))) {
            // this scan keeps "everything found is joined" for its affected components (reported: scvod_batch_cluster_stats)
            atomicAdd(&A.cc_stats[0], 1);
            atomicAdd(&A.cc_stats[1], listed ? na : sampled * 8);
        }
        CCW_MARK(8);
#ifdef SCVOD_CC_DEVCLK
        const long long t_list = wall_clock64();
#endif
        if (na > 0 && na <= exact_max) {
            struct Run {
                int o, v, len;
                int32_t t;
                bool regular;
            };
            auto run_of_node = [&](int j) -> Run {
                Run r;
                r.o = (j < nv) ? vbeg[j] : extras[j - nv];
                r.v = (j < nv) ? j : voxel_of_slot(r.o);
                int w = (r.o + 1) >> 5;
                unsigned m = (w < nw) ? ((unsigned)rstart[w] & ~((1u << ((r.o + 1) & 31)) - 1u)) : 0u;
                while (!m && ++w < nw) m = (unsigned)rstart[w];
                r.len = (m ? min((w << 5) + __ffs((int)m) - 1, n) : n) - r.o;
                r.t = triple_of(j);
                const int ri = (r.t & 2047) - 2, si = ((r.t >> 11) & 2047) - 2, ai = ((r.t >> 22) & 1023) - 2;
                r.regular = ri >= 0 && ri < R && si >= 0 && si < S && ai >= 0 && ai < Az && (ri * S + si + ai * R * S == K.k[r.v]);
                return r;
            };
            // run records + the listed voxels of every affected node (32-bit rows of 32) in the scan's box scratch when it fits
            char* scratch = (char*)(((uintptr_t)(A.cl_bbox + 7 * (size_t)base) + 127) & ~(uintptr_t)127);
            // (16-bit rows of 32 = 64 bytes: the LISTED nodes are numbered 0 .. na-1 -- round 6; voxel numbers until round 5, which a 128-beam
            // scan of 72 k voxels does not fit -- and the tables of the rounds are indexed by these numbers: a listed voxel belongs to the
            // lister's component, and the home voxel of an extra run to the closure above, so every voxel a row or a run names is listed)
            const bool q_fits = n_extra + na <= n;
            const bool rows16 = q_fits && al_ok && n_extra + na + 64 <= n && na <= 0xfffe && (size_t)na * (16 + 64) + ((size_t)nb + 2) * 4 + 512 <= (size_t)n * 7 * sizeof(float);
            const bool tabled = rows16 || (size_t)na * (16 + 128) + 256 <= (size_t)n * 7 * sizeof(float);
            int4* runs = (int4*)scratch;
            uint32_t* nbr = (uint32_t*)(scratch + (size_t)na * 16);
            uint16_t* nbr16 = (uint16_t*)nbr;
            int* loc = A.cl_count + base_al;             // rows16: [nv] voxel -> its number in La
            uint32_t* tabg = (uint32_t*)(((uintptr_t)(scratch + (size_t)na * (16 + 64)) + 127) & ~(uintptr_t)127);  // rows16: [nb + 1] copy of the bucket index for the helper blocks
            int* Tc = A.tk_nuniq + base_al;              // rows16: [na] labelling times by listed number
            int* P1c = A.tk_cursor + base_al;            // rows16: [na] first points
            int* Tnc = A.tk_uniq + ((base + n_extra + 31) & ~31);  // rows16: [na] next round's times (the q of the pass after the rounds lives here afterwards)
            if (rows16) {
                for (int v = tid; v < nv; v += kCcThreads) loc[v] = 0xffff;
                __syncthreads();
                for (int x = tid; x < na; x += kCcThreads)
                    if (La[x] < nv) loc[La[x]] = x;
                __syncthreads();
            }
            if (rows16) {  // run records, first points, cleared times: two nodes per thread and step (their gathers side by side)
                for (int x0 = tid; x0 < na; x0 += 2 * kCcThreads) {
                    int jn[2];
                    Run rn[2];
                    int p1[2], hm[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) jn[u] = x0 + u * kCcThreads < na ? La[x0 + u * kCcThreads] : -1;
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        if (jn[u] >= 0) rn[u] = run_of_node(jn[u]);
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        p1[u] = (jn[u] >= 0 && jn[u] < nv) ? vpts[rn[u].o] : 0x7fffffff;
                        hm[u] = jn[u] >= 0 ? loc[rn[u].v] : 0;
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        if (jn[u] < 0) continue;
                        const int x = x0 + u * kCcThreads;
                        if (hm[u] == 0xffff) {  // (never seen: the closure above lists the home voxel of every listed run; counted, the run then answers for itself)
                            hm[u] = x;
                            atomicAdd(&A.cc_stats[7], 1);
                        }
                        Tc[x] = 0x7fffffff;
                        P1c[x] = p1[u];
                        runs[x] = make_int4(rn[u].o, hm[u], rn[u].len | (rn[u].regular ? (int)0x80000000u : 0), rn[u].t);
                    }
                }
            }
            for (int x = tid; x < na && !rows16; x += kCcThreads) {
                const int j = La[x];
                if (rows16) {
                    Tc[x] = 0x7fffffff;
                    P1c[x] = j < nv ? vpts[vbeg[j]] : 0x7fffffff;
                } else if (j < nv) {
                    Tg[j] = 0x7fffffff;
                    P1g[j] = vpts[vbeg[j]];
                }
                if (tabled) {
                    const Run r = run_of_node(j);
                    int home = r.v;
                    if (rows16) {
                        home = loc[r.v];
                        if (home == 0xffff) {  // (never seen: the closure above lists the home voxel of every listed run; counted, the run then answers for itself)
                            home = x;
                            atomicAdd(&A.cc_stats[7], 1);
                        }
                    }
                    runs[x] = make_int4(r.o, home, r.len | (r.regular ? (int)0x80000000u : 0), r.t);
                    if (rows16) continue;  // (the rows: a pass of their own, shared with the helper blocks -- below)
                    int lst[27];
                    const int jj = cc_list27(K, r.t, R, S, Az, lst);
                    if (rows16) {
                        uint32_t lv[28];
#pragma unroll
                        for (int k = 0; k < 27; ++k) lv[k] = k < jj ? (uint32_t)loc[lst[k]] : 0xffffu;  // (the gathers in flight together)
                        lv[27] = 0xffffu;
                        uint32_t w16[16];
#pragma unroll
                        for (int k = 0; k < 14; ++k) w16[k] = (lv[2 * k] & 0xffffu) | (lv[2 * k + 1] << 16);
                        w16[14] = w16[15] = 0xffffffffu;
                        uint4* row = reinterpret_cast<uint4*>(nbr16 + (size_t)x * 32);  // (64-byte rows behind 16-byte run records: aligned)
#pragma unroll
                        for (int k = 0; k < 4; ++k) row[k] = make_uint4(w16[4 * k], w16[4 * k + 1], w16[4 * k + 2], w16[4 * k + 3]);
                    } else {
                        uint32_t* row = nbr + (size_t)x * 32;
                        for (int k = 0; k < 32; ++k) row[k] = k < jj ? (uint32_t)lst[k] : 0xffffffffu;
                    }
                }
            }
            __syncthreads();
            auto cached_run = [&](int x) -> Run {
                if (!tabled) return run_of_node(La[x]);
                const int4 c = runs[x];
                Run r;
                r.o = c.x;
                r.v = c.y;
                r.len = c.z & 0x7fffffff;
                r.regular = c.z < 0;
                r.t = c.w;
                return r;
            };
            auto walk = [&](int x, int32_t t, auto f) {  // f(u) in list order; false stops
                if (rows16) {
                    const uint16_t* row = nbr16 + (size_t)x * 32;
                    for (int e = 0; e < 27; ++e) {
                        const uint32_t u = row[e];
                        if (u == 0xffffu || !f((int)u)) return;
                    }
                } else if (tabled) {
                    const uint32_t* row = nbr + (size_t)x * 32;
                    for (int e = 0; e < 27; ++e) {
                        const uint32_t u = row[e];
                        if (u == 0xffffffffu || !f((int)u)) return;
                    }
                } else {
                    cc_for_each_listed(K, t, R, S, Az, f);
                }
            };
            auto labelled_voxel = [&](int u, int i) -> bool { return Tg[u] < i; };
            auto load_row = [&](int x, uint32_t(&u)[28]) {  // (rows16) 0xffffffff = no entry
                const uint4* row = reinterpret_cast<const uint4*>(nbr16 + (size_t)x * 32);
                uint4 r[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = row[k];
                const uint32_t w[16] = {r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, r[1].z, r[1].w, r[2].x, r[2].y, r[2].z, r[2].w, r[3].x, r[3].y, r[3].z, r[3].w};
#pragma unroll
                for (int e = 0; e < 28; ++e) {
                    const uint32_t v16 = (w[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
                    u[e] = v16 == 0xffffu ? 0xffffffffu : v16;
                }
            };
            CCW_MARK(9);
            int rounds_done = 0;
            CcExactTabs E;
            E.runs = runs;
            E.nbr16 = nbr16;
            E.Tg = Tc;
            E.P1g = P1c;
            E.Tng = Tnc;
            E.vpts = vpts;
            E.La = La;
            E.qnode = rows16 ? Tnc : A.tk_uniq + base + n_extra;  // (rows16: the next times are dead when the q pass writes)
            E.parent = parent;
            E.touched = touched;
            E.found = found;
            E.keys = K.k;
            E.tabg = tabg;
            E.loc = loc;
            E.nvox = nv;
            E.R = R;
            E.S = S;
            E.Az = Az;
            E.bshift = K.bshift;
            E.agg = nullptr;  // (this workgroup's LDS holds the scan's tables)
            E.remote = false;
            // a large component: the rounds go on the board (see cc_help_loop); wlast[9] = this leader's slot or -1
            int32_t* hslot = nullptr;
            const int nchunks = (na + kCcThreads - 1) / kCcThreads;
            if (rows16 && na >= kCcHelpMinNodes && A.cc_help_blocks > 0) {
                if (tid == 0) {
                    const int k = atomicAdd(&A.cc_help[0], 1);
                    wlast[9] = k < kCcHelpSlots ? k : -1;
                    if (k < kCcHelpSlots) {
                        int32_t* sl = A.cc_help + kCcHelpHdr + (size_t)k * kCcHelpSlotWords;
                        sl[2] = 0;
                        sl[3] = na;
                        *reinterpret_cast<const void**>(sl + 6) = runs;
                        *reinterpret_cast<const void**>(sl + 8) = nbr16;
                        *reinterpret_cast<const void**>(sl + 10) = Tc;
                        *reinterpret_cast<const void**>(sl + 12) = P1c;
                        *reinterpret_cast<void**>(sl + 14) = Tnc;
                        *reinterpret_cast<const void**>(sl + 16) = vpts;
                        *reinterpret_cast<const void**>(sl + 26) = La;
                        *reinterpret_cast<void**>(sl + 28) = E.qnode;
                        *reinterpret_cast<void**>(sl + 30) = parent;
                        *reinterpret_cast<void**>(sl + 32) = touched;
                        *reinterpret_cast<void**>(sl + 34) = found;
                        *reinterpret_cast<const void**>(sl + 48) = K.k;
                        *reinterpret_cast<const void**>(sl + 50) = tabg;
                        *reinterpret_cast<const void**>(sl + 52) = loc;
                        sl[36] = nv;
                        sl[37] = R;
                        sl[44] = S;
                        sl[45] = Az;
                        sl[46] = K.bshift;
                        __hip_atomic_store(&sl[4], nchunks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                __syncthreads();
                if (wlast[9] >= 0) hslot = A.cc_help + kCcHelpHdr + (size_t)wlast[9] * kCcHelpSlotWords;
                if (hslot && tid == 0) {  // development: where the time of a large component goes (SCVOD_CC_HELP_DUMP, 10 ns ticks; the clocks of the phases before: -DSCVOD_CC_DEVCLK)
                    *reinterpret_cast<long long*>(hslot + 20) = wall_clock64();
                    hslot[18] = s;
#ifdef SCVOD_CC_DEVCLK
                    *reinterpret_cast<long long*>(hslot + 38) = t_entry;
                    *reinterpret_cast<long long*>(hslot + 40) = t_rule;
                    *reinterpret_cast<long long*>(hslot + 42) = t_list;
#endif
                }
            }
            int chunks_mine = 0, phase_no = 0, helped = 0;
            E.remote = hslot != nullptr;  // (then this workgroup too reads the times past its caches: it rewrites them with written-through stores)
            // one pass over the listed nodes, shared with the helper blocks when this scan has a slot on the board (else: this workgroup's
            // own loop).  Everything written so far -> release -> the claim word (phase number << 3 | kind in its upper half); the leader takes
            // chunks like everybody else and then waits for the chunks OTHERS claimed (they are running: only a resident workgroup claims)
            auto share = [&](int kind, auto body) {
                if (!hslot) {
                    for (int x = tid; x < na; x += kCcThreads) body(x);
                    __syncthreads();
                    return;
                }
                // the FIRST publication carries everything built so far (rows, run records, first points, the node list): one agent-scope release
                // (this XCD's L2 written back, once per large component).  Later ones only follow written-through stores: a drain is enough.
                if (phase_no == 0)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                else
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __syncthreads();
                ++phase_no;
                if (tid == 0) __hip_atomic_store(cc_help_claim_word(hslot), (unsigned long long)((phase_no << 3) | kind) << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                int mine = 0;
                for (;;) {
                    if (tid == 0) wlast[10] = (int)(__hip_atomic_fetch_add(cc_help_claim_word(hslot), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0xffffffffu);
                    __syncthreads();
                    const int idx = wlast[10];
                    __syncthreads();
                    if (idx >= nchunks) break;
                    const int x = idx * kCcThreads + tid;
                    if (x < na) body(x);
                    ++mine;
                }
                chunks_mine += mine;
                helped += nchunks - mine;  // (the done counter is cumulative: a reset could land behind a fast helper's increment)
                if (tid == 0)
                    while (__hip_atomic_load(&hslot[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < helped) __builtin_amdgcn_s_sleep(8);
                __syncthreads();  // (no acquire: what the helpers produced are atomics and written-through stores, read back past the caches)
            };
            if (rows16) {  // the rows: every node's 27-cell listing (nine searches of the key table), shared
                for (int b = tid; b <= nb; b += kCcThreads) tabg[b] = (uint32_t)tab[b];
                __syncthreads();
                share(kCcPhaseRows, [&](int x) { cc_exact_rows16(E, x); });
            }
            for (int round = 0; round < 1024; ++round) {
                ++rounds_done;
                for (int x = tid; x < na; x += kCcThreads)
                    if (La[x] < nv) {
                        if (hslot)
                            __hip_atomic_store(&Tnc[x], 0x7fffffff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        else
                            (rows16 ? Tnc[x] : Tng[La[x]]) = 0x7fffffff;
                    }
                __syncthreads();
                if (rows16) share(round == 0 ? kCcPhaseRound0 : kCcPhaseRound, [&](int x) { cc_exact_visit16(E, x, round == 0); });
                for (int x = tid; x < na && !rows16; x += kCcThreads) {
                    const Run r = cached_run(x);
                    const int nev = r.regular ? min(r.len, 3) : r.len;
                    for (int p0 = 0; p0 < nev; p0 += 3) {
                        int ie[3], qe[3];
                        bool cs[3];
#pragma unroll
                        for (int e = 0; e < 3; ++e) {
                            ie[e] = (p0 + e < nev) ? vpts[r.o + p0 + e] : 0x7fffffff;
                            cs[e] = p0 + e < nev && (round == 0 || labelled_voxel(r.v, ie[e]));
                            qe[e] = -1;
                        }
                        int jj = 0;
                        walk(x, r.t, [&](int u) -> bool {
                            const int p1 = P1g[u];
#pragma unroll
                            for (int e = 0; e < 3; ++e)
                                if (qe[e] < 0 && ie[e] != 0x7fffffff && (labelled_voxel(u, ie[e]) || p1 < ie[e])) qe[e] = jj;
                            ++jj;
                            return true;
                        });
                        jj = 0;
                        walk(x, r.t, [&](int u) -> bool {
                            const int p1 = P1g[u];
                            int te = 0x7fffffff;
#pragma unroll
                            for (int e = 2; e >= 0; --e)
                                if (ie[e] != 0x7fffffff && (cs[e] || qe[e] < 0 || jj > qe[e] || (jj == qe[e] && p1 < ie[e]))) te = ie[e];
                            if (te != 0x7fffffff && te < cc_ld(&Tng[u])) atomicMin(&Tng[u], te);
                            ++jj;
                            return true;
                        });
                    }
                }
                __syncthreads();
                bool changed = false;
                for (int x = tid; x < na; x += kCcThreads) {
                    const int j = La[x];
                    if (j >= nv) continue;
                    if (rows16) {
                        const int tv = cc_ld(&Tnc[x]);
                        if (hslot) {
                            changed |= tv != cc_ld(&Tc[x]);
                            __hip_atomic_store(&Tc[x], tv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        } else {
                            changed |= tv != Tc[x];
                            Tc[x] = tv;
                        }
                    } else {
                        const int tv = cc_ld(&Tng[j]);
                        changed |= tv != Tg[j];
                        Tg[j] = tv;
                    }
                }
                if (!__syncthreads_or(changed ? 1 : 0)) break;
            }
            if (hslot && tid == 0) {
                *reinterpret_cast<long long*>(hslot + 22) = wall_clock64();
                hslot[19] = rounds_done;
            }
            // q of every listed node at its last point, then the unions of these components from scratch
            int* qnode = A.tk_uniq + base + n_extra;  // [na] (behind the extras list; rows16: the next-times table of the rounds, dead now)
            CCW_MARK(10);
#ifdef SCVOD_PROFILE
            if (tid == 0) atomicAdd(&g_prof[4][13], 100ull * rounds_done);
#endif
            if (rows16) share(kCcPhaseQ, [&](int x) { cc_exact_q16(E, x); });  // (rows16 implies q_fits; the table of the next times the q's overwrite is dead)
            for (int x = tid; x < na && !rows16; x += kCcThreads) {
                const Run r = cached_run(x);
                const int i = vpts[r.o + r.len - 1];
                int q = -1, jj = 0;
                if (!labelled_voxel(r.v, i))
                    walk(x, r.t, [&](int u) -> bool {
                        if (labelled_voxel(u, i) || P1g[u] < i) {
                            q = jj;
                            return false;
                        }
                        ++jj;
                        return true;
                    });
                if (q_fits) qnode[x] = max(q, 0);
            }
            __syncthreads();
            CCW_MARK(11);
            if (q_fits) {
                for (int x = tid; x < na; x += kCcThreads) {
                    const int j = La[x];
                    __hip_atomic_store(&parent[j], j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (helper blocks may run the unions)
                    atomicAnd(&found[j >> 5], ~(1 << (j & 31)));
                    if (j < nv) atomicAnd(&touched[j >> 5], ~(1 << (j & 31)));
                }
                __syncthreads();
                if (rows16) share(kCcPhaseUnion, [&](int x) { cc_exact_union16(E, x); });
                for (int x = tid; x < na && !rows16; x += kCcThreads) {
                    const int j = La[x];
                    const int q = qnode[x];
                    int jj = 0;
                    walk(x, triple_of(j), [&](int u) -> bool {
                        if (jj >= q) {
                            cc_set(touched, u);
                            if (u != j) cc_union(parent, j, u);
                        }
                        ++jj;
                        return true;
                    });
                    if (jj > 0) cc_set(found, j);
                }
                __syncthreads();
                if (hslot && tid == 0) {
                    __hip_atomic_store(cc_help_claim_word(hslot), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // closed
                    hslot[5] = chunks_mine;
                }
                for (int x = tid; x < na; x += kCcThreads) {
                    const int j = La[x];
                    if (j < nv) continue;
                    const int v = voxel_of_slot(extras[j - nv]);
                    if (cc_bit(touched, v)) cc_union(parent, j, v);
                }
                __syncthreads();
            }
            CCW_MARK(12);
            if (hslot && tid == 0) *reinterpret_cast<long long*>(hslot + 24) = wall_clock64();
        }
        if (tid == 0) atomicAdd(&A.cc_help[1], 1);  // past the passes that may ask for help (cc_help_loop leaves when every scan of k_cc_exact is)
        }  // (SHARED)
    }
    if (!FAST) CCW_MARK(7);
    // canonical name of a component: the smallest apri index among the openers of its nodes (every other member of a
    // node sits behind its opener in an ascending point list)
    int* minpt = FAST ? lkeys : A.cl_count + base;  // the key table is not needed any more
    int* flat_g = A.tk_cursor + base;               // [nn] generic variant: root of every node
    for (int j = tid; j < nn; j += kCcThreads) minpt[j] = 0x7fffffff;
    __syncthreads();
    if (FAST) {
        for (int j = tid; j < nn; j += kCcThreads) {
            const int k = (j < nv) ? vbeg[j] : extras[j - nv];
            const int r = cc_find(parent, j);
            atomicMin(&minpt[r], vpts[k]);
        }
    } else {
        // minima in HBM: neighbours in the node list mostly share their root -- one atomic per distinct root of a wave.  Four nodes
        // per thread and step, their gathers and the hops to their roots in flight together; the roots are final here and are
        // kept (flat_g) for the numbering below
        for (int j0 = 0; j0 < nn; j0 += kCcThreads * 4) {
            int kk[4], rr[4], nm[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u * kCcThreads + tid;
                kk[u] = (j < nn) ? ((j < nv) ? vbeg[j] : extras[j - nv]) : 0;
                rr[u] = (j < nn) ? cc_ld(&parent[j]) : 0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) nm[u] = vpts[kk[u]];
            bool more = true;
            while (more) {
                more = false;
                int pp[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) pp[u] = cc_ld(&parent[rr[u]]);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (pp[u] != rr[u]) {
                        rr[u] = pp[u];
                        more = true;
                    }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u * kCcThreads + tid;
                const int r = (j < nn) ? rr[u] : -1;
                if (j < nn) flat_g[j] = r;
                bool todo = r >= 0;
                while (__any(todo)) {
                    const int first = __ffsll((long long)__ballot(todo)) - 1;
                    const int r0 = __shfl(r, first);
                    const bool mine = todo && r == r0;
                    int m = mine ? nm[u] : 0x7fffffff;
#pragma unroll
                    for (int d = 32; d > 0; d >>= 1) m = min(m, __shfl_xor(m, d));
                    if ((tid & 63) == first) atomicMin(&minpt[r0], m);
                    if (mine) todo = false;
                }
            }
        }
    }
    __syncthreads();
    CC_MARK(4);
    // flatten, then number the components 0 .. ncl-1 in node order: parent[j] becomes the compact id of j's component
    int* flat = A.tk_cursor + base;                 // [nn] root of every node (arena scratch, nn <= n)
    if (FAST) {
        for (int j = tid; j < nn; j += kCcThreads) {
            int r = j;
            for (int q = parent[r]; q != r; q = parent[r]) r = q;  // read-only walk: the roots are final
            flat[j] = r;
        }
        __syncthreads();
    }  // (generic variant: written with the names above)
    int* slot_cid = (int*)(A.tk_pairs + base);      // [n] compact id of every apri point's component, -1 = a cluster of its own
    int* rootcid = slot_cid + n;                    // [nn]
    int* names = A.tk_nuniq + base;                 // [ncl] canonical name per compact id
    int ncl = 0;
    if constexpr (FAST) {
        // compact ids of the roots in node order with two barriers: roots counted per (chunk, wave) by ballot, one prefix over the
        // <= kCcNodes / 64 + 16 counts (four per lane of the first wave), then every root knows its id
        constexpr int NW = kCcThreads / 64;
        const int lane = tid & 63, wave = tid >> 6;
        const int chunks = (nn + kCcThreads - 1) / kCcThreads;
        for (int c = 0; c < chunks; ++c) {
            const int j = c * kCcThreads + tid;
            const unsigned long long rb = __ballot((j < nn) && flat[j] == j);
            if (lane == 0) wcnt[c * NW + wave] = __popcll(rb);
        }
        __syncthreads();
        const int ne = chunks * NW;
        if (wave == 0) {
            int a[4], sum = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = (4 * lane + q < ne) ? wcnt[4 * lane + q] : 0;
                sum += a[q];
            }
            const int inc = wave_incl_scan(sum);
            int ex = inc - sum;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (4 * lane + q < ne) wcnt[4 * lane + q] = ex;
                ex += a[q];
            }
            if (lane == 63) wcnt[kCcCounts - 1] = inc;
        }
        __syncthreads();
        ncl = wcnt[kCcCounts - 1];
        for (int c = 0; c < chunks; ++c) {
            const int j = c * kCcThreads + tid;
            const bool isroot = (j < nn) && flat[j] == j;
            const unsigned long long rb = __ballot(isroot);
            if (isroot) {
                const int id = wcnt[c * NW + wave] + __popcll(rb & ((1ull << lane) - 1ull));
                rootcid[j] = id;
                names[id] = minpt[j];
            }
        }
    } else {
        for (int j0 = 0; j0 < nn; j0 += kCcThreads) {
            const int j = j0 + tid;
            const bool isroot = (j < nn) && flat[j] == j;
            int total;
            const int ex = block_excl_scan<kCcThreads>(isroot ? 1 : 0, total, wsum);
            if (isroot) {
                rootcid[j] = ncl + ex;
                names[ncl + ex] = minpt[j];
            }
            ncl += total;
        }
    }
    __syncthreads();
    for (int j = tid; j < nn; j += kCcThreads) parent[j] = rootcid[flat[j]];
    __syncthreads();
    CC_MARK(5);
    for (int k0 = 0; k0 < n; k0 += kCcThreads * 4) {  // four slots per thread and step: their loads are in flight together
        int pv[4], cv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) pv[u] = vpts[min(k0 + u * kCcThreads + tid, n - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * kCcThreads + tid;
            int cid = -2;
            if (k < n) {
                const int v = voxel_of_slot(k);
                if (allreg || cc_bit(touched, v)) {
                    cid = parent[v];
                } else {
                    int o = k;  // opener of this slot's run: the closest run start at or before k (a voxel start is one)
                    {
                        int w = o >> 5;
                        unsigned m = (unsigned)rstart[w] & (0xffffffffu >> (31 - (o & 31)));
                        while (!m) m = (unsigned)rstart[--w];
                        o = (w << 5) + 31 - __clz(m);
                    }
                    const int node = (o == vbeg[v]) ? v : nv + extra_of_slot[o];
                    // a point that found nothing is a cluster of its own (ssc.cpp:347-353); the members of a run that found
                    // something joined what the opener joined
                    cid = cc_bit(found, node) ? parent[node] : -1;
                }
            }
            cv[u] = cid;
        }
        int nm[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) nm[u] = names[max(cv[u], 0)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (cv[u] == -2) continue;
            slot_cid[pv[u]] = cv[u];  // (indexed by apri point from here on: the passes below stream the points in order)
            A.pt_cluster[(size_t)base + pv[u]] = cv[u] >= 0 ? nm[u] : pv[u];
        }
    }
    __syncthreads();
    CC_MARK(6);
    // ---- bounding boxes + type of every cluster (refineClusterByBoundingBox ssc.cpp:437-467, recognize ssc.cpp:849-872).
    // The boxes take the key table's LDS (the search is over); components beyond kCcBoxes take arena scratch.
    uint32_t* bb = (uint32_t*)cc_smem;
    uint32_t* ov = (uint32_t*)(A.cl_bbox + 7 * (size_t)base);  // overflow records, 7 words each
    for (int c = tid; c < ncl; c += kCcThreads) {
        uint32_t* r = c < kCcBoxes ? bb + 7 * c : ov + 7 * (size_t)(c - kCcBoxes);
        r[0] = r[1] = r[2] = 0xffffffffu;  // running minima (order-preserving encoding)
        r[3] = r[4] = r[5] = 0u;           // running maxima
        r[6] = 0u;                         // members
    }
    __syncthreads();
    {
        constexpr int U = 4;  // four points per thread and step: their index and point loads are in flight together (eight: slower)
        for (int i0 = 0; i0 < n; i0 += kCcThreads * U) {
            int cidv[U], srcv[U];
            float4 qv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * kCcThreads + tid;
                cidv[u] = (i < n) ? slot_cid[i] : -2;
                srcv[u] = (i < n && !from_apri) ? A.apri_src[(size_t)base + i] : 0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = min(i0 + u * kCcThreads + tid, n - 1);
                if (from_apri) {  // apri_vec supplied by the caller: no input cloud on the device
                    const scvod_apri& a = A.apri[(size_t)base + i];
                    qv[u] = make_float4(a.x, a.y, a.z, 0.f);
                } else {  // cloud_use[i] = input point apri_src[i]
                    qv[u] = A.pts[base + srcv[u]];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + u * kCcThreads + tid;
                const int cid = cidv[u];
                if (cid == -1) {  // one point: z extent 0 < 0.2 m, erased whatever toBeClass is (ssc.cpp:444)
                    A.pt_type[(size_t)base + i] = 0;
                    A.cl_count[(size_t)base + i] = 1;
                }
                {  // the member count: one add per run of a cluster's points in the wave
                    const int ck = max(cid, 0);
                    cc_run_add(ck < kCcBoxes ? bb + 7 * ck + 6 : ov + 7 * (size_t)(ck - kCcBoxes) + 6, cid);
                }
                if (cid < 0) continue;
                // most points lie inside the box their component has so far: plain reads first, an atomic only to grow it
                uint32_t* r = cid < kCcBoxes ? bb + 7 * cid : ov + 7 * (size_t)(cid - kCcBoxes);
                const uint32_t ox = f2ord(qv[u].x), oy = f2ord(qv[u].y), oz = f2ord(qv[u].z);
                const uint32_t b0 = cc_ldu(&r[0]), b1 = cc_ldu(&r[1]), b2 = cc_ldu(&r[2]), b3 = cc_ldu(&r[3]), b4 = cc_ldu(&r[4]), b5 = cc_ldu(&r[5]);
                if (ox < b0) atomicMin(&r[0], ox);
                if (oy < b1) atomicMin(&r[1], oy);
                if (oz < b2) atomicMin(&r[2], oz);
                if (ox > b3) atomicMax(&r[3], ox);
                if (oy > b4) atomicMax(&r[4], oy);
                if (oz > b5) atomicMax(&r[5], oz);
            }
        }
    }
    CC_MARK(7);
    __syncthreads();
    for (int c = tid; c < ncl; c += kCcThreads) {
        uint32_t* r = c < kCcBoxes ? bb + 7 * c : ov + 7 * (size_t)(c - kCcBoxes);
        const float mnx = ord2f(r[0]), mny = ord2f(r[1]), mnz = ord2f(r[2]);
        const float mxx = ord2f(r[3]), mxy = ord2f(r[4]), mxz = ord2f(r[5]);
        const int cnt = (int)r[6];
        const uint32_t t = cc_type_rule(P, mnx, mny, mnz, mxx, mxy, mxz, cnt);
        r[0] = t;
        r[1] = 0;  // (the box is used up: the word counts the cluster's voxels below)
        r[4] = 0xffffffffu;  // ... and this one takes the lowest voxel slot carrying the cluster's label (its id in the tracking chain)
        A.cl_count[(size_t)base + names[c]] = cnt;  // Cluster::occupy_pts.size(), kept at the cluster's canonical name
    }
    __syncthreads();
    // ---- successor table of the scan: Voxel::label after clusterAndCreateFrame + refineClusterByBoundingBox (ssc.cpp:388-392,
    // 461-466) = the cluster of the voxel's first point, -1 when the refine erased it; |occupy_voxels| of that cluster
    // (sampleVec of its points' voxel_idx, ssc.cpp:382-384) = the number of voxels carrying its label; its type.  This is what
    // SSC::tracking probes a predecessor against and what a shard exports (scvod_batch_export_table).
    auto cid_of_voxel = [&](int v) -> int {  // the voxel's first point opens node v
        return (allreg || cc_bit(touched, v) || cc_bit(found, v)) ? parent[v] : -1;
    };
    for (int v0 = 0; v0 < nv; v0 += kCcThreads) {  // (uniform trip count: cc_run_add is a wave-wide call)
        const int v = v0 + tid;
        int cid = (v < nv) ? cid_of_voxel(v) : -1;
        uint32_t* r = bb;
        if (cid >= 0) {
            r = cid < kCcBoxes ? bb + 7 * cid : ov + 7 * (size_t)(cid - kCcBoxes);
            if (!r[0]) cid = -1;  // (erased by the refine: no label)
        }
        // voxels in key order: a cluster's voxels come in runs; the run's first voxel is its lowest slot
        cc_run_add(r + 1, cid);
        const int prevc = __shfl_up(cid, 1);
        if (cid >= 0 && ((tid & 63) == 0 || prevc != cid)) atomicMin(&r[4], (uint32_t)v);
    }
    __syncthreads();
    for (int v = tid; v < nv; v += kCcThreads) {
        const int cid = cid_of_voxel(v);
        int4 rec = make_int4(A.vox_key[(size_t)base + v], -1, 0, 0);
        int rep = -1;
        if (cid >= 0) {
            const uint32_t* r = cid < kCcBoxes ? bb + 7 * cid : ov + 7 * (size_t)(cid - kCcBoxes);
            if (r[0]) {
                rec.y = names[cid];
                rec.z = (int)r[1];
                rec.w = (int)r[0];
                rep = (int)r[4];
            }
        }
        A.vox_track[(size_t)base + v] = rec;
        A.vox_rep[(size_t)base + v] = rep;
        // for the max_name pass that follows (scvod_lastname.hip): the cluster of the voxel's first point whether the refine erased
        // it or not (-1: not decided here), and that point -- two arrays the voxel stage no longer needs
        A.tmp_vox_key[(size_t)base + v] = cid >= 0 ? names[cid] : -1;
        ((int32_t*)A.sorted_idx)[(size_t)base + v] = vpts[vbeg[v]];
    }
    // ---- member lists of the car clusters (what SSC::tracking walks, ssc.cpp:1274-1321): the car roots in ascending order
    // (tk_clusters), exclusive offsets of their sizes (tk_mbegin at the root), and -- in the per-point pass below -- every
    // car point appended to its cluster's list (tk_members; the order inside a list is immaterial).  The car components are
    // few (tens): listed in the LDS the bit arrays released, ranked by counting.
    __syncthreads();
    int ncar = 0;
    for (int c0 = 0; c0 < ncl; c0 += kCcThreads) {
        const int c = c0 + tid;
        const uint32_t* r = c < kCcBoxes ? bb + 7 * c : ov + 7 * (size_t)(c - kCcBoxes);
        ncar += __syncthreads_count(c < ncl && r[0] == 2u);
    }
    const int carcap = slots_lds ? (3 * kSlotWords) / 4 : 0;
    const bool car_lds = ncar <= carcap;  // four lists of ncar entries; arena scratch (dead by now) when they are many
    int* carname = car_lds ? vstart : A.tk_uniq + base;
    int* carcid = car_lds ? carname + ncar : A.cc_parent + base;
    int* scnt = car_lds ? carcid + ncar : A.tk_hit + base;
    int* scid = car_lds ? scnt + ncar : A.tk_npairs + base;
    {
        int run = 0;
        for (int c0 = 0; c0 < ncl; c0 += kCcThreads) {
            const int c = c0 + tid;
            const uint32_t* r = c < kCcBoxes ? bb + 7 * c : ov + 7 * (size_t)(c - kCcBoxes);
            const bool car = c < ncl && r[0] == 2u;
            int total;
            const int ex = block_excl_scan<kCcThreads>(car ? 1 : 0, total, wsum);
            if (car) {
                carname[run + ex] = names[c];
                carcid[run + ex] = c;
            }
            run += total;
        }
    }
    __syncthreads();
    for (int j = tid; j < ncar; j += kCcThreads) {
        const int mine = carname[j], cid = carcid[j];
        int rank = 0;
        for (int i = 0; i < ncar; ++i) rank += carname[i] < mine ? 1 : 0;
        const uint32_t* r = cid < kCcBoxes ? bb + 7 * cid : ov + 7 * (size_t)(cid - kCcBoxes);
        scnt[rank] = (int)r[6];
        scid[rank] = cid;
        A.tk_clusters[(size_t)base + rank] = mine;
        A.tk_crep[(size_t)base + rank] = (int)r[4];
    }
    __syncthreads();
    {
        int run = 0;
        for (int j0 = 0; j0 < ncar; j0 += kCcThreads) {
            const int j = j0 + tid;
            const int cnt = j < ncar ? scnt[j] : 0;
            int total;
            const int ex = block_excl_scan<kCcThreads>(cnt, total, wsum);
            if (j < ncar) {
                const int cid = scid[j];
                uint32_t* r = cid < kCcBoxes ? bb + 7 * cid : ov + 7 * (size_t)(cid - kCcBoxes);
                r[2] = (uint32_t)(run + ex);  // where the cluster's member list starts
                r[3] = 0u;                    // its cursor
                A.tk_mbegin[(size_t)base + names[cid]] = run + ex;
            }
            run += total;
        }
        if (tid == 0) {
            A.tk_scan[s * 4 + 0] = ncar;
            A.tk_scan[s * 4 + 1] = run;
        }
    }
    __syncthreads();
    CC_MARK(8);
    for (int i0 = 0; i0 < n; i0 += kCcThreads * 4) {
        int cv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * kCcThreads + tid;
            cv[u] = (i < n) ? slot_cid[i] : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int cid = cv[u];
            uint32_t* r = bb;
            uint32_t t = 0u;
            if (cid >= 0) {
                r = cid < kCcBoxes ? bb + 7 * cid : ov + 7 * (size_t)(cid - kCcBoxes);
                t = r[0];
            }
            const int i = i0 + u * kCcThreads + tid;
            // a place in the cluster's member list: the list's cursor is advanced once per run of the cluster's points in the wave
            const uint32_t at = cc_run_add(r + 3, t == 2u ? cid : -1);
            if (cid < 0) continue;
            A.pt_type[(size_t)base + i] = (uint8_t)t;
            if (t == 2u) {
                A.tk_members[(size_t)base + r[2] + at] = i;
                if (!from_apri) A.pt_mapcls[(size_t)base + A.apri_src[(size_t)base + i]] = kMapCar;  // (the batch starts with clean marks)
            }
        }
    }
    CC_MARK(9);
    return true;
}

// the scans with triples outside the grid run the visiting-order model (milliseconds instead of a quarter of one): they are
// handed out first, so that they overlap the regular ones instead of trailing them.  One workgroup, stable partition.
__global__ __launch_bounds__(1024) void k_cc_order(Arena A) {
    __shared__ int wsum[17];
    const int B = A.n_scans;
    int n_irr = 0;
    for (int s0 = 0; s0 < B; s0 += 1024) n_irr += __syncthreads_count(s0 + (int)threadIdx.x < B && A.scan_irr[s0 + threadIdx.x] != 0);
    int run_i = 0, run_r = 0;
    for (int s0 = 0; s0 < B; s0 += 1024) {
        const int s = s0 + threadIdx.x;
        const bool irr = s < B && A.scan_irr[s] != 0;
        int ti, tr;
        const int ei = block_excl_scan<1024>(irr ? 1 : 0, ti, wsum);
        const int er = block_excl_scan<1024>((s < B && !irr) ? 1 : 0, tr, wsum);
        if (s < B) A.cc_perm[irr ? run_i + ei : n_irr + run_r + er] = s;
        run_i += ti;
        run_r += tr;
    }
}

__global__ __launch_bounds__(kCcThreads) void k_cc_scan(DevParams P, Arena A, int from_apri) {
    __shared__ int wsum[17];
    __shared__ int wcnt[kCcCounts];
    __shared__ int wlast[kCcThreads / 64];
    __shared__ int n_extra_s;
    __shared__ int bad_s[kCcBad + 1];
    const int s = A.cc_perm[blockIdx.x];
    const int base = A.scan_off[s];
    const int n = A.counts[s * 8 + 4];
    const int nv = A.counts[s * 8 + 6];
    if (n <= 0) {
        if (threadIdx.x < 2) A.tk_scan[s * 4 + threadIdx.x] = 0;  // no car clusters, no car points
        return;
    }
    bool done = false;
    if (n <= kCcSlots && nv <= kCcNodes && (long long)P.bin.range_num * P.bin.sector_num * P.bin.azimuth_num < 0x7fffffffLL) {
        done = cc_scan_impl<true>(P, A, from_apri, wsum, wcnt, wlast, n_extra_s, bad_s, s, base, n, nv);
        __syncthreads();
    }
    if (!done) cc_scan_impl<false>(P, A, from_apri, wsum, wcnt, wlast, n_extra_s, bad_s, s, base, n, nv);
}

// The scans k_cc_scan handed over (cc_again: a scan of the generic variant with an irregular run that the local rule does not settle), clustered
// again from scratch with the exact re-clustering of the affected components.  Grid = kCcExactBlocks whatever the batch holds (the list is
// on the device): block b < min(listed, kCcExactLeaders) LEADS the scans b, b + leaders, ...; every other block -- and a leader that has
// run out of scans -- HELPS (cc_help_loop: chunks of the passes the leaders publish).  All leaders start together with their helpers
// beside them: no order to guess, nothing to learn from an earlier batch.  Nothing listed: every block leaves at once.
__global__ __launch_bounds__(kCcThreads) void k_cc_exact(DevParams P, Arena A, int from_apri) {
    __shared__ int wsum[17];
    __shared__ int wcnt[kCcCounts];
    __shared__ int wlast[kCcThreads / 64];
    __shared__ int n_extra_s;
    __shared__ int bad_s[kCcBad + 1];
    const int n_redo = min(A.cc_again[0], A.n_scans);
    if (n_redo <= 0) return;
    const int leaders = min(n_redo, kCcExactLeaders);
    if ((int)blockIdx.x < leaders) {
        for (int i = blockIdx.x; i < n_redo; i += leaders) {
            const int s = A.cc_again[1 + i];
            const int base = A.scan_off[s];
            const int n = A.counts[s * 8 + 4];
            const int nv = A.counts[s * 8 + 6];
            __syncthreads();
            if (threadIdx.x == 0) wlast[9] = -1;
            const bool ok = cc_scan_impl<false, true>(P, A, from_apri, wsum, wcnt, wlast, n_extra_s, bad_s, s, base, n, nv);
            if (!ok && threadIdx.x == 0) atomicAdd(&A.cc_help[1], 1);  // (gave up before the passes that signal)
#ifdef SCVOD_CC_DEVCLK
            if (threadIdx.x == 0 && wlast[9] >= 0) *reinterpret_cast<long long*>(A.cc_help + kCcHelpHdr + (size_t)wlast[9] * kCcHelpSlotWords + 54) = wall_clock64();
#endif
        }
        __syncthreads();
    }
    if (A.cc_help_blocks > 0) cc_help_loop(A, wcnt, n_redo);
}
