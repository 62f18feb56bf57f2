// scvod_mapcomp.hip -- connected components of the static map's cells and their vote on the seen-through verdict (gfx950):
// scvod_map_components, scvod_map_component_visibility.
//
// Reference analogue: none; the conventions are this project's.  The map's table is the hash grid the labelling
// needs: nothing is built, the table is only read (through scvod_mapprobe.h's peek and chain walk).
//     k_mc_slots      every record walks the chain of its key; a record that finds its slot leaves its list index in slot_idx[slot]
//                     (atomicMin: the lowest index of a cell is its representative) and remembers the slot
//     k_mc_init       parent[i] = the representative of i's cell (-1: no node).  A duplicate never is a root, so nothing ever hooks
//                     under it or moves it
//     k_mc_union      every representative probes the half neighbourhood (3 / 9 / 13 cells: a union is symmetric) and unites itself
//                     with the representative it finds: find with path halving, the larger root hooked under the smaller by
//                     compare-and-swap.  parent[x] <= x always and only ever falls to another ancestor of x, so every walk ends; a swap
//                     that fails means another thread hooked that root -- progress --, so nothing waits for another workgroup
//     k_mc_flatten    parent[i] = the root of i = the lowest list index of its component; a root takes the next temporary number
//     k_mc_reduce     count, smallest key and cell box per root.  One component may hold nearly the whole list (a list with ground):
//                     a workgroup combines its 2048 records in an LDS table keyed by the root (a wave whose first live lane's root
//                     owns 16 lanes or more reduces those in registers first), then adds each entry once to the root's words
//     sort            rocprim::radix_sort_pairs of (smallest key, temporary number) over n entries; the entries behind the roots hold
//                     all ones
//     k_mc_table      rank -> record, temporary number -> rank, d_n and the stats
//     k_mc_assign     d_component[i] = rank of i's root
//     k_mcv_clear / k_mcv_count / k_mcv_decide / k_mcv_apply   the vote: the same LDS combine over the component index, one thread per
//                     component decides, every record takes its component's byte.  d_n is read on the device
// No grid barrier, no residency assumption, no spinning.  All sums are integers, every minimum is a minimum: the same bytes on every run.
#include <rocprim/device/device_radix_sort.hpp>

#include "scvod_mapprobe.h"

using namespace scvod;

namespace scvod {
namespace {

constexpr unsigned kMcNone = 0xFFFFFFFFu;
constexpr unsigned kMcField = (1u << kCellBits) - 1u;
constexpr int kMcChunk = 2048;      // records per workgroup of the reductions: eight rounds of 256
constexpr int kMcLdsSlots = 512;    // 20 KB (components) / 24 KB (vote)
constexpr int kMcLdsProbes = 8;
constexpr int kMcWaveGroup = 16;    // lanes of one root from which a wave reduces them in registers
constexpr unsigned kMcMaxBlocks = 8192;

// counter words of the labelling ...
enum { kMcNodes = 0, kMcDup, kMcPadding, kMcAbsent, kMcComponents, kMcWritten, kMcOverflow, kMcWords = 16 };
// ... and of the vote
enum { kMvComponents = 0, kMvVoted, kMvSeen, kMvMovedSeen, kMvMovedKeep, kMvWritten, kMvBeyond, kMvOverflow, kMvWords = 8 };

struct McAcc {  // 32 bytes per temporary number, initialised by the root's thread in k_mc_flatten
    unsigned cnt, first;
    unsigned mn[3], mx[3];
};
static_assert(sizeof(McAcc) == 32, "component accumulator");

struct MvAcc {  // 48 bytes per component, cleared by k_mcv_clear
    unsigned n, keep, seen, verdict;  // verdict: 0 none, else the byte
    unsigned long long sum[4];
};
static_assert(sizeof(MvAcc) == 48, "vote accumulator");

__device__ __forceinline__ int mc_load(const int* p, long long x) { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the slot of `key`, walking on from the peek `rec` of slot h: mq_find_from's walk, handing out the slot instead of the value
__device__ __forceinline__ bool mc_find_slot(const MapRec* table, unsigned long long mask, unsigned long long key, unsigned long long h, MapRec rec,
                                             unsigned long long& slot) {
    for (int probes = 0; probes < kMapMaxProbes; ++probes) {
        if (rec.key == key) {
            slot = h;
            return true;
        }
        if (rec.key == kEmpty) return false;
        h = (h + 1) & mask;
        rec = map_peek(table, h);
    }
    return false;
}

// the root of x, halving the path behind it
__device__ __forceinline__ int mc_find(int* parent, int x) {
    for (;;) {
        const int p = mc_load(parent, x);
        if (p == x) return x;
        const int gp = mc_load(parent, p);
        if (gp == p) return p;
        atomicMin(&parent[x], gp);  // (gp is an ancestor of x and stays one)
        x = gp;
    }
}

__device__ __forceinline__ void mc_unite(int* parent, int a, int b) {
    for (;;) {
        a = mc_find(parent, a);
        b = mc_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(&parent[a], a, b) == a) return;  // (a was a root and hangs under the smaller b now; else someone else hooked a)
    }
}

// block-wide: per-wave counts in registers -> LDS -> one atomic per counter and workgroup
template <int N>
__device__ __forceinline__ void mc_add_counters(unsigned* blk, const unsigned (&cnt)[N], unsigned long long* counters, int word0) {
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (cnt[k]) atomicAdd(&blk[k], cnt[k]);
    }
    __syncthreads();
    if (threadIdx.x < N && blk[threadIdx.x]) atomicAdd(&counters[word0 + threadIdx.x], (unsigned long long)blk[threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_mc_slots(const MapRec* __restrict__ recs, int n, const MapRec* __restrict__ table, unsigned long long mask,
                                                  unsigned* slot_idx, int* __restrict__ rec_slot, unsigned long long* counters) {
    __shared__ unsigned blk[2];
    if (threadIdx.x < 2) blk[threadIdx.x] = 0u;
    __syncthreads();
    unsigned cnt[2] = {0u, 0u};  // padding, absent (per wave)
    const long long bound = ((long long)n + 255) & ~255ll;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < bound; i += (long long)gridDim.x * 256) {
        const bool live = i < n;
        const unsigned long long key = live ? recs[i].key : kEmpty;
        unsigned long long slot = 0ull;
        bool found = false;
        if (key != kEmpty) {
            const unsigned long long h = map_home(key, mask);
            found = mc_find_slot(table, mask, key, h, map_peek(table, h), slot);
        }
        if (found) atomicMin(&slot_idx[slot], (unsigned)i);
        if (live) rec_slot[i] = found ? (int)slot : -1;
        cnt[0] += (unsigned)__popcll(__ballot(live && key == kEmpty));
        cnt[1] += (unsigned)__popcll(__ballot(live && key != kEmpty && !found));
    }
    mc_add_counters<2>(blk, cnt, counters, kMcPadding);  // (kMcAbsent follows)
}

__global__ __launch_bounds__(256) void k_mc_init(int n, const unsigned* __restrict__ slot_idx, const int* __restrict__ rec_slot, int* __restrict__ parent,
                                                 unsigned long long* counters) {
    __shared__ unsigned blk[2];
    if (threadIdx.x < 2) blk[threadIdx.x] = 0u;
    __syncthreads();
    unsigned cnt[2] = {0u, 0u};  // nodes, duplicates
    const long long bound = ((long long)n + 255) & ~255ll;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < bound; i += (long long)gridDim.x * 256) {
        int p = -1;
        if (i < n) {
            const int s = rec_slot[i];
            if (s >= 0) p = (int)slot_idx[s];
            parent[i] = p;
        }
        cnt[0] += (unsigned)__popcll(__ballot(p >= 0));
        cnt[1] += (unsigned)__popcll(__ballot(p >= 0 && p != (int)i));
    }
    mc_add_counters<2>(blk, cnt, counters, kMcNodes);  // (kMcDup follows)
}

// LIMIT = the largest |dx| + |dy| + |dz| of an edge: 1, 2, 3 for connectivity 6, 18, 26
template <int LIMIT>
__global__ __launch_bounds__(256) void k_mc_union(const MapRec* __restrict__ recs, int n, const MapRec* __restrict__ table, unsigned long long mask,
                                                  const unsigned* __restrict__ slot_idx, const int* __restrict__ rec_slot, int* parent) {
    for (long long il = (long long)blockIdx.x * 256 + threadIdx.x; il < n; il += (long long)gridDim.x * 256) {
        const int i = (int)il;
        const int s = rec_slot[i];
        if (s < 0 || slot_idx[s] != (unsigned)i) continue;  // no node, or a duplicate of its cell's representative
        const unsigned long long key = recs[i].key;
        const int ux = (int)((key >> (2 * kCellBits)) & kMcField), uy = (int)((key >> kCellBits) & kMcField), uz = (int)(key & kMcField);
        // the 13 offsets that come after (0, 0, 0) in the order x, y, z: the other half is the neighbour's business
#pragma unroll
        for (int c = 14; c < 27; ++c) {
            const int dx = c / 9 - 1, dy = (c / 3) % 3 - 1, dz = c % 3 - 1;
            if ((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz) > LIMIT) continue;
            const int vx = ux + dx, vy = uy + dy, vz = uz + dz;
            // a field that leaves 0 .. 2^21 - 1 is a cell that does not exist: it must not carry into the next field
            if ((unsigned)vx > kMcField || (unsigned)vy > kMcField || (unsigned)vz > kMcField) continue;
            const unsigned long long nkey =
                ((unsigned long long)(unsigned)vx << (2 * kCellBits)) | ((unsigned long long)(unsigned)vy << kCellBits) | (unsigned long long)(unsigned)vz;
            const unsigned long long nh = map_home(nkey, mask);
            unsigned long long nslot;
            if (!mc_find_slot(table, mask, nkey, nh, map_peek(table, nh), nslot)) continue;
            const unsigned j = slot_idx[nslot];
            if (j != kMcNone) mc_unite(parent, i, (int)j);  // (a cell of the map that the list does not hold is no node)
        }
    }
}

// the next `want` numbers of a wave-wide allocation (every lane of the wave must call)
__device__ __forceinline__ int mc_wave_alloc(bool want, unsigned long long* counter) {
    const unsigned long long bal = __ballot(want);
    if (!bal) return -1;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)bal) - 1;
    unsigned long long base = 0ull;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(bal));
    const int b = __shfl((int)base, leader, 64);
    return want ? b + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
}

__global__ __launch_bounds__(256) void k_mc_flatten(int n, int* parent, int* __restrict__ aux, McAcc* __restrict__ acc, unsigned* __restrict__ val_in,
                                                    unsigned long long* counters) {
    const long long bound = ((long long)n + 255) & ~255ll;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < bound; i += (long long)gridDim.x * 256) {
        int r = -1;
        if (i < n) {
            int x = mc_load(parent, i);
            if (x >= 0) {
                for (;;) {
                    const int p = mc_load(parent, x);
                    if (p == x) break;
                    x = p;
                }
                r = x;
                if (r != (int)i) parent[i] = r;  // (another walk that passes here meets an ancestor either way)
            }
        }
        const bool root = r >= 0 && r == (int)i;
        const int t = mc_wave_alloc(root, &counters[kMcComponents]);
        if (root) {
            aux[i] = t;
            val_in[t] = (unsigned)t;
            McAcc a;
            a.cnt = 0u;
            a.first = (unsigned)i;
            a.mn[0] = a.mn[1] = a.mn[2] = kMcNone;
            a.mx[0] = a.mx[1] = a.mx[2] = 0u;
            acc[t] = a;
        }
    }
}

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned w = (unsigned)__shfl_xor((int)v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned w = (unsigned)__shfl_xor((int)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the slot of `tag` in a workgroup's LDS table, -1 when the probes are used up (the caller then adds to the global words itself)
__device__ __forceinline__ int mc_lds_slot(int* tags, int tag) {
    const unsigned h = ((unsigned)tag * 2654435761u) >> 23;
    for (int probe = 0; probe < kMcLdsProbes; ++probe) {
        const int s = (int)((h + probe) & (kMcLdsSlots - 1));
        int cur = tags[s];
        if (cur == -1) cur = atomicCAS(&tags[s], -1, tag);
        if (cur == -1 || cur == tag) return s;
    }
    return -1;
}

struct McLds {
    int tag[kMcLdsSlots];
    unsigned cnt[kMcLdsSlots];
    unsigned long long key[kMcLdsSlots];
    unsigned mn[3][kMcLdsSlots], mx[3][kMcLdsSlots];
};

__device__ __forceinline__ void mc_global_add(McAcc* acc, unsigned long long* key_in, int t, unsigned cnt, unsigned long long key, const unsigned (&mn)[3],
                                              const unsigned (&mx)[3]) {
    atomicAdd(&acc[t].cnt, cnt);
    atomicMin(&key_in[t], key);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        atomicMin(&acc[t].mn[k], mn[k]);
        atomicMax(&acc[t].mx[k], mx[k]);
    }
}

__device__ __forceinline__ void mc_lds_add(McLds& L, McAcc* acc, unsigned long long* key_in, int t, unsigned cnt, unsigned long long key,
                                           const unsigned (&mn)[3], const unsigned (&mx)[3]) {
    const int s = mc_lds_slot(L.tag, t);
    if (s < 0) {
        mc_global_add(acc, key_in, t, cnt, key, mn, mx);
        return;
    }
    atomicAdd(&L.cnt[s], cnt);
    atomicMin(&L.key[s], key);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        atomicMin(&L.mn[k][s], mn[k]);
        atomicMax(&L.mx[k][s], mx[k]);
    }
}

__global__ __launch_bounds__(256) void k_mc_reduce(const MapRec* __restrict__ recs, int n, const int* __restrict__ parent, const int* __restrict__ aux,
                                                   McAcc* acc, unsigned long long* key_in) {
    __shared__ McLds L;
    for (int s = threadIdx.x; s < kMcLdsSlots; s += 256) {
        L.tag[s] = -1;
        L.cnt[s] = 0u;
        L.key[s] = kEmpty;
        L.mn[0][s] = L.mn[1][s] = L.mn[2][s] = kMcNone;
        L.mx[0][s] = L.mx[1][s] = L.mx[2][s] = 0u;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long base = (long long)blockIdx.x * kMcChunk;
#pragma unroll 2
    for (int r = 0; r < kMcChunk / 256; ++r) {
        const long long i = base + r * 256 + threadIdx.x;
        int t = -1;
        unsigned long long key = kEmpty;
        if (i < n) {
            const int root = parent[i];
            if (root >= 0) {
                t = aux[root];
                key = recs[i].key;
            }
        }
        bool todo = t >= 0;
        unsigned mn[3] = {(unsigned)(key >> (2 * kCellBits)) & kMcField, (unsigned)(key >> kCellBits) & kMcField, (unsigned)key & kMcField};
        unsigned mx[3] = {mn[0], mn[1], mn[2]};
        // the root of the wave's first live lane: when it owns many lanes (one component holds most of the list) they are reduced here
        const unsigned long long live = __ballot(todo);
        if (live) {
            const int first = __ffsll((long long)live) - 1;
            const int t0 = __builtin_amdgcn_readlane(t, first);
            const bool mine = todo && t == t0;
            const unsigned long long grp = __ballot(mine);
            if (__popcll(grp) >= kMcWaveGroup) {
                const unsigned long long gk = wave_min_u64(mine ? key : kEmpty);
                unsigned gmn[3], gmx[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    gmn[k] = wave_min_u32(mine ? mn[k] : kMcNone);
                    gmx[k] = wave_max_u32(mine ? mx[k] : 0u);
                }
                if (lane == first) mc_lds_add(L, acc, key_in, t0, (unsigned)__popcll(grp), gk, gmn, gmx);
                if (mine) todo = false;
            }
        }
        if (todo) mc_lds_add(L, acc, key_in, t, 1u, key, mn, mx);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kMcLdsSlots; s += 256) {
        const int t = L.tag[s];
        if (t < 0) continue;
        const unsigned mn[3] = {L.mn[0][s], L.mn[1][s], L.mn[2][s]}, mx[3] = {L.mx[0][s], L.mx[1][s], L.mx[2][s]};
        mc_global_add(acc, key_in, t, L.cnt[s], L.key[s], mn, mx);
    }
}

__global__ __launch_bounds__(256) void k_mc_table(const unsigned long long* __restrict__ key_out, const unsigned* __restrict__ val_out,
                                                  const McAcc* __restrict__ acc, unsigned* __restrict__ rank_of, scvod_map_component* __restrict__ out,
                                                  long long cap, int64_t* d_n, int ranked, unsigned long long* counters) {
    const long long comps = (long long)counters[kMcComponents];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (d_n) *d_n = (int64_t)comps;
        counters[kMcWritten] = out ? (unsigned long long)(comps < cap ? comps : cap) : 0ull;
        counters[kMcOverflow] = (out && comps > cap) ? 1ull : 0ull;
    }
    if (!ranked) return;
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < comps; r += (long long)gridDim.x * 256) {
        const unsigned t = val_out[r];
        rank_of[t] = (unsigned)r;
        if (out && r < cap) {
            const McAcc a = acc[t];
            scvod_map_component c;
            c.key = key_out[r];
            c.n_records = (int32_t)a.cnt;
            c.first_record = (int32_t)a.first;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                c.cell_min[k] = (int32_t)a.mn[k] - kCellBias;
                c.cell_max[k] = (int32_t)a.mx[k] - kCellBias;
            }
            c.reserved[0] = c.reserved[1] = 0;
            out[r] = c;
        }
    }
}

__global__ __launch_bounds__(256) void k_mc_assign(int n, const int* __restrict__ parent, const int* __restrict__ aux, const unsigned* __restrict__ rank_of,
                                                   int32_t* __restrict__ component) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int root = parent[i];
        component[i] = root >= 0 ? (int32_t)rank_of[aux[root]] : -1;
    }
}

// ---- the vote ----

struct MvJob {
    const int32_t* comp;
    int n;
    const int64_t* d_n;
    long long cap_components;  // already clipped to the accumulators the scratch holds
    long long cap_given;       // the caller's cap_components
    const uint8_t* verdict;
    const uint16_t* votes;
    scvod_component_visibility_params p;
    scvod_component_visibility* rec;
    long long cap_records;
    uint8_t* out;
    MvAcc* acc;
    unsigned long long* counters;
};

// components that take part: those the list's indices may name, the caller's cap and the accumulators allow
__device__ __forceinline__ long long mv_limit(const MvJob& J) {
    const long long dn = (long long)J.d_n[0];
    return dn < 0 ? 0 : (dn < J.cap_components ? dn : J.cap_components);
}

__global__ __launch_bounds__(256) void k_mcv_clear(MvJob J) {
    const long long lim = mv_limit(J);
    unsigned long long* w = reinterpret_cast<unsigned long long*>(J.acc);
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < lim * (long long)(sizeof(MvAcc) / 8); k += (long long)gridDim.x * 256) w[k] = 0ull;
}

struct MvLds {
    int tag[kMcLdsSlots];
    unsigned n[kMcLdsSlots], keep[kMcLdsSlots], seen[kMcLdsSlots];
    unsigned long long sum[4][kMcLdsSlots];
};

__device__ __forceinline__ void mv_global_add(MvAcc* acc, int c, unsigned n, unsigned keep, unsigned seen, const unsigned long long (&sum)[4]) {
    atomicAdd(&acc[c].n, n);
    if (keep) atomicAdd(&acc[c].keep, keep);
    if (seen) atomicAdd(&acc[c].seen, seen);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (sum[k]) atomicAdd(&acc[c].sum[k], sum[k]);
}

__device__ __forceinline__ void mv_lds_add(MvLds& L, MvAcc* acc, int c, unsigned n, unsigned keep, unsigned seen, const unsigned long long (&sum)[4]) {
    const int s = mc_lds_slot(L.tag, c);
    if (s < 0) {
        mv_global_add(acc, c, n, keep, seen, sum);
        return;
    }
    atomicAdd(&L.n[s], n);
    if (keep) atomicAdd(&L.keep[s], keep);
    if (seen) atomicAdd(&L.seen[s], seen);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (sum[k]) atomicAdd(&L.sum[k][s], sum[k]);
}

__global__ __launch_bounds__(256) void k_mcv_count(MvJob J) {
    __shared__ MvLds L;
    for (int s = threadIdx.x; s < kMcLdsSlots; s += 256) {
        L.tag[s] = -1;
        L.n[s] = L.keep[s] = L.seen[s] = 0u;
        L.sum[0][s] = L.sum[1][s] = L.sum[2][s] = L.sum[3][s] = 0ull;
    }
    __syncthreads();
    const long long lim = mv_limit(J);
    const int lane = threadIdx.x & 63;
    const long long base = (long long)blockIdx.x * kMcChunk;
#pragma unroll 2
    for (int r = 0; r < kMcChunk / 256; ++r) {
        const long long i = base + r * 256 + threadIdx.x;
        int c = -1;
        unsigned v = 0u;
        unsigned long long sum[4] = {0ull, 0ull, 0ull, 0ull};
        if (i < J.n) {
            c = J.comp[i];
            if (c < 0 || (long long)c >= lim) c = -1;
            if (c >= 0) {
                v = J.verdict[i];
                if (J.votes) {
                    const ushort4 q = *reinterpret_cast<const ushort4*>(J.votes + 4 * i);
                    sum[0] = q.x, sum[1] = q.y, sum[2] = q.z, sum[3] = q.w;
                }
            }
        }
        bool todo = c >= 0;
        const bool keep = todo && v == (unsigned)SCVOD_VIS_KEEP, seen = todo && v == (unsigned)SCVOD_VIS_SEEN_THROUGH;
        const unsigned long long live = __ballot(todo);
        if (live) {
            const int first = __ffsll((long long)live) - 1;
            const int c0 = __builtin_amdgcn_readlane(c, first);
            const bool mine = todo && c == c0;
            const unsigned long long grp = __ballot(mine);
            if (__popcll(grp) >= kMcWaveGroup) {
                const unsigned gk = (unsigned)__popcll(__ballot(mine && keep)), gs = (unsigned)__popcll(__ballot(mine && seen));
                unsigned long long gsum[4] = {0ull, 0ull, 0ull, 0ull};
                if (J.votes) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) gsum[k] = wave_sum_u64(mine ? sum[k] : 0ull);
                }
                if (lane == first) mv_lds_add(L, J.acc, c0, (unsigned)__popcll(grp), gk, gs, gsum);
                if (mine) todo = false;
            }
        }
        if (todo) mv_lds_add(L, J.acc, c, 1u, keep ? 1u : 0u, seen ? 1u : 0u, sum);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kMcLdsSlots; s += 256) {
        const int c = L.tag[s];
        if (c < 0) continue;
        const unsigned long long sum[4] = {L.sum[0][s], L.sum[1][s], L.sum[2][s], L.sum[3][s]};
        mv_global_add(J.acc, c, L.n[s], L.keep[s], L.seen[s], sum);
    }
}

__global__ __launch_bounds__(256) void k_mcv_decide(MvJob J) {
    __shared__ unsigned long long blk[4];
    if (threadIdx.x < 4) blk[threadIdx.x] = 0ull;
    __syncthreads();
    const long long dn = (long long)J.d_n[0] < 0 ? 0 : (long long)J.d_n[0];
    const long long lim = mv_limit(J);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        J.counters[kMvComponents] = (unsigned long long)dn;
        J.counters[kMvWritten] = J.rec ? (unsigned long long)(lim < J.cap_records ? lim : J.cap_records) : 0ull;
        J.counters[kMvBeyond] = (unsigned long long)(dn > J.cap_given ? dn - J.cap_given : 0);
        J.counters[kMvOverflow] = (J.rec && lim > J.cap_records) ? 1ull : 0ull;
    }
    unsigned long long st[4] = {0ull, 0ull, 0ull, 0ull};  // voted, seen, moved to seen, moved to keep
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < lim; c += (long long)gridDim.x * 256) {
        const MvAcc a = J.acc[c];
        const bool pool = (J.p.flags & SCVOD_CMPVIS_POOL_PAIRS) != 0;
        const long long t = pool ? (long long)a.sum[0] : (long long)a.seen, g = pool ? (long long)a.sum[1] : (long long)a.keep;
        const bool votes = (long long)a.n >= (long long)J.p.min_cells && (J.p.max_cells == 0 || (long long)a.n <= (long long)J.p.max_cells) &&
                           (long long)a.keep + (long long)a.seen >= (long long)J.p.min_tested;
        const bool through = t >= (long long)J.p.min_through && t * (long long)J.p.vote_den >= (long long)J.p.vote_num * (t + g);
        const int verdict = votes ? (through ? SCVOD_VIS_SEEN_THROUGH : SCVOD_VIS_KEEP) : -1;
        J.acc[c].verdict = votes ? (unsigned)verdict : 0u;
        if (votes) {
            ++st[0];
            if (through) {
                ++st[1];
                st[2] += (unsigned long long)(a.n - a.seen);
            } else {
                st[3] += (unsigned long long)(a.n - a.keep);
            }
        }
        if (J.rec && c < J.cap_records) {
            scvod_component_visibility r;
            r.n_records = (int32_t)a.n;
            r.n_untested = (int32_t)(a.n - a.keep - a.seen);
            r.n_keep = (int32_t)a.keep;
            r.n_seen = (int32_t)a.seen;
            r.sum_through = (int64_t)a.sum[0];
            r.sum_agree = (int64_t)a.sum[1];
            r.sum_occluded = (int64_t)a.sum[2];
            r.sum_empty = (int64_t)a.sum[3];
            r.verdict = verdict;
            r.how = votes ? 1 : 0;
            r.reserved[0] = r.reserved[1] = 0;
            J.rec[c] = r;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long w = wave_sum_u64(st[k]);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(&blk[k], w);
    }
    __syncthreads();
    if (threadIdx.x < 4 && blk[threadIdx.x]) atomicAdd(&J.counters[kMvVoted + threadIdx.x], blk[threadIdx.x]);  // kMvVoted .. kMvMovedKeep
}

__global__ __launch_bounds__(256) void k_mcv_apply(MvJob J) {
    const long long lim = mv_limit(J);
    const bool in_place = J.out == J.verdict;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < J.n; i += (long long)gridDim.x * 256) {
        const int c = J.comp[i];
        const uint8_t v = J.verdict[i];  // (in place: read by the one thread that may write it)
        uint8_t nv = v;
        if (c >= 0 && (long long)c < lim) {
            const unsigned cv = J.acc[c].verdict;
            if (cv) nv = (uint8_t)cv;
        }
        if (!in_place || nv != v) J.out[i] = nv;
    }
}

size_t mc_align(size_t b) { return (b + 255) & ~(size_t)255; }

size_t mc_sort_bytes(long long n) {
    size_t bytes = 0;
    rocprim::radix_sort_pairs(nullptr, bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, (size_t)n, 0,
                              64, (hipStream_t)0);
    return bytes;
}

unsigned mc_blocks(long long items) {
    const long long b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > (long long)kMcMaxBlocks ? (long long)kMcMaxBlocks : b));
}

bool mc_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace
}  // namespace scvod

extern "C" {

int scvod_map_components(scvod_map* m, const void* d_records, int64_t n, int32_t connectivity, int32_t* d_component, void* d_table, int64_t cap_table,
                         int64_t* d_n, void* stream) {
    if (!m) return SCVOD_ERR_INVALID;
    if (n < 0 || n > 0x7FFFFFFFll) return mfail(m, SCVOD_ERR_INVALID, "n = %lld outside 0 .. 2^31 - 1", (long long)n);
    if (n > 0 && !d_records) return mfail(m, SCVOD_ERR_INVALID, "NULL records of a list that is not empty");
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return mfail(m, SCVOD_ERR_INVALID, "connectivity %d is not 6, 18 or 26", connectivity);
    if (((uintptr_t)d_records & 7u) || ((uintptr_t)d_table & 7u) || ((uintptr_t)d_n & 7u) || ((uintptr_t)d_component & 3u))
        return mfail(m, SCVOD_ERR_INVALID, "a misaligned pointer (records, table, d_n: 8 bytes; d_component: 4)");
    if (cap_table < 0) return mfail(m, SCVOD_ERR_INVALID, "cap_table < 0");
    if (d_table && !d_n) return mfail(m, SCVOD_ERR_INVALID, "a table needs d_n");
    {
        const void* p[4] = {d_records, d_component, d_table, d_n};
        const size_t b[4] = {16 * (size_t)n, 4 * (size_t)n, sizeof(scvod_map_component) * (size_t)cap_table, sizeof(int64_t)};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
                if (mc_overlap(p[i], b[i], p[j], b[j])) return mfail(m, SCVOD_ERR_INVALID, "the outputs overlap the records or each other");
    }
    if (m->capacity > (1ll << 30)) return mfail(m, SCVOD_ERR_INVALID, "a map of more than 2^30 slots");
    MHIP(m, hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)n, C = (size_t)m->capacity;
    const bool ranked = (d_component || d_table) && n > 0;
    const size_t sort_bytes = n > 0 ? mc_sort_bytes(n) : 0;
    // counters | slot_idx | rec_slot / aux | parent | sort keys in, out | sort values in, out | accumulators | rocprim's temporary storage
    size_t off = mc_align(sizeof(unsigned long long) * kMcWords);
    const size_t off_slot = off;
    off += mc_align(4 * C);
    const size_t off_aux = off;
    off += mc_align(4 * N);
    const size_t off_parent = off;
    off += mc_align(4 * N);
    const size_t off_kin = off;
    off += mc_align(8 * N);
    const size_t off_kout = off;
    off += mc_align(8 * N);
    const size_t off_vin = off;
    off += mc_align(4 * N);
    const size_t off_vout = off;
    off += mc_align(4 * N);
    const size_t off_acc = off;
    off += mc_align(sizeof(McAcc) * N);
    const size_t off_tmp = off;
    off += mc_align(sort_bytes);
    if (m->c_cap < off) {  // grow-only; the old block may still be read by work in flight
        MHIP(m, hipStreamSynchronize(st));
        if (m->c_ran && m->c_stream != st) MHIP(m, hipStreamSynchronize(m->c_stream));
        if (m->c_buf) hipFree(m->c_buf);
        m->c_buf = nullptr;
        m->c_cap = 0;
        MHIP(m, hipMalloc(&m->c_buf, off));
        m->c_cap = off;
    }
    unsigned long long* counters = (unsigned long long*)m->c_buf;
    unsigned* slot_idx = (unsigned*)(m->c_buf + off_slot);
    int* aux = (int*)(m->c_buf + off_aux);
    int* parent = (int*)(m->c_buf + off_parent);
    unsigned long long *key_in = (unsigned long long*)(m->c_buf + off_kin), *key_out = (unsigned long long*)(m->c_buf + off_kout);
    unsigned *val_in = (unsigned*)(m->c_buf + off_vin), *val_out = (unsigned*)(m->c_buf + off_vout);
    McAcc* acc = (McAcc*)(m->c_buf + off_acc);
    m->c_records = (long long)n;
    m->c_stream = st;
    m->c_ran = true;
    MHIP(m, hipMemsetAsync(counters, 0, sizeof(unsigned long long) * kMcWords, st));
    const MapRec* recs = (const MapRec*)d_records;
    const unsigned long long mask = (unsigned long long)(m->capacity - 1);
    const int ni = (int)n;
    if (n > 0) {
        MHIP(m, hipMemsetAsync(slot_idx, 0xff, 4 * C, st));
        MHIP(m, hipMemsetAsync(key_in, 0xff, 8 * N, st));
        const unsigned blocks = mc_blocks(n);
        hipLaunchKernelGGL(k_mc_slots, dim3(blocks), dim3(256), 0, st, recs, ni, m->table, mask, slot_idx, aux, counters);
        hipLaunchKernelGGL(k_mc_init, dim3(blocks), dim3(256), 0, st, ni, slot_idx, aux, parent, counters);
        if (connectivity == 6)
            hipLaunchKernelGGL(k_mc_union<1>, dim3(blocks), dim3(256), 0, st, recs, ni, m->table, mask, slot_idx, aux, parent);
        else if (connectivity == 18)
            hipLaunchKernelGGL(k_mc_union<2>, dim3(blocks), dim3(256), 0, st, recs, ni, m->table, mask, slot_idx, aux, parent);
        else
            hipLaunchKernelGGL(k_mc_union<3>, dim3(blocks), dim3(256), 0, st, recs, ni, m->table, mask, slot_idx, aux, parent);
        hipLaunchKernelGGL(k_mc_flatten, dim3(blocks), dim3(256), 0, st, ni, parent, aux, acc, val_in, counters);
        if (ranked) {
            hipLaunchKernelGGL(k_mc_reduce, dim3((unsigned)((n + kMcChunk - 1) / kMcChunk)), dim3(256), 0, st, recs, ni, parent, aux, acc, key_in);
            size_t bytes = sort_bytes;
            const hipError_t e = rocprim::radix_sort_pairs(m->c_buf + off_tmp, bytes, key_in, key_out, val_in, val_out, N, 0, 64, st);
            if (e != hipSuccess) return mfail(m, SCVOD_ERR_HIP, "rocprim::radix_sort_pairs: %s", hipGetErrorString(e));
        }
    }
    // (after the sort val_in is free: it takes the rank of every temporary number)
    hipLaunchKernelGGL(k_mc_table, dim3(n > 0 ? mc_blocks(n) : 1u), dim3(256), 0, st, key_out, val_out, acc, val_in, (scvod_map_component*)d_table,
                       (long long)cap_table, d_n, ranked ? 1 : 0, counters);
    if (ranked && d_component) hipLaunchKernelGGL(k_mc_assign, dim3(mc_blocks(n)), dim3(256), 0, st, ni, parent, aux, val_in, d_component);
    MHIP(m, hipGetLastError());
    return SCVOD_OK;
}

int scvod_map_components_stats(scvod_map* m, int64_t* h_out8) {
    if (!m || !h_out8) return mfail(m, SCVOD_ERR_INVALID, "bad arguments");
    if (!m->c_ran) return mfail(m, SCVOD_ERR_STATE, "scvod_map_components_stats before the first scvod_map_components");
    MHIP(m, hipSetDevice(m->device));
    MHIP(m, hipStreamSynchronize(m->c_stream));
    unsigned long long h[kMcWords];
    MHIP(m, hipMemcpy(h, m->c_buf, sizeof(h), hipMemcpyDeviceToHost));
    h_out8[0] = (int64_t)m->c_records;
    h_out8[1] = (int64_t)h[kMcNodes];
    h_out8[2] = (int64_t)h[kMcPadding];
    h_out8[3] = (int64_t)h[kMcAbsent];
    h_out8[4] = (int64_t)h[kMcDup];
    h_out8[5] = (int64_t)h[kMcComponents];
    h_out8[6] = (int64_t)h[kMcWritten];
    h_out8[7] = (int64_t)h[kMcOverflow];
    if (h[kMcOverflow]) return mfail(m, SCVOD_ERR_CAPACITY, "%lld components outgrow the table", (long long)h[kMcComponents]);
    return SCVOD_OK;
}

int64_t scvod_map_components_scratch_bytes(const scvod_map* m) { return m ? (int64_t)m->c_cap : 0; }

void scvod_component_visibility_params_default(scvod_component_visibility_params* p) {
    if (!p) return;
    p->flags = 0;
    p->min_cells = 1;
    p->max_cells = 0;
    p->min_tested = 1;
    p->min_through = 2;
    p->vote_num = 1;
    p->vote_den = 2;
    p->reserved = 0;
}

int scvod_map_component_visibility(scvod_map* m, const int32_t* d_component, int64_t n, const int64_t* d_n, int64_t cap_components,
                                   const uint8_t* d_verdict, const uint16_t* d_votes, const scvod_component_visibility_params* params, void* d_records,
                                   int64_t cap_records, uint8_t* d_verdict_out, void* stream) {
    if (!m) return SCVOD_ERR_INVALID;
    if (n < 0 || n > 0x7FFFFFFFll) return mfail(m, SCVOD_ERR_INVALID, "n = %lld outside 0 .. 2^31 - 1", (long long)n);
    if (!d_n) return mfail(m, SCVOD_ERR_INVALID, "NULL d_n");
    if (n > 0 && (!d_component || !d_verdict)) return mfail(m, SCVOD_ERR_INVALID, "NULL d_component or d_verdict of a list that is not empty");
    if (cap_components < 0 || cap_records < 0) return mfail(m, SCVOD_ERR_INVALID, "a negative capacity");
    scvod_component_visibility_params p;
    scvod_component_visibility_params_default(&p);
    if (params) p = *params;
    if ((p.flags & ~SCVOD_CMPVIS_POOL_PAIRS) || p.reserved != 0) return mfail(m, SCVOD_ERR_INVALID, "an unknown flag bit, or reserved != 0");
    if (p.min_cells < 1 || p.max_cells < 0 || p.min_tested < 1) return mfail(m, SCVOD_ERR_INVALID, "min_cells < 1, max_cells < 0 or min_tested < 1");
    if (p.vote_den < 1 || p.vote_den > 4096 || p.vote_num < 0 || p.vote_num > 4096)
        return mfail(m, SCVOD_ERR_INVALID, "vote %d / %d outside 0 .. 4096 / 1 .. 4096", p.vote_num, p.vote_den);
    if ((p.flags & SCVOD_CMPVIS_POOL_PAIRS) && !d_votes) return mfail(m, SCVOD_ERR_INVALID, "SCVOD_CMPVIS_POOL_PAIRS needs d_votes");
    if (((uintptr_t)d_component & 3u) || ((uintptr_t)d_n & 7u) || ((uintptr_t)d_votes & 7u) || ((uintptr_t)d_records & 7u))
        return mfail(m, SCVOD_ERR_INVALID, "a misaligned pointer (d_component: 4 bytes; d_n, d_votes, d_records: 8)");
    {
        const size_t N = (size_t)n, rec_bytes = sizeof(scvod_component_visibility) * (size_t)cap_records;
        if (d_verdict_out != d_verdict && mc_overlap(d_verdict_out, N, d_verdict, N))
            return mfail(m, SCVOD_ERR_INVALID, "d_verdict_out overlaps d_verdict without being equal to it");
        if (mc_overlap(d_verdict_out, N, d_component, 4 * N) || mc_overlap(d_verdict_out, N, d_votes, 8 * N) || mc_overlap(d_verdict_out, N, d_records, rec_bytes) ||
            mc_overlap(d_verdict_out, N, d_n, 8) || mc_overlap(d_records, rec_bytes, d_component, 4 * N) || mc_overlap(d_records, rec_bytes, d_verdict, N) ||
            mc_overlap(d_records, rec_bytes, d_votes, 8 * N) || mc_overlap(d_records, rec_bytes, d_n, 8))
            return mfail(m, SCVOD_ERR_INVALID, "an output overlaps another argument");
    }
    MHIP(m, hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)stream;
    const long long lim = cap_components < n ? (long long)cap_components : (long long)n;  // (a list of n records names n components at the most)
    const size_t off_acc = mc_align(sizeof(unsigned long long) * kMvWords);
    const size_t need = off_acc + mc_align(sizeof(MvAcc) * (size_t)lim);
    if (m->v_cap < need) {
        MHIP(m, hipStreamSynchronize(st));
        if (m->v_ran && m->v_stream != st) MHIP(m, hipStreamSynchronize(m->v_stream));
        if (m->v_buf) hipFree(m->v_buf);
        m->v_buf = nullptr;
        m->v_cap = 0;
        MHIP(m, hipMalloc(&m->v_buf, need));
        m->v_cap = need;
    }
    m->v_stream = st;
    m->v_ran = true;
    MvJob J;
    J.comp = d_component;
    J.n = (int)n;
    J.d_n = d_n;
    J.cap_components = lim;
    J.cap_given = (long long)cap_components;
    J.verdict = d_verdict;
    J.votes = d_votes;
    J.p = p;
    J.rec = (scvod_component_visibility*)d_records;
    J.cap_records = (long long)cap_records;
    J.out = d_verdict_out;
    J.acc = (MvAcc*)(m->v_buf + off_acc);
    J.counters = (unsigned long long*)m->v_buf;
    MHIP(m, hipMemsetAsync(J.counters, 0, sizeof(unsigned long long) * kMvWords, st));
    const unsigned cblocks = mc_blocks(lim > 0 ? lim : 1);
    hipLaunchKernelGGL(k_mcv_clear, dim3(cblocks), dim3(256), 0, st, J);
    if (n > 0 && lim > 0) hipLaunchKernelGGL(k_mcv_count, dim3((unsigned)((n + kMcChunk - 1) / kMcChunk)), dim3(256), 0, st, J);
    hipLaunchKernelGGL(k_mcv_decide, dim3(cblocks), dim3(256), 0, st, J);
    if (n > 0 && d_verdict_out) hipLaunchKernelGGL(k_mcv_apply, dim3(mc_blocks(n)), dim3(256), 0, st, J);
    MHIP(m, hipGetLastError());
    return SCVOD_OK;
}

int scvod_map_component_visibility_stats(scvod_map* m, int64_t* h_out8) {
    if (!m || !h_out8) return mfail(m, SCVOD_ERR_INVALID, "bad arguments");
    if (!m->v_ran) return mfail(m, SCVOD_ERR_STATE, "scvod_map_component_visibility_stats before the first scvod_map_component_visibility");
    MHIP(m, hipSetDevice(m->device));
    MHIP(m, hipStreamSynchronize(m->v_stream));
    unsigned long long h[kMvWords];
    MHIP(m, hipMemcpy(h, m->v_buf, sizeof(h), hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; ++i) h_out8[i] = (int64_t)h[i];
    if (h[kMvOverflow]) return mfail(m, SCVOD_ERR_CAPACITY, "%lld components outgrow the records", (long long)h[kMvComponents]);
    return SCVOD_OK;
}

}  // extern "C"
