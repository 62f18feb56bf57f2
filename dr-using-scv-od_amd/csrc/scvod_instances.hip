// scvod_instances.hip -- the points of a labelled cloud grouped by their 32-bit label and counted per group, on the device (gfx950):
// scvod_score_instances_device.
//
// Reference analogue: tool/plotIoU.py:70-84 prints, per sequence, how many high-dynamic objects the truth holds and how many were
// removed, how many low-dynamic ones and how many were retained.  No program of the reference computes them; the object rule is this
// project's and lives on the host (scvod_instance_finish).  The device part is a group-by with integer sums:
//     k_in_aggregate   a 256-thread workgroup walks consecutive tiles of kExpTile points, four consecutive points per lane and round.
//                      Equal keys of a wave are combined before they touch memory: take the key of the first point with work, ballot
//                      the points that hold it, popcount the three flags, take the lowest index, repeat until no point is left.  The
//                      sums of round r wait in lane r; once per tile the lanes add them side by side into a table in LDS (open
//                      addressing, kInLdsSlots slots of 24 bytes: tag, three counts, first index).  A key that finds no slot within kInLdsProbes probes goes straight to the global table and the tile
//                      counts as spilled.  After its last tile the workgroup flushes its occupied slots to the global table
//     global table     open addressing over a power of two of slots >= 2 * cap_instances, cleared by a memset.  A slot's tag is the key
//                      with bit 32 set, claimed with a 64-bit compare-and-swap: 0 is empty for all 2^32 keys.  Counts: 64-bit atomicAdd;
//                      first index: atomicMax of (INT32_MAX - index), so that the memset's 0 is "none"
//     k_in_compact     occupied slots -> a dense list (key, slot) of at most cap_instances entries, one atomic per wave, order arbitrary
//     sort             rocprim::radix_sort_pairs over cap_instances entries on bits 0..32; the entries behind the list hold all ones
//     k_in_gather      the records in key order, d_n and the four stats words
// All sums are integers and first_point is a minimum: the result depends on neither the order of the points, the tile schedule nor
// the slot order.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "scvod_grid.h"

namespace scvod {
namespace {

constexpr int kInLdsSlots = 1024;  // 24 KB: six workgroups share a CU's LDS
constexpr int kInLdsProbes = 16;
constexpr unsigned long long kInTagBit = 1ull << 32;
constexpr unsigned kInFirstBase = 0x7FFFFFFFu;

struct InSlot {  // 40 bytes, all zero when empty
    unsigned long long tag, n_points, n_inlier, n_preserved;
    unsigned inv_first, pad;
};

// counter words: [0..3] what scvod_score_instances_stats returns (written by k_in_gather), [4] occupied slots, [5] the global table
// was full for some key, [6] spilled tiles
enum { kInWritten = 0, kInDistinct, kInOverflow, kInSpilled, kInFound, kInFull, kInSpillRaw };

__device__ __forceinline__ unsigned in_hash(uint32_t key) { return key * 2654435761u; }

__device__ void in_global_add(InSlot* table, unsigned mask, uint32_t key, unsigned long long n, unsigned long long inl, unsigned long long pre,
                              unsigned first, unsigned long long* counters) {
    const unsigned long long tag = kInTagBit | key;
    const unsigned h = in_hash(key) >> 9;  // (the table has 2^23 slots at the most)
    for (unsigned probe = 0; probe <= mask; ++probe) {
        InSlot* s = table + ((h + probe) & mask);
        unsigned long long cur = __hip_atomic_load(&s->tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) cur = atomicCAS(&s->tag, 0ull, tag);
        if (cur == 0ull || cur == tag) {
            atomicAdd(&s->n_points, n);
            if (inl) atomicAdd(&s->n_inlier, inl);
            if (pre) atomicAdd(&s->n_preserved, pre);
            atomicMax(&s->inv_first, kInFirstBase - first);
            return;
        }
        // a table that was full once makes the call an overflow whatever follows: no need to walk it again and again
        if ((probe & 63u) == 63u && __hip_atomic_load(&counters[kInFull], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
    atomicOr(&counters[kInFull], 1ull);
}

constexpr int kInBlockTiles = 2048;  // a workgroup walks this many tiles at the most (launch_instance_score sizes the grid)

struct InLds {
    unsigned long long tag[kInLdsSlots];
    unsigned n[kInLdsSlots], inl[kInLdsSlots], pre[kInLdsSlots], first[kInLdsSlots];
    unsigned spilled[kInBlockTiles / 32];  // one bit per tile of the workgroup
};

// one lane of a wave: the sums of one key into the workgroup's table, or past it (tile: the workgroup's own count)
__device__ __forceinline__ void in_lds_add(InLds& L, uint32_t key, unsigned n, unsigned inl, unsigned pre, unsigned first, int tile,
                                           InSlot* table, unsigned mask, unsigned long long* counters) {
    const unsigned long long tag = kInTagBit | key;
    const unsigned h = in_hash(key) >> 22;
    for (int probe = 0; probe < kInLdsProbes; ++probe) {
        const unsigned s = (h + probe) & (kInLdsSlots - 1);
        unsigned long long cur = L.tag[s];
        if (cur == 0ull) cur = atomicCAS(&L.tag[s], 0ull, tag);
        if (cur == 0ull || cur == tag) {
            atomicAdd(&L.n[s], n);
            if (inl) atomicAdd(&L.inl[s], inl);
            if (pre) atomicAdd(&L.pre[s], pre);
            atomicMin(&L.first[s], first);
            return;
        }
    }
    const unsigned bit = 1u << (tile & 31);
    if (!(atomicOr(&L.spilled[(tile >> 5) & (kInBlockTiles / 32 - 1)], bit) & bit)) atomicAdd(&counters[kInSpillRaw], 1ull);
    in_global_add(table, mask, key, n, inl, pre, first, counters);
}

// a lane's share of a tile: two rounds of four consecutive points
struct InTile {
    uint32_t k[2][4];
    unsigned f[2], valid[2];  // the four result bytes; bit e: point e exists
};

template <bool VEC>
__device__ __forceinline__ InTile in_load(const uint32_t* __restrict__ key, const uint8_t* __restrict__ res, int n, int tile) {
    InTile t;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const long long p = (long long)tile * kExpTile + u * 1024 + threadIdx.x * 4;
        t.k[u][0] = t.k[u][1] = t.k[u][2] = t.k[u][3] = 0u;
        t.f[u] = 0u;
        if (VEC && p + 3 < n) {
            const uint4 kk = *reinterpret_cast<const uint4*>(key + p);
            t.k[u][0] = kk.x, t.k[u][1] = kk.y, t.k[u][2] = kk.z, t.k[u][3] = kk.w;
            t.f[u] = *reinterpret_cast<const unsigned*>(res + p);
            t.valid[u] = 15u;
        } else {
            t.valid[u] = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p + e < n) {
                    t.k[u][e] = key[p + e];
                    t.f[u] |= (unsigned)res[p + e] << (8 * e);
                    t.valid[u] |= 1u << e;
                }
        }
    }
    return t;
}

// WAVE_MATCH 0: every point adds into the LDS table on its own (the plain-atomics variant of profiles/instance_score_cost.txt)
template <bool VEC, bool WAVE_MATCH>
__global__ __launch_bounds__(256) void k_in_aggregate(const uint32_t* __restrict__ key, const uint8_t* __restrict__ res, int n, int tiles,
                                                      InSlot* table, unsigned mask, unsigned long long* counters) {
    __shared__ InLds L;
    for (int s = threadIdx.x; s < kInLdsSlots; s += 256) {
        L.tag[s] = 0ull;
        L.n[s] = L.inl[s] = L.pre[s] = 0u;
        L.first[s] = 0xFFFFFFFFu;
    }
    if (threadIdx.x < kInBlockTiles / 32) L.spilled[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // the sums of the wave's rounds wait in its lanes, round r in lane r, and go to the LDS table side by side once per tile
    int pending = 0;
    uint32_t pk = 0u;
    unsigned pn = 0u, pi = 0u, pp = 0u, pf = 0u;
    // a workgroup takes consecutive tiles: the labels of a neighbourhood come back, so its table stays small.  No barrier inside the
    // loop: the next tile's loads are in flight while this one is worked on
    const int per_block = (tiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int tile_begin = (int)blockIdx.x * per_block;
    const int tile_end = min(tiles, tile_begin + per_block);
    InTile next;
    if (tile_begin < tile_end) next = in_load<VEC>(key, res, n, tile_begin);
    for (int tile = tile_begin; tile < tile_end; ++tile) {
        const InTile t = next;
        if (tile + 1 < tile_end) next = in_load<VEC>(key, res, n, tile + 1);
        const int own = tile - tile_begin;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            // bit e of inl / pre: point e is an inlier / preserved (bit 0 set and bit 1 == bit 2: analysis.py's rule)
            const unsigned f = t.f[u];
            const unsigned inl = (f & 1u) | ((f >> 7) & 2u) | ((f >> 14) & 4u) | ((f >> 21) & 8u);
            const unsigned dif = (f >> 1) ^ (f >> 2);
            const unsigned same = ~((dif & 1u) | ((dif >> 7) & 2u) | ((dif >> 14) & 4u) | ((dif >> 21) & 8u));
            const unsigned pre = inl & same & 15u;
            const unsigned todo = t.valid[u];
            const long long p0 = (long long)tile * kExpTile + u * 1024 + threadIdx.x * 4;
            if (!WAVE_MATCH) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (todo >> e & 1u)
                        in_lds_add(L, t.k[u][e], 1u, inl >> e & 1u, pre >> e & 1u, (unsigned)(p0 + e), own, table, mask, counters);
                continue;
            }
            const long long wave_p0 = p0 - 4 * lane;  // the first point of the wave's 256
            // per element slot e the lanes whose point e is still to do, is an inlier, is preserved: wave-uniform masks, so a round costs
            // four vector compares and the rest is scalar
            unsigned long long td[4], bi[4], bp[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                td[e] = __ballot(todo >> e & 1u);
                bi[e] = __ballot(inl >> e & 1u);
                bp[e] = __ballot(pre >> e & 1u);
            }
            while ((td[0] | td[1] | td[2] | td[3]) != 0ull) {
                if (pending == 64) {
                    in_lds_add(L, pk, pn, pi, pp, pf, own, table, mask, counters);
                    pending = 0;
                }
                uint32_t k0;
                if (td[0])
                    k0 = (uint32_t)__builtin_amdgcn_readlane((int)t.k[u][0], __ffsll((long long)td[0]) - 1);
                else if (td[1])
                    k0 = (uint32_t)__builtin_amdgcn_readlane((int)t.k[u][1], __ffsll((long long)td[1]) - 1);
                else if (td[2])
                    k0 = (uint32_t)__builtin_amdgcn_readlane((int)t.k[u][2], __ffsll((long long)td[2]) - 1);
                else
                    k0 = (uint32_t)__builtin_amdgcn_readlane((int)t.k[u][3], __ffsll((long long)td[3]) - 1);
                unsigned cnt = 0u, c_inl = 0u, c_pre = 0u, first = 0xFFFFFFFFu;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned long long bm = __ballot(t.k[u][e] == k0) & td[e];
                    cnt += __popcll(bm);
                    c_inl += __popcll(bm & bi[e]);
                    c_pre += __popcll(bm & bp[e]);
                    if (bm) {
                        const unsigned cand = (unsigned)(wave_p0 + 4 * (__ffsll((long long)bm) - 1) + e);
                        first = cand < first ? cand : first;
                    }
                    td[e] &= ~bm;
                }
                if (lane == pending) pk = k0, pn = cnt, pi = c_inl, pp = c_pre, pf = first;
                ++pending;
            }
        }
        if (WAVE_MATCH) {
            if (lane < pending) in_lds_add(L, pk, pn, pi, pp, pf, own, table, mask, counters);
            pending = 0;
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kInLdsSlots; s += 256)
        if (L.tag[s]) in_global_add(table, mask, (uint32_t)L.tag[s], L.n[s], L.inl[s], L.pre[s], L.first[s], counters);
}

__global__ __launch_bounds__(256) void k_in_compact(const InSlot* __restrict__ table, unsigned slots, int cap, unsigned long long* sort_key,
                                                    unsigned* sort_val, unsigned long long* counters) {
    // whole waves enter the loop body together (the bound is rounded up to the wave), so wave_list_slot sees every lane
    const unsigned bound = (slots + 63u) & ~63u;
    for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < bound; s += gridDim.x * 256u) {
        const unsigned long long tag = s < slots ? table[s].tag : 0ull;
        const int at = wave_list_slot(tag != 0ull, reinterpret_cast<int*>(&counters[kInFound]));  // (the low word of a cleared counter)
        if (tag != 0ull && at < cap && sort_key) {
            sort_key[at] = tag & 0xFFFFFFFFull;
            sort_val[at] = s;
        }
    }
}

__global__ __launch_bounds__(256) void k_in_gather(const InSlot* __restrict__ table, const unsigned long long* __restrict__ sort_key,
                                                   const unsigned* __restrict__ sort_val, int cap, scvod_instance* out, int64_t* d_n,
                                                   unsigned long long* counters) {
    const long long found = (long long)counters[kInFound];
    const bool overflow = counters[kInFull] != 0ull || found > cap;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        counters[kInWritten] = overflow ? 0ull : (unsigned long long)found;
        counters[kInDistinct] = (unsigned long long)found;
        counters[kInOverflow] = overflow ? 1ull : 0ull;
        counters[kInSpilled] = counters[kInSpillRaw];
        *d_n = overflow ? -1 : (int64_t)found;
    }
    if (overflow || !out || i >= found) return;
    const InSlot s = table[sort_val[i]];
    scvod_instance r;
    r.label = (uint32_t)sort_key[i];
    r.first_point = (int32_t)(kInFirstBase - s.inv_first);
    r.n_points = (int64_t)s.n_points;
    r.n_inlier = (int64_t)s.n_inlier;
    r.n_preserved = (int64_t)s.n_preserved;
    out[i] = r;
}

size_t in_align(size_t b) { return (b + 255) & ~(size_t)255; }

size_t in_sort_bytes(int32_t cap) {
    size_t bytes = 0;
    rocprim::radix_sort_pairs(nullptr, bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr,
                              (size_t)cap, 0, 33, (hipStream_t)0);
    return bytes;
}

}  // namespace

uint32_t in_table_slots(int32_t cap) {
    uint32_t s = 2;
    while (s < 2u * (uint32_t)cap) s <<= 1;
    return s;
}

size_t in_work_bytes(int32_t cap) {
    // table | sort keys in, out | sort values in, out | rocprim's temporary storage
    return in_align(sizeof(InSlot) * (size_t)in_table_slots(cap)) + 2 * in_align(8 * (size_t)cap) + 2 * in_align(4 * (size_t)cap) +
           in_align(in_sort_bytes(cap));
}

int launch_instance_score(const uint32_t* key, const uint8_t* point_result, int32_t n, scvod_instance* out, int32_t cap, int64_t* d_n, void* work,
                          unsigned long long* counters, int variant, hipStream_t st) {
    const uint32_t slots = in_table_slots(cap);
    unsigned char* base = (unsigned char*)work;
    InSlot* table = (InSlot*)base;
    base += in_align(sizeof(InSlot) * (size_t)slots);
    unsigned long long* key_in = (unsigned long long*)base;
    base += in_align(8 * (size_t)cap);
    unsigned long long* key_out = (unsigned long long*)base;
    base += in_align(8 * (size_t)cap);
    unsigned* val_in = (unsigned*)base;
    base += in_align(4 * (size_t)cap);
    unsigned* val_out = (unsigned*)base;
    base += in_align(4 * (size_t)cap);
    hipMemsetAsync(table, 0, sizeof(InSlot) * (size_t)slots, st);
    hipMemsetAsync(counters, 0, sizeof(unsigned long long) * 8, st);
    if (n > 0) {
        const int tiles = (int)(((long long)n + kExpTile - 1) / kExpTile);
        // four workgroups per compute unit, all resident at once (six fit by their LDS): no second round of workgroups
        int dev = 0, cus = 0;
        hipGetDevice(&dev);
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        const int resident = 4 * (cus > 0 ? cus : 256);
        const int fewest = (tiles + kInBlockTiles - 1) / kInBlockTiles;  // (a workgroup marks its spilled tiles in kInBlockTiles bits)
        const unsigned blocks = (unsigned)(tiles < resident ? tiles : (resident > fewest ? resident : fewest));
        const bool vec = ((uintptr_t)key & 15) == 0 && ((uintptr_t)point_result & 3) == 0;
        auto kern = variant == 1 ? (vec ? k_in_aggregate<true, false> : k_in_aggregate<false, false>)
                                 : (vec ? k_in_aggregate<true, true> : k_in_aggregate<false, true>);
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, st, key, point_result, (int)n, tiles, table, slots - 1u, counters);
    }
    const unsigned cblocks = (slots + 255u) / 256u < 2048u ? (slots + 255u) / 256u : 2048u;
    if (out) hipMemsetAsync(key_in, 0xFF, 8 * (size_t)cap, st);
    hipLaunchKernelGGL(k_in_compact, dim3(cblocks), dim3(256), 0, st, table, slots, (int)cap, out ? key_in : nullptr, val_in, counters);
    if (out) {
        size_t bytes = in_sort_bytes(cap);
        const hipError_t e = rocprim::radix_sort_pairs(base, bytes, key_in, key_out, val_in, val_out, (size_t)cap, 0, 33, st);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_in_gather, dim3(out ? ((unsigned)cap + 255u) / 256u : 1u), dim3(256), 0, st, table, key_out, val_out, (int)cap, out, d_n,
                       counters);
    return 0;
}

}  // namespace scvod
