// scvod_objtruth.hip -- the truth label every object of the table covers, on the device (gfx950): scvod_batch_object_truth.
//
// Reference analogue: none.  tool/feature.py (per-class feature boxplots) and tool/plotIoU.py (object counts) hold hard-coded numbers;
// no program of the reference joins its clusters with labelled truth.  The host rule (scvod_object_truth_finish) is this project's
// convention.  The device part is a group-by with integer counts: per object of the table -- its run
// [begin[o], begin[o + 1]) of the sorted member list scvod_batch_objects left in its scratch -- the multiset of the members' 32-bit
// truth labels d_gt_label[scan base + apri_src[slot]], reduced to the label most members carry (equal counts: the smallest label), its
// count, the members of its class, the members of a moving class and the number of distinct labels.
//     k_ot_points      one streaming pass over d_gt_label: the batch's input points of a moving class (ballot + popcount, one 64-bit
//                      atomic per workgroup)
//     k_ot_objects     one wave per object, 64 members per round, the next round's gathers (key -> apri_src -> label) in flight.  Equal
//                      labels of a round are combined first (take the label of the first member left, ballot the members that hold it,
//                      popcount: k_in_aggregate's scheme); the members of a moving class are counted beside it, one ballot per round.  Lane r
//                      then adds the r-th (label, count) into the wave's own open-addressing table in LDS: kOtSlots entries of 8 bytes,
//                      count << 32 | label, so that 0 is an empty slot for all 2^32 labels.  At the end the table is reduced: the winner
//                      is the maximum of count << 32 | ~label, n_class the counts of its class.  The members are read once
//     spill            an object whose distinct labels exceed SCVOD_OBJ_TRUTH_ONCHIP_LABELS leaves the wave's table alone: the wave
//                      stops at the round in which the count passes the bound -- the table then holds at most the bound + 64 labels,
//                      fewer than its slots -- and appends the object to a list.  Whether that happens depends on the multiset alone
//     k_ot_fallback    kOtGroups workgroups, each the owner of one region of 2 * max_scan_pts slots in global memory; workgroup g
//                      takes the list entries g, g + kOtGroups, ...: it clears the 2 n slots an object of n members needs (load factor
//                      <= 0.5), inserts every member with a compare-and-swap and an add, and reduces the slots the same way.  No
//                      workgroup waits for another; the list's length is read from the device
// All results are integer counts, maxima and sums: the same bytes on every run, whatever the slot order or the list order.
#include <hip/hip_runtime.h>

#include "scvod_dev.h"

namespace scvod {
namespace {

constexpr int kOtSlots = 2 * SCVOD_OBJ_TRUTH_ONCHIP_LABELS;  // per wave: 2 KB
static_assert((kOtSlots & (kOtSlots - 1)) == 0 && kOtSlots >= SCVOD_OBJ_TRUTH_ONCHIP_LABELS + 64 + 1 && kOtSlots % 64 == 0,
              "the wave's table must hold the bound plus one round of new labels with a slot to spare");

typedef unsigned long long ot_u64;

__device__ __forceinline__ unsigned ot_hash(uint32_t label) { return (label ^ (label >> 15)) * 2654435761u; }

__device__ __forceinline__ bool ot_moving(const EvClasses& K, uint32_t label) {
    const uint16_t sem = (uint16_t)(label & 0xFFFFu);
    bool m = false;
    for (int k = 0; k < K.n; ++k) m |= sem == K.c[k];
    return m;
}

// the label of slot p of the sorted member list (p < e), else 0
__device__ __forceinline__ uint32_t ot_load(const Arena& A, const uint64_t* __restrict__ key_out, const uint32_t* __restrict__ gt, int p, int e,
                                            int scan_base, int scan_n) {
    uint32_t lab = 0u;
    if (p < e) {
        const uint32_t g = (uint32_t)key_out[p];
        const int src = A.apri_src[g];
        if ((unsigned)src < (unsigned)scan_n) lab = gt[(size_t)scan_base + src];
    }
    return lab;
}

__device__ __forceinline__ ot_u64 wave_max_u64(ot_u64 v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const ot_u64 o = (ot_u64)__shfl_xor((long long)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the scan that holds batch slot g0: the last s with scan_off[s] <= g0
__device__ __forceinline__ int ot_scan_of(const Arena& A, int n_scans, int g0) {
    int lo = 0, hi = n_scans;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.scan_off[mid] <= g0) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_ot_points(const uint32_t* __restrict__ gt, long long n, EvClasses K, ot_u64* counters) {
    __shared__ int wcnt[4];
    int cnt = 0;  // (wave-uniform)
    for (long long i0 = (long long)blockIdx.x * 1024 + threadIdx.x; i0 < n; i0 += (long long)gridDim.x * 1024) {
        uint32_t l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) l[u] = i0 + u * 256 < n ? gt[i0 + u * 256] : 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) cnt += __popcll(__ballot(i0 + u * 256 < n && ot_moving(K, l[u])));
    }
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (t) atomicAdd(&counters[kOtMovingPoints], (ot_u64)t);
    }
}

// one lane: (label, count) into the wave's table; true when the label took a new slot.  The table is never full (header)
__device__ __forceinline__ bool ot_lds_add(ot_u64* tab, uint32_t label, uint32_t count) {
    unsigned s = (ot_hash(label) >> 16) & (kOtSlots - 1);
    for (;;) {
        ot_u64 cur = tab[s];
        if (cur == 0ull) {
            cur = atomicCAS(&tab[s], 0ull, ((ot_u64)count << 32) | label);
            if (cur == 0ull) return true;
        }
        if ((uint32_t)cur == label) {
            atomicAdd(&tab[s], (ot_u64)count << 32);
            return false;
        }
        s = (s + 1) & (kOtSlots - 1);
    }
}

__global__ __launch_bounds__(256) void k_ot_objects(Arena A, TruthJob J, int n_scans) {
    __shared__ ot_u64 lds[4 * kOtSlots];
    const int lane = threadIdx.x & 63;
    ot_u64* tab = lds + (threadIdx.x >> 6) * kOtSlots;
    const long long n_all = J.tab_stats[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        J.counters[kOtWritten] = (ot_u64)(n_all < J.cap ? n_all : J.cap);
        J.counters[kOtObjects] = (ot_u64)n_all;
        J.counters[kOtOverflow] = n_all > J.cap ? 1ull : 0ull;
    }
    for (long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); o < n_all; o += (long long)gridDim.x * 4) {
        const int b = J.begin[o], e = J.begin[o + 1];
        const int g0 = (int)(uint32_t)J.key_out[b];
        const int s = ot_scan_of(A, n_scans, g0);
        const int base = A.scan_off[s];
        const int scan_n = A.scan_off[s + 1] - base;
#pragma unroll
        for (int k = 0; k < kOtSlots / 64; ++k) tab[lane + 64 * k] = 0ull;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        int n_moving = 0, n_distinct = 0;  // (wave-uniform)
        uint32_t cur = ot_load(A, J.key_out, J.gt, b + lane, e, base, scan_n);
        for (int j = b; j < e && n_distinct <= SCVOD_OBJ_TRUTH_ONCHIP_LABELS; j += 64) {
            const uint32_t nxt = ot_load(A, J.key_out, J.gt, j + 64 + lane, e, base, scan_n);
            unsigned long long todo = __ballot(j + lane < e);
            // the moving test per member, one vector compare per class and round whatever the number of labels in the round; made on
            // the combined labels with scalar compares the call took 7.97 instead of 4.34 ms on the K64 job with twelve labels drawn
            // point by point, 5.16 instead of 3.81 ms with runs of one label (profiles/object_truth_cost.txt)
            n_moving += __popcll(__ballot(ot_moving(J.K, cur)) & todo);
            int pending = 0;
            uint32_t my_label = 0u, my_count = 0u;
            while (todo) {
                const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)cur, __ffsll((long long)todo) - 1);
                const unsigned long long bm = __ballot(cur == k0) & todo;
                const int c = __popcll(bm);
                if (lane == pending) my_label = k0, my_count = (uint32_t)c;
                ++pending;
                todo &= ~bm;
            }
            const bool fresh = lane < pending && ot_lds_add(tab, my_label, my_count);
            n_distinct += __popcll(__ballot(fresh));
            cur = nxt;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (n_distinct > SCVOD_OBJ_TRUTH_ONCHIP_LABELS) {  // the whole object again, by the fallback
            if (lane == 0) {
                const ot_u64 at = atomicAdd(&J.counters[kOtFallback], 1ull);
                if (at < (ot_u64)J.list_cap) J.list[at] = (int32_t)o;
            }
            continue;
        }
        ot_u64 slot[kOtSlots / 64];
        ot_u64 best = 0ull;
#pragma unroll
        for (int k = 0; k < kOtSlots / 64; ++k) {
            slot[k] = tab[lane + 64 * k];
            const ot_u64 key = slot[k] ? slot[k] ^ 0xFFFFFFFFull : 0ull;
            best = key > best ? key : best;
        }
        best = wave_max_u64(best);
        const uint32_t label = ~(uint32_t)best;
        int n_class = 0;
#pragma unroll
        for (int k = 0; k < kOtSlots / 64; ++k)
            if (slot[k] && (((uint32_t)slot[k] ^ label) & 0xFFFFu) == 0u) n_class += (int)(slot[k] >> 32);
        n_class = wave_sum_int(n_class);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the next object clears the table after these reads)
        if (lane == 0) {
            if (n_moving) atomicAdd(&J.counters[kOtMovingMembers], (ot_u64)n_moving);
            if (o < J.cap) {
                scvod_object_truth r;
                r.label = label;
                r.n_label = (int32_t)(best >> 32);
                r.n_class = n_class;
                r.n_moving = n_moving;
                r.n_distinct = n_distinct;
                r.n_points = e - b;
                r.reserved[0] = r.reserved[1] = 0;
                J.out[o] = r;
            }
        }
    }
}

template <typename T>
__device__ __forceinline__ T ot_block_reduce(T v, T* scratch, bool take_max) {  // 256 threads; every thread gets the result
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const T o = (T)__shfl_xor((long long)v, d, 64);
        v = take_max ? (o > v ? o : v) : v + o;
    }
    __syncthreads();  // (scratch may still be read from the reduction before)
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = scratch[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) r = take_max ? (scratch[w] > r ? scratch[w] : r) : r + scratch[w];
    return r;
}

__global__ __launch_bounds__(256) void k_ot_fallback(Arena A, TruthJob J, int n_scans) {
    __shared__ ot_u64 red[4];
    ot_u64* region = J.regions + (size_t)blockIdx.x * J.region_slots;
    const ot_u64 listed = __hip_atomic_load(&J.counters[kOtFallback], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long n_list = listed < (ot_u64)J.list_cap ? (long long)listed : J.list_cap;
    for (long long at = blockIdx.x; at < n_list; at += gridDim.x) {
        const long long o = J.list[at];
        const int b = J.begin[o], e = J.begin[o + 1];
        const int g0 = (int)(uint32_t)J.key_out[b];
        const int s = ot_scan_of(A, n_scans, g0);
        const int base = A.scan_off[s];
        const int scan_n = A.scan_off[s + 1] - base;
        // an object lives inside one scan: 2 (e - b) <= region_slots
        const unsigned slots = (unsigned)min((long long)2 * (e - b), J.region_slots);
        for (unsigned k = threadIdx.x; k < slots; k += 256) __hip_atomic_store(&region[k], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        __syncthreads();
        long long n_moving = 0;
        for (int p = b + (int)threadIdx.x; p < e; p += 256) {
            const uint32_t label = ot_load(A, J.key_out, J.gt, p, e, base, scan_n);
            if (ot_moving(J.K, label)) ++n_moving;
            unsigned k = (unsigned)(((ot_u64)ot_hash(label) * slots) >> 32);
            for (unsigned probe = 0; probe < slots; ++probe) {  // (never runs out: at most e - b labels in 2 (e - b) slots)
                ot_u64 cur = __hip_atomic_load(&region[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur == 0ull) {
                    cur = atomicCAS(&region[k], 0ull, (1ull << 32) | label);
                    if (cur == 0ull) break;
                }
                if ((uint32_t)cur == label) {
                    atomicAdd(&region[k], 1ull << 32);
                    break;
                }
                k = k + 1 == slots ? 0u : k + 1;
            }
        }
        __threadfence();
        __syncthreads();
        ot_u64 best = 0ull;
        long long n_distinct = 0;
        for (unsigned k = threadIdx.x; k < slots; k += 256) {
            const ot_u64 v = __hip_atomic_load(&region[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v) {
                const ot_u64 key = v ^ 0xFFFFFFFFull;
                best = key > best ? key : best;
                ++n_distinct;
            }
        }
        best = ot_block_reduce<ot_u64>(best, red, true);
        n_distinct = (long long)ot_block_reduce<ot_u64>((ot_u64)n_distinct, red, false);
        n_moving = (long long)ot_block_reduce<ot_u64>((ot_u64)n_moving, red, false);
        const uint32_t label = ~(uint32_t)best;
        long long n_class = 0;
        for (unsigned k = threadIdx.x; k < slots; k += 256) {
            const ot_u64 v = __hip_atomic_load(&region[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v && (((uint32_t)v ^ label) & 0xFFFFu) == 0u) n_class += (long long)(v >> 32);
        }
        n_class = (long long)ot_block_reduce<ot_u64>((ot_u64)n_class, red, false);
        if (threadIdx.x == 0) {
            if (n_moving) atomicAdd(&J.counters[kOtMovingMembers], (ot_u64)n_moving);
            if (o < J.cap) {
                scvod_object_truth r;
                r.label = label;
                r.n_label = (int32_t)(best >> 32);
                r.n_class = (int32_t)n_class;
                r.n_moving = (int32_t)n_moving;
                r.n_distinct = (int32_t)n_distinct;
                r.n_points = e - b;
                r.reserved[0] = r.reserved[1] = 0;
                J.out[o] = r;
            }
        }
        __syncthreads();  // (the region is cleared again only after every thread has read it)
    }
}

}  // namespace

long long truth_list_cap(long long total_pts) { return total_pts / (SCVOD_OBJ_TRUTH_ONCHIP_LABELS + 1) + 1; }

size_t truth_work_bytes(long long total_pts, int max_scan_pts) {
    const size_t list = ((size_t)truth_list_cap(total_pts) * sizeof(int32_t) + 255) & ~(size_t)255;
    return list + sizeof(ot_u64) * (size_t)kOtGroups * 2 * (size_t)(max_scan_pts > 0 ? max_scan_pts : 1);
}

void launch_object_truth(const Arena& A, TruthJob J, void* work, hipStream_t st) {
    const size_t list = ((size_t)truth_list_cap(A.total_pts) * sizeof(int32_t) + 255) & ~(size_t)255;
    J.list = (int32_t*)work;
    J.list_cap = truth_list_cap(A.total_pts);
    J.regions = (ot_u64*)((unsigned char*)work + list);
    J.region_slots = 2 * (long long)(A.max_scan_pts > 0 ? A.max_scan_pts : 1);
    hipMemsetAsync(J.counters, 0, sizeof(ot_u64) * 8, st);
    if (A.total_pts > 0) {
        const long long blocks = (A.total_pts + 1023) / 1024;
        hipLaunchKernelGGL(k_ot_points, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, J.gt, (long long)A.total_pts, J.K, J.counters);
    }
    long long waves = A.total_pts;  // (an object has at least one of the batch's points)
    if (waves < 1) waves = 1;        // (block 0 writes the stats)
    const long long grid = (waves + 3) / 4;
    hipLaunchKernelGGL(k_ot_objects, dim3((unsigned)(grid < 2048 ? grid : 2048)), dim3(256), 0, st, A, J, A.n_scans);
    hipLaunchKernelGGL(k_ot_fallback, dim3(kOtGroups), dim3(256), 0, st, A, J, A.n_scans);
}

}  // namespace scvod
