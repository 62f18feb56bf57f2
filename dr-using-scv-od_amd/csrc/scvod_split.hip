// scvod_split.hip -- a map split by the nearest-neighbour hits of a cleaned cloud, on the device (gfx950): scvod_map_split_device.
//
// Reference analogue: src/erasor_dynamic.cpp:16-35 (every point of a static map looks up its single nearest point of the original map,
// nearestKSearch(pt, 1) without a radius; the original points nobody hit are the dynamic cloud) and the evaluation block of SSC::segDF
// (ssc.cpp:1511-1540: the same look-up into the labelled original cloud, a hit on a rejected label dropped, the hit ids sorted and made
// unique, the original points at those ids written as the estimate).  Both mark the base points that are the nearest neighbour of some
// query point and hand out the marked and the unmarked points in base order.  Here:
//     grid     the shared CSR hash grid of scvod_grid.h over the base cloud, with the caller's cell edge and record stride
//     pass 1   k_sp_probe: one thread per query, the 27 cells around it.  A query whose candidate lies closer than 0.99 cell edges is
//              FINISHED (nothing nearer can lie outside the cells it looked at; the evaluation's margin); so is every query of an empty
//              base.  The others go to a list with their candidate, one atomic per wave (ballot / popcount rank)
//     pass 2   k_sp_rings: a launch of its own over that list (no workgroup waits for another): ring r = 2 .. max_rings of cells at
//              Chebyshev distance r; after ring r a query is finished once its candidate is closer than 0.99 r cell edges.  What is left
//              goes to a second list
//     pass 3   k_sp_exhaustive: one workgroup per query of the second list scans the whole base cloud (lanes stride over the records,
//              16 bytes per lane at stride 4), (d, index) reduced with the tie rule through wave shuffles and LDS.  n_base records per
//              such query: it exists so that the answer is exact for any input, and it is counted; a cleaned map never reaches it
//     A tie partner at the same distance lies inside the same radius, so the pass that finishes a query has seen it: the result is that
//     of an exhaustive scan, ties (lowest base index) included, whatever the cell edge, the ring limit, the order inside a bucket or
//     the order of a list.  A bucket may hold points of far cells: every candidate is a real base point with its real distance.
//     marks    a finished query stores HIT or GATED (a function of the base point's label alone) at its neighbour's byte: all writers
//              of one byte store the same value, so a plain byte store is enough.  The bytes are cleared on the stream first
//     split    k_sp_count per tile of kSpTile base points and class (ballot / popcount), the counts laid out class-major so that ONE
//              exclusive scan (launch_scan_ints) yields segment base + tile offset at once, k_sp_write (a point's slot is that prefix +
//              the points of its class in the rounds and waves before it + its rank in the wave).  Records move as whole 12- or 16-byte
//              units of 32-bit words: NaN payloads survive.  Integer sums only: the same bytes on every run
#include <hip/hip_runtime.h>

#include "scvod_grid.h"

namespace scvod {
namespace {

// a finished query: its outputs and its neighbour's mark
__device__ __forceinline__ void sp_finish(const SpJob& J, int q, int bi, float best) {
    if (J.nn_idx) J.nn_idx[q] = bi;
    if (J.nn_sq) J.nn_sq[q] = bi >= 0 ? best : __builtin_inff();
    if (bi < 0) return;
    bool gated = false;
    if (J.n_reject > 0) {
        const uint32_t sem = J.base_label[bi] & 0xFFFFu;  // ssc.cpp:1524
        for (int k = 0; k < J.n_reject; ++k) gated |= sem == (uint32_t)J.reject[k];
    }
    J.mark[bi] = gated ? (uint8_t)SCVOD_SPLIT_GATED : (uint8_t)SCVOD_SPLIT_HIT;
}

__global__ __launch_bounds__(256) void k_sp_probe(PointGrid g, SpJob J, float thr1) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = q < J.n_query;
    bool later = false;
    float best = 0.f;
    int bi = -1;
    if (valid) {
        if (J.n_base > 0) {
            const float* p = J.query + (size_t)J.query_stride * (size_t)q;
            const float qx = p[0], qy = p[1], qz = p[2];
            grid_probe27(g, J.base, J.base_stride, qx, qy, qz, best, bi);
            later = !(bi >= 0 && best < thr1);
        }
        if (!later) sp_finish(J, (int)q, bi, best);
    }
    const int slot = wave_list_slot(later, J.n_list1);
    if (later) {
        J.list1_q[slot] = (int)q;
        J.list1_bi[slot] = bi;
        J.list1_best[slot] = best;
    }
}

__global__ __launch_bounds__(256) void k_sp_rings(PointGrid g, SpJob J, float g1) {
    const int nt = *J.n_list1;
    // whole waves enter the loop body together (the bound is rounded up to the wave), so wave_list_slot sees every lane
    const long long nt64 = ((long long)nt + 63) & ~63ll;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < nt64; t += (long long)gridDim.x * 256) {
        bool later = false;
        int q = 0;
        if (t < nt) {
            q = J.list1_q[t];
            int bi = J.list1_bi[t];
            float best = J.list1_best[t];
            const float* p = J.query + (size_t)J.query_stride * (size_t)q;
            const float qx = p[0], qy = p[1], qz = p[2];
            int cx, cy, cz;
            grid_cell(g, qx, qy, qz, cx, cy, cz);
            later = true;
            for (int r = 2; r <= J.max_rings; ++r) {
                grid_shell(g, J.base, J.base_stride, cx, cy, cz, r, qx, qy, qz, best, bi);
                const float reach = g1 * (float)r;
                if (bi >= 0 && best < reach * reach) {
                    later = false;
                    break;
                }
            }
            if (!later) sp_finish(J, q, bi, best);
        }
        const int slot = wave_list_slot(later, J.n_list2);
        if (later) J.list2_q[slot] = q;  // (the exhaustive scan sees the candidate again: it is not carried)
    }
}

// one workgroup per query of the second list
__global__ __launch_bounds__(256) void k_sp_exhaustive(SpJob J) {
    __shared__ float wbest[4];
    __shared__ int wbi[4];
    const int nt = *J.n_list2;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    typedef float f4v __attribute__((ext_vector_type(4)));
    for (int t = blockIdx.x; t < nt; t += gridDim.x) {
        const int q = J.list2_q[t];
        const float* p = J.query + (size_t)J.query_stride * (size_t)q;
        const float qx = p[0], qy = p[1], qz = p[2];
        float best = 0.f;
        int bi = -1;
        if (J.base_stride == 4) {
            const f4v* rec = reinterpret_cast<const f4v*>(J.base);
            for (long long m = threadIdx.x; m < J.n_base; m += 256) {
                const f4v v = rec[m];
                const float ex = v.x - qx, ey = v.y - qy, ez = v.z - qz;
                grid_take((ex * ex + ey * ey) + ez * ez, (int)m, best, bi);
            }
        } else {
            for (long long m = threadIdx.x; m < J.n_base; m += 256) {
                const float* b = J.base + 3 * (size_t)m;
                const float ex = b[0] - qx, ey = b[1] - qy, ez = b[2] - qz;
                grid_take((ex * ex + ey * ey) + ez * ez, (int)m, best, bi);
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ob = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            grid_take(ob, oi, best, bi);
        }
        if (lane == 0) {
            wbest[w] = best;
            wbi[w] = bi;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 1; k < 4; ++k) grid_take(wbest[k], wbi[k], best, bi);
            sp_finish(J, q, bi, best);
        }
        __syncthreads();  // (wbest / wbi are written again by the next query)
    }
}

// points of class HIT / MISS / GATED in tile blockIdx.x -> cnt[class * n_tiles + tile] (HIT, MISS, GATED: the order of the segments)
__global__ __launch_bounds__(256) void k_sp_count(const uint8_t* __restrict__ mark, int n_base, int n_tiles, int* __restrict__ cnt) {
    __shared__ int wcnt[4][2];
    const long long i0 = (long long)blockIdx.x * kSpTile;
    int hit = 0, gated = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const long long i = i0 + u * 256 + threadIdx.x;
        const uint8_t m = i < n_base ? mark[i] : (uint8_t)SCVOD_SPLIT_MISS;
        hit += __popcll(__ballot(m == SCVOD_SPLIT_HIT));
        gated += __popcll(__ballot(m == SCVOD_SPLIT_GATED));
    }
    if ((threadIdx.x & 63) == 0) {
        wcnt[threadIdx.x >> 6][0] = hit;
        wcnt[threadIdx.x >> 6][1] = gated;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int h = wcnt[0][0] + wcnt[1][0] + wcnt[2][0] + wcnt[3][0], gt = wcnt[0][1] + wcnt[1][1] + wcnt[2][1] + wcnt[3][1];
        const long long in_tile = (long long)n_base - i0 < kSpTile ? (long long)n_base - i0 : kSpTile;
        cnt[blockIdx.x] = h;
        cnt[n_tiles + blockIdx.x] = (int)in_tile - h - gt;
        cnt[2 * n_tiles + blockIdx.x] = gt;
    }
}

// the segment bounds and the eight stats words.  off: the exclusive scan of k_sp_count's counts (nullptr: an empty base)
__global__ void k_sp_tail(const int* __restrict__ off, int n_tiles, SpJob J, unsigned long long* __restrict__ stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long a = off ? off[n_tiles] : 0, b = off ? off[2 * (size_t)n_tiles] : 0;
    if (J.seg4) {
        J.seg4[0] = 0;
        J.seg4[1] = a;
        J.seg4[2] = b;
        J.seg4[3] = J.n_base;
    }
    const long long l1 = *J.n_list1, l2 = *J.n_list2;
    stats[0] = (unsigned long long)a;
    stats[1] = (unsigned long long)(b - a);
    stats[2] = (unsigned long long)(J.n_base - b);
    stats[3] = (unsigned long long)(J.n_query - l1);
    stats[4] = (unsigned long long)(l1 - l2);
    stats[5] = (unsigned long long)l2;
    stats[6] = 0;
    stats[7] = 0;
}

// the points of tile blockIdx.x into their slots.  The base is streamed once in input order
template <int STRIDE>
__global__ __launch_bounds__(256) void k_sp_write(const uint8_t* __restrict__ mark, const int* __restrict__ off, int n_tiles, SpJob J) {
    __shared__ int wcnt[3][32];  // [class][round * 4 + wave] points, then their exclusive prefix in (round, wave) order
    const long long i0 = (long long)blockIdx.x * kSpTile;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int cls[8], rank[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const long long i = i0 + u * 256 + threadIdx.x;
        const bool valid = i < J.n_base;
        const uint8_t m = valid ? mark[i] : (uint8_t)SCVOD_SPLIT_MISS;
        // segment of the point: 0 HIT, 1 MISS, 2 GATED; -1: behind the base
        cls[u] = !valid ? -1 : (m == SCVOD_SPLIT_HIT ? 0 : (m == SCVOD_SPLIT_GATED ? 2 : 1));
        rank[u] = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned long long bal = __ballot(cls[u] == k);
            if (cls[u] == k) rank[u] = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[k][u * 4 + w] = __popcll(bal);
        }
    }
    __syncthreads();
    if (w < 3) {  // wave k scans class k
        const int v = lane < 32 ? wcnt[w][lane] : 0;
        const int inc = wave_incl_scan(v);
        if (lane < 32) wcnt[w][lane] = inc - v;
    }
    __syncthreads();
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(J.base);
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(J.base_out);
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (cls[u] < 0) continue;
        const long long i = i0 + u * 256 + threadIdx.x;
        const size_t o = (size_t)off[(size_t)cls[u] * n_tiles + blockIdx.x] + (size_t)(wcnt[cls[u]][u * 4 + w] + rank[u]);
        if (J.order) J.order[o] = (int)i;
        if (dst) {
            if (STRIDE == 4) {
                *reinterpret_cast<u4v*>(dst + 4 * o) = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(src + 4 * (size_t)i));
            } else {
                const uint32_t x = src[3 * (size_t)i], y = src[3 * (size_t)i + 1], z = src[3 * (size_t)i + 2];
                dst[3 * o] = x;
                dst[3 * o + 1] = y;
                dst[3 * o + 2] = z;
            }
        }
        if (J.payload_out) J.payload_out[o] = J.payload_in[i];
    }
}

inline unsigned sp_blocks(long long n) { return (unsigned)((n + 255) / 256); }
inline size_t sp_up(size_t v) { return (v + 255) / 256 * 256; }

struct SpLayout {
    size_t grid, list1, list2, cnt, off, scan_tmp, mark, total;
    int n_tiles;
};
SpLayout sp_layout(int32_t buckets, int32_t n_base, int32_t n_query) {
    SpLayout L;
    const size_t nq = (size_t)(n_query > 0 ? n_query : 1);
    L.n_tiles = (int)(((long long)n_base + kSpTile - 1) / kSpTile);
    const size_t nt3 = 3 * (size_t)(L.n_tiles > 0 ? L.n_tiles : 1);
    size_t o = 0;
    L.grid = o;
    o = sp_up(o + sizeof(int) * grid_work_ints(buckets, n_base));
    L.list1 = o;  // length | query, candidate, distance
    o = sp_up(o + sizeof(int) * (1 + 3 * nq));
    L.list2 = o;  // length | query
    o = sp_up(o + sizeof(int) * (1 + nq));
    L.cnt = o;
    o = sp_up(o + sizeof(int) * nt3);
    L.off = o;
    o = sp_up(o + sizeof(int) * nt3);
    L.scan_tmp = o;  // launch_scan_ints' block totals | grand total
    o = sp_up(o + sizeof(int) * ((nt3 + 1023) / 1024 + 2));
    L.mark = o;
    o = sp_up(o + (size_t)(n_base > 0 ? n_base : 1));
    L.total = o;
    return L;
}

}  // namespace

size_t sp_work_bytes(int32_t buckets, int32_t n_base, int32_t n_query) { return sp_layout(buckets, n_base, n_query).total; }

void launch_map_split(SpJob J, float cell, int32_t buckets, void* work, unsigned long long* stats, hipStream_t st) {
    const SpLayout L = sp_layout(buckets, J.n_base, J.n_query);
    unsigned char* w = (unsigned char*)work;
    const size_t nq = (size_t)(J.n_query > 0 ? J.n_query : 1);
    J.n_list1 = (int*)(w + L.list1);
    J.list1_q = J.n_list1 + 1;
    J.list1_bi = J.list1_q + nq;
    J.list1_best = reinterpret_cast<float*>(J.list1_bi + nq);
    J.n_list2 = (int*)(w + L.list2);
    J.list2_q = J.n_list2 + 1;
    if (!J.mark) J.mark = w + L.mark;
    hipMemsetAsync(J.n_list1, 0, sizeof(int), st);
    hipMemsetAsync(J.n_list2, 0, sizeof(int), st);
    if (J.n_base > 0) hipMemsetAsync(J.mark, SCVOD_SPLIT_MISS, (size_t)J.n_base, st);
    if (J.n_query > 0) {
        const PointGrid g = grid_build(J.base, J.base_stride, nullptr, J.n_base, kGridOrigin0, cell, buckets, (int*)(w + L.grid), st);
        const float g1 = 0.99f * cell;
        hipLaunchKernelGGL(k_sp_probe, dim3(sp_blocks(J.n_query)), dim3(256), 0, st, g, J, g1 * g1);
        if (J.n_base > 0) {
            // the lists' lengths are known on the device only: grid-stride launches; a block that finds nothing to do leaves at once
            const unsigned blocks = sp_blocks(J.n_query) < 2048u ? sp_blocks(J.n_query) : 2048u;
            hipLaunchKernelGGL(k_sp_rings, dim3(blocks), dim3(256), 0, st, g, J, g1);
            hipLaunchKernelGGL(k_sp_exhaustive, dim3(J.n_query < 2048 ? J.n_query : 2048), dim3(256), 0, st, J);
        }
    }
    int* cnt = (int*)(w + L.cnt);
    int* off = (int*)(w + L.off);
    int* tmp = (int*)(w + L.scan_tmp);
    if (J.n_base > 0) {
        hipLaunchKernelGGL(k_sp_count, dim3(L.n_tiles), dim3(256), 0, st, J.mark, J.n_base, L.n_tiles, cnt);
        launch_scan_ints(cnt, off, tmp + 1, tmp, 3 * L.n_tiles, st);
    }
    hipLaunchKernelGGL(k_sp_tail, dim3(1), dim3(64), 0, st, J.n_base > 0 ? off : nullptr, L.n_tiles, J, stats);
    if (J.n_base > 0 && (J.order || J.base_out || J.payload_out)) {
        if (J.base_stride == 4)
            hipLaunchKernelGGL(k_sp_write<4>, dim3(L.n_tiles), dim3(256), 0, st, J.mark, off, L.n_tiles, J);
        else
            hipLaunchKernelGGL(k_sp_write<3>, dim3(L.n_tiles), dim3(256), 0, st, J.mark, off, L.n_tiles, J);
    }
}

}  // namespace scvod
