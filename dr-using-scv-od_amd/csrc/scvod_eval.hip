// scvod_eval.hip -- a cleaned batch or map against labelled truth, on the device (gfx950): scvod_evaluate_device, scvod_batch_evaluate,
// scvod_classify_map_device.
//
// Reference analogue: tool/analysis.py:124-194 (the counters behind PR / RR / F1: a ground-truth point is "preserved" when its nearest
// estimate point lies within voxelsize * sqrt(3) / 2 and both carry a static, resp. a dynamic, label) and the colour classes of the map
// viewer (src/evaluate.cpp:79-145).  pyshim/metric.py states both on the host over a 1-NN look-up; here the look-up, the tests and the
// counters are one kernel per ground-truth cloud.
//     grid     the shared CSR hash grid of scvod_grid.h over the estimate cloud, with an optional keep byte per point: the estimate of
//              a batch is a mask over the batch's world points, never a compaction
//     query    one thread per ground-truth point, the 27-cell probe, nearest candidate, ties to the lowest estimate index.  Every radius
//              that is asked about is below 0.99 cell edges, so a neighbour inside it is among the candidates: no second pass
//     counters ballot / popcount per wave, LDS per block, one 64-bit atomicAdd per counter and block: integer sums, the same on every run
#include <hip/hip_runtime.h>

#include "scvod_grid.h"

namespace scvod {
namespace {

__device__ __forceinline__ bool ev_is_dyn(const EvClasses& K, uint32_t label) {
    const uint32_t sem = label & 0xFFFFu;  // analysis.py:8-12
    bool d = false;
    for (int k = 0; k < K.n; ++k) d |= sem == (uint32_t)K.c[k];
    return d;
}

// NF flags per thread -> counters[slot[f]] += how many threads of the block raised flag f.  Every thread of the block calls it.
template <int NF>
__device__ __forceinline__ void ev_block_count(const bool (&flag)[NF], const int (&slot)[NF], int (*wcnt)[NF], unsigned long long* counters) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int c = __popcll(__ballot(flag[f]));
        if (lane == 0) wcnt[w][f] = c;
    }
    __syncthreads();
    if ((int)threadIdx.x < NF) {
        const int c = wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
        if (c) atomicAdd(&counters[slot[threadIdx.x]], (unsigned long long)c);
    }
}

// counter words of an evaluation, in the order of metric.preservation_rejection's counts
enum { kEvGtStatic = 0, kEvGtDynamic, kEvEstStatic, kEvEstDynamic, kEvPreserved, kEvStaticPreserved, kEvDynamicPreserved };

__global__ __launch_bounds__(256) void k_ev_query(PointGrid g, const float* __restrict__ map_xyz, const uint32_t* __restrict__ map_label, int probe,
                                                  const float* __restrict__ q_xyz, const uint32_t* __restrict__ q_label, int n_q, double limit,
                                                  EvClasses K, unsigned long long* counters, uint8_t* __restrict__ result) {
    __shared__ int wcnt[4][5];
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = q < n_q;
    bool inl = false, gdyn = false, edyn = false;
    if (valid) {
        gdyn = ev_is_dyn(K, q_label[q]);
        if (probe) {
            float best = 0.f;
            int bi = -1;  // (no candidate)
            grid_probe27(g, map_xyz, 3, q_xyz[3 * (size_t)q], q_xyz[3 * (size_t)q + 1], q_xyz[3 * (size_t)q + 2], best, bi);
            inl = bi >= 0 && sqrt((double)best) < limit;  // metric.py:22-23
            if (inl) edyn = ev_is_dyn(K, map_label[bi]);
        }
        if (result) result[q] = (uint8_t)((inl ? 1 : 0) | (gdyn ? 2 : 0) | (edyn ? 4 : 0));
    }
    const bool flag[5] = {valid && !gdyn, valid && gdyn, inl, inl && !gdyn && !edyn, inl && gdyn && edyn};
    const int slot[5] = {kEvGtStatic, kEvGtDynamic, kEvPreserved, kEvStaticPreserved, kEvDynamicPreserved};
    ev_block_count<5>(flag, slot, wcnt, counters);
}

__global__ __launch_bounds__(256) void k_ev_est_count(const uint32_t* __restrict__ label, const uint8_t* __restrict__ keep, int n, EvClasses K,
                                                      unsigned long long* counters) {
    __shared__ int wcnt[4][2];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool kept = i < n && (!keep || keep[i]);
    const bool dyn = kept && ev_is_dyn(K, label[i]);
    const bool flag[2] = {kept && !dyn, dyn};
    const int slot[2] = {kEvEstStatic, kEvEstDynamic};
    ev_block_count<2>(flag, slot, wcnt, counters);
}

// batch mode: the world position of every input point of scan blockIdx.y (tile blockIdx.x, the export's tiles) and its keep byte
__global__ __launch_bounds__(256) void k_ev_world(Arena A, const uint8_t* __restrict__ labels, uint32_t keep_mask, const float* __restrict__ pose,
                                                  float* __restrict__ world, uint8_t* __restrict__ keep) {
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int n = A.scan_off[s + 1] - base;
    const int i0 = blockIdx.x * kExpTile;
    if (i0 >= n) return;
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = pose[12 * (size_t)s + i];
    typedef float f4v __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * 256 + (int)threadIdx.x;
        if (i >= n) continue;
        const size_t p = (size_t)base + i;
        const f4v q = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(&A.pts[p]));
        // the map kernel's expression (Utility::transformCloud, utility.h:400-405): left to right, no contraction
        world[3 * p] = T[0] * q.x + T[1] * q.y + T[2] * q.z + T[3];
        world[3 * p + 1] = T[4] * q.x + T[5] * q.y + T[6] * q.z + T[7];
        world[3 * p + 2] = T[8] * q.x + T[9] * q.y + T[10] * q.z + T[11];
        keep[p] = (uint8_t)((keep_mask >> (labels[p] & 31u)) & 1u);  // the export's rule: a function of the label byte alone
    }
}

// evaluate() of src/evaluate.cpp:79-145 per point of the original map: one probe into the grid over the static cloud, one into the grid
// over the dynamic cloud; the class is metric.classify_map_points' four assignments in its order
__global__ __launch_bounds__(256) void k_ev_classify(PointGrid gs, const float* __restrict__ s_xyz, int probe_s, PointGrid gd, const float* __restrict__ d_xyz,
                                                     int probe_d, const float* __restrict__ o_xyz, const uint8_t* __restrict__ pred_static, int n,
                                                     float r15, float r10, uint8_t* __restrict__ cls, unsigned long long* counters) {
    __shared__ int wcnt[4][5];
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = q < n;
    int out = -1;
    if (valid) {
        const float qx = o_xyz[3 * (size_t)q], qy = o_xyz[3 * (size_t)q + 1], qz = o_xyz[3 * (size_t)q + 2];
        const float r15sq = r15 * r15, r10sq = r10 * r10;
        bool s15 = false, s10 = false, d15 = false, d10 = false;  // an empty cloud matches nothing
        if (probe_s) {
            float best = 0.f;
            int bi = -1;
            grid_probe27(gs, s_xyz, 3, qx, qy, qz, best, bi);
            s15 = bi >= 0 && best < r15sq;
            s10 = bi >= 0 && best < r10sq;
        }
        if (probe_d) {
            float best = 0.f;
            int bi = -1;
            grid_probe27(gd, d_xyz, 3, qx, qy, qz, best, bi);
            d15 = bi >= 0 && best < r15sq;
            d10 = bi >= 0 && best < r10sq;
        }
        const bool ps = pred_static[q] != 0;
        out = 0;                             // UNMATCHED
        if (ps && s15) out = 1;              // TP_STATIC
        if (ps && !s15 && d10) out = 2;      // FN_STATIC
        if (!ps && d15) out = 3;             // TN_DYNAMIC
        if (!ps && !d15 && s10) out = 4;     // FN_DYNAMIC
        if (cls) cls[q] = (uint8_t)out;
    }
    const bool flag[5] = {out == 0, out == 1, out == 2, out == 3, out == 4};
    const int slot[5] = {0, 1, 2, 3, 4};
    ev_block_count<5>(flag, slot, wcnt, counters);
}

inline unsigned ev_blocks(int n) { return (unsigned)(((long long)n + 255) / 256); }

}  // namespace

void launch_eval(const float* gt_xyz, const uint32_t* gt_label, int32_t n_gt, const float* est_xyz, const uint32_t* est_label,
                 const uint8_t* est_keep, int32_t n_est, double limit, const EvClasses& K, float cell, int32_t buckets, int* work,
                 unsigned long long* counters, uint8_t* point_result, hipStream_t st) {
    hipMemsetAsync(counters, 0, sizeof(unsigned long long) * 8, st);
    const PointGrid g = grid_build(est_xyz, 3, est_keep, n_est, kGridOrigin0, cell, buckets, work, st);
    if (n_est > 0) hipLaunchKernelGGL(k_ev_est_count, dim3(ev_blocks(n_est)), dim3(256), 0, st, est_label, est_keep, n_est, K, counters);
    if (n_gt > 0)
        hipLaunchKernelGGL(k_ev_query, dim3(ev_blocks(n_gt)), dim3(256), 0, st, g, est_xyz, est_label, n_est > 0 ? 1 : 0, gt_xyz, gt_label, n_gt,
                           limit, K, counters, point_result);
}

void launch_eval_world(const Arena& A, const uint8_t* labels, uint32_t keep_mask, const float* pose, float* world_xyz, uint8_t* keep,
                       hipStream_t st) {
    if (A.max_scan_pts <= 0 || A.n_scans <= 0) return;
    hipLaunchKernelGGL(k_ev_world, dim3((A.max_scan_pts + kExpTile - 1) / kExpTile, A.n_scans), dim3(256), 0, st, A, labels, keep_mask, pose,
                       world_xyz, keep);
}

void launch_classify(const float* orig_xyz, const uint8_t* pred_static, int32_t n, const float* static_xyz, int32_t n_static,
                     const float* dynamic_xyz, int32_t n_dynamic, float r15, float r10, float cell, int32_t buckets_s, int* work_s,
                     int32_t buckets_d, int* work_d, unsigned long long* counters, uint8_t* cls, hipStream_t st) {
    hipMemsetAsync(counters, 0, sizeof(unsigned long long) * 8, st);
    if (n <= 0) return;
    const PointGrid gs = grid_build(static_xyz, 3, nullptr, n_static, kGridOrigin0, cell, buckets_s, work_s, st);
    const PointGrid gd = grid_build(dynamic_xyz, 3, nullptr, n_dynamic, kGridOrigin0, cell, buckets_d, work_d, st);
    hipLaunchKernelGGL(k_ev_classify, dim3(ev_blocks(n)), dim3(256), 0, st, gs, static_xyz, n_static > 0 ? 1 : 0, gd, dynamic_xyz,
                       n_dynamic > 0 ? 1 : 0, orig_xyz, pred_static, n, r15, r10, cls, counters);
}

}  // namespace scvod
