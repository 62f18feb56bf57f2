// scvod_classes.hip -- the recognised ground / building / tree classes of a map or a batch scored against labelled truth, on the device
// (gfx950): scvod_score_classes_device, scvod_batch_score_classes.
//
// Reference analogue: src/plotObject.cpp:87-146, the tool behind the per-class table of doc/note.txt:57-78 -- a 1-NN look-up from every
// ground-truth point into the class-coloured map, four rules, P and N per class.  Here:
//     grid     the shared CSR hash grid of scvod_grid.h (an optional keep byte per estimate point) with the caller's cell edge
//     pass 1   k_cs_probe: one thread per truth point, the 27 cells around it.  A query whose best candidate lies closer than 0.99 cell
//              edges is FINISHED (nothing nearer can lie outside the cells it looked at; scvod_eval.hip's margin) and scored at once; the
//              others are appended to a list with their candidate, one atomic per wave (ballot / popcount rank)
//     pass 2   k_cs_rings: a launch of its own over that list (no workgroup waits for another one): ring r = 2 .. R of cells at Chebyshev
//              distance r, R = ceil(max_dist / (0.99 cell)); a query stops after ring r once its candidate is closer than 0.99 r cell edges.
//              A tie partner at the same distance lies inside the same radius, so it was seen: the result is that of an exhaustive scan of
//              all (2R + 1)^3 cells, ties (lowest estimate index) included, whatever the order of the list
//     scores   a neighbour counts only when d < max_dist * max_dist; per block an LDS histogram of 21 ints (20 confusion cells + pd_far,
//              integer atomicAdd), then one 64-bit global atomic per non-zero cell and block: integer sums, the same on every run
#include <hip/hip_runtime.h>

#include "scvod_grid.h"

namespace scvod {
namespace {

// truth class of a label: the lists in the order of plotObject.cpp's check(); in no list: pd
__device__ __forceinline__ int cs_truth(const CsLists& L, uint32_t label) {
    const uint32_t sem = label & 0xFFFFu;
    bool g = false, b = false, t = false;
    for (int k = 0; k < L.n_ground; ++k) g |= sem == (uint32_t)L.ground[k];
    for (int k = 0; k < L.n_building; ++k) b |= sem == (uint32_t)L.building[k];
    for (int k = 0; k < L.n_tree; ++k) t |= sem == (uint32_t)L.tree[k];
    return g ? 0 : (b ? 1 : (t ? 2 : 3));
}
// estimate class of a SCVOD_PT_* byte: the colours of SSC::saveSegCloud as plotObject.cpp:51-85 reads them
__device__ __forceinline__ int cs_est(uint8_t pt) {
    return pt == SCVOD_PT_GROUND ? 1 : (pt == SCVOD_PT_STATIC_BUILDING ? 2 : (pt == SCVOD_PT_STATIC_OTHER ? 3 : 0));
}

// one truth point with its final candidate -> its histogram cell, pd_far and its result byte (plotObject.cpp:95-139)
__device__ __forceinline__ void cs_score(int t, int bi, float best, float max2, const uint8_t* __restrict__ est_class, long long q,
                                         uint8_t* __restrict__ result, int* hist) {
    int e = 4;  // none
    if (bi >= 0 && best < max2) e = cs_est(est_class[bi]);
    bool P;
    if (t == 0)
        P = e == 1;
    else if (t == 3)
        P = e == 0 || e == 4 || best > 0.5f;
    else
        P = e == 2 || e == 3;
    atomicAdd(&hist[t * 5 + e], 1);
    if (t == 3 && e >= 1 && e <= 3 && best > 0.5f) atomicAdd(&hist[20], 1);
    if (result) result[q] = (uint8_t)(t | (e << 2) | (P ? 32 : 0));
}

// Every thread of the block calls it, after its last cs_score.
__device__ __forceinline__ void cs_flush(int* hist, unsigned long long* counters) {
    __syncthreads();
    if (threadIdx.x < 21) {
        const int c = hist[threadIdx.x];
        if (c) atomicAdd(&counters[threadIdx.x], (unsigned long long)c);
    }
}

struct CsTodo {  // the pass-2 list: per slot the query and the candidate pass 1 left it with
    int* n;
    int* q;
    int* bi;
    float* best;
};

__global__ __launch_bounds__(256) void k_cs_probe(PointGrid g, const float* __restrict__ est_xyz, const uint8_t* __restrict__ est_class, int probe,
                                                  const float* __restrict__ q_xyz, const uint32_t* __restrict__ q_label, int n_q, CsLists L,
                                                  float thr1, float max2, int rings, CsTodo todo, unsigned long long* counters,
                                                  uint8_t* __restrict__ result) {
    __shared__ int hist[21];
    if (threadIdx.x < 21) hist[threadIdx.x] = 0;
    __syncthreads();
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = q < n_q;
    bool later = false;
    float best = 0.f;
    int bi = -1;
    if (valid) {
        if (probe) {
            const float qx = q_xyz[3 * (size_t)q], qy = q_xyz[3 * (size_t)q + 1], qz = q_xyz[3 * (size_t)q + 2];
            grid_probe27(g, est_xyz, 3, qx, qy, qz, best, bi);
            later = rings > 1 && !(bi >= 0 && best < thr1);
        }
        if (!later) cs_score(cs_truth(L, q_label[q]), bi, best, max2, est_class, q, result, hist);
    }
    // the unfinished queries of the wave take consecutive slots: one atomic per wave
    const int slot = wave_list_slot(later, todo.n);
    if (later) {
        todo.q[slot] = (int)q;
        todo.bi[slot] = bi;
        todo.best[slot] = best;
    }
    cs_flush(hist, counters);
}

__global__ __launch_bounds__(256) void k_cs_rings(PointGrid g, const float* __restrict__ est_xyz, const uint8_t* __restrict__ est_class,
                                                  const float* __restrict__ q_xyz, const uint32_t* __restrict__ q_label, CsLists L, float g1,
                                                  float max2, int rings, CsTodo todo, unsigned long long* counters,
                                                  uint8_t* __restrict__ result) {
    __shared__ int hist[21];
    if (threadIdx.x < 21) hist[threadIdx.x] = 0;
    __syncthreads();
    const int nt = *todo.n;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < nt; t += (long long)gridDim.x * 256) {
        const int q = todo.q[t];
        int bi = todo.bi[t];
        float best = todo.best[t];
        const float qx = q_xyz[3 * (size_t)q], qy = q_xyz[3 * (size_t)q + 1], qz = q_xyz[3 * (size_t)q + 2];
        int cx, cy, cz;
        grid_cell(g, qx, qy, qz, cx, cy, cz);
        for (int r = 2; r <= rings; ++r) {
            grid_shell(g, est_xyz, 3, cx, cy, cz, r, qx, qy, qz, best, bi);
            const float reach = g1 * (float)r;
            if (bi >= 0 && best < reach * reach) break;
        }
        cs_score(cs_truth(L, q_label[q]), bi, best, max2, est_class, q, result, hist);
    }
    cs_flush(hist, counters);
}

inline unsigned cs_blocks(int n) { return (unsigned)(((long long)n + 255) / 256); }

}  // namespace

size_t cs_work_bytes(int32_t buckets, int32_t n_est, int32_t n_gt) {
    // grid ints | list length | list: query, candidate, distance
    return sizeof(int) * (grid_work_ints(buckets, n_est) + 1 + 3 * (size_t)(n_gt > 0 ? n_gt : 1));
}

void launch_class_score(const float* gt_xyz, const uint32_t* gt_label, int32_t n_gt, const float* est_xyz, const uint8_t* est_class,
                        const uint8_t* est_keep, int32_t n_est, const CsLists& L, float cell, float max_dist, int32_t rings, int32_t buckets,
                        int* work, unsigned long long* counters, uint8_t* point_result, hipStream_t st) {
    int* tail = work + grid_work_ints(buckets, n_est);
    CsTodo todo;
    todo.n = tail;
    todo.q = tail + 1;
    todo.bi = todo.q + (n_gt > 0 ? n_gt : 1);
    todo.best = reinterpret_cast<float*>(todo.bi + (n_gt > 0 ? n_gt : 1));
    hipMemsetAsync(counters, 0, sizeof(unsigned long long) * 24, st);  // [0..20] the scores, [21] the pass-2 list's length
    hipMemsetAsync(todo.n, 0, sizeof(int), st);
    if (n_gt <= 0) return;
    const PointGrid g = grid_build(est_xyz, 3, est_keep, n_est, kGridOrigin0, cell, buckets, work, st);
    const float g1 = 0.99f * cell, max2 = max_dist * max_dist;
    hipLaunchKernelGGL(k_cs_probe, dim3(cs_blocks(n_gt)), dim3(256), 0, st, g, est_xyz, est_class, n_est > 0 ? 1 : 0, gt_xyz, gt_label, n_gt, L,
                       g1 * g1, max2, rings, todo, counters, point_result);
    if (n_est > 0 && rings > 1) {
        // the list's length is known on the device only: a grid-stride launch; a block that finds nothing to do leaves at once
        const unsigned blocks = cs_blocks(n_gt) < 2048u ? cs_blocks(n_gt) : 2048u;
        hipLaunchKernelGGL(k_cs_rings, dim3(blocks), dim3(256), 0, st, g, est_xyz, est_class, gt_xyz, gt_label, L, g1, max2, rings, todo, counters,
                           point_result);
    }
    hipMemcpyAsync(counters + 21, todo.n, sizeof(int), hipMemcpyDeviceToDevice, st);  // (the low word of a cleared 64-bit counter)
}

}  // namespace scvod
