// scvod_grid.h -- the CSR hash grid over a point cloud that the nearest-neighbour stages share: the correspondence search
// (scvod_k_nn_grid.inc), the evaluation (scvod_eval.hip), the class scores (scvod_classes.hip) and the map split (scvod_split.hip).
// Points are hashed by cell into `buckets` (a power of two) CSR rows; a query walks the buckets of the cells around it.  Several
// cells may hash to one bucket, and a bucket may hold points of far cells: every candidate is a real point with its real distance,
// so a superset of the cells asked for changes nothing.  All four stages promise bit-exact answers that are the same on every run;
// that rests on the ONE cell rule, hash, distance expression and tie rule below.
// The library is built without relocatable device code: the device helpers are inlined into each unit's kernels; the build kernels
// and grid_build live in scvod_kernels.hip (declared in scvod_kernels.h).
#ifndef SCVOD_GRID_H_
#define SCVOD_GRID_H_
#include "scvod_dev.h"

namespace scvod {

// what a query kernel reads.  work area behind it (grid_work_ints ints): count | start | cursor | entries | grand | block_tot
struct PointGrid {
    float ox, oy, oz, inv_h;  // origin (it only shifts the hash) and 1 / cell edge
    uint32_t mask;            // buckets - 1 (power of two)
    const int* start;
    const int* count;
    const int* entries;  // (the order inside a bucket varies from run to run; the tie rule does not depend on it)
};
// the origin of the stages whose clouds need no shift (x - 0.0f is x bit for bit, NaN included)
constexpr float kGridOrigin0[3] = {0.f, 0.f, 0.f};

static __device__ __forceinline__ void grid_cell(const PointGrid& g, float x, float y, float z, int& cx, int& cy, int& cz) {
    cx = (int)floorf((x - g.ox) * g.inv_h);
    cy = (int)floorf((y - g.oy) * g.inv_h);
    cz = (int)floorf((z - g.oz) * g.inv_h);
}
static __device__ __forceinline__ uint32_t grid_bucket(const PointGrid& g, int cx, int cy, int cz) {
    return ((uint32_t)cx * 73856093u ^ (uint32_t)cy * 19349663u ^ (uint32_t)cz * 83492791u) & g.mask;
}

// (d, m) against (best, bi): the nearer one, ties to the lowest index.  bi = -1: no candidate yet; m = -1: nothing offered (the
// partner lane of a shuffle reduction may hold none)
static __device__ __forceinline__ void grid_take(float d, int m, float& best, int& bi) {
    if (m >= 0 && (bi < 0 || d < best || (d == best && m < bi))) {
        best = d;
        bi = m;
    }
}

// the candidates of bucket b against (best, bi).  stride: floats per record of xyz (a literal folds)
static __device__ __forceinline__ void grid_visit(const PointGrid& g, const float* __restrict__ xyz, int stride, uint32_t b, float qx, float qy,
                                                  float qz, float& best, int& bi) {
    const int s0 = g.start[b], c = g.count[b];
    for (int k = 0; k < c; ++k) {
        const int m = g.entries[s0 + k];
        __builtin_assume(m >= 0);  // (an entry is a point index: grid_take's guard folds away)
        const float* p = xyz + (size_t)stride * (size_t)m;
        const float ex = p[0] - qx, ey = p[1] - qy, ez = p[2] - qz;
        grid_take((ex * ex + ey * ey) + ez * ez, m, best, bi);
    }
}

// the 27 cells around the cell of (qx, qy, qz)
static __device__ __forceinline__ void grid_probe27(const PointGrid& g, const float* __restrict__ xyz, int stride, float qx, float qy, float qz,
                                                    float& best, int& bi) {
    int cx, cy, cz;
    grid_cell(g, qx, qy, qz, cx, cy, cz);
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) grid_visit(g, xyz, stride, grid_bucket(g, cx + dx, cy + dy, cz + dz), qx, qy, qz, best, bi);
}

// the cells at Chebyshev distance exactly r from cell (cx, cy, cz)
static __device__ __forceinline__ void grid_shell(const PointGrid& g, const float* __restrict__ xyz, int stride, int cx, int cy, int cz, int r,
                                                  float qx, float qy, float qz, float& best, int& bi) {
    for (int dz = -r; dz <= r; ++dz)
        for (int dy = -r; dy <= r; ++dy) {
            const bool face = dz == -r || dz == r || dy == -r || dy == r;
            // a row of the shell's faces is walked whole, any other row only touches the shell at its two ends
            for (int dx = -r; dx <= r; dx += face ? 1 : 2 * r)
                grid_visit(g, xyz, stride, grid_bucket(g, cx + dx, cy + dy, cz + dz), qx, qy, qz, best, bi);
        }
}

// the lanes of the wave with `later` set take consecutive slots of a list of length *n: one atomic per wave (ballot / popcount
// rank).  Every lane of the wave calls it; -1 for a lane without `later`
static __device__ __forceinline__ int wave_list_slot(bool later, int* n) {
    const unsigned long long bal = __ballot(later);
    if (!bal) return -1;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)bal) - 1;  // (a grid-stride loop may leave a wave with lane 0 idle)
    int slot0 = 0;
    if (lane == leader) slot0 = atomicAdd(n, __popcll(bal));
    slot0 = __shfl(slot0, leader, 64);
    return later ? slot0 + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
}

}  // namespace scvod
#endif
