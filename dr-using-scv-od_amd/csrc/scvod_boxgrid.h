// scvod_boxgrid.h -- the exact k <= 16 nearest-neighbour search over a uniform CSR grid on a bounding box, shared by the region
// growing (scvod_k_rgrow.inc: one grid per cluster) and the intensity calibration (scvod_k_calib.inc: one grid per scan).  Both
// stages promise bit-exact neighbour lists that are the same on every run; that rests on the ONE cell rule, shape rule, tie rule,
// ring walk and stop rule below.  The search is exact for any cell edge: the shape only sets its cost.
// Plain floats and SCVOD_HD, as scvod_math.h: tests/helpers/boxgrid_replay.cpp runs the same functions on the CPU.  What needs the
// workgroup (the CSR build) or float4 (the stored form) is device code at the end.
#ifndef SCVOD_BOXGRID_H_
#define SCVOD_BOXGRID_H_
#include <math.h>
#include "scvod_math.h"

namespace scvod {

constexpr int kBoxGridK = 16;  // neighbours a query keeps at most

struct BoxGrid {
    float ox, oy, oz, h;  // the box's low corner, the cell edge
    int dx, dy, dz;       // cells per axis
};

SCVOD_HD int bg_imin(int a, int b) { return a < b ? a : b; }
SCVOD_HD int bg_imax(int a, int b) { return a > b ? a : b; }

// ---- cell rule: clamped to the grid, so every point of the cloud (and any query) has a cell
SCVOD_HD int bg_cell1(float v, float o, float h, int d) {
    const float t = (v - o) / h;
    int c = t > 0.f ? (int)t : 0;
    return c < d ? c : d - 1;
}
SCVOD_HD int bg_cell_id(const BoxGrid& g, int x, int y, int z) { return (z * g.dy + y) * g.dx + x; }  // x fastest
SCVOD_HD int bg_cell(const BoxGrid& g, float x, float y, float z) {
    return bg_cell_id(g, bg_cell1(x, g.ox, g.h, g.dx), bg_cell1(y, g.oy, g.h, g.dy), bg_cell1(z, g.oz, g.h, g.dz));
}

// ---- shape rule: the edge for n points in the box [o, o + e]: a surface's worth of cells (surf), a volume's (vol), at least
// 2 a / n, then grown until the table holds at most 2 n cells.
struct BoxShape { float surf, vol, grow; };
constexpr BoxShape kRgShape{1.5f, 1.0f, 1.25f};    // a cluster: about two points per cell on a surface, one in a volume
constexpr BoxShape kCalShape{0.5f, 0.5f, 1.125f};  // a whole scan: the far field is almost empty, the 2 n cells set the edge
SCVOD_HD BoxGrid bg_shape(float ox, float oy, float oz, float ex, float ey, float ez, int n, const BoxShape s) {
    const float a = fmaxf(ex, fmaxf(ey, ez)), cmin = fminf(ex, fminf(ey, ez));
    const float b = ex + ey + ez - a - cmin;
    float h = fmaxf(fmaxf(sqrtf(a * b / (float)n) * s.surf, cbrtf(a * b * cmin / (float)n) * s.vol), 2.f * a / (float)n);
    // a point box, or an extent that overflowed.  (The region growing's candidates passed the range filter: their extents are
    // finite and far from overflow, so only h = 0 reaches this from there.)
    if (!(h > 0.f) || !(h < 3.0e38f)) h = 1.f;
    BoxGrid g{ox, oy, oz, h, 1, 1, 1};
    for (;;) {
        g.dx = (int)fminf(ex / g.h, 1.0e6f) + 1;
        g.dy = (int)fminf(ey / g.h, 1.0e6f) + 1;
        g.dz = (int)fminf(ez / g.h, 1.0e6f) + 1;
        if ((double)g.dx * g.dy * g.dz <= 2.0 * n) break;
        g.h *= s.grow;
    }
    return g;
}

// ---- CSR convention: after the build cell[id] is the END of cell id, so a run of consecutive cells [ia, ib] holds the
// contiguous entries [b, e)
SCVOD_HD void bg_run(const int* cell, int ia, int ib, int& b, int& e) {
    b = ia ? cell[ia - 1] : 0;
    e = cell[ib];
}

// ---- top-k: kBoxGridK (d^2, index) pairs the caller owns (registers), ascending, ties to the lower index; (kth, kq) mirrors
// entry k_eff - 1 so one compare turns most candidates away.  kth is +inf while fewer than k_eff are held.
SCVOD_HD void bg_topk_clear(float (&bd)[kBoxGridK], int (&bq)[kBoxGridK], float& kth, int& kq) {
#pragma unroll
    for (int j = 0; j < kBoxGridK; ++j) {
        bd[j] = u2f(0x7f800000u);
        bq[j] = 0x7fffffff;
    }
    kth = u2f(0x7f800000u);
    kq = 0x7fffffff;
}
SCVOD_HD void bg_topk_insert(float cd, int cq, int keff, float (&bd)[kBoxGridK], int (&bq)[kBoxGridK], float& kth, int& kq) {
    if (!(cd < kth || (cd == kth && cq < kq))) return;
#pragma unroll
    for (int j = 0; j < kBoxGridK; ++j) {
        if (j < keff && (cd < bd[j] || (cd == bd[j] && cq < bq[j]))) {
            const float td = bd[j];
            const int tq = bq[j];
            bd[j] = cd;
            bq[j] = cq;
            cd = td;
            cq = tq;
        }
    }
#pragma unroll
    for (int j = 0; j < kBoxGridK; ++j)
        if (j == keff - 1) {
            kth = bd[j];
            kq = bq[j];
        }
}
// the distance of every candidate: d^2 = (dx*dx + dy*dy) + dz*dz in fp32
SCVOD_HD float bg_dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float ddx = ax - bx, ddy = ay - by, ddz = az - bz;
    return (ddx * ddx + ddy * ddy) + ddz * ddz;
}

// ---- ring walk: the cells at Chebyshev distance exactly r from cell (cx, cy, cz), clipped to the grid, as runs of consecutive
// cells: f(ia, ib, z - cz, y - cy).  On a shell row the whole run x0 .. x1 is new; inside the ring's box only its two x faces are.
template <typename F>
SCVOD_HD void bg_ring_runs(const BoxGrid& g, int cx, int cy, int cz, int r, F f) {
    const int zl = bg_imax(cz - r, 0), zh = bg_imin(cz + r, g.dz - 1), yl = bg_imax(cy - r, 0), yh = bg_imin(cy + r, g.dy - 1);
    const int x0 = bg_imax(cx - r, 0), x1 = bg_imin(cx + r, g.dx - 1);
    for (int z = zl; z <= zh; ++z) {
        for (int y = yl; y <= yh; ++y) {
            const int row = bg_cell_id(g, 0, y, z);
            const bool shell = r == 0 || z == cz - r || z == cz + r || y == cy - r || y == cy + r;
            if (shell) f(row + x0, row + x1, z - cz, y - cy);
            if (!shell && cx - r >= 0) f(row + cx - r, row + cx - r, z - cz, y - cy);
            if (!shell && cx + r <= g.dx - 1) f(row + cx + r, row + cx + r, z - cz, y - cy);
        }
    }
}

// ---- stop rule.  The margin covers the rounding of the cell assignment and of the distances.
SCVOD_HD float bg_margin(const BoxGrid& g) {
    return 1.0e-6f * (fmaxf(fabsf(g.ox), fmaxf(fabsf(g.oy), fabsf(g.oz))) + g.h * (float)bg_imax(g.dx, bg_imax(g.dy, g.dz))) + 1.0e-6f * g.h;
}
// distance from (x, y, z) in cell (cx, cy, cz) to what rings 0 .. r leave unprobed: the nearest face of the probed box that is not a
// face of the grid; +inf when the whole grid is probed
SCVOD_HD float bg_unprobed(const BoxGrid& g, int cx, int cy, int cz, int r, float x, float y, float z) {
    float bnd = u2f(0x7f800000u);
    if (cx - r > 0) bnd = fminf(bnd, x - (g.ox + (float)(cx - r) * g.h));
    if (cx + r < g.dx - 1) bnd = fminf(bnd, (g.ox + (float)(cx + r + 1) * g.h) - x);
    if (cy - r > 0) bnd = fminf(bnd, y - (g.oy + (float)(cy - r) * g.h));
    if (cy + r < g.dy - 1) bnd = fminf(bnd, (g.oy + (float)(cy + r + 1) * g.h) - y);
    if (cz - r > 0) bnd = fminf(bnd, z - (g.oz + (float)(cz - r) * g.h));
    if (cz + r < g.dz - 1) bnd = fminf(bnd, (g.oz + (float)(cz + r + 1) * g.h) - z);
    return bnd;
}
// the search ends after ring r: the whole grid is probed, or the k-th distance lies strictly below the bound (ties at the bound
// widen; kth = +inf while fewer than k_eff are found)
SCVOD_HD bool bg_stop(float bnd, float mg, float kth) {
    if (bnd == u2f(0x7f800000u)) return true;
    const float b = bnd - mg;
    return b > 0.f && kth < (b * b) * 0.99999f;
}

}  // namespace scvod

#if defined(__HIPCC__)
#include "scvod_dev.h"
namespace scvod {
// ---- stored form: {ox, oy, oz, h} {dx, dy, dz, w}; w is the caller's word (the calibration keeps n there)
static __device__ __forceinline__ void bg_store(float4* p, const BoxGrid& g, int w) {
    p[0] = make_float4(g.ox, g.oy, g.oz, g.h);
    p[1] = make_float4(__int_as_float(g.dx), __int_as_float(g.dy), __int_as_float(g.dz), __int_as_float(w));
}
static __device__ __forceinline__ BoxGrid bg_load(const float4* p, int* w = nullptr) {
    const float4 a = p[0], b = p[1];
    if (w) *w = __float_as_int(b.w);
    return BoxGrid{a.x, a.y, a.z, a.w, __float_as_int(b.x), __float_as_int(b.y), __float_as_int(b.z)};
}

// ---- the CSR of n points by one workgroup of THREADS: cell[0 .. nc] (the caller's words; cell[id] = END of id afterwards),
// pcell[k] = the cell of point k.  pt(k) is point k as a float4, put(k, slot, q) stores point k = q at rank `slot` of the cell order
// (q is loaded ahead of the cursor's atomic so the two latencies overlap; a caller that ignores it pays nothing).
// The order inside a cell is whatever the atomics give: the top-k is ordered by (d^2, index), a total order, so no result sees it.
// The caller's barrier precedes the call (g is uniform, a copy in registers); none follows the scatter.
template <int THREADS, typename Pt, typename Put>
static __device__ __forceinline__ void bg_csr_build(const BoxGrid g, int n, int* cell, int* pcell, int* wsum, Pt pt, Put put) {
    const int nc = g.dx * g.dy * g.dz;
    for (int k = threadIdx.x; k <= nc; k += THREADS) cell[k] = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += THREADS) {
        const float4 q = pt(k);
        const int id = bg_cell(g, q.x, q.y, q.z);
        pcell[k] = id;
        atomicAdd(&cell[id], 1);
    }
    __syncthreads();
    int carry = 0;  // exclusive scan of the counts, in place
    for (int k0 = 0; k0 <= nc; k0 += THREADS) {
        const int k = k0 + threadIdx.x;
        const int v = k <= nc ? cell[k] : 0;
        int total;
        const int ex = block_excl_scan<THREADS>(v, total, wsum);
        if (k <= nc) cell[k] = carry + ex;
        carry += total;
        __syncthreads();
    }
    // scatter: cell[id] runs as the cursor of cell id
    for (int k = threadIdx.x; k < n; k += THREADS) {
        const float4 q = pt(k);
        put(k, atomicAdd(&cell[pcell[k]], 1), q);
    }
}

}  // namespace scvod
#endif
#endif
