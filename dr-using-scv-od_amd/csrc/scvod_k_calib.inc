// scvod_k_calib.inc -- intensity calibration by incidence angle: SSC::intensityCalibrationByCurvature (ssc.cpp:98-153), opt-in
// (scvod_set_intensity_calibration).  Included by scvod_kernels.hip; runs between k_emit and the voxel stage.
//
// Per chunk of scans (CalJob: the scratch is sized by a chunk, not by the batch), over the WHOLE non-ground cloud of every scan in
// Patchwork's emission order (nonground_idx): position = index in that order.
//   k_cal_slot   per apri point: the apri slot of its input point (the map from a non-ground position to the record it patches)
//   k_cal_grid   per scan (one workgroup): box of the non-ground cloud, a uniform grid over it in CSR form (at most 2 n cells) and
//                the CELL-SORTED COPY of the points {x, y, z, position}: a run of cells along x is one contiguous run of 16-byte records
//   k_cal_knn    per block of 256 consecutive sorted points (a tile: a run of cells, whose queries read the same candidates): the
//                nine runs of the tile's cells and their rim are staged in LDS when they fit; rings 0 and 1 of every query read the
//                staged runs (lanes of one cell read the same address: a broadcast), wider rings -- and every ring of a tile that
//                does not fit -- read the sorted copy in HBM (the fallback path).  k candidates in registers in (d^2, position)
//                order, ring growth until the k-th distance lies strictly below the bound of the unprobed region (as k_rg_knn).
//                Behind it, fused: normal + curvature (point_normal_f32 over the neighbours in kNN order), the calibrated
//                intensity (calibrated_intensity_f32), the patch of apri_int, the counters.  The neighbour list never reaches HBM.
//   k_cal_apri   per apri point of one scan: the calibrated intensity into a materialised PointAPRI record (after k_apri_expand)
// The static map keeps the RAW intensity of its representative points (it reads the input cloud, not apri_int).

constexpr int kCalThreads = 256;
constexpr int kCalGridThreads = 1024;
constexpr int kCalLdsPts = 4096;  // staged records per tile: 64 KB of LDS, two workgroups per CU -- half the waves 116 VGPRs allow, and
                                  // measured slower than no staging at all for it (DESIGN.md section 4: the first of the next levers)

struct CalGrid {
    float ox, oy, oz, h;
    int dx, dy, dz, n;
};
__device__ __forceinline__ size_t cal_cell_base(const Arena& A, const CalJob& J, int s) {
    return 3 * (size_t)(A.scan_off[s] - J.off0) + 4 * (size_t)(s - J.s0);  // 2 n + 2 <= 3 n + 4 words per scan
}
__device__ __forceinline__ int cal_cell_of(const CalGrid& G, const float4 q) {
    return (rg_cell1(q.z, G.oz, G.h, G.dz) * G.dy + rg_cell1(q.y, G.oy, G.h, G.dy)) * G.dx + rg_cell1(q.x, G.ox, G.h, G.dx);
}

// chunk scan s0 + blockIdx.y, its apri points along x
__global__ __launch_bounds__(kCalThreads) void k_cal_slot(Arena A, CalJob J) {
    const int s = J.s0 + blockIdx.y;
    const int n = A.counts[(size_t)s * 8 + 4];
    const int j = blockIdx.x * kCalThreads + threadIdx.x;
    if (j >= n) return;
    const size_t base = (size_t)A.scan_off[s];
    J.slot[(base - J.off0) + A.apri_src[base + j]] = j;
}

__global__ __launch_bounds__(kCalThreads) void k_cal_apri(Arena A, int s) {
    const int n = A.counts[(size_t)s * 8 + 4];
    const size_t base = (size_t)A.scan_off[s];
    for (int i = blockIdx.x * kCalThreads + threadIdx.x; i < n; i += gridDim.x * kCalThreads) A.apri[base + i].intensity = A.apri_int[base + i];
}

// one workgroup per scan of the chunk
__global__ __launch_bounds__(kCalGridThreads) void k_cal_grid(Arena A, CalJob J) {
    __shared__ int wsum[kCalGridThreads / 64 + 1];
    __shared__ uint32_t bb[6];
    __shared__ CalGrid G;
    const int s = J.s0 + blockIdx.x;
    const int n = A.counts[(size_t)s * 8 + 2];
    const size_t base = (size_t)A.scan_off[s];
    const size_t g0 = base - J.off0;
    if (n <= 0) {
        if (threadIdx.x == 0) {
            J.grid[2 * (size_t)blockIdx.x] = make_float4(0.f, 0.f, 0.f, 1.f);
            J.grid[2 * (size_t)blockIdx.x + 1] = make_float4(__int_as_float(1), __int_as_float(1), __int_as_float(1), __int_as_float(0));
        }
        return;
    }
    if (threadIdx.x < 3) bb[threadIdx.x] = 0xffffffffu;
    else if (threadIdx.x < 6) bb[threadIdx.x] = 0u;
    __syncthreads();
    {
        uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
        for (int k = threadIdx.x; k < n; k += kCalGridThreads) {
            const float4 q = A.pts[base + A.nonground_idx[base + k]];
            const uint32_t e[3] = {f2ord(q.x), f2ord(q.y), f2ord(q.z)};
            for (int a = 0; a < 3; ++a) {
                mn[a] = min(mn[a], e[a]);
                mx[a] = max(mx[a], e[a]);
            }
        }
        for (int a = 0; a < 3; ++a) {
            atomicMin(&bb[a], mn[a]);
            atomicMax(&bb[3 + a], mx[a]);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float ox = ord2f(bb[0]), oy = ord2f(bb[1]), oz = ord2f(bb[2]);
        const float ex = ord2f(bb[3]) - ox, ey = ord2f(bb[4]) - oy, ez = ord2f(bb[5]) - oz;
        const float a = fmaxf(ex, fmaxf(ey, ez)), cmin = fminf(ex, fminf(ey, ez));
        const float b = ex + ey + ez - a - cmin;
        // a surface's worth of cells first, a volume's second; the cell table holds at most 2 n cells, which is what sets the edge of a
        // whole scan (the far field is almost empty).  The kNN is exact for any edge.
        float h = fmaxf(fmaxf(sqrtf(a * b / (float)n) * 0.5f, cbrtf(a * b * cmin / (float)n) * 0.5f), 2.f * a / (float)n);
        if (!(h > 0.f) || !(h < 3.0e38f)) h = 1.f;
        int dx, dy, dz;
        for (;;) {
            dx = (int)fminf(ex / h, 1.0e6f) + 1;
            dy = (int)fminf(ey / h, 1.0e6f) + 1;
            dz = (int)fminf(ez / h, 1.0e6f) + 1;
            if ((double)dx * dy * dz <= 2.0 * n) break;
            h *= 1.125f;
        }
        G = CalGrid{ox, oy, oz, h, dx, dy, dz, n};
        J.grid[2 * (size_t)blockIdx.x] = make_float4(ox, oy, oz, h);
        J.grid[2 * (size_t)blockIdx.x + 1] = make_float4(__int_as_float(dx), __int_as_float(dy), __int_as_float(dz), __int_as_float(n));
    }
    __syncthreads();
    const CalGrid g = G;
    const int nc = g.dx * g.dy * g.dz;
    int* cell = J.cell + cal_cell_base(A, J, s);
    for (int k = threadIdx.x; k <= nc; k += kCalGridThreads) cell[k] = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += kCalGridThreads) {
        const int id = cal_cell_of(g, A.pts[base + A.nonground_idx[base + k]]);
        J.pcell[g0 + k] = id;
        atomicAdd(&cell[id], 1);
    }
    __syncthreads();
    int carry = 0;  // exclusive scan of the counts, in place
    for (int k0 = 0; k0 <= nc; k0 += kCalGridThreads) {
        const int k = k0 + threadIdx.x;
        const int v = k <= nc ? cell[k] : 0;
        int total;
        const int ex = block_excl_scan<kCalGridThreads>(v, total, wsum);
        if (k <= nc) cell[k] = carry + ex;
        carry += total;
        __syncthreads();
    }
    // scatter: cell[id] runs as the cursor of cell id; afterwards cell[id] is the END of id = the start of id + 1.  The order inside
    // a cell is whatever the atomics give: the candidate lists are ordered by (d^2, position), a total order, so no result sees it.
    for (int k = threadIdx.x; k < n; k += kCalGridThreads) {
        const float4 q = A.pts[base + A.nonground_idx[base + k]];
        const int slot = atomicAdd(&cell[J.pcell[g0 + k]], 1);
        J.sxyz[g0 + slot] = make_float4(q.x, q.y, q.z, __int_as_float(k));
    }
}

// one workgroup per 256 consecutive sorted points of chunk scan s0 + blockIdx.y
__global__ __launch_bounds__(kCalThreads) void k_cal_knn(Arena A, CalJob J) {
    extern __shared__ float4 cal_tile[];  // kCalLdsPts records
    __shared__ int r_lo[9], r_hi[9], r_at[9];  // per (dz, dy): staged run [lo, hi) of the sorted copy, its first LDS slot
    __shared__ int fits;
    __shared__ int sst[8];
    __shared__ unsigned long long scand;
    const int s = J.s0 + blockIdx.y;
    const float4 ga = J.grid[2 * (size_t)blockIdx.y], gb = J.grid[2 * (size_t)blockIdx.y + 1];
    const CalGrid G{ga.x, ga.y, ga.z, ga.w, __float_as_int(gb.x), __float_as_int(gb.y), __float_as_int(gb.z), __float_as_int(gb.w)};
    const int n = G.n;
    const int t0 = blockIdx.x * kCalThreads;
    if (t0 >= n) return;
    const size_t base = (size_t)A.scan_off[s];
    const size_t g0 = base - J.off0;
    const int* cell = J.cell + cal_cell_base(A, J, s);
    const float4* sx = J.sxyz + g0;
    const int nc = G.dx * G.dy * G.dz;
    const int keff = n < J.k ? n : J.k;
    const int t = t0 + threadIdx.x;
    const bool live = t < n;
    const float4 x = sx[live ? t : n - 1];
    const int cx = rg_cell1(x.x, G.ox, G.h, G.dx), cy = rg_cell1(x.y, G.oy, G.h, G.dy), cz = rg_cell1(x.z, G.oz, G.h, G.dz);
    if (threadIdx.x < 8) sst[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        scand = 0ull;
        // the tile's cells [ca, cb] in linear order (x fastest); every cell of ring 1 of one of them is ca + off - 1 .. cb + off + 1 for
        // one of the nine row offsets.  Cells a run takes in beyond the ring are more candidates, never fewer.
        const int ca = cal_cell_of(G, sx[t0]), cb = cal_cell_of(G, sx[min(t0 + kCalThreads, n) - 1]);
        int at = 0;
        for (int j = 0; j < 9; ++j) {
            const int off = ((j / 3 - 1) * G.dy + (j % 3 - 1)) * G.dx;
            const long long lo = max((long long)ca + off - 1, 0ll), hi = min((long long)cb + off + 1, (long long)nc - 1);
            r_at[j] = at;
            r_lo[j] = r_hi[j] = 0;
            if (lo > hi) continue;
            r_lo[j] = lo ? cell[lo - 1] : 0;
            r_hi[j] = cell[hi];
            at += r_hi[j] - r_lo[j];
            if (at > kCalLdsPts) break;  // (the runs are never read then)
        }
        fits = (at <= kCalLdsPts && !J.force_fallback) ? 1 : 0;
    }
    __syncthreads();
    const bool staged = fits != 0;
    if (staged) {
        for (int j = 0; j < 9; ++j) {
            const int lo = r_lo[j], cnt = r_hi[j] - lo, at = r_at[j];
            for (int k = threadIdx.x; k < cnt; k += kCalThreads) cal_tile[at + k] = sx[lo + k];
        }
    }
    __syncthreads();
    float bd[16];
    int bq[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        bd[j] = __uint_as_float(0x7f800000u);
        bq[j] = 0x7fffffff;
    }
    float kth = __uint_as_float(0x7f800000u);  // (bd, bq)[keff - 1]: one compare turns most candidates away
    int kq = 0x7fffffff;
    unsigned ncand = 0;
    auto consider = [&](const float4 y4) {
        const float ddx = y4.x - x.x, ddy = y4.y - x.y, ddz = y4.z - x.z;
        float cd = (ddx * ddx + ddy * ddy) + ddz * ddz;
        int cq = __float_as_int(y4.w);
        ++ncand;
        if (cd < kth || (cd == kth && cq < kq)) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
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
            for (int j = 0; j < 16; ++j)
                if (j == keff - 1) {
                    kth = bd[j];
                    kq = bq[j];
                }
        }
    };
    // margin of the bound: rounding of the cell assignment and of the distances
    const float mg = 1.0e-6f * (fmaxf(fabsf(G.ox), fmaxf(fabsf(G.oy), fabsf(G.oz))) + G.h * (float)max(G.dx, max(G.dy, G.dz))) + 1.0e-6f * G.h;
    int ring = 0, fell = 0;
    if (live) {
        for (int r = 0;; ++r) {
            ring = r;
            const int zl = max(cz - r, 0), zh = min(cz + r, G.dz - 1), yl = max(cy - r, 0), yh = min(cy + r, G.dy - 1);
            const int x0 = max(cx - r, 0), x1 = min(cx + r, G.dx - 1);
            const bool in_lds = staged && r <= 1;
            if (!in_lds) fell = 1;
            for (int z = zl; z <= zh; ++z) {
                for (int y = yl; y <= yh; ++y) {
                    const bool shell = r == 0 || z == cz - r || z == cz + r || y == cy - r || y == cy + r;
                    const int row = (z * G.dy + y) * G.dx;
                    // a shell row: the whole run of cells x0 .. x1; inside the ring's box only its two x faces are new
                    for (int part = 0; part < (shell ? 1 : 2); ++part) {
                        int ia, ib;
                        if (shell) {
                            ia = row + x0;
                            ib = row + x1;
                        } else if (part == 0) {
                            if (cx - r < 0) continue;
                            ia = ib = row + cx - r;
                        } else {
                            if (cx + r > G.dx - 1) continue;
                            ia = ib = row + cx + r;
                        }
                        const int b = ia ? cell[ia - 1] : 0, e = cell[ib];
                        if (in_lds) {
                            const int j = (z - cz + 1) * 3 + (y - cy + 1);
                            const float4* src = cal_tile + (r_at[j] - r_lo[j]);
                            for (int u = b; u < e; ++u) consider(src[u]);
                        } else {
                            for (int u = b; u < e; ++u) consider(sx[u]);
                        }
                    }
                }
            }
            // bound of the unprobed region: the nearest face of the probed box that is not a face of the grid
            float bnd = __uint_as_float(0x7f800000u);
            if (cx - r > 0) bnd = fminf(bnd, x.x - (G.ox + (float)(cx - r) * G.h));
            if (cx + r < G.dx - 1) bnd = fminf(bnd, (G.ox + (float)(cx + r + 1) * G.h) - x.x);
            if (cy - r > 0) bnd = fminf(bnd, x.y - (G.oy + (float)(cy - r) * G.h));
            if (cy + r < G.dy - 1) bnd = fminf(bnd, (G.oy + (float)(cy + r + 1) * G.h) - x.y);
            if (cz - r > 0) bnd = fminf(bnd, x.z - (G.oz + (float)(cz - r) * G.h));
            if (cz + r < G.dz - 1) bnd = fminf(bnd, (G.oz + (float)(cz + r + 1) * G.h) - x.z);
            if (bnd == __uint_as_float(0x7f800000u)) break;  // the whole grid is probed
            const float b = bnd - mg;
            if (b > 0.f && kth < (b * b) * 0.99999f) break;  // (kth is +inf while fewer than k_eff are found; ties at the bound widen)
        }
    }
    int fl = 0, isnan_n = 0;
    if (live) {
        const int pos = __float_as_int(x.w);
        int cnt = 0;  // (k_eff: every point of the cloud is a candidate once the rings cover the grid)
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < keff && bq[j] != 0x7fffffff) cnt = j + 1;
        const float4* pts = A.pts + base;
        const int32_t* ng = A.nonground_idx + base;
        float o[4];
        point_normal_f32(cnt, [&](int j, float& px, float& py, float& pz) {
            int q = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i == j) q = bq[i];
            const float4 v = pts[ng[q]];
            px = v.x;
            py = v.y;
            pz = v.z;
        }, o);
        const int id = ng[pos];
        const float val = calibrated_intensity_f32(pts[id].w, J.max_int, o, x.x, x.y, x.z, &fl);
        isnan_n = (o[0] != o[0] || o[1] != o[1] || o[2] != o[2]) ? 1 : 0;
        if (J.out_int) J.out_int[g0 + pos] = val;
        if (J.out_nc) J.out_nc[g0 + pos] = make_float4(o[0], o[1], o[2], o[3]);
        if (J.write_apri) {
            const int slot = J.slot[g0 + id];
            if (slot >= 0) A.apri_int[base + slot] = val;
        }
    }
    if (J.stats) {  // wave-level counts, one LDS atomic per wave and counter, one global atomic per workgroup and counter
        const int lane = threadIdx.x & 63;
        const int c0 = __popcll(__ballot(live)), c1 = __popcll(__ballot(fl & 1)), c2 = __popcll(__ballot(fl & 2)), c3 = __popcll(__ballot(fl & 4));
        const int c4 = __popcll(__ballot(isnan_n)), c5 = __popcll(__ballot(fell));
        unsigned long long cs = ncand;
        int mr = ring;
        for (int d = 32; d > 0; d >>= 1) {
            cs += __shfl_xor(cs, d);
            mr = max(mr, __shfl_xor(mr, d));
        }
        if (lane == 0) {
            atomicAdd(&sst[0], c0);
            atomicAdd(&sst[1], c1);
            atomicAdd(&sst[2], c2);
            atomicAdd(&sst[3], c3);
            atomicAdd(&sst[4], c4);
            atomicAdd(&sst[5], c5);
            atomicMax(&sst[6], mr);
            atomicAdd(&scand, cs);
        }
        __syncthreads();
        if (threadIdx.x < 6 && sst[threadIdx.x]) atomicAdd(&J.stats[threadIdx.x], sst[threadIdx.x]);
        if (threadIdx.x == 6) atomicMax(&J.stats[6], sst[6]);
        if (threadIdx.x == 7) atomicAdd(J.cand, scand);
    }
}
