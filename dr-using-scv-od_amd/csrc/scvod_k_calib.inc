// scvod_k_calib.inc -- intensity calibration by incidence angle: SSC::intensityCalibrationByCurvature (ssc.cpp:98-153), opt-in
// (scvod_set_intensity_calibration).  Included by scvod_kernels.hip; runs between k_emit and the voxel stage.
//
// Per chunk of scans (CalJob: the scratch is sized by a chunk, not by the batch), over the WHOLE non-ground cloud of every scan in
// Patchwork's emission order (nonground_idx): position = index in that order.
//   k_cal_slot   per apri point: the apri slot of its input point (the map from a non-ground position to the record it patches)
//   k_cal_grid   per scan (one workgroup): box of the non-ground cloud, a uniform grid over it in CSR form (scvod_boxgrid.h) and
//                the CELL-SORTED COPY of the points {x, y, z, position}: a run of cells along x is one contiguous run of 16-byte records
//   k_cal_knn    per block of 256 consecutive sorted points (a tile: a run of cells, whose queries read the same candidates): the
//                nine runs of the tile's cells and their rim are staged in LDS when they fit; rings 0 and 1 of every query read the
//                staged runs (lanes of one cell read the same address: a broadcast), wider rings -- and every ring of a tile that
//                does not fit -- read the sorted copy in HBM (the fallback path).  The search itself is scvod_boxgrid.h's: the tile
//                is the reader of the runs its ring walk hands out.
//                Behind it, fused: normal + curvature (point_normal_f32 over the neighbours in kNN order), the calibrated
//                intensity (calibrated_intensity_f32), the patch of apri_int, the counters.  The neighbour list never reaches HBM.
//   k_cal_apri   per apri point of one scan: the calibrated intensity into a materialised PointAPRI record (after k_apri_expand)
// The static map keeps the RAW intensity of its representative points (it reads the input cloud, not apri_int).

constexpr int kCalThreads = 256;
constexpr int kCalGridThreads = 1024;
constexpr int kCalLdsPts = 4096;  // staged records per tile: 64 KB of LDS, two workgroups per CU -- half the waves 110 VGPRs allow, and
                                  // measured slower than no staging at all for it (DESIGN.md section 4: the first of the next levers)

__device__ __forceinline__ size_t cal_cell_base(const Arena& A, const CalJob& J, int s) {
    return 3 * (size_t)(A.scan_off[s] - J.off0) + 4 * (size_t)(s - J.s0);  // 2 n + 2 <= 3 n + 4 words per scan
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
    __shared__ BoxGrid G;
    const int s = J.s0 + blockIdx.x;
    const int n = A.counts[(size_t)s * 8 + 2];
    const size_t base = (size_t)A.scan_off[s];
    const size_t g0 = base - J.off0;
    const float4* pts = A.pts + base;
    const int32_t* ng = A.nonground_idx + base;
    if (n <= 0) {
        if (threadIdx.x == 0) bg_store(J.grid + 2 * (size_t)blockIdx.x, BoxGrid{0.f, 0.f, 0.f, 1.f, 1, 1, 1}, 0);
        return;
    }
    if (threadIdx.x < 3) bb[threadIdx.x] = 0xffffffffu;
    else if (threadIdx.x < 6) bb[threadIdx.x] = 0u;
    __syncthreads();
    {
        uint32_t mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
#pragma unroll 2  // two dependent load chains in flight per lane: the loop is bound by their latency
        for (int k = threadIdx.x; k < n; k += kCalGridThreads) {
            const float4 q = pts[ng[k]];
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
        G = bg_shape(ox, oy, oz, ord2f(bb[3]) - ox, ord2f(bb[4]) - oy, ord2f(bb[5]) - oz, n, kCalShape);
        bg_store(J.grid + 2 * (size_t)blockIdx.x, G, n);
    }
    __syncthreads();
    // the cell order is a copy: sxyz[rank] = {x, y, z, position}
    bg_csr_build<kCalGridThreads>(G, n, J.cell + cal_cell_base(A, J, s), J.pcell + g0, wsum, [=](int k) { return pts[ng[k]]; },
                                  [&](int k, int slot, float4 q) { J.sxyz[g0 + slot] = make_float4(q.x, q.y, q.z, __int_as_float(k)); });
}

// one workgroup per 256 consecutive sorted points of chunk scan s0 + blockIdx.y
__global__ __launch_bounds__(kCalThreads) void k_cal_knn(Arena A, CalJob J) {
    extern __shared__ float4 cal_tile[];  // kCalLdsPts records
    __shared__ int r_lo[9], r_hi[9], r_at[9];  // per (dz, dy): staged run [lo, hi) of the sorted copy, its first LDS slot
    __shared__ int fits;
    __shared__ int sst[8];
    __shared__ unsigned long long scand;
    const int s = J.s0 + blockIdx.y;
    int n;
    const BoxGrid G = bg_load(J.grid + 2 * (size_t)blockIdx.y, &n);
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
    const int cx = bg_cell1(x.x, G.ox, G.h, G.dx), cy = bg_cell1(x.y, G.oy, G.h, G.dy), cz = bg_cell1(x.z, G.oz, G.h, G.dz);
    if (threadIdx.x < 8) sst[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        scand = 0ull;
        // the tile's cells [ca, cb] in linear order (x fastest); every cell of ring 1 of one of them is ca + off - 1 .. cb + off + 1 for
        // one of the nine row offsets.  Cells a run takes in beyond the ring are more candidates, never fewer.
        const float4 fa = sx[t0], fb = sx[min(t0 + kCalThreads, n) - 1];
        const int ca = bg_cell(G, fa.x, fa.y, fa.z), cb = bg_cell(G, fb.x, fb.y, fb.z);
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
    float bd[kBoxGridK], kth;
    int bq[kBoxGridK], kq;
    bg_topk_clear(bd, bq, kth, kq);
    unsigned ncand = 0;
    const float mg = bg_margin(G);
    int ring = 0, fell = 0;
    if (live) {
        for (int r = 0;; ++r) {
            ring = r;
            const bool in_lds = staged && r <= 1;
            if (!in_lds) fell = 1;
            // the reader of a run: the staged copy of its row for rings 0 and 1 of a staged tile, the sorted copy otherwise
            bg_ring_runs(G, cx, cy, cz, r, [&](int ia, int ib, int oz, int oy) {
                int b, e;
                bg_run(cell, ia, ib, b, e);
                ncand += (unsigned)(e - b);
                auto read = [&](const float4* src) {
                    for (int u = b; u < e; ++u) {
                        const float4 y4 = src[u];
                        bg_topk_insert(bg_dist2(y4.x, y4.y, y4.z, x.x, x.y, x.z), __float_as_int(y4.w), keff, bd, bq, kth, kq);
                    }
                };
                const int j = (oz + 1) * 3 + (oy + 1);
                if (in_lds) read(cal_tile + (r_at[j] - r_lo[j]));
                else read(sx);
            });
            if (bg_stop(bg_unprobed(G, cx, cy, cz, r, x.x, x.y, x.z), mg, kth)) break;
        }
    }
    int fl = 0, isnan_n = 0;
    if (live) {
        const int pos = __float_as_int(x.w);
        int cnt = 0;  // (k_eff: every point of the cloud is a candidate once the rings cover the grid)
#pragma unroll
        for (int j = 0; j < kBoxGridK; ++j)
            if (j < keff && bq[j] != 0x7fffffff) cnt = j + 1;
        const float4* pts = A.pts + base;
        const int32_t* ng = A.nonground_idx + base;
        float o[4];
        point_normal_f32(cnt, [&](int j, float& px, float& py, float& pz) {
            int q = 0;
#pragma unroll
            for (int i = 0; i < kBoxGridK; ++i)
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
