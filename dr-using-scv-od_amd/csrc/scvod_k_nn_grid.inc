// scvod_k_nn_grid.inc -- uniform-grid correspondence search (A7).
// Part of the kernels translation unit: included by scvod_kernels.hip (inside namespace scvod), never compiled on its own.
// ---- uniform-grid correspondence search ------------------------------------------------------------
// Map points are entered into the shared hash grid of scvod_grid.h (cell edge h); a query probes the 27 cells around it.
// If the best candidate is within 0.99 h it is the true nearest neighbour (anything outside the 27 cells is farther
// than that; the 1 % covers the fp32 rounding of the cell coordinate, DESIGN.md A7); otherwise the query goes to the exact
// brute-force kernel.  Distances and tie-breaking (lowest map index) are those of the brute-force kernel, so both paths return
// identical results.  The radius search has no second kernel: its cell is chosen so that radius^2 <= (0.99 h)^2.

// exclusive scan of `n` ints, three launches: per-block (1024) scans + block totals, scan of totals, add-back
__global__ __launch_bounds__(1024) void k_scan_blocks(const int* in, int* out, int* block_tot, int n) {
    __shared__ int wsum[17];
    const int i = blockIdx.x * 1024 + threadIdx.x;
    const int v = (i < n) ? in[i] : 0;
    int total;
    const int ex = block_excl_scan<1024>(v, total, wsum);
    if (i < n) out[i] = ex;
    if (threadIdx.x == 0) block_tot[blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void k_scan_totals(int* block_tot, int nb, int* grand_total) {
    __shared__ int wsum[17];
    int run = 0;
    for (int c0 = 0; c0 < nb; c0 += 1024) {
        const int i = c0 + threadIdx.x;
        const int v = (i < nb) ? block_tot[i] : 0;
        int total;
        const int ex = block_excl_scan<1024>(v, total, wsum);
        if (i < nb) block_tot[i] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) *grand_total = run;
}
__global__ __launch_bounds__(1024) void k_scan_add(int* out, const int* block_tot, int n) {
    const int i = blockIdx.x * 1024 + threadIdx.x;
    if (i < n) out[i] += block_tot[blockIdx.x];
}

__global__ __launch_bounds__(256) void k_nn_query(PointGrid g, float h2, const float* __restrict__ map_xyz, const float* __restrict__ q_xyz,
                                                  int n_q, float r2, int32_t* nn_idx, float* nn_sq, uint8_t* within, int* todo, int* n_todo,
                                                  int bounded) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n_q) return;
    const float qx = q_xyz[3 * (size_t)q], qy = q_xyz[3 * (size_t)q + 1], qz = q_xyz[3 * (size_t)q + 2];
    float best = 0.f;
    int bi = -1;
    grid_probe27(g, map_xyz, 3, qx, qy, qz, best, bi);
    if (bounded) {
        // radius search (pcl radiusSearch, evaluate.cpp:95,104): the caller's cell has r2 <= h2 (nn_run), so every map point with
        // d^2 < r2 is closer than 0.99 cell edges and therefore among the candidates: the best of them below r2 is the nearest
        // point inside the radius, and none below r2 means none inside it
        const bool in = bi >= 0 && best < r2;
        nn_idx[q] = in ? bi : -1;
        nn_sq[q] = in ? best : __builtin_huge_valf();
        within[q] = in ? 1 : 0;
    } else if (bi >= 0 && best <= h2) {
        nn_idx[q] = bi;
        nn_sq[q] = best;
        within[q] = best < r2 ? 1 : 0;
    } else {
        todo[atomicAdd(n_todo, 1)] = q;  // exact answer needs the whole map
    }
}

__global__ __launch_bounds__(kNnThreads) void k_nn_brute_list(const float* __restrict__ map_xyz, int n_map,
                                                               const float* __restrict__ q_xyz, const int* todo,
                                                               const int* n_todo, float r2, int32_t* nn_idx, float* nn_sq,
                                                               uint8_t* within) {
    __shared__ float tx[kNnTile], ty[kNnTile], tz[kNnTile];
    const int nt = *n_todo;
    for (int t0q = blockIdx.x * kNnThreads; t0q < nt; t0q += gridDim.x * kNnThreads) {
        const int t = t0q + threadIdx.x;
        const int q = (t < nt) ? todo[t] : -1;
        float qx = 0, qy = 0, qz = 0;
        if (q >= 0) {
            qx = q_xyz[3 * (size_t)q];
            qy = q_xyz[3 * (size_t)q + 1];
            qz = q_xyz[3 * (size_t)q + 2];
        }
        float best = 0.f;
        int bi = -1;
        for (int m0 = 0; m0 < n_map; m0 += kNnTile) {
            const int tn = min(kNnTile, n_map - m0);
            __syncthreads();
            for (int j = threadIdx.x; j < tn; j += kNnThreads) {
                tx[j] = map_xyz[3 * (size_t)(m0 + j)];
                ty[j] = map_xyz[3 * (size_t)(m0 + j) + 1];
                tz[j] = map_xyz[3 * (size_t)(m0 + j) + 2];
            }
            __syncthreads();
            if (q >= 0) {
                for (int j = 0; j < tn; ++j) {
                    const float dx = tx[j] - qx, dy = ty[j] - qy, dz = tz[j] - qz;
                    const float d = (dx * dx + dy * dy) + dz * dz;
                    if (bi < 0 || d < best) {
                        best = d;
                        bi = m0 + j;
                    }
                }
            }
        }
        if (q >= 0) {
            nn_idx[q] = bi;
            nn_sq[q] = best;
            within[q] = (bi >= 0 && best < r2) ? 1 : 0;
        }
    }
}

