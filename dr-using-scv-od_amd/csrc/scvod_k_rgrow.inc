// scvod_k_rgrow.inc -- building / tree of the large clusters: SSC::recognize's region-growing test (ssc.cpp:797-860), opt-in
// (scvod_set_region_growing).  Included by scvod_kernels.hip.
//
// Per chunk of scans (RgJob: the scratch is sized by a chunk, not by the batch), for the clusters that cc_type_rule sends down its
// `square > car_square` branch (the candidates):
//   k_rg_box     per cluster name: box and member count (order-preserving encodings, atomics)
//   k_rg_select  the candidates' points as keys (name << 32 | point), every apri point's default class; then a radix sort (host side)
//                orders them by (scan, cluster, apri index): the positions of the stage
//   k_rg_group   cluster records at the first position of every cluster
//   k_rg_grid    per cluster (one workgroup): a uniform grid over its box in CSR form (at most 2 n cells)
//   k_rg_knn     per point: the exact k nearest points of its cluster in (d^2, index) order
//                (both on scvod_boxgrid.h: shape, cell rule, CSR build, top-k, ring walk and stop rule are stated there)
//   k_rg_normal  per point: normal and curvature (scvod_math.h::point_normal_f32)
//   k_rg_edges   per point: the edges p -> q of the propagation (p capable, |n_p . n_q| not below cos theta), as a bit mask
//   k_rg_grow    per cluster (one workgroup): min-key propagation to a fixpoint (labels in LDS, or in HBM for large clusters), the
//                sequential tail of the points no capable point reached, segment sizes, the 20 % rule, the outputs
// DESIGN.md section 2 derives why the min-key propagation equals RegionGrowing::extract's seed-ordered growth.

constexpr int kRgThreads = 256;
constexpr int kRgLdsPts = 8192;  // labels of up to this many points live in LDS (64 KB); larger clusters take the HBM path

__device__ __forceinline__ float4 rg_point(const Arena& A, int from_apri, int s, int i) {
    const size_t base = (size_t)A.scan_off[s];
    if (from_apri) {
        const scvod_apri& a = A.apri[base + i];
        return make_float4(a.x, a.y, a.z, 0.f);
    }
    return A.pts[base + A.apri_src[base + i]];
}

// chunk scan s0 + blockIdx.y, its apri points along x
__global__ __launch_bounds__(kRgThreads) void k_rg_box(Arena A, RgJob J) {
    const int s = J.s0 + blockIdx.y;
    const int n = A.counts[(size_t)s * 8 + 4];
    const int i = blockIdx.x * kRgThreads + threadIdx.x;
    if (i >= n) return;
    const size_t base = (size_t)A.scan_off[s];
    if (A.pt_type[base + i] != 1) return;
    const int nm = (int)(base - J.off0) + A.pt_cluster[base + i];
    const float4 q = rg_point(A, J.from_apri, s, i);
    atomicMin(&J.bmin[3 * (size_t)nm + 0], f2ord(q.x));
    atomicMin(&J.bmin[3 * (size_t)nm + 1], f2ord(q.y));
    atomicMin(&J.bmin[3 * (size_t)nm + 2], f2ord(q.z));
    atomicMax(&J.bmax[3 * (size_t)nm + 0], f2ord(q.x));
    atomicMax(&J.bmax[3 * (size_t)nm + 1], f2ord(q.y));
    atomicMax(&J.bmax[3 * (size_t)nm + 2], f2ord(q.z));
    atomicAdd(&J.bcnt[nm], 1);
}

__global__ __launch_bounds__(kRgThreads) void k_rg_select(DevParams P, Arena A, RgJob J) {
    const int s = J.s0 + blockIdx.y;
    const int n = A.counts[(size_t)s * 8 + 4];
    const int i = blockIdx.x * kRgThreads + threadIdx.x;
    if (i >= n) return;
    const size_t base = (size_t)A.scan_off[s];
    const uint8_t t = A.pt_type[base + i];
    J.cls[base + i] = t;  // 0 erased, 1 tree, 2 car; the candidates' points get 1 or 3 from k_rg_grow
    J.out_nc[base + i] = make_float4(__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u),
                                     __uint_as_float(0x7fc00000u));
    J.out_seg[base + i] = -1;
    if (t != 1) return;
    const int nm = (int)(base - J.off0) + A.pt_cluster[base + i];
    const uint32_t* mn = J.bmin + 3 * (size_t)nm;
    const uint32_t* mx = J.bmax + 3 * (size_t)nm;
    if (!cc_rg_candidate(P, ord2f(mn[0]), ord2f(mn[1]), ord2f(mx[0]), ord2f(mx[1]))) return;
    const int slot = atomicAdd(&J.cnt[0], 1);
    J.key_in[slot] = ((uint64_t)(uint32_t)nm << 32) | (uint32_t)((int)(base - J.off0) + i);
}

// position p of the sorted keys: its scan and point; the first position of every cluster makes the cluster's record
__global__ __launch_bounds__(kRgThreads) void k_rg_group(Arena A, RgJob J) {
    const int p = blockIdx.x * kRgThreads + threadIdx.x;
    const int m = J.cnt[0];
    if (p >= m) return;
    const uint64_t key = J.key_out[p];
    const int g = (int)(uint32_t)key;
    int lo = J.s0, hi = J.s0 + J.ns - 1;  // scan of chunk point g: the last s with scan_off[s] - off0 <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)(A.scan_off[mid] - J.off0) <= g) lo = mid;
        else hi = mid - 1;
    }
    const int i = g - (int)(A.scan_off[lo] - J.off0);
    J.pl[p] = make_int2(lo, i);
    J.cxyz[p] = rg_point(A, J.from_apri, lo, i);
    if (p == 0 || (uint32_t)(J.key_out[p - 1] >> 32) != (uint32_t)(key >> 32)) {
        const int c = atomicAdd(&J.cnt[1], 1);
        const int nm = (int)(key >> 32);
        J.cl[c] = make_int2(p, J.bcnt[nm]);
        J.cl_name[c] = nm;
    }
}

// one workgroup per cluster (grid-stride): the grid's shape, the cluster id of its positions, the CSR cells at cell[3 p ..]
__global__ __launch_bounds__(kRgThreads) void k_rg_grid(RgJob J) {
    __shared__ int wsum[kRgThreads / 64 + 1];
    __shared__ BoxGrid G;
    const int ncl = J.cnt[1];
    for (int c = blockIdx.x; c < ncl; c += gridDim.x) {
        const int2 cr = J.cl[c];
        const int p0 = cr.x, n = cr.y, nm = J.cl_name[c];
        if (threadIdx.x == 0) {
            const uint32_t* mn = J.bmin + 3 * (size_t)nm;
            const uint32_t* mx = J.bmax + 3 * (size_t)nm;
            const float ox = ord2f(mn[0]), oy = ord2f(mn[1]), oz = ord2f(mn[2]);
            G = bg_shape(ox, oy, oz, ord2f(mx[0]) - ox, ord2f(mx[1]) - oy, ord2f(mx[2]) - oz, n, kRgShape);
            bg_store(J.grid + 2 * (size_t)c, G, 0);
        }
        for (int k = threadIdx.x; k < n; k += kRgThreads) J.pos_cl[p0 + k] = c;
        __syncthreads();
        // nc + 1 <= 2 n + 1 <= 3 n words of this cluster; the cell order is an indirection: cell_pts[rank] = position
        bg_csr_build<kRgThreads>(G, n, J.cell + 3 * (size_t)p0, J.pcell + p0, wsum, [&](int k) { return J.cxyz[p0 + k]; },
                                 [&](int k, int slot, float4) { J.cell_pts[p0 + slot] = p0 + k; });
        __syncthreads();
    }
}

// the k_eff nearest positions of p's cluster, ascending (d^2, position): scvod_boxgrid.h's search, the candidates of a run read
// through cell_pts
__global__ __launch_bounds__(kRgThreads) void k_rg_knn(RgJob J) {
    const int p = blockIdx.x * kRgThreads + threadIdx.x;
    if (p >= J.cnt[0]) return;
    const int c = J.pos_cl[p];
    const int2 cr = J.cl[c];
    const int p0 = cr.x, n = cr.y;
    const int keff = n < J.k ? n : J.k;
    const BoxGrid G = bg_load(J.grid + 2 * (size_t)c);
    const int* cell = J.cell + 3 * (size_t)p0;
    const float4 x = J.cxyz[p];
    const int cx = bg_cell1(x.x, G.ox, G.h, G.dx), cy = bg_cell1(x.y, G.oy, G.h, G.dy), cz = bg_cell1(x.z, G.oz, G.h, G.dz);
    float bd[kBoxGridK], kth;
    int bq[kBoxGridK], kq;
    bg_topk_clear(bd, bq, kth, kq);
    const float mg = bg_margin(G);
    for (int r = 0;; ++r) {
        bg_ring_runs(G, cx, cy, cz, r, [&](int ia, int ib, int, int) {
            int b, e;
            bg_run(cell, ia, ib, b, e);
            for (int t = b; t < e; ++t) {
                const int q = J.cell_pts[p0 + t];
                const float4 y4 = J.cxyz[q];
                bg_topk_insert(bg_dist2(y4.x, y4.y, y4.z, x.x, x.y, x.z), q, keff, bd, bq, kth, kq);
            }
        });
        if (bg_stop(bg_unprobed(G, cx, cy, cz, r, x.x, x.y, x.z), mg, kth)) break;
    }
    int* out = J.nbr + (size_t)p * J.k;
#pragma unroll
    for (int j = 0; j < kBoxGridK; ++j)
        if (j < keff) out[j] = bq[j];
}

__global__ __launch_bounds__(kRgThreads) void k_rg_normal(Arena A, RgJob J) {
    const int p = blockIdx.x * kRgThreads + threadIdx.x;
    if (p >= J.cnt[0]) return;
    const int n = J.cl[J.pos_cl[p]].y;
    const int keff = n < J.k ? n : J.k;
    const int* nb = J.nbr + (size_t)p * J.k;
    float o[4];
    point_normal_f32(keff, [&](int j, float& x, float& y, float& z) {
        const float4 q = J.cxyz[nb[j]];
        x = q.x;
        y = q.y;
        z = q.z;
    }, o);
    const float4 v = make_float4(o[0], o[1], o[2], o[3]);
    J.nrm[p] = v;
    const int2 pl = J.pl[p];
    J.out_nc[(size_t)A.scan_off[pl.x] + pl.y] = v;
}

// p capable (curvature not above the threshold; NaN is capable, as in validatePoint): bit j for the valid edge to its j-th neighbour
__global__ __launch_bounds__(kRgThreads) void k_rg_edges(RgJob J) {
    __shared__ int bsum;
    if (threadIdx.x == 0) bsum = 0;
    __syncthreads();
    const int p = blockIdx.x * kRgThreads + threadIdx.x;
    int e = 0;
    if (p < J.cnt[0]) {
        const int n = J.cl[J.pos_cl[p]].y;
        const int keff = n < J.k ? n : J.k;
        const float4 np = J.nrm[p];
        uint32_t m = 0;
        if (!(np.w > J.curv_thr)) {
            const float a[3] = {np.x, np.y, np.z};
            const int* nb = J.nbr + (size_t)p * J.k;
            for (int j = 0; j < keff; ++j) {
                const int q = nb[j];
                if (q == p) continue;
                const float4 nq = J.nrm[q];
                const float b[3] = {nq.x, nq.y, nq.z};
                if (rg_smooth_ok(b, a, J.cos_t)) m |= 1u << j;
            }
        }
        J.emask[p] = (uint16_t)m;
        e = __popc(m);
    }
    if (e) atomicAdd(&bsum, e);
    __syncthreads();
    if (threadIdx.x == 0 && bsum) atomicAdd(&J.stats[3], bsum);
}

__device__ __forceinline__ uint64_t rg_key(const RgJob& J, int p) {
    return ((uint64_t)rg_curv_key(J.nrm[p].w) << 32) | (uint32_t)p;
}

// block minimum of a 64-bit value (every thread gets it)
__device__ __forceinline__ uint64_t rg_block_min(uint64_t v, uint64_t* red) {
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t m = red[0];
    for (int w = 1; w < kRgThreads / 64; ++w) m = red[w] < m ? red[w] : m;
    return m;
}

// reads and writes of what other lanes of the workgroup change in HBM go past the CU's vector cache (atomics are performed in L2)
template <typename T>
__device__ __forceinline__ T rg_ld(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ void rg_st(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// labels of one cluster: in LDS (plain accesses) or in HBM (coherent accesses)
template <bool LDS>
struct RgLab {
    unsigned long long* a;
    __device__ __forceinline__ unsigned long long get(int k) const { return LDS ? a[k] : rg_ld(a + k); }
    __device__ __forceinline__ void put(int k, unsigned long long v) const {
        if (LDS) a[k] = v;
        else rg_st(a + k, v);
    }
};

template <bool LDS>
__device__ __forceinline__ void rg_grow_cluster(const Arena& A, const RgJob& J, int c, int p0, int n, RgLab<LDS> lab, int* changed,
                                                uint64_t* red, int* tcount, unsigned long long* plane) {
    const unsigned long long NONE = ~0ull;
    for (int k = threadIdx.x; k < n; k += kRgThreads) {
        const int p = p0 + k;
        lab.put(k, (J.nrm[p].w > J.curv_thr) ? NONE : rg_key(J, p));
        rg_st(J.segc + p, 0);
    }
    if (threadIdx.x == 0) {
        *tcount = 0;
        *plane = 0;
    }
    __syncthreads();
    // min-key propagation over the edges: Gauss-Seidel sweeps in alternating direction until a sweep changes nothing
    int rounds = 0;
    for (;;) {
        if (threadIdx.x == 0) *changed = 0;
        __syncthreads();
        const bool up = (rounds & 1) == 0;
        for (int k0 = threadIdx.x; k0 < n; k0 += kRgThreads) {
            const int k = up ? k0 : n - 1 - k0;
            const int p = p0 + k;
            const uint32_t m = J.emask[p];
            if (!m) continue;
            const unsigned long long lp = lab.get(k);
            const int* nb = J.nbr + (size_t)p * J.k;
            for (uint32_t mm = m; mm; mm &= mm - 1) {
                const int q = nb[__ffs(mm) - 1] - p0;
                if (lab.get(q) > lp) {
                    atomicMin(lab.a + q, lp);
                    *changed = 1;
                }
            }
        }
        ++rounds;
        __syncthreads();
        const int ch = *changed;
        __syncthreads();
        if (!ch) break;
    }
    // tail: the points still unlabelled (all non-capable), one by one in key order; each takes its valid unlabelled neighbours
    int* tail = J.tail + p0;
    for (int k = threadIdx.x; k < n; k += kRgThreads)
        if (lab.get(k) == NONE) rg_st(tail + atomicAdd(tcount, 1), p0 + k);
    __syncthreads();
    const int t = *tcount;
    for (int it = 0; it < t; ++it) {
        uint64_t v = NONE;
        for (int k = threadIdx.x; k < t; k += kRgThreads) {
            const int u = rg_ld(tail + k);
            if (lab.get(u - p0) == NONE) {
                const uint64_t key = rg_key(J, u);
                v = key < v ? key : v;
            }
        }
        const uint64_t mkey = rg_block_min(v, red);
        if (mkey == NONE) break;
        if (threadIdx.x == 0) {
            const int u = (int)(uint32_t)mkey;
            lab.put(u - p0, mkey);
            const float4 nu = J.nrm[u];
            const float a[3] = {nu.x, nu.y, nu.z};
            const int* nb = J.nbr + (size_t)u * J.k;
            const int keff = n < J.k ? n : J.k;
            for (int j = 0; j < keff; ++j) {
                const int q = nb[j];
                if (lab.get(q - p0) != NONE) continue;
                const float4 nq = J.nrm[q];
                const float b[3] = {nq.x, nq.y, nq.z};
                if (rg_smooth_ok(b, a, J.cos_t)) lab.put(q - p0, mkey);
            }
        }
        __syncthreads();
    }
    // segment sizes, the kept segments, the class
    for (int k = threadIdx.x; k < n; k += kRgThreads) atomicAdd(&J.segc[(int)(uint32_t)lab.get(k)], 1);
    __syncthreads();
    unsigned long long mine = 0;
    for (int k = threadIdx.x; k < n; k += kRgThreads) {
        const int sz = rg_ld(J.segc + p0 + k);
        if (sz >= J.min_seg && sz <= J.max_seg) mine += (unsigned long long)sz;
    }
    if (mine) atomicAdd(plane, mine);
    __syncthreads();
    const bool building = (double)*plane >= (double)n * J.frac;
    for (int k = threadIdx.x; k < n; k += kRgThreads) {
        const int2 pl = J.pl[p0 + k];
        const size_t o = (size_t)A.scan_off[pl.x] + pl.y;
        J.cls[o] = building ? 3 : 1;
        J.out_seg[o] = J.pl[(int)(uint32_t)lab.get(k)].y;
    }
    if (threadIdx.x == 0) {
        atomicAdd(&J.stats[0], 1);
        if (building) atomicAdd(&J.stats[1], 1);
        atomicAdd(&J.stats[2], n);
        atomicMax(&J.stats[4], rounds);
        if (!LDS) atomicAdd(&J.stats[5], 1);
        atomicAdd(&J.stats[6], t);
    }
    __syncthreads();
}

// one workgroup per cluster (grid-stride)
__global__ __launch_bounds__(kRgThreads) void k_rg_grow(Arena A, RgJob J) {
    extern __shared__ unsigned long long rg_lds[];
    __shared__ int changed, tcount;
    __shared__ uint64_t red[kRgThreads / 64];
    __shared__ unsigned long long plane;
    const int ncl = J.cnt[1];
    for (int c = blockIdx.x; c < ncl; c += gridDim.x) {
        const int2 cr = J.cl[c];
        if (cr.y <= kRgLdsPts)
            rg_grow_cluster<true>(A, J, c, cr.x, cr.y, RgLab<true>{rg_lds}, &changed, red, &tcount, &plane);
        else
            rg_grow_cluster<false>(A, J, c, cr.x, cr.y, RgLab<false>{(unsigned long long*)J.lab + cr.x}, &changed, red, &tcount, &plane);
    }
}
