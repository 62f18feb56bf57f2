// scvod_k_patchwork.inc -- Patchwork: classify / scatter / sort tiers / plane fit / arrange / ordered emission with the fused curved-voxel binning (A1-A4).
// Part of the kernels translation unit: included by scvod_kernels.hip (inside namespace scvod), never compiled on its own.
// ------------------------------------------------------------------------------------------
// Patchwork stage 1: per point patch id + per-(scan, patch) histogram.
// grid = (ceil(max_scan_pts / (256*ITEMS)), B), block = 256.  Coalesced float4 loads.
// ------------------------------------------------------------------------------------------
constexpr int kClsThreads = 256;
constexpr int kClsItems = 8;

__global__ __launch_bounds__(kClsThreads) void k_pw_classify(DevParams P, Arena A) {
    __shared__ int hist[kMaxPatches];
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int n = A.scan_off[s + 1] - base;
    const int start = blockIdx.x * (kClsThreads * kClsItems);
    if (start >= n) return;
    for (int b = threadIdx.x; b < P.n_patches; b += kClsThreads) hist[b] = 0;
    __syncthreads();
    // all loads first (8 x 16 B in flight per lane), then the fp64 zone / ring / sector arithmetic
    float4 pt[kClsItems];
#pragma unroll
    for (int it = 0; it < kClsItems; ++it) {
        const int i = start + it * kClsThreads + threadIdx.x;
        pt[it] = A.pts[base + min(i, n - 1)];
    }
#pragma unroll
    for (int it = 0; it < kClsItems; ++it) {
        const int i = start + it * kClsThreads + threadIdx.x;
        if (i < n) {
            const float4 p = pt[it];
            int pid = czm_patch_of(P.czm, p.x, p.y, p.z);
            A.pid[base + i] = (int16_t)pid;
            A.zkey[base + i] = float_sort_key(p.z);
            if (pid >= 0) atomicAdd(&hist[pid], 1);  // (grouping the wave's lanes by bin -- or by runs of equal ids -- costs more than it saves here)
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < P.n_patches; b += kClsThreads) {
        int c = hist[b];
        if (c) atomicAdd(&A.patch_count[s * kMaxPatches + b], c);
    }
}

// per scan exclusive scan of the patch histogram.  grid = B, block = 1024.
__global__ __launch_bounds__(1024) void k_pw_offsets(DevParams P, Arena A) {
    __shared__ int wsum[17];
    const int s = blockIdx.x;
    int c = (threadIdx.x < (unsigned)P.n_patches) ? A.patch_count[s * kMaxPatches + threadIdx.x] : 0;
    int total;
    int ex = block_excl_scan<1024>(c, total, wsum);
    if (threadIdx.x <= (unsigned)P.n_patches) A.patch_off[s * (kMaxPatches + 1) + threadIdx.x] = ex;
}

// scatter (z key, idx) into patch-major order.  Position inside the patch is arbitrary (the
// patch kernel sorts); block-aggregated so that there is one global atomic per (block, patch).
__global__ __launch_bounds__(kClsThreads) void k_pw_scatter(DevParams P, Arena A) {
    __shared__ int hist[kMaxPatches];
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int n = A.scan_off[s + 1] - base;
    const int start = blockIdx.x * (kClsThreads * kClsItems);
    if (start >= n) return;
    for (int b = threadIdx.x; b < P.n_patches; b += kClsThreads) hist[b] = 0;
    __syncthreads();
    int pid[kClsItems], rank[kClsItems];
    uint32_t zk[kClsItems];
#pragma unroll
    for (int it = 0; it < kClsItems; ++it) {
        const int i = start + it * kClsThreads + threadIdx.x;
        pid[it] = (i < n) ? (int)A.pid[base + i] : -1;
        zk[it] = A.zkey[base + min(i, n - 1)];
    }
#pragma unroll
    for (int it = 0; it < kClsItems; ++it)
        rank[it] = wave_bin_rank(hist, pid[it]);
    __syncthreads();
    for (int b = threadIdx.x; b < P.n_patches; b += kClsThreads) {
        int c = hist[b];
        if (c) hist[b] = A.patch_off[s * (kMaxPatches + 1) + b] + atomicAdd(&A.patch_cursor[s * kMaxPatches + b], c);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kClsItems; ++it) {
        int i = start + it * kClsThreads + threadIdx.x;
        if (i < n && pid[it] >= 0) A.keys[(size_t)base + hist[pid[it]] + rank[it]] = pack_key(zk[it], (uint32_t)i);
    }
}

// ------------------------------------------------------------------------------------------
// Patchwork stage 2 (extract_piecewiseground + gating), split so that every phase has the
// parallel shape that fits it:
//   k_pw_order_*  counting sort of the live patches of the whole batch by quarter-octave size class into order[];
//                 every later kernel is list-driven (persistent grids striding over their slice of the list).
//   k_pw_sort*    tiers by size class: LDS bitonic sort of the patch's (z, idx) keys, then the patch's points are
//                 written in sorted order (packed xyz + input index).
//   k_pw_fit_coop patches of >= 512 points (>= 64 for a handful of scans): GL lanes per patch; products in parallel,
//                 the nine sequential fp32 sums on nine lanes; then the same lanes arrange the patch (arrange_group); LEAN form:
//                 they also bin its kept non-ground points (packed index triple into zkey).
//   k_pw_fit      the smaller patches, ONE LANE PER PATCH (the 3x3 Jacobi SVD then costs one lane, not one wave),
//                 reads staged cooperatively through LDS.
//   k_pw_arrange  the patches of k_pw_fit, one wave per patch: final plane test, [ground part | non-ground part] arrangement
//                 and the per-patch counters the ordered emission needs; LEAN form as arrange_group's.
// ------------------------------------------------------------------------------------------
// size classes (pw_size_class) that bound the sort tiers: class 40 <=> n >= 1024, class 48 <=> n >= 4096
constexpr int kClassXS = 32, kClassM = 40, kClassM2 = 44, kClassL = 48;  // n >= 256 / 1024 / 2048 / 4096
#ifndef SCVOD_FIT_COOP_CLASS
#define SCVOD_FIT_COOP_CLASS 36
#endif
constexpr int kClassFitCoop = SCVOD_FIT_COOP_CLASS;  // 36: n >= 512: plane fit by 16 lanes per patch (k_pw_fit_coop)

// order[] lists live items by descending size class; positions of classes [C_LO, C_HI]
__device__ __forceinline__ void order_range(const int32_t* off, int c_lo, int c_hi, int& lo, int& hi) {
    lo = off[c_hi];
    hi = (c_lo == 0) ? off[64] : off[c_lo - 1];
}

// which tiers run the pad-free network (scvod_sortnet.h): those measured faster with it (profiles/padfree_sort_cost.md);
// the 256 tier is slower and the 1024 tier within noise, they keep the padded network.  SCVOD_SORT_PADFREE=0: none, 2: all
constexpr bool pw_sort_padfree(int cap) { return SCVOD_SORT_PADFREE == 2 || (SCVOD_SORT_PADFREE == 1 && cap >= 2048); }
// which tiers merge their register runs by merge path (scvod_mergepath.h) instead of running the network's later stages: those
// measured faster with it (profiles/merge_sort_cost.md): the 4096 and 8192 tiers; the 2048 tier's gain is within the noise of one
// kernel's figure, it keeps the network.  Only tiers with one 16-key window per thread that run the pad-free start can; the 16 384
// tier and the tiers below 2048 are not candidates.  SCVOD_SORT_MERGE=0: none, 2: the 2048 tier too
constexpr bool pw_sort_merge(int cap) {
    return pw_sort_padfree(cap) && cap >= 2048 && cap <= 8192 && (SCVOD_SORT_MERGE == 2 || (SCVOD_SORT_MERGE == 1 && cap >= 4096));
}

// (the pad-free network carries a predicated and an unpredicated form of every pass: the register budget is held to the
//  four waves per SIMD that the launches below put on a CU -- what the padded network reached on its own; the few values
//  the two large tiers spill are per-item ones, none is touched between the barriers of the network)
template <int CAP, int THREADS, int C_LO, int C_HI, int LGE>
__global__ __launch_bounds__(THREADS)
__attribute__((amdgpu_waves_per_eu(pw_sort_padfree(CAP) ? (CAP >= 1024 ? 4 : 6) : 1, 8)))
void k_pw_sort(DevParams P, Arena A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int lo, hi;
    order_range(A.order_off, C_LO, C_HI, lo, hi);
    constexpr int PK = (CAP == 4096) ? 1 : 2;  // (profiling build: the two large tiers are clocked)
    constexpr bool PADFREE = pw_sort_padfree(CAP);
    constexpr bool MERGE = pw_sort_merge(CAP) && LGE == 4 && (THREADS << LGE) == CAP;  // one window of 16 outputs per thread
    PROF_BEGIN();
    for (int w = lo + blockIdx.x; w < hi; w += gridDim.x) {
        const int4 item = A.order[w];
        const int n = item.y, base = item.z, off = item.w;
        const bool in_lds = (n <= CAP);
        unsigned long long* keys;
        if (CAP >= 4096) PROF_RESET();
        if (in_lds) {
            keys = (unsigned long long*)smem;
            int np2 = 1 << LGE;
            while (np2 < n) np2 <<= 1;
            const int nlive = sortnet::live_end(n, LGE);
            // a full tier: all of a thread's key loads in flight together (coalesced), sorted straight from the registers
            constexpr int IT = CAP / THREADS;
            const unsigned long long* gk = (const unsigned long long*)A.keys + (size_t)base + off;
            bool from_regs = false;
            if constexpr (IT == (1 << LGE) && CAP >= 4096) {  // (the small tiers are occupancy-bound: they keep their registers)
                if (np2 == CAP) {
                    from_regs = true;
                    unsigned long long tmp[IT];
                    if constexpr (PADFREE) {  // the first nlive / IT threads hold the keys, coalesced among themselves
                        if ((int)threadIdx.x < (nlive >> LGE)) {
#pragma unroll
                            for (int it = 0; it < IT; ++it) {
                                const int j = sortnet::start_key(it, (int)threadIdx.x, nlive, LGE);
                                tmp[it] = (j < n) ? gk[j] : kKeyPad;
                            }
                        }
                        if (CAP >= 4096) PROF_MARK(PK, 0);
                        if constexpr (MERGE)
                            mergepath_sort_regs<THREADS, true, LGE, SCVOD_SORT_MERGE_RUN>(tmp, keys, np2, nlive, (unsigned long long)kKeyPad);
                        else
                            padfree_sort_regs<THREADS, true, LGE>(tmp, keys, np2, nlive, (unsigned long long)kKeyPad);
                    } else {
#pragma unroll
                        for (int it = 0; it < IT; ++it) {
                            const int j = it * THREADS + (int)threadIdx.x;
                            tmp[it] = (j < n) ? gk[j] : kKeyPad;
                        }
                        if (CAP >= 4096) PROF_MARK(PK, 0);
                        block_bitonic_sort_pow2_regs<THREADS, true, LGE>(tmp, keys);
                    }
                }
            }
            if (!from_regs) {
                const int nfill = PADFREE ? nlive : np2;  // (pad-free: slots >= nlive are never touched)
                for (int j = threadIdx.x; j < nfill; j += THREADS) keys[sort_slot<true>(j)] = (j < n) ? gk[j] : kKeyPad;
                __syncthreads();
                if (CAP >= 4096) PROF_MARK(PK, 0);
                if constexpr (MERGE)
                    mergepath_sort<THREADS, true, LGE, SCVOD_SORT_MERGE_RUN>(keys, np2, nlive, (unsigned long long)kKeyPad);
                else if constexpr (PADFREE)
                    padfree_sort<THREADS, true, LGE>(keys, np2, nlive, (unsigned long long)kKeyPad);
                else
                    block_bitonic_sort_pow2<THREADS, true, LGE>(keys, np2);
            }
            if (CAP >= 4096) PROF_MARK(PK, 1);
        } else {
            keys = (unsigned long long*)(A.keys + (size_t)base + off);  // oversize patch: sort in place in global memory
            block_bitonic_sort<THREADS, false>(keys, n);
        }
        Xyz* dst = A.sorted_xyz + (size_t)base + off;
        uint32_t* dsti = A.sorted_idx + (size_t)base + off;
        // four independent gathers in flight per thread (the index comes from LDS, the point from anywhere in the scan)
        for (int j0 = threadIdx.x; j0 < n; j0 += 4 * THREADS) {
            uint32_t id[4];
            float4 q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = min(j0 + u * THREADS, n - 1);
                id[u] = key_idx(keys[in_lds ? sort_slot<true>(j) : j]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) q[u] = A.pts[base + id[u]];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u * THREADS;
                if (j < n) {
                    Xyz o;
                    o.x = q[u].x;
                    o.y = q[u].y;
                    o.z = q[u].z;
                    dst[j] = o;
                    dsti[j] = id[u];
                }
            }
        }
        __syncthreads();  // LDS is reused by the next item
        if (CAP >= 4096) PROF_MARK(PK, 2);
    }
}

// patches with fewer than 64 points: one key per lane, bitonic network over the wave with xor-shuffles
// (21 compare-exchange steps, no LDS, no barriers); four patches per 256-thread workgroup
constexpr int kClassWave = 24;  // pw_size_class(64)
__global__ __launch_bounds__(256) void k_pw_sort_wave(DevParams P, Arena A) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    int lo, hi;
    order_range(A.order_off, 0, kClassWave - 1, lo, hi);
    for (int w = lo + blockIdx.x * 4 + wave; w < hi; w += gridDim.x * 4) {
        const int4 item = A.order[w];
        const int n = item.y, base = item.z, off = item.w;  // n < 64
        unsigned long long key = (lane < n) ? A.keys[(size_t)base + off + lane] : kKeyPad;
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
            for (int j = k >> 1; j >= 1; j >>= 1) {
                const unsigned long long other = __shfl_xor(key, j, 64);
                const bool take_min = (((lane & k) == 0) == ((lane & j) == 0));
                unsigned long long mn = key, mx = other;
                cswap_asc(mn, mx);
                key = take_min ? mn : mx;
            }
        }
        if (lane < n) {
            const uint32_t id = key_idx(key);
            const float4 q = A.pts[base + id];
            Xyz o;
            o.x = q.x;
            o.y = q.y;
            o.z = q.z;
            A.sorted_xyz[(size_t)base + off + lane] = o;
            A.sorted_idx[(size_t)base + off + lane] = id;
        }
    }
}

__device__ __forceinline__ int pw_size_class(int n) {  // quarter-octave classes, 0..63
    int lg = 31 - __clz(n);
    int frac = (lg >= 2) ? ((n >> (lg - 2)) & 3) : 0;
    int c = lg * 4 + frac;
    return c > 63 ? 63 : c;
}

__global__ __launch_bounds__(256) void k_pw_order_count(DevParams P, Arena A) {
    __shared__ int hist[64];
    if (threadIdx.x < 64) hist[threadIdx.x] = 0;
    __syncthreads();
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < A.n_scans * P.n_patches) {
        const int s = t / P.n_patches, p = t - s * P.n_patches;
        const int n = A.patch_count[s * kMaxPatches + p];
        if (n <= P.czm.num_min_pts) {  // skipped patch (patchwork.h:331): record only
            PatchRec r = {n, 0, 0, 0, 0};
            A.patch_rec[s * kMaxPatches + p] = r;
            scvod_patch_plane pl = {};
            pl.n_pts = n;
            A.planes[s * kMaxPatches + p] = pl;
        } else {
            atomicAdd(&hist[pw_size_class(n)], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64 && hist[threadIdx.x]) atomicAdd(&A.order_hist[threadIdx.x], hist[threadIdx.x]);
}

__global__ __launch_bounds__(64) void k_pw_order_offsets(Arena A) {
    // descending size: class 63 first
    const int c = 63 - threadIdx.x;
    const int v = A.order_hist[c];
    const int inc = wave_incl_scan(v);
    A.order_off[c] = inc - v;
    if (threadIdx.x == 63) A.order_off[64] = inc;  // number of live patches
}

__global__ __launch_bounds__(256) void k_pw_order_scatter(DevParams P, Arena A) {
    __shared__ int hist[64];
    if (threadIdx.x < 64) hist[threadIdx.x] = 0;
    __syncthreads();
    const int t = blockIdx.x * 256 + threadIdx.x;
    int c = -1, rank = 0;
    int4 item = make_int4(0, 0, 0, 0);
    if (t < A.n_scans * P.n_patches) {
        const int s = t / P.n_patches, p = t - s * P.n_patches;
        const int n = A.patch_count[s * kMaxPatches + p];
        if (n > P.czm.num_min_pts) {
            c = pw_size_class(n);
            rank = atomicAdd(&hist[c], 1);
            item = make_int4(s * kMaxPatches + p, n, A.scan_off[s], A.patch_off[s * (kMaxPatches + 1) + p]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64 && hist[threadIdx.x])
        hist[threadIdx.x] = A.order_off[threadIdx.x] + atomicAdd(&A.order_cursor[threadIdx.x], hist[threadIdx.x]);
    __syncthreads();
    if (c >= 0) A.order[hist[c] + rank] = item;  // {scan*1024 + patch, n, scan base, patch offset}
}

// the same ordering for voxel buckets (counts in vb_count, min size 1)
__global__ __launch_bounds__(256) void k_vx_order_count(DevParams P, Arena A) {
    __shared__ int hist[64];
    if (threadIdx.x < 64) hist[threadIdx.x] = 0;
    __syncthreads();
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < A.n_scans * P.n_buckets) {
        const int s = t / P.n_buckets, b = t - s * P.n_buckets;
        const int m = A.vb_count[s * kMaxBuckets + b];
        if (m > 0)
            atomicAdd(&hist[pw_size_class(m)], 1);
        else
            A.vb_nvox[s * kMaxBuckets + b] = 0;
    }
    __syncthreads();
    if (threadIdx.x < 64 && hist[threadIdx.x]) atomicAdd(&A.vorder_hist[threadIdx.x], hist[threadIdx.x]);
}

__global__ __launch_bounds__(64) void k_vx_order_offsets(Arena A) {
    const int c = 63 - threadIdx.x;
    const int v = A.vorder_hist[c];
    const int inc = wave_incl_scan(v);
    A.vorder_off[c] = inc - v;
    if (threadIdx.x == 63) A.vorder_off[64] = inc;
}

__global__ __launch_bounds__(256) void k_vx_order_scatter(DevParams P, Arena A) {
    __shared__ int hist[64];
    if (threadIdx.x < 64) hist[threadIdx.x] = 0;
    __syncthreads();
    const int t = blockIdx.x * 256 + threadIdx.x;
    int c = -1, rank = 0;
    int4 item = make_int4(0, 0, 0, 0);
    if (t < A.n_scans * P.n_buckets) {
        const int s = t / P.n_buckets, b = t - s * P.n_buckets;
        const int m = A.vb_count[s * kMaxBuckets + b];
        if (m > 0) {
            c = pw_size_class(m);
            rank = atomicAdd(&hist[c], 1);
            item = make_int4(s * kMaxBuckets + b, m, A.scan_off[s], A.vb_off[s * (kMaxBuckets + 1) + b]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64 && hist[threadIdx.x])
        hist[threadIdx.x] = A.vorder_off[threadIdx.x] + atomicAdd(&A.vorder_cursor[threadIdx.x], hist[threadIdx.x]);
    __syncthreads();
    if (c >= 0) A.vorder[hist[c] + rank] = item;
}

// per-point plane residual, Eigen GEMV order: fl(fl(x*n0 + y*n1) + z*n2)
__device__ __forceinline__ float plane_res(const Xyz& q, float n0, float n1, float n2) {
    float r = q.x * n0;
    r = r + q.y * n1;
    r = r + q.z * n2;
    return r;
}

struct FitState {
    float cov[9];
    float mean0, mean1, mean2;
    float n0, n1, n2, thd;
    float sv0, sv1, sv2;
};
__device__ __forceinline__ void fit_state_init(FitState& F) {
#pragma unroll
    for (int k = 0; k < 9; ++k) F.cov[k] = 0.f;
    F.mean0 = F.mean1 = F.mean2 = 0.f;
    F.n0 = F.n1 = F.n2 = F.thd = 0.f;
    F.sv0 = F.sv1 = F.sv2 = 0.f;
}

// estimate_plane_ (patchwork.h:206-232) from the nine sums of pcl::computeMeanAndCovarianceMatrix
__device__ __forceinline__ void fit_update(FitState& F, const CzmParams& cz, float a0, float a1, float a2, float a3, float a4,
                                           float a5, float a6, float a7, float a8, int m) {
    if (m != 0) {  // an empty set leaves cov_/pc_mean_ untouched (PCL)
        const float fn = (float)m;
        a0 = a0 / fn;
        a1 = a1 / fn;
        a2 = a2 / fn;
        a3 = a3 / fn;
        a4 = a4 / fn;
        a5 = a5 / fn;
        a6 = a6 / fn;
        a7 = a7 / fn;
        a8 = a8 / fn;
        F.mean0 = a6;
        F.mean1 = a7;
        F.mean2 = a8;
        F.cov[0] = a0 - a6 * a6;
        F.cov[1] = a1 - a6 * a7;
        F.cov[2] = a2 - a6 * a8;
        F.cov[4] = a3 - a7 * a7;
        F.cov[5] = a4 - a7 * a8;
        F.cov[8] = a5 - a8 * a8;
        F.cov[3] = F.cov[1];
        F.cov[6] = F.cov[2];
        F.cov[7] = F.cov[5];
    }
    Svd3 sv;
    svd3_jacobi(F.cov, sv);
    F.n0 = sv.U[2];
    F.n1 = sv.U[5];
    F.n2 = sv.U[8];
    F.sv0 = sv.sv[0];
    F.sv1 = sv.sv[1];
    F.sv2 = sv.sv[2];
    float dot = F.n0 * F.mean0;
    dot = dot + F.n1 * F.mean1;
    dot = dot + F.n2 * F.mean2;
    const float d = -dot;
    F.thd = (float)(cz.th_dist - (double)d);
}

// gate of a fitted patch (patchwork.h:339-384): 1 kept, 2 rejected (tilt), 3 rejected (elevation + flatness)
__device__ __forceinline__ int fit_status(const DevParams& P, int zone, int ring, int concentric_idx, const FitState& F) {
    const double ground_z_vec = (double)fabs_f(F.n2);
    const double ground_z_elevation = (double)F.mean2;
    float svmin = F.sv0;
    if (F.sv1 < svmin) svmin = F.sv1;
    if (F.sv2 < svmin) svmin = F.sv2;
    const double surface_variable = (double)(svmin / (F.sv0 + F.sv1 + F.sv2));
    if (ground_z_vec < P.czm.uprightness_thr) return 2;
    if (concentric_idx < P.czm.num_rings_of_interest) {
        const int e = ring + 2 * zone;
        if (ground_z_elevation > P.czm.elevation_thr[e]) return (P.czm.flatness_thr[e] > surface_variable) ? 1 : 3;
    }
    return 1;
}

__device__ __forceinline__ void fit_finish(const DevParams& P, const Arena& A, int s, int p, int n, int zone, int ring,
                                           int concentric_idx, const FitState& F) {
    const float n0 = F.n0, n1 = F.n1, n2 = F.n2, thd = F.thd, mean0 = F.mean0, mean1 = F.mean1, mean2 = F.mean2;
    const float sv0 = F.sv0, sv1 = F.sv1, sv2 = F.sv2;
    const int status = fit_status(P, zone, ring, concentric_idx, F);
    scvod_patch_plane pl;
    pl.normal[0] = n0;
    pl.normal[1] = n1;
    pl.normal[2] = n2;
    pl.mean[0] = mean0;
    pl.mean[1] = mean1;
    pl.mean[2] = mean2;
    pl.sv[0] = sv0;
    pl.sv[1] = sv1;
    pl.sv[2] = sv2;
    pl.n_pts = n;
    pl.n_ground = 0;  // filled by k_pw_arrange
    pl.status = status;
    A.planes[s * kMaxPatches + p] = pl;
    A.fit_thd[s * kMaxPatches + p] = thd;
}

// index triple of a point that passed the range/FOV test, packed (pack_idx3): the guarded estimate decides it away from the bin
// edges, the reference arithmetic next to one.  The lean emission's arrange pass computes it from the coordinates it holds anyway.
__device__ __forceinline__ uint32_t triple_of_point(const DevParams& P, float x, float y, float z) {
    int32_t ri, si, ai;
    if (!idx3_fast(P.bin, P.binfast, x, y, z, &ri, &si, &ai)) {
        Apri a;
        apri_of_point(P.bin, x, y, z, 0.f, a);
        ri = a.range_idx;
        si = a.sector_idx;
        ai = a.azimuth_idx;
    }
    return (uint32_t)pack_idx3(ri, si, ai);
}

// Final plane test of every point of a fitted patch (patchwork.h:488-501) by the GL lanes that fitted it: [ground part -> | <- non-ground
// part] arrangement in z order (element r of the non-ground part lives at seg[n - 1 - r]; k_emit reads it that way), the range/FOV
// verdict of makeApriVec for the points that reach the non-ground stream, the per-patch counters the ordered emission needs.
// Wave-uniform call (ballots): groups without a patch pass n = 0.  n_max = largest n of the wave's groups.
// LEAN (the lean emission): a kept point's packed index triple goes to stage[] at the position of its seg word, so that k_emit<true>
// never fetches the point again.
template <int GL, bool LEAN>
__device__ __forceinline__ void arrange_group(const DevParams& P, const Arena& A, const Xyz* __restrict__ sp, const uint32_t* __restrict__ si, uint32_t* seg,
                                              uint32_t* stage, int n, int n_max, int slot, bool live, int r, int gbase, float n0, float n1, float n2, float thd, int status) {
    constexpr unsigned long long FULL = (GL == 64) ? ~0ull : ((1ull << (GL & 63)) - 1ull);
    auto group_bits = [&](unsigned long long ballot) -> unsigned long long { return (ballot >> gbase) & FULL; };
    const bool rejected = (status >= 2);
    const int n_last = max(n - 1, 0);
    int n_g = 0, n_ng = 0, a_g = 0, a_ng = 0;
    Xyz q_next = sp[min(r, n_last)];
    uint32_t w_next = si[min(r, n_last)];
    const unsigned long long below = (1ull << r) - 1ull;
    for (int j0 = 0; j0 < n_max; j0 += GL) {
        const int j = j0 + r;
        int g = 0, keep = 0;
        const Xyz q = q_next;
        uint32_t w = w_next;
        q_next = sp[min(j + GL, n_last)];  // the next GL points are in flight while this step is classified (clamped, unconditional loads)
        w_next = si[min(j + GL, n_last)];
        if (j < n) {
            g = plane_res(q, n0, n1, n2) < thd;
            if (!g || rejected) {
                keep = keep_of_point(P.bin, P.keep, q.x, q.y, q.z);
                w |= keep ? 0x80000000u : 0u;
            }
        }
        const unsigned long long bg = group_bits(__ballot(g));
        const unsigned long long bn = group_bits(__ballot(!g && j < n));
        if (j < n) {
            if (g)
                seg[n_g + __popcll(bg & below)] = w;
            else
                seg[n - 1 - (n_ng + __popcll(bn & below))] = w;
            if constexpr (LEAN) {
                if (keep) stage[g ? n_g + __popcll(bg & below) : n - 1 - (n_ng + __popcll(bn & below))] = triple_of_point(P, q.x, q.y, q.z);
            }
        }
        a_g += __popcll(group_bits(__ballot(g && keep)));
        a_ng += __popcll(group_bits(__ballot(!g && keep && j < n)));
        n_g += __popcll(bg);
        n_ng += __popcll(bn);
    }
    if (live && r == 0) {
        PatchRec rec;
        rec.n = n;
        rec.n_g = n_g;
        rec.status = status;
        rec.a_g = a_g;
        rec.a_ng = a_ng;
        A.patch_rec[slot] = rec;
        A.planes[slot].n_ground = n_g;
    }
}

// Every lane owns one patch (the fp32 sums of the fit are strictly sequential, so a patch cannot be
// split across lanes), but the wave READS cooperatively: per step it copies the next kFitCh points of
// each of its 64 patches into LDS with contiguous 192-byte runs per patch, and every lane then consumes
// its own row.  A lane-per-patch walk straight from global memory touches 64 different cache lines per
// load instruction and was bound by the L1/TA, not by HBM.
constexpr int kFitCh = 16;               // points per patch per step
constexpr int kFitRow = kFitCh * 3;      // dwords per patch per step
constexpr int kFitQuads = kFitRow / 4;   // 16-byte quads per row (12)
constexpr int kFitStride = kFitRow + 4;  // row stride 52 dwords: 16-byte aligned rows, b128 row accesses of 8
                                         // consecutive lanes cover all 32 banks once
constexpr int kFitLoads = kFitQuads;     // 64 lanes x 12 quad loads cover 64 rows x 12 quads

typedef float fitq_mem __attribute__((ext_vector_type(4), aligned(4)));  // rows start on any point boundary
typedef float fitq __attribute__((ext_vector_type(4)));

struct FitTile {
    fitq row[64 * kFitStride / 4];
    uint32_t start[64];  // first point of the lane's patch in sorted_xyz (units of points)
    int n[64];
};

// fetch step `c` of all 64 patches into registers (12 quads per lane): load j covers quad f = j * 64 + lane
// = row f / 12, quad f % 12.  A quad is fetched when its first dword belongs to the patch; its tail may run up to
// 12 bytes into whatever follows (never consumed: the consumers test the point index).
__device__ __forceinline__ void fit_fetch(const FitTile& T, const float* __restrict__ src, int c, int lane, fitq (&r)[kFitLoads]) {
#pragma unroll
    for (int j = 0; j < kFitLoads; ++j) {
        const int f = j * 64 + lane;
        const int pp = f / kFitQuads;
        const int w = (f - pp * kFitQuads) * 4;
        const int pt = c * kFitCh + w / 3;
        fitq v = {0.f, 0.f, 0.f, 0.f};
        if (pt < T.n[pp]) v = *(const fitq_mem*)(src + ((size_t)T.start[pp] * 3 + (size_t)(c * kFitRow + w)));
        r[j] = v;
    }
}
__device__ __forceinline__ void fit_store(FitTile& T, int lane, const fitq (&r)[kFitLoads]) {
#pragma unroll
    for (int j = 0; j < kFitLoads; ++j) {
        const int f = j * 64 + lane;
        const int pp = f / kFitQuads;
        const int w4 = f - pp * kFitQuads;
        T.row[pp * (kFitStride / 4) + w4] = r[j];
    }
}

__global__ __launch_bounds__(64) void k_pw_fit(DevParams P, Arena A, int coop_class) {
    __shared__ FitTile T;
    const int lane = threadIdx.x;
    int lo, hi;
    order_range(A.order_off, 0, coop_class - 1, lo, hi);  // the larger patches go to k_pw_fit_coop
    const int t = lo + blockIdx.x * 64 + lane;
    if (lo + blockIdx.x * 64 >= hi) return;
    const bool live = t < hi;
    const int4 item = live ? A.order[t] : make_int4(0, 0, 0, 0);
    const int code = item.x;
    const int s = code / kMaxPatches, p = code - s * kMaxPatches;
    const int n = live ? item.y : 0;
    T.start[lane] = (uint32_t)(item.z + item.w);
    T.n[lane] = n;
    int n_max = n;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n_max = max(n_max, __shfl_xor(n_max, d));
    const int n_steps = (n_max + kFitCh - 1) / kFitCh;
    const float* __restrict__ src = (const float*)A.sorted_xyz;
    const fitq* myq = T.row + lane * (kFitStride / 4);
    __syncthreads();

    int zone = 0;
    while (zone < 3 && p >= P.czm.patch_base[zone + 1]) ++zone;
    const int ring = (p - P.czm.patch_base[zone]) / P.czm.num_sectors[zone];
    int concentric_idx = ring;
    for (int k = 0; k < zone; ++k) concentric_idx += P.czm.num_rings[k];

    fitq regs[kFitLoads];
    float my[kFitRow];

    // ---- extract_initial_seeds_ (patchwork.h:235-268): skip the too-low prefix (zone 0), mean z of the
    // next num_lpr points ----
    double sum = 0;
    int cnt = 0;
    {
        bool skipping = (zone == 0);
        bool busy = n > 0;
        fit_fetch(T, src, 0, lane, regs);
        for (int c = 0; c < n_steps; ++c) {
            fit_store(T, lane, regs);
            __syncthreads();
            if (c + 1 < n_steps) fit_fetch(T, src, c + 1, lane, regs);
            if (busy) {
#pragma unroll
                for (int g = 0; g < kFitQuads; ++g) {
                    const fitq v = myq[g];
                    my[4 * g] = v.x;
                    my[4 * g + 1] = v.y;
                    my[4 * g + 2] = v.z;
                    my[4 * g + 3] = v.w;
                }
#pragma unroll
                for (int k = 0; k < kFitCh; ++k) {
                    const float z = my[3 * k + 2];
                    const bool valid = (c * kFitCh + k < n);
                    if (skipping && !(valid && (double)z < P.czm.seed_margin_z)) skipping = false;
                    if (valid && !skipping && cnt < P.czm.num_lpr) {
                        sum += (double)z;
                        ++cnt;
                    }
                }
                if ((!skipping && cnt >= P.czm.num_lpr) || (c + 1) * kFitCh >= n) busy = false;
            }
            __syncthreads();
            if (!__any(busy)) break;
        }
    }
    const double lpr = cnt != 0 ? sum / cnt : 0.0;
    const double seed_thr = lpr + P.czm.th_seeds;

    FitState F;
    fit_state_init(F);

    for (int iter = 0; iter < P.czm.num_iter; ++iter) {
        const float n0 = F.n0, n1 = F.n1, n2 = F.n2, thd = F.thd;
        // pcl::computeMeanAndCovarianceMatrix over the current ground set, strictly in z order.  Membership
        // is a select; adding +0.0f is exact here because the accumulators can never be -0.0f.
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f, a8 = 0.f;
        int m = 0;
        bool busy = n > 0;
        fit_fetch(T, src, 0, lane, regs);
        for (int c = 0; c < n_steps; ++c) {
            fit_store(T, lane, regs);
            __syncthreads();
            if (c + 1 < n_steps) fit_fetch(T, src, c + 1, lane, regs);  // in flight while this step is summed
            if (busy) {
#pragma unroll
                for (int g = 0; g < kFitQuads; ++g) {
                    const fitq v = myq[g];
                    my[4 * g] = v.x;
                    my[4 * g + 1] = v.y;
                    my[4 * g + 2] = v.z;
                    my[4 * g + 3] = v.w;
                }
#pragma unroll
                for (int k = 0; k < kFitCh; ++k) {
                    Xyz q;
                    q.x = my[3 * k];
                    q.y = my[3 * k + 1];
                    q.z = my[3 * k + 2];
                    bool in = (c * kFitCh + k < n);
                    if (iter == 0)
                        in = in && ((double)q.z < seed_thr);
                    else
                        in = in && (plane_res(q, n0, n1, n2) < thd);
                    const float t0 = q.x * q.x, t1 = q.x * q.y, t2 = q.x * q.z, t3 = q.y * q.y, t4 = q.y * q.z,
                                t5 = q.z * q.z;
                    a0 += in ? t0 : 0.f;
                    a1 += in ? t1 : 0.f;
                    a2 += in ? t2 : 0.f;
                    a3 += in ? t3 : 0.f;
                    a4 += in ? t4 : 0.f;
                    a5 += in ? t5 : 0.f;
                    a6 += in ? q.x : 0.f;
                    a7 += in ? q.y : 0.f;
                    a8 += in ? q.z : 0.f;
                    m += in ? 1 : 0;
                }
                if ((c + 1) * kFitCh >= n) busy = false;
                // seeds are a prefix of the z-sorted patch: once the last point of a step fails, the rest fail
                if (iter == 0 && busy && !((double)my[3 * (kFitCh - 1) + 2] < seed_thr)) busy = false;
            }
            __syncthreads();
            if (!__any(busy)) break;
        }
        fit_update(F, P.czm, a0, a1, a2, a3, a4, a5, a6, a7, a8, m);
    }
    if (!live) return;

    fit_finish(P, A, s, p, n, zone, ring, concentric_idx, F);
}

// Patches of 512 points or more (class kClassFitCoop): a lane per patch leaves the chip almost empty (a K64 scan has ~40 such
// patches holding 80 % of its points) and runs each of them as one dependent chain thousands of points long.  Here
// 16 lanes share a patch: each step they test 16 points and form the 9 products in parallel, pass them through LDS
// transposed, and lanes 0..8 of the group add "their" accumulator over the 16 points IN ORDER -- the sums are the
// same sequential fp32 sums, only the nine independent chains run on nine lanes instead of one.
// GL lanes share a patch, 64 / GL patches per wave.  GL = 16 for sequence shards (throughput: four patches keep the
// nine adding lanes of each busy); GL = 64 for a handful of scans (latency: the parallel part of the largest patch takes
// a quarter of the steps, only its sequential adds remain a chain).
#ifndef SCVOD_COOP_WAVES
#define SCVOD_COOP_WAVES 4
#endif
#ifndef SCVOD_COOP_PF
#define SCVOD_COOP_PF 4
#endif
// LEAN: the arrangement behind the fit stages the kept points' index triples for the lean emission (arrange_group).
template <int GL, bool LEAN>
__global__ __launch_bounds__(64, GL == 16 ? SCVOD_COOP_WAVES : 1) void k_pw_fit_coop(DevParams P, Arena A, int coop_class) {
    constexpr int NG = 64 / GL;
    constexpr int ROW = GL + 4;             // floats per product row: padded so the nine row reads spread over the banks
    constexpr int PF = (GL == 16) ? SCVOD_COOP_PF : 2;  // steps in flight per lane (128 points of the patch either way)
    constexpr unsigned long long FULL = (GL == 64) ? ~0ull : ((1ull << (GL & 63)) - 1ull);
    __shared__ fitq tile[NG * 9 * ROW / 4];  // [group][accumulator][GL points]
    const int lane = threadIdx.x, g = lane / GL, r = lane % GL, gbase = g * GL;
    auto group_bits = [&](unsigned long long ballot) -> unsigned long long { return (ballot >> gbase) & FULL; };
    int lo, hi;
    order_range(A.order_off, coop_class, 63, lo, hi);
    if (lo + (int)blockIdx.x * NG >= hi) return;
    const int w = lo + blockIdx.x * NG + g;
    const bool live = w < hi;
    const int4 item = live ? A.order[w] : make_int4(0, 0, 0, 0);
    const int code = item.x;
    const int s = code / kMaxPatches, p = code - s * kMaxPatches;
    const int n = live ? item.y : 0;
    const Xyz* __restrict__ sp = A.sorted_xyz + (size_t)item.z + item.w;
    int n_max = n;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) n_max = max(n_max, __shfl_xor(n_max, d));
    const int n_blocks = (n_max + GL * PF - 1) / (GL * PF);

    int zone = 0;
    while (zone < 3 && p >= P.czm.patch_base[zone + 1]) ++zone;
    const int ring = (p - P.czm.patch_base[zone]) / P.czm.num_sectors[zone];
    int concentric_idx = ring;
    for (int k = 0; k < zone; ++k) concentric_idx += P.czm.num_rings[k];

    // ---- extract_initial_seeds_ (patchwork.h:235-268) ----
    int init_idx = 0;
    {
        bool searching = live && (zone == 0);
        for (int c = 0; __any(searching); ++c) {
            if (searching) {
                const int j = c * GL + r;
                const bool low = (j < n) && ((double)sp[j].z < P.czm.seed_margin_z);
                const unsigned long long mg = group_bits(__ballot(low));
                if (mg != FULL) {
                    init_idx = c * GL + __builtin_ctzll(~mg);
                    searching = false;
                }
            }
        }
    }
    double sum = 0;
    int cnt = 0;
    for (int i0 = 0; i0 < P.czm.num_lpr; i0 += GL) {
        const int j = init_idx + i0 + r;
        const float zc = (j < n) ? sp[j].z : 0.f;
        const int kmax = min(GL, P.czm.num_lpr - i0);
        for (int k = 0; k < kmax; ++k) {
            const float z = __shfl(zc, gbase + k);
            if (init_idx + i0 + k < n) {
                sum += (double)z;
                ++cnt;
            }
        }
    }
    const double lpr = cnt != 0 ? sum / cnt : 0.0;
    const double seed_thr = lpr + P.czm.th_seeds;

    FitState F;
    fit_state_init(F);
    const int n_last = max(n - 1, 0);
    float* tf = (float*)tile;
    const int acc_row = (g * 9 + (r < 9 ? r : 8)) * (ROW / 4);  // lanes 9.. shadow accumulator 8

    // one pass over the patch; FIRST = the seed pass (members: a z prefix, tested in fp64), otherwise the plane test of the previous fit.
    // Two instantiations instead of a test per step: the step is ~90 instructions, a dozen of them were this distinction.
    auto fit_pass = [&](auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const float n0 = F.n0, n1 = F.n1, n2 = F.n2, thd = F.thd;
        float acc = 0.f;
        int m_lane = 0;
        bool busy = n > 0;
        Xyz cur[PF], nxt[PF];
#pragma unroll
        for (int k = 0; k < PF; ++k) cur[k] = sp[min(k * GL + r, n_last)];
        for (int b = 0; b < n_blocks; ++b) {
            const int j0 = b * GL * PF;
            // unconditional (clamped) loads: a load under a branch would have to land before the branch joins, which
            // serialises the whole block behind one memory latency
#pragma unroll
            for (int k = 0; k < PF; ++k) nxt[k] = sp[min(j0 + (PF + k) * GL + r, n_last)];
#pragma unroll
            for (int k = 0; k < PF; ++k) {
                const Xyz q = cur[k];
                const int j = j0 + k * GL + r;
                bool in = busy && (j < n);
                bool fails = false;
                if constexpr (FIRST) {
                    fails = in && !((double)q.z < seed_thr);
                    in = in && !fails;
                } else {
                    in = in && (plane_res(q, n0, n1, n2) < thd);
                }
                // non-members contribute +0.0f to every sum: zero the point, the products follow (0 * 0 = +0)
                const float zx = in ? q.x : 0.f, zy = in ? q.y : 0.f, zz = in ? q.z : 0.f;
                float* col = tf + g * 9 * ROW + r;
                col[0 * ROW] = zx * zx;
                col[1 * ROW] = zx * zy;
                col[2 * ROW] = zx * zz;
                col[3 * ROW] = zy * zy;
                col[4 * ROW] = zy * zz;
                col[5 * ROW] = zz * zz;
                col[6 * ROW] = zx;
                col[7 * ROW] = zy;
                col[8 * ROW] = zz;
                m_lane += in ? 1 : 0;
                // seeds are a prefix of the z-sorted patch: the group stops after the step in which one fails
                const bool stop = FIRST && (group_bits(__ballot(fails)) != 0ull);
                // the LDS unit executes one wave's instructions in order, so the rows written above are what the reads
                // below see; only the compiler has to be kept from reordering them
                __builtin_amdgcn_wave_barrier();
                // adding +0.0f for non-members is exact: the accumulators can never be -0.0f
#pragma unroll
                for (int q4 = 0; q4 < GL / 4; ++q4) {
                    const fitq v = tile[acc_row + q4];
                    acc += v.x;
                    acc += v.y;
                    acc += v.z;
                    acc += v.w;
                }
                __builtin_amdgcn_wave_barrier();
                if (stop || j0 + (k + 1) * GL >= n) busy = false;
            }
#pragma unroll
            for (int k = 0; k < PF; ++k) cur[k] = nxt[k];
            if (!__any(busy)) break;
        }
        int m = m_lane;  // members seen by this lane -> members of the group's patch
#pragma unroll
        for (int d = GL / 2; d > 0; d >>= 1) m += __shfl_xor(m, d);
        const float a0 = __shfl(acc, gbase + 0), a1 = __shfl(acc, gbase + 1), a2 = __shfl(acc, gbase + 2),
                    a3 = __shfl(acc, gbase + 3), a4 = __shfl(acc, gbase + 4), a5 = __shfl(acc, gbase + 5),
                    a6 = __shfl(acc, gbase + 6), a7 = __shfl(acc, gbase + 7), a8 = __shfl(acc, gbase + 8);
        fit_update(F, P.czm, a0, a1, a2, a3, a4, a5, a6, a7, a8, m);
    };
    for (int iter = 0; iter < P.czm.num_iter; ++iter) {
        if (iter == 0)
            fit_pass(std::true_type{});
        else
            fit_pass(std::false_type{});
    }
    if (live && r == 0) fit_finish(P, A, s, p, n, zone, ring, concentric_idx, F);
    // the arrangement by the lanes that fitted the patch (round 5; was k_pw_arrange, a pass of its own over every patch)
    const int status = fit_status(P, zone, ring, concentric_idx, F);
    arrange_group<GL, LEAN>(P, A, sp, A.sorted_idx + (size_t)item.z + item.w, A.seg + (size_t)item.z + item.w, A.zkey + (size_t)item.z + item.w, n, n_max, code, live, r, gbase, F.n0, F.n1, F.n2,
                      F.thd, status);
}


// one wave per (scan, patch): final plane test of every point (patchwork.h:488-501), keeps the
// z order inside the ground part and the non-ground part, counts what k_emit_offsets needs.
// GL lanes per patch: 64 for patches of 64 points or more, 16 (four patches per wave) for the many smaller ones, whose
// cost is the per-patch latency chain, not the points.
// LEAN: as arrange_group<GL, true>, the staging words live in zkey (dead since k_pw_scatter, free until the max_name pass).
template <int GL, bool LEAN>
__global__ __launch_bounds__(256) void k_pw_arrange(DevParams P, Arena A, int c_lo, int c_hi) {
    constexpr int NG = 64 / GL;
    constexpr unsigned long long FULL = (GL == 64) ? ~0ull : ((1ull << (GL & 63)) - 1ull);
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g_ = lane / GL, r = lane % GL, gbase = g_ * GL;
    auto group_bits = [&](unsigned long long ballot) -> unsigned long long { return (ballot >> gbase) & FULL; };
    int lo, total;
    order_range(A.order_off, c_lo, c_hi, lo, total);
    if (lo >= total) return;
    const int stride = gridDim.x * 4 * NG;
    int wi = lo + (blockIdx.x * 4 + wave) * NG + g_;
    if (lo + (int)(blockIdx.x * 4 + wave) * NG >= total) return;
    // Half of the live patches hold fewer than 64 points: a wave would spend its time in the dependent chain
    // order[] -> plane -> points.  So the chain is software-pipelined ACROSS patches: the list item two patches ahead
    // and the plane + first points of the next patch are in flight while the current patch is arranged (all loads
    // unconditional with clamped indices, so none has to land before a branch joins).
    struct Head {
        float n0, n1, n2, thd;
        int status;
        Xyz q;
        uint32_t w;
    };
    auto load_item = [&](int k) -> int4 { return A.order[min(k, total - 1)]; };
    auto load_head = [&](const int4& it) -> Head {
        const int slot = it.x;  // scan * kMaxPatches + patch
        const size_t first = (size_t)it.z + it.w + min(r, it.y - 1);
        Head h;
        h.n0 = A.planes[slot].normal[0];
        h.n1 = A.planes[slot].normal[1];
        h.n2 = A.planes[slot].normal[2];
        h.status = A.planes[slot].status;
        h.thd = A.fit_thd[slot];
        h.q = A.sorted_xyz[first];
        h.w = A.sorted_idx[first];
        return h;
    };
    int4 item = load_item(wi), item1 = load_item(wi + stride);
    Head head = load_head(item);
    for (; __any(wi < total); wi += stride) {
        const int4 item2 = load_item(wi + 2 * stride);
        const Head head1 = load_head(item1);
        const bool live = wi < total;  // uniform inside a group
        const int code = item.x;
        const int s = code / kMaxPatches, p = code - s * kMaxPatches;
        const int n = live ? item.y : 0, base = item.z, off = item.w;
        const int n_last = max(n - 1, 0);
        const Xyz* __restrict__ sp = A.sorted_xyz + (size_t)base + off;
        const uint32_t* __restrict__ si = A.sorted_idx + (size_t)base + off;
        const float n0 = head.n0, n1 = head.n1, n2 = head.n2;
        const float thd = head.thd;
        const int status = head.status;
        const bool rejected = (status >= 2);
        int n_max = n;
        if (NG > 1) {
#pragma unroll
            for (int d = 32; d >= GL; d >>= 1) n_max = max(n_max, __shfl_xor(n_max, d));
        }
        // ONE pass: ground part grows from the front in z order, the non-ground part from the back
        // (element r of the non-ground part lives at seg[n - 1 - r]; k_emit reads it that way)
        int n_g = 0, n_ng = 0, a_g = 0, a_ng = 0;
        uint32_t* seg = A.seg + (size_t)base + off;
        uint32_t* stage = A.zkey + (size_t)base + off;
        // the next GL points are in flight while this step is classified (clamped, unconditional loads)
        Xyz q_next = head.q;
        uint32_t w_next = head.w;
        const unsigned long long below = (1ull << r) - 1ull;
        for (int j0 = 0; j0 < n_max; j0 += GL) {
            const int j = j0 + r;
            int g = 0, keep = 0;
            const Xyz q = q_next;
            uint32_t w = w_next;
            q_next = sp[min(j + GL, n_last)];
            w_next = si[min(j + GL, n_last)];
            if (j < n) {
                g = plane_res(q, n0, n1, n2) < thd;
                // range/FOV verdict of makeApriVec, only for points that reach the non-ground stream
                if (!g || rejected) {
                    keep = keep_of_point(P.bin, P.keep, q.x, q.y, q.z);
                    w |= keep ? 0x80000000u : 0u;
                }
            }
            const unsigned long long bg = group_bits(__ballot(g));
            const unsigned long long bn = group_bits(__ballot(!g && j < n));
            if (j < n) {
                if (g)
                    seg[n_g + __popcll(bg & below)] = w;
                else
                    seg[n - 1 - (n_ng + __popcll(bn & below))] = w;
                if constexpr (LEAN) {
                    if (keep) stage[g ? n_g + __popcll(bg & below) : n - 1 - (n_ng + __popcll(bn & below))] = triple_of_point(P, q.x, q.y, q.z);
                }
            }
            a_g += __popcll(group_bits(__ballot(g && keep)));
            a_ng += __popcll(group_bits(__ballot(!g && keep && j < n)));
            n_g += __popcll(bg);
            n_ng += __popcll(bn);
        }
        if (live && r == 0) {
            PatchRec rec;
            rec.n = n;
            rec.n_g = n_g;
            rec.status = status;
            rec.a_g = a_g;
            rec.a_ng = a_ng;
            A.patch_rec[s * kMaxPatches + p] = rec;
            A.planes[s * kMaxPatches + p].n_ground = n_g;
        }
        item = item1;
        item1 = item2;
        head = head1;
    }
}

// ------------------------------------------------------------------------------------------
// Emission: per-scan exclusive scans over patches (reference emission order = patch order),
// then one wave per patch writes cloud_out / cloud_nonground indices, apri_vec (ordered
// compaction of the non-ground stream by the range/FOV verdict) and the rejected list.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_emit_offsets(DevParams P, Arena A) {
    __shared__ int wsum[17];
    const int s = blockIdx.x;
    const int t = threadIdx.x;
    int eg = 0, eng = 0, ea = 0, er = 0;
    if (t < P.n_patches) {
        PatchRec r = A.patch_rec[s * kMaxPatches + t];
        if (r.status == 1) {
            eg = r.n_g;
            eng = r.n - r.n_g;
            ea = r.a_ng;
        } else if (r.status >= 2) {
            eng = r.n;
            ea = r.a_g + r.a_ng;
        }
        er = eng - ea;
    }
    int tg, tng, ta, tr;
    int xg = block_excl_scan<1024>(eg, tg, wsum);
    int xng = block_excl_scan<1024>(eng, tng, wsum);
    int xa = block_excl_scan<1024>(ea, ta, wsum);
    int xr = block_excl_scan<1024>(er, tr, wsum);
    if (t < P.n_patches) {
        int* o = A.emit_off + ((size_t)s * kMaxPatches + t) * 4;
        o[0] = xg;
        o[1] = xng;
        o[2] = xa;
        o[3] = xr;
    }
    if (t == 0) {
        int n = A.scan_off[s + 1] - A.scan_off[s];
        int* c = A.counts + s * 8;
        c[0] = n;
        c[1] = tg;
        c[2] = tng;
        c[3] = n - tg - tng;
        c[4] = ta;
        c[5] = tr;
        c[6] = 0;
        c[7] = P.n_patches;
        A.scan_irr[s] = 0;
        A.irr_list[(size_t)s * (kIrrListCap + 1)] = 0;  // (k_emit lists the points whose index triple leaves the grid: the max_name pass reads them)
    }
}

// Two forms.  The eager one (LEAN = false) gathers every kept point from the input cloud: index triple, voxel key and the compact
// intensity come from its coordinates, and it writes the three index lists (ground_idx, nonground_idx, rejected_src).  The lean one
// is a pure compaction: the arrange pass staged the packed triple next to the seg word (zkey), the key is recomputed from it (exact
// while the grid fits the packing: idx3_roundtrip_ok, decided on the host), apri_int stays unwritten until somebody asks
// (k_apri_intensity), and so do the three lists (k_emit_lists): no kernel of the batch chain reads them.  It never touches the
// ground part of a kept patch.
constexpr int kEmitThreads = 256;
template <bool LEAN>
__global__ __launch_bounds__(kEmitThreads) void k_emit(DevParams P, Arena A) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int total = A.order_off[64];
    if ((int)(blockIdx.x * 4 + wave) >= total) return;
    // the dependent chain list item -> patch record / output offsets -> seg words is software-pipelined ACROSS patches (most
    // hold a few hundred points): the item two patches ahead and the record + offsets of the next patch are in flight while
    // the current patch is emitted (clamped, unconditional loads)
    const int stride = gridDim.x * 4;
    struct Meta {
        PatchRec r;
        int4 o;
    };
    auto load_item = [&](int k) -> int4 { return A.order[min(k, total - 1)]; };
    auto load_meta = [&](const int4& it) -> Meta {
        Meta m;
        m.r = A.patch_rec[it.x];  // it.x = scan * kMaxPatches + patch
        m.o = *reinterpret_cast<const int4*>(A.emit_off + (size_t)it.x * 4);
        return m;
    };
    int w = blockIdx.x * 4 + wave;
    int4 item = load_item(w), item1 = load_item(w + stride);
    Meta meta = load_meta(item);
    for (; w < total; w += stride) {
        const int4 item2 = load_item(w + 2 * stride);
        const Meta meta1 = load_meta(item1);
        const int code = item.x;
        const int s = code / kMaxPatches, p = code - s * kMaxPatches;
        const PatchRec r = meta.r;
        const int base = item.z, off = item.w;
        const int xg = meta.o.x, xng = meta.o.y, xa = meta.o.z, xr = meta.o.w;
        const bool kept = (r.status == 1);
        const uint32_t* seg = A.seg + (size_t)base + off;
        const uint32_t* stage = A.zkey + (size_t)base + off;
        // ground part of a kept patch -> cloud_out
        if constexpr (!LEAN) {
            if (kept) {
                for (int e = lane; e < r.n_g; e += 64) {
                    const uint32_t id = seg[e] & 0x7fffffffu;
                    A.ground_idx[(size_t)base + xg + e] = (int32_t)id;
                }
            }
        }
        // non-ground stream of this patch: for a rejected patch the ground part (front, ascending) followed
        // by the non-ground part; the latter is stored back to front by k_pw_arrange
        const int e0 = kept ? r.n_g : 0;
        if constexpr (LEAN) {
            if (e0 >= r.n) {  // a kept patch that is all ground: nothing to compact
                item = item1;
                item1 = item2;
                meta = meta1;
                continue;
            }
        }
        int run_keep = 0;
        auto seg_pos = [&](int e) -> int {  // clamped position of stream element e in the patch (callers test e < r.n)
            const int k = (e < r.n_g) ? e : r.n - 1 - (e - r.n_g);
            return min(max(k, 0), r.n - 1);
        };
        auto seg_at = [&](int e) -> uint32_t { return seg[seg_pos(e)]; };  // clamped, unconditional load
        // eager form: two steps of seg words and one step of point gathers are in flight while a step is emitted; lanes that
        // keep nothing gather the scan's first point (one shared line) so the load needs no branch.
        // lean form: two steps of seg words and of staged triples (a word of a point that was not kept holds anything: never used)
        auto gather = [&](uint32_t v, int e) -> float4 {
            if constexpr (LEAN) {
                return make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                const bool k = (e < r.n) && (v >> 31);
                return A.pts[base + (k ? (v & 0x7fffffffu) : 0u)];
            }
        };
        auto stage_at = [&](int e) -> uint32_t {
            if constexpr (LEAN)
                return stage[seg_pos(e)];
            else
                return 0u;
        };
        uint32_t v0 = seg_at(e0 + lane), v1 = seg_at(e0 + 64 + lane);
        uint32_t t0 = stage_at(e0 + lane), t1 = stage_at(e0 + 64 + lane);
        float4 q0 = gather(v0, e0 + lane);
        for (int c0 = e0; c0 < r.n; c0 += 64) {
            const int e = c0 + lane;
            const uint32_t v = v0;
            const uint32_t t = t0;
            const float4 q = q0;
            const uint32_t v2 = seg_at(e + 128);
            const uint32_t t2 = stage_at(e + 128);
            q0 = gather(v1, e + 64);
            v0 = v1;
            v1 = v2;
            t0 = t1;
            t1 = t2;
            const int keep = (e < r.n) ? (int)(v >> 31) : 0;
            const unsigned long long bk = __ballot(keep);
            const int ek = __popcll(bk & ((1ull << lane) - 1ull));
            const int nk = __popcll(bk);
            const size_t dst0 = (size_t)base + xa + run_keep;  // first PointAPRI slot of this step
            if (e < r.n) {
                const uint32_t id = v & 0x7fffffffu;
                const int spos = e - e0;  // position in the non-ground stream of this patch
                if constexpr (!LEAN) A.nonground_idx[(size_t)base + xng + spos] = (int32_t)id;
                if (keep) {
                    // apri_vec is kept in its compact form (source index, voxel key, intensity, index triple); the 44-byte
                    // PointAPRI records are expanded from it on request (k_apri_expand).  Only the indices are needed here: the
                    // guarded estimate decides them away from the bin edges, the reference arithmetic next to one
                    int32_t ri, si, ai;
                    if constexpr (LEAN) {
                        unpack_idx3((int32_t)t, &ri, &si, &ai);  // (exactly the point's indices: the host checked that the grid fits the packing)
                    } else if (!idx3_fast(P.bin, P.binfast, q.x, q.y, q.z, &ri, &si, &ai)) {
                        Apri a;
                        apri_of_point(P.bin, q.x, q.y, q.z, q.w, a);
                        ri = a.range_idx;
                        si = a.sector_idx;
                        ai = a.azimuth_idx;
                    }
                    A.apri_src[dst0 + ek] = (int32_t)id;
                    A.apri_key[dst0 + ek] = ai * P.bin.range_num * P.bin.sector_num + ri * P.bin.sector_num + si;
                    if constexpr (LEAN) {
                        A.apri_idx3[dst0 + ek] = (int32_t)t;
                    } else {
                        A.apri_int[dst0 + ek] = q.w;
                        A.apri_idx3[dst0 + ek] = pack_idx3(ri, si, ai);
                    }
                    if ((unsigned)ri >= (unsigned)P.bin.range_num || (unsigned)si >= (unsigned)P.bin.sector_num || (unsigned)ai >= (unsigned)P.bin.azimuth_num)
{
                        A.scan_irr[s] = 1;  // (rare: a -1 bin; every writer stores the same value)
                        int32_t* il = A.irr_list + (size_t)s * (kIrrListCap + 1);
                        const int x = atomicAdd(&il[0], 1);
                        if (x < kIrrListCap) il[1 + x] = (int32_t)(xa + run_keep + ek);
                    }
                } else if constexpr (!LEAN) {
                    A.rejected_src[(size_t)base + xr + (spos - (run_keep + ek))] = (int32_t)id;
                }
            }
            run_keep += nk;
        }
        item = item1;
        item1 = item2;
        meta = meta1;
    }
}

// the three index lists a lean emission left out, for the whole batch, on request (ensure_lists): k_emit's walk -- one wave per
// item of A.order -- over patch_rec, emit_off and seg only, and exactly the words k_emit<false> writes, at the same positions.
// Neither the staged triples nor the input cloud are read: later stages reuse zkey, keys, sorted_xyz and sorted_idx.
__global__ __launch_bounds__(kEmitThreads) void k_emit_lists(Arena A) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int total = A.order_off[64];
    if ((int)(blockIdx.x * 4 + wave) >= total) return;
    const int stride = gridDim.x * 4;
    struct Meta {
        PatchRec r;
        int4 o;
    };
    auto load_item = [&](int k) -> int4 { return A.order[min(k, total - 1)]; };
    auto load_meta = [&](const int4& it) -> Meta {
        Meta m;
        m.r = A.patch_rec[it.x];
        m.o = *reinterpret_cast<const int4*>(A.emit_off + (size_t)it.x * 4);
        return m;
    };
    int w = blockIdx.x * 4 + wave;
    int4 item = load_item(w), item1 = load_item(w + stride);
    Meta meta = load_meta(item);
    for (; w < total; w += stride) {  // (the same pipeline across patches as k_emit: item two ahead, record + offsets one ahead)
        const int4 item2 = load_item(w + 2 * stride);
        const Meta meta1 = load_meta(item1);
        const PatchRec r = meta.r;
        const int base = item.z, off = item.w;
        const int xg = meta.o.x, xng = meta.o.y, xr = meta.o.w;
        const bool kept = (r.status == 1);
        const uint32_t* seg = A.seg + (size_t)base + off;
        if (kept) {
            for (int e = lane; e < r.n_g; e += 64) A.ground_idx[(size_t)base + xg + e] = (int32_t)(seg[e] & 0x7fffffffu);
        }
        const int e0 = kept ? r.n_g : 0;
        auto seg_at = [&](int e) -> uint32_t {  // stream element e of the patch, clamped (callers test e < r.n)
            const int k = (e < r.n_g) ? e : r.n - 1 - (e - r.n_g);
            return seg[min(max(k, 0), r.n - 1)];
        };
        int run_keep = 0;
        uint32_t v0 = seg_at(e0 + lane);
        for (int c0 = e0; c0 < r.n; c0 += 64) {
            const int e = c0 + lane;
            const uint32_t v = v0;
            v0 = seg_at(e + 64);
            const int keep = (e < r.n) ? (int)(v >> 31) : 0;
            const unsigned long long bk = __ballot(keep);
            const int ek = __popcll(bk & ((1ull << lane) - 1ull));
            if (e < r.n) {
                const int32_t id = (int32_t)(v & 0x7fffffffu);
                const int spos = e - e0;
                A.nonground_idx[(size_t)base + xng + spos] = id;
                if (!keep) A.rejected_src[(size_t)base + xr + (spos - (run_keep + ek))] = id;
            }
            run_keep += __popcll(bk);
        }
        item = item1;
        item1 = item2;
        meta = meta1;
    }
}

// the compact intensities a lean emission left out, on request (ensure_intensities): apri_int[i] = intensity of apri point i's input
// point.  Streams apri_src, gathers 4 of the point's 16 bytes.  grid = (blocks along a scan, B).
__global__ __launch_bounds__(256) void k_apri_intensity(Arena A) {
    const int s = blockIdx.y;
    const size_t base = (size_t)A.scan_off[s];
    const int n = A.counts[s * 8 + 4];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) A.apri_int[base + i] = A.pts[base + A.apri_src[base + i]].w;
}
