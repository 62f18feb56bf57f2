// scvod_k_voxels.inc -- PointAPRI expansion, direct binning, the voxel stage: buckets, LDS sort, per-voxel descriptors (A4-A5).
// Part of the kernels translation unit: included by scvod_kernels.hip (inside namespace scvod), never compiled on its own.
// PointAPRI records (ssc.cpp:176-193) of scans [s0, s0 + gridDim.y), rebuilt from the compact apri_vec: the same spec
// function on the same point gives the same bits k_emit saw when it derived key and intensity.
__global__ __launch_bounds__(256) void k_apri_expand(DevParams P, Arena A, int s0) {
    const int s = s0 + blockIdx.y;
    const int base = A.scan_off[s];
    const int n = A.counts[s * 8 + 4];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float4 q = A.pts[base + A.apri_src[(size_t)base + i]];
        Apri a;
        apri_of_point(P.bin, q.x, q.y, q.z, q.w, a);
        scvod_apri out;
        out.x = a.x;
        out.y = a.y;
        out.z = a.z;
        out.range = a.range;
        out.angle = a.angle;
        out.azimuth = a.azimuth;
        out.intensity = a.intensity;
        out.range_idx = a.range_idx;
        out.sector_idx = a.sector_idx;
        out.azimuth_idx = a.azimuth_idx;
        out.voxel_idx = a.voxel_idx;
        A.apri[(size_t)base + i] = out;
    }
}

// Per-point class array of ONE scan, built on request from the two index lists (the reference holds the two clouds,
// never a class array; materialising it for every scan of a batch cost 0.9 ms per sequence in byte scatters).
__global__ __launch_bounds__(256) void k_cls_from_lists(Arena A, int s) {
    const int base = A.scan_off[s];
    const int n_g = A.counts[s * 8 + 1], n_ng = A.counts[s * 8 + 2];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_g + n_ng; i += gridDim.x * 256) {
        if (i < n_g)
            A.cls[base + A.ground_idx[(size_t)base + i]] = SCVOD_CLS_GROUND;
        else
            A.cls[base + A.nonground_idx[(size_t)base + (i - n_g)]] = SCVOD_CLS_NONGROUND;
    }
}

// makeApriVec on an arbitrary cloud in input order (no Patchwork): one workgroup per scan walks
// the scan in chunks, ordered compaction by block scan.  apply_filter == 0 keeps every point.
__global__ __launch_bounds__(1024) void k_bin_direct(DevParams P, Arena A, int apply_filter) {
    __shared__ int wsum[17];
    const int s = blockIdx.x;
    const int base = A.scan_off[s];
    const int n = A.scan_off[s + 1] - base;
    int run = 0;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        int i = c0 + threadIdx.x;
        int keep = 0;
        Apri a;
        if (i < n) {
            float4 q = A.pts[base + i];
            keep = apri_of_point(P.bin, q.x, q.y, q.z, q.w, a);
            if (!apply_filter) keep = 1;
        }
        int tk;
        int ek = block_excl_scan<1024>(keep, tk, wsum);
        if (i < n) {
            if (keep) {
                size_t dst = (size_t)base + run + ek;
                scvod_apri out;
                out.x = a.x;
                out.y = a.y;
                out.z = a.z;
                out.range = a.range;
                out.angle = a.angle;
                out.azimuth = a.azimuth;
                out.intensity = a.intensity;
                out.range_idx = a.range_idx;
                out.sector_idx = a.sector_idx;
                out.azimuth_idx = a.azimuth_idx;
                out.voxel_idx = a.voxel_idx;
                A.apri[dst] = out;
                A.apri_src[dst] = i;
                A.apri_key[dst] = a.voxel_idx;
                A.apri_int[dst] = a.intensity;
                A.apri_idx3[dst] = pack_idx3(a.range_idx, a.sector_idx, a.azimuth_idx);
            } else {
                A.rejected_src[(size_t)base + (i - (run + ek))] = i;
            }
        }
        run += tk;
    }
    if (threadIdx.x == 0) {
        A.scan_irr[s] = 0;  // (order hint only: k_cc_scan decides regularity itself)
        A.irr_list[(size_t)s * (kIrrListCap + 1)] = -1;  // (not listed here: the max_name pass looks through the points itself)
        int* c = A.counts + s * 8;
        c[0] = n;
        c[1] = 0;
        c[2] = 0;
        c[3] = 0;
        c[4] = run;
        c[5] = n - run;
        c[6] = 0;
        c[7] = 0;
    }
}

// apri_vec supplied by the caller (scvod_voxelize): derive the compact key / intensity arrays
__global__ __launch_bounds__(256) void k_apri_split(Arena A) {
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int n = A.counts[s * 8 + 4];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const scvod_apri& a = A.apri[(size_t)base + i];
        A.apri_key[(size_t)base + i] = a.voxel_idx;
        A.apri_int[(size_t)base + i] = a.intensity;
        A.apri_idx3[(size_t)base + i] = pack_idx3(a.range_idx, a.sector_idx, a.azimuth_idx);
    }
}

// ------------------------------------------------------------------------------------------
// Voxel stage (SSC::makeHashCloud): bucket by the high bits of the key, sort (key, apri idx)
// inside each bucket, per-voxel sequential intensity mean / variance.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int vx_bucket_of(const DevParams& P, const Arena& A, int s, int32_t voxel_idx) {
    if (A.vb_lut) {  // VoxelGrid run: population-balanced monotone table (cell indices are far from uniform)
        if (voxel_idx == 0x7fffffff) return kMaxBuckets - 1;
        return A.vb_lut[(size_t)s * kVgLutBins + (voxel_idx >> *A.vb_lut_shift)];
    }
    int64_t b = ((int64_t)voxel_idx + P.key_off) >> P.vb_shift;
    if (b < 0) b = 0;
    if (b > P.n_buckets - 1) b = P.n_buckets - 1;
    return (int)b;
}
__device__ __forceinline__ uint32_t vx_bias(int32_t k) { return (uint32_t)k ^ 0x80000000u; }
__device__ __forceinline__ int32_t vx_unbias(uint32_t u) { return (int32_t)(u ^ 0x80000000u); }

// count + offsets + scatter of a scan's voxel keys in ONE kernel (round 5): one workgroup per scan takes its keys twice -- the
// second time out of L2 (a 64-beam scan holds 44 k of them: 174 KB) -- with the bucket histogram, its prefix and the scatter
// cursors in LDS.  Position inside a bucket is arbitrary (the bucket kernels sort).  grid = B, block = 1024.
__global__ __launch_bounds__(1024) void k_vx_partition(DevParams P, Arena A) {
    __shared__ int hist[kMaxBuckets];
    __shared__ int wsum[17];
    const int s = blockIdx.x;
    const int base = A.scan_off[s];
    const int n = A.counts[s * 8 + 4];
    const int tid = threadIdx.x;
    if (tid < kMaxBuckets) hist[tid] = 0;
    __syncthreads();
    constexpr int U = 4;  // keys in flight per thread: the loop is a chain of memory round trips otherwise
    for (int i0 = 0; i0 < n; i0 += 1024 * U) {
        int32_t key[U];
#pragma unroll
        for (int u = 0; u < U; ++u) key[u] = A.apri_key[(size_t)base + min(i0 + u * 1024 + tid, n - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u) wave_bin_add(hist, i0 + u * 1024 + tid < n ? vx_bucket_of(P, A, s, key[u]) : -1);
    }
    __syncthreads();
    const int c = (tid < P.n_buckets) ? hist[tid] : 0;
    int total;
    const int ex = block_excl_scan<1024>(c, total, wsum);
    if (tid < kMaxBuckets) {
        A.vb_count[s * kMaxBuckets + tid] = c;
        hist[tid] = ex;  // (from here on: the bucket's cursor)
    }
    if (tid <= P.n_buckets) A.vb_off[s * (kMaxBuckets + 1) + tid] = ex;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 1024 * U) {
        int32_t key[U];
#pragma unroll
        for (int u = 0; u < U; ++u) key[u] = A.apri_key[(size_t)base + min(i0 + u * 1024 + tid, n - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 1024 + tid;
            const int bk = i < n ? vx_bucket_of(P, A, s, key[u]) : -1;
            const int at = wave_bin_rank(hist, bk);  // (one LDS atomic per lane instead: 0.67 vs 0.52 ms on 64-beam scans, 0.73 vs 0.88 on 128-beam ones)
            if (bk >= 0) {
                if (A.vx_k32)  // key relative to its bucket's first key | apri index: fits 32 bits (see vx_k32 in scvod_kernels.h)
                    ((uint32_t*)A.vkeys)[(size_t)base + at] = (uint32_t)((((int64_t)key[u] + P.key_off) & ((1ll << P.vb_shift) - 1)) << A.vx_idx_bits) | (uint32_t)i;
                else
                    A.vkeys[(size_t)base + at] = pack_key(vx_bias(key[u]), (uint32_t)i);
            }
        }
    }
}

// MODE 0: SSC::makeHashCloud (intensity mean / variance per voxel).  MODE 1: pcl::VoxelGrid run (keys = cell indices):
// per cell the CentroidPoint sums of its points in ascending input index, straight from the sorted keys in LDS; no
// point lists, no intensity statistics; the bucket of the dropped points is skipped.
// KT = unsigned long long: (biased voxel key, apri index) under the double-encoded exponent (any key, VoxelGrid cells).
// KT = uint32_t: hot path of a filtered batch -- (key - first key of the bucket) << idx_bits | apri index; a bucket spans
// 2^vb_shift keys and a scan 2^idx_bits points, vb_shift + idx_bits <= 32 (checked on the host): half the LDS traffic, and
// the compare-exchange is a full-rate v_min_u32 + v_max_u32.
// LDS of one workgroup: padded keys + voxel starts + staged intensities (+ the scan's wave sums).  SCVOD_VOX_K32_LDS = 1: the key
// area of the 4-byte keys is 4 bytes per slot, which lets a third (sixth, twelfth) workgroup of the 4096 (2048, 1024) tier onto a CU
#ifndef SCVOD_VOX_K32_LDS
#define SCVOD_VOX_K32_LDS 1
#endif
constexpr size_t vox_key_bytes(int cap, size_t ksize) { return (((size_t)(cap + cap / 8) * (SCVOD_VOX_K32_LDS ? ksize : 8)) + 15) & ~(size_t)15; }
// DESC = false (the lean form): no staged intensities; what is left of that area holds the <= 128 (chunk, wave) head counts
constexpr size_t vox_aux_bytes(int cap, bool desc) { return desc ? (size_t)cap * 4 : ((size_t)(cap / 64) * 4 + 15) & ~(size_t)15; }
constexpr size_t vox_lds_bytes(int cap, size_t ksize = 8, bool desc = true) {
    return vox_key_bytes(cap, ksize) + (size_t)cap * 4 + vox_aux_bytes(cap, desc) + 128;
}
// workgroups per CU of the lean 4096 tier with 32-bit keys (x2 for the 2048 tier): 35.2 KB of LDS each, four fit where the full form's
// 51.3 KB allows three (profiles/lazy_voxel_descriptors_cost.md has both measured)
#ifndef SCVOD_VOX_LEAN_MORE
#define SCVOD_VOX_LEAN_MORE 4
#endif
#ifndef SCVOD_VOX_LEAN_S
#define SCVOD_VOX_LEAN_S 12  // workgroups per CU of the lean 1024 tier (8.9 KB of LDS each; the fused form runs eight)
#endif
// The intensity descriptor of one voxel (SSC::makeHashCloud's intensity_av / intensity_cov): fp32 running sum in list order, divided by
// float(count); population variance accumulated as float += double.  ONE routine for the fused form (k_vx_bucket<..., DESC = true>)
// and the on-demand kernel (k_vx_descriptors), so their bits cannot drift apart.  at(j): intensity of the voxel's j-th point;
// U values are fetched together before they are added in order (U > 1 where at() is a chain of global loads).
template <int U, typename F>
__device__ __forceinline__ void vx_descriptor(int n, F&& at, float& av_out, float& cov_out) {
    float av = 0.f;
    for (int j0 = 0; j0 < n; j0 += U) {
        float x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = (j0 + u < n) ? at(j0 + u) : 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (j0 + u < n) av += x[u];
    }
    const float fn = (float)n;
    av = av / fn;
    float cov = 0.f;
    for (int j0 = 0; j0 < n; j0 += U) {
        float x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = (j0 + u < n) ? at(j0 + u) : 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (j0 + u < n) {
                const double d = (double)(x[u] - av);
                cov = (float)((double)cov + d * d);
            }
    }
    av_out = av;
    cov_out = cov / fn;
}
// which tiers run the pad-free network (scvod_sortnet.h): those measured faster with it (profiles/padfree_sort_cost.md);
// the 256 and 1024 tiers are slower, they keep the padded network.  SCVOD_VOX_PADFREE=0: none, 2: all
constexpr bool vx_bucket_padfree(int cap) { return SCVOD_VOX_PADFREE == 2 || (SCVOD_VOX_PADFREE == 1 && cap >= 2048); }
// DESC = false (MODE 0 only): the lean form of a batch whose descriptors are computed on demand (k_vx_descriptors) -- no intensity
// staging, no per-voxel sums, no tmp_vox_av / tmp_vox_cov
template <int CAP, int THREADS, int C_LO, int C_HI, int LGE, int MODE = 0, typename KT = unsigned long long, bool DESC = true>
__global__ __launch_bounds__(THREADS)
#if SCVOD_VOX_K32_LDS
__attribute__((amdgpu_waves_per_eu((sizeof(KT) == 4 && CAP <= 4096 && CAP >= 2048) ? (DESC ? 6 : 2 * SCVOD_VOX_LEAN_MORE) : 1, 8)))
#endif
void k_vx_bucket(DevParams P, Arena A) {
    static_assert(DESC || MODE == 0, "the lean form is makeHashCloud's");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool K32 = sizeof(KT) == 4;
    constexpr bool PADFREE = vx_bucket_padfree(CAP);
    constexpr bool PADK = true;  // both key types: unpadded 4-byte keys let the compiler fuse neighbouring LDS accesses into
                                 // wide ones that fault on the network's unaligned groups (seen on the 8192-key tier)
    constexpr int SLOTS = CAP + CAP / 8;
    KT* l_keys = (KT*)smem;   // padded layout (8-byte keys)
    constexpr size_t KB = vox_key_bytes(CAP, sizeof(KT));
    static_assert(KB >= (size_t)SLOTS * sizeof(KT), "key area");
    int* l_vbeg = (int*)(smem + KB);                         // [CAP]
    float* l_int = (float*)(smem + KB + (size_t)CAP * 4);    // [CAP] intensity in sorted order (DESC), else the [CAP / 64] head counts only
    int* wsum = (int*)(smem + KB + (size_t)CAP * 4 + vox_aux_bytes(CAP, DESC));
    int lo, hi;
    order_range(A.vorder_off, C_LO, C_HI, lo, hi);
    constexpr bool PV = (CAP == 4096 && MODE == 0);  // (profiling build: the dominant tier is clocked)
    PROF_BEGIN();
    for (int w = lo + blockIdx.x; w < hi; w += gridDim.x) {
    if (PV) PROF_RESET();
    const int4 item = A.vorder[w];
    const int code = item.x;
    const int s = code / kMaxBuckets, b = code - s * kMaxBuckets;
    const int m = item.y;
    const int base = item.z, off = item.w;
    if (MODE == 1 && b == kMaxBuckets - 1) {  // dropped points (label filter): no cells
        if (threadIdx.x == 0) A.vb_nvox[s * kMaxBuckets + b] = 0;
        continue;
    }
    const bool in_lds = (m <= CAP);
    KT* keys;
    int* vbeg;
    float* ints;
    KT* gkeys = (KT*)A.vkeys + (size_t)base + off;
    const KT kpad = K32 ? (KT)0xffffffffu : (KT)kKeyPad;
    const uint32_t imask = (1u << A.vx_idx_bits) - 1u;
    auto k_major = [&](KT k) -> uint32_t { return K32 ? (uint32_t)k >> A.vx_idx_bits : key_major((unsigned long long)k); };
    auto k_idx = [&](KT k) -> uint32_t { return K32 ? (uint32_t)k & imask : key_idx((unsigned long long)k); };
    if (in_lds) {
        int np2 = 1 << LGE;
        while (np2 < m) np2 <<= 1;
        const int nlive = sortnet::live_end(m, LGE);  // the later phases read keys [0, m) only
        // a full tier: all of a thread's key loads in flight together (coalesced), sorted straight from the registers
        constexpr int IT = CAP / THREADS;
        keys = l_keys;
        vbeg = l_vbeg;
        ints = l_int;
        bool from_regs = false;
        if constexpr (IT == (1 << LGE) && CAP >= 4096) {  // (the small tiers are occupancy-bound: they keep their registers)
            if (np2 == CAP) {
                from_regs = true;
                KT tmp[IT];
                if constexpr (PADFREE) {  // the first nlive / IT threads hold the keys, coalesced among themselves
                    if ((int)threadIdx.x < (nlive >> LGE)) {
#pragma unroll
                        for (int it = 0; it < IT; ++it) {
                            const int j = sortnet::start_key(it, (int)threadIdx.x, nlive, LGE);
                            tmp[it] = (j < m) ? gkeys[j] : kpad;
                        }
                    }
                    if (PV) PROF_MARK(3, 0);
                    padfree_sort_regs<THREADS, PADK, LGE>(tmp, keys, np2, nlive, kpad);
                } else {
#pragma unroll
                    for (int it = 0; it < IT; ++it) {
                        const int j = it * THREADS + (int)threadIdx.x;
                        tmp[it] = (j < m) ? gkeys[j] : kpad;
                    }
                    if (PV) PROF_MARK(3, 0);
                    block_bitonic_sort_pow2_regs<THREADS, PADK, LGE>(tmp, keys);
                }
            }
        }
        if (!from_regs) {
            const int nfill = PADFREE ? nlive : np2;  // (pad-free: slots >= nlive are never touched)
            for (int j = threadIdx.x; j < nfill; j += THREADS) l_keys[sort_slot<PADK>(j)] = (j < m) ? gkeys[j] : kpad;
            __syncthreads();
            if (PV) PROF_MARK(3, 0);
            if constexpr (PADFREE)
                padfree_sort<THREADS, PADK, LGE>(keys, np2, nlive, kpad);
            else
                block_bitonic_sort_pow2<THREADS, PADK, LGE>(keys, np2);
        }
        if (PV) PROF_MARK(3, 1);
    } else {
        keys = gkeys;
        vbeg = A.tmp_vox_begin + (size_t)base + off;  // rewritten below with final values
        ints = nullptr;                               // (the per-voxel loops gather from apri_int themselves)
        block_bitonic_sort<THREADS, false>(keys, m);
    }
#define KX(j) (in_lds ? sort_slot<PADK>(j) : (j))
    // head flags + compaction of voxel starts; stage the intensities in sorted order
    int run = 0;
    if (in_lds) {
        // two barriers for the whole bucket instead of three per THREADS keys: heads counted per (chunk, wave) by ballot, ONE prefix
        // over those <= CAP / 64 counts (two per lane of the first wave), then every head knows its place.  The counts borrow the
        // intensity area, which is idle until the staging below (the lean form keeps just these counts of it).
        constexpr int NW = THREADS / 64;
        static_assert(CAP / 64 <= 128, "two (chunk, wave) counts per lane");
        int* wcnt = (int*)l_int;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int chunks = (m + THREADS - 1) / THREADS;
        auto head_of = [&](int j, KT& cur) -> bool {
            cur = keys[KX(j)];
            const KT prev = keys[KX(j > 0 ? j - 1 : 0)];  // (never form keys[-1]: with flat addressing that leaves the LDS aperture)
            return (j == 0) || (k_major(cur) != k_major(prev));
        };
        for (int c = 0; c < chunks; ++c) {
            const int j = c * THREADS + threadIdx.x;
            bool head = false;
            if (j < m) {
                KT cur;
                head = head_of(j, cur);
                if (MODE == 0) A.vox_pts[(size_t)base + off + j] = (int32_t)k_idx(cur);
            }
            const unsigned long long hb = __ballot(head);
            if (lane == 0) wcnt[c * NW + wave] = __popcll(hb);
        }
        __syncthreads();
        const int ne = chunks * NW;
        if (wave == 0) {
            const int a0 = (2 * lane < ne) ? wcnt[2 * lane] : 0, a1 = (2 * lane + 1 < ne) ? wcnt[2 * lane + 1] : 0;
            const int inc = wave_incl_scan(a0 + a1);
            if (2 * lane < ne) wcnt[2 * lane] = inc - a0 - a1;
            if (2 * lane + 1 < ne) wcnt[2 * lane + 1] = inc - a1;
            if (lane == 63) wsum[0] = inc;
        }
        __syncthreads();
        run = wsum[0];
        for (int c = 0; c < chunks; ++c) {
            const int j = c * THREADS + threadIdx.x;
            KT cur;
            const bool head = (j < m) && head_of(j, cur);
            const unsigned long long hb = __ballot(head);
            if (head) vbeg[wcnt[c * NW + wave] + __popcll(hb & ((1ull << lane) - 1ull))] = j;
        }
    }
    for (int c0 = 0; c0 < m && !in_lds; c0 += THREADS) {
        int j = c0 + threadIdx.x;
        int head = 0;
        if (j < m) {
            // never form keys[-1]: with flat addressing that leaves the LDS aperture
            const KT cur = keys[KX(j)];
            const KT prev = keys[KX(j > 0 ? j - 1 : 0)];
            head = (j == 0) || (k_major(cur) != k_major(prev));
            const uint32_t idx = k_idx(cur);
            if (MODE == 0) A.vox_pts[(size_t)base + off + j] = (int32_t)idx;
        }
        int th;
        int eh = block_excl_scan<THREADS>(head, th, wsum);
        if (head) vbeg[run + eh] = j;
        run += th;
    }
    __syncthreads();
    if (PV) PROF_MARK(3, 2);
    const int nv = run;
    if (MODE == 1) {
        // CentroidPoint (PCL 1.8.1 accumulators.hpp): fp32 running sums of x, y, z, intensity in ascending input index,
        // each divided by float(count); the intensity is the loader's scaled one when labels are given
        float4* tmp = (float4*)A.apri;  // idle in a VoxelGrid run: 16 of its 44 bytes per point hold the centroids
        for (int v = threadIdx.x; v < nv; v += THREADS) {
            const int j0 = vbeg[v];
            const int j1 = (v + 1 < nv) ? vbeg[v + 1] : m;
            float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
            for (int j = j0; j < j1; ++j) {
                const float4 p = A.pts[base + k_idx(keys[KX(j)])];
                sx += p.x;
                sy += p.y;
                sz += p.z;
                si += A.vg_labels ? p.w * A.vg_max_intensity : p.w;
            }
            const float fn = (float)(j1 - j0);
            tmp[(size_t)base + off + v] = make_float4(sx / fn, sy / fn, sz / fn, si / fn);
        }
        if (threadIdx.x == 0) A.vb_nvox[s * kMaxBuckets + b] = nv;
        __syncthreads();  // LDS is reused by the next item
        continue;
    }
    auto vox_key_of = [&](int j0) -> int32_t {
        return K32 ? (int32_t)(((int64_t)b << P.vb_shift) + (int64_t)k_major(keys[KX(j0)]) - P.key_off) : vx_unbias(k_major(keys[KX(j0)]));
    };
    if constexpr (DESC) {
        if (in_lds) {
            for (int j = threadIdx.x; j < m; j += THREADS) ints[j] = A.apri_int[(size_t)base + k_idx(keys[KX(j)])];
            __syncthreads();
        }
        if (PV) PROF_MARK(3, 3);
        // per voxel: sequential fp32 mean, then population variance accumulated as float += double
        for (int v = threadIdx.x; v < nv; v += THREADS) {
            const int j0 = vbeg[v];
            const int j1 = (v + 1 < nv) ? vbeg[v + 1] : m;
            float av, cov;
            if (in_lds)
                vx_descriptor<1>(j1 - j0, [&](int j) { return ints[j0 + j]; }, av, cov);
            else
                vx_descriptor<1>(j1 - j0, [&](int j) { return A.apri_int[(size_t)base + k_idx(keys[j0 + j])]; }, av, cov);
            A.tmp_vox_key[(size_t)base + off + v] = vox_key_of(j0);
            A.tmp_vox_cov[(size_t)base + off + v] = cov;
            A.tmp_vox_av[(size_t)base + off + v] = av;
        }
        __syncthreads();
        if (PV) PROF_MARK(3, 4);
        // vbeg aliases tmp_vox_begin in the oversize path: every thread rewrites only its own entries
        for (int v = threadIdx.x; v < nv; v += THREADS) A.tmp_vox_begin[(size_t)base + off + v] = off + vbeg[v];
    } else {
        if (PV) PROF_MARK(3, 3);
        if (PV) PROF_MARK(3, 4);
        // key and list start of every voxel; vbeg aliases tmp_vox_begin in the oversize path: a thread reads and rewrites only its own entries
        for (int v = threadIdx.x; v < nv; v += THREADS) {
            const int j0 = vbeg[v];
            A.tmp_vox_key[(size_t)base + off + v] = vox_key_of(j0);
            A.tmp_vox_begin[(size_t)base + off + v] = off + j0;
        }
    }
    if (threadIdx.x == 0) A.vb_nvox[s * kMaxBuckets + b] = nv;
    __syncthreads();  // LDS is reused by the next item
    if (PV) PROF_MARK(3, 5);
    }
#undef KX
}

__global__ __launch_bounds__(1024) void k_vx_final_offsets(DevParams P, Arena A) {
    __shared__ int wsum[17];
    const int s = blockIdx.x;
    int c = (threadIdx.x < (unsigned)P.n_buckets) ? A.vb_nvox[s * kMaxBuckets + threadIdx.x] : 0;
    int total;
    int ex = block_excl_scan<1024>(c, total, wsum);
    if (threadIdx.x <= (unsigned)P.n_buckets) A.vox_off[s * (kMaxBuckets + 1) + threadIdx.x] = ex;
    if (threadIdx.x == 0) {
        A.counts[s * 8 + 6] = total;
        A.vox_pt_begin[(size_t)A.scan_off[s] + s + total] = A.counts[s * 8 + 4];
    }
}

// one WAVE per (scan, bucket) -- a bucket holds a few dozen voxels -- four buckets per workgroup: a quarter of the workgroups to dispatch
// DESC = false: keys and point-list starts only (the lean form wrote no tmp_vox_av / tmp_vox_cov)
template <bool DESC>
__global__ __launch_bounds__(256) void k_vx_final(DevParams P, Arena A) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), s = blockIdx.y;
    if (b >= P.n_buckets) return;
    const int nv = A.vb_nvox[s * kMaxBuckets + b];
    if (nv == 0) return;
    const int base = A.scan_off[s];
    const int src = A.vb_off[s * (kMaxBuckets + 1) + b];
    const int dst = A.vox_off[s * (kMaxBuckets + 1) + b];
    for (int v = threadIdx.x & 63; v < nv; v += 64) {
        A.vox_key[(size_t)base + dst + v] = A.tmp_vox_key[(size_t)base + src + v];
        A.vox_pt_begin[(size_t)base + s + dst + v] = A.tmp_vox_begin[(size_t)base + src + v];
        if constexpr (DESC) {
            A.vox_av[(size_t)base + dst + v] = A.tmp_vox_av[(size_t)base + src + v];
            A.vox_cov[(size_t)base + dst + v] = A.tmp_vox_cov[(size_t)base + src + v];
        }
    }
}

// vox_av / vox_cov of scans [s0, s0 + gridDim.y) from the finished lists of a lean voxel stage, on demand (the batch's first fetch, the
// intensity merge).  A voxel's points stand in vox_pts in (key, apri index) order, the order the fused form sums in.  A thread per
// voxel: a 64-beam scan has 15 k voxels of three points on average, and the few voxels of several hundred points (next to the
// sensor) cost their thread two passes of eight gathers in flight -- short beside the scan's other voxels spread over the chip.
__global__ __launch_bounds__(256) void k_vx_descriptors(Arena A, int s0) {
    const int s = s0 + blockIdx.y;
    const int base = A.scan_off[s];
    const int nv = A.counts[s * 8 + 6];
    const int32_t* vbeg = A.vox_pt_begin + (size_t)base + s;
    const int32_t* vpts = A.vox_pts + (size_t)base;
    const float* in = A.apri_int + (size_t)base;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < nv; v += gridDim.x * 256) {
        const int j0 = vbeg[v];
        float av, cov;
        vx_descriptor<8>(vbeg[v + 1] - j0, [&](int j) { return in[vpts[j0 + j]]; }, av, cov);
        A.vox_av[(size_t)base + v] = av;
        A.vox_cov[(size_t)base + v] = cov;
    }
}
