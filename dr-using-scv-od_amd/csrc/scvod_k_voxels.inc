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
// COUNT = true (KT = uint32_t, MODE 0; launch_vx_tier picks it when the batch's buckets span 2^kVxCountShift keys): no network -- the bucket's
// points are placed by key counting (vx_bucket_count below); only a bucket whose largest voxel exceeds kVxCountDense points is sorted.
// Both forms write the same arrays, bit for bit: keys are unique, ascending (key, apri index) is one total order.
// LDS of a COUNT workgroup: cnt[2^kVxCountShift] (a voxel's population, then start | population << 16) + lst[CAP + 4] (the keys listed by
// voxel, 4 pad keys) (+ DESC: c_int[CAP] intensities in final order, c_vbeg[CAP] voxel starts) + the scan's wave sums; it is given the larger
// of this and the network's need, which a dense bucket uses (vox_lds_bytes).
// LDS of one network workgroup: padded keys + voxel starts + staged intensities (+ the scan's wave sums).  SCVOD_VOX_K32_LDS = 1: the key
// area of the 4-byte keys is 4 bytes per slot, which lets a third (sixth, twelfth) workgroup of the 4096 (2048, 1024) tier onto a CU
#ifndef SCVOD_VOX_K32_LDS
#define SCVOD_VOX_K32_LDS 1
#endif
constexpr size_t vox_key_bytes(int cap, size_t ksize) { return (((size_t)(cap + cap / 8) * (SCVOD_VOX_K32_LDS ? ksize : 8)) + 15) & ~(size_t)15; }
// DESC = false (the lean form): no staged intensities; what is left of that area holds the <= 128 (chunk, wave) head counts
constexpr size_t vox_aux_bytes(int cap, bool desc) { return desc ? (size_t)cap * 4 : ((size_t)(cap / 64) * 4 + 15) & ~(size_t)15; }
// The counting form (32-bit keys, MODE 0): a bucket whose keys span 2^kVxCountShift voxels is ordered without a comparison network --
// one LDS counter per voxel of the span gives every voxel's population, the prefix over the counters every voxel's start (the voxel's key
// is the counter's index), and a point's place is its voxel's start + the number of smaller keys in the voxel's own segment.
// SCVOD_VOX_COUNT = 0: network everywhere, 1: the tiers measured faster with it (profiles/voxel_counting_cost.md), 2: every tier that can
#ifndef SCVOD_VOX_COUNT
#define SCVOD_VOX_COUNT 1
#endif
constexpr int kVxCountShift = 12;     // the span the counters are sized for: semantickitti and parkinglot grids (os128_fine: 2^14, network)
// a bucket whose largest voxel holds more points than this takes the network: the segment walks of a voxel of c points cost c^2 / 4 16-byte
// reads, 16 k at c = 256 next to the 229 k accesses of the network on 4096 keys.  Measured (tools/voxel_dense_bench.py): one voxel of c
// points per bucket crosses the network's time near c = 480, and a bucket that falls back pays 37 % more than the network alone; 256 leaves
// room for several such voxels in one bucket, the criterion sees the largest only (profiles/voxel_counting_cost.md)
#ifndef SCVOD_VOX_COUNT_DENSE
#define SCVOD_VOX_COUNT_DENSE 256
#endif
constexpr int kVxCountDense = SCVOD_VOX_COUNT_DENSE;
#ifndef SCVOD_VOX_COUNT_M
#define SCVOD_VOX_COUNT_M 4  // workgroups per CU of the lean 2048 tier in the counting form (24.7 KB of LDS, 116 VGPRs; the network form runs eight)
#endif
#ifndef SCVOD_VOX_COUNT_L
#define SCVOD_VOX_COUNT_L 2  // ... of the lean 4096 tier (35.2 KB of LDS, the network fallback's): two leave the kernel its 120 VGPRs; at three (80 VGPRs) it spills 40 and is 0.26 ms slower
#endif
// which tiers count, next to vx_bucket_padfree: the 256 and 1024 tiers cannot hold 16 KB of counters per workgroup at their 32 and 12 workgroups
// per CU; the fused (DESC) form is tested but not timed, it counts with SCVOD_VOX_COUNT=2 only
constexpr bool vx_bucket_counting(int cap, size_t ksize, int mode, bool desc) {
    return ksize == 4 && mode == 0 && cap >= 2048 && (SCVOD_VOX_COUNT == 2 || (SCVOD_VOX_COUNT == 1 && !desc));
}
// workgroups per CU of the counting kernels: ONE place for the launch (launch_vx_tier) and for the kernels' amdgpu_waves_per_eu bound
// (per CU x waves of a workgroup / 4 SIMDs).  The fused (DESC) form's LDS (40.1 / 64.2 KB) allows three / two
constexpr int vx_count_per_cu(int cap, bool desc) { return cap >= 8192 ? 1 : cap >= 4096 ? (desc ? 2 : SCVOD_VOX_COUNT_L) : (desc ? 3 : SCVOD_VOX_COUNT_M); }
// LDS of the counting form: counters + the bucket's keys listed by voxel (+ 4 pad keys) (+ DESC: staged intensities, voxel starts)
constexpr size_t vox_count_bytes(int cap, bool desc) { return ((size_t)4 << kVxCountShift) + (size_t)(cap + 4) * 4 + (desc ? (size_t)cap * 8 : 0); }
constexpr size_t vox_lds_bytes(int cap, size_t ksize = 8, bool desc = true, bool count = false) {
    const size_t net = vox_key_bytes(cap, ksize) + (size_t)cap * 4 + vox_aux_bytes(cap, desc);
    const size_t cnt = count ? vox_count_bytes(cap, desc) : 0;  // (a dense bucket takes the network in the same kernel)
    return (net > cnt ? net : cnt) + 128;
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
// The counting form of one bucket in LDS (see vx_bucket_counting above).  Returns false, having written nothing, when the bucket's largest
// voxel exceeds kVxCountDense: the caller's network takes it.  Uniform over the workgroup.
struct VxCountArgs {
    const uint32_t* gkeys;   // the bucket's m keys, (voxel key relative to the bucket) << ib | apri index, in arbitrary order
    int32_t* vox_pts;        // the outputs, all at the bucket's place (base + off)
    int32_t* out_key;
    int32_t* out_beg;
    float* out_av;
    float* out_cov;
    const float* apri_int;   // the scan's
    int32_t* nvox;
    int32_t key0;
    int m, off, ib;
};
template <int CAP, int THREADS, bool DESC, bool PV>
__device__ __forceinline__ bool vx_bucket_count(const VxCountArgs& ca
#ifdef SCVOD_PROFILE
                                             , unsigned long long& t_prev
#endif
) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int SPAN = 1 << kVxCountShift;
    constexpr int IT = CAP / THREADS;    // keys per thread
    constexpr int CPT = SPAN / THREADS;  // consecutive counters per thread in the prefix
    static_assert(CPT % 4 == 0 && IT % 2 == 0 && CAP <= 8192, "16-byte counter reads; start (13 bits) and count (14) share a word");
    uint32_t* cnt = (uint32_t*)smem;                                 // [SPAN] population, then start | population << 16
    uint32_t* lst = cnt + SPAN;                                      // [CAP + 4] the keys listed by voxel, in arrival order
    float* c_int = (float*)(lst + CAP + 4);                          // [CAP] (DESC) intensities in final order
    int* c_vbeg = (int*)(c_int + CAP);                               // [CAP] (DESC) voxel starts
    int* c_wsum = (int*)(smem + vox_count_bytes(CAP, DESC));
    const int m = ca.m, ib = ca.ib;
    const uint32_t imask = (1u << ib) - 1u;
    for (int i = threadIdx.x; i < SPAN / 4; i += THREADS) ((uint4*)cnt)[i] = make_uint4(0u, 0u, 0u, 0u);
    uint32_t key[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it)  // all of a thread's key loads in flight together (coalesced); m > 0
        key[it] = ca.gkeys[min(it * THREADS + (int)threadIdx.x, m - 1)];
    __syncthreads();
    if (PV) PROF_MARK(3, 0);
    // arrival number of every key in its voxel (arbitrary order), two 16-bit numbers per register
    uint32_t arr[IT / 2];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        uint32_t a = 0u;
        if (it * THREADS + (int)threadIdx.x < m) a = atomicAdd(&cnt[key[it] >> ib], 1u);
        if (it & 1)
            arr[it / 2] |= a << 16;
        else
            arr[it / 2] = a;
    }
    __syncthreads();
    if (PV) PROF_MARK(3, 1);
    // population of the thread's CPT consecutive voxels; they are read again after the prefix, not held
    const uint4* my_cnt = (const uint4*)cnt + threadIdx.x * (CPT / 4);
    uint32_t sum = 0, nz = 0, mx = 0;
#pragma unroll
    for (int q = 0; q < CPT / 4; ++q) {
        const uint4 x = my_cnt[q];
        sum += x.x + x.y + x.z + x.w;
        nz += (x.x ? 1u : 0u) + (x.y ? 1u : 0u) + (x.z ? 1u : 0u) + (x.w ? 1u : 0u);
        mx = max(max(mx, max(x.x, x.y)), max(x.z, x.w));
    }
    if (__syncthreads_or(mx > (uint32_t)kVxCountDense)) return false;
    int tot;
    const int ex = block_excl_scan<THREADS>((int)(sum | (nz << 16)), tot, c_wsum);  // (points <= 8192, voxels <= 4096: no carry)
    const int nv = tot >> 16;
    int start = ex & 0xffff, v = ex >> 16;
    int32_t vkey = ca.key0 + (int32_t)threadIdx.x * CPT;  // the voxel's key is the counter's index: no key is read for it
    auto voxel = [&](uint32_t& n) {
        if (n) {
            ca.out_key[v] = vkey;
            ca.out_beg[v] = ca.off + start;
            if constexpr (DESC) c_vbeg[v] = start;
            const int first = start;
            start += (int)n;
            n = (uint32_t)first | (n << 16);
            ++v;
        }
        ++vkey;
    };
#pragma unroll
    for (int q = 0; q < CPT / 4; ++q) {
        uint4 x = my_cnt[q];
        voxel(x.x);
        voxel(x.y);
        voxel(x.z);
        voxel(x.w);
        ((uint4*)cnt)[threadIdx.x * (CPT / 4) + q] = x;
    }
    if (threadIdx.x < 4) lst[m + (int)threadIdx.x] = 0xffffffffu;  // (the walks below read whole 16-byte groups)
    if (threadIdx.x == 0) *ca.nvox = nv;
    __syncthreads();
    if (PV) PROF_MARK(3, 2);
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        if (it * THREADS + (int)threadIdx.x < m)
            lst[(cnt[key[it] >> ib] & 0xffffu) + ((arr[it / 2] >> ((it & 1) * 16)) & 0xffffu)] = key[it];
    }
    __syncthreads();
    if (PV) PROF_MARK(3, 3);
    // by position: neighbouring lanes stand in the same voxel, their walks are equally long and their reads broadcast.  Keys are
    // unique and ascend with the voxel, so place = keys below mine in [start rounded down to 4, end of my voxel's segment)
    for (int p = threadIdx.x; p < m; p += THREADS) {
        const uint32_t k = lst[p];
        const uint32_t sc = cnt[k >> ib];
        const int end = (int)(sc & 0xffffu) + (int)(sc >> 16);
        int place = (int)(sc & 0xfffcu);
        for (int q = place; q < end; q += 4) {
            const uint4 x = *(const uint4*)(lst + q);
            place += (int)(x.x < k) + (int)(x.y < k) + (int)(x.z < k) + (int)(x.w < k);
        }
        ca.vox_pts[place] = (int32_t)(k & imask);
        if constexpr (DESC) c_int[place] = ca.apri_int[k & imask];
    }
    if constexpr (DESC) {
        __syncthreads();
        if (PV) PROF_MARK(3, 4);
        // per voxel: sequential fp32 mean, then population variance accumulated as float += double, in list order
        for (int u = threadIdx.x; u < nv; u += THREADS) {
            const int j0 = c_vbeg[u];
            const int j1 = (u + 1 < nv) ? c_vbeg[u + 1] : m;
            float av, cov;
            vx_descriptor<1>(j1 - j0, [&](int j) { return c_int[j0 + j]; }, av, cov);
            ca.out_cov[u] = cov;
            ca.out_av[u] = av;
        }
    } else {
        if (PV) PROF_MARK(3, 4);
    }
    __syncthreads();  // LDS is reused by the next item
    if (PV) PROF_MARK(3, 5);
    return true;
}
// which tiers run the pad-free network (scvod_sortnet.h): those measured faster with it (profiles/padfree_sort_cost.md);
// the 256 and 1024 tiers are slower, they keep the padded network.  SCVOD_VOX_PADFREE=0: none, 2: all
constexpr bool vx_bucket_padfree(int cap) { return SCVOD_VOX_PADFREE == 2 || (SCVOD_VOX_PADFREE == 1 && cap >= 2048); }
// DESC = false (MODE 0 only): the lean form of a batch whose descriptors are computed on demand (k_vx_descriptors) -- no intensity
// staging, no per-voxel sums, no tmp_vox_av / tmp_vox_cov
// COUNT: the kernel of a batch whose buckets span 2^kVxCountShift keys (chosen at the launch, launch_vx_tier): buckets count, dense ones sort
template <int CAP, int THREADS, int C_LO, int C_HI, int LGE, int MODE = 0, typename KT = unsigned long long, bool DESC = true, bool COUNT = false>
__global__ __launch_bounds__(THREADS)
#if SCVOD_VOX_K32_LDS
__attribute__((amdgpu_waves_per_eu((sizeof(KT) == 4 && CAP <= 4096 && CAP >= 2048) ? (COUNT ? vx_count_per_cu(CAP, DESC) * (THREADS / 64) / 4 : DESC ? 6 : 2 * SCVOD_VOX_LEAN_MORE) : 1, 8)))
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
    if constexpr (COUNT) {
        static_assert(vx_bucket_counting(CAP, sizeof(KT), MODE, DESC), "a tier that counts");
        if (in_lds) {
            VxCountArgs ca;
            ca.gkeys = (const uint32_t*)gkeys;
            ca.vox_pts = A.vox_pts + (size_t)base + off;
            ca.out_key = A.tmp_vox_key + (size_t)base + off;
            ca.out_beg = A.tmp_vox_begin + (size_t)base + off;
            ca.out_av = DESC ? A.tmp_vox_av + (size_t)base + off : nullptr;
            ca.out_cov = DESC ? A.tmp_vox_cov + (size_t)base + off : nullptr;
            ca.apri_int = DESC ? A.apri_int + (size_t)base : nullptr;
            ca.nvox = A.vb_nvox + s * kMaxBuckets + b;
            ca.key0 = (int32_t)(((int64_t)b << P.vb_shift) - P.key_off);  // the key of the bucket's first voxel (as vox_key_of forms it)
            ca.m = m;
            ca.off = off;
            ca.ib = A.vx_idx_bits;
#ifdef SCVOD_PROFILE
            if (vx_bucket_count<CAP, THREADS, DESC, PV>(ca, t_prev)) continue;
#else
            if (vx_bucket_count<CAP, THREADS, DESC, PV>(ca)) continue;
#endif
            // (a dense bucket: the network below reads its keys again, nothing has been written yet)
        }
    }
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
