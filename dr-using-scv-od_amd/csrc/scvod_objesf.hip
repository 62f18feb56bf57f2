// scvod_objesf.hip -- the ESF descriptor of grouped points on the device (gfx950): one 64-byte scvod_object_esf and, on request, the
// normalised 640-bin signature per object (scvod_esf_device, scvod_batch_object_esf).
//
// Reference analogue: SSC::getDescriptorByEnsembleShape (ssc.cpp:760-786), pcl::ESFEstimation behind it.  The definition is the
// esf_* functions of scvod_math.h (include/scvod.h states it; DESIGN.md section 2 says why parity is unpinned).
//
// k_esf: one 256-thread workgroup per object; the workgroups take objects from a counter until none is left, so an object that is
// masked out, too small or large costs its neighbours nothing and no workgroup waits for another.  Per object, all in LDS:
//     the points          raw, then scaled in place (up to kEsfCachePts; a larger object is read from global memory and scaled on
//                         every fetch -- the same two operations, the same bits)
//     centroid            wave 0, three sequential fp32 chains in member order (the rule of k_obj_reduce)
//     extent              an exact maximum (order-independent)
//     occupancy grid      64^3 bits = 32 KB; a point's 3x3x3 stamp is nine rows of three bits: one or two atomicOr per row
//     sweep 1             the samples spread over the lanes: draw, validity, the three lines through the grid, the corner and
//                         ratio bins (integer LDS atomics), the maxima (integer atomicMax on the bits of positive floats), and
//                         one byte per sample -- line and triangle classes, 255 = invalid -- into the workgroup's own slice of
//                         the stage's scratch
//     sweep 2             the same lane reads its byte back, redraws the triple and bins D2 / D3 against the maxima; no line is
//                         traced twice
//     signature           lane 0 adds the 640 values in order; every entry is divided once; ten lanes fold
// All counters are integers and both maxima exact, so nothing depends on which lane or workgroup did what: the record is the same
// bits on every run.  LDS: 78.7 KB per workgroup, two workgroups per CU.
#include <hip/hip_runtime.h>

#include "scvod_dev.h"

namespace scvod {
namespace {

constexpr int kEsfThreads = 256;
constexpr int kEsfGridWords = kEsfGrid * kEsfGrid * kEsfGrid / 32;

struct EsfLds {
    uint32_t grid[kEsfGridWords];
    int hist[kEsfSig];
    float px[kEsfCachePts], py[kEsfCachePts], pz[kEsfCachePts];  // (px[0 .. 640) holds the signature at the end)
    float T[64];
    float red[4];
    float c[3];
    float total;
    uint32_t max_d2, max_d3;   // bits of positive floats
    int cnt[4];                // valid samples, lines IN / OUT / MIX
    long long next;
};
static_assert(sizeof(EsfLds) <= 80 * 1024, "two workgroups must fit the 160 KB of a CU");

__device__ const float esf_cos_table[64] = SCVOD_ESF_COS_TABLE;

__device__ __forceinline__ bool esf_not_finite(float x) { return (f2u(x) & 0x7f800000u) == 0x7f800000u; }

__device__ __forceinline__ int esf_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ float esf_wave_max(float v) {  // of values that are numbers
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const float w = __shfl_xor(v, d, 64);
        v = w > v ? w : v;
    }
    return v;
}

__global__ __launch_bounds__(kEsfThreads) void k_esf(EsfJob J) {
    extern __shared__ __align__(16) unsigned char esf_smem[];
    EsfLds& S = *reinterpret_cast<EsfLds*>(esf_smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n_all = J.n_dev ? J.n_dev[1] : J.n_host;
    const long long n_obj = n_all < J.cap ? n_all : J.cap;
    if (blockIdx.x == 0 && tid == 0) {
        J.counters[0] = (unsigned long long)n_obj;
        J.counters[1] = (unsigned long long)n_all;
        J.counters[3] = n_all > J.cap ? 1ull : 0ull;
    }
    if (tid < 64) S.T[tid] = esf_cos_table[tid];
    uint8_t* const bytes = J.sample_bytes + (size_t)blockIdx.x * (size_t)J.samples;
    for (;;) {
        __syncthreads();  // the last object's LDS is read no more
        if (tid == 0) S.next = (long long)atomicAdd(&J.counters[8], 1ull);
        __syncthreads();
        const long long o = S.next;
        if (o >= n_obj) break;
        const int b = J.begin[o];
        int n = J.begin[o + 1] - b;
        if (n < 0) n = 0;
        int flags = 0;
        if (J.obj_cls) {
            const unsigned c = J.obj_cls[o];
            if (c >= 32u || !((J.cls_mask >> c) & 1u)) flags = kEsfFlagMasked;
        }
        if (!flags && n < J.min_points) flags = kEsfFlagFewPoints;
        const bool cached = n <= kEsfCachePts;
        float scale = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
        if (!flags) {
            if (cached)
                for (int i = tid; i < n; i += kEsfThreads) {
                    const float4 q = J.pts[(size_t)b + i];
                    S.px[i] = q.x, S.py[i] = q.y, S.pz[i] = q.z;
                }
            else if (tid == 0)
                atomicAdd(&J.counters[6], 1ull);
            for (int i = tid; i < kEsfGridWords; i += kEsfThreads) S.grid[i] = 0u;
            for (int i = tid; i < kEsfSig; i += kEsfThreads) S.hist[i] = 0;
            if (tid < 4) S.cnt[tid] = 0;
            if (tid == 0) S.max_d2 = 0u, S.max_d3 = 0u;
            __syncthreads();
            if (wave == 0) {  // the centroid: the loads of 64 points are the wave's, the additions one chain's
                float sx = 0.f, sy = 0.f, sz = 0.f;
                const auto load = [&](int i, float& x, float& y, float& z) {
                    x = y = z = 0.f;
                    if (i < n) {
                        if (cached) {
                            x = S.px[i], y = S.py[i], z = S.pz[i];
                        } else {
                            const float4 q = J.pts[(size_t)b + i];
                            x = q.x, y = q.y, z = q.z;
                        }
                    }
                };
                float nx, ny, nz;
                load(lane, nx, ny, nz);
                for (int j = 0; j < n; j += 64) {
                    const float x = nx, y = ny, z = nz;
                    load(j + 64 + lane, nx, ny, nz);  // the next 64 points are in flight while this round's additions run
                    if (n - j >= 64) {
#pragma unroll
                        for (int k = 0; k < 64; ++k) {
                            sx += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), k));
                            sy += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), k));
                            sz += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z), k));
                        }
                    } else {
                        for (int k = 0; k < n - j; ++k) {
                            sx += __shfl(x, k, 64);
                            sy += __shfl(y, k, 64);
                            sz += __shfl(z, k, 64);
                        }
                    }
                }
                if (lane == 0) {
                    const float cnt = (float)n;
                    S.c[0] = sx / cnt, S.c[1] = sy / cnt, S.c[2] = sz / cnt;
                }
            }
            __syncthreads();
            cx = S.c[0], cy = S.c[1], cz = S.c[2];
            float r2 = 0.f;
            for (int i = tid; i < n; i += kEsfThreads) {
                float x, y, z;
                if (cached) {
                    x = S.px[i], y = S.py[i], z = S.pz[i];
                } else {
                    const float4 q = J.pts[(size_t)b + i];
                    x = q.x, y = q.y, z = q.z;
                }
                const float d2 = esf_dist2(x, y, z, cx, cy, cz);
                if (d2 > r2) r2 = d2;  // (what is no number never is the maximum)
            }
            r2 = esf_wave_max(r2);
            if (lane == 0) S.red[wave] = r2;
            __syncthreads();
            r2 = S.red[0];
            for (int w = 1; w < 4; ++w)
                if (S.red[w] > r2) r2 = S.red[w];
            const float r = sqrt_f(r2);
            if (r == 0.f || esf_not_finite(r)) flags = kEsfFlagExtent;
            scale = 32.0f / r;
        }
        if (flags) {  // (the same on every lane)
            if (tid < 10) J.out[o].fold10[tid] = 0.f;
            if (tid == 10) {
                ObjEsf& r = J.out[o];
                r.n_valid = 0, r.n_points = n, r.flags = flags;
                r.lines[0] = r.lines[1] = r.lines[2] = 0u;
                atomicAdd(&J.counters[2], 1ull);
                if (flags & kEsfFlagMasked) atomicAdd(&J.counters[5], 1ull);
            }
            if (J.sig)
                for (int i = tid; i < kEsfSig; i += kEsfThreads) J.sig[(size_t)o * kEsfSig + i] = 0.f;
            continue;
        }
        // scaled points and the occupancy grid
        for (int i = tid; i < n; i += kEsfThreads) {
            float x, y, z;
            if (cached) {
                x = S.px[i], y = S.py[i], z = S.pz[i];
            } else {
                const float4 q = J.pts[(size_t)b + i];
                x = q.x, y = q.y, z = q.z;
            }
            const float ux = (x - cx) * scale, uy = (y - cy) * scale, uz = (z - cz) * scale;
            if (cached) S.px[i] = ux, S.py[i] = uy, S.pz[i] = uz;
            const int vx = esf_voxel(ux), vy = esf_voxel(uy), vz = esf_voxel(uz);
            const unsigned long long row = vx == 0 ? 3ull : (7ull << (vx - 1));  // voxels vx - 1 .. vx + 1 of a row of 64, clipped
            const uint32_t lo = (uint32_t)row, hi = (uint32_t)(row >> 32);
            for (int z1 = (vz > 0 ? vz - 1 : 0); z1 <= (vz < kEsfGrid - 1 ? vz + 1 : kEsfGrid - 1); ++z1)
                for (int y1 = (vy > 0 ? vy - 1 : 0); y1 <= (vy < kEsfGrid - 1 ? vy + 1 : kEsfGrid - 1); ++y1) {
                    uint32_t* w = S.grid + (z1 * kEsfGrid + y1) * 2;
                    if (lo) atomicOr(w, lo);
                    if (hi) atomicOr(w + 1, hi);
                }
        }
        __syncthreads();
        const auto pt = [&](int i, float u[3]) {
            if (cached) {
                u[0] = S.px[i], u[1] = S.py[i], u[2] = S.pz[i];
            } else {
                const float4 q = J.pts[(size_t)b + i];
                u[0] = (q.x - cx) * scale, u[1] = (q.y - cy) * scale, u[2] = (q.z - cz) * scale;
            }
        };
        // sweep 1
        int nv = 0, nl[3] = {0, 0, 0};
        float m2 = 0.f, m3 = 0.f;
        for (int k = tid; k < J.samples; k += kEsfThreads) {
            float u[3][3];
            const EsfSample s = esf_sample(J.seed, (uint32_t)k, n, pt, u);
            uint8_t code = 255;
            if (s.valid) {
                const EsfLines L = esf_trace(S.grid, u);
                int bins[3];
                esf_corner_bins(S.T, u, s, bins);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    atomicAdd(&S.hist[esf_row_a3(L.tri) * kEsfBins + bins[a]], 1);
                    if (L.ratio_bin[a] >= 0) atomicAdd(&S.hist[kEsfRowRatio * kEsfBins + L.ratio_bin[a]], 1);
                    nl[0] += L.cls[a] == kEsfIn, nl[1] += L.cls[a] == kEsfOut, nl[2] += L.cls[a] == kEsfMix;
                }
                float d = s.a > s.b ? s.a : s.b;
                d = s.c > d ? s.c : d;
                m2 = d > m2 ? d : m2;
                const float d3 = sqrt_f(sqrt_f(s.heron));
                m3 = d3 > m3 ? d3 : m3;
                ++nv;
                code = (uint8_t)(L.cls[0] + 3 * L.cls[1] + 9 * L.cls[2] + 27 * L.tri);
            }
#ifndef SCVOD_ESF_RETRACE
            bytes[k] = code;
#endif
        }
        nv = esf_wave_sum(nv);
#pragma unroll
        for (int a = 0; a < 3; ++a) nl[a] = esf_wave_sum(nl[a]);
        m2 = esf_wave_max(m2);
        m3 = esf_wave_max(m3);
        if (lane == 0) {
            atomicAdd(&S.cnt[0], nv);
#pragma unroll
            for (int a = 0; a < 3; ++a) atomicAdd(&S.cnt[1 + a], nl[a]);
            atomicMax(&S.max_d2, f2u(m2));
            atomicMax(&S.max_d3, f2u(m3));
        }
        __syncthreads();
        // sweep 2: D2 and D3 against the maxima
        const float max_d2 = u2f(S.max_d2), max_d3 = u2f(S.max_d3);
        for (int k = tid; k < J.samples; k += kEsfThreads) {
            float u[3][3];
#ifndef SCVOD_ESF_RETRACE
            const int code = bytes[k];  // (this lane's own store)
            if (code == 255) continue;
            const EsfSample s = esf_sample(J.seed, (uint32_t)k, n, pt, u);
#else  // development build (make esf_retrace): no byte per sample, every line is traced again; measured in profiles/object_esf_cost.txt
            const EsfSample s = esf_sample(J.seed, (uint32_t)k, n, pt, u);
            if (!s.valid) continue;
            const EsfLines L = esf_trace(S.grid, u);
            const int code = L.cls[0] + 3 * L.cls[1] + 9 * L.cls[2] + 27 * L.tri;
#endif
            const int tri = code / 27;
            const int lc[3] = {code % 3, (code / 3) % 3, (code / 9) % 3};
            atomicAdd(&S.hist[esf_row_d3(tri) * kEsfBins + esf_bin_of(sqrt_f(sqrt_f(s.heron)), max_d3)], 1);
            atomicAdd(&S.hist[esf_row_d2(lc[0]) * kEsfBins + esf_bin_of(s.a, max_d2)], 1);
            atomicAdd(&S.hist[esf_row_d2(lc[1]) * kEsfBins + esf_bin_of(s.b, max_d2)], 1);
            atomicAdd(&S.hist[esf_row_d2(lc[2]) * kEsfBins + esf_bin_of(s.c, max_d2)], 1);
        }
        __syncthreads();
        // the signature
        if (tid == 0) {
            float total = 0.f;
            for (int i = 0; i < kEsfSig; ++i) total += esf_sig_value(i, S.hist[i]);
            S.total = total;
        }
        __syncthreads();
        const float total = S.total;
        const bool empty = total == 0.f;
        for (int i = tid; i < kEsfSig; i += kEsfThreads) {
            const float v = empty ? 0.f : esf_sig_value(i, S.hist[i]) / total;
            S.px[i] = v;
            if (J.sig) J.sig[(size_t)o * kEsfSig + i] = v;
        }
        __syncthreads();
        if (tid < 10) J.out[o].fold10[tid] = esf_fold(S.px, tid);
        if (tid == 10) {
            ObjEsf& r = J.out[o];
            r.n_valid = S.cnt[0], r.n_points = n, r.flags = empty ? kEsfFlagNoSample : 0;
            r.lines[0] = (uint32_t)S.cnt[1], r.lines[1] = (uint32_t)S.cnt[2], r.lines[2] = (uint32_t)S.cnt[3];
            if (empty) atomicAdd(&J.counters[2], 1ull);
            atomicAdd(&J.counters[4], (unsigned long long)S.cnt[0]);
        }
    }
}

// member slot p of the table -> the point obj_load (scvod_objects.hip) reads for it; object o -> the class byte of its first member
__global__ __launch_bounds__(256) void k_esf_gather(Arena A, const uint64_t* key_out, const int32_t* begin, const long long* tab_stats,
                                                    const uint8_t* cls, float4* pts_out, uint8_t* cls_out) {
    const long long n_obj = tab_stats[1];
    const long long members = n_obj > 0 ? begin[n_obj] : 0;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < members; p += (long long)gridDim.x * 256) {
        const uint32_t g = (uint32_t)key_out[p];
        int lo = 0, hi = A.n_scans;  // the scan of slot g: the last s with scan_off[s] <= g
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((uint32_t)A.scan_off[mid] <= g) lo = mid; else hi = mid;
        }
        const int base = A.scan_off[lo];
        const int scan_n = A.scan_off[lo + 1] - base;
        const int src = A.apri_src[g];
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)src < (unsigned)scan_n) q = A.pts[(size_t)base + src];
        pts_out[p] = q;
        if (p < n_obj) cls_out[p] = cls[(uint32_t)key_out[begin[p]]];
    }
}

}  // namespace

size_t esf_work_bytes(int blocks, int samples) { return ((size_t)blocks * (size_t)samples + 255) & ~(size_t)255; }

void launch_esf(const EsfJob& J, hipStream_t st) {
    // (function attributes are per device: set on every launch, as the sibling units do)
    hipFuncSetAttribute((const void*)k_esf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(EsfLds));
    hipMemsetAsync(J.counters, 0, sizeof(unsigned long long) * 16, st);
    hipLaunchKernelGGL(k_esf, dim3((unsigned)J.blocks), dim3(kEsfThreads), sizeof(EsfLds), st, J);
}

void launch_esf_gather(const Arena& A, const uint64_t* key_out, const int32_t* begin, const long long* tab_stats, const uint8_t* cls,
                       float4* pts_out, uint8_t* cls_out, hipStream_t st) {
    long long blocks = (A.total_pts + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_esf_gather, dim3((unsigned)blocks), dim3(256), 0, st, A, key_out, begin, tab_stats, cls, pts_out, cls_out);
}

}  // namespace scvod
