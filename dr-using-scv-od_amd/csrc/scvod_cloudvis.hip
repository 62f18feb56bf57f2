// scvod_cloudvis.hip -- a world-frame cloud against the range images of every scan of a trajectory (gfx950).  The kernels of
// scvod_cloud_visibility_device and the host-only functions of the stage (defaults, parameter check).
//
// Reference analogue: none (include/scvod.h, DESIGN.md section 2: this project's convention).  The pair rule is the scan stage's
// (scvod_vispair.h); what differs is who looks at what: every scan of the call is a viewer of every point, and nearly all of those
// (point, scan) pairs are OUTSIDE -- the point is farther from the sensor than the grid reaches.  The stage exists to not pay for them.
//
// k_cvis_key    one key per point: the interleaved (Morton) bits of its 2 m world tile in x and y, so consecutive keys are neighbours;
//               records that are not finite and tiles beyond +-16.384 km get the last key.  rocprim::radix_sort_pairs orders
//               (key, index) on the kCvisKeyBits bits a key can differ in.
// k_cvis_vote   a workgroup -- one wave -- owns kCvisChunk consecutive points of the sorted list (or of the input, SCVOD_CVIS_NO_SORT) and
//               keeps its 8 records per thread in registers.  It reduces the chunk's bounding box and, around the box's centre, its bounding radius
//               once; then it walks all scans, 64 at a time: lane l moves the centre into the frame of scan s0 + l, and the scan is skipped
//               when the centre's 2-D distance minus the radius exceeds the reach plus a slack (DESIGN.md section 2 states the bound):
//               no point of the chunk can then have a pair that is not OUTSIDE.  The ballot of the scans that are left is uniform; for
//               each of them the matrix comes through uniform loads and every record gets its exact class.  Counters and verdict go to
//               the ORIGINAL index.
// No workgroup waits for another; the only LDS are the reduction words.  Every sum is an integer: all outputs are the same on every run
// and do not depend on the order of the points.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <cstring>
#include <initializer_list>

#include "scvod_vispair.h"

namespace scvod {
namespace {

// the key: kCvisAxisBits bits per axis, interleaved; tiles of kCvisTileEdge metres, 2^kCvisAxisBits of them per axis around the origin
// (+-16.384 km).  The sort runs over the kCvisKeyBits bits a key can differ in.
constexpr int kCvisAxisBits = 14;
constexpr int kCvisKeyBits = 2 * kCvisAxisBits;
constexpr float kCvisTileEdge = 2.0f;
constexpr float kCvisTiles = (float)(1 << kCvisAxisBits);

static __device__ __forceinline__ uint32_t cvis_spread(uint32_t v) {  // bit k of a 16-bit value to bit 2 k
    v &= 0xFFFFu;
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

__global__ __launch_bounds__(256) void k_cvis_key(const float4* __restrict__ pts, long long n, uint32_t* __restrict__ key,
                                                  uint32_t* __restrict__ idx) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 q = pts[i];
    uint32_t k = (1u << kCvisKeyBits) - 1u;
    if (vis_finite(q.x, q.y, q.z)) {
        const float tx = floorf(q.x * (1.0f / kCvisTileEdge)) + 0.5f * kCvisTiles, ty = floorf(q.y * (1.0f / kCvisTileEdge)) + 0.5f * kCvisTiles;
        if (tx >= 0.0f && tx < kCvisTiles && ty >= 0.0f && ty < kCvisTiles) k = cvis_spread((uint32_t)tx) | (cvis_spread((uint32_t)ty) << 1);
    }
    key[i] = k;
    idx[i] = (uint32_t)i;
}

// the class of one (point, viewer) pair of this stage: 0 THROUGH, 1 AGREE, 2 OCCLUDED, 3 EMPTY, 4 OUTSIDE.  Every OUTSIDE case of vis_pair
// is decided here first (with the one addition of this stage, max_range), so vis_pair's 3 is EMPTY
static __device__ __forceinline__ int cvis_pair(const CvisJob& J, const float* __restrict__ img, int A, int S, float x, float y, float z) {
    // makeApriVec's range test on the same sqrt: beyond the reach the pair is OUTSIDE whatever its angles are (a NaN passes on)
    const float d2 = point_distance2d(x, y);
    if (d2 > J.reach || d2 < J.V.bin.min_dis) return 4;
    if (!vis_finite(x, y, z)) return 4;
    float dis;
    int32_t si, ai;
    if (!vis_bin(J.V, x, y, z, &dis, &si, &ai)) return 4;
    if (si < 0 || si >= S || ai < 0 || ai >= A) return 4;
    if (J.max_range > 0.0f && dis > J.max_range) return 4;
    return vis_pair(J.V, img, A, S, x, y, z);
}

static __device__ __forceinline__ float cvis_uniform(float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); }

static __device__ __forceinline__ float cvis_wave_min(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
    return v;
}
static __device__ __forceinline__ float cvis_wave_max(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}

__global__ __launch_bounds__(kCvisThreads) void k_cvis_vote(CvisJob J) {
    constexpr int NW = kCvisThreads / 64;
    __shared__ float box[NW][8];
    __shared__ unsigned int wcnt[NW][10];
    const int S = J.V.bin.sector_num, A = J.V.bin.azimuth_num;
    const size_t img_words = (size_t)A * (size_t)S;
    const long long i0 = (long long)blockIdx.x * kCvisChunk + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float qx[8], qy[8], qz[8];
    unsigned long long cnt[8];  // four 16-bit counters: THROUGH, AGREE, OCCLUDED, EMPTY (n_scans <= 65535: none wraps)
    unsigned int fin = 0;       // bit u: record u of this thread exists and is finite
    const float inf = __builtin_inff();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const long long i = i0 + u * kCvisThreads;
        qx[u] = qy[u] = qz[u] = 0.f;
        cnt[u] = 0ull;
        if (i < J.n) {
            const float4 q = J.pts[J.order ? (size_t)J.order[i] : (size_t)i];
            qx[u] = q.x;
            qy[u] = q.y;
            qz[u] = q.z;
            if (vis_finite(q.x, q.y, q.z)) {
                fin |= 1u << u;
                lo[0] = fminf(lo[0], q.x), hi[0] = fmaxf(hi[0], q.x);
                lo[1] = fminf(lo[1], q.y), hi[1] = fmaxf(hi[1], q.y);
                lo[2] = fminf(lo[2], q.z), hi[2] = fmaxf(hi[2], q.z);
            }
        }
    }
    // the chunk's box, its centre, and the largest distance of a finite record from that centre
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = cvis_wave_min(lo[k]), b = cvis_wave_max(hi[k]);
        if (lane == 0) box[w][k] = a, box[w][3 + k] = b;
    }
    __syncthreads();
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float a = box[0][k], b = box[0][3 + k];
#pragma unroll
        for (int v = 1; v < NW; ++v) a = fminf(a, box[v][k]), b = fmaxf(b, box[v][3 + k]);
        c[k] = cvis_uniform(0.5f * a + 0.5f * b);  // (an empty chunk: NaN, and `any` below is false)
    }
    float r2 = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u)
        if ((fin >> u) & 1u) {
            const float dx = qx[u] - c[0], dy = qy[u] - c[1], dz = qz[u] - c[2];
            r2 = fmaxf(r2, dx * dx + dy * dy + dz * dz);
        }
    r2 = cvis_wave_max(r2);
    const unsigned long long wave_any = __ballot(fin != 0u);
    if (lane == 0) box[w][6] = r2, box[w][7] = wave_any ? 1.f : 0.f;
    __syncthreads();
    float r2max = box[0][6], n_any = box[0][7];
#pragma unroll
    for (int v = 1; v < NW; ++v) r2max = fmaxf(r2max, box[v][6]), n_any += box[v][7];
    const float rad = cvis_uniform(sqrtf(r2max));
    const bool any = cvis_uniform(n_any) > 0.f;
    const float reach_c = J.reach + 1.0e-3f + 2.0e-5f * (fabsf(c[0]) + fabsf(c[1]) + fabsf(c[2]) + rad);
    unsigned int steps = 0;  // scans of this chunk that were not skipped (uniform)
    const int n_scans = any ? J.n_scans : 0;
    for (int s0 = 0; s0 < n_scans; s0 += 64) {
        // 64 scans at a time, one per lane: the centre in the viewer's frame.  A point of the chunk lies within rad of it, so its 2-D
        // distance from the sensor is at least d - rad; the slack covers the fp32 rounding of both transforms, of the radius and of
        // a matrix that is a rotation to a few ulp.  A NaN or inf - inf on either side compares false: the scan is then looked at.
        bool look = false;
        if (s0 + lane < n_scans) {
            const float* M = J.T + 12 * (size_t)(s0 + lane);
            const float ux = M[0] * c[0] + M[1] * c[1] + M[2] * c[2] + M[3];
            const float uy = M[4] * c[0] + M[5] * c[1] + M[6] * c[2] + M[7];
            const float d = point_distance2d(ux, uy);
            look = !(d - rad > reach_c + 2.0e-5f * (fabsf(M[3]) + fabsf(M[7]) + fabsf(M[11])));
        }
        unsigned long long todo = __ballot(look);  // (uniform: the scans of this group that are looked at)
        while (todo) {
            const int s = s0 + (int)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const float* M = J.T + 12 * (size_t)s;
            float T[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = cvis_uniform(M[k]);
            ++steps;
            const float* __restrict__ img = J.images + (size_t)s * img_words;
#pragma unroll 2
            for (int u = 0; u < 8; ++u) {
                if (!((fin >> u) & 1u)) continue;
                // the map kernel's expression: left to right in fp32, no contraction
                const float x = T[0] * qx[u] + T[1] * qy[u] + T[2] * qz[u] + T[3];
                const float y = T[4] * qx[u] + T[5] * qy[u] + T[6] * qz[u] + T[7];
                const float z = T[8] * qx[u] + T[9] * qy[u] + T[10] * qz[u] + T[11];
                const int cls = cvis_pair(J, img, A, S, x, y, z);
                if (cls < 4) cnt[u] += 1ull << (16 * cls);
            }
        }
    }
    // points, finite, SEEN_THROUGH, KEEP, UNTESTED among the finite, pairs THROUGH, AGREE, OCCLUDED, EMPTY
    unsigned int sum[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const long long i = i0 + u * kCvisThreads;
        if (i >= J.n) continue;
        const size_t at = J.order ? (size_t)J.order[i] : (size_t)i;
        const bool finite = (fin >> u) & 1u;
        const unsigned int n_through = (unsigned int)(cnt[u] & 0xFFFFull), n_agree = (unsigned int)((cnt[u] >> 16) & 0xFFFFull);
        uint8_t verdict = SCVOD_VIS_UNTESTED;
        if (cnt[u] != 0ull)
            verdict = ((int)n_through >= J.V.min_through &&
                       (long long)n_through * J.V.vote_den >= (long long)J.V.vote_num * (long long)(n_through + n_agree))
                          ? SCVOD_VIS_SEEN_THROUGH
                          : SCVOD_VIS_KEEP;
        if (J.votes) reinterpret_cast<unsigned long long*>(J.votes)[at] = cnt[u];  // little endian: {n_through, n_agree, n_occluded, n_empty}
        if (J.verdict) J.verdict[at] = verdict;
        sum[0] += 1u;
        sum[1] += finite ? 1u : 0u;
        sum[2] += verdict == SCVOD_VIS_SEEN_THROUGH ? 1u : 0u;
        sum[3] += verdict == SCVOD_VIS_KEEP ? 1u : 0u;
        sum[4] += finite && verdict == SCVOD_VIS_UNTESTED ? 1u : 0u;
        sum[5] += n_through;
        sum[6] += n_agree;
        sum[7] += (unsigned int)((cnt[u] >> 32) & 0xFFFFull);
        sum[8] += (unsigned int)(cnt[u] >> 48);
    }
    // (8 records x 65535 scans per thread, at most 256 threads: a block's sum stays below 2^32)
#pragma unroll
    for (int f = 0; f < 9; ++f) {
        unsigned int v = sum[f];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        if (lane == 0) wcnt[w][f] = v;
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        unsigned long long v = steps;
        if (threadIdx.x < 9) {
            v = 0ull;
#pragma unroll
            for (int k = 0; k < NW; ++k) v += wcnt[k][threadIdx.x];
        }
        if (v) atomicAdd(&J.counters[threadIdx.x], v);
    }
}

}  // namespace

size_t cvis_sort_bytes(long long n) {
    size_t bytes = 0;
    rocprim::radix_sort_pairs(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n,
                              0, kCvisKeyBits, (hipStream_t)0);
    return bytes;
}

void launch_cvis_key(const float4* pts, long long n, uint32_t* key, uint32_t* idx, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_cvis_key, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pts, n, key, idx);
}

hipError_t launch_cvis_sort(void* tmp, size_t tmp_bytes, const uint32_t* key_in, uint32_t* key_out, const uint32_t* idx_in, uint32_t* idx_out,
                            long long n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, key_in, key_out, idx_in, idx_out, (size_t)n, 0, kCvisKeyBits, st);
}

void launch_cvis_vote(const CvisJob& J, hipStream_t st) {
    if (J.n <= 0) return;
    hipLaunchKernelGGL(k_cvis_vote, dim3((unsigned)((J.n + kCvisChunk - 1) / kCvisChunk)), dim3(kCvisThreads), 0, st, J);
}

int cvis_check_params(const scvod_cloud_visibility_params* p) {
    if (!p) return SCVOD_ERR_INVALID;
    if (p->halo < 0 || p->halo > 1 || p->reserved != 0) return SCVOD_ERR_INVALID;
    if (p->vote_den < 1 || p->vote_den > (1 << 20) || p->vote_num < 0 || p->vote_num > (1 << 20)) return SCVOD_ERR_INVALID;
    for (const float v : {p->gap_abs, p->gap_rel, p->max_range})
        if (!(v >= 0.f) || !std::isfinite(v)) return SCVOD_ERR_INVALID;
    return SCVOD_OK;
}

}  // namespace scvod

extern "C" {

void scvod_cloud_visibility_params_default(scvod_cloud_visibility_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->halo = 0;
    p->gap_abs = 0.4f;
    p->gap_rel = 0.02f;
    p->max_range = 0.f;
    p->min_through = 2;
    p->vote_num = 1;
    p->vote_den = 2;
}

}  // extern "C"
