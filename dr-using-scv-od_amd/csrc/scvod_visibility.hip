// scvod_visibility.hip -- seen-through points: the range-image vote of neighbouring scans (gfx950).  The kernels of
// scvod_visibility_device / scvod_batch_visibility and the host-only functions of the stage (defaults, parameter check, viewer lists).
//
// Reference analogue: none (include/scvod.h, DESIGN.md section 2: this project's convention).  SSC::tracking decides "dynamic" for
// car-typed clusters only; here every point of a scan is looked at from the scans around it: the point is moved into a viewer's frame,
// binned with SSC::makeApriVec's arithmetic, and compared with the nearest return the viewer measured in that direction.
//
// k_vis_image   one pass over every scan: the minimum `dis` per (azimuth, sector) pixel, an integer atomicMin on the float's bits
//               (dis >= 0: the bits order as the values do), so the image does not depend on the order of the points; runs of
//               consecutive lanes with one pixel are reduced in the wave first, and a value that lowers nothing is not sent
// k_vis_vote    a workgroup owns one 2048-point tile of ONE scan and keeps its 8 records per thread in registers over the loop of that
//               scan's viewers; matrix and image base are scalar per viewer, the gathers hit an image of 4 A S bytes that stays in L2
// Both take the host's tile table (k_stack_tiles' scheme): an empty scan launches nothing, no workgroup searches or waits for another.
// The only LDS are the 24 counter words of a workgroup (the evaluation's scheme: per wave, LDS per block, one 64-bit atomicAdd per
// counter and block); every sum is an integer, so all outputs are the same on every run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "scvod_vispair.h"

namespace scvod {
namespace {

__global__ __launch_bounds__(256) void k_vis_image(VisJob J) {
    const StackTile t = J.tiles[blockIdx.x];
    const VisScan sc = J.scans[t.seg];
    const int S = J.bin.sector_num, A = J.bin.azimuth_num;
    const int s = __builtin_amdgcn_readfirstlane(t.seg);
    unsigned int* img = reinterpret_cast<unsigned int*>(J.images + (size_t)s * (size_t)A * (size_t)S);
    const size_t base = (size_t)sc.base;
    const int n = sc.n, i0 = t.first + (int)threadIdx.x;
    float4 q[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * 256;
        q[u] = make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f);
        if (i < n) q[u] = J.pts[base + i];
    }
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        int32_t px = -1;  // the record's pixel, -1: it has none (a record past the scan's end is NaN)
        unsigned int bits = 0u;
        if (vis_finite(q[u].x, q[u].y, q[u].z)) {
            float dis;
            int32_t si, ai;
            if (vis_bin(J, q[u].x, q[u].y, q[u].z, &dis, &si, &ai) && si >= 0 && si < S && ai >= 0 && ai < A) {
                px = ai * S + si;
                bits = __float_as_uint(dis);
            }
        }
        // a sensor writes a ring in order: consecutive records share a pixel.  A segmented minimum over the runs of equal pixels among
        // consecutive lanes, and only the last lane of a run goes to memory -- and only when it would lower what the pixel holds (a
        // stale read is a larger value: the atomic is issued needlessly, never skipped wrongly)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t opx = __shfl_up(px, d, 64);
            const unsigned int ob = __shfl_up(bits, d, 64);
            if (lane >= d && opx == px && ob < bits) bits = ob;
        }
        const int32_t npx = __shfl_down(px, 1, 64);
        if (px >= 0 && (lane == 63 || npx != px) && bits < img[px]) atomicMin(&img[px], bits);
    }
}

__global__ __launch_bounds__(256) void k_vis_vote(VisJob J) {
    __shared__ unsigned int wcnt[4][6];
    const StackTile t = J.tiles[blockIdx.x];
    const VisScan sc = J.scans[t.seg];
    const int S = J.bin.sector_num, A = J.bin.azimuth_num;
    const int s = __builtin_amdgcn_readfirstlane(t.seg);
    const int pair_begin = __builtin_amdgcn_readfirstlane(sc.pair_begin), n_pairs = __builtin_amdgcn_readfirstlane(sc.n_pairs);
    const size_t base = (size_t)sc.base;
    const int n = sc.n, i0 = t.first + (int)threadIdx.x;
    const size_t img_words = (size_t)A * (size_t)S;
    float qx[8], qy[8], qz[8];
    unsigned int cnt[8];
    unsigned int is_q = 0;  // bit u: record u of this thread is a query
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * 256;
        qx[u] = qy[u] = qz[u] = 0.f;
        cnt[u] = 0u;
        if (i < n) {
            const float4 q = J.pts[base + i];
            qx[u] = q.x;
            qy[u] = q.y;
            qz[u] = q.z;
            if (!J.mask || J.mask[base + i]) is_q |= 1u << u;
        }
    }
    for (int v = 0; v < n_pairs; ++v) {
        const VisPair* P = &J.pairs[pair_begin + v];
        float T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(P->T[k])));
        const float* __restrict__ img = J.images + (size_t)__builtin_amdgcn_readfirstlane(P->viewer) * img_words;
#pragma unroll 2
        for (int u = 0; u < 8; ++u) {
            if (!((is_q >> u) & 1u)) continue;
            // the map kernel's expression: left to right in fp32, no contraction
            const float x = T[0] * qx[u] + T[1] * qy[u] + T[2] * qz[u] + T[3];
            const float y = T[4] * qx[u] + T[5] * qy[u] + T[6] * qz[u] + T[7];
            const float z = T[8] * qx[u] + T[9] * qy[u] + T[10] * qz[u] + T[11];
            cnt[u] += 1u << (8 * vis_pair(J, img, A, S, x, y, z));
        }
    }
    unsigned int sum[6] = {0u, 0u, 0u, 0u, 0u, 0u};  // queries, SEEN_THROUGH, pairs THROUGH, AGREE, OCCLUDED, OUTSIDE + EMPTY
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * 256;
        if (i >= n) continue;
        const bool query = (is_q >> u) & 1u;
        const int n_through = (int)(cnt[u] & 255u), n_agree = (int)((cnt[u] >> 8) & 255u);
        uint8_t verdict = SCVOD_VIS_UNTESTED;
        if (query && n_pairs > 0)
            verdict = (n_through >= J.min_through && n_through * J.vote_den >= J.vote_num * (n_through + n_agree)) ? SCVOD_VIS_SEEN_THROUGH
                                                                                                                 : SCVOD_VIS_KEEP;
        if (J.votes) J.votes[base + i] = cnt[u];
        if (J.verdict) J.verdict[base + i] = verdict;
        sum[0] += query ? 1u : 0u;
        sum[1] += verdict == SCVOD_VIS_SEEN_THROUGH ? 1u : 0u;
        sum[2] += cnt[u] & 255u;
        sum[3] += (cnt[u] >> 8) & 255u;
        sum[4] += (cnt[u] >> 16) & 255u;
        sum[5] += cnt[u] >> 24;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        unsigned int c = sum[f];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
        if (lane == 0) wcnt[w][f] = c;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const unsigned long long c = (unsigned long long)wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
        if (c) {
            atomicAdd(&J.counters[threadIdx.x], c);
            if (J.scan_counts) atomicAdd(&J.scan_counts[6 * (size_t)s + threadIdx.x], c);
        }
    }
}

__global__ __launch_bounds__(256) void k_vis_mask(Arena A, uint8_t* __restrict__ mask) {
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int n_ng = A.counts[s * 8 + 2];
    for (int t = blockIdx.x * 256 + threadIdx.x; t < n_ng; t += gridDim.x * 256) mask[(size_t)base + A.nonground_idx[(size_t)base + t]] = 1;
}

}  // namespace

void launch_vis_image(const VisJob& J, hipStream_t st) {
    if (J.n_tiles <= 0) return;
    hipLaunchKernelGGL(k_vis_image, dim3(J.n_tiles), dim3(256), 0, st, J);
}

void launch_vis_vote(const VisJob& J, hipStream_t st) {
    if (J.n_tiles <= 0) return;
    hipLaunchKernelGGL(k_vis_vote, dim3(J.n_tiles), dim3(256), 0, st, J);
}

void launch_vis_mask(const Arena& A, uint8_t* mask, hipStream_t st) {
    if (A.n_scans <= 0 || A.max_scan_pts <= 0) return;
    hipLaunchKernelGGL(k_vis_mask, dim3((A.max_scan_pts + 2047) / 2048, A.n_scans), dim3(256), 0, st, A, mask);
}

int vis_check_params(const scvod_visibility_params* p) {
    if (!p) return SCVOD_ERR_INVALID;
    if (p->before < 0 || p->before > SCVOD_VIS_MAX_WINDOW || p->after < 0 || p->after > SCVOD_VIS_MAX_WINDOW || (p->before == 0 && p->after == 0))
        return SCVOD_ERR_INVALID;
    if (p->halo < 0 || p->halo > 1) return SCVOD_ERR_INVALID;
    if (p->vote_den < 1 || p->vote_den > (1 << 20) || p->vote_num < 0 || p->vote_num > (1 << 20)) return SCVOD_ERR_INVALID;
    if (!(p->gap_abs >= 0.f) || !std::isfinite(p->gap_abs) || !(p->gap_rel >= 0.f) || !std::isfinite(p->gap_rel)) return SCVOD_ERR_INVALID;
    return SCVOD_OK;
}

int vis_viewers(const int32_t* h_next_scan, int n_scans, int before, int after, std::vector<int32_t>& begin, std::vector<int32_t>& viewers) {
    if (n_scans < 0 || before < 0 || before > SCVOD_VIS_MAX_WINDOW || after < 0 || after > SCVOD_VIS_MAX_WINDOW || (before == 0 && after == 0))
        return SCVOD_ERR_INVALID;
    std::vector<int32_t> next((size_t)n_scans), prev((size_t)n_scans, -1);
    for (int s = 0; s < n_scans; ++s) {
        const int32_t v = h_next_scan ? h_next_scan[s] : (s + 1 < n_scans ? s + 1 : -1);
        if (v >= n_scans || v == s) return SCVOD_ERR_INVALID;
        next[s] = v < 0 ? -1 : v;  // (-1: none; <= -2: an external table of scvod_batch_track, no scan of this batch)
        if (v >= 0) {
            if (prev[v] >= 0) return SCVOD_ERR_INVALID;  // two scans name one successor
            prev[v] = s;
        }
    }
    // every scan hangs on a chain that starts at a scan nobody names: what is left over is a ring
    int reached = 0;
    for (int s = 0; s < n_scans; ++s)
        if (prev[s] < 0)
            for (int k = s; k >= 0; k = next[k]) ++reached;
    if (reached != n_scans) return SCVOD_ERR_INVALID;
    begin.assign((size_t)n_scans + 1, 0);
    viewers.clear();
    for (int j = 0; j < n_scans; ++j) {
        int k = j;
        for (int a = 0; a < after && next[k] >= 0; ++a) viewers.push_back(k = next[k]);
        k = j;
        for (int b = 0; b < before && prev[k] >= 0; ++b) viewers.push_back(k = prev[k]);
        begin[(size_t)j + 1] = (int32_t)viewers.size();
    }
    return SCVOD_OK;
}

}  // namespace scvod

extern "C" {

void scvod_visibility_params_default(scvod_visibility_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->before = p->after = 2;
    p->halo = 0;
    p->gap_abs = 0.4f;
    p->gap_rel = 0.02f;
    p->min_through = 2;
    p->vote_num = 1;
    p->vote_den = 2;
}

int scvod_visibility_viewers(const int32_t* h_next_scan, int32_t n_scans, int32_t before, int32_t after, int32_t* h_begin, int32_t* h_viewers,
                             int32_t cap) {
    std::vector<int32_t> begin, viewers;
    if (int rc = scvod::vis_viewers(h_next_scan, n_scans, before, after, begin, viewers)) return rc;
    if (viewers.size() > 2147483647ull) return SCVOD_ERR_CAPACITY;
    if (h_viewers && (long long)viewers.size() > (long long)cap) return SCVOD_ERR_CAPACITY;
    if (h_begin) memcpy(h_begin, begin.data(), sizeof(int32_t) * begin.size());
    if (h_viewers && !viewers.empty()) memcpy(h_viewers, viewers.data(), sizeof(int32_t) * viewers.size());
    return (int)viewers.size();
}

}  // extern "C"
