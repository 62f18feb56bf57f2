// scvod_export.hip -- the result of a batch handed to the next consumer on the device (gfx950): one label byte per INPUT point
// (scvod_batch_point_labels; scvod_batch_point_classes with the building / tree split) and the kept points of every scan, compacted in
// input order (scvod_batch_export_points).
//
// Reference analogue: the `static_pt` / `dynamic_pt` lists of SSC::saveSegCloud mode 3 (ssc.cpp:477-554) and the clouds of the
// evaluation block (`cloud_eva_static`, `g_cloud_vec`, the _static / _dynamic / _original .pcd files, ssc.cpp:1454-1540).  The
// reference builds them by appending cluster clouds on one thread; here every array they are made of is in the arena, or is put
// there by one pass before the first of these calls (ground_idx / rejected_src of a lean batch: ensure_lists, scvod_capi.hip):
//     ground_idx / rejected_src / apri_src   which cloud an input point went to (a point in none of them was dropped by Patchwork)
//     pt_type                                the segmentation's type of an apri point's cluster (0 erased, 1 other, 2 car)
//     pt_dyn                                 what scvod_batch_track decided for it
// Labels: the buffer is cleared to DROPPED, then the three lists are scattered through their source indices.  Compaction: three
// passes over tiles of kExpTile points that never cross a scan -- count (ballot / popcount of the keep bit), exclusive scan (per scan
// over its tiles, then one workgroup over the scans: separate launches, no workgroup ever waits for another), write (the ballots
// are computed again, a point's slot is its tile's prefix + the kept points of the rounds and waves before it + its rank in the wave).
// The order is the input order, so the output is the same bit for bit on every run.
#include <hip/hip_runtime.h>

#include "scvod_dev.h"

namespace scvod {
namespace {

// what an apri point's type and tracking byte say (include/scvod.h, SCVOD_PT_*)
__device__ __forceinline__ uint8_t exp_label_of(uint8_t type, uint8_t dyn, int use_dyn) {
    if (use_dyn && dyn == SCVOD_DYN_DYNAMIC) return SCVOD_PT_DYNAMIC;
    return type == 0 ? SCVOD_PT_UNCLUSTERED : (type == 2 ? SCVOD_PT_STATIC_CAR : SCVOD_PT_STATIC_OTHER);
}

// the three lists of scan blockIdx.y, scattered to the input points they name: apri order first (type and tracking byte), then
// cloud_out, then the range/FOV rejects.  The lists are disjoint, so the stores never meet; an index outside the scan is not followed.
__global__ __launch_bounds__(256) void k_exp_labels(Arena A, uint8_t* __restrict__ labels, int use_dyn) {
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int n = A.scan_off[s + 1] - base;
    const int n_g = A.counts[s * 8 + 1], n_a = A.counts[s * 8 + 4], n_r = A.counts[s * 8 + 5];
    const int total = n_a + n_g + n_r;
    constexpr int U = 4;  // list entries per thread in flight: index -> byte store is two dependent accesses deep
    for (int t0 = blockIdx.x * (256 * U) + threadIdx.x; t0 < total; t0 += gridDim.x * (256 * U)) {
        int idx[U];
        uint8_t lab[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + u * 256;
            idx[u] = -1;
            lab[u] = SCVOD_PT_DROPPED;
            if (t < n_a) {
                idx[u] = A.apri_src[(size_t)base + t];
                lab[u] = exp_label_of(A.pt_type[(size_t)base + t], use_dyn ? A.pt_dyn[(size_t)base + t] : (uint8_t)0, use_dyn);
            } else if (t < n_a + n_g) {
                idx[u] = A.ground_idx[(size_t)base + (t - n_a)];
                lab[u] = SCVOD_PT_GROUND;
            } else if (t < total) {
                idx[u] = A.rejected_src[(size_t)base + (t - n_a - n_g)];
                lab[u] = SCVOD_PT_REJECTED;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if ((unsigned)idx[u] < (unsigned)n) labels[(size_t)base + idx[u]] = lab[u];
    }
}

// k_exp_labels with the region growing's split carried into the byte (scvod_batch_point_classes): the same three lists, and per apri
// point one more byte -- cls, the class of its cluster (3: building).  A point that would be STATIC_OTHER becomes STATIC_BUILDING there.
__global__ __launch_bounds__(256) void k_exp_classes(Arena A, const uint8_t* __restrict__ cls, uint8_t* __restrict__ labels, int use_dyn) {
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int n = A.scan_off[s + 1] - base;
    const int n_g = A.counts[s * 8 + 1], n_a = A.counts[s * 8 + 4], n_r = A.counts[s * 8 + 5];
    const int total = n_a + n_g + n_r;
    constexpr int U = 4;
    for (int t0 = blockIdx.x * (256 * U) + threadIdx.x; t0 < total; t0 += gridDim.x * (256 * U)) {
        int idx[U];
        uint8_t lab[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + u * 256;
            idx[u] = -1;
            lab[u] = SCVOD_PT_DROPPED;
            if (t < n_a) {
                idx[u] = A.apri_src[(size_t)base + t];
                lab[u] = exp_label_of(A.pt_type[(size_t)base + t], use_dyn ? A.pt_dyn[(size_t)base + t] : (uint8_t)0, use_dyn);
                if (lab[u] == SCVOD_PT_STATIC_OTHER && cls[(size_t)base + t] == 3) lab[u] = SCVOD_PT_STATIC_BUILDING;
            } else if (t < n_a + n_g) {
                idx[u] = A.ground_idx[(size_t)base + (t - n_a)];
                lab[u] = SCVOD_PT_GROUND;
            } else if (t < total) {
                idx[u] = A.rejected_src[(size_t)base + (t - n_a - n_g)];
                lab[u] = SCVOD_PT_REJECTED;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if ((unsigned)idx[u] < (unsigned)n) labels[(size_t)base + idx[u]] = lab[u];
    }
}

// kept points of tile blockIdx.x of scan blockIdx.y
__global__ __launch_bounds__(256) void k_exp_count(Arena A, ExportJob J) {
    __shared__ int wcnt[4];
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int n = A.scan_off[s + 1] - base;
    const int i0 = blockIdx.x * kExpTile;
    int c = 0;
    if (i0 < n) {
        uint8_t lab[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) lab[u] = J.labels[(size_t)base + min(i0 + u * 256 + (int)threadIdx.x, n - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool keep = (i0 + u * 256 + (int)threadIdx.x < n) && ((J.keep_mask >> lab[u]) & 1u);
            c += __popcll(__ballot(keep));
        }
    }
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) J.tile_cnt[(size_t)s * J.tiles_per_scan + blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// per scan: its tiles' counts -> exclusive prefix inside the scan, and the scan's total (a scan has at most
// SCVOD_MAX_SCAN_POINTS / kExpTile = 256 tiles: one round of one workgroup)
__global__ __launch_bounds__(256) void k_exp_scan_tiles(ExportJob J) {
    __shared__ int wsum[5];
    const int s = blockIdx.x;
    int32_t* cnt = J.tile_cnt + (size_t)s * J.tiles_per_scan;
    const int v = (int)threadIdx.x < J.tiles_per_scan ? cnt[threadIdx.x] : 0;
    int total;
    const int ex = block_excl_scan<256>(v, total, wsum);
    if ((int)threadIdx.x < J.tiles_per_scan) cnt[threadIdx.x] = ex;
    if (threadIdx.x == 0) J.scan_cnt[s] = total;
}

// one workgroup: the scans' totals -> the caller's offsets; the sizes and the overflow latch
__global__ __launch_bounds__(1024) void k_exp_scan_scans(int n_scans, ExportJob J) {
    __shared__ int wsum[17];
    long long carry = 0;
    for (int b = 0; b < n_scans; b += 1024) {
        const int i = b + (int)threadIdx.x;
        const int v = i < n_scans ? J.scan_cnt[i] : 0;
        int total;
        const int ex = block_excl_scan<1024>(v, total, wsum);
        if (i < n_scans) J.out_off[i] = (int32_t)(carry + ex);
        carry += total;
    }
    if (threadIdx.x == 0) {
        J.out_off[n_scans] = (int32_t)carry;
        J.stats[0] = J.out ? (carry < J.cap ? carry : J.cap) : 0;
        J.stats[1] = carry;
        J.stats[2] = (J.out && carry > J.cap) ? 1 : 0;
        J.stats[3] = 0;
    }
}

// the kept points of tile blockIdx.x of scan blockIdx.y into their slots.  The scan is streamed once in input order: 16-byte
// non-temporal loads (as k_map_accumulate reads it), float4 stores; nothing is written at or behind slot J.cap.
__global__ __launch_bounds__(256) void k_exp_write(Arena A, ExportJob J) {
    __shared__ int wcnt[32];  // [round][wave] kept points, then their exclusive prefix in (round, wave) order
    const int s = blockIdx.y;
    const int base = A.scan_off[s];
    const int n = A.scan_off[s + 1] - base;
    const int i0 = blockIdx.x * kExpTile;
    if (i0 >= n) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint8_t lab[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) lab[u] = __builtin_nontemporal_load(&J.labels[(size_t)base + min(i0 + u * 256 + (int)threadIdx.x, n - 1)]);
    bool keep[8];
    int rank[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        keep[u] = (i0 + u * 256 + (int)threadIdx.x < n) && ((J.keep_mask >> lab[u]) & 1u);
        const unsigned long long bal = __ballot(keep[u]);
        rank[u] = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[u * 4 + w] = __popcll(bal);
    }
    __syncthreads();
    if (w == 0) {
        const int v = lane < 32 ? wcnt[lane] : 0;
        const int inc = wave_incl_scan(v);
        if (lane < 32) wcnt[lane] = inc - v;
    }
    __syncthreads();
    const long long tile_base = (long long)J.out_off[s] + J.tile_cnt[(size_t)s * J.tiles_per_scan + blockIdx.x];
    typedef float f4v __attribute__((ext_vector_type(4)));
    f4v q[8];
    uint32_t pay[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const size_t g = (size_t)base + i0 + u * 256 + threadIdx.x;
        keep[u] = keep[u] && (tile_base + wcnt[u * 4 + w] + rank[u] < J.cap);
        q[u] = f4v{0.f, 0.f, 0.f, 0.f};
        pay[u] = 0u;
        if (keep[u]) {
            q[u] = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(&A.pts[g]));
            if (J.payload_in && J.payload_out) pay[u] = __builtin_nontemporal_load(&J.payload_in[g]);
        }
    }
    float T[12];
    if (J.pose) {
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = J.pose[12 * (size_t)s + i];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (!keep[u]) continue;
        const long long o = tile_base + wcnt[u * 4 + w] + rank[u];
        float4 r = make_float4(q[u].x, q[u].y, q[u].z, q[u].w);
        if (J.pose) {  // the map kernel's expression (Utility::transformCloud, utility.h:400-405): left to right, no contraction
            r.x = T[0] * q[u].x + T[1] * q[u].y + T[2] * q[u].z + T[3];
            r.y = T[4] * q[u].x + T[5] * q[u].y + T[6] * q[u].z + T[7];
            r.z = T[8] * q[u].x + T[9] * q[u].y + T[10] * q[u].z + T[11];
        }
        J.out[o] = r;
        if (J.src_out) J.src_out[o] = i0 + u * 256 + (int)threadIdx.x;
        if (J.payload_in && J.payload_out) J.payload_out[o] = pay[u];
    }
}

}  // namespace

void launch_point_labels(const Arena& A, uint8_t* labels, int use_dyn, hipStream_t st) {
    if (A.max_scan_pts <= 0) return;
    hipLaunchKernelGGL(k_exp_labels, dim3((A.max_scan_pts + 2047) / 2048, A.n_scans), dim3(256), 0, st, A, labels, use_dyn);
}

void launch_point_classes(const Arena& A, const uint8_t* cls, uint8_t* labels, int use_dyn, hipStream_t st) {
    if (A.max_scan_pts <= 0) return;
    hipLaunchKernelGGL(k_exp_classes, dim3((A.max_scan_pts + 2047) / 2048, A.n_scans), dim3(256), 0, st, A, cls, labels, use_dyn);
}

void launch_export(const Arena& A, const ExportJob& J, hipStream_t st) {
    const dim3 grid(J.tiles_per_scan > 0 ? J.tiles_per_scan : 1, A.n_scans);
    if (J.tiles_per_scan > 0) hipLaunchKernelGGL(k_exp_count, grid, dim3(256), 0, st, A, J);
    hipLaunchKernelGGL(k_exp_scan_tiles, dim3(A.n_scans), dim3(256), 0, st, J);
    hipLaunchKernelGGL(k_exp_scan_scans, dim3(1), dim3(1024), 0, st, A.n_scans, J);
    if (J.tiles_per_scan > 0 && J.out) hipLaunchKernelGGL(k_exp_write, grid, dim3(256), 0, st, A, J);
}

}  // namespace scvod
