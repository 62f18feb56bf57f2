// scvod_stack.hip -- neighbouring scans stacked into the middle scan's frame (gfx950): the kernel of scvod_batch_stack_scans and the
// two host-only functions of the stage (scvod_stack_offsets, scvod_pose_from_matrix).
//
// Reference analogue: src/makeScan.cpp:153-244.  Per group of `window` consecutive scans the reference loads the clouds, moves the
// first and the third into the frame of the second (trans_2.inverse() * trans_k, transformCloud of makeScan.cpp:76-88) and appends
// them to the second, which it never touches.  Here every (group, scan of its window) pair is a segment of the host-built table: a
// contiguous run of input records that goes to a contiguous run of output records with one matrix, or with none.  The host also lists
// the tiles of the non-empty segments, so a workgroup owns kStackTile records of ONE segment: the matrix, both base addresses and the
// "copy only" decision are uniform over the workgroup (scalar loads, scalar registers, a uniform branch), an empty segment launches
// nothing, and no workgroup searches, counts or waits for anything.  One streaming pass: 16 bytes in, 16 bytes out per point, a lane
// per record (1 KiB per wave instruction), eight independent loads in flight per lane.
#include <hip/hip_runtime.h>

#include <cmath>

#include "scvod_dev.h"

namespace scvod {
namespace {

__global__ __launch_bounds__(256) void k_stack_tiles(const StackSeg* __restrict__ segs, const StackTile* __restrict__ tiles,
                                                      const float4* __restrict__ in, float4* __restrict__ out,
                                                      const uint32_t* __restrict__ payload_in, uint32_t* __restrict__ payload_out,
                                                      int32_t* __restrict__ src_out) {
    const StackTile t = tiles[blockIdx.x];
    const StackSeg* S = &segs[t.seg];
    const int n = S->n, copy = S->copy;
    const size_t in0 = (size_t)S->in_base, out0 = (size_t)S->out_base;
    const int i0 = t.first + (int)threadIdx.x;
    typedef float f4v __attribute__((ext_vector_type(4)));
    f4v q[8];
    uint32_t pay[8];
    // the input is read once: non-temporal loads, as k_exp_write and k_map_accumulate read a scan
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * 256;
        q[u] = f4v{0.f, 0.f, 0.f, 0.f};
        pay[u] = 0u;
        if (i < n) {
            q[u] = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(&in[in0 + i]));
            if (payload_out) pay[u] = __builtin_nontemporal_load(&payload_in[in0 + i]);
        }
    }
    if (!copy) {
        float T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = S->T[k];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            // the map kernel's expression (transformCloud, makeScan.cpp:83-85): left to right in fp32, no contraction
            const float x = T[0] * q[u].x + T[1] * q[u].y + T[2] * q[u].z + T[3];
            const float y = T[4] * q[u].x + T[5] * q[u].y + T[6] * q[u].z + T[7];
            const float z = T[8] * q[u].x + T[9] * q[u].y + T[10] * q[u].z + T[11];
            q[u].x = x;
            q[u].y = y;
            q[u].z = z;
        }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * 256;
        if (i < n) {
            *reinterpret_cast<f4v*>(&out[out0 + i]) = q[u];
            if (payload_out) payload_out[out0 + i] = pay[u];
            if (src_out) src_out[out0 + i] = (int32_t)(in0 + i);
        }
    }
}

}  // namespace

void launch_stack(const StackSeg* segs, const StackTile* tiles, int n_tiles, const float4* in, float4* out, const uint32_t* payload_in,
                  uint32_t* payload_out, int32_t* src_out, hipStream_t st) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(k_stack_tiles, dim3(n_tiles), dim3(256), 0, st, segs, tiles, in, out, payload_in, payload_out, src_out);
}

}  // namespace scvod

extern "C" {

int scvod_stack_offsets(const int32_t* h_in_offsets, int32_t n_in, int32_t window, int32_t interval, int32_t flags,
                        int32_t* h_out_offsets, int32_t* h_mid, int32_t cap_out, int32_t* largest_scan) {
    if (window < 1 || window > SCVOD_STACK_MAX_WINDOW || !(window & 1) || interval < 1 || (flags & ~SCVOD_STACK_REFERENCE_BOUND) || n_in < 0)
        return SCVOD_ERR_INVALID;
    const bool sizes = h_out_offsets || largest_scan;
    if (sizes && !h_in_offsets) return SCVOD_ERR_INVALID;
    if (h_in_offsets)
        for (int k = 0; k < n_in; ++k)
            if (h_in_offsets[k + 1] < h_in_offsets[k]) return SCVOD_ERR_INVALID;
    // group g exists iff its window fits; the reference's loop (makeScan.cpp:156) also wants g * interval < n_in - interval
    long long n_out = 0;
    if (n_in >= window) {
        n_out = ((long long)n_in - window) / interval + 1;
        if (flags & SCVOD_STACK_REFERENCE_BOUND) {
            const long long lim = (long long)n_in - interval;  // first scans below lim
            const long long by_bound = lim > 0 ? (lim + interval - 1) / interval : 0;
            if (by_bound < n_out) n_out = by_bound;
        }
    }
    if ((h_out_offsets || h_mid) && n_out > cap_out) return SCVOD_ERR_CAPACITY;
    long long run = 0, largest = 0;
    if (h_out_offsets) h_out_offsets[0] = 0;
    for (long long g = 0; g < n_out; ++g) {
        const long long first = g * interval;
        if (h_mid) h_mid[g] = (int32_t)(first + window / 2);
        if (sizes) {
            const long long pts = (long long)h_in_offsets[first + window] - (long long)h_in_offsets[first];
            run += pts;
            if (run > 2147483647ll) return SCVOD_ERR_CAPACITY;
            if (pts > largest) largest = pts;
            if (h_out_offsets) h_out_offsets[g + 1] = (int32_t)run;
        }
    }
    if (largest_scan) *largest_scan = (int32_t)largest;
    return (int)n_out;
}

void scvod_pose_from_matrix(const float M[12], float pose_out[6]) {
    if (!M || !pose_out) return;
    // makeScan.cpp:57-74: R(i, j) = M[4 * i + j]; sqrt / atan2 on floats are the float overloads; `sy < 1e-6` compares in double
    const float sy = std::sqrt(M[0] * M[0] + M[4] * M[4]);
    const bool singular = sy < 1e-6;
    float x, y, z;
    if (!singular) {
        x = std::atan2(M[9], M[10]);
        y = std::atan2(-M[8], sy);
        z = std::atan2(M[4], M[0]);
    } else {
        x = std::atan2(-M[6], M[5]);
        y = std::atan2(-M[8], sy);
        z = 0;
    }
    pose_out[0] = M[3];
    pose_out[1] = M[7];
    pose_out[2] = M[11];
    pose_out[3] = x;
    pose_out[4] = y;
    pose_out[5] = z;
}

}  // extern "C"
