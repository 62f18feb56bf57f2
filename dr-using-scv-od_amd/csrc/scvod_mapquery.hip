// scvod_mapquery.hip -- asking the static map: the cell of a point and the nearest representative around it (gfx950).
//
// The map (scvod_map.hip) is an open-addressing table of occupied cells with one measured point per cell.  A query moves a point to the
// world frame with k_map_accumulate's expression, takes the key map_encode gives it and walks the probe chain insertion walks: the key
// is present iff it is met from its home slot before an empty slot and within kMapMaxProbes slots.  With a radius (at most 0.99 cells)
// the representatives of the 27 cells around the own cell are the candidates of a nearest-point search; every number is fp32, rounded
// operation by operation, so the answer is a function of the table's contents and the point alone.
// Nothing here writes the table, and the counters are an allocation of the query's own.
// The probe itself (chain walk, select test, own cell, the 27 cells) is scvod_mapprobe.h, shared with the filter.
#include "scvod_mapprobe.h"

using namespace scvod;

namespace scvod {
namespace {

// MODE 0: radius == 0, the own cell only.  MODE 1: a radius, but no nn output: a point whose own cell is occupied is finished after the
// own-cell pass.  MODE 2: a radius and the nn pair: every point with a cell looks at its 27 cells.
//
// Own-cell pass: k_map_accumulate's shape (256 threads, one point per thread and round, kMapPts points per workgroup, scan blockIdx.y),
// non-temporal 16-byte loads of the stream and non-temporal stores of the outputs so that the table's lines keep the L2; runs of
// consecutive lanes with one key are found by ballot, the head of a run probes and the run takes the head's record by __shfl.  A point
// without a cell (key kEmpty) splits a run and probes nothing.
// Neighbour pass, MODE 2: in the round, every lane for its own point.  MODE 1: few points need it (on a map that holds the scene, the
// ones Patchwork dropped and what is new), scattered over many waves, and a wave pays the 26 dependent loads for one lane as for 64;
// so each wave queues its points without an own cell in LDS and looks at their neighbours 64 at a time, the rest at its end.  The
// queue is the wave's own: no barrier, the wave's LDS operations complete in order.
// Counters: ballot + popcount per wave into registers, LDS per block, one 64-bit atomicAdd per counter and block.
template <int MODE>
__global__ __launch_bounds__(256) void k_mq_query(int s_first, const float4* __restrict__ pts, const int32_t* __restrict__ scan_off,
                                                  const float* __restrict__ pose, const MapRec* __restrict__ table, unsigned long long mask, float inv_leaf,
                                                  float leaf, float radius, int sel, unsigned long long k0, unsigned long long k1, unsigned long long k2,
                                                  unsigned long long k3, uint8_t* __restrict__ out_result, unsigned long long* __restrict__ out_val,
                                                  unsigned long long* __restrict__ out_nn_key, float* __restrict__ out_nn_sq,
                                                  unsigned long long* scan_counts, unsigned long long* counters) {
    __shared__ unsigned int blk[4];
    __shared__ float4 q_pt[MODE == 1 ? 4 : 1][MODE == 1 ? kMqQueue : 1];              // x, y, z, the point's index in its scan
    __shared__ unsigned long long q_key[MODE == 1 ? 4 : 1][MODE == 1 ? kMqQueue : 1];
    const int s = s_first + blockIdx.y;
    const int base = scan_off[s];
    const int n = scan_off[s + 1] - base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 4) blk[threadIdx.x] = 0;
    __syncthreads();
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = pose[12 * s + i];
    const float r2 = radius * radius;
    unsigned int n_cell = 0, n_near = 0, n_miss = 0, n_out = 0;  // per wave (the same in every lane)
    int q_n = 0;                                                 // MODE 1: entries waiting in the wave's queue (the same in every lane)
    // MODE 1: the neighbours of queue entries [first, first + count), count <= 64, one per lane
    auto drain = [&](int first, int count) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const bool look = lane < count;
        const float4 e = q_pt[MODE == 1 ? wave : 0][MODE == 1 ? first + (look ? lane : 0) : 0];
        const unsigned long long key = look ? q_key[MODE == 1 ? wave : 0][MODE == 1 ? first + lane : 0] : kEmpty;
        unsigned long long best_key = kEmpty;
        float best_d = __builtin_inff();
        mq_neighbours(table, mask, leaf, radius, r2, sel, k0, k1, k2, k3, look, e.x, e.y, e.z, key, map_home(key, mask), false, kEmpty, best_key, best_d);
        const bool near = look && best_key != kEmpty;
        if (look && out_result)
            __builtin_nontemporal_store((uint8_t)(near ? SCVOD_MAPQ_NEAR : SCVOD_MAPQ_MISS), &out_result[(size_t)base + (size_t)__float_as_int(e.w)]);
        n_near += (unsigned int)__popcll(__ballot(near));
        n_miss += (unsigned int)__popcll(__ballot(look && !near));
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    };
    for (int i0 = blockIdx.x * 256; i0 < n; i0 += gridDim.x * 256) {
        const int i = i0 + (int)threadIdx.x;
        const size_t at = (size_t)base + (size_t)min(i, n - 1);
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v q = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(&pts[at]));
        const bool live = i < n;
        const float x = T[0] * q.x + T[1] * q.y + T[2] * q.z + T[3];
        const float y = T[4] * q.x + T[5] * q.y + T[6] * q.z + T[7];
        const float z = T[8] * q.x + T[9] * q.y + T[10] * q.z + T[11];
        unsigned long long key = kEmpty, unused = kEmpty;
        if (!live || !map_encode(x, y, z, 0.f, inv_leaf, key, unused)) key = kEmpty;
        // runs of equal keys among consecutive lanes: only the head probes
        unsigned long long h0, val;
        const bool found = mq_own_cell(table, mask, sel, k0, k1, k2, k3, lane, key, h0, val);
        const bool has_cell = key != kEmpty;

        unsigned long long best_key = kEmpty;
        float best_d = __builtin_inff();
        bool queued = false;
        if (MODE == 2) {
            mq_neighbours(table, mask, leaf, radius, r2, sel, k0, k1, k2, k3, has_cell, x, y, z, key, h0, found, val, best_key, best_d);
        } else if (MODE == 1) {
            queued = has_cell && !found;
            const unsigned long long qs = __ballot(queued);
            if (queued) {
                const int at_q = q_n + __popcll(qs & ((1ull << lane) - 1ull));
                q_pt[MODE == 1 ? wave : 0][MODE == 1 ? at_q : 0] = make_float4(x, y, z, __int_as_float(i));
                q_key[MODE == 1 ? wave : 0][MODE == 1 ? at_q : 0] = key;
            }
            q_n += __popcll(qs);
            if (q_n >= 64) {
                q_n -= 64;
                drain(q_n, 64);
            }
        }
        const bool near = MODE == 2 && has_cell && !found && best_key != kEmpty;
        if (live) {
            const size_t o = (size_t)base + (size_t)i;
            if (out_result && !queued)
                __builtin_nontemporal_store((uint8_t)(!has_cell ? SCVOD_MAPQ_OUT : (found ? SCVOD_MAPQ_CELL : (near ? SCVOD_MAPQ_NEAR : SCVOD_MAPQ_MISS))),
                                            &out_result[o]);
            if (out_val) __builtin_nontemporal_store(val, &out_val[o]);
            if (MODE == 2) {
                if (out_nn_key) __builtin_nontemporal_store(best_key, &out_nn_key[o]);
                if (out_nn_sq) __builtin_nontemporal_store(best_d, &out_nn_sq[o]);
            }
        }
        n_cell += (unsigned int)__popcll(__ballot(live && found));
        n_near += (unsigned int)__popcll(__ballot(live && near));
        n_miss += (unsigned int)__popcll(__ballot(live && has_cell && !found && !near && !queued));
        n_out += (unsigned int)__popcll(__ballot(live && !has_cell));
    }
    if (MODE == 1 && q_n > 0) drain(0, q_n);
    if (lane == 0) {
        if (n_cell) atomicAdd(&blk[0], n_cell);
        if (n_near) atomicAdd(&blk[1], n_near);
        if (n_miss) atomicAdd(&blk[2], n_miss);
        if (n_out) atomicAdd(&blk[3], n_out);
    }
    __syncthreads();
    if (threadIdx.x < 4 && blk[threadIdx.x]) {
        atomicAdd(&counters[threadIdx.x], (unsigned long long)blk[threadIdx.x]);
        if (scan_counts) atomicAdd(&scan_counts[4 * (size_t)s + threadIdx.x], (unsigned long long)blk[threadIdx.x]);
    }
}

struct MqArgs {
    float radius;
    const uint8_t* h_select256;
    uint8_t* d_result;
    uint64_t* d_cell_val;
    uint64_t* d_nn_key;
    float* d_nn_sqdist;
    int64_t* d_scan_counts;
};

// what both forms refuse before a device is touched
int mq_check(scvod_map* m, const MqArgs& a) {
    if (!(a.radius >= 0.f) || a.radius > 0.99f * m->leaf)
        return mfail(m, SCVOD_ERR_INVALID, "radius %g outside [0, 0.99 * leaf = %g]", (double)a.radius, (double)(0.99f * m->leaf));
    if (a.radius == 0.f && (a.d_nn_key || a.d_nn_sqdist)) return mfail(m, SCVOD_ERR_INVALID, "radius 0 probes the own cell only: d_nn_key and d_nn_sqdist must be NULL");
    if (a.h_select256 && m->kind != SCVOD_MAP_KIND_LABELLED) return mfail(m, SCVOD_ERR_INVALID, "a select table needs a map of kind SCVOD_MAP_KIND_LABELLED");
    return SCVOD_OK;
}

// scans [0, n_scans) of a cloud whose offsets and poses are on the device already; `points` = the cloud's size (for the stats)
int mq_launch(scvod_map* m, const void* d_xyzi, const int32_t* d_offs, int n_scans, int max_pts, long long points, const MqArgs& a, hipStream_t st) {
    if (!m->q_counters) MHIP(m, hipMalloc(&m->q_counters, 4 * sizeof(unsigned long long)));
    MHIP(m, hipMemsetAsync(m->q_counters, 0, 4 * sizeof(unsigned long long), st));
    if (a.d_scan_counts && n_scans > 0) MHIP(m, hipMemsetAsync(a.d_scan_counts, 0, 4 * sizeof(int64_t) * (size_t)n_scans, st));
    m->q_points = points;
    m->q_stream = st;
    m->q_ran = true;
    unsigned long long k[4];
    map_table256(a.h_select256, k);
    const int sel = a.h_select256 ? 1 : 0;
    const int mode = a.radius == 0.f ? 0 : ((a.d_nn_key || a.d_nn_sqdist) ? 2 : 1);
    constexpr int kMaxGridY = 65535;
    for (int s0 = 0; s0 < n_scans && max_pts > 0; s0 += kMaxGridY) {
        const int ny = n_scans - s0 < kMaxGridY ? n_scans - s0 : kMaxGridY;
        const dim3 grid((max_pts + kMapPts - 1) / kMapPts, ny), block(256);
#define MQ_LAUNCH(MODE)                                                                                                                          \
    hipLaunchKernelGGL(k_mq_query<MODE>, grid, block, 0, st, s0, (const float4*)d_xyzi, d_offs, m->d_pose, m->table,                              \
                       (unsigned long long)(m->capacity - 1), 1.0f / m->leaf, m->leaf, a.radius, sel, k[0], k[1], k[2], k[3], a.d_result,        \
                       (unsigned long long*)a.d_cell_val, (unsigned long long*)a.d_nn_key, a.d_nn_sqdist, (unsigned long long*)a.d_scan_counts, \
                       m->q_counters)
        if (mode == 0)
            MQ_LAUNCH(0);
        else if (mode == 1)
            MQ_LAUNCH(1);
        else
            MQ_LAUNCH(2);
#undef MQ_LAUNCH
        MHIP(m, hipGetLastError());
    }
    return SCVOD_OK;
}

}  // namespace
}  // namespace scvod

extern "C" {

int scvod_map_query(scvod_map* m, const void* d_xyzi, const int32_t* h_scan_offsets, int32_t n_scans, const float* h_poses, float radius,
                    const uint8_t* h_select256, uint8_t* d_result, uint64_t* d_cell_val, uint64_t* d_nn_key, float* d_nn_sqdist,
                    int64_t* d_scan_counts, void* stream) {
    if (!m || n_scans < 0 || (n_scans > 0 && !h_scan_offsets)) return mfail(m, SCVOD_ERR_INVALID, "bad arguments");
    const MqArgs a = {radius, h_select256, d_result, d_cell_val, d_nn_key, d_nn_sqdist, d_scan_counts};
    if (int rc = mq_check(m, a)) return rc;
    int max_pts = 0;
    if (n_scans > 0)
        if (int rc = map_check_offsets(m, h_scan_offsets, n_scans, &max_pts)) return rc;
    if (max_pts > 0 && !d_xyzi) return mfail(m, SCVOD_ERR_INVALID, "NULL points of a cloud that is not empty");
    if ((uintptr_t)d_xyzi & 15u) return mfail(m, SCVOD_ERR_INVALID, "d_xyzi is not 16-byte aligned");
    MHIP(m, hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)stream;
    if (max_pts > 0) {
        if (int rc = map_stage_poses(m, h_poses, n_scans, st)) return rc;
        if (int rc = map_stage_offsets(m, h_scan_offsets, n_scans, st)) return rc;
    }
    const long long points = n_scans > 0 ? (long long)h_scan_offsets[n_scans] - h_scan_offsets[0] : 0;
    return mq_launch(m, d_xyzi, m->d_offs, n_scans, max_pts, points, a, st);
}

int scvod_batch_map_query(scvod_ctx* ctx, scvod_map* m, const float* h_poses, float radius, const uint8_t* h_select256, uint8_t* d_result,
                          uint64_t* d_cell_val, uint64_t* d_nn_key, float* d_nn_sqdist, int64_t* d_scan_counts, void* stream) {
    if (!ctx || !m || !h_poses) return mfail(m, SCVOD_ERR_INVALID, "bad arguments");
    const MqArgs a = {radius, h_select256, d_result, d_cell_val, d_nn_key, d_nn_sqdist, d_scan_counts};
    if (int rc = mq_check(m, a)) return rc;
    Arena A;
    int device = 0, track_valid = 0, batch_valid = 0, n_scans = 0, max_pts = 0, mode = 0, min_pts = 0;
    scvod__ctx_view(ctx, &A, &device, &track_valid, &batch_valid, &n_scans, &max_pts, &mode, &min_pts);
    if (!batch_valid || !A.pts) return mfail(m, SCVOD_ERR_STATE, "scvod_batch_map_query needs a processed batch of input clouds");
    if (device != m->device) return mfail(m, SCVOD_ERR_INVALID, "map and ctx live on different devices");
    MHIP(m, hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)scvod__ctx_stream(ctx, stream);
    if (int rc = map_stage_poses(m, h_poses, n_scans, st)) return rc;
    return mq_launch(m, A.pts, A.scan_off, n_scans, max_pts, (long long)A.total_pts, a, st);
}

int scvod_map_query_stats(scvod_map* m, int64_t* h_out8) {
    if (!m || !h_out8) return mfail(m, SCVOD_ERR_INVALID, "bad arguments");
    if (!m->q_ran) return mfail(m, SCVOD_ERR_STATE, "scvod_map_query_stats before the first query");
    MHIP(m, hipSetDevice(m->device));
    MHIP(m, hipStreamSynchronize(m->q_stream));
    unsigned long long h[4] = {0, 0, 0, 0};
    MHIP(m, hipMemcpy(h, m->q_counters, sizeof(h), hipMemcpyDeviceToHost));
    h_out8[0] = (int64_t)m->q_points;
    for (int i = 0; i < 4; ++i) h_out8[1 + i] = (int64_t)h[i];
    h_out8[5] = h_out8[6] = h_out8[7] = 0;
    return SCVOD_OK;
}

int64_t scvod_map_query_scratch_bytes(const scvod_map* m) { return (m && m->q_counters) ? (int64_t)(4 * sizeof(unsigned long long)) : 0; }

}  // extern "C"
