// scvod_maptable.h -- the static map's table as its translation units see it: the record, the map object, the hash, the cell of a
// point, the probe load, the decode of a record and the host-side staging of poses and scan offsets.  scvod_map.hip fills, merges and
// exports the table; scvod_mapquery.hip and scvod_mapfilter.hip only read it (through scvod_mapprobe.h).
#ifndef SCVOD_MAPTABLE_H_
#define SCVOD_MAPTABLE_H_
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "scvod_dev.h"

struct MapRec {
    unsigned long long key;  // ~0 = empty
    unsigned long long val;  // packed {qx, qy, qz, qi}, 16 bits each, smallest wins (labelled kind: {qx, qy, qz} 16 bits each, label 8, qi 8)
};
static_assert(sizeof(MapRec) == 16, "map record");

struct scvod_map {
    int device = 0;
    float leaf = 0.2f;
    long long capacity = 0;  // power of two
    MapRec* table = nullptr;
    unsigned long long* counters = nullptr;  // [0] records exported, [1] insertions dropped (table full / out of range), [2..2+64) per-part counts / cursors
    float* d_pose = nullptr;                 // [pose_cap][12]
    long long pose_cap = 0;
    std::vector<float> up_pose;
    int kind = SCVOD_MAP_KIND_PLAIN;
    // scan offsets of the ctx-free calls (staged like the poses) and, labelled kind only, the class bytes of the batch form
    int32_t* d_offs = nullptr;  // [offs_cap]
    long long offs_cap = 0;
    std::vector<int32_t> up_offs;
    uint8_t* d_cls = nullptr;  // [cls_cap] one byte per input point of the largest batch seen (grow-only)
    long long cls_cap = 0;
    // scvod_map_query: {CELL, NEAR, MISS, OUT} of the last query, an allocation of the query's own (made by the first query)
    unsigned long long* q_counters = nullptr;  // [4]
    long long q_points = 0;                    // points of the last query
    hipStream_t q_stream = nullptr;            // its stream
    bool q_ran = false;
    // scvod_map_filter: one grow-only block of the filter's own (its counters, side and result bytes, tile counts; scvod_mapfilter.hip)
    unsigned char* f_buf = nullptr;
    size_t f_cap = 0;
    long long f_points = 0;          // points of the last filter
    hipStream_t f_stream = nullptr;  // its stream
    bool f_ran = false;
    // scvod_map_components / scvod_map_component_visibility: one grow-only block each, of their own (scvod_mapcomp.hip)
    unsigned char* c_buf = nullptr;
    size_t c_cap = 0;
    long long c_records = 0;         // records of the last components call
    hipStream_t c_stream = nullptr;  // its stream
    bool c_ran = false;
    unsigned char* v_buf = nullptr;
    size_t v_cap = 0;
    hipStream_t v_stream = nullptr;  // the stream of the last component vote
    bool v_ran = false;
    // scvod_map_register: the state of scvod_register.hip (its grow-only block, the staged poses and offsets), made by the first call
    void* reg_state = nullptr;
    std::string err;
};

namespace scvod {
namespace {

constexpr unsigned long long kEmpty = ~0ull;
constexpr int kMapMaxProbes = 512;  // linear probing: longer runs only appear beyond ~95 % load
constexpr int kCellBits = 21, kCellBias = 1 << 20;
// k_map_accumulate: points per thread and round / points per workgroup.  Measured on the 2761-scan K64 job (round 3): one point per
// thread beats two / four / eight in flight (4.82 / 4.96 / 5.43 / 6.19 ms at 2048 points per workgroup: the extra registers cost
// occupancy and the later atomics act on staler peeks), and 8192 points per workgroup beat 512 .. 32768 (5.03 .. 4.45 .. 4.58 ms)
constexpr int kMapU = 1, kMapPts = 8192;

int mfail(scvod_map* m, int code, const char* fmt, ...) {
    if (m) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        m->err = buf;
    }
    return code;
}
#define MHIP(m, call)                                                                                    \
    do {                                                                                                 \
        hipError_t e__ = (call);                                                                         \
        if (e__ != hipSuccess) return mfail(m, SCVOD_ERR_HIP, "%s: %s", #call, hipGetErrorString(e__)); \
    } while (0)

__device__ __forceinline__ unsigned long long map_mix(unsigned long long k) {  // murmur3 finaliser
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// home slot of a cell: a hash of the whole cell.  (Blocks of neighbouring cells laid side by side in the table were measured in rounds 3
// and 5, from 2 x 2 x 1 to 4 x 4 x 4 cells: every one slower -- profiles/r05_experiments.md.)
__device__ __forceinline__ unsigned long long map_home(unsigned long long key, unsigned long long mask) { return map_mix(key) & mask; }

// cell + packed in-cell offset of a world point.  floor(p * inv_leaf) like pcl::VoxelGrid's cell index; the offset is
// quantised to 16 bits of the cell edge, the intensity to 1/256 (clamped to [0, 255.996]).
__device__ __forceinline__ bool map_encode(float x, float y, float z, float intensity, float inv_leaf, unsigned long long& key,
                                           unsigned long long& val) {
    const float fx = x * inv_leaf, fy = y * inv_leaf, fz = z * inv_leaf;
    const float cx = floor_f(fx), cy = floor_f(fy), cz = floor_f(fz);
    if (!(cx >= -(float)kCellBias && cx < (float)kCellBias && cy >= -(float)kCellBias && cy < (float)kCellBias &&
          cz >= -(float)kCellBias && cz < (float)kCellBias))
        return false;  // also NaN
    const unsigned long long ux = (unsigned long long)((int)cx + kCellBias), uy = (unsigned long long)((int)cy + kCellBias),
                             uz = (unsigned long long)((int)cz + kCellBias);
    key = (ux << (2 * kCellBits)) | (uy << kCellBits) | uz;
    auto q16 = [](float f) -> unsigned long long {
        int q = (int)(f * 65536.0f);
        return (unsigned long long)(q < 0 ? 0 : (q > 65535 ? 65535 : q));
    };
    float in = intensity * 256.0f;
    in = in < 0.f ? 0.f : (in > 65535.f ? 65535.f : in);
    val = (q16(fx - cx) << 48) | (q16(fy - cy) << 32) | (q16(fz - cz) << 16) | (unsigned long long)(int)in;
    return true;
}

// One 16-byte load per probe (key and value together).  The load is an ordinary cached one: a key, once set, never changes
// and a value only decreases, so a stale record can only show (a) an empty slot that is taken by now -- the CAS then returns
// the owner -- or (b) a value above the current one -- the atomicMin then runs although it was not needed.  Both are harmless.
__device__ __forceinline__ MapRec map_peek(const MapRec* table, unsigned long long h) {
    const ulonglong2 r = *reinterpret_cast<const ulonglong2*>(&table[h]);
    MapRec m;
    m.key = r.x;
    m.val = r.y;
    return m;
}

// is `label` set in the 256-bit table k0..k3?  The four words are kernel arguments: they live in scalar registers
__device__ __forceinline__ bool map_bit256(unsigned long long k0, unsigned long long k1, unsigned long long k2, unsigned long long k3,
                                           unsigned int label) {
    const unsigned long long lo = (label & 64u) ? k1 : k0, hi = (label & 64u) ? k3 : k2;
    return (((label & 128u) ? hi : lo) >> (label & 63u)) & 1ull;
}

// one axis of a record's point: cell c, 16-bit offset q inside it (what scvod_map_points hands out, and what a query measures against)
__device__ __forceinline__ float map_decode(int c, float q, float leaf) { return ((float)c + (q + 0.5f) / 65536.0f) * leaf; }

// the 256 keep / select bytes as the four words the kernels take; NULL = every label
void map_table256(const uint8_t* h256, unsigned long long k[4]) {
    for (int w = 0; w < 4; ++w) {
        k[w] = h256 ? 0ull : ~0ull;
        if (h256)
            for (int b = 0; b < 64; ++b)
                if (h256[64 * w + b]) k[w] |= 1ull << b;
    }
}

// the poses of a call as matrices on the device (h_poses NULL: the zero pose, n times).  The staging vector may still feed an earlier
// asynchronous copy: values that differ from the previous call's wait for `st` first.
int map_stage_poses(scvod_map* m, const float* h_poses, int n, hipStream_t st) {
    const float zero[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    std::vector<float> T((size_t)12 * n);
    for (int s = 0; s < n; ++s) scvod_pose_matrix(h_poses ? h_poses + 6 * s : zero, T.data() + 12 * s);
    if (m->pose_cap < n) {
        MHIP(m, hipStreamSynchronize(st));
        if (m->d_pose) hipFree(m->d_pose);
        m->d_pose = nullptr;
        m->pose_cap = 0;
        m->up_pose.clear();
        MHIP(m, hipMalloc(&m->d_pose, sizeof(float) * 12 * (size_t)n));
        m->pose_cap = n;
    }
    if (m->up_pose != T) {
        MHIP(m, hipStreamSynchronize(st));
        m->up_pose = T;
        MHIP(m, hipMemcpyAsync(m->d_pose, m->up_pose.data(), sizeof(float) * T.size(), hipMemcpyHostToDevice, st));
    }
    return SCVOD_OK;
}

// the n_scans + 1 host scan offsets of a ctx-free call on the device (the same hazard as the poses' staging vector)
int map_stage_offsets(scvod_map* m, const int32_t* h_scan_offsets, int n_scans, hipStream_t st) {
    const std::vector<int32_t> offs(h_scan_offsets, h_scan_offsets + n_scans + 1);
    if (m->offs_cap < n_scans + 1) {
        MHIP(m, hipStreamSynchronize(st));
        if (m->d_offs) hipFree(m->d_offs);
        m->d_offs = nullptr;
        m->offs_cap = 0;
        m->up_offs.clear();
        MHIP(m, hipMalloc(&m->d_offs, sizeof(int32_t) * ((size_t)n_scans + 1)));
        m->offs_cap = (long long)n_scans + 1;
    }
    if (m->up_offs != offs) {
        MHIP(m, hipStreamSynchronize(st));
        m->up_offs = offs;
        MHIP(m, hipMemcpyAsync(m->d_offs, m->up_offs.data(), sizeof(int32_t) * offs.size(), hipMemcpyHostToDevice, st));
    }
    return SCVOD_OK;
}

// the scan-offset checks of a ctx-free call; max_pts = the longest scan
int map_check_offsets(scvod_map* m, const int32_t* h_scan_offsets, int n_scans, int* max_pts) {
    if (h_scan_offsets[0] < 0) return mfail(m, SCVOD_ERR_INVALID, "scan offsets start below 0");
    *max_pts = 0;
    for (int s = 0; s < n_scans; ++s) {
        if (h_scan_offsets[s + 1] < h_scan_offsets[s]) return mfail(m, SCVOD_ERR_INVALID, "scan offsets decrease at scan %d", s);
        if (h_scan_offsets[s + 1] - h_scan_offsets[s] > *max_pts) *max_pts = h_scan_offsets[s + 1] - h_scan_offsets[s];
    }
    return SCVOD_OK;
}

}  // namespace
}  // namespace scvod

// the one place the map code needs the batch context: its arena, parameters and validity flags
struct scvod_ctx;
extern "C" int scvod__ctx_types_valid(scvod_ctx* c);
extern "C" int scvod__ctx_view(scvod_ctx* ctx, scvod::Arena* arena, int* device, int* track_valid, int* batch_valid, int* n_scans,
                               int* max_scan_pts, int* batch_mode, int* num_min_pts);
extern "C" void* scvod__ctx_stream(scvod_ctx* ctx, void* stream);
extern "C" void** scvod__ctx_register_slot(scvod_ctx* ctx, int* device, void** own_stream);
extern "C" void** scvod__ctx_normals_slot(scvod_ctx* ctx, int* device, void** own_stream);
extern "C" int scvod__ctx_fail(scvod_ctx* ctx, int code, const char* msg);
extern "C" void scvod__register_free(void* state);  // scvod_register.hip: frees what a reg_state slot holds (NULL: nothing)
extern "C" int scvod__ctx_ensure_lists(scvod_ctx* ctx, void* stream);  // ground_idx / nonground_idx / rejected_src of a lean batch, before their reader
extern "C" int scvod__ctx_object_lists(scvod_ctx* ctx, const char* who, const long long** tab_stats, const uint64_t** key_out, const int32_t** begin,
                                       const char** err);

#endif
