// scvod_normals.hip -- surface normals and curvature of a cloud in HBM, or of the static map's points, on the device (gfx950).
//
// Not from the reference.  The neighbourhood, the ten int64 sums of a query and the finish are defined once, in
// scvod_math.h (nrm_*, normal_finish, normal_flip): this file finds the candidates of every query in the shared CSR grid of
// scvod_grid.h and feeds them to those functions.  A call enqueues k_nrm_keep (the keep byte of every cloud point), the grid build and
// k_nrm_accumulate; nothing is read on the host in between and no workgroup waits for another.
//
// Several of the 27 cells around a query may hash to one bucket, and a bucket may hold points of far cells.  The nearest-neighbour
// stages do not mind a point offered twice; a sum does.  A candidate therefore counts in the visit of cell c only if its own
// grid_cell is c: every point inside the radius lies in exactly one of the 27 cells, and is met in that cell's bucket.
#include "scvod_grid.h"
#include "scvod_maptable.h"

using namespace scvod;

namespace scvod {
namespace {

constexpr int kNrmMaxCloud = 1 << 28;
// Which arm the self form takes when nobody asks (scvod_set_normals_variant): a thread per grid entry, so that the lanes of a wave
// share buckets and cache lines, or a thread per query in the caller's order.  profiles/normals_cost.txt holds both times.
constexpr bool kNrmEntryOrder = true;

struct NrmK {  // what the kernels take
    const float* cloud;
    const float* query;  // the cloud itself in the self form
    int cloud_stride, query_stride, n_cloud, n_query;
    PointGrid grid;
    const uint8_t* keep;  // one byte per cloud point: 0 = never a neighbour
    float r2;
    int min_nb;
    const int32_t* seg_off;  // [n_seg + 1], or n_seg == 0
    const float* view;       // [n_seg][3]
    int n_seg;
    float* normals;
    float* curv;        // or nullptr
    int32_t* count;     // or nullptr
    long long* sums;    // or nullptr
    unsigned long long* stats;  // [8]: queries, finite normals, below min_neighbours, non-finite queries, cloud points left out, largest k, sum k, 0
};

// the keep byte of every cloud point, and how many were left out; one thread per point
__global__ __launch_bounds__(256) void k_nrm_keep(const float* __restrict__ cloud, int stride, int n, uint8_t* keep, unsigned long long* stats) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool out = false;
    if (i < n) {
        const float* p = cloud + (size_t)stride * (size_t)i;
        const bool ok = nrm_usable(p[0], p[1], p[2]);
        keep[i] = ok ? 1 : 0;
        out = !ok;
    }
    const unsigned long long bal = __ballot(out);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&stats[4], (unsigned long long)__popcll(bal));
}

// the segment of query q: the last s with seg_off[s] <= q (empty segments share an offset with the one behind them)
__device__ __forceinline__ int nrm_segment(const int32_t* __restrict__ seg_off, int n_seg, int q) {
    int lo = 0, hi = n_seg;  // the answer lies in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_off[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// One thread per query, the ten accumulators in registers, the finish fused behind the probe.
// ENTRY 0: thread t takes query t.  ENTRY 1 (self form only): thread t takes the point of grid entry t, so the lanes of a wave
// walk the same few buckets; a point that was left out of the grid is not among the entries, and thread t writes its NaN row when
// point t is such a point.  Every output row is written by exactly one thread in either arm.
// The loop waits on the dependent loads of a CSR walk (start / count -> entries -> coordinates); the sums are integers, so neither
// the order inside a bucket nor the arm nor the workgroup size changes a bit of the result.
template <int ENTRY>
__global__ __launch_bounds__(256) void k_nrm_accumulate(NrmK a) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) a.stats[0] = (unsigned long long)a.n_query;
    int q = -1, bad_q = -1;  // the query this thread probes, the query it only marks as not finite
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (ENTRY == 0) {
        if (t < a.n_query) q = (int)t;
    } else {
        const int n_in = a.n_cloud - (int)a.stats[4];  // (k_nrm_keep has finished: the stream orders it)
        if (t < n_in) q = a.grid.entries[t];
        if (t < a.n_cloud && !a.keep[t]) bad_q = (int)t;
    }
    if (q >= 0) {
        const float* p = a.query + (size_t)a.query_stride * (size_t)q;
        qx = p[0], qy = p[1], qz = p[2];
        if (ENTRY == 0 && !nrm_usable(qx, qy, qz)) {
            bad_q = q;
            q = -1;
        }
    }
    long long s[kNrmWords];
#pragma unroll
    for (int i = 0; i < kNrmWords; ++i) s[i] = 0;
    float out[4];
    const float nan = u2f(0x7fc00000u);
    out[0] = out[1] = out[2] = out[3] = nan;
    if (q >= 0) {
        if (a.n_cloud > 0) {
            int cx, cy, cz;
            grid_cell(a.grid, qx, qy, qz, cx, cy, cz);
            for (int dz = -1; dz <= 1; ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int ccx = cx + dx, ccy = cy + dy, ccz = cz + dz;
                        const uint32_t b = grid_bucket(a.grid, ccx, ccy, ccz);
                        const int s0 = a.grid.start[b], c = a.grid.count[b];
                        for (int k = 0; k < c; ++k) {
                            const int m = a.grid.entries[s0 + k];
                            const float* p = a.cloud + (size_t)a.cloud_stride * (size_t)m;
                            const float px = p[0], py = p[1], pz = p[2];
                            const float ex = px - qx, ey = py - qy, ez = pz - qz;
                            if ((ex * ex + ey * ey) + ez * ez < a.r2) {
                                int pcx, pcy, pcz;
                                grid_cell(a.grid, px, py, pz, pcx, pcy, pcz);
                                if (pcx == ccx && pcy == ccy && pcz == ccz) nrm_add(px, py, pz, qx, qy, qz, a.r2, s);
                            }
                        }
                    }
        }
        normal_finish(s, a.min_nb, out);
        if (a.n_seg > 0) normal_flip(a.view + 3 * (size_t)nrm_segment(a.seg_off, a.n_seg, q), qx, qy, qz, out);
    }
    if (q >= 0) {
        a.normals[3 * (size_t)q] = out[0];
        a.normals[3 * (size_t)q + 1] = out[1];
        a.normals[3 * (size_t)q + 2] = out[2];
        if (a.curv) a.curv[q] = out[3];
        if (a.count) a.count[q] = (int32_t)s[0];
        if (a.sums) {
#pragma unroll
            for (int i = 0; i < kNrmWords; ++i) a.sums[(size_t)kNrmWords * (size_t)q + i] = s[i];
        }
    }
    if (bad_q >= 0) {  // (ENTRY 1: a thread may hold a query of either kind, two different rows)
        a.normals[3 * (size_t)bad_q] = a.normals[3 * (size_t)bad_q + 1] = a.normals[3 * (size_t)bad_q + 2] = nan;
        if (a.curv) a.curv[bad_q] = nan;
        if (a.count) a.count[bad_q] = 0;
        if (a.sums) {
#pragma unroll
            for (int i = 0; i < kNrmWords; ++i) a.sums[(size_t)kNrmWords * (size_t)bad_q + i] = 0;
        }
    }
    // the counters: wave-uniform (ballot + popcount), the largest k and the sum of k through a butterfly
    const bool probed = q >= 0;
    const bool finite = probed && out[0] == out[0] && out[1] == out[1] && out[2] == out[2];
    const unsigned long long n_finite = __popcll(__ballot(finite));
    const unsigned long long n_below = __popcll(__ballot(probed && s[0] < (long long)a.min_nb));
    const unsigned long long n_bad = __popcll(__ballot(bad_q >= 0));
    long long ksum = s[0];
    int kmax = (int)s[0];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        ksum += __shfl_xor(ksum, d);
        kmax = max(kmax, __shfl_xor(kmax, d));
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_finite) atomicAdd(&a.stats[1], n_finite);
        if (n_below) atomicAdd(&a.stats[2], n_below);
        if (n_bad) atomicAdd(&a.stats[3], n_bad);
        if (kmax) atomicMax(&a.stats[5], (unsigned long long)kmax);
        if (ksum) atomicAdd(&a.stats[6], (unsigned long long)ksum);
    }
}

// what hangs on a ctx: one grow-only block, the last call's stream (compared, never used again) and the event behind that call
struct NrmState {
    unsigned char* buf = nullptr;
    size_t cap = 0;
    hipStream_t stream = nullptr;
    bool ran = false;
    int variant = 0;  // scvod_set_normals_variant
    hipEvent_t done = nullptr;  // behind the last call's last kernel: what a call on another stream, a grow and the stats wait for
};

// the segment tables of one call on the host: they feed the call's copies and are freed by a host function behind them on the stream
struct NrmStage {
    std::vector<int32_t> seg;
    std::vector<float> view;
};
void nrm_stage_free(void* p) { delete (NrmStage*)p; }

size_t nrm_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct NrmLayout {
    size_t stats, seg, view, keep, grid, bytes;
};
NrmLayout nrm_layout(int n_seg, int n_cloud, size_t grid_ints) {
    NrmLayout L;
    size_t o = 0;
    L.stats = o;
    o = nrm_up(o + 8 * sizeof(unsigned long long));
    L.seg = o;
    o = nrm_up(o + (n_seg > 0 ? sizeof(int32_t) * ((size_t)n_seg + 1) : 0));
    L.view = o;
    o = nrm_up(o + sizeof(float) * 3 * (size_t)n_seg);
    L.keep = o;
    o = nrm_up(o + (size_t)(n_cloud > 0 ? n_cloud : 1));
    L.grid = o;
    o = nrm_up(o + sizeof(int) * grid_ints);
    L.bytes = o;
    return L;
}

scvod_normal_params nrm_params(const scvod_normal_params* params) {
    scvod_normal_params p;
    if (params)
        p = *params;
    else
        scvod_normal_params_default(&p);
    return p;
}

const char* nrm_check(const scvod_normal_params& p, int cloud_stride, long long n_cloud, int query_stride, long long n_query, const int32_t* h_seg,
                      const float* h_view, int n_seg) {
    if (!(p.radius > 0.f) || !(p.radius <= 4.f)) return "radius outside (0, 4]";
    if (p.min_neighbours < 3) return "min_neighbours below 3";
    if (p.flags != 0 || p.reserved != 0) return "flags and reserved must be 0";
    if (cloud_stride != 3 && cloud_stride != 4) return "the cloud's stride is neither 3 nor 4";
    if (query_stride != 0 && query_stride != 3 && query_stride != 4) return "the queries' stride is neither 3 nor 4";
    if (n_cloud < 0 || n_cloud > kNrmMaxCloud) return "n_cloud outside 0 .. 2^28";
    if (n_query < 0 || n_query > 0x7fffffffll) return "n_query outside 0 .. 2^31 - 1";
    if (n_seg < 0) return "n_segments below 0";
    if (n_seg == 0 && (h_seg || h_view)) return "segment offsets or viewpoints with n_segments 0";
    if (n_seg > 0) {
        if (!h_seg) return "viewpoints without segment offsets";
        if (!h_view) return "segment offsets without viewpoints";
        if (h_seg[0] != 0) return "segment offsets do not start at 0";
        for (int s = 0; s < n_seg; ++s)
            if (h_seg[s + 1] < h_seg[s]) return "segment offsets decrease";
        if ((long long)h_seg[n_seg] != n_query) return "segment offsets do not end at n_query";
    }
    return nullptr;
}

#define NHIP(call)                                                                  \
    do {                                                                            \
        hipError_t e__ = (call);                                                    \
        if (e__ != hipSuccess) {                                                    \
            err = std::string(#call) + ": " + hipGetErrorString(e__);              \
            return SCVOD_ERR_HIP;                                                   \
        }                                                                           \
    } while (0)

struct NrmCall {
    const float* cloud;
    const float* query;  // nullptr: the self form
    int cloud_stride, query_stride, n_cloud, n_query;
    const int32_t* h_seg;
    const float* h_view;
    int n_seg;
    scvod_normal_params p;
    float* normals;
    float* curv;
    int32_t* count;
    long long* sums;
};

// the whole call, after its argument checks
int nrm_run(NrmState** slot, int device, const NrmCall& c, hipStream_t st, std::string& err) {
    NHIP(hipSetDevice(device));
    if (!*slot) *slot = new NrmState();
    NrmState& R = **slot;
    if (!R.done) NHIP(hipEventCreateWithFlags(&R.done, hipEventDisableTiming));
    // the block and the counters are shared: a call on another stream is ordered behind the last one on the device, not on the host
    // (the event, not the earlier stream's handle, which its owner may have destroyed since)
    if (R.ran && R.stream != st) NHIP(hipStreamWaitEvent(st, R.done, 0));
    float cell = 0.f;
    int32_t buckets = 0;
    size_t grid_ints = 0;
    if (c.n_cloud > 0) {
        cell = c.p.radius > 0.2f ? c.p.radius : 0.2f;
        if (c.p.radius * c.p.radius > (0.99f * cell) * (0.99f * cell)) cell = c.p.radius / 0.98f;
        buckets = grid_buckets(c.n_cloud);
        grid_ints = grid_work_ints(buckets, c.n_cloud);
    }
    const NrmLayout L = nrm_layout(c.n_seg, c.n_cloud, grid_ints);
    if (L.bytes > R.cap) {
        if (R.ran) NHIP(hipEventSynchronize(R.done));
        if (R.buf) hipFree(R.buf);
        R.buf = nullptr;
        R.cap = 0;
        const size_t grown = L.bytes + L.bytes / 4;
        NHIP(hipMalloc(&R.buf, grown));
        R.cap = grown;
    }
    R.stream = st;
    R.ran = true;
    unsigned long long* stats = (unsigned long long*)(R.buf + L.stats);
    NHIP(hipMemsetAsync(stats, 0, 8 * sizeof(unsigned long long), st));
    // the segment tables: copied from a staging object of this call's own, which a host function behind the copies frees -- the
    // caller's arrays are read before this returns and no call waits for an earlier one's copy
    if (c.n_seg > 0) {
        NrmStage* stage = new NrmStage{std::vector<int32_t>(c.h_seg, c.h_seg + c.n_seg + 1), std::vector<float>(c.h_view, c.h_view + 3 * (size_t)c.n_seg)};
        hipError_t e = hipMemcpyAsync(R.buf + L.seg, stage->seg.data(), sizeof(int32_t) * stage->seg.size(), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(R.buf + L.view, stage->view.data(), sizeof(float) * stage->view.size(), hipMemcpyHostToDevice, st);
        if (e != hipSuccess || hipLaunchHostFunc(st, nrm_stage_free, stage) != hipSuccess) {
            hipStreamSynchronize(st);  // (an error path: nothing may read the staging object once it is gone)
            delete stage;
            if (e != hipSuccess) {
                err = std::string("hipMemcpyAsync of the segment tables: ") + hipGetErrorString(e);
                return SCVOD_ERR_HIP;
            }
        }
    }
    NrmK a;
    memset(&a, 0, sizeof(a));
    a.cloud = c.cloud;
    a.cloud_stride = c.cloud_stride;
    a.n_cloud = c.n_cloud;
    a.query = c.query ? c.query : c.cloud;
    a.query_stride = c.query ? c.query_stride : c.cloud_stride;
    a.n_query = c.n_query;
    a.keep = R.buf + L.keep;
    a.r2 = c.p.radius * c.p.radius;
    a.min_nb = c.p.min_neighbours;
    a.seg_off = (const int32_t*)(R.buf + L.seg);
    a.view = (const float*)(R.buf + L.view);
    a.n_seg = c.n_seg;
    a.normals = c.normals;
    a.curv = c.curv;
    a.count = c.count;
    a.sums = c.sums;
    a.stats = stats;
    if (c.n_cloud > 0) {
        hipLaunchKernelGGL(k_nrm_keep, dim3((unsigned)(((long long)c.n_cloud + 255) / 256)), dim3(256), 0, st, c.cloud, c.cloud_stride, c.n_cloud,
                           (uint8_t*)(R.buf + L.keep), stats);
        a.grid = grid_build(c.cloud, c.cloud_stride, a.keep, c.n_cloud, kGridOrigin0, cell, buckets, (int*)(R.buf + L.grid), st);
    }
    if (c.n_query > 0) {
        const int arm = R.variant & 3;
        const bool entry = !c.query && c.n_cloud > 0 && (arm == 2 || (arm == 0 && kNrmEntryOrder));
        const int threads = (R.variant & 4) ? 64 : 256;
        const dim3 grid((unsigned)(((long long)c.n_query + threads - 1) / threads)), block(threads);
        if (entry)
            hipLaunchKernelGGL(k_nrm_accumulate<1>, grid, block, 0, st, a);
        else
            hipLaunchKernelGGL(k_nrm_accumulate<0>, grid, block, 0, st, a);
    }
    NHIP(hipGetLastError());
    NHIP(hipEventRecord(R.done, st));
    return SCVOD_OK;
}

NrmState** nrm_slot(scvod_ctx* ctx, int* device, hipStream_t* own) {
    void* s = nullptr;
    void** slot = scvod__ctx_normals_slot(ctx, device, &s);
    *own = (hipStream_t)s;
    return (NrmState**)slot;
}

}  // namespace
}  // namespace scvod

extern "C" {

void scvod__normals_free(void* state) {
    NrmState* R = (NrmState*)state;
    if (!R) return;
    if (R->done) {
        if (R->ran) hipEventSynchronize(R->done);
        hipEventDestroy(R->done);
    }
    if (R->buf) hipFree(R->buf);
    delete R;
}

void scvod_normal_params_default(scvod_normal_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->radius = 0.5f;
    p->min_neighbours = 5;
}

int scvod_normals_check(const scvod_normal_params* params, int32_t cloud_stride, int64_t n_cloud, int32_t query_stride, int64_t n_query,
                        const int32_t* h_seg_offsets, const float* h_viewpoints, int32_t n_segments) {
    return nrm_check(nrm_params(params), cloud_stride, n_cloud, query_stride, n_query, h_seg_offsets, h_viewpoints, n_segments) ? SCVOD_ERR_INVALID
                                                                                                                                : SCVOD_OK;
}

int scvod_set_normals_variant(scvod_ctx* ctx, int32_t variant) {
    if (!ctx) return SCVOD_ERR_INVALID;
    if (variant < 0 || variant > 7 || (variant & 3) == 3) return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "scvod_set_normals_variant: unknown variant");
    int device = 0;
    hipStream_t own = nullptr;
    NrmState** slot = nrm_slot(ctx, &device, &own);
    if (!*slot) *slot = new NrmState();
    (*slot)->variant = variant;
    return SCVOD_OK;
}

int scvod_normals_device(scvod_ctx* ctx, const float* d_cloud, int32_t cloud_stride, int32_t n_cloud, const float* d_query, int32_t query_stride,
                         int32_t n_query, const int32_t* h_seg_offsets, const float* h_viewpoints, int32_t n_segments,
                         const scvod_normal_params* params, float* d_normals, float* d_curvature, int32_t* d_count, int64_t* d_sums, void* stream) {
    if (!ctx) return SCVOD_ERR_INVALID;
    const scvod_normal_params p = nrm_params(params);
    if (const char* why = nrm_check(p, cloud_stride, n_cloud, d_query ? query_stride : 0, n_query, h_seg_offsets, h_viewpoints, n_segments))
        return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, (std::string("scvod_normals_device: ") + why).c_str());
    if (!d_query && n_query != n_cloud) return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "scvod_normals_device: the self form needs n_query == n_cloud");
    if ((n_cloud > 0 && !d_cloud) || (n_query > 0 && !d_normals))
        return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "scvod_normals_device: NULL cloud or normals of a call that is not empty");
    if (((uintptr_t)d_cloud & 3u) || ((uintptr_t)d_query & 3u) || ((uintptr_t)d_normals & 3u) || ((uintptr_t)d_curvature & 3u) || ((uintptr_t)d_count & 3u) ||
        ((uintptr_t)d_sums & 7u))
        return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "scvod_normals_device: a pointer is not aligned to its element");
    int device = 0;
    hipStream_t own = nullptr;
    NrmState** slot = nrm_slot(ctx, &device, &own);
    NrmCall c;
    memset(&c, 0, sizeof(c));
    c.cloud = d_cloud;
    c.query = d_query;
    c.cloud_stride = cloud_stride;
    c.query_stride = query_stride;
    c.n_cloud = n_cloud;
    c.n_query = n_query;
    c.h_seg = h_seg_offsets;
    c.h_view = h_viewpoints;
    c.n_seg = n_segments;
    c.p = p;
    c.normals = d_normals;
    c.curv = d_curvature;
    c.count = d_count;
    c.sums = (long long*)d_sums;
    std::string err;
    const int rc = nrm_run(slot, device, c, stream ? (hipStream_t)stream : own, err);
    return rc ? scvod__ctx_fail(ctx, rc, err.c_str()) : SCVOD_OK;
}

int scvod_normals_stats(scvod_ctx* ctx, int64_t* h_out8) {
    if (!ctx) return SCVOD_ERR_INVALID;
    if (!h_out8) return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "bad arguments");
    int device = 0;
    hipStream_t own = nullptr;
    NrmState* R = *nrm_slot(ctx, &device, &own);
    if (!R || !R->ran) return scvod__ctx_fail(ctx, SCVOD_ERR_STATE, "scvod_normals_stats before the first call");
    if (hipSetDevice(device) != hipSuccess || hipEventSynchronize(R->done) != hipSuccess) return scvod__ctx_fail(ctx, SCVOD_ERR_HIP, "scvod_normals_stats: the stream failed");
    unsigned long long h[8] = {0};
    if (hipMemcpy(h, R->buf, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)  // (the counters lead the block)
        return scvod__ctx_fail(ctx, SCVOD_ERR_HIP, "scvod_normals_stats: the copy failed");
    for (int i = 0; i < 8; ++i) h_out8[i] = (int64_t)h[i];
    return SCVOD_OK;
}

int64_t scvod_normals_scratch_bytes(scvod_ctx* ctx) {
    if (!ctx) return 0;
    int device = 0;
    hipStream_t own = nullptr;
    NrmState* R = *nrm_slot(ctx, &device, &own);
    return R ? (int64_t)R->cap : 0;
}

int scvod_map_points_normals(scvod_ctx* ctx, scvod_map* map, const scvod_normal_params* params, const uint8_t* h_select256, void* d_xyzi,
                             uint8_t* d_labels, float* d_normals, float* d_curvature, int64_t cap, int64_t* n_out, void* stream) {
    if (!ctx) return SCVOD_ERR_INVALID;
    if (!map || !n_out || cap < 0 || !d_xyzi || !d_normals) return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "scvod_map_points_normals: bad arguments");
    const scvod_normal_params p = nrm_params(params);
    if (const char* why = nrm_check(p, 4, 0, 0, 0, nullptr, nullptr, 0))
        return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, (std::string("scvod_map_points_normals: ") + why).c_str());
    const bool labelled = map->kind == SCVOD_MAP_KIND_LABELLED;
    if (!labelled && (h_select256 || d_labels))
        return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "scvod_map_points_normals: a select table or label bytes need a map of kind SCVOD_MAP_KIND_LABELLED");
    if (((uintptr_t)d_xyzi & 15u) || ((uintptr_t)d_normals & 3u) || ((uintptr_t)d_curvature & 3u))
        return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "scvod_map_points_normals: d_xyzi is not 16-byte aligned, or an output not 4-byte aligned");
    int device = 0;
    hipStream_t own = nullptr;
    NrmState** slot = nrm_slot(ctx, &device, &own);
    if (device != map->device) return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "scvod_map_points_normals: map and ctx live on different devices");
    hipStream_t st = stream ? (hipStream_t)stream : own;
    const int rc = labelled ? scvod_map_points_labelled(map, d_xyzi, d_labels, nullptr, cap, h_select256, n_out, st)
                            : scvod_map_points(map, d_xyzi, nullptr, cap, n_out, st);
    if (rc) return scvod__ctx_fail(ctx, rc, (std::string("scvod_map_points_normals: ") + map->err).c_str());
    if (*n_out > kNrmMaxCloud) return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "scvod_map_points_normals: the map holds more than 2^28 cells");
    NrmCall c;
    memset(&c, 0, sizeof(c));
    c.cloud = (const float*)d_xyzi;
    c.cloud_stride = 4;
    c.n_cloud = c.n_query = (int)*n_out;
    c.p = p;
    c.normals = d_normals;
    c.curv = d_curvature;
    std::string err;
    const int rc2 = nrm_run(slot, device, c, st, err);
    return rc2 ? scvod__ctx_fail(ctx, rc2, err.c_str()) : SCVOD_OK;
}

}  // extern "C"
