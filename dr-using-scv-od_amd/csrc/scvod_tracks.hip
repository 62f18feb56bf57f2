// scvod_tracks.hip -- the objects of a batch linked into tracks on the device (gfx950): scvod_object_tracks_device,
// scvod_batch_object_tracks (include/scvod.h; the association rule: DESIGN.md section 2).
//
// Reference analogue: Cluster::track_id (src/ssc.cpp:1266-1272, 1356, 1381, 1400) names the identity; the rule here is this project's
// convention.  Everything it reads is in HBM after scvod_batch_track and scvod_batch_objects: the 64-byte records of the table, its
// per-scan offsets, and the first-order remap_name pairs (or a caller's candidate lists).  The chain kernel is not touched.
//     k_trk_offsets   batch form: the per-scan object counts of the table's scratch -> offsets
//     k_trk_world     per object: world centre (the map kernel's expression) and box diagonal; clears its proposal slot
//     k_trk_link      one wave per object A: the best overlap candidate, else the best object of the successor scan inside the gate; a
//                     wave reduction of a packed 64-bit key, then one 64-bit atomicMax into the winner's slot
//     k_trk_confirm   per object: who won its slot (pred, kind, weight, step) and whether its own proposal was accepted (succ)
//     k_trk_jump      pointer jumping over pred, double-buffered, ceil(log2(max(n_scans, 2))) rounds known on the host
//     k_trk_chain     length and last object of every chain: one 64-bit atomicMax of (rank, object) at the head
//     k_trk_flag      per object: (1, length) packed for the listed heads, 0 otherwise; rocprim's exclusive scan gives the track
//                     index and the first slot of the track's run at once
//     k_trk_scatter   track / rank of every object, the track-object list, the head of every track
//     k_trk_reduce    one wave per track over its contiguous run, 64 members at a time; the path is the sequential fp32 sum
// Nothing waits for another workgroup; launch sizes come from the caller's capacity and n_scans, the true counts are read on the
// device.  Integer atomics (max, add) and fixed-order float chains only: every output is the same bit for bit on every run and for any
// launch geometry.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <cmath>
#include <cstring>

#include "scvod_dev.h"
#include "scvod_math.h"

namespace scvod {
namespace {

constexpr unsigned long long kTrkNone = ~0ull;

__device__ __forceinline__ unsigned long long trk_shfl_xor(unsigned long long v, int d) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long trk_wave_max(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = trk_shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long trk_wave_min(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = trk_shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int trk_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the objects of the table, or -1 when the caller's capacity does not hold them: then the stage does nothing but say so
__device__ __forceinline__ int trk_objects(const TrkJob& J) {
    const int n = J.obj_off[J.n_scans];
    return (n < 0 || (long long)n > J.cap) ? -1 : n;
}

// squared distance of two world centres: (dx*dx + dy*dy) + dz*dz in fp32
__device__ __forceinline__ float trk_d2(const float4& a, const float4& b) {
    const float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// apri point c of the scan at `base` names an object of the table (scvod_objects.hip's test)
__device__ __forceinline__ bool trk_is_root(const Arena& A, int base, int n_a, int c) {
    return (unsigned)c < (unsigned)n_a && A.pt_type[(size_t)base + c] != 0 && A.pt_cluster[(size_t)base + c] == c;
}

// batch form: the table's per-scan object counts (scan_cnt[2 s]) -> J.obj_off; one workgroup
__global__ __launch_bounds__(1024) void k_trk_offsets(const int32_t* scan_cnt, int32_t* off, int n_scans) {
    __shared__ int wsum[17];
    int carry = 0;
    for (int b = 0; b < n_scans; b += 1024) {
        const int i = b + (int)threadIdx.x;
        const int v = i < n_scans ? scan_cnt[2 * i] : 0;
        int total;
        const int ex = block_excl_scan<1024>(v, total, wsum);
        if (i < n_scans) off[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) off[n_scans] = carry;
}

__global__ __launch_bounds__(256) void k_trk_world(TrkJob J) {
    const int n_obj = trk_objects(J);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_obj) return;
    const scvod_object& o = J.objects[i];
    const int s = o.scan;
    const float x = o.center[0], y = o.center[1], z = o.center[2];
    float4 w = make_float4(x, y, z, 0.f);
    if ((unsigned)s < (unsigned)J.n_scans) {
        const float* T = J.T + 12 * (size_t)s;
        w.x = T[0] * x + T[1] * y + T[2] * z + T[3];
        w.y = T[4] * x + T[5] * y + T[6] * z + T[7];
        w.z = T[8] * x + T[9] * y + T[10] * z + T[11];
    }
    const float ex = o.box_max[0] - o.box_min[0], ey = o.box_max[1] - o.box_min[1], ez = o.box_max[2] - o.box_min[2];
    w.w = sqrt_f((ex * ex + ey * ey) + ez * ez);
    J.cw[i] = w;
    J.slot[i] = 0ull;
    J.chain[i] = 0ull;
}

// One wave per object A.  ARENA: the overlap candidates are the remap_name pairs of A's root in the arena, their labels mapped through
// the table's root_obj; otherwise the caller's lists.  Scan, successor, run bounds and A's record are wave-uniform.
template <bool ARENA>
__global__ __launch_bounds__(256) void k_trk_link(Arena A, TrkJob J) {
    const int n_obj = trk_objects(J);
    const int a = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= n_obj) return;
    const scvod_object& ra = J.objects[a];
    const int s = ra.scan;
    int nx = (unsigned)s < (unsigned)J.n_scans ? J.next[s] : -1;
    if (nx >= J.n_scans) nx = -1;
    unsigned long long key = 0ull;
    int b = -1;
    if (nx >= 0) {
        const int lo = max(J.obj_off[nx], 0), hi = min(J.obj_off[nx + 1], n_obj);
        const int a_cls = ra.cls;
        if (a_cls == 2) {  // overlap: the largest count among the car successors that A fills to the occupancy; ties to the smaller B
            unsigned long long best = 0ull;
            int c0 = 0, c1 = 0, base_n = 0, n_an = 0;
            const int2* list = nullptr;
            if (ARENA) {
                const int base = A.scan_off[s], n_a = A.counts[s * 8 + 4], name = ra.name;
                if ((unsigned)name < (unsigned)n_a && A.pt_type[(size_t)base + name] == 2 && A.pt_cluster[(size_t)base + name] == name) {
                    const int mb = A.tk_mbegin[(size_t)base + name], np = A.tk_npairs[(size_t)base + name];
                    if (mb >= 0 && np > 0 && mb + np <= n_a) {
                        list = A.tk_pairs + (size_t)base + mb;
                        c1 = np;
                    }
                }
                base_n = A.scan_off[nx];
                n_an = A.counts[nx * 8 + 4];
            } else if (J.cand_begin) {
                c0 = J.cand_begin[a];
                c1 = J.cand_begin[a + 1];
                list = J.cand;
            }
            for (int j = c0 + lane; j < c1; j += 64) {
                const int2 e = list[j];
                int cb = e.x;
                if (ARENA) cb = trk_is_root(A, base_n, n_an, e.x) ? J.root_obj[(size_t)base_n + e.x] : -1;
                if (cb < lo || cb >= hi || e.y < 0) continue;
                const scvod_object& rb = J.objects[cb];
                if (rb.cls != 2 || !((float)e.y / (float)rb.n_voxels >= J.occupancy)) continue;
                const unsigned long long k = ((unsigned long long)(unsigned)e.y << 32) | (unsigned)~cb;
                best = k > best ? k : best;
            }
            best = trk_wave_max(best);
            if (best) {
                b = (int)~(unsigned)best;
                key = (1ull << 63) | (best & 0x7fffffff00000000ull) | (unsigned)~a;
            }
        }
        if (b < 0 && !(J.flags & SCVOD_TRK_NO_GATE) && ((J.flags & SCVOD_TRK_ANY_CLASS) || a_cls == 2) && ra.n_points >= J.min_points) {
            // gate: the nearest world centre among the successor scan's objects of A's class and size; ties to the smaller B
            const float4 wa = J.cw[a];
            unsigned long long best = kTrkNone;
            for (int cb = lo + lane; cb < hi; cb += 64) {
                const scvod_object& rb = J.objects[cb];
                if (rb.cls != a_cls || rb.n_points < J.min_points) continue;
                const float4 wb = J.cw[cb];
                if (!(wa.w <= J.size_ratio * wb.w) || !(wb.w <= J.size_ratio * wa.w)) continue;
                const float d2 = trk_d2(wa, wb);
                if (!(d2 < J.gate2)) continue;
                const unsigned long long k = ((unsigned long long)f2u(d2) << 32) | (unsigned)cb;  // d2 >= 0: its bits order as it does
                best = k < best ? k : best;
            }
            best = trk_wave_min(best);
            if (best != kTrkNone) {
                b = (int)(unsigned)best;
                key = ((unsigned long long)(0x7fffffffu - (unsigned)(best >> 32)) << 32) | (unsigned)~a;
            }
        }
    }
    if (lane == 0) {
        J.prop_b[a] = b;
        J.prop_key[a] = key;
        // B accepts the largest key: kind 1 above kind 2, then the larger count / the smaller d2, then the smaller A.  0 is empty
        if (b >= 0) atomicMax(&J.slot[b], key);
    }
}

__global__ __launch_bounds__(256) void k_trk_confirm(TrkJob J) {
    const int n_obj = trk_objects(J);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n_obj;
    int kind = 0;
    bool refused = false;
    if (in) {
        const unsigned long long sk = J.slot[i];
        scvod_object_link L;
        L.track = -1;
        L.rank = 0;
        L.pred = -1;
        L.kind = 0;
        L.weight = 0;
        L.step = 0.f;
        L.reserved = 0;
        if (sk) {
            L.pred = (int)~(unsigned)sk;
            L.kind = kind = (sk >> 63) ? 1 : 2;
            L.weight = kind == 1 ? (int)((sk >> 32) & 0x7fffffffu) : 0;
            L.step = sqrt_f(trk_d2(J.cw[L.pred], J.cw[i]));
        }
        const int b = J.prop_b[i];
        const bool won = b >= 0 && J.slot[b] == J.prop_key[i];
        refused = b >= 0 && !won;
        L.succ = won ? b : -1;
        J.links[i] = L;
        J.rank[0][i] = L.pred >= 0 ? 1 : 0;
        J.jump[0][i] = L.pred >= 0 ? L.pred : i;
    }
    const int n1 = __popcll(__ballot(kind == 1)), n2 = __popcll(__ballot(kind == 2)), nr = __popcll(__ballot(refused));
    if ((threadIdx.x & 63) == 0) {
        if (n1) atomicAdd(&J.counters[kTrkStKind1], (unsigned long long)n1);
        if (n2) atomicAdd(&J.counters[kTrkStKind2], (unsigned long long)n2);
        if (nr) atomicAdd(&J.counters[kTrkStRefused], (unsigned long long)nr);
    }
}

// one round: rank += rank[jump]; jump = jump[jump].  A head has rank 0 and jumps to itself
__global__ __launch_bounds__(256) void k_trk_jump(TrkJob J, int from) {
    const int n_obj = trk_objects(J);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_obj) return;
    const int j = J.jump[from][i];
    J.rank[from ^ 1][i] = J.rank[from][i] + J.rank[from][j];
    J.jump[from ^ 1][i] = J.jump[from][j];
}

__global__ __launch_bounds__(256) void k_trk_chain(TrkJob J, int buf) {
    const int n_obj = trk_objects(J);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_obj) return;
    atomicMax(&J.chain[J.jump[buf][i]], ((unsigned long long)(unsigned)J.rank[buf][i] << 32) | (unsigned)i);
}

// over the whole capacity (the scan's length is the host's bound): listed heads carry (1, length), everything else 0
__global__ __launch_bounds__(256) void k_trk_flag(TrkJob J, int n) {
    const int n_obj = trk_objects(J);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned long long v = 0ull;
    if (i < n_obj && J.links[i].pred < 0) {
        const unsigned len = (unsigned)(J.chain[i] >> 32) + 1u;
        if ((int)len >= J.min_length) v = (1ull << 32) | len;
    }
    J.val[i] = v;
}

__global__ __launch_bounds__(256) void k_trk_scatter(TrkJob J, int buf) {
    const int n_obj = trk_objects(J);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_obj) return;
    const int h = J.jump[buf][i], r = J.rank[buf][i];
    int track = -1;
    if (J.val[h]) {
        const unsigned long long p = J.pre[h];
        track = (int)(p >> 32);
        const int at = (int)(unsigned)p + r;  // (< the objects: the runs of the listed tracks are disjoint)
        J.tobj[at] = i;
        if (J.out_tobj) J.out_tobj[at] = i;
        if (i == h) J.heads[track] = i;
    }
    if (J.out_links) {
        scvod_object_link L = J.links[i];
        L.track = track;
        L.rank = r;
        J.out_links[i] = L;
    }
}

__global__ __launch_bounds__(256) void k_trk_reduce(TrkJob J) {
    const int n_raw = J.obj_off[J.n_scans];
    const int n_obj = trk_objects(J);
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (n_obj < 0) {  // more objects than the caller vouched for
        if (first) {
            J.counters[kTrkStObjects] = (unsigned long long)(long long)n_raw;
            J.counters[kTrkStOverflow] = 1ull;
            if (J.n_tracks) J.n_tracks[0] = -1;
        }
        return;
    }
    const int n_trk = n_obj > 0 ? (int)((J.pre[n_obj - 1] + J.val[n_obj - 1]) >> 32) : 0;
    if (first) {
        const bool over = J.out_tracks && (long long)n_trk > J.cap_tracks;
        J.counters[kTrkStObjects] = (unsigned long long)n_obj;
        J.counters[kTrkStFound] = (unsigned long long)n_trk;
        J.counters[kTrkStWritten] = J.out_tracks ? (unsigned long long)(over ? J.cap_tracks : n_trk) : 0ull;
        J.counters[kTrkStOverflow] = over ? 1ull : 0ull;
        if (J.n_tracks) J.n_tracks[0] = over ? -1 : n_trk;
    }
    const int lane = threadIdx.x & 63;
    for (int t = blockIdx.x * 4 + ((int)threadIdx.x >> 6); t < n_trk; t += gridDim.x * 4) {
        const int h = J.heads[t];
        const unsigned long long ch = J.chain[h];
        const int len = (int)(ch >> 32) + 1, last = (int)(unsigned)ch, ob = (int)(unsigned)J.pre[h];
        int n_dyn = 0, n_gate = 0;
        float mx = 0.f, path = 0.f;
        for (int k0 = 0; k0 < len; k0 += 64) {
            const bool in = k0 + lane < len;
            float step = 0.f;
            if (in) {
                const int o = J.tobj[ob + k0 + lane];
                step = J.links[o].step;
                n_gate += J.links[o].kind == 2 ? 1 : 0;
                n_dyn += J.objects[o].dynamic == 1 ? 1 : 0;
                mx = step > mx ? step : mx;
            }
            const int cnt = min(64, len - k0);
            for (int k = 0; k < cnt; ++k) path += __shfl(step, k);  // the sequential sum in rank order, every lane the same
        }
        n_dyn = trk_wave_sum(n_dyn);
        n_gate = trk_wave_sum(n_gate);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const float o = __shfl_xor(mx, d);
            mx = o > mx ? o : mx;
        }
        if (lane == 0) {
            atomicMax(&J.counters[kTrkStLongest], (unsigned long long)len);
            if (J.out_tracks && (long long)t < J.cap_tracks) {
                const float4 w0 = J.cw[h], w1 = J.cw[last];
                scvod_track R;
                R.first_object = h;
                R.last_object = last;
                R.length = len;
                R.first_scan = J.objects[h].scan;
                R.last_scan = J.objects[last].scan;
                R.n_dynamic = n_dyn;
                R.n_gate_links = n_gate;
                R.object_begin = ob;
                R.net[0] = w1.x - w0.x;
                R.net[1] = w1.y - w0.y;
                R.net[2] = w1.z - w0.z;
                R.path = path;
                R.max_step = mx;
                R.reserved[0] = R.reserved[1] = R.reserved[2] = 0;
                J.out_tracks[t] = R;
            }
        }
    }
}

size_t trk_align(size_t v) { return (v + 255) / 256 * 256; }

size_t trk_scan_bytes(size_t n) {
    size_t bytes = 0;
    rocprim::exclusive_scan(nullptr, bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, n, rocprim::plus<unsigned long long>(),
                            (hipStream_t)0);
    return bytes;
}

}  // namespace

int trk_rounds(int n_scans) {
    int r = 1;
    while ((1 << r) < n_scans) ++r;
    return r;
}

size_t trk_tables_bytes(int n_scans) {
    const size_t B = (size_t)(n_scans > 0 ? n_scans : 0);
    return trk_align(sizeof(float) * 12 * B) + trk_align(sizeof(int32_t) * B) + trk_align(sizeof(int32_t) * (B + 1));
}

size_t trk_work_bytes(long long cap, int n_scans) {
    const size_t n = (size_t)(cap > 0 ? cap : 1);
    return trk_tables_bytes(n_scans) + trk_align(16 * n) + 5 * trk_align(8 * n) + trk_align(sizeof(scvod_object_link) * n) + 7 * trk_align(4 * n) +
           trk_align(trk_scan_bytes(n)) + 256;
}

// J: the caller's side filled in (objects, cap, candidates, flags and parameters, outputs, counters, n_scans; obj_off unless scan_cnt is
// given: then the offsets are made here).  work: trk_work_bytes bytes whose first trk_tables_bytes hold [T][next] already (staged by
// the caller); the counters were cleared on `st`
hipError_t launch_object_tracks(const Arena& A, TrkJob J, const int32_t* scan_cnt, void* work, hipStream_t st) {
    const size_t n = (size_t)(J.cap > 0 ? J.cap : 1), B = (size_t)(J.n_scans > 0 ? J.n_scans : 0);
    unsigned char* p = (unsigned char*)work;
    auto take = [&](size_t bytes) {
        unsigned char* q = p;
        p += trk_align(bytes);
        return q;
    };
    J.T = (const float*)take(sizeof(float) * 12 * B);
    J.next = (const int32_t*)take(sizeof(int32_t) * B);
    int32_t* off = (int32_t*)take(sizeof(int32_t) * (B + 1));
    J.cw = (float4*)take(16 * n);
    J.slot = (unsigned long long*)take(8 * n);
    J.prop_key = (unsigned long long*)take(8 * n);
    J.chain = (unsigned long long*)take(8 * n);
    J.val = (unsigned long long*)take(8 * n);
    J.pre = (unsigned long long*)take(8 * n);
    J.links = (scvod_object_link*)take(sizeof(scvod_object_link) * n);
    J.prop_b = (int32_t*)take(4 * n);
    J.rank[0] = (int32_t*)take(4 * n);
    J.rank[1] = (int32_t*)take(4 * n);
    J.jump[0] = (int32_t*)take(4 * n);
    J.jump[1] = (int32_t*)take(4 * n);
    J.tobj = (int32_t*)take(4 * n);
    J.heads = (int32_t*)take(4 * n);
    void* scan_tmp = p;
    size_t scan_bytes = trk_scan_bytes(n);
    if (scan_cnt) {
        k_trk_offsets<<<1, 1024, 0, st>>>(scan_cnt, off, J.n_scans);
        J.obj_off = off;
    }
    const int g256 = (int)((n + 255) / 256), g4 = (int)((n + 3) / 4);
    k_trk_world<<<g256, 256, 0, st>>>(J);
    if (J.root_obj)
        k_trk_link<true><<<g4, 256, 0, st>>>(A, J);
    else
        k_trk_link<false><<<g4, 256, 0, st>>>(A, J);
    k_trk_confirm<<<g256, 256, 0, st>>>(J);
    const int rounds = trk_rounds(J.n_scans);
    for (int r = 0; r < rounds; ++r) k_trk_jump<<<g256, 256, 0, st>>>(J, r & 1);
    const int buf = rounds & 1;
    k_trk_chain<<<g256, 256, 0, st>>>(J, buf);
    k_trk_flag<<<g256, 256, 0, st>>>(J, (int)n);
    const hipError_t e = rocprim::exclusive_scan(scan_tmp, scan_bytes, J.val, J.pre, 0ull, n, rocprim::plus<unsigned long long>(), st);
    if (e != hipSuccess) return e;
    k_trk_scatter<<<g256, 256, 0, st>>>(J, buf);
    k_trk_reduce<<<g4 < 2048 ? g4 : 2048, 256, 0, st>>>(J);
    return hipGetLastError();
}

}  // namespace scvod

extern "C" {

void scvod_track_params_default(scvod_track_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->flags = 0;
    p->occupancy = -1.f;
    p->gate = 2.0f;
    p->size_ratio = 1.5f;
    p->min_points = 10;
    p->min_length = 2;
}

// Host only, in double.  A track moves iff sqrt(net . net) >= min_travel
int scvod_tracks_finish(const scvod_track* tracks, int64_t n, double min_travel, scvod_tracks_result* out) {
    if (!out || n < 0 || (n > 0 && !tracks)) return SCVOD_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    for (int64_t t = 0; t < n; ++t) {
        const double x = (double)tracks[t].net[0], y = (double)tracks[t].net[1], z = (double)tracks[t].net[2];
        const bool moving = std::sqrt(x * x + y * y + z * z) >= min_travel;
        ++out->tracks;
        if (moving) {
            ++out->moving_tracks;
            out->moving_members += tracks[t].length;
            out->moving_members_dynamic += tracks[t].n_dynamic;
        } else {
            ++out->still_tracks;
            out->still_members += tracks[t].length;
            out->still_members_dynamic += tracks[t].n_dynamic;
        }
    }
    const double nan = std::nan("");
    const int64_t along = out->moving_members - out->moving_tracks;  // the last member of a track has no successor: it is never dynamic
    out->recall_along = along != 0 ? 100.0 * (double)out->moving_members_dynamic / (double)along : nan;
    out->false_alarm = out->still_members != 0 ? 100.0 * (double)out->still_members_dynamic / (double)out->still_members : nan;
    return SCVOD_OK;
}

}  // extern "C"
