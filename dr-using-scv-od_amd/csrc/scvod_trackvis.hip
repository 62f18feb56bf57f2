// scvod_trackvis.hip -- the tracks of a batch vote on the seen-through verdict (gfx950): scvod_track_visibility_device
// (include/scvod.h; the rule: DESIGN.md section 2).
//
// Reference analogue: none.  Everything read is the caller's: the object table, its offsets, the link / track / track-object tables of
// the tracks stage, optionally the records of the objects' vote, and one int32 and one byte per input point.
//     k_tv_world    per object: world centre (k_trk_world's expression, restated); clears the object's verdict byte; the counts
//     k_tv_member   per object: its track and rank, the two clamped look-ups into the track-object list, travel2, moved, flagged
//     k_tv_track    one wave per listed track over its contiguous run, 64 members a round: ballot / popcount sums, the integer max of
//                   the float image of travel2, the decision, the track record
//     k_tv_spread   per object: the verdict by the precedence motion > vote > clear, the object record, one verdict byte in scratch
//     k_tv_paint    the hot path: streams over the input points, 16 consecutive points a lane (four 16-byte loads of object indices,
//                   one 16-byte load and one 16-byte store of bytes), a byte gather of the object's verdict that stays in cache
// Nothing waits for another workgroup; launch sizes come from the caller's capacities, the true counts are read on the device.
// Integer atomics (add, or) and fixed-order float expressions only: every output is the same bit for bit on every run and for any
// launch geometry.  Nothing read from a table is used as an index unchecked.
#include <hip/hip_runtime.h>

#include <cstring>

#include "scvod_dev.h"
#include "scvod_math.h"

namespace scvod {
namespace {

constexpr unsigned char kTvNone = 0xFF;  // verdict byte of an object without a verdict
enum { kTvOk = 0, kTvShort = 1, kTvRefused = 2 };

// what the device reads of the tables' sizes.  up: upstream overflow (then n_obj = n_trk = 0 and no object gets a verdict);
// rec_over: a record buffer is too small (then no byte of the per-point output changes)
struct TvState {
    int n_obj, n_trk, raw_obj, raw_trk;
    bool up, rec_over;
};
__device__ __forceinline__ TvState tv_state(const TvJob& J) {
    TvState S;
    S.raw_obj = J.obj_off[J.n_scans];
    S.raw_trk = J.n_tracks[0];
    S.up = S.raw_obj < 0 || (long long)S.raw_obj > J.cap || S.raw_trk < 0 || (long long)S.raw_trk > J.cap_tracks;
    S.n_obj = S.up ? 0 : S.raw_obj;
    S.n_trk = S.up ? 0 : S.raw_trk;
    S.rec_over = !S.up && ((J.out_tracks && (long long)S.n_trk > J.cap_tvotes) || (J.out_objs && (long long)S.n_obj > J.cap_ovotes));
    return S;
}

__device__ __forceinline__ int tv_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// (dx*dx + dy*dy) + dz*dz in fp32
__device__ __forceinline__ float tv_d2(const float4& a, const float4& b) {
    const float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// launched over cap + 1 threads: slot J.cap of the verdict bytes is the one every point without an object reads
__global__ __launch_bounds__(256) void k_tv_world(TvJob J) {
    const TvState S = tv_state(J);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        J.counters[kTvStObjects] = (unsigned long long)(long long)S.raw_obj;
        J.counters[kTvStTracks] = (unsigned long long)(long long)S.raw_trk;
        const unsigned long long latch = (S.up ? 2ull : 0ull) | (S.rec_over ? 1ull : 0ull);
        if (latch) atomicOr(&J.counters[kTvStLatch], latch);
        J.vb[J.cap] = kTvNone;
    }
    if (i >= S.n_obj) return;
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
    J.cw[i] = w;
    J.vb[i] = kTvNone;
}

__global__ __launch_bounds__(256) void k_tv_member(TvJob J) {
    const TvState S = tv_state(J);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S.n_obj) return;
    bool flagged = !(J.flags & SCVOD_TRKVIS_NO_DYNAMIC) && J.objects[i].dynamic == 1;
    if (J.ovis && J.ovis[i].verdict == SCVOD_VIS_SEEN_THROUGH) flagged = true;
    const int t = J.links[i].track, r = J.links[i].rank;
    float trav = 0.f;
    bool moved = false;
    if (t >= 0 && t < S.n_trk) {
        const int L = J.tracks[t].length, ob = J.tracks[t].object_begin;
        if (L >= J.min_length && ob >= 0 && (long long)ob + L <= J.cap && r >= 0 && r < L) {
            const int w = J.window;
            const int ia = w == 0 ? 0 : max(r - w, 0);
            const int ib = w == 0 ? L - 1 : (int)min((long long)r + w, (long long)L - 1);
            const int a = J.tobj[ob + ia], b = J.tobj[ob + ib];
            if ((unsigned)a < (unsigned)S.n_obj && (unsigned)b < (unsigned)S.n_obj) {
                trav = tv_d2(J.cw[a], J.cw[b]);
                moved = trav >= J.travel2_min;  // (false for NaN)
            }
        }
    }
    J.trav[i] = trav;
    J.mf[i] = (unsigned char)((flagged ? 1 : 0) | (moved ? 2 : 0));
}

__global__ __launch_bounds__(256) void k_tv_track(TvJob J) {
    const TvState S = tv_state(J);
    const int lane = threadIdx.x & 63;
    int n_how1 = 0;
    bool any_refused = false;
    for (int t = blockIdx.x * 4 + ((int)threadIdx.x >> 6); t < S.n_trk; t += gridDim.x * 4) {
        const int L = J.tracks[t].length, ob = J.tracks[t].object_begin;
        int state = kTvOk, nf = 0, nm = 0;
        unsigned mx = 0u;
        if (L < J.min_length) {
            state = kTvShort;
        } else if (ob < 0 || (long long)ob + L > J.cap) {
            state = kTvRefused;
        } else {
            bool bad = false;
            for (int k0 = 0; k0 < L; k0 += 64) {
                const bool in = k0 + lane < L;
                int m = 0;
                if (in) {
                    const int o = J.tobj[ob + k0 + lane];
                    if ((unsigned)o < (unsigned)S.n_obj) {
                        m = J.mf[o];
                        const float tr = J.trav[o];
                        if (tr == tr) mx = max(mx, f2u(tr));  // travel2 >= 0: its bits order as it does
                    } else {
                        bad = true;
                    }
                }
                nf += __popcll(__ballot(m & 1));
                nm += __popcll(__ballot(m & 2));
            }
            if (__ballot(bad)) state = kTvRefused;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, d));
        }
        int verdict = -1, how = 0;
        if (state == kTvOk) {
            if (nf >= J.min_flagged && (long long)nf * J.vote_den >= (long long)J.vote_num * L) {
                verdict = SCVOD_VIS_SEEN_THROUGH;
                how = 1;
            } else if (J.flags & SCVOD_TRKVIS_CLEAR) {
                verdict = SCVOD_VIS_KEEP;
                how = 3;
            }
        } else {
            nf = nm = 0;
            mx = 0u;
        }
        n_how1 += how == 1 ? 1 : 0;
        any_refused |= state == kTvRefused;
        if (lane == 0) {
            J.tdec[t] = make_int4(state, how, nm, 0);
            if (J.out_tracks && (long long)t < J.cap_tvotes) {
                scvod_track_vote R;
                R.length = L;
                R.n_flagged = nf;
                R.n_moved = nm;
                R.verdict = verdict;
                R.how = how;
                R.max_travel2 = u2f(mx);
                R.reserved[0] = R.reserved[1] = 0;
                J.out_tracks[t] = R;
            }
        }
    }
    if (lane == 0) {
        if (n_how1) atomicAdd(&J.counters[kTvStVoted], (unsigned long long)n_how1);
        if (any_refused) atomicOr(&J.counters[kTvStLatch], 8ull);
    }
}

__global__ __launch_bounds__(256) void k_tv_spread(TvJob J) {
    const TvState S = tv_state(J);
    const int i = blockIdx.x * 256 + threadIdx.x;
    int how = 0;
    bool bad = false;
    if (i < S.n_obj) {
        const int t = J.links[i].track;
        int track = -1, verdict = -1;
        float trav = 0.f;
        if (t < -1 || t >= S.n_trk) {
            bad = true;
        } else if (t >= 0) {
            const int4 d = J.tdec[t];
            if (d.x == kTvShort) {
                track = t;
            } else if (d.x == kTvOk) {
                const int r = J.links[i].rank;
                if (r < 0 || r >= J.tracks[t].length) {
                    bad = true;
                } else {
                    track = t;
                    trav = J.trav[i];
                    if ((J.mf[i] & 2) && (J.window > 0 || d.z >= J.min_moved)) {
                        verdict = SCVOD_VIS_SEEN_THROUGH;
                        how = 2;
                    } else if (d.y == 1) {
                        verdict = SCVOD_VIS_SEEN_THROUGH;
                        how = 1;
                    } else if (d.y == 3) {
                        verdict = SCVOD_VIS_KEEP;
                        how = 3;
                    }
                }
            }
        }
        if (verdict >= 0) J.vb[i] = (unsigned char)verdict;
        if (J.out_objs && (long long)i < J.cap_ovotes) {
            scvod_object_track_vote R;
            R.track = track;
            R.verdict = verdict;
            R.how = how;
            R.travel2 = trav;
            J.out_objs[i] = R;
        }
    }
    const int n2 = __popcll(__ballot(how == 2)), n3 = __popcll(__ballot(how == 3));
    const bool nb = __ballot(bad) != 0ull;
    if ((threadIdx.x & 63) == 0) {
        if (n2) atomicAdd(&J.counters[kTvStMotion], (unsigned long long)n2);
        if (n3) atomicAdd(&J.counters[kTvStCleared], (unsigned long long)n3);
        if (nb) atomicOr(&J.counters[kTvStLatch], 8ull);
    }
}

// One point: the verdict byte of its object, or the input byte.  slot: the object's index, or J.cap (no verdict) for -1 and for an
// entry outside the table, which is counted in `broken`
__device__ __forceinline__ int tv_slot(int o, int n_obj, int none, bool& broken) {
    if ((unsigned)o < (unsigned)n_obj) return o;
    broken |= o != -1;
    return none;
}

__global__ __launch_bounds__(256) void k_tv_paint(TvJob J) {
    __shared__ int red[3][4];
    const TvState S = tv_state(J);
    if (S.rec_over) return;  // (the whole grid alike)
    const int n_obj = S.n_obj, none = (int)J.cap;
    const long long n = J.n_points;
    const long long head = min(n, (long long)((0 - (uintptr_t)J.out) & 15u));
    const long long chunks = (n - head) >> 4, tail = head + (chunks << 4);
    int to_seen = 0, to_keep = 0;
    bool broken = false;
    if (blockIdx.x == 0) {  // the points in front of the first and behind the last 16-byte block of the output, one a thread
        long long i = -1;
        if ((long long)threadIdx.x < head) i = threadIdx.x;
        if (threadIdx.x >= 64 && tail + (threadIdx.x - 64) < n) i = tail + (threadIdx.x - 64);
        if (i >= 0) {
            const unsigned in = J.verdict ? J.verdict[i] : (unsigned)SCVOD_VIS_UNTESTED;
            const unsigned v = J.vb[tv_slot(J.point_object[i], n_obj, none, broken)];
            to_seen += (v == SCVOD_VIS_SEEN_THROUGH && in != SCVOD_VIS_SEEN_THROUGH) ? 1 : 0;
            to_keep += (v == SCVOD_VIS_KEEP && in != SCVOD_VIS_KEEP) ? 1 : 0;
            J.out[i] = (unsigned char)(v != kTvNone ? v : in);
        }
    }
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (long long)gridDim.x * 256) {
        const long long base = head + (c << 4);
        int o[16];
        unsigned in4[4] = {0u, 0u, 0u, 0u};  // SCVOD_VIS_UNTESTED
        __builtin_memcpy(o, J.point_object + base, 64);  // (4-byte aligned: the caller's pointer)
        if (J.verdict) __builtin_memcpy(in4, J.verdict + base, 16);  // (any address)
        unsigned v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = J.vb[tv_slot(o[k], n_obj, none, broken)];
        unsigned out4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned w = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned in = (in4[q] >> (8 * b)) & 0xFFu, g = v[4 * q + b];
                to_seen += (g == SCVOD_VIS_SEEN_THROUGH && in != SCVOD_VIS_SEEN_THROUGH) ? 1 : 0;
                to_keep += (g == SCVOD_VIS_KEEP && in != SCVOD_VIS_KEEP) ? 1 : 0;
                w |= (g != kTvNone ? g : in) << (8 * b);
            }
            out4[q] = w;
        }
        *reinterpret_cast<uint4*>(J.out + base) = make_uint4(out4[0], out4[1], out4[2], out4[3]);  // 16-byte aligned by the head
    }
    to_seen = tv_wave_sum(to_seen);
    to_keep = tv_wave_sum(to_keep);
    const int nb = __ballot(broken) != 0ull ? 1 : 0;
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = to_seen;
        red[1][wave] = to_keep;
        red[2][wave] = nb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int a = red[0][0] + red[0][1] + red[0][2] + red[0][3], b = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        if (a) atomicAdd(&J.counters[kTvStToSeen], (unsigned long long)a);
        if (b) atomicAdd(&J.counters[kTvStToKeep], (unsigned long long)b);
        if (!S.up && (red[2][0] | red[2][1] | red[2][2] | red[2][3])) atomicOr(&J.counters[kTvStLatch], 4ull);
    }
}

size_t tv_align(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

size_t tv_tables_bytes(int n_scans) { return tv_align(sizeof(float) * 12 * (size_t)(n_scans > 0 ? n_scans : 0)); }

size_t tv_work_bytes(long long cap, long long cap_tracks, int n_scans) {
    const size_t n = (size_t)(cap > 0 ? cap : 0) + 1, nt = (size_t)(cap_tracks > 0 ? cap_tracks : 1);
    return tv_tables_bytes(n_scans) + tv_align(16 * n) + tv_align(4 * n) + 2 * tv_align(n) + tv_align(16 * nt);
}

// J: the caller's side filled in.  work: tv_work_bytes bytes whose first tv_tables_bytes hold the pose matrices already (staged by the
// caller); the counters were cleared on `st`
hipError_t launch_track_visibility(TvJob J, void* work, hipStream_t st) {
    const size_t n = (size_t)(J.cap > 0 ? J.cap : 0) + 1, nt = (size_t)(J.cap_tracks > 0 ? J.cap_tracks : 1);
    unsigned char* p = (unsigned char*)work;
    auto take = [&](size_t bytes) {
        unsigned char* q = p;
        p += tv_align(bytes);
        return q;
    };
    J.T = (const float*)take(sizeof(float) * 12 * (size_t)(J.n_scans > 0 ? J.n_scans : 0));
    J.cw = (float4*)take(16 * n);
    J.trav = (float*)take(4 * n);
    J.mf = take(n);
    J.vb = take(n);
    J.tdec = (int4*)take(16 * nt);
    const int g256 = (int)((n + 255) / 256), g4 = (int)((nt + 3) / 4);
    k_tv_world<<<g256, 256, 0, st>>>(J);
    k_tv_member<<<g256, 256, 0, st>>>(J);
    k_tv_track<<<g4 < 2048 ? g4 : 2048, 256, 0, st>>>(J);
    k_tv_spread<<<g256, 256, 0, st>>>(J);
    if (J.out && J.n_points > 0) {
        const long long blocks = (J.n_points / 16 + 255) / 256 + 1;
        k_tv_paint<<<(int)(blocks < 2048 ? blocks : 2048), 256, 0, st>>>(J);
    }
    return hipGetLastError();
}

}  // namespace scvod

extern "C" {

void scvod_track_visibility_params_default(scvod_track_visibility_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->flags = 0;
    p->window = 0;
    p->min_travel = 2.0f;
    p->min_length = 2;
    p->min_moved = 1;
    p->min_flagged = 2;
    p->vote_num = 1;
    p->vote_den = 2;
}

}  // extern "C"
