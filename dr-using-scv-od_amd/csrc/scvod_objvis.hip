// scvod_objvis.hip -- the objects of a batch vote on the seen-through verdict, on the device (gfx950): scvod_batch_object_visibility.
//
// Reference analogue: none.  No program of the reference joins free-space evidence with its clusters; the rule and its defaults are this
// project's convention.  The device part is a segmented sum over the sorted member list scvod_batch_objects left in
// its scratch -- key_out[p] = object << 32 | batch slot, begin[o] the first position of object o -- cut into tiles of SCVOD_OBJVIS_TILE
// consecutive POSITIONS, not into objects: the K64 table's largest object has 35 537 members, the OS128 table's 136 320, and a wave that
// owns a whole object (k_mf_vote, k_ot_objects) walks those alone.
//     k_ov_tiles      a workgroup per tile, a wave per 512 positions.  The wave issues the gathers of its eight rounds of 64 positions
//                     at once (key -> apri_src -> verdict byte and vote word; the scan of the range by one wave-wide search in scan_off, a
//                     per-lane step only where the range crosses a scan), then walks the objects that overlap its range round by
//                     round: the two counted bytes by ballot + popcount under the object's lane mask, the four byte sums of the vote word
//                     as differences of one packed inclusive wave scan per round.  An object inside the wave's range is finished there:
//                     verdict, record, the new byte of its lanes.  An object that crosses the range adds its partial counts into one of
//                     five LDS slots of the workgroup (the slot of the wave in whose range it begins; slot 4: it begins before the tile);
//                     behind one barrier the waves that hold a piece of an object inside the tile read the slot's totals and finish it,
//                     and the slots of the (at most two) objects that cross a tile edge are added, word by word, to the global accumulator
//                     of the tile in which the object BEGINS.  At most one object begins in a tile and leaves it, so the accumulators are
//                     8 words per tile and nothing per object.  Every lane then stores the bytes that changed
//     k_ov_straddle   the same tiles again, in a second launch: a tile looks at the object of its first and of its last position; one that
//                     crosses a tile edge has its totals in the accumulator of tile begin / TILE.  Every tile it touches takes the same
//                     verdict from the same integers; the tile in which it begins writes the record and the stats; each tile rewrites
//                     its own piece
// No workgroup waits for another, there is no grid barrier and no residency assumption: the launch boundary orders the accumulators.  In
// place (out == verdict) a byte is read by the one wave that owns its position, before that wave or any later launch writes it.  All sums
// are integers: the same bytes on every run.  The stats are kept per wave and added once per wave.
#include <hip/hip_runtime.h>

#include "scvod_dev.h"

namespace scvod {
namespace {

constexpr int kOvTile = SCVOD_OBJVIS_TILE;
constexpr int kOvRounds = 8;              // rounds of 64 positions per wave
constexpr int kOvWave = 64 * kOvRounds;   // positions per wave
static_assert(kOvTile == 4 * kOvWave, "a tile is four waves of eight rounds");
// the words of a slot / an accumulator
enum { kOvKeep = 0, kOvSeen, kOvThrough, kOvAgree, kOvOccluded, kOvOther, kOvWords = 8 };

struct OvSum {
    unsigned w[6];
};

// per wave (kept by the lane that publishes), added once at the end
struct OvStats {
    unsigned long long voted = 0, forced = 0, seen = 0, moved_seen = 0, moved_keep = 0;
};

// the scan that holds batch slot g (the same in every lane of a full wave): the last s with scan_off[s] <= g.  The 64 lanes probe 64
// evenly spaced entries per step, so the bench jobs' 1000 to 2761 scans take two dependent loads, not eleven
__device__ __forceinline__ int ov_scan_of(const Arena& A, int n_scans, int g, int lane) {
    int lo = 0, hi = n_scans;  // scan_off[lo] <= g, and hi == n_scans or scan_off[hi] > g
    while (hi - lo > 1) {
        const int step = (hi - lo + 63) / 64;
        const long long probe = (long long)lo + (long long)(lane + 1) * step;
        const bool le = probe < hi && A.scan_off[probe] <= g;
        const int k = __popcll(__ballot(le));  // (the probes ascend and so does scan_off: the lanes that say yes are a prefix)
        lo += k * step;
        hi = min(hi, lo + step);
    }
    return lo;
}

// the rule of the header: verdict and how of object o from its totals
__device__ __forceinline__ void ov_decide(const ObjVisJob& J, long long o, int n_points, const OvSum& s, int& verdict, int& how) {
    const long long t = J.pool ? (long long)(int32_t)s.w[kOvThrough] : (long long)s.w[kOvSeen];
    const long long a = J.pool ? (long long)(int32_t)s.w[kOvAgree] : (long long)s.w[kOvKeep];
    const bool votes = n_points >= J.min_points && (long long)s.w[kOvKeep] + (long long)s.w[kOvSeen] >= (long long)J.min_tested;
    const bool through = t >= (long long)J.min_through && t * J.vote_den >= (long long)J.vote_num * (t + a);
    if (J.obj_bytes && J.obj_bytes[(size_t)o * sizeof(scvod_object) + offsetof(scvod_object, dynamic)] == 1) {
        verdict = SCVOD_VIS_SEEN_THROUGH;
        how = 2;
    } else if (votes) {
        verdict = through ? SCVOD_VIS_SEEN_THROUGH : SCVOD_VIS_KEEP;
        how = 1;
    } else {
        verdict = -1;
        how = 0;
    }
}

// one lane: the record of object o and its share of the stats
__device__ __forceinline__ void ov_publish(const ObjVisJob& J, long long o, int n_points, const OvSum& s, int verdict, int how, OvStats& st) {
    if (how == 1) ++st.voted;
    if (how == 2) ++st.forced;
    if (how != 0 && verdict == SCVOD_VIS_SEEN_THROUGH) {
        ++st.seen;
        st.moved_seen += (unsigned long long)(n_points - (int)s.w[kOvSeen]);
    }
    if (how != 0 && verdict == SCVOD_VIS_KEEP) st.moved_keep += (unsigned long long)(n_points - (int)s.w[kOvKeep]);
    if (J.rec && o < J.cap) {
        scvod_object_visibility r;
        r.n_points = n_points;
        r.n_untested = n_points - (int)s.w[kOvKeep] - (int)s.w[kOvSeen];
        r.n_keep = (int32_t)s.w[kOvKeep];
        r.n_seen = (int32_t)s.w[kOvSeen];
        r.sum_through = (int32_t)s.w[kOvThrough];
        r.sum_agree = (int32_t)s.w[kOvAgree];
        r.sum_occluded = (int32_t)s.w[kOvOccluded];
        r.sum_other = (int32_t)s.w[kOvOther];
        r.verdict = verdict;
        r.how = how;
        r.reserved[0] = r.reserved[1] = 0;
        J.rec[o] = r;
    }
}

__device__ __forceinline__ void ov_add_stats(const ObjVisJob& J, const OvStats& st) {
    if (st.voted) atomicAdd(&J.counters[kOvStVoted], st.voted);
    if (st.forced) atomicAdd(&J.counters[kOvStForced], st.forced);
    if (st.seen) atomicAdd(&J.counters[kOvStSeen], st.seen);
    if (st.moved_seen) atomicAdd(&J.counters[kOvStMovedSeen], st.moved_seen);
    if (st.moved_keep) atomicAdd(&J.counters[kOvStMovedKeep], st.moved_keep);
}

// the lanes [l0, l1) of a round, 0 <= l0 < l1 <= 64
__device__ __forceinline__ unsigned long long ov_mask(int l0, int l1) {
    const unsigned long long upto = l1 >= 64 ? ~0ull : (1ull << l1) - 1ull;
    return upto & ~((1ull << l0) - 1ull);
}

__global__ __launch_bounds__(256) void k_ov_tiles(Arena A, ObjVisJob J, int n_scans) {
    __shared__ unsigned slot_sum[5][kOvWords];
    __shared__ int slot_tile[5];  // 1 + the tile whose accumulator the slot's object adds into; 0: the object lies inside this tile
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long n_obj = J.tab_stats[1];
    const int M = (int)J.tab_stats[2];  // members of the table: positions of the list
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        J.counters[kOvStObjects] = (unsigned long long)n_obj;
        J.counters[kOvStWritten] = J.rec ? (unsigned long long)(n_obj < J.cap ? n_obj : J.cap) : 0ull;
        J.counters[kOvStOverflow] = (J.rec && n_obj > J.cap) ? 1ull : 0ull;
    }
    const long long t0l = (long long)blockIdx.x * kOvTile;
    if (t0l >= (long long)M) return;  // (the grid is sized from the batch's points; the table's members are fewer)
    const int t0 = (int)t0l;
    const long long t1 = t0l + kOvTile;
    if (threadIdx.x < 5 * kOvWords) (&slot_sum[0][0])[threadIdx.x] = 0u;
    if (threadIdx.x < 5) slot_tile[threadIdx.x] = 0;
    __syncthreads();
    const int w0 = t0 + w * kOvWave;
    const int w1 = (int)min((long long)w0 + kOvWave, (long long)M);
    const bool live = w0 < M;  // (wave-uniform; a wave without positions still meets the barrier)
    int idx[kOvRounds];        // the input point of the lane's position in round r, -1: none
    unsigned v[kOvRounds], nv[kOvRounds];
    OvStats st;
    // the (at most two) objects of this wave's range that cross it: `in` begins before w0, `out` begins inside and ends behind w1
    int in_o = -1, in_b = 0, in_e = 0, out_o = -1, out_b = 0, out_e = 0;
    if (live) {
        uint64_t key[kOvRounds];
#pragma unroll
        for (int r = 0; r < kOvRounds; ++r) {
            const int p = w0 + 64 * r + lane;
            key[r] = p < w1 ? J.key_out[p] : 0ull;
        }
        const uint64_t key_last = J.key_out[w1 - 1];
        int src[kOvRounds];
#pragma unroll
        for (int r = 0; r < kOvRounds; ++r) {
            const int p = w0 + 64 * r + lane;
            src[r] = p < w1 ? A.apri_src[(uint32_t)key[r]] : -1;
        }
        // the list is in table order, scans ascending: the scans of the wave's range lie in [s_lo, s_hi], nearly always one scan
        const int s_lo = ov_scan_of(A, n_scans, __builtin_amdgcn_readfirstlane((int)(uint32_t)key[0]), lane);
        const int base_lo = A.scan_off[s_lo], end_lo = A.scan_off[s_lo + 1];
        const int s_hi = (int)(uint32_t)key_last < end_lo ? s_lo : ov_scan_of(A, n_scans, (int)(uint32_t)key_last, lane);
        unsigned q[kOvRounds];
#pragma unroll
        for (int r = 0; r < kOvRounds; ++r) {
            const int g = (int)(uint32_t)key[r];
            int base = base_lo, end = end_lo;
            if (s_hi != s_lo && g >= end_lo) {
                int s = s_lo + 1;
                while (s < s_hi && g >= A.scan_off[s + 1]) ++s;
                base = A.scan_off[s];
                end = A.scan_off[s + 1];
            }
            idx[r] = (unsigned)src[r] < (unsigned)(end - base) ? base + src[r] : -1;  // (src -1 behind the range: none)
        }
#pragma unroll
        for (int r = 0; r < kOvRounds; ++r) {
            v[r] = idx[r] >= 0 ? (unsigned)J.verdict[(size_t)idx[r]] : 0xFFu;
            q[r] = (J.votes && idx[r] >= 0) ? J.votes[(size_t)idx[r]] : 0u;
            nv[r] = v[r];
        }
        // the walk: the objects in ascending order, the rounds in ascending order; begin[] of up to 63 objects sits in the lanes
        long long o = (long long)(key[0] >> 32);
        o = ((long long)__builtin_amdgcn_readfirstlane((int)(o >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)o);
        long long ob = o;
        int bl = J.begin[min(ob + lane, n_obj)];
        OvSum acc = {{0u, 0u, 0u, 0u, 0u, 0u}};
        auto finish = [&](int b, int e) {  // the counts of [max(b, w0), min(e, w1)) of object o are in acc
            if (b >= w0 && e <= w1) {
                int verdict, how;
                ov_decide(J, o, e - b, acc, verdict, how);
                if (lane == 0) ov_publish(J, o, e - b, acc, verdict, how, st);
                if (how != 0) {
#pragma unroll
                    for (int r = 0; r < kOvRounds; ++r) {
                        const int p = w0 + 64 * r + lane;
                        if (p >= b && p < e) nv[r] = (unsigned)verdict;
                    }
                }
            } else {
                const int slot = b < t0 ? 4 : (b - t0) / kOvWave;
                if (lane == 0) {
#pragma unroll
                    for (int k = 0; k < 6; ++k)
                        if (acc.w[k]) atomicAdd(&slot_sum[slot][k], acc.w[k]);
                    if (b < t0 || (long long)e > t1) slot_tile[slot] = 1 + b / kOvTile;  // (every wave with a piece stores the same value)
                }
                if (b < w0)
                    in_o = (int)o, in_b = b, in_e = e;
                else
                    out_o = (int)o, out_b = b, out_e = e;
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) acc.w[k] = 0u;
        };
        int b = 0, e = 0;
        bool open = false;  // acc holds a piece of object o = [b, e) that goes on behind the round
#pragma unroll
        for (int r = 0; r < kOvRounds; ++r) {
            const int r0 = w0 + 64 * r;
            if (r0 < w1) {
                const int r1 = min(r0 + 64, w1);
                const unsigned long long b_seen = __ballot(v[r] == (unsigned)SCVOD_VIS_SEEN_THROUGH);
                const unsigned long long b_keep = __ballot(v[r] == (unsigned)SCVOD_VIS_KEEP);
                int pre_ta = 0, pre_oo = 0;  // inclusive prefixes over the lanes: through | agree << 16, occluded | other << 16 (64 * 255 < 2^16)
                if (J.votes) {
                    pre_ta = wave_incl_scan((int)((q[r] & 0xFFu) | ((q[r] & 0xFF00u) << 8)));
                    pre_oo = wave_incl_scan((int)(((q[r] >> 16) & 0xFFu) | ((q[r] >> 24) << 16)));
                }
                while (o < n_obj) {
                    if (!open) {
                        if (o - ob >= 63) {
                            ob = o;
                            bl = J.begin[min(ob + lane, n_obj)];
                        }
                        b = __builtin_amdgcn_readlane(bl, (int)(o - ob));
                        e = __builtin_amdgcn_readlane(bl, (int)(o - ob) + 1);
                    }
                    if (b >= r1) break;
                    const int l0 = max(b, r0) - r0, l1 = min(e, r1) - r0;
                    if (l1 <= l0) break;  // (never: a run has at least one member)
                    const unsigned long long m = ov_mask(l0, l1);
                    acc.w[kOvSeen] += (unsigned)__popcll(b_seen & m);
                    acc.w[kOvKeep] += (unsigned)__popcll(b_keep & m);
                    if (J.votes) {
                        unsigned ta = (unsigned)__builtin_amdgcn_readlane(pre_ta, l1 - 1), oo = (unsigned)__builtin_amdgcn_readlane(pre_oo, l1 - 1);
                        if (l0 > 0) {
                            ta -= (unsigned)__builtin_amdgcn_readlane(pre_ta, l0 - 1);
                            oo -= (unsigned)__builtin_amdgcn_readlane(pre_oo, l0 - 1);
                        }
                        acc.w[kOvThrough] += ta & 0xFFFFu;
                        acc.w[kOvAgree] += ta >> 16;
                        acc.w[kOvOccluded] += oo & 0xFFFFu;
                        acc.w[kOvOther] += oo >> 16;
                    }
                    open = e > r1;
                    if (open) break;
                    finish(b, e);
                    ++o;
                }
            }
        }
        if (open) finish(b, e);  // (the object goes on behind the wave's range)
    }
    __syncthreads();
    if (live) {
        // the objects that cross this wave's range and lie inside the tile: every wave with a piece takes the same verdict from the
        // slot's totals; the wave in whose range the object begins publishes it
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int o = k ? out_o : in_o, b = k ? out_b : in_b, e = k ? out_e : in_e;
            if (o < 0 || b < t0 || (long long)e > t1) continue;
            const int slot = (b - t0) / kOvWave;
            OvSum s;
#pragma unroll
            for (int j = 0; j < 6; ++j) s.w[j] = slot_sum[slot][j];
            int verdict, how;
            ov_decide(J, o, e - b, s, verdict, how);
            if (k == 1 && lane == 0) ov_publish(J, o, e - b, s, verdict, how, st);
            if (how != 0) {
#pragma unroll
                for (int r = 0; r < kOvRounds; ++r) {
                    const int p = w0 + 64 * r + lane;
                    if (p >= b && p < e) nv[r] = (unsigned)verdict;
                }
            }
        }
        if (J.out) {
#pragma unroll
            for (int r = 0; r < kOvRounds; ++r)
                if (idx[r] >= 0 && nv[r] != v[r]) J.out[(size_t)idx[r]] = (uint8_t)nv[r];
        }
        if (lane == 0) ov_add_stats(J, st);
    }
    // the objects that cross a tile edge: their partial counts into the accumulator of the tile in which they begin
    if (threadIdx.x < 5 * kOvWords) {
        const int slot = threadIdx.x / kOvWords, word = threadIdx.x % kOvWords;
        const int tile = slot_tile[slot];
        const unsigned val = slot_sum[slot][word];
        if (tile > 0 && val) atomicAdd(&J.acc[(size_t)(tile - 1) * kOvWords + word], val);
    }
}

__global__ __launch_bounds__(256) void k_ov_straddle(Arena A, ObjVisJob J, int n_scans) {
    const int M = (int)J.tab_stats[2];
    const long long t0l = (long long)blockIdx.x * kOvTile;
    if (t0l >= (long long)M) return;
    const int t0 = (int)t0l;
    const long long t1 = t0l + kOvTile;
    const int last = (int)min(t1, (long long)M) - 1;
    const int o_first = (int)(J.key_out[t0] >> 32), o_last = (int)(J.key_out[last] >> 32);
    OvStats st;
    for (int k = 0; k < 2; ++k) {
        if (k == 1 && o_last == o_first) break;
        const int o = k ? o_last : o_first;
        const int b = J.begin[o], e = J.begin[o + 1];
        if (b >= t0 && (long long)e <= t1) continue;  // inside the tile: k_ov_tiles finished it
        const unsigned* a = J.acc + (size_t)(b / kOvTile) * kOvWords;
        OvSum s;
#pragma unroll
        for (int j = 0; j < 6; ++j) s.w[j] = a[j];
        int verdict, how;
        ov_decide(J, o, e - b, s, verdict, how);
        if (b >= t0 && threadIdx.x == 0) ov_publish(J, o, e - b, s, verdict, how, st);
        if (how == 0 || !J.out) continue;
        const int lo = max(b, t0), hi = (int)min((long long)e, t1);
        const int sc = ov_scan_of(A, n_scans, (int)(uint32_t)J.key_out[lo], (int)(threadIdx.x & 63));  // (an object lives inside one scan)
        const int base = A.scan_off[sc];
        const int scan_n = A.scan_off[sc + 1] - base;
        for (int p0 = lo; p0 < hi; p0 += 4 * 256) {
            int src[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = p0 + u * 256 + (int)threadIdx.x;
                src[u] = p < hi ? A.apri_src[(uint32_t)J.key_out[p]] : -1;
            }
            // (a byte is written only where it changes, as k_mf_vote does: most members of an object already carry its verdict, and a
            // gathered read costs less than a scattered write.  In place the byte is read before this thread alone may write it)
            uint8_t cur[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) cur[u] = (unsigned)src[u] < (unsigned)scan_n ? J.verdict[(size_t)base + src[u]] : (uint8_t)verdict;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (cur[u] != (uint8_t)verdict) J.out[(size_t)base + src[u]] = (uint8_t)verdict;
        }
    }
    if (threadIdx.x == 0) ov_add_stats(J, st);
}

}  // namespace

long long objvis_tiles(long long total_pts) { return total_pts > 0 ? (total_pts + kOvTile - 1) / kOvTile : 1; }

size_t objvis_work_bytes(long long total_pts) { return sizeof(unsigned) * kOvWords * (size_t)objvis_tiles(total_pts); }

void launch_object_visibility(const Arena& A, ObjVisJob J, void* work, hipStream_t st) {
    const long long tiles = objvis_tiles(A.total_pts);  // (an object has at least one of the batch's points: members <= points)
    J.acc = (unsigned*)work;
    hipMemsetAsync(J.counters, 0, sizeof(unsigned long long) * 8, st);
    hipMemsetAsync(J.acc, 0, objvis_work_bytes(A.total_pts), st);
    if (J.out && J.out != J.verdict && A.total_pts > 0) hipMemcpyAsync(J.out, J.verdict, (size_t)A.total_pts, hipMemcpyDeviceToDevice, st);
    hipLaunchKernelGGL(k_ov_tiles, dim3((unsigned)tiles), dim3(256), 0, st, A, J, A.n_scans);
    hipLaunchKernelGGL(k_ov_straddle, dim3((unsigned)tiles), dim3(256), 0, st, A, J, A.n_scans);
}

}  // namespace scvod
