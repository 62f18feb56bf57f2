// scvod_mapfilter.hip -- cleaning scans against a prior static map (gfx950): scvod_map_filter / scvod_batch_map_filter.
//
// Reference analogue: none.  The reference keeps its map as a PCL cloud and has no program that splits a new scan against it; the
// sides and the vote rule are this project's convention.
//     k_mf_probe    k_mq_query's own-cell pass and, with a radius, its per-wave LDS queue for the points without an own cell
//                   (scvod_mapprobe.h: the same chain walk, select test, run heads and 27 cells, so the result byte IS the query's).
//                   Writes the result byte and the point's own side; counts the own sides (ballot + popcount per wave, LDS per
//                   block, one 64-bit atomic per counter and block)
//     k_mf_vote     k_ot_objects' walk: one wave per object of the table, 64 members per round, the next round's gathers
//                   (key -> apri_src -> result byte) in flight; the four results are counted by ballot + popcount.  The SAME wave then
//                   takes the verdict from its registers and walks the run again to rewrite the sides that differ, so the counts never
//                   leave the wave, no workgroup waits for another, and the caller's d_votes is written but never read.  The chunked
//                   form (integer atomics into per-object words, verdict in a later launch) was not built: see README, "Cleaning scans
//                   against a prior map"
//     k_mf_count    per tile of kMfTile consecutive points of one scan: its KNOWN and NOVEL points
//     k_mf_scan     one workgroup per scan: exclusive prefix of both counts over the scan's tiles, the scan's totals, d_bounds
//     k_mf_write    per tile: in-wave ranks by ballot, the (round, wave) prefix in LDS, the tile's prefix, the segment's start;
//                   16-byte non-temporal record moves
// A partition never crosses a scan, so there is no scan over the scans.  All numbers are integer counts: the same bytes on every run.
#include "scvod_mapprobe.h"

using namespace scvod;

namespace scvod {
namespace {

constexpr int kMfTile = SCVOD_MAP_FILTER_TILE;
static_assert(kMfTile == 8 * 256, "a tile is eight rounds of one workgroup");
constexpr int kMaxGridY = 65535;
// the counter words at the head of the scratch
enum { kMfOwnKnown = 0, kMfOwnNovel, kMfOwnOut, kMfMovedNK, kMfMovedKN, kMfVoted, kMfVotedKnown, kMfOverflow, kMfWords };
constexpr size_t kMfHead = 256;

__device__ __forceinline__ uint8_t mf_side_of(uint8_t result) {
    return result == SCVOD_MAPQ_OUT ? SCVOD_MAPF_OUT : (result == SCVOD_MAPQ_MISS ? SCVOD_MAPF_NOVEL : SCVOD_MAPF_KNOWN);
}

// MODE 0: radius == 0, the own cell only.  MODE 1: a radius: a point whose own cell is occupied is finished after the own-cell pass,
// the others wait in the wave's LDS queue and look at their neighbours 64 at a time (k_mq_query<1>, which see).
template <int MODE>
__global__ __launch_bounds__(256) void k_mf_probe(int s_first, const float4* __restrict__ pts, const int32_t* __restrict__ scan_off,
                                                  const float* __restrict__ pose, const MapRec* __restrict__ table, unsigned long long mask, float inv_leaf,
                                                  float leaf, float radius, int sel, unsigned long long k0, unsigned long long k1, unsigned long long k2,
                                                  unsigned long long k3, uint8_t* __restrict__ out_result, uint8_t* __restrict__ out_side,
                                                  unsigned long long* counters) {
    __shared__ unsigned int blk[3];
    __shared__ float4 q_pt[MODE == 1 ? 4 : 1][MODE == 1 ? kMqQueue : 1];  // x, y, z, the point's index in its scan
    __shared__ unsigned long long q_key[MODE == 1 ? 4 : 1][MODE == 1 ? kMqQueue : 1];
    const int s = s_first + blockIdx.y;
    const int base = scan_off[s];
    const int n = scan_off[s + 1] - base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 3) blk[threadIdx.x] = 0;
    __syncthreads();
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = pose[12 * s + i];
    const float r2 = radius * radius;
    unsigned int n_known = 0, n_novel = 0, n_out = 0;  // per wave (the same in every lane)
    int q_n = 0;                                       // MODE 1: entries waiting in the wave's queue (the same in every lane)
    auto drain = [&](int first, int count) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const bool look = lane < count;
        const float4 e = q_pt[MODE == 1 ? wave : 0][MODE == 1 ? first + (look ? lane : 0) : 0];
        const unsigned long long key = look ? q_key[MODE == 1 ? wave : 0][MODE == 1 ? first + lane : 0] : kEmpty;
        unsigned long long best_key = kEmpty;
        float best_d = __builtin_inff();
        mq_neighbours(table, mask, leaf, radius, r2, sel, k0, k1, k2, k3, look, e.x, e.y, e.z, key, map_home(key, mask), false, kEmpty, best_key, best_d);
        const bool near = look && best_key != kEmpty;
        if (look) {
            const size_t o = (size_t)base + (size_t)__float_as_int(e.w);
            if (out_result) __builtin_nontemporal_store((uint8_t)(near ? SCVOD_MAPQ_NEAR : SCVOD_MAPQ_MISS), &out_result[o]);
            __builtin_nontemporal_store((uint8_t)(near ? SCVOD_MAPF_KNOWN : SCVOD_MAPF_NOVEL), &out_side[o]);
        }
        n_known += (unsigned int)__popcll(__ballot(near));
        n_novel += (unsigned int)__popcll(__ballot(look && !near));
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
        unsigned long long h0, val;
        const bool found = mq_own_cell(table, mask, sel, k0, k1, k2, k3, lane, key, h0, val);
        const bool has_cell = key != kEmpty;
        bool queued = false;
        if (MODE == 1) {
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
        if (live && !queued) {
            const size_t o = (size_t)base + (size_t)i;
            const uint8_t r = (uint8_t)(!has_cell ? SCVOD_MAPQ_OUT : (found ? SCVOD_MAPQ_CELL : SCVOD_MAPQ_MISS));
            if (out_result) __builtin_nontemporal_store(r, &out_result[o]);
            __builtin_nontemporal_store(mf_side_of(r), &out_side[o]);
        }
        n_known += (unsigned int)__popcll(__ballot(live && found));
        n_novel += (unsigned int)__popcll(__ballot(live && has_cell && !found && !queued));
        n_out += (unsigned int)__popcll(__ballot(live && !has_cell));
    }
    if (MODE == 1 && q_n > 0) drain(0, q_n);
    if (lane == 0) {
        if (n_known) atomicAdd(&blk[0], n_known);
        if (n_novel) atomicAdd(&blk[1], n_novel);
        if (n_out) atomicAdd(&blk[2], n_out);
    }
    __syncthreads();
    if (threadIdx.x < 3 && blk[threadIdx.x]) atomicAdd(&counters[kMfOwnKnown + threadIdx.x], (unsigned long long)blk[threadIdx.x]);
}

struct MfVote {
    const uint64_t* key_out;     // the table's sorted member list
    const int32_t* begin;        // the table's run starts
    const long long* tab_stats;  // the table's stats ([1]: its objects)
    const uint8_t* result;       // [points] what k_mf_probe wrote
    uint8_t* side;               // [points] own sides in, final sides out
    scvod_map_filter_object* out;  // [cap] caller's, or nullptr
    long long cap;
    int32_t vote_num, vote_den, min_points;
    unsigned long long* counters;
};

// the scan that holds batch slot g0: the last s with scan_off[s] <= g0
__device__ __forceinline__ int mf_scan_of(const Arena& A, int n_scans, int g0) {
    int lo = 0, hi = n_scans;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.scan_off[mid] <= g0) lo = mid; else hi = mid;
    }
    return lo;
}

// the input index (inside its scan) of slot p of the sorted member list, -1 behind the run's end or for an index outside the scan
__device__ __forceinline__ int mf_member(const Arena& A, const uint64_t* __restrict__ key_out, int p, int e, int scan_n) {
    if (p >= e) return -1;
    const int src = A.apri_src[(uint32_t)key_out[p]];
    return (unsigned)src < (unsigned)scan_n ? src : -1;
}

__global__ __launch_bounds__(256) void k_mf_vote(Arena A, MfVote J, int n_scans) {
    const int lane = threadIdx.x & 63;
    const long long n_all = J.tab_stats[1];
    if (blockIdx.x == 0 && threadIdx.x == 0 && J.out && n_all > J.cap) J.counters[kMfOverflow] = 1ull;
    unsigned long long moved_nk = 0, moved_kn = 0, voted = 0, voted_known = 0;  // per wave (the same in every lane)
    for (long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); o < n_all; o += (long long)gridDim.x * 4) {
        const int b = J.begin[o], e = J.begin[o + 1];
        const int s = mf_scan_of(A, n_scans, (int)(uint32_t)J.key_out[b]);
        const int base = A.scan_off[s];
        const int scan_n = A.scan_off[s + 1] - base;
        int n_cell = 0, n_near = 0, n_miss = 0, n_out = 0;  // (wave-uniform)
        int src = mf_member(A, J.key_out, b + lane, e, scan_n);
        uint8_t cur = src >= 0 ? J.result[(size_t)base + src] : (uint8_t)0xFF;
        for (int j = b; j < e; j += 64) {
            const int nsrc = mf_member(A, J.key_out, j + 64 + lane, e, scan_n);
            const uint8_t nxt = nsrc >= 0 ? J.result[(size_t)base + nsrc] : (uint8_t)0xFF;
            n_cell += __popcll(__ballot(cur == SCVOD_MAPQ_CELL));
            n_near += __popcll(__ballot(cur == SCVOD_MAPQ_NEAR));
            n_miss += __popcll(__ballot(cur == SCVOD_MAPQ_MISS));
            n_out += __popcll(__ballot(cur == SCVOD_MAPQ_OUT));
            cur = nxt;
        }
        const int n_points = e - b;
        const bool votes = n_points >= J.min_points;
        const bool known = (long long)(n_cell + n_near) * J.vote_den >= (long long)J.vote_num * n_points;
        if (votes) {
            // the members whose side differs from the verdict: MISS under KNOWN, CELL / NEAR under NOVEL; OUT stays
            const uint8_t verdict = known ? SCVOD_MAPF_KNOWN : SCVOD_MAPF_NOVEL;
            if (known ? n_miss > 0 : n_cell + n_near > 0) {
                for (int j = b; j < e; j += 64) {
                    const int m = mf_member(A, J.key_out, j + lane, e, scan_n);
                    if (m < 0) continue;
                    const uint8_t r = J.result[(size_t)base + m];
                    if (known ? r == SCVOD_MAPQ_MISS : (r == SCVOD_MAPQ_CELL || r == SCVOD_MAPQ_NEAR)) J.side[(size_t)base + m] = verdict;
                }
            }
            ++voted;
            if (known) {
                ++voted_known;
                moved_nk += (unsigned long long)n_miss;
            } else {
                moved_kn += (unsigned long long)(n_cell + n_near);
            }
        }
        if (lane == 0 && J.out && o < J.cap) {
            scvod_map_filter_object r;
            r.n_cell = n_cell;
            r.n_near = n_near;
            r.n_miss = n_miss;
            r.n_out = n_out;
            r.n_points = n_points;
            r.verdict = votes ? (known ? SCVOD_MAPF_KNOWN : SCVOD_MAPF_NOVEL) : -1;
            r.reserved[0] = r.reserved[1] = 0;
            J.out[o] = r;
        }
    }
    if (lane == 0) {
        if (moved_nk) atomicAdd(&J.counters[kMfMovedNK], moved_nk);
        if (moved_kn) atomicAdd(&J.counters[kMfMovedKN], moved_kn);
        if (voted) atomicAdd(&J.counters[kMfVoted], voted);
        if (voted_known) atomicAdd(&J.counters[kMfVotedKnown], voted_known);
    }
}

// the partition's view of a call: tile (s, t) owns tile_cnt[2 * (s * tps + t)] (KNOWN) and the word behind it (NOVEL)
struct MfPart {
    const int32_t* scan_off;
    const uint8_t* side;
    int32_t* tile_cnt;   // [n_scans][tps][2] counts, then exclusive prefixes inside the scan
    int32_t* scan_tot;   // [n_scans][2] KNOWN, NOVEL of the scan
    int tps;             // tiles of the longest scan
    int32_t* order;      // caller's, each nullptr when not asked for
    int32_t* bounds;
    float4* xyzi_out;
    const uint32_t* payload_in;
    uint32_t* payload_out;
};

// KNOWN and NOVEL points of tile blockIdx.x of scan s_first + blockIdx.y
__global__ __launch_bounds__(256) void k_mf_count(int s_first, MfPart J) {
    __shared__ int wcnt[2][4];
    const int s = s_first + blockIdx.y;
    const int base = J.scan_off[s];
    const int n = J.scan_off[s + 1] - base;
    const int i0 = blockIdx.x * kMfTile;
    if (i0 >= n) return;  // (k_mf_scan reads the tiles a scan has, no others)
    uint8_t c[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) c[u] = J.side[(size_t)base + min(i0 + u * 256 + (int)threadIdx.x, n - 1)];
    int ck = 0, cn = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const bool live = i0 + u * 256 + (int)threadIdx.x < n;
        ck += __popcll(__ballot(live && c[u] == SCVOD_MAPF_KNOWN));
        cn += __popcll(__ballot(live && c[u] == SCVOD_MAPF_NOVEL));
    }
    if ((threadIdx.x & 63) == 0) wcnt[0][threadIdx.x >> 6] = ck, wcnt[1][threadIdx.x >> 6] = cn;
    __syncthreads();
    if (threadIdx.x < 2)
        J.tile_cnt[2 * ((size_t)s * J.tps + blockIdx.x) + threadIdx.x] =
            wcnt[threadIdx.x][0] + wcnt[threadIdx.x][1] + wcnt[threadIdx.x][2] + wcnt[threadIdx.x][3];
}

// scan blockIdx.x: its tiles' counts -> exclusive prefixes inside the scan (256 tiles per round), its totals and its bounds
__global__ __launch_bounds__(256) void k_mf_scan(MfPart J) {
    __shared__ int wsum[5];
    const int s = blockIdx.x;
    const int n = J.scan_off[s + 1] - J.scan_off[s];
    const int tiles = (n + kMfTile - 1) / kMfTile;
    int32_t* cnt = J.tile_cnt + 2 * (size_t)s * J.tps;
    int carry_k = 0, carry_n = 0;
    for (int t0 = 0; t0 < tiles; t0 += 256) {
        const int t = t0 + (int)threadIdx.x;
        const int vk = t < tiles ? cnt[2 * t] : 0, vn = t < tiles ? cnt[2 * t + 1] : 0;
        int tot_k, tot_n;
        const int ek = block_excl_scan<256>(vk, tot_k, wsum);
        const int en = block_excl_scan<256>(vn, tot_n, wsum);
        if (t < tiles) {
            cnt[2 * t] = carry_k + ek;
            cnt[2 * t + 1] = carry_n + en;
        }
        carry_k += tot_k;
        carry_n += tot_n;
    }
    if (threadIdx.x == 0) {
        J.scan_tot[2 * (size_t)s] = carry_k;
        J.scan_tot[2 * (size_t)s + 1] = carry_n;
        if (J.bounds) {
            J.bounds[2 * (size_t)s] = carry_k;
            J.bounds[2 * (size_t)s + 1] = carry_k + carry_n;
        }
    }
}

// the points of tile blockIdx.x of scan s_first + blockIdx.y into their slots of the scan's three segments.  (The second launch bound
// keeps the eight records of a thread in flight in 64 VGPRs; without it the compiler spends 196 and two waves fit a SIMD.)
__global__ __launch_bounds__(256, 4) void k_mf_write(int s_first, const float4* __restrict__ pts, MfPart J) {
    __shared__ int wcnt[2][32];  // [side][round][wave] points, then their exclusive prefix in (round, wave) order
    const int s = s_first + blockIdx.y;
    const int base = J.scan_off[s];
    const int n = J.scan_off[s + 1] - base;
    const int i0 = blockIdx.x * kMfTile;
    if (i0 >= n) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint8_t c[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) c[u] = __builtin_nontemporal_load(&J.side[(size_t)base + min(i0 + u * 256 + (int)threadIdx.x, n - 1)]);
    int rank[8];  // among the points of its side in its wave and round
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const bool live = i0 + u * 256 + (int)threadIdx.x < n;
        const unsigned long long bk = __ballot(live && c[u] == SCVOD_MAPF_KNOWN), bn = __ballot(live && c[u] == SCVOD_MAPF_NOVEL);
        const unsigned long long below = (1ull << lane) - 1ull;
        const int pk = __popcll(bk & below), pn = __popcll(bn & below);
        rank[u] = c[u] == SCVOD_MAPF_KNOWN ? pk : (c[u] == SCVOD_MAPF_NOVEL ? pn : lane - pk - pn);  // (the live lanes are a prefix)
        if (lane == 0) wcnt[0][u * 4 + w] = __popcll(bk), wcnt[1][u * 4 + w] = __popcll(bn);
    }
    __syncthreads();
    if (w < 2) {
        const int v = lane < 32 ? wcnt[w][lane] : 0;
        const int inc = wave_incl_scan(v);
        if (lane < 32) wcnt[w][lane] = inc - v;
    }
    __syncthreads();
    const size_t tile = 2 * ((size_t)s * J.tps + blockIdx.x);
    const int tile_k = J.tile_cnt[tile], tile_n = J.tile_cnt[tile + 1];
    const int tot_k = J.scan_tot[2 * (size_t)s], tot_n = J.scan_tot[2 * (size_t)s + 1];
    typedef float f4v __attribute__((ext_vector_type(4)));
    const bool records = J.xyzi_out != nullptr, payload = J.payload_out != nullptr;
    f4v q[8];
    uint32_t pay[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * 256 + (int)threadIdx.x;
        q[u] = f4v{0.f, 0.f, 0.f, 0.f};
        pay[u] = 0u;
        if (i < n) {
            if (records) q[u] = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(&pts[(size_t)base + i]));
            if (payload) pay[u] = __builtin_nontemporal_load(&J.payload_in[(size_t)base + i]);
        }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * 256 + (int)threadIdx.x;
        if (i >= n) continue;
        const int before_k = tile_k + wcnt[0][u * 4 + w], before_n = tile_n + wcnt[1][u * 4 + w];
        int j;  // the point's slot in its scan
        if (c[u] == SCVOD_MAPF_KNOWN)
            j = before_k + rank[u];
        else if (c[u] == SCVOD_MAPF_NOVEL)
            j = tot_k + before_n + rank[u];
        else
            j = tot_k + tot_n + (i0 + u * 256 + w * 64 - before_k - before_n) + rank[u];
        const size_t o = (size_t)base + (size_t)j;
        if (J.order) __builtin_nontemporal_store(i, &J.order[o]);
        if (records) __builtin_nontemporal_store(q[u], reinterpret_cast<f4v*>(&J.xyzi_out[o]));
        if (payload) __builtin_nontemporal_store(pay[u], &J.payload_out[o]);
    }
}

struct MfArgs {
    scvod_map_filter_params p;
    const uint8_t* h_select256;
    uint8_t* d_result;
    uint8_t* d_side;
    int32_t* d_order;
    int32_t* d_bounds;
    void* d_xyzi_out;
    const uint32_t* d_payload_in;
    uint32_t* d_payload_out;
    void* d_votes;
    int64_t cap_votes;
};

// what both forms refuse before a device is touched; batch: the form that knows objects
int mf_check(scvod_map* m, const scvod_map_filter_params* params, MfArgs& a, bool batch) {
    if (params)
        a.p = *params;
    else
        scvod_map_filter_params_default(&a.p);
    const scvod_map_filter_params& p = a.p;
    if (!(p.radius >= 0.f) || p.radius > 0.99f * m->leaf)
        return mfail(m, SCVOD_ERR_INVALID, "radius %g outside [0, 0.99 * leaf = %g]", (double)p.radius, (double)(0.99f * m->leaf));
    if (a.h_select256 && m->kind != SCVOD_MAP_KIND_LABELLED) return mfail(m, SCVOD_ERR_INVALID, "a select table needs a map of kind SCVOD_MAP_KIND_LABELLED");
    if (p.reserved != 0) return mfail(m, SCVOD_ERR_INVALID, "scvod_map_filter_params::reserved must be 0");
    if (p.flags & ~SCVOD_MAPF_OBJECT_VOTE) return mfail(m, SCVOD_ERR_INVALID, "unknown flag bit (flags %d)", p.flags);
    if (p.vote_den < 1 || p.vote_den > (1 << 20) || p.vote_num < 0 || p.vote_num > p.vote_den)
        return mfail(m, SCVOD_ERR_INVALID, "vote %d / %d: 0 <= vote_num <= vote_den, 1 <= vote_den <= 2^20", p.vote_num, p.vote_den);
    if (p.min_points < 1) return mfail(m, SCVOD_ERR_INVALID, "min_points %d below 1", p.min_points);
    const bool vote = (p.flags & SCVOD_MAPF_OBJECT_VOTE) != 0;
    if (vote && !batch) return mfail(m, SCVOD_ERR_INVALID, "SCVOD_MAPF_OBJECT_VOTE needs the batch form: scvod_map_filter knows no objects");
    if (a.d_votes && !vote) return mfail(m, SCVOD_ERR_INVALID, "d_votes without SCVOD_MAPF_OBJECT_VOTE");
    if (a.cap_votes < 0) return mfail(m, SCVOD_ERR_INVALID, "cap_votes below 0");
    if (a.d_payload_out && !a.d_payload_in) return mfail(m, SCVOD_ERR_INVALID, "d_payload_out without d_payload_in");
    if ((uintptr_t)a.d_xyzi_out & 15u) return mfail(m, SCVOD_ERR_INVALID, "d_xyzi_out is not 16-byte aligned");
    if (((uintptr_t)a.d_order & 3u) || ((uintptr_t)a.d_bounds & 3u) || ((uintptr_t)a.d_payload_in & 3u) || ((uintptr_t)a.d_payload_out & 3u) ||
        ((uintptr_t)a.d_votes & 3u))
        return mfail(m, SCVOD_ERR_INVALID, "d_order, d_bounds, the payloads and d_votes must be 4-byte aligned");
    return SCVOD_OK;
}

// does any output touch the input records [first, end) of d_xyzi?
int mf_check_overlap(scvod_map* m, const MfArgs& a, const void* d_xyzi, long long first, long long end, int n_scans) {
    if (end <= first) return SCVOD_OK;
    const uintptr_t in0 = (uintptr_t)d_xyzi + 16u * (uintptr_t)first, in1 = (uintptr_t)d_xyzi + 16u * (uintptr_t)end;
    auto hits = [&](const void* p, size_t elem, long long lo, long long hi) {
        if (!p || hi <= lo) return false;
        const uintptr_t o0 = (uintptr_t)p + elem * (uintptr_t)lo, o1 = (uintptr_t)p + elem * (uintptr_t)hi;
        return o0 < in1 && in0 < o1;
    };
    if (hits(a.d_result, 1, first, end) || hits(a.d_side, 1, first, end) || hits(a.d_order, 4, first, end) || hits(a.d_bounds, 8, 0, n_scans) ||
        hits(a.d_xyzi_out, 16, first, end) || hits(a.d_payload_out, 4, first, end) ||
        hits(a.d_votes, sizeof(scvod_map_filter_object), 0, a.cap_votes))
        return mfail(m, SCVOD_ERR_INVALID, "an output overlaps the input cloud");
    return SCVOD_OK;
}

size_t mf_align(size_t v) { return (v + 255) & ~(size_t)255; }

// Scans [0, n_scans) of a cloud whose offsets and poses are on the device already.  span: the index behind the cloud's last point (what
// the per-point arrays are indexed up to); points: the cloud's size; V: nullptr, or the vote's view of the object table
int mf_launch(scvod_map* m, const void* d_xyzi, const int32_t* d_offs, int n_scans, int max_pts, long long span, long long points, const MfArgs& a,
              const Arena* A, MfVote* V, hipStream_t st) {
    const bool part = a.d_order || a.d_bounds || a.d_xyzi_out || a.d_payload_out;
    const int tps = (max_pts + kMfTile - 1) / kMfTile;
    // the scratch: counters | side bytes (unless the caller's) | result bytes (a vote without the caller's) | tile counts | scan totals
    const size_t per_point = mf_align((size_t)(span > 0 ? span : 0));
    const size_t off_side = kMfHead, off_result = off_side + (a.d_side ? 0 : per_point);
    const size_t off_tiles = off_result + ((V && !a.d_result) ? per_point : 0);
    const size_t off_tot = off_tiles + (part ? mf_align(sizeof(int32_t) * 2 * (size_t)n_scans * (size_t)tps) : 0);
    const size_t need = off_tot + (part ? mf_align(sizeof(int32_t) * 2 * (size_t)n_scans) : 0);
    if (m->f_cap < need) {  // grow-only; the old block may still be read by work on `st`
        MHIP(m, hipStreamSynchronize(st));
        if (m->f_ran && m->f_stream != st) MHIP(m, hipStreamSynchronize(m->f_stream));
        if (m->f_buf) hipFree(m->f_buf);
        m->f_buf = nullptr;
        m->f_cap = 0;
        m->f_ran = false;
        MHIP(m, hipMalloc(&m->f_buf, need));
        m->f_cap = need;
    }
    unsigned long long* counters = (unsigned long long*)m->f_buf;
    MHIP(m, hipMemsetAsync(counters, 0, sizeof(unsigned long long) * kMfWords, st));
    m->f_points = points;
    m->f_stream = st;
    m->f_ran = true;
    uint8_t* side = a.d_side ? a.d_side : m->f_buf + off_side;
    uint8_t* result = a.d_result ? a.d_result : (V ? m->f_buf + off_result : nullptr);
    if (max_pts <= 0) {  // no point anywhere: the bounds are all there is to write
        if (a.d_bounds && n_scans > 0) MHIP(m, hipMemsetAsync(a.d_bounds, 0, sizeof(int32_t) * 2 * (size_t)n_scans, st));
        if (V && V->out) {  // (a batch without points has no objects; the table's count still decides the latch)
            V->result = result, V->side = side, V->counters = counters;
            hipLaunchKernelGGL(k_mf_vote, dim3(1), dim3(256), 0, st, *A, *V, A->n_scans);
            MHIP(m, hipGetLastError());
        }
        return SCVOD_OK;
    }
    unsigned long long k[4];
    map_table256(a.h_select256, k);
    const int sel = a.h_select256 ? 1 : 0;
    for (int s0 = 0; s0 < n_scans; s0 += kMaxGridY) {
        const int ny = n_scans - s0 < kMaxGridY ? n_scans - s0 : kMaxGridY;
        const dim3 grid((max_pts + kMapPts - 1) / kMapPts, ny), block(256);
#define MF_LAUNCH(MODE)                                                                                                                       \
    hipLaunchKernelGGL(k_mf_probe<MODE>, grid, block, 0, st, s0, (const float4*)d_xyzi, d_offs, m->d_pose, m->table,                          \
                       (unsigned long long)(m->capacity - 1), 1.0f / m->leaf, m->leaf, a.p.radius, sel, k[0], k[1], k[2], k[3], result, side, \
                       counters)
        if (a.p.radius == 0.f)
            MF_LAUNCH(0);
        else
            MF_LAUNCH(1);
#undef MF_LAUNCH
        MHIP(m, hipGetLastError());
    }
    if (V) {
        V->result = result, V->side = side, V->counters = counters;
        long long waves = A->total_pts > 0 ? A->total_pts : 1;  // (an object has at least one of the batch's points)
        const long long grid = (waves + 3) / 4;
        hipLaunchKernelGGL(k_mf_vote, dim3((unsigned)(grid < 2048 ? grid : 2048)), dim3(256), 0, st, *A, *V, A->n_scans);
        MHIP(m, hipGetLastError());
    }
    if (!part) return SCVOD_OK;
    MfPart J;
    J.scan_off = d_offs;
    J.side = side;
    J.tile_cnt = (int32_t*)(m->f_buf + off_tiles);
    J.scan_tot = (int32_t*)(m->f_buf + off_tot);
    J.tps = tps;
    J.order = a.d_order;
    J.bounds = a.d_bounds;
    J.xyzi_out = (float4*)a.d_xyzi_out;
    J.payload_in = a.d_payload_in;
    J.payload_out = a.d_payload_out;
    for (int s0 = 0; s0 < n_scans; s0 += kMaxGridY) {
        const int ny = n_scans - s0 < kMaxGridY ? n_scans - s0 : kMaxGridY;
        hipLaunchKernelGGL(k_mf_count, dim3(tps, ny), dim3(256), 0, st, s0, J);
    }
    hipLaunchKernelGGL(k_mf_scan, dim3(n_scans), dim3(256), 0, st, J);
    if (a.d_order || a.d_xyzi_out || a.d_payload_out)
        for (int s0 = 0; s0 < n_scans; s0 += kMaxGridY) {
            const int ny = n_scans - s0 < kMaxGridY ? n_scans - s0 : kMaxGridY;
            hipLaunchKernelGGL(k_mf_write, dim3(tps, ny), dim3(256), 0, st, s0, (const float4*)d_xyzi, J);
        }
    MHIP(m, hipGetLastError());
    return SCVOD_OK;
}

}  // namespace
}  // namespace scvod

extern "C" {

void scvod_map_filter_params_default(scvod_map_filter_params* p) {
    if (!p) return;
    p->radius = 0.f;
    p->flags = 0;
    p->vote_num = 1;
    p->vote_den = 2;
    p->min_points = 1;
    p->reserved = 0;
}

int scvod_map_filter(scvod_map* m, const void* d_xyzi, const int32_t* h_scan_offsets, int32_t n_scans, const float* h_poses,
                     const scvod_map_filter_params* params, const uint8_t* h_select256, uint8_t* d_result, uint8_t* d_side, int32_t* d_order,
                     int32_t* d_bounds, void* d_xyzi_out, const uint32_t* d_payload_in, uint32_t* d_payload_out, void* stream) {
    if (!m || n_scans < 0 || (n_scans > 0 && !h_scan_offsets)) return mfail(m, SCVOD_ERR_INVALID, "bad arguments");
    MfArgs a = {{}, h_select256, d_result, d_side, d_order, d_bounds, d_xyzi_out, d_payload_in, d_payload_out, nullptr, 0};
    if (int rc = mf_check(m, params, a, false)) return rc;
    int max_pts = 0;
    if (n_scans > 0)
        if (int rc = map_check_offsets(m, h_scan_offsets, n_scans, &max_pts)) return rc;
    if (max_pts > 0 && !d_xyzi) return mfail(m, SCVOD_ERR_INVALID, "NULL points of a cloud that is not empty");
    if ((uintptr_t)d_xyzi & 15u) return mfail(m, SCVOD_ERR_INVALID, "d_xyzi is not 16-byte aligned");
    const long long first = n_scans > 0 ? h_scan_offsets[0] : 0, span = n_scans > 0 ? h_scan_offsets[n_scans] : 0;
    if (int rc = mf_check_overlap(m, a, d_xyzi, first, span, n_scans)) return rc;
    MHIP(m, hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)stream;
    if (max_pts > 0) {
        if (int rc = map_stage_poses(m, h_poses, n_scans, st)) return rc;
        if (int rc = map_stage_offsets(m, h_scan_offsets, n_scans, st)) return rc;
    }
    return mf_launch(m, d_xyzi, m->d_offs, n_scans, max_pts, span, span - first, a, nullptr, nullptr, st);
}

int scvod_batch_map_filter(scvod_ctx* ctx, scvod_map* m, const float* h_poses, const scvod_map_filter_params* params, const uint8_t* h_select256,
                           uint8_t* d_result, uint8_t* d_side, int32_t* d_order, int32_t* d_bounds, void* d_xyzi_out, const uint32_t* d_payload_in,
                           uint32_t* d_payload_out, void* d_votes, int64_t cap_votes, void* stream) {
    if (!ctx || !m || !h_poses) return mfail(m, SCVOD_ERR_INVALID, "bad arguments");
    MfArgs a = {{}, h_select256, d_result, d_side, d_order, d_bounds, d_xyzi_out, d_payload_in, d_payload_out, d_votes, cap_votes};
    if (int rc = mf_check(m, params, a, true)) return rc;
    Arena A;
    int device = 0, track_valid = 0, batch_valid = 0, n_scans = 0, max_pts = 0, mode = 0, min_pts = 0;
    scvod__ctx_view(ctx, &A, &device, &track_valid, &batch_valid, &n_scans, &max_pts, &mode, &min_pts);
    if (!batch_valid || !A.pts) return mfail(m, SCVOD_ERR_STATE, "scvod_batch_map_filter needs a processed batch of input clouds");
    if (device != m->device) return mfail(m, SCVOD_ERR_INVALID, "map and ctx live on different devices");
    MfVote V{};
    const bool vote = (a.p.flags & SCVOD_MAPF_OBJECT_VOTE) != 0;
    if (vote) {
        const char* why = "";
        if (int rc = scvod__ctx_object_lists(ctx, "scvod_batch_map_filter", &V.tab_stats, &V.key_out, &V.begin, &why)) return mfail(m, rc, "%s", why);
        V.out = (scvod_map_filter_object*)d_votes;
        V.cap = (long long)cap_votes;
        V.vote_num = a.p.vote_num;
        V.vote_den = a.p.vote_den;
        V.min_points = a.p.min_points;
    }
    if (int rc = mf_check_overlap(m, a, A.pts, 0, (long long)A.total_pts, n_scans)) return rc;
    MHIP(m, hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)scvod__ctx_stream(ctx, stream);
    if (int rc = map_stage_poses(m, h_poses, n_scans, st)) return rc;
    return mf_launch(m, A.pts, A.scan_off, n_scans, max_pts, (long long)A.total_pts, (long long)A.total_pts, a, &A, vote ? &V : nullptr, st);
}

int scvod_map_filter_stats(scvod_map* m, int64_t* h_out8) {
    if (!m || !h_out8) return mfail(m, SCVOD_ERR_INVALID, "bad arguments");
    if (!m->f_ran) return mfail(m, SCVOD_ERR_STATE, "scvod_map_filter_stats before the first filter");
    MHIP(m, hipSetDevice(m->device));
    MHIP(m, hipStreamSynchronize(m->f_stream));
    unsigned long long h[kMfWords] = {0};
    MHIP(m, hipMemcpy(h, m->f_buf, sizeof(h), hipMemcpyDeviceToHost));
    h_out8[0] = (int64_t)m->f_points;
    h_out8[1] = (int64_t)(h[kMfOwnKnown] + h[kMfMovedNK] - h[kMfMovedKN]);
    h_out8[2] = (int64_t)(h[kMfOwnNovel] + h[kMfMovedKN] - h[kMfMovedNK]);
    h_out8[3] = (int64_t)h[kMfOwnOut];
    h_out8[4] = (int64_t)h[kMfMovedNK];
    h_out8[5] = (int64_t)h[kMfMovedKN];
    h_out8[6] = (int64_t)h[kMfVoted];
    h_out8[7] = (int64_t)h[kMfVotedKnown];
    if (h[kMfOverflow]) return mfail(m, SCVOD_ERR_CAPACITY, "the object table holds more objects than cap_votes");
    return SCVOD_OK;
}

int64_t scvod_map_filter_scratch_bytes(const scvod_map* m) { return m ? (int64_t)m->f_cap : 0; }

}  // extern "C"
