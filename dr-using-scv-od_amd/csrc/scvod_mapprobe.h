// scvod_mapprobe.h -- how a kernel asks the static map's table about a point: the walk of a probe chain, the select test, the own
// cell of the points of a wave and the 27 cells around a point.  scvod_mapquery.hip (the query) and scvod_mapfilter.hip (the filter)
// include it, so that both give the same answer by construction.  Device code only; nothing here writes the table.
#ifndef SCVOD_MAPPROBE_H_
#define SCVOD_MAPPROBE_H_
#include "scvod_maptable.h"

namespace scvod {
namespace {

// Two development switches, so that the variants profiles/map_query_experiments.md compares build from this file; the shipped library
// is built with neither.  SCVOD_MQ_GROUP: home-slot peeks of neighbour cells issued before the first is looked at.  Measured 1, 3, 9
// and 27: the fewer registers the better -- the kernel lives on waves in flight, not on loads in flight per wave.
// SCVOD_MQ_PRUNE: skip neighbour cells that lie wholly beyond the radius (exact, see mq_prune): 3.6 x at 0.25 * leaf, free at 0.99.
#ifndef SCVOD_MQ_GROUP
#define SCVOD_MQ_GROUP 1
#endif
#ifndef SCVOD_MQ_PRUNE
#define SCVOD_MQ_PRUNE 1
#endif
constexpr int kMqGroup = SCVOD_MQ_GROUP;
static_assert(kMqGroup == 1 || kMqGroup == 3 || kMqGroup == 9 || kMqGroup == 27, "group of neighbour peeks");

// the record of `key`, walking on from the peek `rec` of slot h (the home slot at first): found, or absent behind an empty slot / the bound
__device__ __forceinline__ bool mq_find_from(const MapRec* table, unsigned long long mask, unsigned long long key, unsigned long long h, MapRec rec,
                                             unsigned long long& val) {
    for (int probes = 0; probes < kMapMaxProbes; ++probes) {
        if (rec.key == key) {
            val = rec.val;
            return true;
        }
        if (rec.key == kEmpty) return false;
        h = (h + 1) & mask;
        rec = map_peek(table, h);
    }
    return false;
}

// does the label byte of a labelled map's value pass the select table?  (sel == 0: a plain map, or no table)
__device__ __forceinline__ bool mq_selected(int sel, unsigned long long k0, unsigned long long k1, unsigned long long k2, unsigned long long k3,
                                            unsigned long long val) {
    return !sel || map_bit256(k0, k1, k2, k3, (unsigned int)(val >> 8) & 0xffu);
}

// The own cell of the 64 points of a wave, one key per lane (kEmpty: no cell; every lane of the wave must call).  Runs of consecutive
// lanes with one key are found by ballot, the head of a run probes and the run takes the head's record by __shfl; a point without a
// cell splits a run and probes nothing.  A cell that is not selected counts as empty.  h0: the home slot of the lane's key;
// val: the cell's value, kEmpty when the answer is false.
__device__ __forceinline__ bool mq_own_cell(const MapRec* __restrict__ table, unsigned long long mask, int sel, unsigned long long k0,
                                            unsigned long long k1, unsigned long long k2, unsigned long long k3, int lane, unsigned long long key,
                                            unsigned long long& h0, unsigned long long& val) {
    const unsigned long long prev = __shfl_up(key, 1);
    const bool head = (lane == 0) || (prev != key);
    const unsigned long long heads = __ballot(head);
    const int my_head = 63 - __clzll((long long)(heads & ((2ull << lane) - 1ull)));
    const bool need = head && key != kEmpty;
    h0 = map_home(key, mask);
    val = kEmpty;
    bool found = false;
    if (need) found = mq_find_from(table, mask, key, h0, map_peek(table, h0), val);
    if (found && !mq_selected(sel, k0, k1, k2, k3, val)) found = false;  // a cell that is not selected counts as empty
    if (!found) val = kEmpty;
    const unsigned long long founds = __ballot(found);
    val = __shfl(val, my_head);
    return (founds >> my_head) & 1ull;
}

// May the cells on the far side of the face at cell coordinate `face` be skipped?  A representative of a cell c >= face decodes to
// X = fl(fl(c + t) * leaf) >= fl((float)face * leaf) (rounding is monotone and t > 0), so fl(X - x) >= fl(fl(face * leaf) - x); when
// that is >= radius, dx * dx >= radius * radius after rounding too and d = (dx*dx + dy*dy) + dz*dz >= dx*dx can never be < r2.  The
// mirror image holds for cells c < face.  No margin is involved: the test uses the very roundings the distance uses.
__device__ __forceinline__ bool mq_prune(float x, int face, float leaf, float radius, bool above) {
    const float f = (float)face * leaf;
    return (above ? f - x : x - f) >= radius;
}

// The 27 cells around the own cell of the point (x, y, z) with key `key` (home slot h0): the nearest candidate, equal d to the smaller
// key.  own_found / own_val: the own cell's record, which the caller holds already.  Each of the 26 other cells is hashed on its own;
// their home-slot peeks are issued kMqGroup at a time (a cell that is pruned or outside the +-2^20 range peeks the own cell's home
// slot, a line the wave just read).  Lanes with look == false take part in the loads only.
__device__ __forceinline__ void mq_neighbours(const MapRec* __restrict__ table, unsigned long long mask, float leaf, float radius, float r2, int sel,
                                              unsigned long long k0, unsigned long long k1, unsigned long long k2, unsigned long long k3, bool look,
                                              float x, float y, float z, unsigned long long key, unsigned long long h0, bool own_found,
                                              unsigned long long own_val, unsigned long long& best_key, float& best_d) {
    const int cx = (int)(key >> (2 * kCellBits)) - kCellBias, cy = (int)((key >> kCellBits) & ((1u << kCellBits) - 1u)) - kCellBias,
              cz = (int)(key & ((1u << kCellBits) - 1u)) - kCellBias;
    // per axis: may the cells below (bit 0) / above (bit 2) be left out?  bit 1 (the own column) never
    unsigned int skip_x = 0, skip_y = 0, skip_z = 0;
    if (cx - 1 < -kCellBias || (SCVOD_MQ_PRUNE && mq_prune(x, cx, leaf, radius, false))) skip_x |= 1u;
    if (cx + 1 >= kCellBias || (SCVOD_MQ_PRUNE && mq_prune(x, cx + 1, leaf, radius, true))) skip_x |= 4u;
    if (cy - 1 < -kCellBias || (SCVOD_MQ_PRUNE && mq_prune(y, cy, leaf, radius, false))) skip_y |= 1u;
    if (cy + 1 >= kCellBias || (SCVOD_MQ_PRUNE && mq_prune(y, cy + 1, leaf, radius, true))) skip_y |= 4u;
    if (cz - 1 < -kCellBias || (SCVOD_MQ_PRUNE && mq_prune(z, cz, leaf, radius, false))) skip_z |= 1u;
    if (cz + 1 >= kCellBias || (SCVOD_MQ_PRUNE && mq_prune(z, cz + 1, leaf, radius, true))) skip_z |= 4u;
    auto consider = [&](unsigned long long ckey, int ax, int ay, int az, unsigned long long cval) {
        const float px = map_decode(ax, (float)((cval >> 48) & 0xffffu), leaf), py = map_decode(ay, (float)((cval >> 32) & 0xffffu), leaf),
                    pz = map_decode(az, (float)((cval >> 16) & 0xffffu), leaf);
        const float dx = x - px, dy = y - py, dz = z - pz;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (d < r2 && (d < best_d || (d == best_d && ckey < best_key))) {
            best_d = d;
            best_key = ckey;
        }
    };
    if (look && own_found) consider(key, cx, cy, cz, own_val);
#pragma unroll
    for (int g0 = 0; g0 < 27; g0 += kMqGroup) {
        unsigned long long nkey[kMqGroup], nh[kMqGroup];
        bool on[kMqGroup];
        MapRec first[kMqGroup];
#pragma unroll
        for (int j = 0; j < kMqGroup; ++j) {
            const int c = g0 + j, ox = c / 9, oy = (c / 3) % 3, oz = c % 3;  // offsets + 1
            on[j] = look && c != 13 && !((skip_x >> ox) & 1u) && !((skip_y >> oy) & 1u) && !((skip_z >> oz) & 1u);
            // (an offset that is skipped may leave the key's range: the key is not used then)
            nkey[j] = ((unsigned long long)(unsigned int)(cx + ox - 1 + kCellBias) << (2 * kCellBits)) |
                      ((unsigned long long)(unsigned int)(cy + oy - 1 + kCellBias) << kCellBits) |
                      (unsigned long long)(unsigned int)(cz + oz - 1 + kCellBias);
            nh[j] = on[j] ? map_home(nkey[j], mask) : (h0 & mask);
        }
#pragma unroll
        for (int j = 0; j < kMqGroup; ++j) first[j] = map_peek(table, nh[j]);
#pragma unroll
        for (int j = 0; j < kMqGroup; ++j) {
            const int c = g0 + j, ox = c / 9, oy = (c / 3) % 3, oz = c % 3;
            unsigned long long nval = kEmpty;
            if (on[j] && mq_find_from(table, mask, nkey[j], nh[j], first[j], nval) && mq_selected(sel, k0, k1, k2, k3, nval))
                consider(nkey[j], cx + ox - 1, cy + oy - 1, cz + oz - 1, nval);
        }
    }
}

constexpr int kMqQueue = 128;  // per wave: fewer than 64 waiting entries + at most 64 new ones

}  // namespace
}  // namespace scvod

#endif
