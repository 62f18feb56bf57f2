// scvod_register.hip -- refining scan poses against the static map or a cloud by Gauss-Newton on the device (gfx950).
//
// Not from the reference.  The step is defined once, in scvod_math.h (reg_*): this file finds the correspondence
// of every source point, feeds it to those functions and iterates.  Two targets, one body:
//   the static map   the query's rule through scvod_mapprobe.h (own cell, then the 27 cells: nearest decoded representative, ties to
//                    the smaller key, the select table honoured); the table is only read
//   a cloud          the shared CSR grid of scvod_grid.h, built once per call, grid_probe27, ties to the lowest index
// A call enqueues k_reg_init and max_iterations rounds of {k_reg_accumulate, k_reg_solve}; nothing is read on the host in between.
// k_reg_solve leaves the sums of its scan cleared for the next round, so the "clear" of a round costs no launch of its own.
// The running pose is d_pose_out itself (fp64), the latch is the status word of the scan's record.
#include "scvod_grid.h"
#include "scvod_mapprobe.h"

using namespace scvod;

namespace scvod {
namespace {

constexpr int kRegPts = 4096;  // points of a scan per workgroup (16 rounds of 256): the closing reduction is paid once per 4096 points
int g_reg_blocks = 0;          // scvod__debug_register_blocks: workgroups per scan, 0 = by kRegPts (the sums may not depend on it)

struct RegK {  // what the kernels take
    const float4* pts;
    const int32_t* scan_off;
    const uint8_t* labels;  // or nullptr
    double* pose;           // [n_scans][12], the running pose
    scvod_register_record* rec;
    long long* sums;  // [n_scans][kRegWords]
    unsigned long long* totals;  // [8]
    unsigned long long use0, use1, use2, use3;
    float max_dist, r2, range2;
    // the map target
    const MapRec* table;
    unsigned long long mask;
    float inv_leaf, leaf;
    int sel;
    unsigned long long k0, k1, k2, k3;
    // the cloud target
    PointGrid grid;
    const float* tgt;
    const float* nrm;
    int n_tgt;
};

struct RegSolveK {
    long long min_corr;
    double lambda, pivot_eps, eps_rot, eps_trans;
};

// the poses of the call widened to fp64, the records and the sums cleared; one thread per scan (and per word of the sums)
__global__ __launch_bounds__(256) void k_reg_init(int n_scans, const float* __restrict__ pose32, const int32_t* __restrict__ scan_off, double* pose,
                                                  scvod_register_record* rec, long long* sums, unsigned long long* totals) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < 8) totals[t] = t == 0 ? (unsigned long long)n_scans : (t == 7 ? (unsigned long long)(scan_off[n_scans] - scan_off[0]) : 0ull);
    if (t < (long long)n_scans * kRegWords) sums[t] = 0;
    if (t < (long long)n_scans * 12) pose[t] = (double)pose32[t];
    if (t < n_scans) {
        scvod_register_record r;
        r.status = SCVOD_REG_MAX_ITERATIONS;
        r.iterations = 0;
        r.n_corr = 0;
        r.sum_r2 = 0.0;
        r.last_omega = 0.0;
        r.last_v = 0.0;
        r.skip_nan = r.skip_range = r.skip_label = r.skip_no_corr = r.skip_normal = 0;
        r.reserved = 0;
        rec[t] = r;
    }
}

// The 8 values v[] of every lane of a wave summed over the wave: afterwards lane L holds the sum of v[L >> 3].  A transposed butterfly:
// at each of the first three steps a lane hands the half of its values that its partner keeps across and adds what it receives to the
// half it keeps (4 + 2 + 1 shuffles of 64 bits), three plain steps finish the one value left.  Integer sums: the order does not matter.
template <int H>
__device__ __forceinline__ void reg_fold_step(long long* v, bool upper, int mask) {
#pragma unroll
    for (int k = 0; k < H; ++k) {
        const long long send = upper ? v[k] : v[k + H], keep = upper ? v[k + H] : v[k];
        v[k] = keep + __shfl_xor(send, mask);
    }
}
__device__ __forceinline__ long long reg_fold8(long long* v, int lane) {
    reg_fold_step<4>(v, (lane & 32) != 0, 32);
    reg_fold_step<2>(v, (lane & 16) != 0, 16);
    reg_fold_step<1>(v, (lane & 8) != 0, 8);
    long long x = v[0];
    x += __shfl_xor(x, 4);
    x += __shfl_xor(x, 2);
    x += __shfl_xor(x, 1);
    return x;
}

// Point mode needs 16 of the 28 sums: J = [ -[p]x , I ] makes the omega-v block of J^T J the sums of x, y, z (each once with either sign,
// reg_fix is odd), three of its entries and the off-diagonal of the v-v block exactly 0, and the v-v diagonal the count times 2^20.
// kPointPick: the terms that are folded; kPointWord / kPointNeg: the words a folded sum goes to, as it is and negated (-1: none).
//   words (row-major upper triangle): (wx,vy) 4 = -Z, (wx,vz) 5 = +Y, (wy,vx) 8 = +Z, (wy,vz) 10 = -X, (wz,vx) 12 = -Y, (wz,vy) 13 = +X
__device__ constexpr int kPointPick[16] = {0, 1, 2, 6, 7, 11, 13, 5, 8, 21, 22, 23, 24, 25, 26, 27};
__device__ constexpr int kPointNeg[16] = {-1, -1, -1, -1, -1, -1, 10, 12, 4, -1, -1, -1, -1, -1, -1, -1};

// TARGET 0: the static map, 1: a cloud.  MODE: SCVOD_REG_POINT / SCVOD_REG_PLANE.
// 256 threads, scan blockIdx.y, a grid-stride loop over the scan's points with non-temporal 16-byte loads of the stream (the table's or
// grid's lines keep the L2).  The terms of a point live only between its probe and the wave's fold (reg_fold8), after which each lane
// carries one running sum per part of eight terms over its whole stride (point mode: two parts, plane mode: four): 28 accumulators per lane held across the probe cost 56 registers on top of the probe's
// and left 3 waves per SIMD where the query runs 7; the kernel lives on waves in flight.  The five skip
// counters and the correspondences are wave-uniform (ballot + popcount, scalar registers).  The block adds its four waves once through
// LDS, then one 64-bit atomicAdd per word and block.  A latched scan returns at once.
template <int TARGET, int MODE>
__global__ __launch_bounds__(256) void k_reg_accumulate(int s_first, RegK a) {
    __shared__ long long red[4][kRegUsed];
    __shared__ double sT[12];
    __shared__ unsigned long long sUse[4];
    const int s = s_first + blockIdx.y;
    if (a.rec[s].status != SCVOD_REG_MAX_ITERATIONS) return;  // (the same for the whole block)
    const int base = a.scan_off[s];
    const int n = a.scan_off[s + 1] - base;
    if ((int)(blockIdx.x * 256) >= n) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // The fp64 pose and the label table wait in LDS and are read (volatile: not hoisted) where a correspondence needs them: held across
    // the probe they cost 32 scalar registers, which the probe's own state had spilled into vector lanes.  The fp32 pose stays scalar.
    if (threadIdx.x < 12) sT[threadIdx.x] = a.pose[12 * (size_t)s + threadIdx.x];
    if (threadIdx.x < 4) sUse[threadIdx.x] = threadIdx.x == 0 ? a.use0 : (threadIdx.x == 1 ? a.use1 : (threadIdx.x == 2 ? a.use2 : a.use3));
    __syncthreads();
    float Tf[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) Tf[i] = (float)a.pose[12 * (size_t)s + i];
    constexpr int kParts = MODE == SCVOD_REG_POINT ? 2 : 4;  // eight folded terms each
    long long mine[kParts];  // the running sums of folded terms 8 * part + (lane >> 3) (the same in the eight lanes of a group)
#pragma unroll
    for (int part = 0; part < kParts; ++part) mine[part] = 0;
    unsigned int n_corr = 0, n_nan = 0, n_range = 0, n_label = 0, n_none = 0, n_normal = 0;  // per wave (the same in every lane)
    for (int i0 = blockIdx.x * 256; i0 < n; i0 += gridDim.x * 256) {
        const int i = i0 + (int)threadIdx.x;
        const bool live = i < n;
        const size_t at = (size_t)base + (size_t)min(i, n - 1);
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v q4 = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(&a.pts[at]));
        const float p[3] = {q4.x, q4.y, q4.z};
        const int gate = reg_gate(p[0], p[1], p[2], a.range2);
        const bool is_nan = live && gate == 1, is_far = live && gate == 2;
        bool ok = live && gate == 0;
        bool no_label = false;
        if (ok && a.labels) {
            const unsigned int label = a.labels[at];
            no_label = !((((const volatile unsigned long long*)sUse)[label >> 6] >> (label & 63u)) & 1ull);
        }
        ok = ok && !no_label;
        float w[3];
        reg_move(Tf, p[0], p[1], p[2], w);
        float q[3] = {0.f, 0.f, 0.f};
        bool has = false;
        int bi = -1;
        if (TARGET == 0) {
            unsigned long long key = kEmpty, unused = kEmpty;
            if (!ok || !map_encode(w[0], w[1], w[2], 0.f, a.inv_leaf, key, unused)) key = kEmpty;
            unsigned long long h0, val;
            const bool found = mq_own_cell(a.table, a.mask, a.sel, a.k0, a.k1, a.k2, a.k3, lane, key, h0, val);  // (every lane of the wave calls)
            unsigned long long best_key = kEmpty;
            float best_d = __builtin_inff();
            mq_neighbours(a.table, a.mask, a.leaf, a.max_dist, a.r2, a.sel, a.k0, a.k1, a.k2, a.k3, key != kEmpty, w[0], w[1], w[2], key, h0, found, val,
                          best_key, best_d);
            has = best_key != kEmpty;
            if (has) {
                // the winner's value: the own cell's is at hand, a neighbour's is one more walk of a chain the lane just read
                unsigned long long bval = val;
                if (best_key != key) {
                    const unsigned long long bh = map_home(best_key, a.mask);
                    mq_find_from(a.table, a.mask, best_key, bh, map_peek(a.table, bh), bval);
                }
                const int cx = (int)(best_key >> (2 * kCellBits)) - kCellBias, cy = (int)((best_key >> kCellBits) & ((1u << kCellBits) - 1u)) - kCellBias,
                          cz = (int)(best_key & ((1u << kCellBits) - 1u)) - kCellBias;
                q[0] = map_decode(cx, (float)((bval >> 48) & 0xffffu), a.leaf);
                q[1] = map_decode(cy, (float)((bval >> 32) & 0xffffu), a.leaf);
                q[2] = map_decode(cz, (float)((bval >> 16) & 0xffffu), a.leaf);
            }
        } else {
            if (ok && a.n_tgt > 0) {
                float best = 0.f;
                grid_probe27(a.grid, a.tgt, 3, w[0], w[1], w[2], best, bi);
                has = bi >= 0 && best < a.r2;
                if (has) {
                    q[0] = a.tgt[3 * (size_t)bi];
                    q[1] = a.tgt[3 * (size_t)bi + 1];
                    q[2] = a.tgt[3 * (size_t)bi + 2];
                }
            }
        }
        float nv[3] = {0.f, 0.f, 0.f};
        if (MODE == SCVOD_REG_PLANE && has) {
            nv[0] = a.nrm[3 * (size_t)bi];
            nv[1] = a.nrm[3 * (size_t)bi + 1];
            nv[2] = a.nrm[3 * (size_t)bi + 2];
        }
        // The terms in parts of eight: each part evaluates the step's functions again and keeps its eight terms (the compiler
        // drops the rest), so that no more than eight terms are alive at once.  Point mode folds 16 terms (kPointPick), plane mode all 28.
        bool good = false;
        if (__ballot(has)) {
#pragma unroll
            for (int part = 0; part < kParts; ++part) {
                long long acc[kRegTerms];
#pragma unroll
                for (int k = 0; k < kRegTerms; ++k) acc[k] = 0;
                if (has) {
                    double T[12];
#pragma unroll
                    for (int k = 0; k < 12; ++k) T[k] = ((const volatile double*)sT)[k];
                    if (MODE == SCVOD_REG_POINT) {
                        reg_point_terms(T, p, q, acc);
                        good = true;
                    } else {
                        good = reg_plane_terms(T, p, q, nv, acc);
                    }
                }
                long long v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    v[k] = MODE == SCVOD_REG_POINT ? acc[kPointPick[8 * part + k]] : (8 * part + k < kRegTerms ? acc[8 * part + k] : 0);
                mine[part] += reg_fold8(v, lane);
            }
        }
        const bool bad_normal = has && !good;
        const unsigned long long with_terms = __ballot(has && good);
        n_corr += (unsigned int)__popcll(with_terms);
        n_nan += (unsigned int)__popcll(__ballot(is_nan));
        n_range += (unsigned int)__popcll(__ballot(is_far));
        n_label += (unsigned int)__popcll(__ballot(no_label));
        n_none += (unsigned int)__popcll(__ballot(ok && !has));
        n_normal += (unsigned int)__popcll(__ballot(bad_normal));
    }
    if (lane < kRegUsed) red[wave][lane] = 0;  // (the wave's LDS operations complete in order)
    if (!(lane & 7)) {
#pragma unroll
        for (int part = 0; part < kParts; ++part) {
            const int f = 8 * part + (lane >> 3);
            if (MODE == SCVOD_REG_POINT) {
                red[wave][kPointPick[f]] = mine[part];
                if (kPointNeg[f] >= 0) red[wave][kPointNeg[f]] = -mine[part];
            } else if (f < kRegTerms) {
                red[wave][f] = mine[part];
            }
        }
    }
    if (lane == 0) {
        if (MODE == SCVOD_REG_POINT) red[wave][15] = red[wave][18] = red[wave][20] = (long long)n_corr << 20;  // the v-v diagonal
        red[wave][kRegCorr] = (long long)n_corr;
        red[wave][kRegSkip + 0] = (long long)n_nan;
        red[wave][kRegSkip + 1] = (long long)n_range;
        red[wave][kRegSkip + 2] = (long long)n_label;
        red[wave][kRegSkip + 3] = (long long)n_none;
        red[wave][kRegSkip + 4] = (long long)n_normal;
    }
    __syncthreads();
    if (threadIdx.x < kRegUsed) {
        const long long v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(&a.sums[(size_t)kRegWords * s + threadIdx.x]), (unsigned long long)v);
    }
}

// one thread per scan: the solve and the update of scvod_math.h, the record, the latch; the sums are left cleared for the next round
__global__ __launch_bounds__(64) void k_reg_solve(int n_scans, RegSolveK k, double* pose, scvod_register_record* rec, long long* sums,
                                                 unsigned long long* totals, int last) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_scans) return;
    scvod_register_record r = rec[s];
    if (r.status != SCVOD_REG_MAX_ITERATIONS) return;
    long long w[kRegUsed];
#pragma unroll
    for (int i = 0; i < kRegUsed; ++i) {
        w[i] = sums[(size_t)kRegWords * s + i];
        sums[(size_t)kRegWords * s + i] = 0;
    }
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = pose[12 * (size_t)s + i];
    double on, vn;
    const int status = reg_solve_update(w, k.min_corr, k.lambda, k.pivot_eps, k.eps_rot, k.eps_trans, T, &on, &vn);
    if (status != kRegDegenerate) {
#pragma unroll
        for (int i = 0; i < 12; ++i) pose[12 * (size_t)s + i] = T[i];
    }
    r.status = status;
    r.iterations += 1;
    r.n_corr = w[kRegCorr];
    r.sum_r2 = (double)w[kRegR2] * kRegInvScale;
    r.last_omega = on;
    r.last_v = vn;
    r.skip_nan = (int32_t)w[kRegSkip];
    r.skip_range = (int32_t)w[kRegSkip + 1];
    r.skip_label = (int32_t)w[kRegSkip + 2];
    r.skip_no_corr = (int32_t)w[kRegSkip + 3];
    r.skip_normal = (int32_t)w[kRegSkip + 4];
    rec[s] = r;
    if (status != kRegGo || last) {
        atomicAdd(&totals[1 + (status == kRegConverged ? 0 : (status == kRegGo ? 1 : 2))], 1ull);
        atomicAdd(&totals[4], (unsigned long long)w[kRegCorr]);
        atomicAdd(&totals[5], (unsigned long long)r.iterations);
        atomicAdd(&totals[6], (unsigned long long)(w[kRegSkip] + w[kRegSkip + 1] + w[kRegSkip + 2] + w[kRegSkip + 3] + w[kRegSkip + 4]));
    }
}

// what hangs on a map or a ctx: one grow-only block, the staging of poses and offsets, the last call's stream
struct RegState {
    unsigned char* buf = nullptr;
    size_t cap = 0;
    hipStream_t stream = nullptr;
    bool ran = false;
    std::vector<float> up_pose;    // what the block holds at the pose32 / offs place of the last call's layout; empty: nothing to rely on
    std::vector<int32_t> up_offs;
    int last_scans = -1;           // the places of pose32 and offs in the block depend on n_scans alone
    std::string err;
};

size_t reg_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct RegLayout {
    size_t pose32, offs, sums, totals, grid, bytes;
};
RegLayout reg_layout(int n_scans, bool own_offs, size_t grid_ints) {
    RegLayout L;
    size_t o = 0;
    L.totals = o;
    o = reg_up(o + 8 * sizeof(unsigned long long));
    L.sums = o;
    o = reg_up(o + sizeof(long long) * kRegWords * (size_t)(n_scans > 0 ? n_scans : 1));
    L.pose32 = o;
    o = reg_up(o + sizeof(float) * 12 * (size_t)(n_scans > 0 ? n_scans : 1));
    L.offs = o;
    o = reg_up(o + (own_offs ? sizeof(int32_t) * ((size_t)n_scans + 1) : 0));
    L.grid = o;
    o = reg_up(o + sizeof(int) * grid_ints);
    L.bytes = o;
    return L;
}

const char* reg_check(const scvod_register_params& p, float leaf, int has_normals, const void* d_src) {
    if (p.max_iterations < 1 || p.max_iterations > 64) return "max_iterations outside 1 .. 64";
    if (p.min_corr < 6) return "min_corr below 6";
    if (p.mode != SCVOD_REG_POINT && p.mode != SCVOD_REG_PLANE) return "unknown mode";
    if (p.reserved != 0) return "reserved must be 0";
    if (!(p.max_dist > 0.f) || !(p.max_dist <= 256.f)) return "max_dist outside (0, 256]";
    if (!(p.max_range > 0.f)) return "max_range must be positive";
    if (!(p.eps_rot >= 0.0) || !(p.eps_trans >= 0.0) || !(p.lambda >= 0.0) || !(p.pivot_eps >= 0.0)) return "eps_rot, eps_trans, lambda and pivot_eps must be >= 0";
    if (leaf > 0.f) {
        if (p.max_dist > 0.99f * leaf) return "max_dist above 0.99 * leaf";
        if (p.mode != SCVOD_REG_POINT) return "the map target is point-to-point only";
    } else if (p.mode == SCVOD_REG_PLANE && !has_normals) {
        return "plane mode needs target normals";
    }
    if ((uintptr_t)d_src & 15u) return "the source cloud is not 16-byte aligned";
    return nullptr;
}

struct RegCall {
    RegState** slot;
    int device;
    const float4* pts;
    const int32_t* h_offs;  // ctx-free: staged; nullptr: d_offs is the batch's
    const int32_t* d_offs;
    int n_scans, max_pts;
    const float* h_poses;
    const uint8_t* labels;
    scvod_register_params p;
    double* pose_out;
    scvod_register_record* rec;
    // map target
    scvod_map* map;
    const uint8_t* h_select256;
    // cloud target
    const float* tgt;
    const float* nrm;
    int n_tgt;
};

#define RHIP(call)                                                                  \
    do {                                                                            \
        hipError_t e__ = (call);                                                    \
        if (e__ != hipSuccess) {                                                    \
            err = std::string(#call) + ": " + hipGetErrorString(e__);              \
            return SCVOD_ERR_HIP;                                                   \
        }                                                                           \
    } while (0)

// the whole call, after its argument checks
int reg_run(const RegCall& c, hipStream_t st, std::string& err) {
    RHIP(hipSetDevice(c.device));
    if (!*c.slot) *c.slot = new RegState();
    RegState& R = **c.slot;
    if (R.ran && R.stream != st) RHIP(hipStreamSynchronize(R.stream));  // the block and the totals are shared
    const bool cloud = c.map == nullptr;
    float cell = 0.f;
    int32_t buckets = 0;
    size_t grid_ints = 0;
    if (cloud && c.n_tgt > 0) {
        cell = c.p.max_dist > 0.2f ? c.p.max_dist : 0.2f;
        if (c.p.max_dist * c.p.max_dist > (0.99f * cell) * (0.99f * cell)) cell = c.p.max_dist / 0.98f;
        buckets = grid_buckets(c.n_tgt);
        grid_ints = grid_work_ints(buckets, c.n_tgt);
    }
    const RegLayout L = reg_layout(c.n_scans, c.h_offs != nullptr, grid_ints);
    if (L.bytes > R.cap) {
        if (R.ran) RHIP(hipStreamSynchronize(R.stream));
        if (R.buf) hipFree(R.buf);
        R.buf = nullptr;
        R.cap = 0;
        R.up_pose.clear();
        R.up_offs.clear();
        const size_t grown = L.bytes + L.bytes / 4;
        RHIP(hipMalloc(&R.buf, grown));
        R.cap = grown;
    }
    // What was staged is only there while the layout stands: with another n_scans the sums of this call lie where the poses or
    // offsets of the last one lay, and a batch call (offsets of the ctx) says nothing about the staged offsets of the call after it.
    if (c.n_scans != R.last_scans) R.up_pose.clear();
    if (c.n_scans != R.last_scans || !c.h_offs) R.up_offs.clear();
    R.last_scans = c.n_scans;
    R.stream = st;
    R.ran = true;
    unsigned long long* totals = (unsigned long long*)(R.buf + L.totals);
    if (c.n_scans <= 0) {
        RHIP(hipMemsetAsync(totals, 0, 8 * sizeof(unsigned long long), st));
        return SCVOD_OK;
    }
    // the poses as fp32 matrices and the offsets, staged like the map's (a staging vector may still feed an earlier copy)
    const float zero[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    std::vector<float> T32((size_t)12 * c.n_scans);
    for (int s = 0; s < c.n_scans; ++s) scvod_pose_matrix(c.h_poses ? c.h_poses + 6 * s : zero, T32.data() + 12 * s);
    float* d_pose32 = (float*)(R.buf + L.pose32);
    if (R.up_pose != T32) {
        RHIP(hipStreamSynchronize(st));
        R.up_pose = T32;
        RHIP(hipMemcpyAsync(d_pose32, R.up_pose.data(), sizeof(float) * T32.size(), hipMemcpyHostToDevice, st));
    }
    const int32_t* d_offs = c.d_offs;
    if (c.h_offs) {
        const std::vector<int32_t> offs(c.h_offs, c.h_offs + c.n_scans + 1);
        if (R.up_offs != offs) {
            RHIP(hipStreamSynchronize(st));
            R.up_offs = offs;
            RHIP(hipMemcpyAsync(R.buf + L.offs, R.up_offs.data(), sizeof(int32_t) * offs.size(), hipMemcpyHostToDevice, st));
        }
        d_offs = (const int32_t*)(R.buf + L.offs);
    }
    RegK a;
    memset(&a, 0, sizeof(a));
    a.pts = c.pts;
    a.scan_off = d_offs;
    a.labels = c.labels;
    a.pose = c.pose_out;
    a.rec = c.rec;
    a.sums = (long long*)(R.buf + L.sums);
    a.totals = totals;
    unsigned long long use[4];
    map_table256(c.labels ? c.p.use256 : nullptr, use);
    a.use0 = use[0], a.use1 = use[1], a.use2 = use[2], a.use3 = use[3];
    a.max_dist = c.p.max_dist;
    a.r2 = c.p.max_dist * c.p.max_dist;
    a.range2 = c.p.max_range * c.p.max_range;
    if (!cloud) {
        unsigned long long k[4];
        map_table256(c.h_select256, k);
        a.table = c.map->table;
        a.mask = (unsigned long long)(c.map->capacity - 1);
        a.inv_leaf = 1.0f / c.map->leaf;
        a.leaf = c.map->leaf;
        a.sel = c.h_select256 ? 1 : 0;
        a.k0 = k[0], a.k1 = k[1], a.k2 = k[2], a.k3 = k[3];
    } else {
        a.tgt = c.tgt;
        a.nrm = c.nrm;
        a.n_tgt = c.n_tgt;
        if (c.n_tgt > 0) a.grid = grid_build(c.tgt, 3, nullptr, c.n_tgt, kGridOrigin0, cell, buckets, (int*)(R.buf + L.grid), st);
    }
    const long long init_threads = (long long)c.n_scans * kRegWords;
    hipLaunchKernelGGL(k_reg_init, dim3((unsigned)((init_threads + 255) / 256)), dim3(256), 0, st, c.n_scans, d_pose32, d_offs, c.pose_out, c.rec, a.sums,
                       totals);
    const RegSolveK k = {(long long)c.p.min_corr, c.p.lambda, c.p.pivot_eps, c.p.eps_rot, c.p.eps_trans};
    int bx = g_reg_blocks > 0 ? g_reg_blocks : (c.max_pts + kRegPts - 1) / kRegPts;
    if (bx < 1) bx = 1;
    constexpr int kMaxGridY = 65535;
    for (int it = 0; it < c.p.max_iterations; ++it) {
        for (int s0 = 0; s0 < c.n_scans && c.max_pts > 0; s0 += kMaxGridY) {
            const int ny = c.n_scans - s0 < kMaxGridY ? c.n_scans - s0 : kMaxGridY;
            const dim3 grid(bx, ny), block(256);
            if (!cloud)
                hipLaunchKernelGGL((k_reg_accumulate<0, SCVOD_REG_POINT>), grid, block, 0, st, s0, a);
            else if (c.p.mode == SCVOD_REG_POINT)
                hipLaunchKernelGGL((k_reg_accumulate<1, SCVOD_REG_POINT>), grid, block, 0, st, s0, a);
            else
                hipLaunchKernelGGL((k_reg_accumulate<1, SCVOD_REG_PLANE>), grid, block, 0, st, s0, a);
        }
        hipLaunchKernelGGL(k_reg_solve, dim3((c.n_scans + 63) / 64), dim3(64), 0, st, c.n_scans, k, c.pose_out, c.rec, a.sums, totals,
                           it + 1 == c.p.max_iterations ? 1 : 0);
    }
    RHIP(hipGetLastError());
    return SCVOD_OK;
}

int reg_stats(RegState* R, int device, int64_t* h_out8, std::string& err) {
    RHIP(hipSetDevice(device));
    RHIP(hipStreamSynchronize(R->stream));
    unsigned long long h[8] = {0};
    RHIP(hipMemcpy(h, R->buf, sizeof(h), hipMemcpyDeviceToHost));  // (the totals lead the block)
    for (int i = 0; i < 8; ++i) h_out8[i] = (int64_t)h[i];
    return SCVOD_OK;
}

scvod_register_params reg_params(const scvod_register_params* params) {
    scvod_register_params p;
    if (params)
        p = *params;
    else
        scvod_register_params_default(&p);
    return p;
}

// the argument checks the two map calls share
int reg_map_check(scvod_map* m, const scvod_register_params& p, const void* d_xyzi, const uint8_t* h_select256, const double* d_pose_out,
                  const void* d_records) {
    if (const char* why = reg_check(p, m->leaf, 0, d_xyzi)) return mfail(m, SCVOD_ERR_INVALID, "scvod_map_register: %s", why);
    if (h_select256 && m->kind != SCVOD_MAP_KIND_LABELLED) return mfail(m, SCVOD_ERR_INVALID, "a select table needs a map of kind SCVOD_MAP_KIND_LABELLED");
    if (!d_pose_out || !d_records || ((uintptr_t)d_pose_out & 7u) || ((uintptr_t)d_records & 7u))
        return mfail(m, SCVOD_ERR_INVALID, "d_pose_out and d_records are required and 8-byte aligned");
    return SCVOD_OK;
}

}  // namespace
}  // namespace scvod

extern "C" {

void scvod__register_free(void* state) {
    RegState* R = (RegState*)state;
    if (!R) return;
    if (R->buf) hipFree(R->buf);
    delete R;
}

// development only: workgroups per scan of k_reg_accumulate (0: the default); the results may not depend on it
void scvod__debug_register_blocks(int blocks) { g_reg_blocks = blocks; }

void scvod_register_params_default(scvod_register_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_iterations = 10;
    p->min_corr = 30;
    p->mode = SCVOD_REG_POINT;
    p->max_dist = 0.19f;
    p->max_range = 80.f;
    p->eps_rot = 1e-6;
    p->eps_trans = 1e-5;
    p->lambda = 0.0;
    p->pivot_eps = 1e-9;
    p->use256 = nullptr;
}

int scvod_register_check(const scvod_register_params* params, float leaf, int32_t has_normals, const void* d_src_xyzi) {
    if (!(leaf >= 0.f)) return SCVOD_ERR_INVALID;
    return reg_check(reg_params(params), leaf, has_normals, d_src_xyzi) ? SCVOD_ERR_INVALID : SCVOD_OK;
}

int scvod_map_register(scvod_map* m, const void* d_xyzi, const int32_t* h_scan_offsets, int32_t n_scans, const float* h_poses, const uint8_t* d_labels,
                       const scvod_register_params* params, const uint8_t* h_select256, double* d_pose_out, void* d_records, void* stream) {
    if (!m || n_scans < 0 || (n_scans > 0 && !h_scan_offsets)) return mfail(m, SCVOD_ERR_INVALID, "bad arguments");
    const scvod_register_params p = reg_params(params);
    if (int rc = reg_map_check(m, p, d_xyzi, h_select256, d_pose_out, d_records)) return rc;
    int max_pts = 0;
    if (n_scans > 0)
        if (int rc = map_check_offsets(m, h_scan_offsets, n_scans, &max_pts)) return rc;
    if (max_pts > 0 && !d_xyzi) return mfail(m, SCVOD_ERR_INVALID, "NULL points of a cloud that is not empty");
    RegCall c;
    memset(&c, 0, sizeof(c));
    c.slot = (RegState**)&m->reg_state;
    c.device = m->device;
    c.pts = (const float4*)d_xyzi;
    c.h_offs = h_scan_offsets;
    c.n_scans = n_scans;
    c.max_pts = max_pts;
    c.h_poses = h_poses;
    c.labels = d_labels;
    c.p = p;
    c.pose_out = d_pose_out;
    c.rec = (scvod_register_record*)d_records;
    c.map = m;
    c.h_select256 = h_select256;
    const int rc = reg_run(c, (hipStream_t)stream, m->err);
    return rc;
}

int scvod_batch_map_register(scvod_ctx* ctx, scvod_map* m, const float* h_poses, const uint8_t* d_labels, const scvod_register_params* params,
                             const uint8_t* h_select256, double* d_pose_out, void* d_records, void* stream) {
    if (!ctx || !m || !h_poses) return mfail(m, SCVOD_ERR_INVALID, "bad arguments");
    const scvod_register_params p = reg_params(params);
    Arena A;
    int device = 0, track_valid = 0, batch_valid = 0, n_scans = 0, max_pts = 0, mode = 0, min_pts = 0;
    scvod__ctx_view(ctx, &A, &device, &track_valid, &batch_valid, &n_scans, &max_pts, &mode, &min_pts);
    if (int rc = reg_map_check(m, p, A.pts, h_select256, d_pose_out, d_records)) return rc;
    if (!batch_valid || !A.pts) return mfail(m, SCVOD_ERR_STATE, "scvod_batch_map_register needs a processed batch of input clouds");
    if (device != m->device) return mfail(m, SCVOD_ERR_INVALID, "map and ctx live on different devices");
    RegCall c;
    memset(&c, 0, sizeof(c));
    c.slot = (RegState**)&m->reg_state;
    c.device = m->device;
    c.pts = (const float4*)A.pts;
    c.d_offs = A.scan_off;
    c.n_scans = n_scans;
    c.max_pts = max_pts;
    c.h_poses = h_poses;
    c.labels = d_labels;
    c.p = p;
    c.pose_out = d_pose_out;
    c.rec = (scvod_register_record*)d_records;
    c.map = m;
    c.h_select256 = h_select256;
    return reg_run(c, (hipStream_t)scvod__ctx_stream(ctx, stream), m->err);
}

int scvod_map_register_stats(scvod_map* m, int64_t* h_out8) {
    if (!m || !h_out8) return mfail(m, SCVOD_ERR_INVALID, "bad arguments");
    RegState* R = (RegState*)m->reg_state;
    if (!R || !R->ran) return mfail(m, SCVOD_ERR_STATE, "scvod_map_register_stats before the first call");
    return reg_stats(R, m->device, h_out8, m->err);
}

int64_t scvod_map_register_scratch_bytes(const scvod_map* m) { return (m && m->reg_state) ? (int64_t)((RegState*)m->reg_state)->cap : 0; }

int scvod_register_device(scvod_ctx* ctx, const void* d_src_xyzi, const int32_t* h_scan_offsets, int32_t n_scans, const float* h_poses,
                          const uint8_t* d_labels, const float* d_tgt_xyz, const float* d_tgt_normals, int32_t n_tgt, const scvod_register_params* params,
                          double* d_pose_out, void* d_records, void* stream) {
    if (!ctx) return SCVOD_ERR_INVALID;
    if (n_scans < 0 || (n_scans > 0 && !h_scan_offsets) || n_tgt < 0 || (n_tgt > 0 && !d_tgt_xyz))
        return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "bad arguments");
    const scvod_register_params p = reg_params(params);
    if (const char* why = reg_check(p, 0.f, d_tgt_normals != nullptr, d_src_xyzi))
        return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, (std::string("scvod_register_device: ") + why).c_str());
    if (!d_pose_out || !d_records || ((uintptr_t)d_pose_out & 7u) || ((uintptr_t)d_records & 7u))
        return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "d_pose_out and d_records are required and 8-byte aligned");
    int max_pts = 0;
    if (n_scans > 0) {
        if (h_scan_offsets[0] < 0) return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "scan offsets start below 0");
        for (int s = 0; s < n_scans; ++s) {
            if (h_scan_offsets[s + 1] < h_scan_offsets[s]) return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "scan offsets decrease");
            if (h_scan_offsets[s + 1] - h_scan_offsets[s] > max_pts) max_pts = h_scan_offsets[s + 1] - h_scan_offsets[s];
        }
    }
    if (max_pts > 0 && !d_src_xyzi) return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "NULL points of a cloud that is not empty");
    int device = 0;
    void* own = nullptr;
    void** slot = scvod__ctx_register_slot(ctx, &device, &own);
    RegCall c;
    memset(&c, 0, sizeof(c));
    c.slot = (RegState**)slot;
    c.device = device;
    c.pts = (const float4*)d_src_xyzi;
    c.h_offs = h_scan_offsets;
    c.n_scans = n_scans;
    c.max_pts = max_pts;
    c.h_poses = h_poses;
    c.labels = d_labels;
    c.p = p;
    c.pose_out = d_pose_out;
    c.rec = (scvod_register_record*)d_records;
    c.tgt = d_tgt_xyz;
    c.nrm = d_tgt_normals;
    c.n_tgt = n_tgt;
    std::string err;
    const int rc = reg_run(c, stream ? (hipStream_t)stream : (hipStream_t)own, err);
    return rc ? scvod__ctx_fail(ctx, rc, err.c_str()) : SCVOD_OK;
}

int scvod_register_stats(scvod_ctx* ctx, int64_t* h_out8) {
    if (!ctx) return SCVOD_ERR_INVALID;
    if (!h_out8) return scvod__ctx_fail(ctx, SCVOD_ERR_INVALID, "bad arguments");
    int device = 0;
    void* own = nullptr;
    RegState* R = (RegState*)*scvod__ctx_register_slot(ctx, &device, &own);
    if (!R || !R->ran) return scvod__ctx_fail(ctx, SCVOD_ERR_STATE, "scvod_register_stats before the first call");
    std::string err;
    const int rc = reg_stats(R, device, h_out8, err);
    return rc ? scvod__ctx_fail(ctx, rc, err.c_str()) : SCVOD_OK;
}

int64_t scvod_register_scratch_bytes(scvod_ctx* ctx) {
    if (!ctx) return 0;
    int device = 0;
    void* own = nullptr;
    RegState* R = (RegState*)*scvod__ctx_register_slot(ctx, &device, &own);
    return R ? (int64_t)R->cap : 0;
}

}  // extern "C"
