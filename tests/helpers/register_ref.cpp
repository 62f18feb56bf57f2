// CPU statement of scvod_map_register / scvod_register_device (register_ref.py) -- test infrastructure only.  A plain sequential loop
// over scans, iterations and points that calls the reg_* functions of the library's scvod_math.h, with an EXHAUSTIVE search for the
// correspondence (every target point, the target's tie rule); no part of the kernels.  Built by the tests with -ffp-contract=off, as
// the library is.
#include <cstdint>
#include <cstring>

#include "../../dr-using-scv-od_amd/csrc/scvod_math.h"

using namespace scvod;

namespace {
struct Record {  // scvod_register_record
    int32_t status, iterations;
    int64_t n_corr;
    double sum_r2, last_omega, last_v;
    int32_t skip_nan, skip_range, skip_label, skip_no_corr, skip_normal, reserved;
};
static_assert(sizeof(Record) == 64, "record");
}  // namespace

extern "C" {

// src [n][4], offs [n_scans + 1], pose32 [n_scans][12] (the fp32 matrices of the start poses), labels [n] or NULL, use256 [256] or NULL.
// Target: tgt_xyz [n_tgt][3]; tgt_key [n_tgt] (the map: ties to the smaller key) or NULL (a cloud: ties to the lowest index);
// tgt_nrm [n_tgt][3] or NULL.  Outputs: pose_out [n_scans][12], records [n_scans] x 64 bytes, sums [n_scans][34] = the int64 sums of the
// last accumulation each scan took part in, match0 [n] = the target index of every source point at iteration 0 (-1: none), or NULL.
void register_ref(const float* src, const int* offs, int n_scans, const float* pose32, const unsigned char* labels, const unsigned char* use256,
                  const float* tgt_xyz, const unsigned long long* tgt_key, const float* tgt_nrm, int n_tgt, int max_iterations, int min_corr, int mode,
                  float max_dist, float max_range, double eps_rot, double eps_trans, double lambda, double pivot_eps, double* pose_out,
                  void* records, long long* sums, int* match0) {
    const float r2 = max_dist * max_dist, range2 = max_range * max_range;
    for (int s = 0; s < n_scans; ++s) {
        double* T = pose_out + 12 * s;
        for (int i = 0; i < 12; ++i) T[i] = (double)pose32[12 * s + i];
        Record rec;
        std::memset(&rec, 0, sizeof(rec));
        long long* w = sums + (size_t)kRegUsed * s;
        for (int i = 0; i < kRegUsed; ++i) w[i] = 0;
        for (int it = 0; it < max_iterations && rec.status == kRegGo; ++it) {
            for (int i = 0; i < kRegUsed; ++i) w[i] = 0;
            float Tf[12];
            reg_pose32(T, Tf);
            for (int i = offs[s]; i < offs[s + 1]; ++i) {
                const float* p = src + 4 * (size_t)i;
                if (it == 0 && match0) match0[i] = -1;
                const int gate = reg_gate(p[0], p[1], p[2], range2);
                if (gate) {
                    ++w[kRegSkip + gate - 1];
                    continue;
                }
                if (labels && use256 && !use256[labels[i]]) {
                    ++w[kRegSkip + 2];
                    continue;
                }
                float x[3];
                reg_move(Tf, p[0], p[1], p[2], x);
                int best = -1;
                float best_d = 0.f;
                for (int m = 0; m < n_tgt; ++m) {
                    const float dx = x[0] - tgt_xyz[3 * (size_t)m], dy = x[1] - tgt_xyz[3 * (size_t)m + 1], dz = x[2] - tgt_xyz[3 * (size_t)m + 2];
                    const float d = (dx * dx + dy * dy) + dz * dz;
                    if (!(d < r2)) continue;
                    if (best < 0 || d < best_d || (d == best_d && tgt_key && tgt_key[m] < tgt_key[best])) {
                        best = m;
                        best_d = d;
                    }
                }
                if (it == 0 && match0) match0[i] = best;
                if (best < 0) {
                    ++w[kRegSkip + 3];
                    continue;
                }
                if (mode == 0) {
                    reg_point_terms(T, p, tgt_xyz + 3 * (size_t)best, w);
                } else if (!reg_plane_terms(T, p, tgt_xyz + 3 * (size_t)best, tgt_nrm + 3 * (size_t)best, w)) {
                    ++w[kRegSkip + 4];
                    continue;
                }
                ++w[kRegCorr];
            }
            double on, vn;
            rec.status = reg_solve_update(w, min_corr, lambda, pivot_eps, eps_rot, eps_trans, T, &on, &vn);
            rec.iterations = it + 1;
            rec.n_corr = w[kRegCorr];
            rec.sum_r2 = (double)w[kRegR2] * kRegInvScale;
            rec.last_omega = on;
            rec.last_v = vn;
            rec.skip_nan = (int32_t)w[kRegSkip];
            rec.skip_range = (int32_t)w[kRegSkip + 1];
            rec.skip_label = (int32_t)w[kRegSkip + 2];
            rec.skip_no_corr = (int32_t)w[kRegSkip + 3];
            rec.skip_normal = (int32_t)w[kRegSkip + 4];
        }
        std::memcpy((char*)records + 64 * (size_t)s, &rec, sizeof(rec));
    }
}

}  // extern "C"
