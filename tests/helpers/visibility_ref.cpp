// Brute-force restatement of the seen-through vote (include/scvod.h: scvod_visibility_device) -- test infrastructure only.
// Plain loops over (scan, viewer, point, window): no tiles, no guarded estimate, every point through apri_of_point of the product's own
// scvod_math.h compiled for the host.  The viewer lists and the matrices are inputs (tests/helpers/visibility_ref.py builds them).
#include <cmath>
#include <cstdint>
#include <limits>

#include "../../dr-using-scv-od_amd/csrc/scvod_math.h"

using namespace scvod;

namespace {

BinParams grid_of(const float* g9, const int* dims3) {
    BinParams g;
    g.min_dis = g9[0];
    g.max_dis = g9[1];
    g.min_angle = g9[2];
    g.max_angle = g9[3];
    g.min_azimuth = g9[4];
    g.max_azimuth = g9[5];
    g.range_res = g9[6];
    g.sector_res = g9[7];
    g.azimuth_res = g9[8];
    g.range_num = dims3[0];
    g.sector_num = dims3[1];
    g.azimuth_num = dims3[2];
    g.bin_num = dims3[0] * dims3[1] * dims3[2];
    return g;
}

bool finite3(float x, float y, float z) { return std::isfinite(x) && std::isfinite(y) && std::isfinite(z); }

}  // namespace

extern "C" {

// classes of a pair as this helper reports them (the library packs 3 and 4 into one byte counter)
enum { THROUGH = 0, AGREE = 1, OCCLUDED = 2, OUTSIDE = 3, EMPTY = 4 };

// g9 / dims3: the grid (min_dis, max_dis, min_angle, max_angle, min_azimuth, max_azimuth, range_res, sector_res, azimuth_res; range /
// sector / azimuth bins).  xyzi [off[n_scans]][4]; begin [n_scans + 1] / viewers / T [pairs][12]: per scan its viewers and the matrix
// into each; mask [points] or NULL; ip = {halo, min_through, vote_num, vote_den}; fp = {gap_abs, gap_rel}.
// images [n_scans][A * S]; votes, verdict [points]; scan_counts [n_scans][6]; pair_class: for pair k of scan j the n_j classes at pc_off[k].
void vis_ref(const float* g9, const int* dims3, const float* xyzi, const int* off, int n_scans, const int* begin, const int* viewers,
             const float* T, const unsigned char* mask, const int* ip, const float* fp, float* images, uint32_t* votes, unsigned char* verdict,
             long long* scan_counts, unsigned char* pair_class, const long long* pc_off) {
    const BinParams g = grid_of(g9, dims3);
    const int S = g.sector_num, A = g.azimuth_num;
    const float inf = std::numeric_limits<float>::infinity();
    const int halo = ip[0], min_through = ip[1], vote_num = ip[2], vote_den = ip[3];
    const float gap_abs = fp[0], gap_rel = fp[1];
    for (long long k = 0; k < (long long)n_scans * A * S; ++k) images[k] = inf;
    for (int s = 0; s < n_scans; ++s) {
        float* img = images + (long long)s * A * S;
        for (int i = off[s]; i < off[s + 1]; ++i) {
            const float x = xyzi[4 * (long long)i], y = xyzi[4 * (long long)i + 1], z = xyzi[4 * (long long)i + 2];
            if (!finite3(x, y, z)) continue;
            Apri a;
            if (!apri_of_point(g, x, y, z, 0.f, a)) continue;
            if (a.sector_idx < 0 || a.sector_idx >= S || a.azimuth_idx < 0 || a.azimuth_idx >= A) continue;
            float& px = img[a.azimuth_idx * S + a.sector_idx];
            if (a.range < px) px = a.range;
        }
    }
    for (int j = 0; j < n_scans; ++j) {
        long long* sc = scan_counts + 6 * (long long)j;
        for (int f = 0; f < 6; ++f) sc[f] = 0;
        const int nv = begin[j + 1] - begin[j];
        for (int i = off[j]; i < off[j + 1]; ++i) {
            const bool query = !mask || mask[i];
            const float qx = xyzi[4 * (long long)i], qy = xyzi[4 * (long long)i + 1], qz = xyzi[4 * (long long)i + 2];
            int n[5] = {0, 0, 0, 0, 0};
            for (int k = begin[j]; k < begin[j + 1]; ++k) {
                const float* M = T + 12 * (long long)k;
                const float* img = images + (long long)viewers[k] * A * S;
                int cls;
                // left to right in fp32, no contraction (the build passes -ffp-contract=off)
                const float x = M[0] * qx + M[1] * qy + M[2] * qz + M[3];
                const float y = M[4] * qx + M[5] * qy + M[6] * qz + M[7];
                const float z = M[8] * qx + M[9] * qy + M[10] * qz + M[11];
                Apri a;
                if (!finite3(x, y, z) || !apri_of_point(g, x, y, z, 0.f, a) || a.sector_idx < 0 || a.sector_idx >= S || a.azimuth_idx < 0 ||
                    a.azimuth_idx >= A) {
                    cls = OUTSIDE;
                } else {
                    const float dis = a.range;
                    const float gap = gap_abs + gap_rel * dis;
                    float r_min = inf;
                    bool agree = false;
                    for (int ai = a.azimuth_idx - halo; ai <= a.azimuth_idx + halo; ++ai)
                        for (int si = a.sector_idx - halo; si <= a.sector_idx + halo; ++si) {
                            if (ai < 0 || ai >= A || si < 0 || si >= S) continue;  // clipped, no wrap across the sector seam
                            const float r = img[ai * S + si];
                            if (r < r_min) r_min = r;
                            if (std::fabs(r - dis) <= gap) agree = true;
                        }
                    if (r_min == inf)
                        cls = EMPTY;
                    else if (r_min > dis + gap)
                        cls = THROUGH;
                    else if (agree)
                        cls = AGREE;
                    else
                        cls = OCCLUDED;
                }
                if (pair_class) pair_class[pc_off[k] + (i - off[j])] = (unsigned char)cls;
                if (query) ++n[cls];
            }
            uint32_t v = 0;
            unsigned char vd = 0;
            if (query) {
                v = (uint32_t)n[THROUGH] | ((uint32_t)n[AGREE] << 8) | ((uint32_t)n[OCCLUDED] << 16) | ((uint32_t)(n[OUTSIDE] + n[EMPTY]) << 24);
                if (nv > 0) vd = (n[THROUGH] >= min_through && n[THROUGH] * vote_den >= vote_num * (n[THROUGH] + n[AGREE])) ? 2 : 1;
                sc[0] += 1;
                sc[1] += vd == 2;
                sc[2] += n[THROUGH];
                sc[3] += n[AGREE];
                sc[4] += n[OCCLUDED];
                sc[5] += n[OUTSIDE] + n[EMPTY];
            }
            votes[i] = v;
            verdict[i] = vd;
        }
    }
}

}  // extern "C"
