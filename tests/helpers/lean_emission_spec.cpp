// CPU side of tests/test_gpu_lean_emission.py: the product's own scvod_math.h, compiled for the host.
// The lean emission recomputes a kept point's voxel key from the PACKED index triple (pack_idx3 -> unpack_idx3); this counts the
// points for which that key differs from apri_of_point's voxel_idx, and reports how far the indices of kept points reach.
#include "../../dr-using-scv-od_amd/csrc/scvod_math.h"

using namespace scvod;

extern "C" {

// g9: min_dis, max_dis, min_angle, max_angle, min_azimuth, max_azimuth, range_res, sector_res, azimuth_res; dims3: range / sector /
// azimuth bins; xyz: n points.  out[0] kept points, out[1] kept points whose recomputed key differs, out[2] kept points whose
// unpacked triple differs, out[3..8] min / max of (range, sector, azimuth) index over the kept points, out[9] kept points whose
// triple leaves the grid, out[10] kept points the guarded estimate left undecided (idx3_fast == false), out[11] points (kept or not)
// whose verdict by keep_of_point -- what the arrange pass asks -- differs from apri_of_point's.  Returns idx3_roundtrip_ok.
int lean_key_compare(const float* g9, const int* dims3, const float* xyz, long n, long* out) {
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
    const BinFast f = bin_fast_of(g);
    const KeepFast kf = keep_fast_of(g);
    for (int k = 0; k < 12; ++k) out[k] = 0;
    out[3] = out[5] = out[7] = 1 << 30;
    out[4] = out[6] = out[8] = -(1 << 30);
    for (long i = 0; i < n; ++i) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        Apri a;
        const int keep = apri_of_point(g, x, y, z, 0.f, a);
        if (keep_of_point(g, kf, x, y, z) != keep) ++out[11];
        if (!keep) continue;
        ++out[0];
        // the triple as the arrange pass computes it: the estimate where it decides, the reference arithmetic elsewhere
        int32_t ri, si, ai;
        if (!idx3_fast(g, f, x, y, z, &ri, &si, &ai)) {
            ri = a.range_idx;
            si = a.sector_idx;
            ai = a.azimuth_idx;
            ++out[10];
        }
        int32_t ur, us, ua;
        unpack_idx3(pack_idx3(ri, si, ai), &ur, &us, &ua);
        const int32_t key = ua * g.range_num * g.sector_num + ur * g.sector_num + us;
        if (key != a.voxel_idx) ++out[1];
        if (ur != a.range_idx || us != a.sector_idx || ua != a.azimuth_idx) ++out[2];
        const int32_t v[3] = {a.range_idx, a.sector_idx, a.azimuth_idx};
        for (int k = 0; k < 3; ++k) {
            if (v[k] < out[3 + 2 * k]) out[3 + 2 * k] = v[k];
            if (v[k] > out[4 + 2 * k]) out[4 + 2 * k] = v[k];
        }
        if ((unsigned)v[0] >= (unsigned)g.range_num || (unsigned)v[1] >= (unsigned)g.sector_num || (unsigned)v[2] >= (unsigned)g.azimuth_num) ++out[9];
    }
    return idx3_roundtrip_ok(g) ? 1 : 0;
}

}  // extern "C"
