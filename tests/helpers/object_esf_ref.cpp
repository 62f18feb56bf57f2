// CPU statement of scvod_esf_device for one object (object_esf_ref.py) -- test infrastructure only.  A plain sequential loop over one
// object's points and samples that calls the esf_* functions of the library's scvod_math.h; no part of the kernel.  Built by the
// tests with -ffp-contract=off, as the library is.
#include <cstring>
#include <vector>

#include "../../dr-using-scv-od_amd/csrc/scvod_math.h"

using namespace scvod;

extern "C" {

// xyz [n][3] in member order -> out = one scvod_object_esf (64 bytes), hist = the 640 integer counters, sig = the 640 normalised
// values, extra = {triangles OUT, IN, MIX}
void esf_ref(const float* xyz, int n, int samples, unsigned seed, int min_points, void* out, int* hist, float* sig, int* extra) {
    ObjEsf r;
    std::memset(&r, 0, sizeof(r));
    r.n_points = n;
    for (int i = 0; i < kEsfSig; ++i) hist[i] = 0, sig[i] = 0.f;
    extra[0] = extra[1] = extra[2] = 0;
    const auto done = [&](int flags) {
        r.flags = flags;
        std::memcpy(out, &r, sizeof(r));
    };
    if (n < min_points) return done(kEsfFlagFewPoints);
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = 0; i < n; ++i) {
        sx += xyz[3 * i];
        sy += xyz[3 * i + 1];
        sz += xyz[3 * i + 2];
    }
    const float cnt = (float)n;
    const float cx = sx / cnt, cy = sy / cnt, cz = sz / cnt;
    float r2 = 0.f;
    for (int i = 0; i < n; ++i) {
        const float d2 = esf_dist2(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, cz);
        if (d2 > r2) r2 = d2;
    }
    const float rad = sqrt_f(r2);
    if (rad == 0.f || (f2u(rad) & 0x7f800000u) == 0x7f800000u) return done(kEsfFlagExtent);
    const float scale = 32.0f / rad;
    std::vector<float> u((size_t)n * 3);
    std::vector<uint32_t> grid(kEsfGrid * kEsfGrid * kEsfGrid / 32, 0u);
    for (int i = 0; i < n; ++i) {
        u[3 * i] = (xyz[3 * i] - cx) * scale;
        u[3 * i + 1] = (xyz[3 * i + 1] - cy) * scale;
        u[3 * i + 2] = (xyz[3 * i + 2] - cz) * scale;
        const int v[3] = {esf_voxel(u[3 * i]), esf_voxel(u[3 * i + 1]), esf_voxel(u[3 * i + 2])};
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int x = v[0] + dx, y = v[1] + dy, z = v[2] + dz;
                    if (x < 0 || y < 0 || z < 0 || x >= kEsfGrid || y >= kEsfGrid || z >= kEsfGrid) continue;
                    const int b = (z * kEsfGrid + y) * kEsfGrid + x;
                    grid[b >> 5] |= 1u << (b & 31);
                }
    }
    const float T[64] = SCVOD_ESF_COS_TABLE;
    const auto pt = [&](int i, float p[3]) { p[0] = u[3 * i], p[1] = u[3 * i + 1], p[2] = u[3 * i + 2]; };
    // sweep 1: everything but the D2 / D3 bins, and the maxima
    std::vector<unsigned char> code((size_t)samples, 255);
    float max_d2 = 0.f, max_d3 = 0.f;
    for (int k = 0; k < samples; ++k) {
        float q[3][3];
        const EsfSample s = esf_sample(seed, (uint32_t)k, n, pt, q);
        if (!s.valid) continue;
        const EsfLines L = esf_trace(grid.data(), q);
        int bins[3];
        esf_corner_bins(T, q, s, bins);
        for (int a = 0; a < 3; ++a) {
            ++hist[esf_row_a3(L.tri) * kEsfBins + bins[a]];
            if (L.ratio_bin[a] >= 0) ++hist[kEsfRowRatio * kEsfBins + L.ratio_bin[a]];
            ++r.lines[L.cls[a]];
        }
        ++extra[L.tri == kEsfOut ? 0 : (L.tri == kEsfIn ? 1 : 2)];
        if (s.a > max_d2) max_d2 = s.a;
        if (s.b > max_d2) max_d2 = s.b;
        if (s.c > max_d2) max_d2 = s.c;
        const float d3 = sqrt_f(sqrt_f(s.heron));
        if (d3 > max_d3) max_d3 = d3;
        ++r.n_valid;
        code[k] = (unsigned char)(L.cls[0] + 3 * L.cls[1] + 9 * L.cls[2] + 27 * L.tri);
    }
    // sweep 2
    for (int k = 0; k < samples; ++k) {
        if (code[k] == 255) continue;
        float q[3][3];
        const EsfSample s = esf_sample(seed, (uint32_t)k, n, pt, q);
        const int c = code[k];
        ++hist[esf_row_d3(c / 27) * kEsfBins + esf_bin_of(sqrt_f(sqrt_f(s.heron)), max_d3)];
        ++hist[esf_row_d2(c % 3) * kEsfBins + esf_bin_of(s.a, max_d2)];
        ++hist[esf_row_d2((c / 3) % 3) * kEsfBins + esf_bin_of(s.b, max_d2)];
        ++hist[esf_row_d2((c / 9) % 3) * kEsfBins + esf_bin_of(s.c, max_d2)];
    }
    float total = 0.f;
    for (int i = 0; i < kEsfSig; ++i) total += esf_sig_value(i, hist[i]);
    if (total == 0.f) return done(kEsfFlagNoSample);
    for (int i = 0; i < kEsfSig; ++i) sig[i] = esf_sig_value(i, hist[i]) / total;
    for (int j = 0; j < 10; ++j) r.fold10[j] = esf_fold(sig, j);
    done(0);
}

void esf_cos_table(float* out64) {
    const float T[64] = SCVOD_ESF_COS_TABLE;
    for (int i = 0; i < 64; ++i) out64[i] = T[i];
}
}
