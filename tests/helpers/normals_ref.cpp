// CPU statement of scvod_normals_device (normals_ref.py) -- test infrastructure only.  A plain sequential loop over the queries with an
// EXHAUSTIVE neighbour loop (every cloud point, no grid) that calls the nrm_* / normal_* functions of the library's scvod_math.h; no
// part of the kernels.  Built by the tests with -ffp-contract=off, as the library is.
#include <cstdint>
#include <cstring>

#include "../../dr-using-scv-od_amd/csrc/scvod_math.h"

using namespace scvod;

extern "C" {

// cloud [n_cloud][cloud_stride], query [n_query][query_stride] or NULL (the queries are the cloud), seg [n_seg + 1] and view [n_seg][3]
// or n_seg == 0.  Outputs: normals [n_query][3], curv [n_query], count [n_query], sums [n_query][10], stats [8] as scvod_normals_stats.
void normals_ref(const float* cloud, int cloud_stride, int n_cloud, const float* query, int query_stride, int n_query, const int* seg,
                 const float* view, int n_seg, float radius, int min_neighbours, float* normals, float* curv, int* count, long long* sums,
                 long long* stats) {
    if (!query) {
        query = cloud;
        query_stride = cloud_stride;
    }
    const float r2 = radius * radius;
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    stats[0] = n_query;
    for (int m = 0; m < n_cloud; ++m) {
        const float* p = cloud + (size_t)cloud_stride * m;
        if (!nrm_usable(p[0], p[1], p[2])) ++stats[4];
    }
    int s_of = 0;
    for (int q = 0; q < n_query; ++q) {
        const float* c = query + (size_t)query_stride * q;
        long long s[kNrmWords];
        for (int i = 0; i < kNrmWords; ++i) s[i] = 0;
        float out[4];
        if (!nrm_usable(c[0], c[1], c[2])) {
            uint32_t nan = 0x7fc00000u;
            for (int i = 0; i < 4; ++i) std::memcpy(&out[i], &nan, 4);
            ++stats[3];
        } else {
            for (int m = 0; m < n_cloud; ++m) {
                const float* p = cloud + (size_t)cloud_stride * m;
                if (nrm_usable(p[0], p[1], p[2])) nrm_add(p[0], p[1], p[2], c[0], c[1], c[2], r2, s);
            }
            normal_finish(s, min_neighbours, out);
            if (n_seg > 0) {
                while (s_of + 1 < n_seg && seg[s_of + 1] <= q) ++s_of;
                normal_flip(view + 3 * s_of, c[0], c[1], c[2], out);
            }
            if (s[0] < min_neighbours) ++stats[2];
            if (out[0] == out[0] && out[1] == out[1] && out[2] == out[2]) ++stats[1];
            if (s[0] > stats[5]) stats[5] = s[0];
            stats[6] += s[0];
        }
        for (int i = 0; i < 3; ++i) normals[3 * (size_t)q + i] = out[i];
        curv[q] = out[3];
        count[q] = (int)s[0];
        for (int i = 0; i < kNrmWords; ++i) sums[(size_t)kNrmWords * q + i] = s[i];
    }
}

}  // extern "C"
