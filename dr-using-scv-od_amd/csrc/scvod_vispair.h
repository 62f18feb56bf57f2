// scvod_vispair.h -- the class of one (point, viewer) pair of the range-image vote: the one statement of the rule, shared by the scan
// stage (scvod_visibility.hip) and the cloud stage (scvod_cloudvis.hip).  include/scvod.h and DESIGN.md section 2 state the convention.
#ifndef SCVOD_VISPAIR_H_
#define SCVOD_VISPAIR_H_
#include "scvod_dev.h"

namespace scvod {

static __device__ __forceinline__ bool vis_finite(float x, float y, float z) { return (x - x) == 0.0f && (y - y) == 0.0f && (z - z) == 0.0f; }

// makeApriVec's verdict, depth and pixel of a finite point: the guarded estimate where it decides (scvod_math.h::idx3_fast, the index is
// then apri_of_point's; the verdict by keep_of_point, the depth by the same sqrt), apri_of_point next to a bin edge
static __device__ __forceinline__ int vis_bin(const VisJob& J, float x, float y, float z, float* dis, int32_t* si, int32_t* ai) {
    int32_t ri;
    if (idx3_fast(J.bin, J.binfast, x, y, z, &ri, si, ai)) {
        *dis = point_distance2d(x, y);
        return keep_of_point(J.bin, J.keep, x, y, z);
    }
    Apri a;
    const int keep = apri_of_point(J.bin, x, y, z, 0.f, a);
    *dis = a.range;
    *si = a.sector_idx;
    *ai = a.azimuth_idx;
    return keep;
}

// the class of one (point, viewer) pair: 0 THROUGH, 1 AGREE, 2 OCCLUDED, 3 OUTSIDE or EMPTY
static __device__ __forceinline__ int vis_pair(const VisJob& J, const float* __restrict__ img, int A, int S, float x, float y, float z) {
    if (!vis_finite(x, y, z)) return 3;
    float dis;
    int32_t si, ai;
    if (!vis_bin(J, x, y, z, &dis, &si, &ai)) return 3;
    if (si < 0 || si >= S || ai < 0 || ai >= A) return 3;
    const float gap = J.gap_abs + J.gap_rel * dis;
    const float lim = dis + gap;
    float r_min = __builtin_inff();
    bool agree = false;
    if (J.halo == 0) {
        const float r = img[ai * S + si];
        r_min = r;
        agree = fabsf(r - dis) <= gap;
    } else {
        // clipped to the image: no wrap across the sector seam
        const int a0 = ai > 0 ? ai - 1 : 0, a1 = ai + 1 < A ? ai + 1 : A - 1;
        const int s0 = si > 0 ? si - 1 : 0, s1 = si + 1 < S ? si + 1 : S - 1;
        for (int a = a0; a <= a1; ++a)
            for (int c = s0; c <= s1; ++c) {
                const float r = img[a * S + c];
                r_min = r < r_min ? r : r_min;
                agree = agree || fabsf(r - dis) <= gap;
            }
    }
    if (r_min == __builtin_inff()) return 3;
    if (r_min > lim) return 0;
    return agree ? 1 : 2;
}

}  // namespace scvod
#endif
