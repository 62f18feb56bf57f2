// CPU statements the object table's helper (objects_ref.py) needs in the library's own arithmetic -- test infrastructure only.
//   obj_center      getCenterOfCloud (ssc.cpp:427-435) by the convention of DESIGN.md section 2: three sequential fp32 sums over the
//                   points in the order given, each divided by (float)n
//   obj_angle_diff  f_11(0, 8) of getDescriptorByEigenValue (ssc.cpp:731-733) with PointAPRI::angle's expression (scvod_math.h)
// Built by the tests with -ffp-contract=off, as the library is.
#include "../../dr-using-scv-od_amd/csrc/scvod_math.h"

extern "C" {

void obj_center(const float* xyz, int n, float* out3) {
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = 0; i < n; ++i) {
        sx += xyz[3 * i];
        sy += xyz[3 * i + 1];
        sz += xyz[3 * i + 2];
    }
    const float c = (float)n;
    out3[0] = sx / c;
    out3[1] = sy / c;
    out3[2] = sz / c;
}

float obj_angle_diff(float min_x, float min_y, float max_x, float max_y) {
    return scvod::fabs_f(scvod::polar_angle_deg(max_x, max_y) - scvod::polar_angle_deg(min_x, min_y));
}
}
