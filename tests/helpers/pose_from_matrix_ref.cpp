// Euler angles of a row-major 3x4 pose, restated for the test of scvod_pose_from_matrix (the stacker's extraction: sy from the first
// column, the regular branch unless sy < 1e-6, yaw 0 in the singular one), with float sqrt / atan2 and no contraction
// (-ffp-contract=off); and this image's atan2f itself, for the tolerance of the round-trip test.
#include <cmath>

extern "C" void ref_pose_from_matrix(const float* M, float* pose) {
    const float r00 = M[0], r10 = M[4], r20 = M[8], r21 = M[9], r22 = M[10], r11 = M[5], r12 = M[6];
    const float sq = r00 * r00 + r10 * r10;
    const float sy = sqrtf(sq);
    float roll, pitch, yaw;
    if ((double)sy < 1e-6) {
        roll = atan2f(-r12, r11);
        pitch = atan2f(-r20, sy);
        yaw = 0.0f;
    } else {
        roll = atan2f(r21, r22);
        pitch = atan2f(-r20, sy);
        yaw = atan2f(r10, r00);
    }
    pose[0] = M[3];
    pose[1] = M[7];
    pose[2] = M[11];
    pose[3] = roll;
    pose[4] = pitch;
    pose[5] = yaw;
}

extern "C" float ref_atan2f(float y, float x) { return atan2f(y, x); }
extern "C" float ref_sqrtf(float v) { return sqrtf(v); }
