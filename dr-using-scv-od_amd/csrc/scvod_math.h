// scvod_math.h -- arithmetic spec of the SCV-OD hot path, shared by the HIP kernels and
// the host side of libscvod (compiled by hipcc for gfx950 and by g++ for the CPU unit
// tests of the spec itself).
//
// Everything that decides an INTEGER (bin index, patch id, ground/non-ground class) is
// written here with explicit IEEE-754 operations only: no libm / ocml transcendental is
// called, FMA contraction is disabled for the whole library (-ffp-contract=off), and
// fp32/fp64 division and sqrt are the correctly rounded HIP defaults.  The reference
// calls glibc here:
//   * atan2f  (include/utility.h:382,385,391 -- float overload)
//   * atan2   (include/patchwork.h:419,421 -- double)
// glibc 2.27-2.40 implement atan2f/atanf with the Sun fdlibm algorithm in pure fp32
// arithmetic, which is restated below operation by operation, so it is bit-identical to
// glibc on the CPU (tests/test_math_spec.py checks that against the libm of this image)
// and, because it only uses IEEE add/mul/div, bit-identical on the GPU.
// For the double atan2 the fdlibm double algorithm is used (error < 1 ulp); it feeds
// only `int(theta / sector_size)` in pc2czm, where a last-bit difference to glibc can
// matter only within 1 ulp of a sector boundary (counted by the same test: 0 flips).
#ifndef SCVOD_MATH_H_
#define SCVOD_MATH_H_

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SCVOD_HD __host__ __device__ __forceinline__
#else
#define SCVOD_HD inline
#endif

namespace scvod {

SCVOD_HD uint32_t f2u(float f) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(f);
#else
    memcpy(&u, &f, 4);
#endif
    return u;
}
SCVOD_HD float u2f(uint32_t u) {
    float f;
#if defined(__HIP_DEVICE_COMPILE__)
    f = __uint_as_float(u);
#else
    memcpy(&f, &u, 4);
#endif
    return f;
}
SCVOD_HD uint64_t d2u(double d) {
    uint64_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = (uint64_t)__double_as_longlong(d);
#else
    memcpy(&u, &d, 8);
#endif
    return u;
}
SCVOD_HD double u2d(uint64_t u) {
    double d;
#if defined(__HIP_DEVICE_COMPILE__)
    d = __longlong_as_double((long long)u);
#else
    memcpy(&d, &u, 8);
#endif
    return d;
}

SCVOD_HD float fabs_f(float x) { return u2f(f2u(x) & 0x7fffffffu); }
SCVOD_HD double fabs_d(double x) { return u2d(d2u(x) & 0x7fffffffffffffffull); }

// correctly rounded sqrt (IEEE): sqrtf / sqrt map to v_sqrt + fixup on gfx950 under the
// default -fhip-fp32-correctly-rounded-divide-sqrt; on the host they are SSE sqrtss/sd.
SCVOD_HD float sqrt_f(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_sqrtf(x);  // llvm.sqrt.f32, correctly rounded (HIP's __fsqrt_rn is the 1-ulp native sqrt)
#else
    return __builtin_sqrtf(x);
#endif
}
SCVOD_HD double sqrt_d(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_sqrt(x);
#else
    return __builtin_sqrt(x);
#endif
}
SCVOD_HD float floor_f(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ::floorf(x);
#else
    return __builtin_floorf(x);
#endif
}
SCVOD_HD float ceil_f(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ::ceilf(x);
#else
    return __builtin_ceilf(x);
#endif
}

// ---- fdlibm atanf / atan2f in fp32 (glibc sysdeps/ieee754/flt-32/{s_atanf,e_atan2f}.c
// algorithm: argument reduction to [0, 7/16] around 0.5, 1, 1.5, inf and an 11-term odd
// polynomial split into even/odd halves) ------------------------------------------------
SCVOD_HD float atan_f32(float x) {
    const float atanhi[4] = {u2f(0x3eed6338u), u2f(0x3f490fdau), u2f(0x3f7b985eu), u2f(0x3fc90fdau)};
    const float atanlo[4] = {u2f(0x31ac3769u), u2f(0x33222168u), u2f(0x33140fb4u), u2f(0x33a22168u)};
    const float aT0 = u2f(0x3eaaaaabu), aT1 = u2f(0xbe4ccccdu), aT2 = u2f(0x3e124925u),
                aT3 = u2f(0xbde38e38u), aT4 = u2f(0x3dba2e6eu), aT5 = u2f(0xbd9d8795u),
                aT6 = u2f(0x3d886b35u), aT7 = u2f(0xbd6ef16bu), aT8 = u2f(0x3d4bda59u),
                aT9 = u2f(0xbd15a221u), aT10 = u2f(0x3c8569d7u);
    const float one = 1.0f;
    uint32_t hx = f2u(x);
    uint32_t ix = hx & 0x7fffffffu;
    int id;
    if (ix >= 0x4c000000u) { /* |x| >= 2^25 */
        if (ix > 0x7f800000u) return x + x; /* NaN */
        if ((int32_t)hx > 0) return atanhi[3] + atanlo[3];
        return -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3ee00000u) { /* |x| < 0.4375 */
        if (ix < 0x31000000u) return x; /* |x| < 2^-29 */
        id = -1;
    } else {
        x = fabs_f(x);
        if (ix < 0x3f980000u) {     /* |x| < 1.1875 */
            if (ix < 0x3f300000u) { /* 7/16 <= |x| < 11/16 */
                id = 0;
                x = (2.0f * x - one) / (2.0f + x);
            } else { /* 11/16 <= |x| < 19/16 */
                id = 1;
                x = (x - one) / (x + one);
            }
        } else {
            if (ix < 0x401c0000u) { /* |x| < 2.4375 */
                id = 2;
                x = (x - 1.5f) / (one + 1.5f * x);
            } else { /* 2.4375 <= |x| < 2^25 */
                id = 3;
                x = -1.0f / x;
            }
        }
    }
    float z = x * x;
    float w = z * z;
    float s1 = z * (aT0 + w * (aT2 + w * (aT4 + w * (aT6 + w * (aT8 + w * aT10)))));
    float s2 = w * (aT1 + w * (aT3 + w * (aT5 + w * (aT7 + w * aT9))));
    if (id < 0) return x - x * (s1 + s2);
    z = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return ((int32_t)hx < 0) ? -z : z;
}

SCVOD_HD float atan2_f32(float y, float x) {
    const float tiny = 1.0e-30f;
    const float pi_o_4 = u2f(0x3f490fdbu), pi_o_2 = u2f(0x3fc90fdbu), pi = u2f(0x40490fdbu),
                pi_lo = u2f(0xb3bbbd2eu);
    uint32_t hx = f2u(x), hy = f2u(y);
    uint32_t ix = hx & 0x7fffffffu, iy = hy & 0x7fffffffu;
    if (ix > 0x7f800000u || iy > 0x7f800000u) return x + y; /* NaN */
    if (hx == 0x3f800000u) return atan_f32(y);              /* x = 1.0 */
    int m = (int)((hy >> 31) & 1u) | (int)((hx >> 30) & 2u); /* 2*sign(x)+sign(y) */
    if (iy == 0) {
        switch (m) {
            case 0:
            case 1: return y;
            case 2: return pi + tiny;
            default: return -pi - tiny;
        }
    }
    if (ix == 0) return ((int32_t)hy < 0) ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7f800000u) {
        if (iy == 0x7f800000u) {
            switch (m) {
                case 0: return pi_o_4 + tiny;
                case 1: return -pi_o_4 - tiny;
                case 2: return 3.0f * pi_o_4 + tiny;
                default: return -3.0f * pi_o_4 - tiny;
            }
        } else {
            switch (m) {
                case 0: return 0.0f;
                case 1: return -0.0f;
                case 2: return pi + tiny;
                default: return -pi - tiny;
            }
        }
    }
    if (iy == 0x7f800000u) return ((int32_t)hy < 0) ? -pi_o_2 - tiny : pi_o_2 + tiny;
    int32_t k = ((int32_t)iy - (int32_t)ix) >> 23;
    float z;
    if (k > 60)
        z = pi_o_2 + 0.5f * pi_lo;
    else if ((int32_t)hx < 0 && k < -60)
        z = 0.0f;
    else
        z = atan_f32(fabs_f(y / x));
    switch (m) {
        case 0: return z;
        case 1: return u2f(f2u(z) ^ 0x80000000u);
        case 2: return pi - (z - pi_lo);
        default: return (z - pi_lo) - pi;
    }
}

// ---- fdlibm atan / atan2 in fp64 (Sun s_atan.c / e_atan2.c algorithm) ------------------
SCVOD_HD double atan_f64(double x) {
    const double atanhi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01,
                              9.82793723247329054082e-01, 1.57079632679489655800e+00};
    const double atanlo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17,
                              1.39033110312309984516e-17, 6.12323399573676603587e-17};
    const double aT0 = 3.33333333333329318027e-01, aT1 = -1.99999999998764832476e-01,
                 aT2 = 1.42857142725034663711e-01, aT3 = -1.11111104054623557880e-01,
                 aT4 = 9.09088713343650656196e-02, aT5 = -7.69187620504482999495e-02,
                 aT6 = 6.66107313738753120669e-02, aT7 = -5.83357013379057348645e-02,
                 aT8 = 4.97687799461593236017e-02, aT9 = -3.65315727442169155270e-02,
                 aT10 = 1.62858201153657823623e-02;
    uint64_t bx = d2u(x);
    int32_t hx = (int32_t)(bx >> 32);
    int32_t ix = hx & 0x7fffffff;
    int id;
    if (ix >= 0x44100000) { /* |x| >= 2^66 */
        uint32_t lx = (uint32_t)bx;
        if (ix > 0x7ff00000 || (ix == 0x7ff00000 && lx != 0)) return x + x;
        if (hx > 0) return atanhi[3] + atanlo[3];
        return -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3fdc0000) {               /* |x| < 0.4375 */
        if (ix < 0x3e200000) return x;   /* |x| < 2^-29 */
        id = -1;
    } else {
        x = fabs_d(x);
        if (ix < 0x3ff30000) {     /* |x| < 1.1875 */
            if (ix < 0x3fe60000) { /* 7/16 <= |x| < 11/16 */
                id = 0;
                x = (2.0 * x - 1.0) / (2.0 + x);
            } else {
                id = 1;
                x = (x - 1.0) / (x + 1.0);
            }
        } else {
            if (ix < 0x40038000) { /* |x| < 2.4375 */
                id = 2;
                x = (x - 1.5) / (1.0 + 1.5 * x);
            } else {
                id = 3;
                x = -1.0 / x;
            }
        }
    }
    double z = x * x;
    double w = z * z;
    double s1 = z * (aT0 + w * (aT2 + w * (aT4 + w * (aT6 + w * (aT8 + w * aT10)))));
    double s2 = w * (aT1 + w * (aT3 + w * (aT5 + w * (aT7 + w * aT9))));
    if (id < 0) return x - x * (s1 + s2);
    z = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return (hx < 0) ? -z : z;
}

SCVOD_HD double atan2_f64(double y, double x) {
    const double tiny = 1.0e-300;
    const double pi_o_4 = 7.8539816339744827900E-01, pi_o_2 = 1.5707963267948965580E+00,
                 pi = 3.1415926535897931160E+00, pi_lo = 1.2246467991473531772E-16;
    uint64_t bx = d2u(x), by = d2u(y);
    int32_t hx = (int32_t)(bx >> 32), hy = (int32_t)(by >> 32);
    uint32_t lx = (uint32_t)bx, ly = (uint32_t)by;
    int32_t ix = hx & 0x7fffffff, iy = hy & 0x7fffffff;
    if (((uint32_t)ix | ((lx | (0u - lx)) >> 31)) > 0x7ff00000u ||
        ((uint32_t)iy | ((ly | (0u - ly)) >> 31)) > 0x7ff00000u)
        return x + y; /* NaN */
    if (((uint32_t)(hx - 0x3ff00000) | lx) == 0) return atan_f64(y); /* x = 1.0 */
    int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);
    if (((uint32_t)iy | ly) == 0) {
        switch (m) {
            case 0:
            case 1: return y;
            case 2: return pi + tiny;
            default: return -pi - tiny;
        }
    }
    if (((uint32_t)ix | lx) == 0) return (hy < 0) ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7ff00000) {
        if (iy == 0x7ff00000) {
            switch (m) {
                case 0: return pi_o_4 + tiny;
                case 1: return -pi_o_4 - tiny;
                case 2: return 3.0 * pi_o_4 + tiny;
                default: return -3.0 * pi_o_4 - tiny;
            }
        } else {
            switch (m) {
                case 0: return 0.0;
                case 1: return -0.0;
                case 2: return pi + tiny;
                default: return -pi - tiny;
            }
        }
    }
    if (iy == 0x7ff00000) return (hy < 0) ? -pi_o_2 - tiny : pi_o_2 + tiny;
    int32_t k = (iy - ix) >> 20;
    double z;
    if (k > 60)
        z = pi_o_2 + 0.5 * pi_lo;
    else if (hx < 0 && k < -60)
        z = 0.0;
    else
        z = atan_f64(fabs_d(y / x));
    switch (m) {
        case 0: return z;
        case 1: return -z;
        case 2: return pi - (z - pi_lo);
        default: return (z - pi_lo) - pi;
    }
}

// ---- curved-voxel binning: SSC::makeApriVec (src/ssc.cpp:155-195) with
// Utility::pointDistance2d / getPolarAngle / getAzimuth / rad2deg
// (include/utility.h:346-349, 371-392) ------------------------------------------------------
struct BinParams {
    float min_dis, max_dis, min_angle, max_angle, min_azimuth, max_azimuth;
    float range_res, sector_res, azimuth_res;
    int32_t range_num, sector_num, azimuth_num, bin_num;
};

#define SCVOD_M_PI 3.14159265358979323846

// rad2deg: `(float)radians * 180.0 / M_PI` evaluated in double, returned as float
// (utility.h:346-349)
SCVOD_HD float rad2deg_f(float radians) { return (float)((double)radians * 180.0 / SCVOD_M_PI); }

SCVOD_HD float point_distance2d(float x, float y) {
    // (float)sqrt(x*x + y*y): fp32 products and sum (no FMA), correctly rounded sqrt
    float s = x * x + y * y;
    return sqrt_f(s);
}

SCVOD_HD float polar_angle_deg(float x, float y) {
    if (x == 0.0f && y == 0.0f) return 0.0f;
    if (y >= 0.0f) return rad2deg_f(atan2_f32(y, x));
    // (float)rad2deg((float)atan2(y,x) + 2*M_PI): the sum is a double, rad2deg casts it to
    // float first (utility.h:348,385)
    double s = (double)atan2_f32(y, x) + 2.0 * SCVOD_M_PI;
    return rad2deg_f((float)s);
}

SCVOD_HD float azimuth_deg(float z, float dis) { return rad2deg_f(atan2_f32(z, dis)); }

struct Apri {
    float x, y, z, range, angle, azimuth, intensity;
    int32_t range_idx, sector_idx, azimuth_idx, voxel_idx;
};

// returns 1 when the point passes the range / FOV test of ssc.cpp:161-172
SCVOD_HD int apri_of_point(const BinParams& g, float x, float y, float z, float intensity,
                           Apri& a) {
    float dis = point_distance2d(x, y);
    float angle = polar_angle_deg(x, y);
    float azimuth = azimuth_deg(z, dis);
    int keep = 1;
    if (dis < g.min_dis || dis > g.max_dis) keep = 0;
    if (angle < g.min_angle || angle > g.max_angle) keep = 0;
    if (azimuth < g.min_azimuth || azimuth > g.max_azimuth) keep = 0;
    a.x = x;
    a.y = y;
    a.z = z;
    a.range = dis;
    a.angle = angle;
    a.azimuth = azimuth;
    a.intensity = intensity;
    // std::ceil(float) - 1 -> float -> int (ssc.cpp:185-187)
    a.range_idx = (int32_t)(ceil_f((dis - g.min_dis) / g.range_res) - 1.0f);
    a.sector_idx = (int32_t)(ceil_f((angle - g.min_angle) / g.sector_res) - 1.0f);
    a.azimuth_idx = (int32_t)(ceil_f((azimuth - g.min_azimuth) / g.azimuth_res) - 1.0f);
    a.voxel_idx = a.azimuth_idx * g.range_num * g.sector_num + a.range_idx * g.sector_num + a.sector_idx;
    return keep;
}

// ---- voxel index of a point WITHOUT the reference's arithmetic where that provably cannot matter (SSC::tracking re-bins
// every transformed point, ssc.cpp:1280-1286; only the index is used).  The two angles are estimated with a polynomial
// arctangent (Abramowitz & Stegun 4.4.49, |error| <= 2e-8 rad) in fp32: the estimate and the reference's
// float(double(atan2f(..)) * 180 / pi) both lie within 2.5e-4 degrees of each other (measured over 10^9 points,
// tests/test_math_spec.py: < 6e-5), so when the estimate is farther than 1.5e-3 degrees (plus the rounding of the scaled
// value) from every bin edge the index is the reference's; otherwise -- a few points per thousand -- the caller evaluates
// apri_of_point.  y == +-0 (angle exactly 0 / 180 / -180: sector -1 and the signed-zero cases of atan2f) and the origin
// always take the reference arithmetic.  The range index is the reference's own computation (one sqrt, one division).
struct BinFast {
    float inv_sector_res, inv_azimuth_res;
    float m_sector, m_azimuth;  // distance to a bin edge, in bins, below which the estimate decides nothing
};
inline BinFast bin_fast_of(const BinParams& g) {
    BinFast f;
    f.inv_sector_res = 1.0f / g.sector_res;
    f.inv_azimuth_res = 1.0f / g.azimuth_res;
    f.m_sector = 1.5e-3f * f.inv_sector_res + 2.0e-4f;
    f.m_azimuth = 1.5e-3f * f.inv_azimuth_res + 2.0e-4f;
    return f;
}
SCVOD_HD float atan01_poly(float t) {  // t in [0, 1]
    const float s = t * t;
    float q = 0.0028662257f;
    q = q * s + -0.0161657367f;
    q = q * s + 0.0429096138f;
    q = q * s + -0.0752896400f;
    q = q * s + 0.1065626393f;
    q = q * s + -0.1420889944f;
    q = q * s + 0.1999355085f;
    q = q * s + -0.3333314528f;
    q = q * s + 1.0f;
    return t * q;
}
SCVOD_HD float rcp_fast(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}
// atan2(|y|, x) in [0, pi] for |y| > 0, within 6.1e-7 rad of the exact value: atan01_poly is within 1.05e-7 rad of atan over ALL
// 2^30 floats of [0, 1] (checked exhaustively on the CPU, the same unfused arithmetic), the quotient within 1.8e-7 of mn / mx
// (v_rcp_f32: 1 ulp, + the product's rounding), the two folds add 1.1e-7 and 2.1e-7 (constants + roundings).  NaN in, NaN out.
SCVOD_HD float atan2_abs_rad_fast(float ay, float x) {
    const float ax = fabs_f(x);
    const float mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
    float a = atan01_poly(mn * rcp_fast(mx));
    if (ay > ax) a = 1.57079632679f - a;
    if (x < 0.0f) a = 3.14159265359f - a;
    return a;
}
// degrees in [0, 180] of atan2(|y|, x) for |y| > 0
SCVOD_HD float atan2_abs_deg_fast(float ay, float x) { return atan2_abs_rad_fast(ay, x) * 57.2957795131f; }
// true: (*ri, *si, *ai) are the reference's range / sector / azimuth indices of the point; false: undecided (use apri_of_point)
SCVOD_HD bool idx3_fast(const BinParams& g, const BinFast& f, float x, float y, float z, int32_t* ri_out, int32_t* si_out, int32_t* ai_out) {
    const float ay = fabs_f(y);
    if (!(ay > 0.0f)) return false;  // y == +-0 (and NaN)
    const float dis = point_distance2d(x, y);
    float ang = atan2_abs_deg_fast(ay, x);
    if (y < 0.0f) ang = 360.0f - ang;
    const float us = (ang - g.min_angle) * f.inv_sector_res;
    const float fs = floor_f(us);
    const float ds = us - fs;
    if (!(ds > f.m_sector && ds < 1.0f - f.m_sector)) return false;
    const float az = (z == 0.0f) ? 0.0f : atan2_abs_deg_fast(fabs_f(z), dis);
    const float azs = z < 0.0f ? -az : az;
    const float ua = (azs - g.min_azimuth) * f.inv_azimuth_res;
    const float fa = floor_f(ua);
    const float da = ua - fa;
    if (!(da > f.m_azimuth && da < 1.0f - f.m_azimuth)) return false;
    if (!(fabs_f(us) < 1.0e6f && fabs_f(ua) < 1.0e6f)) return false;
    *ri_out = (int32_t)(ceil_f((dis - g.min_dis) / g.range_res) - 1.0f);
    *si_out = (int32_t)fs;
    *ai_out = (int32_t)fa;
    return true;
}
// true: *voxel_idx is SSC::tracking's index of the point; false: undecided (use apri_of_point)
SCVOD_HD bool voxel_idx_fast(const BinParams& g, const BinFast& f, float x, float y, float z, int32_t* voxel_idx) {
    int32_t ri, si, ai;
    if (!idx3_fast(g, f, x, y, z, &ri, &si, &ai)) return false;
    *voxel_idx = ai * g.range_num * g.sector_num + ri * g.sector_num + si;
    return true;
}

// ---- index triple of an apri point, packed by the arrange kernels (lean emission) / k_emit / k_bin_direct / k_apri_split:
// 11 + 11 + 10 bits, each index clamped to [-2, limit] and biased by 2 (indices at or beyond -2 / dim + 1 have no in-grid
// neighbour at all, so clamping them keeps both the run comparison and the neighbourhood exact).
// A point that passed the range / FOV test has its indices in [-1, dim] (the quotient at the upper limit may round one bin up),
// so unpacking returns them -- and with them voxel_idx -- exactly as long as dim <= kIdx3Max*: the lean emission's condition
// (idx3_roundtrip_ok; tests/test_gpu_lean_emission.py checks the bound against apri_of_point on the CPU).
constexpr int32_t kIdx3MaxRS = 2045, kIdx3MaxA = 1021;
SCVOD_HD int32_t pack_idx3(int32_t r, int32_t s, int32_t a) {
    r = (r < -2 ? -2 : (r > kIdx3MaxRS ? kIdx3MaxRS : r)) + 2;
    s = (s < -2 ? -2 : (s > kIdx3MaxRS ? kIdx3MaxRS : s)) + 2;
    a = (a < -2 ? -2 : (a > kIdx3MaxA ? kIdx3MaxA : a)) + 2;
    return r | (s << 11) | (int32_t)((uint32_t)a << 22);
}
SCVOD_HD void unpack_idx3(int32_t t, int32_t* r, int32_t* s, int32_t* a) {
    *r = (t & 2047) - 2;
    *s = ((t >> 11) & 2047) - 2;
    *a = ((t >> 22) & 1023) - 2;
}
inline bool idx3_roundtrip_ok(const BinParams& g) {  // every index in [-1, dim] survives the clamp
    return g.range_num < kIdx3MaxRS && g.sector_num < kIdx3MaxRS && g.azimuth_num < kIdx3MaxA;
}

// ---- range / FOV verdict of makeApriVec WITHOUT the two atan2f of apri_of_point, for callers that only need the
// verdict (k_pw_arrange).  Same result by construction:
//   * range: the same fp32 sqrt and comparisons.
//   * angle: with min_angle <= 0 and max_angle >= 360 the test cannot fail -- polar_angle_deg returns at most
//     fl32(fl32(2 pi) * 180 / pi) = 360.0f (360.00001 rounds down, the float spacing there is 3e-5) and never a
//     negative value; NaN compares false in both forms.
//   * azimuth: atan2f(z, dis) and the conversion to degrees are within 1.2e-5 deg of atan(z / dis) * 180 / pi, so when
//     t = z / dis is farther than 2e-6 * (1 + t^2) (six times that error, in units of t) from tan(min_azimuth) and
//     tan(max_azimuth) the decision is known; only points inside that sliver evaluate apri_of_point.
//   * y == +-0 takes the reference arithmetic: atan2f(-0, x < 0) is -pi, the one direction whose polar angle IS negative
//     (-180 degrees: the reference drops the point).
struct KeepFast {
    int32_t ok;      // the shortcut is valid for this parameter set
    float tan_lo, tan_hi;
};
inline KeepFast keep_fast_of(const BinParams& g) {
    KeepFast k;
    k.ok = (g.min_angle <= 0.0f && g.max_angle >= 360.0f && g.min_azimuth > -89.0f && g.max_azimuth < 89.0f &&
            g.min_azimuth < g.max_azimuth)
               ? 1
               : 0;
    k.tan_lo = (float)__builtin_tan((double)g.min_azimuth * SCVOD_M_PI / 180.0);
    k.tan_hi = (float)__builtin_tan((double)g.max_azimuth * SCVOD_M_PI / 180.0);
    return k;
}
SCVOD_HD int keep_of_point(const BinParams& g, const KeepFast& k, float x, float y, float z) {
    if (k.ok && y != 0.0f) {
        const float dis = point_distance2d(x, y);
        if (dis < g.min_dis || dis > g.max_dis) return 0;
        const float t = z / dis;  // dis == 0: inf / NaN, which fails every comparison below -> reference arithmetic
        const float m = 2.0e-6f * (1.0f + t * t);
        if (t > k.tan_lo + m && t < k.tan_hi - m) return 1;
        if (t < k.tan_lo - m || t > k.tan_hi + m) return 0;
    }
    Apri a;
    return apri_of_point(g, x, y, z, 0.f, a);
}

// ---- Patchwork concentric zone model: pc2czm / xy2theta / xy2radius
// (include/patchwork.h:416-459) ------------------------------------------------------------
struct CzmParams {
    double min_range, max_range;
    double zone_min[4];     // min_ranges (patchwork.h:87)
    double ring_size[4];    // patchwork.h:88-91
    double sector_size[4];  // patchwork.h:92-94
    int32_t num_rings[4], num_sectors[4];
    int32_t patch_base[4];  // first patch id of each zone in (zone, ring, sector) order
    int32_t num_patches;
    double z_cut;           // -1.8 * sensor_height (patchwork.h:304)
    double seed_margin_z;   // adaptive_seed_selection_margin * sensor_height (patchwork.h:247)
    double th_seeds, th_dist, uprightness_thr;
    double elevation_thr[4], flatness_thr[4];
    int32_t num_iter, num_lpr, num_min_pts, num_rings_of_interest;
    // derived constants of the cheap (fp32 / reciprocal) evaluation, czm_finalize(); they only decide WHEN the cheap
    // value is trusted, never what the result is
    int32_t fast_ok;           // ranges small enough for the fp32 error bound below
    float r_margin;            // |r_fp32 - r_fp64| stays far below this (1.2e-7 * r for r <= 1000 m)
    float min_range_f, max_range_f, zone_min_f[4], inv_ring_f[4], ring_margin_f[4];
    double inv_sector[4], sector_margin[4];
    double sector_margin_est[4];  // the same for the branch-free estimate of the angle (atan2_abs_rad_fast)
};

inline void czm_finalize(CzmParams& c) {
    c.fast_ok = (c.max_range <= 1000.0 && c.min_range >= 0.0) ? 1 : 0;
    c.r_margin = 1.0e-3f;
    c.min_range_f = (float)c.min_range;
    c.max_range_f = (float)c.max_range;
    for (int k = 0; k < 4; ++k) {
        c.zone_min_f[k] = (float)c.zone_min[k];
        c.inv_ring_f[k] = (float)(1.0 / c.ring_size[k]);
        c.ring_margin_f[k] = (float)(2.0e-3 / c.ring_size[k] + 1.0e-4);
        if (!(c.ring_size[k] > 1.0e-2) || c.num_rings[k] > 256) c.fast_ok = 0;  // keeps (r - zone_min) / ring_size <= 256
        c.inv_sector[k] = 1.0 / c.sector_size[k];
        c.sector_margin[k] = 1.0e-6 / c.sector_size[k] + 1.0e-9;
        c.sector_margin_est[k] = 4.0e-6 / c.sector_size[k] + 1.0e-9;  // 6.5 x the estimate's error bound (6.1e-7 rad)
    }
}

// patch id in (zone, ring, sector) emission order, or -1 when the point is not binned
SCVOD_HD int32_t czm_patch_of(const CzmParams& c, float xf, float yf, float zf) {
    if ((double)zf < c.z_cut) return -1;  // erased prefix of the z-sorted cloud (patchwork.h:302-310)
    double x = (double)xf, y = (double)yf;
    // Zone and ring from the fp32 radius when it is farther than r_margin from every boundary that matters (its error
    // against the reference's double sqrt is below 1.3e-7 * r): same decisions, no fp64 sqrt / division.  Points next
    // to a boundary, NaNs and exotic parameter sets take the reference arithmetic below.
    int k = -1;
    int32_t ring = 0;
    if (c.fast_ok) {
        const float rf = sqrt_f(xf * xf + yf * yf);
        const float m = c.r_margin;
        if (fabs_f(rf - c.max_range_f) > m && fabs_f(rf - c.min_range_f) > m && fabs_f(rf - c.zone_min_f[1]) > m &&
            fabs_f(rf - c.zone_min_f[2]) > m && fabs_f(rf - c.zone_min_f[3]) > m) {
            if (!((rf <= c.max_range_f) && (rf > c.min_range_f))) return -1;
            const int kf = (rf < c.zone_min_f[1]) ? 0 : (rf < c.zone_min_f[2]) ? 1 : (rf < c.zone_min_f[3]) ? 2 : 3;
            const float v = (rf - c.zone_min_f[kf]) * c.inv_ring_f[kf];
            const int32_t rv = (int32_t)v;
            const float fr = v - (float)rv;
            if (fr > c.ring_margin_f[kf] && fr < 1.0f - c.ring_margin_f[kf]) {
                k = kf;
                ring = rv;
            }
        }
    }
    if (k < 0) {
        double r = sqrt_d(x * x + y * y);  // pow(x,2) == x*x exactly for float-valued doubles
        if (!((r <= c.max_range) && (r > c.min_range))) return -1;
        if (r < c.zone_min[1])
            k = 0;
        else if (r < c.zone_min[2])
            k = 1;
        else if (r < c.zone_min[3])
            k = 2;
        else
            k = 3;
        ring = (int32_t)((r - c.zone_min[k]) / c.ring_size[k]);
    }
    if (ring > c.num_rings[k] - 1) ring = c.num_rings[k] - 1;
    // sector = int(theta / sector_size) with theta = atan2(y, x) in double (+2 pi for y < 0).  The fp32 fdlibm
    // atan2 of the same (float-valued) arguments is within 3e-7 rad of it, so whenever theta_f / sector_size is
    // farther than that from an integer the cheap value decides the SAME index; only the rare points next to a
    // sector boundary (and the exact axis directions) take the fp64 evaluation.
    int32_t sector = 0;
    bool have_sector = false;
    // first a branch-free estimate (one reciprocal, a degree-17 polynomial: k_pw_classify is bound by VALU issue, and the fdlibm
    // evaluation below is five argument ranges with a division each, executed one after the other by a wave whose lanes differ):
    // it decides the sector whenever theta / sector_size is farther than 6.5 x its error bound from an integer
    if (c.fast_ok && fabs_f(yf) > 0.0f) {  // (y == +-0: the signed-zero cases of atan2 take the reference arithmetic)
        const float a = atan2_abs_rad_fast(fabs_f(yf), xf);
        const double te = (yf < 0.0f) ? 2.0 * SCVOD_M_PI - (double)a : (double)a;
        const double u = te * c.inv_sector[k];
        const int32_t su = (int32_t)u;
        const double fr = u - (double)su;
        const double margin = c.sector_margin_est[k];
        if (fr > margin && fr < 1.0 - margin) {  // (false for NaN)
            sector = su;
            have_sector = true;
        }
    }
    if (!have_sector) {
        double tf = (double)atan2_f32(yf, xf);
        if (y < 0.0) tf += 2.0 * SCVOD_M_PI;
        const double u = tf * c.inv_sector[k];  // within 1e-15 of tf / sector_size: far inside the margin
        const int32_t su = (int32_t)u;
        const double fr = u - (double)su;
        const double margin = c.sector_margin[k];
        if (fr > margin && fr < 1.0 - margin) {
            sector = su;
        } else {
            const double theta = (y >= 0.0) ? atan2_f64(y, x) : 2.0 * SCVOD_M_PI + atan2_f64(y, x);
            sector = (int32_t)(theta / c.sector_size[k]);
        }
    }
    if (sector > c.num_sectors[k] - 1) sector = c.num_sectors[k] - 1;
    if (sector < 0) sector = 0;  // y == -0.0f with x < 0 gives theta = -pi: out-of-bounds indexing in the reference
    return c.patch_base[k] + ring * c.num_sectors[k] + sector;
}

// monotone map float -> uint32 (ascending float order == ascending unsigned order;
// -0.0 sorts before +0.0, which std::sort's `a.z < b.z` treats as equal: ties)
SCVOD_HD uint32_t float_sort_key(float f) {
    uint32_t u = f2u(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- 3x3 SVD: Eigen 3.3 JacobiSVD<MatrixXf>(cov, ComputeFullU) restated (two-sided Jacobi,
// sweep order (p,q) = (1,0),(2,0),(2,1); Eigen/src/SVD/JacobiSVD.h, Jacobi/Jacobi.h).
// Outputs: singular values sorted descending, U columns. -----------------------------------
struct Svd3 {
    float sv[3];
    float U[9];  // row-major U(r,c) = U[3*r+c]
};

SCVOD_HD void jacobi_make(float x, float y, float z, float& c, float& s) {
    // JacobiRotation::makeJacobi(x, y, z)
    float deno = 2.0f * fabs_f(y);
    if (deno < 1.17549435e-38f) {
        c = 1.0f;
        s = 0.0f;
    } else {
        float tau = (x - z) / deno;
        float w = sqrt_f(tau * tau + 1.0f);
        float t;
        if (tau > 0.0f)
            t = 1.0f / (tau + w);
        else
            t = 1.0f / (tau - w);
        float sign_t = t > 0.0f ? 1.0f : -1.0f;
        float n = 1.0f / sqrt_f(t * t + 1.0f);
        s = -sign_t * (y / fabs_f(y)) * fabs_f(t) * n;
        c = n;
    }
}

SCVOD_HD void svd3_jacobi(const float cov[9], Svd3& out) {
    const float precision = 2.0f * 1.1920929e-07f;  // 2 * epsilon
    const float considerAsZero = 1.17549435e-38f;    // numeric_limits<float>::min()
    float W[9], U[9];
    float scale = 0.0f;
    for (int i = 0; i < 9; ++i) {
        float a = fabs_f(cov[i]);
        if (a > scale) scale = a;
    }
    if (scale == 0.0f) scale = 1.0f;
    for (int i = 0; i < 9; ++i) W[i] = cov[i] / scale;
    for (int i = 0; i < 9; ++i) U[i] = 0.0f;
    U[0] = U[4] = U[8] = 1.0f;
    float maxDiag = fabs_f(W[0]);
    if (fabs_f(W[4]) > maxDiag) maxDiag = fabs_f(W[4]);
    if (fabs_f(W[8]) > maxDiag) maxDiag = fabs_f(W[8]);
    bool finished = false;
    int guard = 0;
    while (!finished && guard < 64) {
        ++guard;
        finished = true;
        for (int p = 1; p < 3; ++p) {
            for (int q = 0; q < p; ++q) {
                float thr = precision * maxDiag;
                if (considerAsZero > thr) thr = considerAsZero;
                float wpq = W[3 * p + q], wqp = W[3 * q + p];
                if (fabs_f(wpq) > thr || fabs_f(wqp) > thr) {
                    finished = false;
                    // real_2x2_jacobi_svd
                    float m00 = W[3 * p + p], m01 = wpq, m10 = wqp, m11 = W[3 * q + q];
                    float t = m00 + m11;
                    float d = m10 - m01;
                    float r1c, r1s;
                    if (fabs_f(d) < considerAsZero) {
                        r1s = 0.0f;
                        r1c = 1.0f;
                    } else {
                        float u = t / d;
                        float tmp = sqrt_f(1.0f + u * u);
                        r1s = 1.0f / tmp;
                        r1c = u / tmp;
                    }
                    // m.applyOnTheLeft(0,1,rot1): row0' = c*row0 + s*row1 ; row1' = -s*row0 + c*row1
                    if (!(r1c == 1.0f && r1s == 0.0f)) {
                        float a0 = m00, a1 = m01, b0 = m10, b1 = m11;
                        m00 = r1c * a0 + r1s * b0;
                        m01 = r1c * a1 + r1s * b1;
                        m10 = -r1s * a0 + r1c * b0;
                        m11 = -r1s * a1 + r1c * b1;
                    }
                    float jrc, jrs;
                    jacobi_make(m00, m01, m11, jrc, jrs);
                    // j_left = rot1 * j_right.transpose();  transpose = (c, -s)
                    float tc = jrc, ts = -jrs;
                    float jlc = r1c * tc - r1s * ts;
                    float jls = r1c * ts + r1s * tc;
                    // m_workMatrix.applyOnTheLeft(p,q,j_left): rows p,q
                    if (!(jlc == 1.0f && jls == 0.0f)) {
                        for (int i = 0; i < 3; ++i) {
                            float xi = W[3 * p + i], yi = W[3 * q + i];
                            W[3 * p + i] = jlc * xi + jls * yi;
                            W[3 * q + i] = -jls * xi + jlc * yi;
                        }
                    }
                    // m_matrixU.applyOnTheRight(p,q,j_left.transpose()): columns p,q rotated
                    // by (j_left.transpose()).transpose() == j_left
                    if (!(jlc == 1.0f && jls == 0.0f)) {
                        for (int i = 0; i < 3; ++i) {
                            float xi = U[3 * i + p], yi = U[3 * i + q];
                            U[3 * i + p] = jlc * xi + jls * yi;
                            U[3 * i + q] = -jls * xi + jlc * yi;
                        }
                    }
                    // m_workMatrix.applyOnTheRight(p,q,j_right): columns p,q by j_right.transpose()
                    if (!(tc == 1.0f && ts == 0.0f)) {
                        for (int i = 0; i < 3; ++i) {
                            float xi = W[3 * i + p], yi = W[3 * i + q];
                            W[3 * i + p] = tc * xi + ts * yi;
                            W[3 * i + q] = -ts * xi + tc * yi;
                        }
                    }
                    float ap = fabs_f(W[3 * p + p]), aq = fabs_f(W[3 * q + q]);
                    float mx = ap > aq ? ap : aq;
                    if (mx > maxDiag) maxDiag = mx;
                }
            }
        }
    }
    float sv[3];
    for (int i = 0; i < 3; ++i) {
        float a = W[4 * i];
        sv[i] = fabs_f(a);
        if (a < 0.0f) {
            U[i] = -U[i];
            U[3 + i] = -U[3 + i];
            U[6 + i] = -U[6 + i];
        }
    }
    for (int i = 0; i < 3; ++i) sv[i] *= scale;
    // sort descending (first maximum wins), stop at a zero remainder
    for (int i = 0; i < 3; ++i) {
        int pos = i;
        float mx = sv[i];
        for (int j = i + 1; j < 3; ++j)
            if (sv[j] > mx) {
                mx = sv[j];
                pos = j;
            }
        if (mx == 0.0f) break;
        if (pos != i) {
            float t = sv[i];
            sv[i] = sv[pos];
            sv[pos] = t;
            for (int r = 0; r < 3; ++r) {
                float tu = U[3 * r + i];
                U[3 * r + i] = U[3 * r + pos];
                U[3 * r + pos] = tu;
            }
        }
    }
    for (int i = 0; i < 3; ++i) out.sv[i] = sv[i];
    for (int i = 0; i < 9; ++i) out.U[i] = U[i];
}

// ---- fp32 sin / cos (the closed-form cubic of pcl::computeRoots).  The reference calls glibc's sinf / cosf; they are restated
// here by a double evaluation rounded once to float, the same on the host and on the device: argument reduction by the nearest
// multiple of pi/2 (fdlibm's two-part pi/2, exact for |x| < 2^20), then Taylor series to x^17 / x^16 on |r| <= pi/4 (truncation
// below 1e-18 relative).  Almost always the correctly rounded result; glibc's are within 0.56 ulp, so a few results differ from
// glibc in the last bit (DESIGN section 2 gives the count over [0, pi/3], tests/test_region_growing_ref.py checks it). ----------
SCVOD_HD double sin_poly_d(double r) {
    const double z = r * r;
    double p = 1.0 / 355687428096000.0;                   // 1/17!
    p = p * z - 1.0 / 1307674368000.0;                    // 1/15!
    p = p * z + 1.0 / 6227020800.0;                       // 1/13!
    p = p * z - 1.0 / 39916800.0;                         // 1/11!
    p = p * z + 1.0 / 362880.0;                           // 1/9!
    p = p * z - 1.0 / 5040.0;                             // 1/7!
    p = p * z + 1.0 / 120.0;                              // 1/5!
    p = p * z - 1.0 / 6.0;                                // 1/3!
    return r + r * (z * p);
}
SCVOD_HD double cos_poly_d(double r) {
    const double z = r * r;
    double p = 1.0 / 20922789888000.0;                    // 1/16!
    p = p * z - 1.0 / 87178291200.0;                      // 1/14!
    p = p * z + 1.0 / 479001600.0;                        // 1/12!
    p = p * z - 1.0 / 3628800.0;                          // 1/10!
    p = p * z + 1.0 / 40320.0;                            // 1/8!
    p = p * z - 1.0 / 720.0;                              // 1/6!
    p = p * z + 1.0 / 24.0;                               // 1/4!
    p = p * z - 0.5;                                      // 1/2!
    return 1.0 + z * p;
}
// quadrant q of x and the reduced argument r = x - q pi/2
SCVOD_HD double trig_reduce(float x, int* q) {
    const double xd = (double)x;
    const double k = __builtin_rint(xd * 6.36619772367581382433e-01);  // 2/pi
    *q = (int)((long long)k & 3);
    return (xd - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11;
}
SCVOD_HD float sin_f32(float x) {
    if (!(fabs_f(x) < 1048576.f)) return x - x;  // NaN / inf -> NaN; |x| >= 2^20 is outside the domain (never met here)
    int q;
    const double r = trig_reduce(x, &q);
    const double v = (q & 1) ? cos_poly_d(r) : sin_poly_d(r);
    return (float)((q & 2) ? -v : v);
}
SCVOD_HD float cos_f32(float x) {
    if (!(fabs_f(x) < 1048576.f)) return x - x;
    int q;
    const double r = trig_reduce(x, &q);
    const double v = (q & 1) ? sin_poly_d(r) : cos_poly_d(r);
    return (float)(((q + 1) & 2) ? -v : v);
}

// ---- smallest eigenpair of a symmetric 3x3 float matrix: pcl::eigen33(mat, eigenvalue, eigenvector) of PCL 1.8
// (common/include/pcl/common/impl/eigen.hpp) with pcl::computeRoots / computeRoots2, in pure fp32 (row-major m[9]).  Eigen's
// reductions over three terms (squaredNorm, dot) add as a + (b + c); std::sin / std::cos / std::atan2 are sin_f32 / cos_f32 /
// atan2_f32.  Returns the eigenvalue scaled back; v is the normalised largest row cross product (NaN for a zero matrix). ----------
SCVOD_HD void eig_roots2_f32(float b, float c, float r[3]) {
    r[0] = 0.f;
    float d = (float)((double)(b * b) - 4.0 * (double)c);  // Scalar(b * b - 4.0 * c): the 4.0 is a double
    if ((double)d < 0.0) d = 0.f;
    const float sd = sqrt_f(d);
    r[2] = 0.5f * (b + sd);
    r[1] = 0.5f * (b - sd);
}
SCVOD_HD void eig_roots_f32(const float m[9], float r[3]) {
    const float m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[4], m12 = m[5], m22 = m[8];
    const float c0 = m00 * m11 * m22 + 2.f * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01;
    const float c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12;
    const float c2 = m00 + m11 + m22;
    if (fabs_f(c0) < 1.1920928955078125e-07f) {  // Eigen::NumTraits<float>::epsilon()
        eig_roots2_f32(c2, c1, r);
        return;
    }
    const float s_inv3 = (float)(1.0 / 3.0);
    const float s_sqrt3 = sqrt_f(3.f);
    const float c2_over_3 = c2 * s_inv3;
    float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
    if (a_over_3 > 0.f) a_over_3 = 0.f;
    const float half_b = 0.5f * (c0 + c2_over_3 * (2.f * c2_over_3 * c2_over_3 - c1));
    float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
    if (q > 0.f) q = 0.f;
    const float rho = sqrt_f(-a_over_3);
    const float theta = atan2_f32(sqrt_f(-q), half_b) * s_inv3;
    const float cos_theta = cos_f32(theta);
    const float sin_theta = sin_f32(theta);
    r[0] = c2_over_3 + 2.f * rho * cos_theta;
    r[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
    r[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
    float t;
    if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
    if (r[1] >= r[2]) {
        t = r[1]; r[1] = r[2]; r[2] = t;
        if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
    }
    if (r[0] <= 0.f) eig_roots2_f32(c2, c1, r);
}
SCVOD_HD void eigen33_min_f32(const float mat[9], float* eigenvalue, float v[3]) {
    float scale = 0.f;
    for (int i = 0; i < 9; ++i) {
        const float a = fabs_f(mat[i]);
        if (a > scale) scale = a;  // (Eigen's maxCoeff: the first of equal maxima; NaN never replaces)
    }
    if (scale <= 1.17549435082228750797e-38f) scale = 1.f;  // std::numeric_limits<float>::min()
    float m[9];
    for (int i = 0; i < 9; ++i) m[i] = mat[i] / scale;
    float r[3];
    eig_roots_f32(m, r);
    *eigenvalue = r[0] * scale;
    m[0] -= r[0];
    m[4] -= r[0];
    m[8] -= r[0];
    float c[3][3];
    const int ra[3] = {0, 0, 1}, rb[3] = {1, 2, 2};  // rows (0,1), (0,2), (1,2)
    float len[3];
    for (int k = 0; k < 3; ++k) {
        const float* a = m + 3 * ra[k];
        const float* b = m + 3 * rb[k];
        c[k][0] = a[1] * b[2] - a[2] * b[1];
        c[k][1] = a[2] * b[0] - a[0] * b[2];
        c[k][2] = a[0] * b[1] - a[1] * b[0];
        len[k] = c[k][0] * c[k][0] + (c[k][1] * c[k][1] + c[k][2] * c[k][2]);
    }
    const int k = (len[0] >= len[1] && len[0] >= len[2]) ? 0 : ((len[1] >= len[0] && len[1] >= len[2]) ? 1 : 2);
    const float n = sqrt_f(len[k]);
    v[0] = c[k][0] / n;
    v[1] = c[k][1] / n;
    v[2] = c[k][2] / n;
}

// ---- normal and curvature of one point from its neighbours, NormalEstimation::computePointNormal (PCL 1.8): the covariance of
// computeMeanAndCovarianceMatrix in its indices form (Scalar = float; nine sums in list order, divided by the count, diagonal
// E[xx] - mean^2), then solvePlaneParameters.  xyz: the cnt neighbours' coordinates in list order.  out = {nx, ny, nz, curvature};
// NaN everywhere for fewer than 3 neighbours. ---------------------------------------------------------------------------------
template <typename GetXyz>
SCVOD_HD void point_normal_f32(int cnt, GetXyz xyz, float out[4]) {
    if (cnt < 3) {
        const float nan = u2f(0x7fc00000u);
        out[0] = out[1] = out[2] = out[3] = nan;
        return;
    }
    float a[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < cnt; ++j) {
        float x, y, z;
        xyz(j, x, y, z);
        a[0] += x * x;
        a[1] += x * y;
        a[2] += x * z;
        a[3] += y * y;
        a[4] += y * z;
        a[5] += z * z;
        a[6] += x;
        a[7] += y;
        a[8] += z;
    }
    const float fc = (float)cnt;
    for (int i = 0; i < 9; ++i) a[i] = a[i] / fc;
    float cov[9];
    cov[0] = a[0] - a[6] * a[6];
    cov[1] = a[1] - a[6] * a[7];
    cov[2] = a[2] - a[6] * a[8];
    cov[4] = a[3] - a[7] * a[7];
    cov[5] = a[4] - a[7] * a[8];
    cov[8] = a[5] - a[8] * a[8];
    cov[3] = cov[1];
    cov[6] = cov[2];
    cov[7] = cov[5];
    float ev, v[3];
    eigen33_min_f32(cov, &ev, v);
    out[0] = v[0];
    out[1] = v[1];
    out[2] = v[2];
    const float eig_sum = cov[0] + cov[4] + cov[8];
    out[3] = eig_sum != 0.f ? fabs_f(ev / eig_sum) : 0.f;
}

// RegionGrowing::validatePoint in smooth mode: q joins p's segment unless |n_q . n_p| < cos(theta) (NaN passes)
SCVOD_HD bool rg_smooth_ok(const float* nq, const float* np, float cos_t) {
    const float d = nq[0] * np[0] + (nq[1] * np[1] + nq[2] * np[2]);
    return !(fabs_f(d) < cos_t);
}
// seed rank of a curvature: ascending, NaN before every finite value
SCVOD_HD uint32_t rg_curv_key(float c) { return c != c ? 0u : float_sort_key(c); }

// ---- intensity calibration by incidence angle, SSC::intensityCalibrationByCurvature (ssc.cpp:101-105, 140-151) for one point:
// intensity clamped to max_intensity, divided by |cos| of the angle between the normal n and the point p (floor 0.3), capped again.
// Eigen's fixed-size 3-vector reductions associate as a0 + (a1 + a2); no FMA.  A NaN normal gives NaN: both
// comparisons are false, as in the C++.  flags (optional): bit 0 clamped before, bit 1 floored at 0.3, bit 2 capped after. -------
SCVOD_HD float calibrated_intensity_f32(float intensity, float max_intensity, const float n[3], float px, float py, float pz, int* flags) {
    int f = 0;
    float i0 = intensity;
    if (i0 > max_intensity) {
        i0 = max_intensity;
        f |= 1;
    }
    const float dot = n[0] * px + (n[1] * py + n[2] * pz);
    const float nn = sqrt_f(n[0] * n[0] + (n[1] * n[1] + n[2] * n[2]));
    const float pn = sqrt_f(px * px + (py * py + pz * pz));
    float c = fabs_f(dot / (nn * pn));
    if ((double)c < 0.3) {
        c = (float)0.3;
        f |= 2;
    }
    float v = i0 / c;
    if (v > max_intensity) {
        v = max_intensity;
        f |= 4;
    }
    if (flags) *flags = f;
    return v;
}

// ---- double log / exp (the eigenvalue features call std::log and std::pow, ssc.cpp:703, 713).  The device's libm and glibc do not
// agree bit for bit, so Sun fdlibm's e_log.c / e_exp.c are restated operation by operation: IEEE add / mul / div only, the same bits
// on the host and on the device, each within 1 ulp of the exact value.  How far they are from glibc is measured, not assumed
// (tests/test_capi_object_shapes.py). -----------------------------------------------------------------------------
SCVOD_HD double log_f64(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, two54 = 1.80143985094819840000e+16,
                 Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                 Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    const double zero = 0.0;
    uint64_t bx = d2u(x);
    int32_t hx = (int32_t)(bx >> 32);
    uint32_t lx = (uint32_t)bx;
    int32_t k = 0;
    if (hx < 0x00100000) {                                                /* x < 2**-1022 */
        if ((((uint32_t)hx & 0x7fffffffu) | lx) == 0) return -two54 / zero; /* log(+-0) = -inf */
        if (hx < 0) return (x - x) / zero;                                /* log(-#) = NaN */
        k -= 54;
        x *= two54; /* subnormal number, scale up x */
        bx = d2u(x);
        hx = (int32_t)(bx >> 32);
    }
    if (hx >= 0x7ff00000) return x + x;
    k += (hx >> 20) - 1023;
    hx &= 0x000fffff;
    int32_t i = (hx + 0x95f64) & 0x100000;
    x = u2d(((uint64_t)(uint32_t)(hx | (i ^ 0x3ff00000)) << 32) | (uint32_t)bx); /* normalize x or x/2 */
    k += (i >> 20);
    const double f = x - 1.0;
    if ((0x000fffff & (2 + hx)) < 3) { /* |f| < 2**-20 */
        if (f == zero) {
            if (k == 0) return zero;
            const double dk = (double)k;
            return dk * ln2_hi + dk * ln2_lo;
        }
        const double R = f * f * (0.5 - 0.33333333333333333 * f);
        if (k == 0) return f - R;
        const double dk = (double)k;
        return dk * ln2_hi - ((R - dk * ln2_lo) - f);
    }
    const double s = f / (2.0 + f);
    const double dk = (double)k;
    const double z = s * s;
    i = hx - 0x6147a;
    const double w = z * z;
    const int32_t j = 0x6b851 - hx;
    const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
    const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    i |= j;
    const double R = t2 + t1;
    if (i > 0) {
        const double hfsq = 0.5 * f * f;
        if (k == 0) return f - (hfsq - s * (hfsq + R));
        return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
    }
    if (k == 0) return f - s * (f - R);
    return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

SCVOD_HD double exp_f64(double x) {
    const double one = 1.0, huge = 1.0e+300, twom1000 = 9.33263618503218878990e-302, o_threshold = 7.09782712893383973096e+02,
                 u_threshold = -7.45133219101941108420e+02, ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10,
                 invln2 = 1.44269504088896338700e+00, P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03,
                 P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
    const uint64_t bx = d2u(x);
    uint32_t hx = (uint32_t)(bx >> 32);
    const int xsb = (int)((hx >> 31) & 1u); /* sign bit of x */
    hx &= 0x7fffffffu;                      /* high word of |x| */
    if (hx >= 0x40862E42u) {                /* |x| >= 709.78... */
        if (hx >= 0x7ff00000u) {
            if (((hx & 0xfffffu) | (uint32_t)bx) != 0) return x + x; /* NaN */
            return (xsb == 0) ? x : 0.0;                            /* exp(+-inf) = {inf, 0} */
        }
        if (x > o_threshold) return huge * huge;         /* overflow */
        if (x < u_threshold) return twom1000 * twom1000; /* underflow */
    }
    double hi = 0.0, lo = 0.0;
    int32_t k = 0;
    if (hx > 0x3fd62e42u) {        /* |x| > 0.5 ln2 */
        if (hx < 0x3FF0A2B2u) {    /* and |x| < 1.5 ln2 */
            hi = xsb ? x + ln2HI : x - ln2HI;
            lo = xsb ? -ln2LO : ln2LO;
            k = 1 - xsb - xsb;
        } else {
            k = (int32_t)(invln2 * x + (xsb ? -0.5 : 0.5));
            const double t = (double)k;
            hi = x - t * ln2HI; /* t * ln2HI is exact here */
            lo = t * ln2LO;
        }
        x = hi - lo;
    } else if (hx < 0x3e300000u) { /* |x| < 2**-28 */
        if (huge + x > one) return one + x;
    }
    const double t = x * x;
    const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    if (k == 0) return one - ((x * c) / (c - 2.0) - x);
    const double y = one - ((lo - (x * c) / (2.0 - c)) - hi);
    if (k >= -1021) return u2d(d2u(y) + ((uint64_t)(int64_t)k << 52)); /* add k to y's exponent */
    return u2d(d2u(y) + ((uint64_t)(int64_t)(k + 1000) << 52)) * twom1000;
}

// pow(x, k) of the features: exp_f64(k * log_f64(x)) for x > 0 (not the correctly rounded power: the product's rounding is magnified
// by its size); the C library's special cases otherwise -- pow(x, 0) = 1 also for a NaN, NaN in NaN out,
// pow(+-0, k) = 0 for k > 0 and inf for k < 0 (signed for an odd integer k), a negative finite x with a k that is not an integer
// NaN.  An integer k with a negative x goes through |x| and takes the sign of an odd k.  pow_f64_with takes log_f64(|x|) from the
// caller, who may have one inlined copy of log_f64 serve several arguments (k_obj_shape: scalar registers).
SCVOD_HD bool finite_d(double x) { return (d2u(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
SCVOD_HD double pow_f64_with(double x, double k, double log_abs_x) {
    if (k == 0.0) return 1.0;
    if (x != x || k != k) return x + k;
    if (x == 0.0) {
        const bool odd = fabs_d(k) < 9007199254740992.0 && (double)(int64_t)k == k && ((int64_t)k & 1) != 0;
        const double r = k > 0.0 ? 0.0 : 1.0 / 0.0;
        return (odd && (d2u(x) >> 63)) ? -r : r;  // (an odd integer k keeps the sign of a zero)
    }
    bool neg = false;
    if (x < 0.0 && fabs_d(k) < 9007199254740992.0) {  // (every double of that size and beyond, +-inf included, is an even integer)
        const double kt = (double)(int64_t)k;
        if (kt != k) return finite_d(x) ? (x - x) / (x - x) : (k > 0.0 ? 1.0 / 0.0 : 0.0);  // NaN; pow(-inf, k) = +inf or +0
        neg = ((int64_t)k & 1) != 0;
    }
    const double r = exp_f64(k * log_abs_x);
    return neg ? -r : r;
}
SCVOD_HD double pow_f64(double x, double k) { return pow_f64_with(x, k, log_f64(fabs_d(x))); }

// ---- the eigenvalue descriptor of one cluster, SSC::getDescriptorByEigenValue (ssc.cpp:659-721, switched off there) --------------
struct FeatureParams {  // feature/k*_ (utility.h:246-253, 318-325); the layout of scvod_feature_params
    double one_third, linearity_max, planarity_max, scattering_max, omnivariance_max, anisotropy_max, eigen_entropy_max,
        change_of_curvature_max;
};
struct ObjShape {  // the layout of scvod_object_shape (96 bytes)
    float cov[6];
    float eig[3];
    int32_t flags;
    double feat[7];
};
// pcl::computeCovarianceMatrix(cloud, centroid, cov) of PCL 1.8 for one point: the six products of p = xyz - centroid that the six
// chains add (xx, xy, xz through q = p * p.x; yy, yz, zz directly).  Order {xx, xy, xz, yy, yz, zz}.
SCVOD_HD void shape_products(float x, float y, float z, float cx, float cy, float cz, float pr[6]) {
    const float px = x - cx, py = y - cy, pz = z - cz;
    pr[3] = py * py;
    pr[4] = py * pz;
    pr[5] = pz * pz;
    pr[0] = px * px;
    pr[1] = py * px;
    pr[2] = pz * px;
}

// from the six sums to the record: singular values of the symmetric matrix by svd3_jacobi, ascending (swap_if_gt, ssc.cpp:4-10,
// 676-678), then the features in double, literally as ssc.cpp:680-718 writes them (e1 is the SMALLEST eigenvalue's share; of the
// entropy only the third term is divided).  Divisions by zero and 0 * -inf stay what IEEE makes of them: flags bit 0.
SCVOD_HD void shape_finish(const float cov6[6], int n_points, const FeatureParams& K, ObjShape& r) {
    for (int i = 0; i < 6; ++i) r.cov[i] = cov6[i];
    const float m[9] = {cov6[0], cov6[1], cov6[2], cov6[1], cov6[3], cov6[4], cov6[2], cov6[4], cov6[5]};
    Svd3 sv;
    svd3_jacobi(m, sv);
    float ev0 = sv.sv[0], ev1 = sv.sv[1], ev2 = sv.sv[2], t;
    if (ev0 > ev1) { t = ev0; ev0 = ev1; ev1 = t; }
    if (ev0 > ev2) { t = ev0; ev0 = ev2; ev2 = t; }
    if (ev1 > ev2) { t = ev1; ev1 = ev2; ev2 = t; }
    r.eig[0] = ev0;
    r.eig[1] = ev1;
    r.eig[2] = ev2;
    const double sum_eigenvalues = (double)(ev0 + ev1 + ev2);  // (the additions are float's)
    const double e1 = (double)ev0 / sum_eigenvalues;
    const double e2 = (double)ev1 / sum_eigenvalues;
    const double e3 = (double)ev2 / sum_eigenvalues;
    const double sum_of_eigenvalues = e1 + e2 + e3;
    const double e123 = e1 * e2 * e3;
    double l1 = e1, l2 = e2, l3 = e3, l123 = fabs_d(e123);  // -> log_f64 of each, by ONE inlined copy of log_f64
#if defined(__clang__)
#pragma clang loop unroll(disable)
#endif
    for (int it = 0; it < 4; ++it) {
        const double l = log_f64(l1);
        l1 = l2;
        l2 = l3;
        l3 = l123;
        l123 = l;
    }
    r.feat[0] = fabs_d((e1 - e2) / e1 / K.linearity_max);
    r.feat[1] = fabs_d((e2 - e3) / e1 / K.planarity_max);
    r.feat[2] = fabs_d(e3 / e1 / K.scattering_max);
    r.feat[3] = fabs_d(pow_f64_with(e123, K.one_third, l123) / K.omnivariance_max);
    r.feat[4] = fabs_d((e1 - e3) / e1 / K.anisotropy_max);
    r.feat[5] = fabs_d((e1 * l1) + (e2 * l2) + (e3 * l3) / K.eigen_entropy_max);
    r.feat[6] = fabs_d(e3 / sum_of_eigenvalues / K.change_of_curvature_max);
    int fl = n_points < 3 ? 2 : 0;
    for (int i = 0; i < 7; ++i)
        if (!finite_d(r.feat[i])) fl |= 1;
    r.flags = fl;
}

// ---- the ESF descriptor of one cluster (SSC::getDescriptorByEnsembleShape, ssc.cpp:760-786; pcl::ESFEstimation of PCL 1.8's
// features/impl/esf.hpp in structure).  The reference's numbers do not repeat (rand() seeded with time(0), an uninitialised fold
// array), so this is the project's convention: a counter-based sampler, invalid samples skipped, integer
// histograms.  fp32 throughout, in the written order, no contraction.  The kernel (scvod_objesf.hip) and the CPU helper
// (tests/helpers/object_esf_ref.cpp) both call these. -------------------------------------------------------------------------------
constexpr int kEsfGrid = 64;          // voxels per axis of the occupancy grid
constexpr int kEsfBins = 64;          // bins per histogram
constexpr int kEsfHists = 10;         // A3 in / out / mix, D3 in / out / mix, D2 in / out / mix, ratio
constexpr int kEsfSig = kEsfHists * kEsfBins;
constexpr int kEsfIn = 0, kEsfOut = 1, kEsfMix = 2;  // class of a line or a triangle; the order of scvod_object_esf::lines
constexpr int kEsfFlagNoSample = 1, kEsfFlagFewPoints = 2, kEsfFlagExtent = 4, kEsfFlagMasked = 8;
struct ObjEsf {  // the layout of scvod_object_esf (64 bytes)
    float fold10[10];
    int32_t n_valid, n_points, flags;
    uint32_t lines[3];
};
// T[b] = (float)cos((b - 0.5) * pi / 126), b = 1 .. 63 (T[0] is never read): the angle bin of a cosine x is the number of b with
// x <= T[b], so no inverse trigonometric function runs anywhere (tests/test_capi_object_esf.py checks the literals)
#define SCVOD_ESF_COS_TABLE                                                                                                  \
    {2.0f, 0.999922276f, 0.999300718f, 0.998057902f, 0.99619472f, 0.993712187f, 0.99061197f, 0.986895978f,                 \
     0.982566476f, 0.977626145f, 0.972078145f, 0.965925813f, 0.959173083f, 0.951824069f, 0.943883359f,                      \
     0.935355842f, 0.926246941f, 0.916562259f, 0.906307817f, 0.895489931f, 0.884115398f, 0.87219125f,                       \
     0.859724939f, 0.846724212f, 0.833197117f, 0.819152057f, 0.804597795f, 0.789543331f, 0.773998082f,                      \
     0.757971704f, 0.741474152f, 0.724515676f, 0.707106769f, 0.689258337f, 0.670981407f, 0.652287424f,                      \
     0.63318789f, 0.613694787f, 0.593820214f, 0.57357645f, 0.552976131f, 0.532032073f, 0.510757267f,                        \
     0.489165008f, 0.467268616f, 0.44508177f, 0.42261827f, 0.399892032f, 0.376917213f, 0.353708059f,                        \
     0.330279052f, 0.306644738f, 0.282819808f, 0.258819044f, 0.234657407f, 0.210349888f, 0.185911611f,                      \
     0.16135776f, 0.13670361f, 0.111964479f, 0.0871557444f, 0.0622928292f, 0.0373911932f, 0.0124663142f}

SCVOD_HD uint32_t esf_mix(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}
// index j (0, 1, 2) of sample k in an object of n points: a function of (seed, k, n) alone
SCVOD_HD int esf_draw(uint32_t seed, uint32_t k, int j, int n) {
    const uint32_t h = esf_mix(seed + 0x9E3779B9u * (3u * k + (uint32_t)j + 1u));
    return (int)(((uint64_t)h * (uint64_t)(uint32_t)n) >> 32);
}
SCVOD_HD float esf_dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return dx * dx + dy * dy + dz * dz;
}
// the voxel of a scaled coordinate (the points lie in [-32, 32]); a coordinate that is no number lands in voxel 0
SCVOD_HD int esf_voxel(float v) {
    float f = v < 0.f ? floor_f(v) + 32.0f : ceil_f(v) + 31.0f;
    if (!(f >= 0.f)) f = 0.f;
    if (f > 63.0f) f = 63.0f;
    return (int)f;
}
SCVOD_HD bool esf_grid_test(const uint32_t* grid, int x, int y, int z) {
    const int i = (z * kEsfGrid + y) * kEsfGrid + x;
    return (grid[i >> 5] >> (i & 31)) & 1u;
}
// the line from voxel A to voxel B: m + 1 voxels, `in` of them set.  Returns the class; *cnt and *in the two counts
SCVOD_HD int esf_line(const uint32_t* grid, const int A[3], const int B[3], int* cnt, int* in) {
    const int dx = B[0] - A[0], dy = B[1] - A[1], dz = B[2] - A[2];
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
    const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1, sz = dz < 0 ? -1 : 1;
    int m = ax > ay ? ax : ay;
    if (az > m) m = az;
    // step t visits A_i + s_i * ((2 |d_i| t + m) / (2m)); the quotient and the remainder are carried from step to step (2 |d_i| <= 2m:
    // the quotient grows by at most one), so no division runs
    const int m2 = 2 * m;
    int x = A[0], y = A[1], z = A[2], ex = m, ey = m, ez = m, n_in = 0;
    for (int t = 0;;) {
        n_in += esf_grid_test(grid, x, y, z) ? 1 : 0;
        if (++t > m) break;
        ex += 2 * ax;
        ey += 2 * ay;
        ez += 2 * az;
        if (ex >= m2) ex -= m2, x += sx;
        if (ey >= m2) ey -= m2, y += sy;
        if (ez >= m2) ez -= m2, z += sz;
    }
    *cnt = m + 1;
    *in = n_in;
    return n_in >= m ? kEsfIn : (n_in <= 7 ? kEsfOut : kEsfMix);
}
SCVOD_HD int esf_triangle_class(int sum_in, int sum_cnt) { return sum_in <= 21 ? kEsfOut : (sum_cnt - sum_in < 4 ? kEsfIn : kEsfMix); }
// angle bin of the corner between two edges of lengths l1, l2 with scalar product dot.  T: SCVOD_ESF_COS_TABLE (descending, so the
// count of b with x <= T[b] is found by bisection)
SCVOD_HD int esf_angle_bin(const float* T, float dot, float l1, float l2) {
    float x = fabs_f(dot) / (l1 * l2);
    if (x > 1.0f) x = 1.0f;
    int n = 0;
    for (int step = 32; step; step >>= 1)
        if (x <= T[n + step]) n += step;
    return n;
}
SCVOD_HD int esf_bin63(float v) { return (int)floor_f(v * 63.0f + 0.5f); }
SCVOD_HD int esf_bin_of(float d, float d_max) { return esf_bin63(d / d_max); }

struct EsfSample {      // what a sample yields before its lines are traced
    int i[3];
    float a, b, c;      // edge lengths 12, 13, 23
    float heron;
    bool valid;
};
// P(i, xyz): the scaled point i of the object
template <class P>
SCVOD_HD EsfSample esf_sample(uint32_t seed, uint32_t k, int n, const P& pt, float u[3][3]) {
    EsfSample s;
    for (int j = 0; j < 3; ++j) s.i[j] = esf_draw(seed, k, j, n);
    s.valid = s.i[0] != s.i[1] && s.i[0] != s.i[2] && s.i[1] != s.i[2];
    s.a = s.b = s.c = s.heron = 0.f;
    if (!s.valid) return s;
    for (int j = 0; j < 3; ++j) pt(s.i[j], u[j]);
    s.a = sqrt_f(esf_dist2(u[0][0], u[0][1], u[0][2], u[1][0], u[1][1], u[1][2]));
    s.b = sqrt_f(esf_dist2(u[0][0], u[0][1], u[0][2], u[2][0], u[2][1], u[2][2]));
    s.c = sqrt_f(esf_dist2(u[1][0], u[1][1], u[1][2], u[2][0], u[2][1], u[2][2]));
    const float h = (s.a + s.b + s.c) * 0.5f;
    s.heron = ((h * (h - s.a)) * (h - s.b)) * (h - s.c);
    s.valid = s.heron > 0.001f;
    return s;
}
// the three corner bins of a valid sample: corner 1 (edges a, b), corner 2 (a, c), corner 3 (b, c)
SCVOD_HD void esf_corner_bins(const float* T, float u[3][3], const EsfSample& s, int bins[3]) {
    float e12[3], e13[3], e23[3];
    for (int a = 0; a < 3; ++a) {
        e12[a] = u[1][a] - u[0][a];
        e13[a] = u[2][a] - u[0][a];
        e23[a] = u[2][a] - u[1][a];
    }
    bins[0] = esf_angle_bin(T, e12[0] * e13[0] + e12[1] * e13[1] + e12[2] * e13[2], s.a, s.b);
    bins[1] = esf_angle_bin(T, e12[0] * e23[0] + e12[1] * e23[1] + e12[2] * e23[2], s.a, s.c);
    bins[2] = esf_angle_bin(T, e13[0] * e23[0] + e13[1] * e23[1] + e13[2] * e23[2], s.b, s.c);
}
// the lines 12, 13, 23 of a sample: class per line, the triangle's class, the ratio bin of a MIX line (else -1)
struct EsfLines {
    int cls[3], ratio_bin[3], tri;
};
SCVOD_HD EsfLines esf_trace(const uint32_t* grid, float u[3][3]) {
    int v[3][3];
    for (int j = 0; j < 3; ++j)
        for (int a = 0; a < 3; ++a) v[j][a] = esf_voxel(u[j][a]);
    EsfLines L;
    int sum_in = 0, sum_cnt = 0;
    const int from[3] = {0, 0, 1}, to[3] = {1, 2, 2};
    for (int l = 0; l < 3; ++l) {
        int cnt, in;
        L.cls[l] = esf_line(grid, v[from[l]], v[to[l]], &cnt, &in);
        L.ratio_bin[l] = L.cls[l] == kEsfMix ? esf_bin63((float)in / (float)cnt) : -1;
        sum_in += in;
        sum_cnt += cnt;
    }
    L.tri = esf_triangle_class(sum_in, sum_cnt);
    return L;
}
// histogram rows of the signature
SCVOD_HD int esf_row_a3(int tri) { return tri; }
SCVOD_HD int esf_row_d3(int tri) { return 3 + tri; }
SCVOD_HD int esf_row_d2(int line) { return 6 + line; }
constexpr int kEsfRowRatio = 9;
// one entry of the unnormalised signature from its counter
SCVOD_HD float esf_sig_value(int i, int count) {
    const float w[kEsfHists] = {0.5f, 0.5f, 0.5f, 0.5f, 0.5f, 1.0f, 1.0f, 2.0f, 2.0f, 2.0f};
    const int h = i / kEsfBins;
    const float value = h < 3 ? (float)count / 3.0f : (float)count;
    return value * w[h];
}
// fold10[j] of a normalised signature: ssc.cpp:774-776 from a zeroed array
SCVOD_HD float esf_fold(const float* sig, int j) {
    double s = 0.0;
    for (int i = j; i < kEsfSig; i += 10) s += (double)sig[i];
    return (float)s;
}

// ---- pose refinement (scvod_register.hip): one Gauss-Newton step, defined once.  Not from the reference. ----
// The running pose T of a scan is a row-major 3x4 in fp64.  A source point is moved with the fp32 rounding of T (reg_move, the map
// kernels' expression), its correspondence q is the target's nearest point, and the step minimises the residual over a RIGHT
// perturbation T <- T * exp(xi), xi = (omega, v): the Jacobian lives in the sensor frame and is bounded by max_range wherever the
// world origin is.  Every term of the normal equations is an fp64 expression of the fp32 inputs in the order written below, scaled
// by 2^20, rounded to nearest (ties to even) and summed as int64: integer sums do not depend on the order of the points.
//
// The scale.  With |p| <= max_range <= 256 = 2^8 and a unit normal, every entry of J is at most 2^8 in size and |r| <= 2^8 (r is
// bounded by the distance gate, max_dist <= 256): every product J_i * J_j, J_i * r, r * r is at most 2^16, scaled 2^36, and its
// rounding adds at most 1/2.  A point contributes at most three rows and a scan at most 2^24 points: |sum| <= 3 * 2^24 * (2^36 + 1)
// < 2^62 < 2^63.  The rounding error of a term is 2^-21; over n terms of either sign the sum is off by about 2^-21 * sqrt(n) of n
// units, far below the fp32 rounding of the inputs.  2^36 < 2^51 is also what reg_fix's rounding trick needs.
// Words of a scan's sums: the 21 upper-triangle entries of J^T J row by row, the 6 of J^T r, sum r^2, the correspondences, and the
// five skip counters {NaN, range, label, no correspondence, normal}.
constexpr int kRegWords = 40;  // per scan (34 used)
constexpr int kRegB = 21, kRegR2 = 27, kRegCorr = 28, kRegSkip = 29, kRegUsed = 34, kRegTerms = 28;
constexpr double kRegScale = 1048576.0, kRegInvScale = 1.0 / 1048576.0;  // 2^20
constexpr double kRegNormalEps = 1e-6;  // a target normal shorter than this (or not finite) gives no row
constexpr int kRegGo = 0, kRegConverged = 1, kRegDegenerate = 2;  // SCVOD_REG_MAX_ITERATIONS / CONVERGED / DEGENERATE

// x * 2^20 rounded to nearest, ties to even, for |x| < 2^31: y + 1.5 * 2^52 lies in [2^52, 2^53), where the 52 stored mantissa bits
// ARE the integer y + 2^51 after the addition's own rounding.  One fp64 addition and two integer operations, no conversion.
SCVOD_HD long long reg_fix(double x) {
    const double y = x * kRegScale;
    return (long long)(d2u(y + 6755399441055744.0) & 0xfffffffffffffull) - (1ll << 51);
}
// the fp32 rounding of the running pose, and a point moved by it
SCVOD_HD void reg_pose32(const double* T, float* Tf) {
    for (int i = 0; i < 12; ++i) Tf[i] = (float)T[i];
}
SCVOD_HD void reg_move(const float* T, float x, float y, float z, float* w) {
    w[0] = T[0] * x + T[1] * y + T[2] * z + T[3];
    w[1] = T[4] * x + T[5] * y + T[6] * z + T[7];
    w[2] = T[8] * x + T[9] * y + T[10] * z + T[11];
}
// 0: the point takes part; 1: a NaN coordinate; 2: sensor-frame range beyond max_range (range2 = max_range * max_range in fp32)
SCVOD_HD int reg_gate(float x, float y, float z, float range2) {
    if (x != x || y != y || z != z) return 1;
    return ((x * x + y * y) + z * z > range2) ? 2 : 0;
}
// one row (J, r) into the 28 term sums
SCVOD_HD void reg_row(const double* J, double r, long long* acc) {
    int k = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 6; ++i) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = i; j < 6; ++j) acc[k++] += reg_fix(J[i] * J[j]);
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 6; ++i) acc[kRegB + i] += reg_fix(J[i] * r);
    acc[kRegR2] += reg_fix(r * r);
}
// the sensor-frame residual r = p - R^T (q - t): dq = q - t, u = R^T dq summed left to right, r = p - u
SCVOD_HD void reg_residual(const double* T, const float* p, const float* q, double* r) {
    const double d0 = (double)q[0] - T[3], d1 = (double)q[1] - T[7], d2 = (double)q[2] - T[11];
    r[0] = (double)p[0] - ((T[0] * d0 + T[4] * d1) + T[8] * d2);
    r[1] = (double)p[1] - ((T[1] * d0 + T[5] * d1) + T[9] * d2);
    r[2] = (double)p[2] - ((T[2] * d0 + T[6] * d1) + T[10] * d2);
}
// point-to-point: three rows, J = [ -[p]x , I ]
SCVOD_HD void reg_point_terms(const double* T, const float* p, const float* q, long long* acc) {
    double r[3];
    reg_residual(T, p, q, r);
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const double J0[6] = {0.0, z, -y, 1.0, 0.0, 0.0}, J1[6] = {-z, 0.0, x, 0.0, 1.0, 0.0}, J2[6] = {y, -x, 0.0, 0.0, 0.0, 1.0};
    reg_row(J0, r[0], acc);
    reg_row(J1, r[1], acc);
    reg_row(J2, r[2], acc);
}
// point-to-plane: one row.  nu = n / sqrt(n . n) in fp64, n_l = R^T nu, e = n_l . r, J = [ (p x n_l)^T , n_l^T ].  false: the normal is
// not finite or shorter than kRegNormalEps, and nothing was added
SCVOD_HD bool reg_plane_terms(const double* T, const float* p, const float* q, const float* n, long long* acc) {
    const double a = (double)n[0], b = (double)n[1], c = (double)n[2];
    const double nn = (a * a + b * b) + c * c;
    if (!(nn >= kRegNormalEps * kRegNormalEps) || !finite_d(nn)) return false;
    const double len = sqrt_d(nn);
    const double u0 = a / len, u1 = b / len, u2 = c / len;
    const double l0 = (T[0] * u0 + T[4] * u1) + T[8] * u2, l1 = (T[1] * u0 + T[5] * u1) + T[9] * u2, l2 = (T[2] * u0 + T[6] * u1) + T[10] * u2;
    double r[3];
    reg_residual(T, p, q, r);
    const double e = (l0 * r[0] + l1 * r[1]) + l2 * r[2];
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const double J[6] = {y * l2 - z * l1, z * l0 - x * l2, x * l1 - y * l0, l0, l1, l2};
    reg_row(J, e, acc);
    return true;
}
// The solve and the update of one scan from its sums (kRegUsed words); T is updated in place unless the scan is degenerate.
//   H = sums / 2^20, g = -J^T r; H_ii += lambda * H_ii; LDL^T in place, a pivot that is not above pivot_eps * max_i H_ii is DEGENERATE,
//   as are fewer than min_corr correspondences and a step that is not finite.  Sums run over k ascending, one subtraction per term.
//   Update: the unit quaternion of (1, omega / 2) (a Cayley step: first-order correct, fixed point xi = 0, + - * / sqrt only), dR its
//   rotation matrix, R <- R dR, t <- R v + t.  dR is orthonormal to a few ulp of fp64 by construction, so over max_iterations <= 64
//   steps the product leaves the orthonormality of the initial matrix (an fp32 one, about 1e-7) by at most 64 * a few 1e-16: nothing
//   is re-orthonormalised.
// Returns kRegGo, kRegConverged (|omega| < eps_rot and |v| < eps_trans, after the update) or kRegDegenerate.
SCVOD_HD int reg_solve_update(const long long* s, long long min_corr, double lambda, double pivot_eps, double eps_rot, double eps_trans, double* T,
                              double* omega_norm, double* v_norm) {
    *omega_norm = 0.0;
    *v_norm = 0.0;
    if (s[kRegCorr] < min_corr) return kRegDegenerate;
    double H[6][6], x[6];
    int k = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 6; ++i) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = i; j < 6; ++j) {
            H[i][j] = (double)s[k] * kRegInvScale;
            H[j][i] = H[i][j];
            ++k;
        }
    }
    double top = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 6; ++i) {
        x[i] = -((double)s[kRegB + i] * kRegInvScale);
        H[i][i] = H[i][i] + lambda * H[i][i];
        if (H[i][i] > top) top = H[i][i];
    }
    const double floor_pivot = pivot_eps * top;
    // LDL^T in place: d_j on the diagonal, L below it
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 6; ++j) {
        double d = H[j][j];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int m = 0; m < j; ++m) d = d - (H[j][m] * H[j][m]) * H[m][m];
        if (!(d > floor_pivot)) return kRegDegenerate;
        H[j][j] = d;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = j + 1; i < 6; ++i) {
            double a = H[i][j];
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int m = 0; m < j; ++m) a = a - (H[i][m] * H[j][m]) * H[m][m];
            H[i][j] = a / d;
        }
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 6; ++i) {  // L z = g
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int m = 0; m < i; ++m) x[i] = x[i] - H[i][m] * x[m];
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 6; ++i) x[i] = x[i] / H[i][i];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 5; i >= 0; --i) {  // L^T xi = y
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int m = i + 1; m < 6; ++m) x[i] = x[i] - H[m][i] * x[m];
    }
    const double on = sqrt_d((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), vn = sqrt_d((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
    if (!finite_d(on) || !finite_d(vn)) return kRegDegenerate;
    const double hx = 0.5 * x[0], hy = 0.5 * x[1], hz = 0.5 * x[2];
    const double qn = sqrt_d(1.0 + ((hx * hx + hy * hy) + hz * hz));
    const double qw = 1.0 / qn, qx = hx / qn, qy = hy / qn, qz = hz / qn;
    const double D[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw),       2.0 * (qx * qz + qy * qw),
                         2.0 * (qx * qy + qz * qw),       1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw),
                         2.0 * (qx * qz - qy * qw),       2.0 * (qy * qz + qx * qw),       1.0 - 2.0 * (qx * qx + qy * qy)};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 3; ++i) {
        const double a = T[4 * i], b = T[4 * i + 1], c = T[4 * i + 2];
        T[4 * i + 3] = ((a * x[3] + b * x[4]) + c * x[5]) + T[4 * i + 3];
        T[4 * i] = (a * D[0] + b * D[3]) + c * D[6];
        T[4 * i + 1] = (a * D[1] + b * D[4]) + c * D[7];
        T[4 * i + 2] = (a * D[2] + b * D[5]) + c * D[8];
    }
    *omega_norm = on;
    *v_norm = vn;
    return (on < eps_rot && vn < eps_trans) ? kRegConverged : kRegGo;
}

// ---- surface normals of a cloud (scvod_normals.hip), defined once.  Not from the reference. ----
// The neighbourhood of a query q is every usable cloud point p with fp32 d = (ex*ex + ey*ey) + ez*ez < radius*radius, e = p - q one
// fp32 subtraction per component (q itself when it is a point of the cloud: d == 0).  Ten int64 words per query: the count k, the
// sums of e_a (3) and of e_a e_b (6: xx, xy, xz, yy, yz, zz).  A term is the fp64 product of the fp32 offsets (48 significant bits:
// exact), times 2^30, rounded to nearest (ties to even): integer sums do not depend on the order of the neighbours.
//
// The scale.  radius <= 4 bounds |e_a| by 4 (a rounding above it), a product by 2^4, a scaled term by 2^34; a cloud has at most 2^28
// points: |sum| <= 2^28 * (2^34 + 1) < 2^63.  The rounding of a term is 2^-31, below the fp32 rounding of an offset of 2^-7 m.
constexpr int kNrmWords = 10;
constexpr double kNrmScale = 1073741824.0;  // 2^30
constexpr float kNrmMaxCoord = 1.0e6f;      // a coordinate beyond it (or not finite) keeps a point out: its cell index stays an int

// a point that may be a neighbour or a query (NaN fails the comparison, an infinity exceeds the bound)
SCVOD_HD bool nrm_usable(float x, float y, float z) { return fabs_f(x) <= kNrmMaxCoord && fabs_f(y) <= kNrmMaxCoord && fabs_f(z) <= kNrmMaxCoord; }
// x * 2^30 rounded to nearest, ties to even, for |x| < 2^21 (reg_fix's expression at this scale)
SCVOD_HD long long nrm_fix(double x) {
    const double y = x * kNrmScale;
    return (long long)(d2u(y + 6755399441055744.0) & 0xfffffffffffffull) - (1ll << 51);
}
// the candidate p against the query q: true, and the ten words moved, iff p is inside the radius (r2 = radius * radius in fp32)
SCVOD_HD bool nrm_add(float px, float py, float pz, float qx, float qy, float qz, float r2, long long* s) {
    const float ex = px - qx, ey = py - qy, ez = pz - qz;
    const float d = (ex * ex + ey * ey) + ez * ez;
    if (!(d < r2)) return false;
    const double x = (double)ex, y = (double)ey, z = (double)ez;
    s[0] += 1;
    s[1] += nrm_fix(x);
    s[2] += nrm_fix(y);
    s[3] += nrm_fix(z);
    s[4] += nrm_fix(x * x);
    s[5] += nrm_fix(x * y);
    s[6] += nrm_fix(x * z);
    s[7] += nrm_fix(y * y);
    s[8] += nrm_fix(y * z);
    s[9] += nrm_fix(z * z);
    return true;
}
// The sums of a query to {nx, ny, nz, curvature}: mean and covariance of the offsets in fp64, narrowed to float, then the solver and the
// curvature expression of point_normal_f32 (one eigen specification).  NaN everywhere below min_neighbours; a zero covariance gives
// the NaN eigen33_min_f32 gives.
SCVOD_HD void normal_finish(const long long* s, int min_neighbours, float out[4]) {
    if (s[0] < (long long)min_neighbours) {
        const float nan = u2f(0x7fc00000u);
        out[0] = out[1] = out[2] = out[3] = nan;
        return;
    }
    const double k = (double)s[0];
    const double mx = (double)s[1] / kNrmScale / k, my = (double)s[2] / kNrmScale / k, mz = (double)s[3] / kNrmScale / k;
    float cov[9];
    cov[0] = (float)((double)s[4] / kNrmScale / k - mx * mx);
    cov[1] = (float)((double)s[5] / kNrmScale / k - mx * my);
    cov[2] = (float)((double)s[6] / kNrmScale / k - mx * mz);
    cov[4] = (float)((double)s[7] / kNrmScale / k - my * my);
    cov[5] = (float)((double)s[8] / kNrmScale / k - my * mz);
    cov[8] = (float)((double)s[9] / kNrmScale / k - mz * mz);
    cov[3] = cov[1];
    cov[6] = cov[2];
    cov[7] = cov[5];
    float ev, v[3];
    eigen33_min_f32(cov, &ev, v);
    out[0] = v[0];
    out[1] = v[1];
    out[2] = v[2];
    const float eig_sum = (cov[0] + cov[4]) + cov[8];
    out[3] = eig_sum != 0.f ? fabs_f(ev / eig_sum) : 0.f;
}
// pcl::flipNormalTowardsViewpoint: the normal n of the query q is negated iff it points away from the viewpoint v (a NaN normal stays)
SCVOD_HD void normal_flip(const float* v, float qx, float qy, float qz, float* n) {
    const float dot = ((v[0] - qx) * n[0] + (v[1] - qy) * n[1]) + (v[2] - qz) * n[2];
    if (dot < 0.f) {
        n[0] = -n[0];
        n[1] = -n[1];
        n[2] = -n[2];
    }
}

}  // namespace scvod
#endif  // SCVOD_MATH_H_
