// CPU statement of scvod_batch_object_shapes for one object (object_shape_ref.py) -- test infrastructure only.  A plain sequential
// loop over a list of points in the library's own arithmetic (scvod_math.h: the six products, the Jacobi, log_f64 / exp_f64 and the
// feature formulas), and this image's glibc log / exp / pow beside the restated ones so that their distance can be measured.
// Built by the tests with -ffp-contract=off, as the library is.
#include <cmath>

#include "../../dr-using-scv-od_amd/csrc/scvod_math.h"

extern "C" {

// xyz [n][3] in member order, K8 = scvod_feature_params, out = one scvod_object_shape (96 bytes)
void shape_ref(const float* xyz, int n, const double* K8, void* out) {
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = 0; i < n; ++i) {
        sx += xyz[3 * i];
        sy += xyz[3 * i + 1];
        sz += xyz[3 * i + 2];
    }
    const float c = (float)n;
    const float cx = sx / c, cy = sy / c, cz = sz / c;
    float c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < n; ++i) {
        float pr[6];
        scvod::shape_products(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, cz, pr);
        for (int a = 0; a < 6; ++a) c6[a] += pr[a];
    }
    scvod::FeatureParams K = {K8[0], K8[1], K8[2], K8[3], K8[4], K8[5], K8[6], K8[7]};
    scvod::shape_finish(c6, n, K, *(scvod::ObjShape*)out);
}

void spec_log_many(const double* x, long n, double* out) {
    for (long i = 0; i < n; ++i) out[i] = scvod::log_f64(x[i]);
}
void spec_exp_many(const double* x, long n, double* out) {
    for (long i = 0; i < n; ++i) out[i] = scvod::exp_f64(x[i]);
}
void spec_pow_many(const double* x, double k, long n, double* out) {
    for (long i = 0; i < n; ++i) out[i] = scvod::pow_f64(x[i], k);
}
void libm_log_many(const double* x, long n, double* out) {
    for (long i = 0; i < n; ++i) out[i] = std::log(x[i]);
}
void libm_exp_many(const double* x, long n, double* out) {
    for (long i = 0; i < n; ++i) out[i] = std::exp(x[i]);
}
void libm_pow_many(const double* x, double k, long n, double* out) {
    for (long i = 0; i < n; ++i) out[i] = std::pow(x[i], k);
}
}
