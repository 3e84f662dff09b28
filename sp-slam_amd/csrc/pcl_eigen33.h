// The steps of pcl::eigen33 (float) that the plane segmentation and the supposed-plane line fit share:
// pcl::computeRoots on a scaled matrix and the eigenvector of a shifted one.  Semantics:
// oracle/plane_oracle.cpp, oracle/supposed_oracle.cpp.  Every float operation is in the reference's order
// (the build has -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "libm_restated.h"

namespace spslam {
namespace pcl_eigen {

__device__ inline void roots2(float b, float c, float* r) {
    r[0] = 0.f;
    float d = (float)(b * b - 4.0 * c);
    if (d < 0.0) d = 0.0;
    const float sd = sqrtf(d);
    r[2] = 0.5f * (b + sd);
    r[1] = 0.5f * (b - sd);
}
// pcl::computeRoots on a scaled matrix (float), glibc-exact transcendental calls (libm_restated.h).
__device__ inline void roots3(const float (&m)[3][3], float* r) {
    const float c0 = m[0][0] * m[1][1] * m[2][2] + 2.f * m[0][1] * m[0][2] * m[1][2] - m[0][0] * m[1][2] * m[1][2] -
                     m[1][1] * m[0][2] * m[0][2] - m[2][2] * m[0][1] * m[0][1];
    const float c1 = m[0][0] * m[1][1] - m[0][1] * m[0][1] + m[0][0] * m[2][2] - m[0][2] * m[0][2] +
                     m[1][1] * m[2][2] - m[1][2] * m[1][2];
    const float c2 = m[0][0] + m[1][1] + m[2][2];
    if (fabsf(c0) < FLT_EPSILON) { roots2(c2, c1, r); return; }
    const float s_inv3 = (float)(1.0 / 3.0), s_sqrt3 = sqrtf(3.0f);
    const float c2_over_3 = c2 * s_inv3;
    float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
    if (a_over_3 > 0.f) a_over_3 = 0.f;
    const float half_b = 0.5f * (c0 + c2_over_3 * (2.f * c2_over_3 * c2_over_3 - c1));
    float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
    if (q > 0.f) q = 0.f;
    const float rho = sqrtf(-a_over_3);
    const float theta = libm::atan2f_(sqrtf(-q), half_b) * s_inv3;
    float st, ct;
    libm::sincosf_(theta, &st, &ct);
    r[0] = c2_over_3 + 2.f * rho * ct;
    r[1] = c2_over_3 - rho * (ct + s_sqrt3 * st);
    r[2] = c2_over_3 - rho * (ct - s_sqrt3 * st);
    float t;
    if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
    if (r[1] >= r[2]) {
        t = r[1]; r[1] = r[2]; r[2] = t;
        if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
    }
    if (r[0] <= 0) roots2(c2, c1, r);
}
// the scale of eigen33: the largest |entry|, 1 where that is not above FLT_MIN
__device__ inline float max_abs3(const float (&m)[3][3]) {
    float s = 0.f;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) s = fmaxf(s, fabsf(m[i][j]));
    if (s <= FLT_MIN) s = 1.f;
    return s;
}
// The eigenvector of the (scaled, eigenvalue-shifted) matrix m: the longest cross product of two of its rows,
// normalised.
__device__ inline void eigenvector_of(const float (&m)[3][3], float* evec) {
    const int pr[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    float v[3][3], len[3];
    for (int k = 0; k < 3; k++) {
        const float* a = m[pr[k][0]];
        const float* b = m[pr[k][1]];
        v[k][0] = a[1] * b[2] - a[2] * b[1];
        v[k][1] = a[2] * b[0] - a[0] * b[2];
        v[k][2] = a[0] * b[1] - a[1] * b[0];
        len[k] = v[k][0] * v[k][0] + v[k][1] * v[k][1] + v[k][2] * v[k][2];
    }
    int k = 2;
    if (len[0] >= len[1] && len[0] >= len[2]) k = 0;
    else if (len[1] >= len[0] && len[1] >= len[2]) k = 1;
    const float sl = sqrtf(len[k]);
    for (int j = 0; j < 3; j++) evec[j] = v[k][j] / sl;
}

}  // namespace pcl_eigen
}  // namespace spslam
