// Sim3Solver's arithmetic (src/Sim3Solver.cc), one copy for the gfx950 kernels (sim3_kernels.hip) and for a host
// build (tests/sim3_math_host.cpp, which tests/test_sim3_solver_host.py holds against tests/sim3_solver_ref.py on a CPU): the draws, ComputeSim3 with
// cv::eigen and cv::Rodrigues restated, Project / FromCameraToImage and CheckInliers' test.  Readings: DESIGN.md
// 3.18.  Every operation rounds once (the builds keep fp contraction off); the one contraction the reference's
// compiler makes, u = fx*x + cx, is written as fmaf.  Nothing but + - * / sqrt, fmaf and libm64cr's correctly
// rounded atan2 / sincos is used, so that the host and the device agree bit for bit.
#pragma once
#include <cstdint>

#include "libm64_cr.h"

#if defined(__HIP__)
#define SPSLAM_SIM3_HD __host__ __device__ inline
#else
#include <cmath>
#define SPSLAM_SIM3_HD inline
#endif

namespace spslam {
namespace sim3 {

// One kept correspondence of the constructor (:62-109), in mvnIndices1's order.
struct Corr {
    float X1[3], X2[3];  // mvX3Dc1 / mvX3Dc2
    float p1[2], p2[2];  // mvP1im1 / mvP2im2
    float b1, b2;        // (float)mvnMaxError1 / 2: the size_t bound as the comparison converts it
    int32_t i1, pad;     // mvnIndices1
};
static_assert(sizeof(Corr) == 56, "Corr is 56 bytes (include/spslam_gpu.h states the scratch size)");

// One hypothesis between the two passes: mnInliersi and what GetEstimated* returns for it.
struct Hyp {
    int32_t n;
    float s;
    float R[9], t[3];
    int32_t pad[2];
};
static_assert(sizeof(Hyp) == 64, "Hyp is 64 bytes");

SPSLAM_SIM3_HD float absf(float x) { return x < 0.f ? -x : x; }

// cv::Mat 3x3 * 3x1 (+ 3x1) on rows at stride `ld`: each row summed in double from 0.0, scaled by sign, the addend
// added, rounded once (the matcher family's mat3_mul)
SPSLAM_SIM3_HD void mat3_mul(const float* T, int ld, const float* x, const float* c, double sign, float* y) {
    for (int r = 0; r < 3; r++) {
        double s = 0.0;
        for (int k = 0; k < 3; k++) s = s + (double)T[ld * r + k] * (double)x[k];
        s = s * sign;
        if (c) s = s + (double)c[r];
        y[r] = (float)s;
    }
}

// Project / FromCameraToImage (:382-423): invz = 1/z in float, x, y, then fx*x+cx contracted
SPSLAM_SIM3_HD void to_image(const float* P, float fx, float fy, float cx, float cy, float* uv) {
    const float invz = 1.0f / P[2];
    const float x = P[0] * invz, y = P[1] * invz;
    uv[0] = fmaf(fx, x, cx);
    uv[1] = fmaf(fy, y, cy);
}

// RandomInt(0, size - 1) from a raw rand() value; a value outside [0, rand_max] is clamped into the list
SPSLAM_SIM3_HD int random_int(int r, int rand_max, int size) {
    const int v = (int)(((double)r / ((double)rand_max + 1.0)) * (double)size);
    return v < 0 ? 0 : (v >= size ? size - 1 : v);
}

// The three draws of one iteration (:163-177) on vAvailableIndices = 0 .. n-1 without the array: a position holds
// its own index unless a swap-with-back wrote it, and the latest write wins.  n >= 3.
SPSLAM_SIM3_HD void draw3(const int32_t* r, int rand_max, int n, int* idx) {
    const int r0 = random_int(r[0], rand_max, n), r1 = random_int(r[1], rand_max, n - 1);
    const int r2 = random_int(r[2], rand_max, n - 2);
    idx[0] = r0;                         // position r0 then holds n-1 (the back)
    idx[1] = r1 == r0 ? n - 1 : r1;      // position r1 then holds the back of n-1 entries: position n-2's value
    const int back1 = r0 == n - 2 ? n - 1 : n - 2;
    idx[2] = r2 == r1 ? back1 : (r2 == r0 ? n - 1 : r2);
}

// The storage of the 4x4 Jacobi: a(i, j), v(i, j), w(i) floats and ir(i), ic(i) ints, indexed at run time.  The
// host keeps them in arrays; the device keeps each lane's in LDS (registers cannot be indexed at run time).
struct JacobiHost {
    float A[16], V[16], W[4];
    int R[4], C[4];
    float& a(int i, int j) { return A[4 * i + j]; }
    float& v(int i, int j) { return V[4 * i + j]; }
    float& w(int i) { return W[i]; }
    int& ir(int i) { return R[i]; }
    int& ic(int i) { return C[i]; }
};

// hypot of the Jacobi: sqrt(a*a + b*b) in double, rounded to float (floats squared in double neither overflow nor
// lose a bit, so no scaling is needed)
SPSLAM_SIM3_HD float hypot_f(float a, float b) {
    return (float)sqrt((double)a * (double)a + (double)b * (double)b);
}

template <class S>
SPSLAM_SIM3_HD void jacobi_row_max(S& J, int k) {  // indR[k]: the largest |A[k][i]|, i > k, the first of equals
    int m = k + 1;
    float mv = absf(J.a(k, m));
    for (int i = k + 2; i < 4; i++) {
        const float val = absf(J.a(k, i));
        if (mv < val) { mv = val; m = i; }
    }
    J.ir(k) = m;
}
template <class S>
SPSLAM_SIM3_HD void jacobi_col_max(S& J, int k) {  // indC[k]: the largest |A[i][k]|, i < k
    int m = 0;
    float mv = absf(J.a(0, k));
    for (int i = 1; i < k; i++) {
        const float val = absf(J.a(i, k));
        if (mv < val) { mv = val; m = i; }
    }
    J.ic(k) = m;
}
SPSLAM_SIM3_HD void jacobi_rotate(float& v0, float& v1, float c, float s) {
    const float a0 = v0, b0 = v1;
    v0 = a0 * c - b0 * s;
    v1 = a0 * s + b0 * c;
}

// cv::eigen on a symmetric 4x4 float matrix: the classical Jacobi in float on the upper triangle, the pivot the
// largest off-diagonal entry tracked per row and per column, until |pivot| <= FLT_EPSILON or 30*4*4 rotations;
// eigenvalues sorted descending by selection, eigenvectors as rows.  J.a must hold the matrix; q receives row 0.
template <class S>
SPSLAM_SIM3_HD void jacobi_first_eigenvector(S& J, float* q) {
    const float eps = 1.1920928955078125e-07f;
    for (int i = 0; i < 4; i++) {
        for (int j = 0; j < 4; j++) J.v(i, j) = i == j ? 1.f : 0.f;
        J.w(i) = J.a(i, i);
    }
    for (int k = 0; k < 4; k++) {
        if (k < 3) jacobi_row_max(J, k);
        if (k > 0) jacobi_col_max(J, k);
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int it = 0; it < 30 * 4 * 4; it++) {
        int k = 0;
        float mv = absf(J.a(0, J.ir(0)));
        for (int i = 1; i < 3; i++) {
            const float val = absf(J.a(i, J.ir(i)));
            if (mv < val) { mv = val; k = i; }
        }
        int l = J.ir(k);
        for (int i = 1; i < 4; i++) {
            const float val = absf(J.a(J.ic(i), i));
            if (mv < val) { mv = val; k = J.ic(i); l = i; }
        }
        const float p = J.a(k, l);
        if (absf(p) <= eps) break;
        const float y = (float)((double)(J.w(l) - J.w(k)) * 0.5);
        float t = absf(y) + hypot_f(p, y);
        float s = hypot_f(p, t);
        const float c = t / s;
        s = p / s;
        t = (p / t) * p;
        if (y < 0.f) { s = -s; t = -t; }
        J.a(k, l) = 0.f;
        J.w(k) = J.w(k) - t;
        J.w(l) = J.w(l) + t;
        for (int i = 0; i < k; i++) jacobi_rotate(J.a(i, k), J.a(i, l), c, s);
        for (int i = k + 1; i < l; i++) jacobi_rotate(J.a(k, i), J.a(i, l), c, s);
        for (int i = l + 1; i < 4; i++) jacobi_rotate(J.a(k, i), J.a(l, i), c, s);
        for (int i = 0; i < 4; i++) jacobi_rotate(J.v(k, i), J.v(l, i), c, s);
        for (int j = 0; j < 2; j++) {
            const int idx = j == 0 ? k : l;
            if (idx < 3) jacobi_row_max(J, idx);
            if (idx > 0) jacobi_col_max(J, idx);
        }
    }
    // only row 0 of the sorted eigenvectors is read: the first largest eigenvalue's row
    int m = 0;
    for (int i = 1; i < 4; i++)
        if (J.w(m) < J.w(i)) m = i;
    for (int i = 0; i < 4; i++) q[i] = J.v(m, i);
}

// T12 = [s*R | t] and T21 = [(1.0/s)*R.t() | -sRinv*t] as rows at stride 4 (:318-336), 12 floats each
SPSLAM_SIM3_HD void transforms(float s, const float* R, const float* t, float* T12, float* T21) {
    const double inv = 1.0 / (double)s;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            T12[4 * r + c] = s * R[3 * r + c];
            T21[4 * r + c] = (float)((double)R[3 * c + r] * inv);
        }
        T12[4 * r + 3] = t[r];
    }
    float tinv[3];
    mat3_mul(T21, 4, t, nullptr, -1.0, tinv);
    T21[3] = tinv[0]; T21[7] = tinv[1]; T21[11] = tinv[2];
}

// ComputeSim3 (:226-337) on the columns X1[i], X2[i], i = 0..2: ms12i, mR12i, mt12i
template <class S>
SPSLAM_SIM3_HD void compute_sim3(S& J, const float (&X1)[3][3], const float (&X2)[3][3], bool fix_scale, float* s12,
                                 float* R, float* t) {
    // centroids: cv::reduce sums a row as (c0 + c2) + c1 in float; C / 3 is the sum times the double 1.0/3
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];  // Pr[r][i]: row r, column (point) i
    const double third = 1.0 / 3.0;
    for (int r = 0; r < 3; r++) {
        O1[r] = (float)((double)((X1[0][r] + X1[2][r]) + X1[1][r]) * third);
        O2[r] = (float)((double)((X2[0][r] + X2[2][r]) + X2[1][r]) * third);
        for (int i = 0; i < 3; i++) {
            Pr1[r][i] = X1[i][r] - O1[r];
            Pr2[r][i] = X2[i][r] - O2[r];
        }
    }
    // M = Pr2 * Pr1.t()
    float M[3][3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double d = 0.0;
            for (int k = 0; k < 3; k++) d = d + (double)Pr2[r][k] * (double)Pr1[c][k];
            M[r][c] = (float)d;
        }
    // N: float sums, left to right
    const float N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2];
    const float N14 = M[0][1] - M[1][0], N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0];
    const float N24 = M[2][0] + M[0][2], N33 = -M[0][0] + M[1][1] - M[2][2], N34 = M[1][2] + M[2][1];
    const float N44 = -M[0][0] - M[1][1] + M[2][2];
    J.a(0, 0) = N11; J.a(0, 1) = N12; J.a(0, 2) = N13; J.a(0, 3) = N14;
    J.a(1, 0) = N12; J.a(1, 1) = N22; J.a(1, 2) = N23; J.a(1, 3) = N24;
    J.a(2, 0) = N13; J.a(2, 1) = N23; J.a(2, 2) = N33; J.a(2, 3) = N34;
    J.a(3, 0) = N14; J.a(3, 1) = N24; J.a(3, 2) = N34; J.a(3, 3) = N44;
    float q[4];
    jacobi_first_eigenvector(J, q);
    // ang = atan2(norm(vec), q0); vec = 2*ang*vec/norm(vec): the element times the double (2*ang)*(1.0/norm)
    float sq = q[1] * q[1];
    sq = sq + q[2] * q[2];
    sq = sq + q[3] * q[3];
    const double nrm = sqrt((double)sq);
    const double ang = libm64cr::atan2_(nrm, (double)q[0]);
    const double f = (2.0 * ang) * (1.0 / nrm);
    const float vec[3] = {(float)((double)q[1] * f), (float)((double)q[2] * f), (float)((double)q[3] * f)};
    // cv::Rodrigues in double: R = c*I + (1-c)*r*r^T + s*[r]x, rounded to float at the end
    double rx = (double)vec[0], ry = (double)vec[1], rz = (double)vec[2];
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < 2.220446049250313e-16) {
        for (int k = 0; k < 9; k++) R[k] = k % 4 == 0 ? 1.f : 0.f;
    } else {
        double sn, cs;
        libm64cr::sincos_(theta, &sn, &cs);
        const double c1 = 1.0 - cs, itheta = 1.0 / theta;
        rx = rx * itheta; ry = ry * itheta; rz = rz * itheta;
        const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
        const double rxm[9] = {0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0};
        for (int k = 0; k < 9; k++) R[k] = (float)((cs * (k % 4 == 0 ? 1.0 : 0.0) + c1 * rrt[k]) + sn * rxm[k]);
    }
    // P3 = R * Pr2; the scale
    float s = 1.0f;
    if (!fix_scale) {
        double nom = 0.0, den = 0.0;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                double d = 0.0;
                for (int k = 0; k < 3; k++) d = d + (double)R[3 * r + k] * (double)Pr2[k][c];
                const float p3 = (float)d;
                nom = nom + (double)Pr1[r][c] * (double)p3;  // Mat::dot, row-major, in double
                den = den + (double)(p3 * p3);               // cv::pow(P3, 2): the float square, summed in double
            }
        s = (float)(nom / den);
    }
    *s12 = s;
    // t12 = O1 - s*R*O2: the row summed in double times the double s, rounded, then the float difference
    float sRO2[3];
    mat3_mul(R, 3, O2, nullptr, (double)s, sRO2);
    for (int r = 0; r < 3; r++) t[r] = O1[r] - sRO2[r];
}

// CheckInliers' test for one correspondence (:343-362): a NaN error is no inlier
SPSLAM_SIM3_HD bool is_inlier(const Corr& c, const float* T12, const float* T21, float fx, float fy, float cx, float cy) {
    const float t12[3] = {T12[3], T12[7], T12[11]}, t21[3] = {T21[3], T21[7], T21[11]};
    float Pa[3], Pb[3], q1[2], q2[2];
    mat3_mul(T12, 4, c.X2, t12, 1.0, Pa);  // Project(mvX3Dc2, vP2im1, mT12i, mK1)
    mat3_mul(T21, 4, c.X1, t21, 1.0, Pb);  // Project(mvX3Dc1, vP1im2, mT21i, mK2)
    to_image(Pa, fx, fy, cx, cy, q1);
    to_image(Pb, fx, fy, cx, cy, q2);
    const float d1x = c.p1[0] - q1[0], d1y = c.p1[1] - q1[1];
    const float d2x = q2[0] - c.p2[0], d2y = q2[1] - c.p2[1];
    const float err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
    const float err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
    return err1 < c.b1 && err2 < c.b2;
}

}  // namespace sim3
}  // namespace spslam
