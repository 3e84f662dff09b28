// Optimizer::OptimizeSim3's arithmetic (src/Optimizer.cc:2279-2474 over Thirdparty/g2o), one copy for the gfx950
// kernel (sim3_opt_kernels.hip) and for a host build (tests/sim3_opt_host.cpp, which tests/test_sim3_opt_host.py
// holds against the sequential referee tests/sim3_opt_ref.cpp on a CPU): g2o::Sim3 (types/sim3.h),
// VertexSim3Expmap::oplusImpl and the two projection edges (types/types_seven_dof_expmap.h), the numeric Jacobian and
// the robust quadratic form of BaseBinaryEdge (core/base_binary_edge.hpp), Eigen's pivoted dense LDLT sized by a
// template parameter, and the Levenberg-Marquardt driver with the two inlier checks.  Readings: DESIGN.md 3.19.
// All arithmetic is double in the reference's expression order, every operation rounds once (the builds keep fp
// contraction off), and sin / cos are libm64cr's correctly rounded ones, so that host and device agree bit for bit.
//
// Fixed scale only (RGB-D: mbFixScale = mSensor != MONOCULAR).  Under _fix_scale oplusImpl zeroes update[6], so
// sigma is exactly 0 and s = exp(0) = 1 in every libm; a free scale needs a correctly rounded exp, which libm64cr
// does not have.  sim3_exp therefore takes exp(sigma) from its caller, and the only caller passes 1.0.
#pragma once
#include <cstdint>

#include "libm64_cr.h"
#include "sim3_math.h"

#if defined(__HIP__)
#define SPSLAM_S3O_HD __host__ __device__ inline
#define SPSLAM_S3O_UNROLL _Pragma("unroll")
#else
#define SPSLAM_S3O_HD inline
#define SPSLAM_S3O_UNROLL
#endif

namespace spslam {
namespace sim3opt {

struct V3 { double x, y, z; };
struct Q { double w, x, y, z; };
struct S3 { Q r; V3 t; double s; };  // g2o::Sim3: the quaternion is never normalised
struct Cam { double fx, fy, cx, cy; };  // _focal_length1 = 2, _principle_point1 = 2: the context's camera, widened

// One kept correspondence of :2332-2411, in vnIndexEdge's order: e12 is (X2, obs1, w1), e21 is (X1, obs2, w2).
struct Corr {
    double X1[3], X2[3];  // P3D1c, P3D2c: float cv::Mat products, widened
    double o1[2], o2[2];  // kpUn1.pt, kpUn2.pt
    double w1, w2;        // mvInvLevelSigma2[octave], widened
    int32_t i, removed;   // vnIndexEdge; removeEdge after the first check
};
static_assert(sizeof(Corr) == 104, "Corr is 104 bytes (include/spslam_gpu.h states the scratch size)");

constexpr int kTerms = 36;  // per edge: the robust chi2, the 28 lower terms of B^T W B, the 7 of B^T omega_r
constexpr double kDelta = 1e-9;  // linearizeOplus' step

SPSLAM_S3O_HD V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
SPSLAM_S3O_HD V3 scale(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
SPSLAM_S3O_HD V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
SPSLAM_S3O_HD double abs_(double x) { return fabs(x); }
SPSLAM_S3O_HD bool finite_(double x) { return abs_(x) <= 1.7976931348623157e308; }

template <int I, int J, int K>
SPSLAM_S3O_HD void q_case(const double* R, Q& q) {
    double t = sqrt(R[4 * I] - R[4 * J] - R[4 * K] + 1.0);
    const double ci = 0.5 * t;
    t = 0.5 / t;
    q.w = (R[3 * K + J] - R[3 * J + K]) * t;
    const double cj = (R[3 * J + I] + R[3 * I + J]) * t;
    const double ck = (R[3 * K + I] + R[3 * I + K]) * t;
    q.x = I == 0 ? ci : (J == 0 ? cj : ck);
    q.y = I == 1 ? ci : (J == 1 ? cj : ck);
    q.z = I == 2 ? ci : (J == 2 ? cj : ck);
}
// Eigen Quaternion(Matrix3), R row-major; one branch per largest diagonal so that every index is a constant
SPSLAM_S3O_HD Q q_from_rot(const double* R) {
    Q q;
    double t = R[0] + R[4] + R[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (R[7] - R[5]) * t;
        q.y = (R[2] - R[6]) * t;
        q.z = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > (i == 0 ? R[0] : R[4])) i = 2;
        if (i == 0) q_case<0, 1, 2>(R, q);
        else if (i == 1) q_case<1, 2, 0>(R, q);
        else q_case<2, 0, 1>(R, q);
    }
    return q;
}
// Eigen toRotationMatrix, row-major
SPSLAM_S3O_HD void q_to_rot(const Q& q, double* R) {
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
SPSLAM_S3O_HD Q q_mul(const Q& a, const Q& b) {
    return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
            a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
SPSLAM_S3O_HD V3 q_rot(const Q& q, V3 v) {  // Eigen _transformVector
    const V3 qv{q.x, q.y, q.z};
    V3 uv = cross(qv, v);
    uv = add(uv, uv);
    return add(add(v, scale(q.w, uv)), cross(qv, uv));
}

// Sim3(const Matrix3d&, const Vector3d&, double) from float inputs (Converter::toMatrix3d / toVector3d); R at stride ld
SPSLAM_S3O_HD S3 sim3_from_float(const float* R, int ld, float tx, float ty, float tz, double s) {
    double M[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) M[3 * r + c] = (double)R[ld * r + c];
    return S3{q_from_rot(M), V3{(double)tx, (double)ty, (double)tz}, s};
}

// Sim3(const Vector7d&) (sim3.h:70-142); s = exp(sigma) comes from the caller.  *branch: 0 / 1 = theta below / not
// below eps with |sigma| < eps, 2 / 3 the same with |sigma| >= eps.
SPSLAM_S3O_HD S3 sim3_exp(const double* u, double s, int* branch) {
    const V3 w{u[0], u[1], u[2]}, ups{u[3], u[4], u[5]};
    const double sigma = u[6];
    const double theta = sqrt(w.x * w.x + w.y * w.y + w.z * w.z);
    const double O[9] = {0, -w.z, w.y, w.z, 0, -w.x, -w.y, w.x, 0};
    double O2[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    const double eps = 0.00001;
    double A, B, C, R[9];
    double sn = 0, cs = 0;
    const bool small_theta = theta < eps;
    if (!small_theta) libm64cr::sincos_(theta, &sn, &cs);
    if (small_theta)
        for (int k = 0; k < 9; k++) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + O[k]) + O2[k];
    else {
        const double a = sn / theta, b = (1 - cs) / (theta * theta);
        for (int k = 0; k < 9; k++) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + a * O[k]) + b * O2[k];
    }
    if (abs_(sigma) < eps) {
        C = 1;
        if (small_theta) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cs) / (theta2);
            B = (theta - sn) / (theta2 * theta);
        }
        *branch = small_theta ? 0 : 1;
    } else {
        C = (s - 1) / sigma;
        const double sigma2 = sigma * sigma;
        if (small_theta) {
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs, theta2 = theta * theta;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
        *branch = small_theta ? 2 : 3;
    }
    S3 out;
    out.r = q_from_rot(R);
    double W[9];
    for (int k = 0; k < 9; k++) W[k] = (A * O[k] + B * O2[k]) + C * (k % 4 == 0 ? 1.0 : 0.0);
    out.t = V3{W[0] * ups.x + W[1] * ups.y + W[2] * ups.z, W[3] * ups.x + W[4] * ups.y + W[5] * ups.z,
               W[6] * ups.x + W[7] * ups.y + W[8] * ups.z};
    out.s = s;
    return out;
}

SPSLAM_S3O_HD V3 sim3_map(const S3& S, V3 p) { return add(scale(S.s, q_rot(S.r, p)), S.t); }
SPSLAM_S3O_HD S3 sim3_inverse(const S3& S) {
    const Q c{S.r.w, -S.r.x, -S.r.y, -S.r.z};
    return S3{c, q_rot(c, scale(-1. / S.s, S.t)), 1. / S.s};
}
SPSLAM_S3O_HD S3 sim3_mul(const S3& a, const S3& b) {
    return S3{q_mul(a.r, b.r), add(scale(a.s, q_rot(a.r, b.t)), a.t), a.s * b.s};
}
// VertexSim3Expmap::oplusImpl under _fix_scale: update[6] = 0 in the caller's array, then Sim3(update) * estimate
SPSLAM_S3O_HD S3 sim3_oplus_fixed(const S3& S, double* update, int* branch) {
    update[6] = 0;
    return sim3_mul(sim3_exp(update, 1.0, branch), S);
}

// computeError of either edge: T is the estimate (e12) or its inverse (e21)
SPSLAM_S3O_HD void edge_error(const S3& T, const double* X, const double* obs, const Cam& c, double* e) {
    const V3 p = sim3_map(T, V3{X[0], X[1], X[2]});
    const double px = p.x / p.z, py = p.y / p.z;
    e[0] = obs[0] - (px * c.fx + c.cx);
    e[1] = obs[1] - (py * c.fy + c.cy);
}
// Omega * e with Omega = Identity * w: the off-diagonal zeros are multiplied (0 * inf is NaN)
SPSLAM_S3O_HD void omega_times(double w, const double* e, double* r) {
    r[0] = w * e[0] + 0.0 * e[1];
    r[1] = 0.0 * e[0] + w * e[1];
}
SPSLAM_S3O_HD double edge_chi2(double w, const double* e) {
    double r[2];
    omega_times(w, e, r);
    return e[0] * r[0] + e[1] * r[1];
}
// RobustKernelHuber::robustify
SPSLAM_S3O_HD void huber(double chi, double delta, double* rho0, double* rho1) {
    const double dsqr = delta * delta;
    if (chi <= dsqr) { *rho0 = chi; *rho1 = 1.0; return; }
    const double s = sqrt(chi);
    *rho0 = 2 * s * delta - dsqr;
    *rho1 = delta / s;
}
SPSLAM_S3O_HD double edge_robust_chi2(const S3& T, const double* X, const double* obs, double w, const Cam& c,
                                      double delta) {
    double e[2], r0, r1;
    edge_error(T, X, obs, c, e);
    huber(edge_chi2(w, e), delta, &r0, &r1);
    return r0;
}

// The 14 estimates of one linearisation, Sim3(+-delta e_d) * S: entry 2d + (0: plus, 1: minus).  They do not depend
// on the edge.
SPSLAM_S3O_HD S3 perturbed(const S3& S, int which) {
    double add_v[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int d = 0; d < 7; d++)
        if (d == which >> 1) add_v[d] = which & 1 ? -kDelta : kDelta;
    int branch;
    return sim3_oplus_fixed(S, add_v, &branch);
}

// One edge's terms at the linearisation point: the error at T, the Jacobian from the 14 perturbed estimates P (for
// e21 their inverses), then constructQuadraticForm's robust branch on Eigen's evaluation structure:
// (B^T * weightedOmega) as a 7x2 temporary times B, and B^T * (rho[1] * (-Omega e)).
SPSLAM_S3O_HD void edge_terms(const S3& T, const S3* P, const double* X, const double* obs, double w, const Cam& c,
                              double delta, double* out) {
    const double scalar = 1.0 / (2 * kDelta);
    double e[2], J[2][7];
    edge_error(T, X, obs, c, e);
    SPSLAM_S3O_UNROLL
    for (int d = 0; d < 7; d++) {
        double ep[2], em[2];
        edge_error(P[2 * d], X, obs, c, ep);
        edge_error(P[2 * d + 1], X, obs, c, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
    double rho0, rho1, oe[2];
    omega_times(w, e, oe);
    huber(e[0] * oe[0] + e[1] * oe[1], delta, &rho0, &rho1);
    out[0] = rho0;
    const double w00 = rho1 * w, w01 = rho1 * 0.0;  // robustInformation
    const double r0 = (-oe[0]) * rho1, r1 = (-oe[1]) * rho1;  // omega_r *= rho[1]
    int n = 1;
    SPSLAM_S3O_UNROLL
    for (int i = 0; i < 7; i++) {
        const double t0 = J[0][i] * w00 + J[1][i] * w01, t1 = J[0][i] * w01 + J[1][i] * w00;
        SPSLAM_S3O_UNROLL
        for (int j = 0; j <= i; j++) out[n++] = t0 * J[0][j] + t1 * J[1][j];
    }
    SPSLAM_S3O_UNROLL
    for (int i = 0; i < 7; i++) out[29 + i] = J[0][i] * r0 + J[1][i] * r1;
}

SPSLAM_S3O_HD void swapd(double& a, double& b) { const double t = a; a = b; b = t; }

// Eigen::LDLT<MatrixXd> (diagonal pivoting, lower storage) compute + solve of (H + lambda I) x = b, as
// LinearSolverDense calls it (solvers/linear_solver_dense.h:104-112); false when the matrix is not positive, x
// untouched then.  H: the lower triangle packed by rows.  Fully unrolled, the data-dependent pivot swaps over the
// candidate rows, so that the matrix stays in registers and the arithmetic is Eigen's unblocked one.
template <int N>
SPSLAM_S3O_HD bool ldlt_solve(const double* H, double lambda, const double* b, double* x) {
    double m[N][N];
    SPSLAM_S3O_UNROLL
    for (int i = 0; i < N; i++) {
        SPSLAM_S3O_UNROLL
        for (int j = 0; j < N; j++) {
            const double h = i >= j ? H[i * (i + 1) / 2 + j] : H[j * (j + 1) / 2 + i];
            m[i][j] = i == j ? h + lambda : h;
        }
    }
    int tr[N];
    int sign = 0;
    SPSLAM_S3O_UNROLL
    for (int k = 0; k < N; ++k) {
        int big = k;
        double bv = abs_(m[k][k]);
        SPSLAM_S3O_UNROLL
        for (int i = k + 1; i < N; i++)
            if (abs_(m[i][i]) > bv) { bv = abs_(m[i][i]); big = i; }
        tr[k] = big;
        SPSLAM_S3O_UNROLL
        for (int c = k + 1; c < N; c++) {
            if (big == c) {
                SPSLAM_S3O_UNROLL
                for (int j = 0; j < k; j++) swapd(m[k][j], m[c][j]);
                SPSLAM_S3O_UNROLL
                for (int i = c + 1; i < N; i++) swapd(m[i][k], m[i][c]);
                swapd(m[k][k], m[c][c]);
                SPSLAM_S3O_UNROLL
                for (int i = k + 1; i < c; ++i) swapd(m[i][k], m[c][i]);
            }
        }
        if (k > 0) {
            double temp[N];
            SPSLAM_S3O_UNROLL
            for (int j = 0; j < k; j++) temp[j] = m[j][j] * m[k][j];
            double s = 0;
            SPSLAM_S3O_UNROLL
            for (int j = 0; j < k; j++) s += m[k][j] * temp[j];
            m[k][k] -= s;
            SPSLAM_S3O_UNROLL
            for (int i = k + 1; i < N; i++) {
                double t = 0;
                SPSLAM_S3O_UNROLL
                for (int j = 0; j < k; j++) t += m[i][j] * temp[j];
                m[i][k] -= t;
            }
        }
        const double akk = m[k][k];
        const bool valid = abs_(akk) > 0;
        if (k == 0 && !valid) return false;
        if (k + 1 < N && valid) {
            SPSLAM_S3O_UNROLL
            for (int i = k + 1; i < N; i++) m[i][k] /= akk;
        }
        if (sign == 1) { if (akk < 0) sign = 3; }
        else if (sign == 2) { if (akk > 0) sign = 3; }
        else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
    }
    if (!(sign == 1 || sign == 0)) return false;
    double y[N];
    SPSLAM_S3O_UNROLL
    for (int i = 0; i < N; i++) y[i] = b[i];
    SPSLAM_S3O_UNROLL
    for (int k = 0; k < N; k++) {
        SPSLAM_S3O_UNROLL
        for (int c = k + 1; c < N; c++)
            if (tr[k] == c) swapd(y[k], y[c]);
    }
    SPSLAM_S3O_UNROLL
    for (int i = 0; i < N; i++) {
        SPSLAM_S3O_UNROLL
        for (int j = 0; j < i; j++) y[i] -= m[i][j] * y[j];
    }
    SPSLAM_S3O_UNROLL
    for (int i = 0; i < N; i++) y[i] = abs_(m[i][i]) > 2.2250738585072014e-308 ? y[i] / m[i][i] : 0.0;
    SPSLAM_S3O_UNROLL
    for (int i = N - 1; i >= 0; i--) {
        SPSLAM_S3O_UNROLL
        for (int j = i + 1; j < N; j++) y[i] -= m[j][i] * y[j];
    }
    SPSLAM_S3O_UNROLL
    for (int k = N - 1; k >= 0; k--) {
        SPSLAM_S3O_UNROLL
        for (int c = k + 1; c < N; c++)
            if (tr[k] == c) swapd(y[k], y[c]);
    }
    SPSLAM_S3O_UNROLL
    for (int i = 0; i < N; i++) x[i] = y[i];
    return true;
}

// What one optimize() leaves behind for the check after it.
struct OptStats {
    int its, trials;
    S3 last;  // the estimate of the last computeActiveErrors: the edges' cached chi2 belong to it, accepted or not
};

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg on the one 7-dof vertex, as
// oracle/pose_oracle.cpp restates it for PoseOptimization.  Ops supplies the edge passes over the active edges in
// insertion order:
//   n_active()                  edges in the active set
//   linearize(S, &chi, H, b)    computeActiveErrors + activeRobustChi2 at S, then buildSystem: the 28 lower H terms
//                               and b, each chained edge by edge
//   robust_chi2(S, &chi)        computeActiveErrors + activeRobustChi2 at a trial estimate
// xs is the solver's x: kept over the trials and both optimize calls, written only by a successful solve (and its
// seventh entry by oplusImpl); a failed LDLT leaves the previous solution, which update() and computeScale() use.
// Every thread of a workgroup runs this with the same values; nothing but the Ops passes is divided among them.
template <class Ops>
SPSLAM_S3O_HD void optimize(Ops& ops, S3& S, int iterations, double* xs, OptStats* st) {
    st->its = 0;
    st->trials = 0;
    st->last = S;
    if (ops.n_active() == 0) return;  // "0 vertices to optimize": no iteration, no trial
    double lambda = -1, ni = 2;
    int n_bad = 0;
    for (int it = 0; it < iterations; it++) {
        double H[28], b[7], current_chi;
        ops.linearize(S, &current_chi, H, b);
        st->last = S;
        double temp_chi = current_chi;
        const double ini_chi = current_chi;
        if (it == 0) {  // computeLambdaInit
            double max_diag = 0;
            SPSLAM_S3O_UNROLL
            for (int j = 0; j < 7; j++) {
                const double d = abs_(H[j * (j + 1) / 2 + j]);
                max_diag = d < max_diag ? max_diag : d;  // std::max(fabs(h), maxDiagonal)
            }
            lambda = 1e-5 * max_diag;
            ni = 2;
            n_bad = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const S3 backup = S;
            double xn[7];
            const bool ok = ldlt_solve<7>(H, lambda, b, xn);
            st->trials++;
            if (ok) {
                SPSLAM_S3O_UNROLL
                for (int j = 0; j < 7; j++) xs[j] = xn[j];
            }
            int branch;
            S = sim3_oplus_fixed(S, xs, &branch);
            ops.note_update(branch);
            ops.robust_chi2(S, &temp_chi);
            st->last = S;
            if (!ok) temp_chi = 1.7976931348623157e308;
            rho = current_chi - temp_chi;
            double sc = 0;
            SPSLAM_S3O_UNROLL
            for (int j = 0; j < 7; j++) sc += xs[j] * (lambda * xs[j] + b[j]);
            sc += 1e-3;
            rho /= sc;
            const bool accepted = rho > 0 && finite_(temp_chi);
            if (accepted) {
                double alpha = 1. - libm64cr::cube_(2 * rho - 1);
                alpha = 2. / 3. < alpha ? 2. / 3. : alpha;                  // std::min(alpha, 2/3)
                const double sf = 1. / 3. < alpha ? alpha : 1. / 3.;         // std::max(1/3, alpha)
                lambda *= sf;
                ni = 2;
                current_chi = temp_chi;
            } else {
                lambda *= ni;
                ni *= 2;
                S = backup;
            }
            ops.note_trial(lambda, rho, accepted);
            qmax++;
        } while (rho < 0 && qmax < 10);
        st->its++;
        if (qmax == 10 || rho == 0) break;
        if ((ini_chi - current_chi) * 1e3 < ini_chi) n_bad++;
        else n_bad = 0;
        if (n_bad >= 3) break;
    }
}

// What OptimizeSim3 returns, before Scw.
struct Outcome {
    int n_in, n_corr, n_bad, too_few;
    int its[2], trials[2];
    S3 S12;
    S3 last[2];  // per optimize call, the estimate its check read the errors at (the host build's tests compare it)
};

// OptimizeSim3 after the gather (:2413-2473).  Ops adds
//   n_corr()                    nCorrespondences
//   check_first(last, th2)      :2419-2436 on the chi2 cached at `last`: nulls the matches, removes the pairs, nBad
//   check_final(last, th2)      :2453-2467: nulls the matches, returns nIn
template <class Ops>
SPSLAM_S3O_HD void optimize_sim3(Ops& ops, const S3& S0, double th2, Outcome* out) {
    S3 S = S0;
    double xs[7] = {0, 0, 0, 0, 0, 0, 0};
    OptStats st;
    out->n_corr = ops.n_corr();
    out->its[1] = out->trials[1] = 0;
    ops.note_optimize(0);
    optimize(ops, S, 5, xs, &st);
    out->its[0] = st.its;
    out->trials[0] = st.trials;
    out->last[0] = out->last[1] = st.last;
    const int n_bad = ops.check_first(st.last, th2);
    out->n_bad = n_bad;
    const int more = n_bad > 0 ? 10 : 5;
    if (out->n_corr - n_bad < 10) {  // return 0 after the match12 writes, g2oS12 untouched
        out->too_few = 1;
        out->n_in = 0;
        out->S12 = S0;
        return;
    }
    ops.note_optimize(1);
    optimize(ops, S, more, xs, &st);
    out->its[1] = st.its;
    out->trials[1] = st.trials;
    out->last[1] = st.last;
    out->too_few = 0;
    out->n_in = ops.check_final(st.last, th2);
    out->S12 = S;
}

// LoopClosing.cc:335-337 and Converter::toCvMat(g2o::Sim3): Scw = S12 * gSmw and mScw = [s*R | t] as floats
SPSLAM_S3O_HD void scw_of(const S3& S12, const float* Tcw2, double* Scw8, float* mScw) {
    const S3 Smw = sim3_from_float(Tcw2, 4, Tcw2[3], Tcw2[7], Tcw2[11], 1.0);
    const S3 Scw = sim3_mul(S12, Smw);
    Scw8[0] = Scw.r.x; Scw8[1] = Scw.r.y; Scw8[2] = Scw.r.z; Scw8[3] = Scw.r.w;
    Scw8[4] = Scw.t.x; Scw8[5] = Scw.t.y; Scw8[6] = Scw.t.z; Scw8[7] = Scw.s;
    double R[9];
    q_to_rot(Scw.r, R);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) mScw[4 * r + c] = (float)(Scw.s * R[3 * r + c]);
    mScw[3] = (float)Scw.t.x; mScw[7] = (float)Scw.t.y; mScw[11] = (float)Scw.t.z;
    mScw[12] = mScw[13] = mScw[14] = 0.f;
    mScw[15] = 1.f;
}

}  // namespace sim3opt
}  // namespace spslam
