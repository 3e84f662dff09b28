// Referee of the OptimizeSim3 tests: a literal, sequential restatement of Optimizer::OptimizeSim3
// (src/Optimizer.cc:2279-2474) on the g2o pieces it runs, written from the reference and not from the kernels'
// header (sp-slam_amd/csrc/sim3_opt_math.h):
//   g2o::Sim3                                   Thirdparty/g2o/g2o/types/sim3.h
//   VertexSim3Expmap, EdgeSim3ProjectXYZ,
//   EdgeInverseSim3ProjectXYZ                   types/types_seven_dof_expmap.h
//   BaseVertex push / pop / discardTop          core/base_vertex.h
//   BaseBinaryEdge linearizeOplus (numeric),
//   constructQuadraticForm (robust branch)      core/base_binary_edge.hpp:55-205
//   RobustKernelHuber                           core/robust_kernel_impl.cpp
//   SparseOptimizer optimize / removeEdge,
//   OptimizationAlgorithmLevenberg::solve       as oracle/pose_oracle.cpp restates them
//   LinearSolverDense                           Eigen::LDLT<MatrixXd>, as oracle/pose_oracle.cpp restates it
// with a vertex that keeps an estimate stack, edge objects that cache their error, a per-edge, per-column oplus for
// the Jacobian and an edge list that removeEdge shrinks.  sin / cos / x^3 are oracle/libm_cr_oracle.h's correctly
// rounded ones.  Fixed scale only.  Build: g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC ... -lquadmath.
// It keeps a trace (see sim3_opt_ref_run) that tests/test_sim3_opt_host.py reads.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../oracle/libm_cr_oracle.h"

namespace {

namespace cr = oracle::libm_cr;

struct Vec3 {
    double v[3];
    double& operator[](int i) { return v[i]; }
    double operator[](int i) const { return v[i]; }
};
struct Mat3 {
    double m[3][3];
};
struct Quat {
    double x, y, z, w;
};

Vec3 vcross(const Vec3& a, const Vec3& b) {
    return Vec3{{a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]}};
}
Vec3 vadd(const Vec3& a, const Vec3& b) { return Vec3{{a[0] + b[0], a[1] + b[1], a[2] + b[2]}}; }
Vec3 vscale(double s, const Vec3& a) { return Vec3{{s * a[0], s * a[1], s * a[2]}}; }

// Eigen: Quaterniond(Matrix3d) (Geometry/Quaternion.h, quaternionbase_assign_impl<Other,3,3>)
Quat quat_of(const Mat3& M) {
    Quat q;
    double t = M.m[0][0] + M.m[1][1] + M.m[2][2];
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q.w = 0.5 * t;
        t = 0.5 / t;
        q.x = (M.m[2][1] - M.m[1][2]) * t;
        q.y = (M.m[0][2] - M.m[2][0]) * t;
        q.z = (M.m[1][0] - M.m[0][1]) * t;
    } else {
        int i = 0;
        if (M.m[1][1] > M.m[0][0]) i = 1;
        if (M.m[2][2] > M.m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(M.m[i][i] - M.m[j][j] - M.m[k][k] + 1.0);
        double c[3];
        c[i] = 0.5 * t;
        t = 0.5 / t;
        q.w = (M.m[k][j] - M.m[j][k]) * t;
        c[j] = (M.m[j][i] + M.m[i][j]) * t;
        c[k] = (M.m[k][i] + M.m[i][k]) * t;
        q.x = c[0]; q.y = c[1]; q.z = c[2];
    }
    return q;
}
// Eigen: QuaternionBase::toRotationMatrix
Mat3 matrix_of(const Quat& q) {
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    Mat3 R;
    R.m[0][0] = 1 - (tyy + tzz); R.m[0][1] = txy - twz; R.m[0][2] = txz + twy;
    R.m[1][0] = txy + twz; R.m[1][1] = 1 - (txx + tzz); R.m[1][2] = tyz - twx;
    R.m[2][0] = txz - twy; R.m[2][1] = tyz + twx; R.m[2][2] = 1 - (txx + tyy);
    return R;
}
// Eigen: quat_product<double>
Quat qprod(const Quat& a, const Quat& b) {
    Quat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}
// Eigen: QuaternionBase::_transformVector
Vec3 qrotate(const Quat& q, const Vec3& v) {
    const Vec3 qv{{q.x, q.y, q.z}};
    Vec3 uv = vcross(qv, v);
    uv = vadd(uv, uv);
    return vadd(vadd(v, vscale(q.w, uv)), vcross(qv, uv));
}

thread_local int g_branch = -1;  // which eps branch the last Sim3(update) took

struct Sim3 {
    Quat r{0, 0, 0, 1};
    Vec3 t{{0, 0, 0}};
    double s = 1.;
    Sim3() {}
    Sim3(const Quat& r_, const Vec3& t_, double s_) : r(r_), t(t_), s(s_) {}
    Sim3(const Mat3& R, const Vec3& t_, double s_) : r(quat_of(R)), t(t_), s(s_) {}
    // sim3.h:70-142.  exp(sigma): under fixed scale sigma is exactly 0 here and exp(0) = 1
    explicit Sim3(const double* update) {
        Vec3 omega, upsilon;
        for (int i = 0; i < 3; i++) omega[i] = update[i];
        for (int i = 0; i < 3; i++) upsilon[i] = update[i + 3];
        const double sigma = update[6];
        const double theta = std::sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]);
        Mat3 Omega{{{0, -omega[2], omega[1]}, {omega[2], 0, -omega[0]}, {-omega[1], omega[0], 0}}};
        s = sigma == 0.0 ? 1.0 : std::exp(sigma);
        Mat3 Omega2;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                Omega2.m[i][j] = Omega.m[i][0] * Omega.m[0][j] + Omega.m[i][1] * Omega.m[1][j] + Omega.m[i][2] * Omega.m[2][j];
        Mat3 I{{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}}, R;
        const double eps = 0.00001;
        double A, B, C;
        if (std::fabs(sigma) < eps) {
            C = 1;
            if (theta < eps) {
                A = 1. / 2.;
                B = 1. / 6.;
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) R.m[i][j] = (I.m[i][j] + Omega.m[i][j]) + Omega2.m[i][j];
                g_branch = 0;
            } else {
                const double theta2 = theta * theta;
                A = (1 - cr::cos(theta)) / (theta2);
                B = (theta - cr::sin(theta)) / (theta2 * theta);
                const double a = cr::sin(theta) / theta, b = (1 - cr::cos(theta)) / (theta * theta);
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) R.m[i][j] = (I.m[i][j] + a * Omega.m[i][j]) + b * Omega2.m[i][j];
                g_branch = 1;
            }
        } else {
            C = (s - 1) / sigma;
            if (theta < eps) {
                const double sigma2 = sigma * sigma;
                A = ((sigma - 1) * s + 1) / sigma2;
                B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) R.m[i][j] = (I.m[i][j] + Omega.m[i][j]) + Omega2.m[i][j];
                g_branch = 2;
            } else {
                const double sa = cr::sin(theta) / theta, sb = (1 - cr::cos(theta)) / (theta * theta);
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) R.m[i][j] = (I.m[i][j] + sa * Omega.m[i][j]) + sb * Omega2.m[i][j];
                const double a = s * cr::sin(theta), b = s * cr::cos(theta);
                const double theta2 = theta * theta, sigma2 = sigma * sigma;
                const double c = theta2 + sigma2;
                A = (a * sigma + (1 - b) * theta) / (theta * c);
                B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
                g_branch = 3;
            }
        }
        r = quat_of(R);
        Mat3 W;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) W.m[i][j] = (A * Omega.m[i][j] + B * Omega2.m[i][j]) + C * I.m[i][j];
        for (int i = 0; i < 3; i++) t[i] = W.m[i][0] * upsilon[0] + W.m[i][1] * upsilon[1] + W.m[i][2] * upsilon[2];
    }
    Vec3 map(const Vec3& xyz) const { return vadd(vscale(s, qrotate(r, xyz)), t); }
    Sim3 inverse() const {
        const Quat c{-r.x, -r.y, -r.z, r.w};
        return Sim3(c, qrotate(c, vscale(-1. / s, t)), 1. / s);
    }
    Sim3 operator*(const Sim3& o) const {
        Sim3 ret;
        ret.r = qprod(r, o.r);
        ret.t = vadd(vscale(s, qrotate(r, o.t)), t);
        ret.s = s * o.s;
        return ret;
    }
};

struct VertexSim3Expmap {
    Sim3 estimate;
    std::vector<Sim3> backups;
    bool fix_scale = true;
    double pp1[2], fl1[2], pp2[2], fl2[2];
    double hessian[7][7], b[7];
    void push() { backups.push_back(estimate); }
    void pop() { estimate = backups.back(); backups.pop_back(); }
    void discardTop() { backups.pop_back(); }
    void oplus(double* update) {
        if (fix_scale) update[6] = 0;
        Sim3 s(update);
        estimate = s * estimate;
    }
    void cam_map1(const double* v, double* res) const { res[0] = v[0] * fl1[0] + pp1[0]; res[1] = v[1] * fl1[1] + pp1[1]; }
    void cam_map2(const double* v, double* res) const { res[0] = v[0] * fl2[0] + pp2[0]; res[1] = v[1] * fl2[1] + pp2[1]; }
};

struct VertexPoint { Vec3 estimate; };

struct Edge {
    bool inverse;  // EdgeInverseSim3ProjectXYZ
    VertexPoint* point;
    VertexSim3Expmap* v1;
    double measurement[2];
    double information[2][2];
    double huber_delta;
    double error[2] = {0, 0};
    double J[2][7];
    int pair;  // index into vpEdges12 / vpEdges21

    void computeError() {
        double proj[2], mapped[2];
        const Vec3 p = inverse ? v1->estimate.inverse().map(point->estimate) : v1->estimate.map(point->estimate);
        proj[0] = p[0] / p[2];
        proj[1] = p[1] / p[2];
        if (inverse) v1->cam_map2(proj, mapped); else v1->cam_map1(proj, mapped);
        error[0] = measurement[0] - mapped[0];
        error[1] = measurement[1] - mapped[1];
    }
    void omega_error(double* out) const {  // information * error, a 2x2 times a 2x1
        out[0] = information[0][0] * error[0] + information[0][1] * error[1];
        out[1] = information[1][0] * error[0] + information[1][1] * error[1];
    }
    double chi2() const {
        double oe[2];
        omega_error(oe);
        return error[0] * oe[0] + error[1] * oe[1];
    }
    void robustify(double e, double* rho) const {
        const double dsqr = huber_delta * huber_delta;
        if (e <= dsqr) {
            rho[0] = e; rho[1] = 1.; rho[2] = 0.;
        } else {
            const double sqrte = std::sqrt(e);
            rho[0] = 2 * sqrte * huber_delta - dsqr;
            rho[1] = huber_delta / sqrte;
            rho[2] = -0.5 * rho[1] / e;
        }
    }
    // base_binary_edge.hpp:131-205, the free vertex (vertex 1) only: the point is fixed
    void linearizeOplus() {
        const double delta = 1e-9;
        const double scalar = 1.0 / (2 * delta);
        double errorBak[2];
        const double errorBeforeNumeric[2] = {error[0], error[1]};
        double add_vj[7];
        std::fill(add_vj, add_vj + 7, 0.0);
        for (int d = 0; d < 7; ++d) {
            v1->push();
            add_vj[d] = delta;
            v1->oplus(add_vj);
            computeError();
            errorBak[0] = error[0]; errorBak[1] = error[1];
            v1->pop();
            v1->push();
            add_vj[d] = -delta;
            v1->oplus(add_vj);
            computeError();
            errorBak[0] -= error[0]; errorBak[1] -= error[1];
            v1->pop();
            add_vj[d] = 0.0;
            J[0][d] = scalar * errorBak[0];
            J[1][d] = scalar * errorBak[1];
        }
        error[0] = errorBeforeNumeric[0]; error[1] = errorBeforeNumeric[1];
    }
    // base_binary_edge.hpp:91-113 for `to`
    void constructQuadraticForm() {
        double omega_r[2];
        omega_error(omega_r);
        omega_r[0] = -omega_r[0]; omega_r[1] = -omega_r[1];
        const double e = chi2();
        double rho[3];
        robustify(e, rho);
        double weightedOmega[2][2];
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < 2; j++) weightedOmega[i][j] = rho[1] * information[i][j];
        omega_r[0] *= rho[1]; omega_r[1] *= rho[1];
        for (int i = 0; i < 7; i++) v1->b[i] += J[0][i] * omega_r[0] + J[1][i] * omega_r[1];
        double BtW[7][2];  // B.transpose() * weightedOmega
        for (int i = 0; i < 7; i++)
            for (int k = 0; k < 2; k++) BtW[i][k] = J[0][i] * weightedOmega[0][k] + J[1][i] * weightedOmega[1][k];
        for (int i = 0; i < 7; i++)
            for (int j = 0; j < 7; j++) v1->hessian[i][j] += BtW[i][0] * J[0][j] + BtW[i][1] * J[1][j];
    }
};

// Eigen::LDLT<MatrixXd> compute + solve on the lower triangle, and isPositive, as oracle/pose_oracle.cpp restates it
bool ldlt_solve(int n, const double* A, const double* b, double* x) {
    std::vector<double> mm(A, A + n * n), temp(n), y(b, b + n);
    auto m = [&](int i, int j) -> double& { return mm[i * n + j]; };
    std::vector<int> tr(n);
    int sign = 0;
    for (int k = 0; k < n; ++k) {
        int big = k;
        double bv = std::fabs(m(k, k));
        for (int i = k + 1; i < n; i++)
            if (std::fabs(m(i, i)) > bv) { bv = std::fabs(m(i, i)); big = i; }
        tr[k] = big;
        if (k != big) {
            for (int j = 0; j < k; j++) std::swap(m(k, j), m(big, j));
            for (int i = big + 1; i < n; i++) std::swap(m(i, k), m(i, big));
            std::swap(m(k, k), m(big, big));
            for (int i = k + 1; i < big; ++i) std::swap(m(i, k), m(big, i));
        }
        if (k > 0) {
            for (int j = 0; j < k; j++) temp[j] = m(j, j) * m(k, j);
            double s = 0;
            for (int j = 0; j < k; j++) s += m(k, j) * temp[j];
            m(k, k) -= s;
            for (int i = k + 1; i < n; i++) {
                double t = 0;
                for (int j = 0; j < k; j++) t += m(i, j) * temp[j];
                m(i, k) -= t;
            }
        }
        const double akk = m(k, k);
        const bool valid = std::fabs(akk) > 0;
        if (k == 0 && !valid) return false;
        if (n - k - 1 > 0 && valid)
            for (int i = k + 1; i < n; i++) m(i, k) /= akk;
        if (sign == 1) { if (akk < 0) sign = 3; }
        else if (sign == 2) { if (akk > 0) sign = 3; }
        else if (sign == 0) { if (akk > 0) sign = 1; else if (akk < 0) sign = 2; }
    }
    if (!(sign == 1 || sign == 0)) return false;
    for (int k = 0; k < n; k++) std::swap(y[k], y[tr[k]]);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < i; j++) y[i] -= m(i, j) * y[j];
    for (int i = 0; i < n; i++) y[i] = std::fabs(m(i, i)) > DBL_MIN ? y[i] / m(i, i) : 0.0;
    for (int i = n - 1; i >= 0; i--)
        for (int j = i + 1; j < n; j++) y[i] -= m(j, i) * y[j];
    for (int k = n - 1; k >= 0; k--) std::swap(y[k], y[tr[k]]);
    std::copy(y.begin(), y.end(), x);
    return true;
}

struct Trace {
    double* trials;  // 8 per trial: optimize call, iteration, trial, lambda after, rho, accepted, Sim3(update) branch, solve ok
    int max_trials;
    double* lin;     // 10 per linearisation: optimize call, iteration, the estimate x y z w t s
    int max_lin;
    int n_trials = 0, n_lin = 0;
    bool last_errors_rejected = false;  // the cached errors belong to a trial that was rejected
};

struct Optimizer {
    VertexSim3Expmap* v = nullptr;
    std::vector<Edge*> edges;   // the graph's edges in insertion order
    std::vector<Edge*> active;  // initializeOptimization
    double x[7] = {0, 0, 0, 0, 0, 0, 0};  // the solver's x
    Trace* tr = nullptr;
    int its = 0, trials = 0;

    void removeEdge(Edge* e) { edges.erase(std::find(edges.begin(), edges.end(), e)); }
    void initializeOptimization() { active = edges; }
    Sim3 errors_at;  // the estimate the cached errors were computed at
    void computeActiveErrors() {
        for (Edge* e : active) e->computeError();
        errors_at = v->estimate;
    }
    double activeRobustChi2() const {
        double chi = 0.0;
        for (const Edge* e : active) {
            double rho[3];
            e->robustify(e->chi2(), rho);
            chi += rho[0];
        }
        return chi;
    }
    // optimize(iterations) with OptimizationAlgorithmLevenberg and the stop rule of the vendored g2o
    void optimize(int call, int iterations) {
        its = trials = 0;
        if (active.empty()) return;  // "0 vertices to optimize"
        double lambda = -1, ni = 2;
        int nBad = 0;
        for (int it = 0; it < iterations; it++) {
            computeActiveErrors();
            tr->last_errors_rejected = false;
            double currentChi = activeRobustChi2(), tempChi = currentChi;
            const double iniChi = currentChi;
            // buildSystem
            std::memset(v->hessian, 0, sizeof v->hessian);
            std::memset(v->b, 0, sizeof v->b);
            if (tr->n_lin < tr->max_lin) {
                double* L = tr->lin + 10 * tr->n_lin++;
                const Sim3& S = v->estimate;
                const double rec[10] = {(double)call, (double)it, S.r.x, S.r.y, S.r.z, S.r.w, S.t[0], S.t[1], S.t[2], S.s};
                std::copy(rec, rec + 10, L);
            }
            for (Edge* e : active) {
                e->linearizeOplus();
                e->constructQuadraticForm();
            }
            if (it == 0) {  // computeLambdaInit
                double maxDiagonal = 0;
                for (int j = 0; j < 7; j++) maxDiagonal = std::max(std::fabs(v->hessian[j][j]), maxDiagonal);
                lambda = 1e-5 * maxDiagonal;
                ni = 2;
                nBad = 0;
            }
            double rho = 0;
            int qmax = 0;
            do {
                v->push();
                double Hl[49];
                for (int i = 0; i < 7; i++)
                    for (int j = 0; j < 7; j++) Hl[7 * i + j] = v->hessian[i][j];
                for (int i = 0; i < 7; i++) Hl[8 * i] += lambda;  // setLambda; restoreDiagonal puts the backup back
                double xn[7];
                const bool ok2 = ldlt_solve(7, Hl, v->b, xn);
                trials++;
                if (ok2) std::copy(xn, xn + 7, x);
                v->oplus(x);  // update(): writes x[6] = 0 under fixed scale
                const int branch = g_branch;
                computeActiveErrors();
                tempChi = activeRobustChi2();
                if (!ok2) tempChi = std::numeric_limits<double>::max();
                rho = currentChi - tempChi;
                double scale = 0;
                for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + v->b[j]);
                scale += 1e-3;
                rho /= scale;
                const bool accepted = rho > 0 && std::isfinite(tempChi);
                if (accepted) {
                    double alpha = 1. - cr::cube(2 * rho - 1);
                    alpha = std::min(alpha, 2. / 3.);
                    const double scaleFactor = std::max(1. / 3., alpha);
                    lambda *= scaleFactor;
                    ni = 2;
                    currentChi = tempChi;
                    v->discardTop();
                } else {
                    lambda *= ni;
                    ni *= 2;
                    v->pop();
                }
                tr->last_errors_rejected = !accepted;
                if (tr->n_trials < tr->max_trials) {
                    double* T = tr->trials + 8 * tr->n_trials++;
                    const double rec[8] = {(double)call, (double)it, (double)qmax, lambda, rho, accepted ? 1. : 0.,
                                           (double)branch, ok2 ? 1. : 0.};
                    std::copy(rec, rec + 8, T);
                }
                qmax++;
            } while (rho < 0 && qmax < 10);
            its++;
            if (qmax == 10 || rho == 0) break;
            if ((iniChi - currentChi) * 1e3 < iniChi) nBad++;
            else nBad = 0;
            if (nBad >= 3) break;
        }
    }
};

// chi2 of an edge re-evaluated at the vertex's current estimate; the cached error stays as it is
double chi2_at_estimate(const Edge* e) {
    Edge copy = *e;
    copy.computeError();
    return copy.chi2();
}

#pragma pack(push, 1)
struct KeyPoint { float x, y, size, angle, response; int32_t octave, class_id; };
#pragma pack(pop)
static_assert(sizeof(KeyPoint) == 28, "cv::KeyPoint");

struct Result {
    int32_t n_in, n_corr, n_bad, status, accepted, iterations1, trials1, iterations2, trials2, pad;
    double S12[8], Scw[8];
    float mScw[16];
};
static_assert(sizeof(Result) == 232, "spslam_sim3_opt_result");

// cv::Mat (3x3 float) * (3x1 float) + (3x1 float): each row summed in double, the addend added, rounded once
// (the readings of the matcher family)
void camera_point(const float* Tcw, const float* xw, float* out) {
    for (int r = 0; r < 3; r++) {
        double s = 0.0;
        for (int k = 0; k < 3; k++) s = s + (double)Tcw[4 * r + k] * (double)xw[k];
        s = s + (double)Tcw[4 * r + 3];
        out[r] = (float)s;
    }
}

Mat3 rotation_of(const float* R, int ld) {
    Mat3 M;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M.m[i][j] = R[ld * i + j];
    return M;
}

void put(const Sim3& S, double* o) {
    o[0] = S.r.x; o[1] = S.r.y; o[2] = S.r.z; o[3] = S.r.w;
    o[4] = S.t[0]; o[5] = S.t[1]; o[6] = S.t[2]; o[7] = S.s;
}

}  // namespace

extern "C" {

// One OptimizeSim3 and the Scw after it.  cam: fx fy cx cy (K1 = K2, floats); inv_sigma2: mvInvLevelSigma2, 8 floats;
// a keyframe is (Tcw 16 floats, n cv::KeyPoint, n rows into the point table or -1); xw: 3 floats per table row;
// bad: one byte per row or NULL; pair: s12, R12 (9), t12 (3) as 13 floats.  match12 is vpMatches1, rewritten.
// Trace: trials / lin as struct Trace says, counts[0..1] = their numbers; chi_first / chi_final: per kept
// correspondence (e12 chi2, e21 chi2) as the check read them, -1 where the pair was no longer in the graph;
// kept: the kept keypoints i; flags[0] / flags[1]: the first / final check read errors cached by a rejected trial;
// chi_*_at_estimate: the same pairs' chi2 had the check evaluated them at the vertex's estimate instead; errors_at:
// per optimize call the estimate (x y z w t s) of the last computeActiveErrors, 16 doubles.
int sim3_opt_ref_run(const float* cam, const float* inv_sigma2, const float* Tcw1, const KeyPoint* kun1, const int32_t* rows1,
                     int n1, const float* Tcw2, const KeyPoint* kun2, const int32_t* rows2, int n2, const float* xw,
                     const uint8_t* bad, const float* pair, float th2, int min_inliers, int32_t* match12, Result* out,
                     double* trials, int max_trials, double* lin, int max_lin, int32_t* counts, double* chi_first,
                     double* chi_final, int32_t* kept, int32_t* flags, double* chi_first_at_estimate,
                     double* chi_final_at_estimate, double* errors_at) {
    Optimizer optimizer;
    Trace tr{trials, max_trials, lin, max_lin};
    optimizer.tr = &tr;
    VertexSim3Expmap vSim3;
    vSim3.fix_scale = true;
    Sim3 g2oS12(rotation_of(pair + 1, 3), Vec3{{pair[10], pair[11], pair[12]}}, (double)pair[0]);
    vSim3.estimate = g2oS12;
    vSim3.pp1[0] = cam[2]; vSim3.pp1[1] = cam[3]; vSim3.fl1[0] = cam[0]; vSim3.fl1[1] = cam[1];
    vSim3.pp2[0] = cam[2]; vSim3.pp2[1] = cam[3]; vSim3.fl2[0] = cam[0]; vSim3.fl2[1] = cam[1];
    optimizer.v = &vSim3;
    const int N = n1;
    std::vector<VertexPoint> points1(N), points2(N);
    std::vector<Edge> store12(N), store21(N);
    std::vector<Edge*> vpEdges12, vpEdges21;
    std::vector<size_t> vnIndexEdge;
    const float deltaHuber = std::sqrt(th2);
    int nCorrespondences = 0;
    for (int i = 0; i < N; i++) {
        const int i2 = match12[i];
        if (i2 < 0 || i2 >= n2) continue;      // !vpMatches1[i]
        const int r1 = rows1[i], r2 = rows2[i2];
        if (r1 < 0 || r2 < 0) continue;        // pMP1 && pMP2 (pMP2's index in KF2 is i2: the contract)
        if (bad && (bad[r1] || bad[r2])) continue;
        float P1[3], P2[3];
        camera_point(Tcw1, xw + 3 * r1, P1);
        camera_point(Tcw2, xw + 3 * r2, P2);
        points1[i].estimate = Vec3{{P1[0], P1[1], P1[2]}};
        points2[i].estimate = Vec3{{P2[0], P2[1], P2[2]}};
        nCorrespondences++;
        const int o1 = kun1[i].octave, o2 = kun2[i2].octave;
        const float invSigmaSquare1 = inv_sigma2[o1 >= 1 && o1 < 8 ? o1 : 0];
        const float invSigmaSquare2 = inv_sigma2[o2 >= 1 && o2 < 8 ? o2 : 0];
        Edge& e12 = store12[i];
        e12.inverse = false; e12.point = &points2[i]; e12.v1 = &vSim3;
        e12.measurement[0] = kun1[i].x; e12.measurement[1] = kun1[i].y;
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++) e12.information[a][b] = (a == b ? 1.0 : 0.0) * invSigmaSquare1;
        e12.huber_delta = deltaHuber;
        e12.pair = (int)vpEdges12.size();
        optimizer.edges.push_back(&e12);
        Edge& e21 = store21[i];
        e21.inverse = true; e21.point = &points1[i]; e21.v1 = &vSim3;
        e21.measurement[0] = kun2[i2].x; e21.measurement[1] = kun2[i2].y;
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++) e21.information[a][b] = (a == b ? 1.0 : 0.0) * invSigmaSquare2;
        e21.huber_delta = deltaHuber;
        e21.pair = (int)vpEdges21.size();
        optimizer.edges.push_back(&e21);
        vpEdges12.push_back(&e12);
        vpEdges21.push_back(&e21);
        vnIndexEdge.push_back(i);
        kept[vnIndexEdge.size() - 1] = i;
    }
    std::memset(out, 0, sizeof *out);
    out->n_corr = nCorrespondences;

    optimizer.initializeOptimization();
    optimizer.optimize(0, 5);
    out->iterations1 = optimizer.its;
    out->trials1 = optimizer.trials;
    if (nCorrespondences == 0) optimizer.errors_at = vSim3.estimate;  // nothing was evaluated
    put(optimizer.errors_at, errors_at);
    put(optimizer.errors_at, errors_at + 8);
    flags[0] = tr.last_errors_rejected ? 1 : 0;
    flags[1] = 0;

    int nBad = 0;
    for (size_t i = 0; i < vpEdges12.size(); i++) {
        Edge* e12 = vpEdges12[i];
        Edge* e21 = vpEdges21[i];
        chi_final[2 * i] = chi_final[2 * i + 1] = -1;
        if (!e12 || !e21) continue;
        chi_first[2 * i] = e12->chi2();
        chi_first[2 * i + 1] = e21->chi2();
        chi_first_at_estimate[2 * i] = chi2_at_estimate(e12);
        chi_first_at_estimate[2 * i + 1] = chi2_at_estimate(e21);
        if (e12->chi2() > th2 || e21->chi2() > th2) {
            const size_t idx = vnIndexEdge[i];
            match12[idx] = -1;
            optimizer.removeEdge(e12);
            optimizer.removeEdge(e21);
            vpEdges12[i] = nullptr;
            vpEdges21[i] = nullptr;
            nBad++;
        }
    }
    out->n_bad = nBad;
    const int nMoreIterations = nBad > 0 ? 10 : 5;
    int nIn = 0;
    bool returned_early = false;
    if (nCorrespondences - nBad < 10) {
        returned_early = true;  // return 0: g2oS12 is not written
    } else {
        optimizer.initializeOptimization();
        optimizer.optimize(1, nMoreIterations);
        out->iterations2 = optimizer.its;
        out->trials2 = optimizer.trials;
        put(optimizer.errors_at, errors_at + 8);
        flags[1] = tr.last_errors_rejected ? 1 : 0;
        for (size_t i = 0; i < vpEdges12.size(); i++) {
            Edge* e12 = vpEdges12[i];
            Edge* e21 = vpEdges21[i];
            if (!e12 || !e21) continue;
            chi_final[2 * i] = e12->chi2();
            chi_final[2 * i + 1] = e21->chi2();
            chi_final_at_estimate[2 * i] = chi2_at_estimate(e12);
            chi_final_at_estimate[2 * i + 1] = chi2_at_estimate(e21);
            if (e12->chi2() > th2 || e21->chi2() > th2) {
                const size_t idx = vnIndexEdge[i];
                match12[idx] = -1;
            } else
                nIn++;
        }
        g2oS12 = vSim3.estimate;
    }
    out->n_in = returned_early ? 0 : nIn;
    out->status = returned_early ? 1 : 0;
    out->accepted = out->n_in >= min_inliers ? 1 : 0;
    put(g2oS12, out->S12);
    // LoopClosing.cc:335-337 and Converter::toCvMat(const g2o::Sim3&)
    const Sim3 gSmw(rotation_of(Tcw2, 4), Vec3{{Tcw2[3], Tcw2[7], Tcw2[11]}}, 1.0);
    const Sim3 Scw = g2oS12 * gSmw;
    put(Scw, out->Scw);
    const Mat3 eigR = matrix_of(Scw.r);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out->mScw[4 * i + j] = (float)(Scw.s * eigR.m[i][j]);
        out->mScw[4 * i + 3] = (float)Scw.t[i];
    }
    out->mScw[15] = 1.f;
    counts[0] = tr.n_trials;
    counts[1] = tr.n_lin;
    return out->n_in;
}

// The referee's numeric Jacobian (linearizeOplus on edge objects) of n edges at the estimate S (x y z w t s):
// X 3 per edge, kinds 0 = EdgeSim3ProjectXYZ, 1 = EdgeInverseSim3ProjectXYZ.  J: 14 per edge (row-major 2x7);
// depth: the z the projection divided by.
void sim3_opt_ref_jacobians(const double* S, const float* cam, int n, const double* X, const int32_t* kinds, double* J,
                            double* depth) {
    VertexSim3Expmap v;
    v.estimate = Sim3(Quat{S[0], S[1], S[2], S[3]}, Vec3{{S[4], S[5], S[6]}}, S[7]);
    v.pp1[0] = v.pp2[0] = cam[2]; v.pp1[1] = v.pp2[1] = cam[3];
    v.fl1[0] = v.fl2[0] = cam[0]; v.fl1[1] = v.fl2[1] = cam[1];
    for (int k = 0; k < n; k++) {
        VertexPoint p{Vec3{{X[3 * k], X[3 * k + 1], X[3 * k + 2]}}};
        Edge e;
        e.inverse = kinds[k] != 0; e.point = &p; e.v1 = &v;
        e.measurement[0] = e.measurement[1] = 0;
        e.computeError();
        e.linearizeOplus();
        for (int r = 0; r < 2; r++)
            for (int d = 0; d < 7; d++) J[14 * k + 7 * r + d] = e.J[r][d];
        depth[k] = (e.inverse ? v.estimate.inverse().map(p.estimate) : v.estimate.map(p.estimate))[2];
    }
}

}
