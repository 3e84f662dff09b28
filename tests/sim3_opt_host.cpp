// Host build of the OptimizeSim3 kernel's arithmetic and driver (sp-slam_amd/csrc/sim3_opt_math.h) behind a C ABI,
// compiled by tests/test_sim3_opt_host.py with g++ -O2 -ffp-contract=off and held against tests/sim3_opt_ref.cpp bit
// for bit.  The edge passes are the kernel's, run by one thread: the same gather, the 14 shared perturbed estimates,
// the chains in insertion order with removed pairs skipped, the checks at the estimate of the last error evaluation.
#include <cmath>
#include <cstring>
#include <vector>

#include "../sp-slam_amd/csrc/sim3_opt_math.h"

using namespace spslam::sim3opt;

namespace {

#pragma pack(push, 1)
struct KeyPoint { float x, y, size, angle, response; int32_t octave, class_id; };
#pragma pack(pop)

struct Result {
    int32_t n_in, n_corr, n_bad, status, accepted, iterations1, trials1, iterations2, trials2, pad;
    double S12[8], Scw[8];
    float mScw[16];
};
static_assert(sizeof(Result) == 232, "spslam_sim3_opt_result");

struct HostOps {
    std::vector<Corr> C;
    int32_t* match12;
    Cam cam;
    double delta;
    int n_removed = 0;
    double* trials;  // 5 per trial: optimize call, lambda after, rho, accepted, Sim3(update) branch
    int max_trials, n_trials = 0, call = 0, branch = -1;

    int n_corr() const { return (int)C.size(); }
    int n_active() const { return 2 * ((int)C.size() - n_removed); }
    void note_optimize(int c) { call = c; }
    void note_update(int b) { branch = b; }
    void note_trial(double lambda, double rho, bool accepted) {
        if (n_trials < max_trials) {
            const double rec[5] = {(double)call, lambda, rho, accepted ? 1. : 0., (double)branch};
            std::memcpy(trials + 5 * n_trials++, rec, sizeof rec);
        }
    }
    void linearize(const S3& S, double* chi, double* H, double* b) {
        S3 P[2][14];
        for (int k = 0; k < 14; k++) {
            P[0][k] = perturbed(S, k);
            P[1][k] = sim3_inverse(P[0][k]);
        }
        const S3 Sinv = sim3_inverse(S);
        double acc[kTerms];
        for (double& a : acc) a = 0.0;
        for (const Corr& c : C) {
            if (c.removed) continue;
            for (int kind = 0; kind < 2; kind++) {
                double out[kTerms];
                edge_terms(kind ? Sinv : S, P[kind], kind ? c.X1 : c.X2, kind ? c.o2 : c.o1, kind ? c.w2 : c.w1, cam, delta,
                           out);
                for (int k = 0; k < kTerms; k++) acc[k] += out[k];
            }
        }
        *chi = acc[0];
        for (int k = 0; k < 28; k++) H[k] = acc[1 + k];
        for (int k = 0; k < 7; k++) b[k] = acc[29 + k];
    }
    void robust_chi2(const S3& S, double* chi) {
        const S3 Sinv = sim3_inverse(S);
        double acc = 0.0;
        for (const Corr& c : C) {
            if (c.removed) continue;
            acc += edge_robust_chi2(S, c.X2, c.o1, c.w1, cam, delta);
            acc += edge_robust_chi2(Sinv, c.X1, c.o2, c.w2, cam, delta);
        }
        *chi = acc;
    }
    int check(const S3& last, double th2, bool first) {
        const S3 Sinv = sim3_inverse(last);
        int count = 0;
        for (Corr& c : C) {
            if (c.removed) continue;
            double e[2];
            edge_error(last, c.X2, c.o1, cam, e);
            const double c12 = edge_chi2(c.w1, e);
            edge_error(Sinv, c.X1, c.o2, cam, e);
            const double c21 = edge_chi2(c.w2, e);
            const bool bad = c12 > th2 || c21 > th2;
            if (bad) {
                match12[c.i] = -1;
                if (first) c.removed = 1;
            }
            if (bad == first) count++;
        }
        return count;
    }
    int check_first(const S3& last, double th2) { return n_removed = check(last, th2, true); }
    int check_final(const S3& last, double th2) { return check(last, th2, false); }
};

}  // namespace

extern "C" {

// The arguments of sim3_opt_ref_run up to the result; trials as HostOps says, *n_trials their number; errors_at: per
// optimize call the estimate (x y z w t s) at which its check evaluates the edges.
int sim3_opt_host_run(const float* cam, const float* inv_sigma2, const float* Tcw1, const KeyPoint* kun1, const int32_t* rows1,
                      int n1, const float* Tcw2, const KeyPoint* kun2, const int32_t* rows2, int n2, const float* xw,
                      const uint8_t* bad, const float* pair, float th2, int min_inliers, int32_t* match12, Result* out,
                      double* trials, int max_trials, int32_t* n_trials, double* errors_at) {
    HostOps ops;
    ops.match12 = match12;
    ops.cam = Cam{(double)cam[0], (double)cam[1], (double)cam[2], (double)cam[3]};
    ops.delta = (double)sqrtf(th2);
    ops.trials = trials;
    ops.max_trials = max_trials;
    for (int i1 = 0; i1 < n1; i1++) {
        const int i2 = match12[i1];
        if (i2 < 0 || i2 >= n2) continue;
        const int row1 = rows1[i1], row2 = rows2[i2];
        if (row1 < 0 || row2 < 0) continue;
        if (bad && (bad[row1] || bad[row2])) continue;
        Corr c;
        float X1[3], X2[3];
        const float t1[3] = {Tcw1[3], Tcw1[7], Tcw1[11]}, t2[3] = {Tcw2[3], Tcw2[7], Tcw2[11]};
        spslam::sim3::mat3_mul(Tcw1, 4, xw + 3 * row1, t1, 1.0, X1);
        spslam::sim3::mat3_mul(Tcw2, 4, xw + 3 * row2, t2, 1.0, X2);
        for (int r = 0; r < 3; r++) {
            c.X1[r] = (double)X1[r];
            c.X2[r] = (double)X2[r];
        }
        c.o1[0] = (double)kun1[i1].x; c.o1[1] = (double)kun1[i1].y;
        c.o2[0] = (double)kun2[i2].x; c.o2[1] = (double)kun2[i2].y;
        const int l1 = kun1[i1].octave, l2 = kun2[i2].octave;
        c.w1 = (double)inv_sigma2[l1 >= 1 && l1 < 8 ? l1 : 0];
        c.w2 = (double)inv_sigma2[l2 >= 1 && l2 < 8 ? l2 : 0];
        c.i = i1;
        c.removed = 0;
        ops.C.push_back(c);
    }
    const S3 S0 = sim3_from_float(pair + 1, 3, pair[10], pair[11], pair[12], (double)pair[0]);
    Outcome o;
    optimize_sim3(ops, S0, (double)th2, &o);
    std::memset(out, 0, sizeof *out);
    out->n_in = o.n_in; out->n_corr = o.n_corr; out->n_bad = o.n_bad;
    out->status = o.too_few ? 1 : 0;
    out->accepted = o.n_in >= min_inliers ? 1 : 0;
    out->iterations1 = o.its[0]; out->trials1 = o.trials[0];
    out->iterations2 = o.its[1]; out->trials2 = o.trials[1];
    out->S12[0] = o.S12.r.x; out->S12[1] = o.S12.r.y; out->S12[2] = o.S12.r.z; out->S12[3] = o.S12.r.w;
    out->S12[4] = o.S12.t.x; out->S12[5] = o.S12.t.y; out->S12[6] = o.S12.t.z; out->S12[7] = o.S12.s;
    scw_of(o.S12, Tcw2, out->Scw, out->mScw);
    *n_trials = ops.n_trials;
    for (int k = 0; k < 2; k++) {
        const S3& E = o.last[k];
        const double rec[8] = {E.r.x, E.r.y, E.r.z, E.r.w, E.t.x, E.t.y, E.t.z, E.s};
        std::memcpy(errors_at + 8 * k, rec, sizeof rec);
    }
    return o.n_in;
}

// (H + lambda I) x = b for n = 6 or 7; H: the lower triangle packed by rows.  Returns the solver's verdict.
int sim3_opt_host_ldlt(int n, const double* H, double lambda, const double* b, double* x) {
    return n == 6 ? ldlt_solve<6>(H, lambda, b, x) : ldlt_solve<7>(H, lambda, b, x);
}

}
