// PnPsolver's arithmetic (src/PnPsolver.cc), one copy for the gfx950 kernels (pnp_kernels.hip) and for a host build
// (tests/pnp_host.cpp, which tests/test_pnp_host.py holds against the sequential referee tests/pnp_ref.cpp on a CPU):
// the draws, EPnP (compute_pose) with cvMulTransposed, cvSVD, cvSolve(CV_SVD) and cvInvert(CV_SVD) restated, and
// CheckInliers' test.  Readings: DESIGN.md 3.20.  All of EPnP is fp64 and every operation rounds once (the builds
// keep fp contraction off); the contractions written out are CheckInliers' (check_inlier below).  Nothing but
// + - * / sqrt and fma is used, so that the host and the device agree bit for bit.
//
// EPnP runs over a *source* of correspondences: first(pw, us) gives the first one, each(f) calls f(pw, us) for all
// of them in order.  The per-correspondence arrays of the reference (alphas, pcs) are recomputed in every pass from
// the same inputs by the same operations, which gives the same bits and needs no storage that grows with n.
#pragma once
#include <cstdint>

#if defined(__HIP__)
#define SPSLAM_PNP_HD __host__ __device__ inline
#else
#include <cmath>
#define SPSLAM_PNP_HD inline
#endif

namespace spslam {
namespace pnp {

constexpr double kDblMin = 2.2250738585072014e-308, kDblEps = 2.220446049250313e-16;

// One kept correspondence of the constructor (:78-101), in mvKeyPointIndices' order.
struct Corr {
    float xw[3];      // mvP3Dw
    float uv[2];      // mvP2D
    float max_error;  // mvMaxError: mvSigma2 * th2 in float
    int32_t index;    // mvKeyPointIndices
    int32_t row;      // the map point's row
};
static_assert(sizeof(Corr) == 32, "Corr is 32 bytes (include/spslam_gpu.h states the scratch size)");

// One hypothesis between the two passes: mRi, mti, mnInliersi and the solution compute_pose chose.
struct Hyp {
    double R[9], t[3];
    int32_t n, which;
};
static_assert(sizeof(Hyp) == 104, "Hyp is 104 bytes");

struct Cam { double fu, fv, uc, vc; };  // the Frame's float fx, fy, cx, cy widened (:104-107)

SPSLAM_PNP_HD double absd(double x) { return x < 0.0 ? -x : x; }
SPSLAM_PNP_HD double sqrtd(double x) { return sqrt(x); }

// RandomInt(0, size - 1) from a raw rand() value; a value outside [0, rand_max] is clamped into the list
SPSLAM_PNP_HD int random_int(int r, int rand_max, int size) {
    const int v = (int)(((double)r / ((double)rand_max + 1.0)) * (double)size);
    return v < 0 ? 0 : (v >= size ? size - 1 : v);
}

// The four draws of one iteration (:188-201) on vAvailableIndices = 0 .. n-1 without the array: a position holds its
// own index unless a swap-with-back wrote it, and the latest write wins.  n >= 4.
SPSLAM_PNP_HD void draw4(const int32_t* r, int rand_max, int n, int* idx) {
    int wp[4], wv[4];
    for (int d = 0; d < 4; d++) {
        const int size = n - d, pos = random_int(r[d], rand_max, size);
        int v = pos, back = size - 1;
        for (int q = 0; q < d; q++) {   // in write order: the latest wins
            if (wp[q] == pos) v = wv[q];
            if (wp[q] == size - 1) back = wv[q];
        }
        idx[d] = v;
        wp[d] = pos;
        wv[d] = back;
    }
}

// OpenCV's generator, which JacobiSVD seeds with 0x12345678 to complete a basis
struct CvRng {
    uint64_t state;
    SPSLAM_PNP_HD unsigned next() {
        state = (uint64_t)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
        return (unsigned)state;
    }
};

// JacobiSVDImpl_<double> (OpenCV, modules/core/src/lapack.cpp) with n1 = n: At is n rows of m (the columns of the
// decomposed matrix), which become the left singular vectors; Vt (n x n, may be null) accumulates the rotations;
// W is sorted descending by selection.  hypot(p, beta) is sqrt(p*p + beta*beta).  n <= 12.
SPSLAM_PNP_HD void jacobi_svd(double* At, int m, int n, double* W, double* Vt) {
    const double eps = kDblEps * 10, minval = kDblMin;
    const int max_iter = m > 30 ? m : 30;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
        W[i] = sd;
        if (Vt) {
            for (int k = 0; k < n; k++) Vt[i * n + k] = 0;
            Vt[i * n + i] = 1;
        }
    }
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double* Ai = At + i * m;
                double* Aj = At + j * m;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += Ai[k] * Aj[k];
                if (absd(p) <= eps * sqrtd(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = sqrtd(p * p + beta * beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrtd(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrtd((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const double t0 = c * Ai[k] + s * Aj[k];
                    const double t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += t0 * t0; b += t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                if (Vt) {
                    double* Vi = Vt + i * n;
                    double* Vj = Vt + j * n;
                    for (int k = 0; k < n; k++) {
                        const double t0 = c * Vi[k] + s * Vj[k];
                        const double t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0; Vj[k] = t1;
                    }
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
        W[i] = sqrtd(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            double t = W[i]; W[i] = W[j]; W[j] = t;
            for (int k = 0; k < m; k++) { t = At[i * m + k]; At[i * m + k] = At[j * m + k]; At[j * m + k] = t; }
            if (Vt)
                for (int k = 0; k < n; k++) { t = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = t; }
        }
    }
    CvRng rng{0x12345678u};
    for (int i = 0; i < n; i++) {
        double sd = W[i];
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            // a singular value at or below the minimum: a vector of +-1/m from the generator, made orthogonal to
            // the vectors before it, twice, and normalised
            const double val0 = 1. / m;
            for (int k = 0; k < m; k++) At[i * m + k] = (rng.next() & 256) != 0 ? val0 : -val0;
            for (int iter = 0; iter < 2; iter++)
                for (int j = 0; j < i; j++) {
                    sd = 0;
                    for (int k = 0; k < m; k++) sd += At[i * m + k] * At[j * m + k];
                    double asum = 0;
                    for (int k = 0; k < m; k++) {
                        const double t = At[i * m + k] - sd * At[j * m + k];
                        At[i * m + k] = t;
                        asum += absd(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; k++) At[i * m + k] *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; k++) { const double t = At[i * m + k]; sd += t * t; }
            sd = sqrtd(sd);
        }
        const double s = sd > minval ? 1 / sd : 0.;
        for (int k = 0; k < m; k++) At[i * m + k] *= s;
    }
}

// cvSolve(L, Rho, X, CV_SVD) for L 6 x K (row-major, K <= 5): the SVD of L's transpose as stored, then SVBkSb with
// one right-hand side: the threshold is the sum of the singular values times 2 * DBL_EPSILON.
SPSLAM_PNP_HD void svd_solve6(const double* L, int K, const double* b, double* x) {
    double At[5 * 6], W[5], Vt[5 * 5];
    for (int i = 0; i < K; i++)
        for (int j = 0; j < 6; j++) At[i * 6 + j] = L[j * K + i];
    jacobi_svd(At, 6, K, W, Vt);
    for (int i = 0; i < K; i++) x[i] = 0;
    double threshold = 0;
    for (int i = 0; i < K; i++) threshold += W[i];
    threshold *= kDblEps * 2;
    for (int i = 0; i < K; i++) {
        double wi = W[i];
        if (absd(wi) <= threshold) continue;
        wi = 1 / wi;
        double s = 0;
        for (int j = 0; j < 6; j++) s += At[i * 6 + j] * b[j];
        s *= wi;
        for (int j = 0; j < K; j++) x[j] = x[j] + s * Vt[i * K + j];
    }
}

// cvInvert(CC, CC_inv, CV_SVD) for 3 x 3: SVD::compute, then backSubst without a right-hand side
SPSLAM_PNP_HD void svd_invert3(const double* cc, double* inv) {
    double At[9], W[3], Vt[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) At[i * 3 + j] = cc[j * 3 + i];
    jacobi_svd(At, 3, 3, W, Vt);
    for (int i = 0; i < 9; i++) inv[i] = 0;
    double threshold = 0;
    for (int i = 0; i < 3; i++) threshold += W[i];
    threshold *= kDblEps * 2;
    for (int i = 0; i < 3; i++) {
        double wi = W[i];
        if (absd(wi) <= threshold) continue;
        wi = 1 / wi;
        double buffer[3];
        for (int j = 0; j < 3; j++) buffer[j] = At[i * 3 + j] * wi;   // U(j, i) * wi
        for (int j = 0; j < 3; j++) {
            const double s = Vt[i * 3 + j];
            for (int k = 0; k < 3; k++) inv[j * 3 + k] = inv[j * 3 + k] + s * buffer[k];
        }
    }
}

SPSLAM_PNP_HD double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SPSLAM_PNP_HD double dist2(const double* p1, const double* p2) {
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

// qr_solve (:860-950) for the 6 x 4 system of gauss_newton.  Returns false, with x untouched, on eta == 0.
SPSLAM_PNP_HD bool qr_solve(double* A, double* b, double* X) {
    const int nr = 6, nc = 4;
    double reflect[4], diagonal[4];
    for (int k = 0; k < nc; k++) {
        double largest = absd(A[k * nc + k]);
        for (int i = k; i < nr - 1; i++) {   // rows k .. nr - 2: (k,k) twice, (nr-1,k) never
            const double m = absd(A[i * nc + k]);
            if (largest < m) largest = m;
        }
        if (largest == 0) return false;
        const double shrink = 1. / largest;
        double squares = 0.0;
        for (int i = k; i < nr; i++) {
            A[i * nc + k] *= shrink;
            squares += A[i * nc + k] * A[i * nc + k];
        }
        double sigma = sqrtd(squares);
        if (A[k * nc + k] < 0) sigma = -sigma;
        A[k * nc + k] += sigma;
        reflect[k] = sigma * A[k * nc + k];
        diagonal[k] = -largest * sigma;
        for (int j = k + 1; j < nc; j++) {
            double along = 0;
            for (int i = k; i < nr; i++) along += A[i * nc + k] * A[i * nc + j];
            const double tau = along / reflect[k];
            for (int i = k; i < nr; i++) A[i * nc + j] -= tau * A[i * nc + k];
        }
    }
    for (int j = 0; j < nc; j++) {   // b <- Q^T b
        double tau = 0;
        for (int i = j; i < nr; i++) tau += A[i * nc + j] * b[i];
        tau /= reflect[j];
        for (int i = j; i < nr; i++) b[i] -= tau * A[i * nc + j];
    }
    X[nc - 1] = b[nc - 1] / diagonal[nc - 1];   // back substitution
    for (int i = nc - 2; i >= 0; i--) {
        double known = 0;
        for (int j = i + 1; j < nc; j++) known += A[i * nc + j] * X[j];
        X[i] = (b[i] - known) / diagonal[i];
    }
    return true;
}

// gauss_newton (:840-858): x of the first iteration is 0 where the reference leaves it indeterminate.  *singular
// counts qr_solve's early returns.
SPSLAM_PNP_HD void gauss_newton(const double* L, const double* rho, double* betas, int* singular) {
    double a[24], b[6], x[4] = {0, 0, 0, 0};
    for (int k = 0; k < 5; k++) {
        for (int i = 0; i < 6; i++) {
            const double* r = L + i * 10;
            double* ra = a + i * 4;
            ra[0] = 2 * r[0] * betas[0] + r[1] * betas[1] + r[3] * betas[2] + r[6] * betas[3];
            ra[1] = r[1] * betas[0] + 2 * r[2] * betas[1] + r[4] * betas[2] + r[7] * betas[3];
            ra[2] = r[3] * betas[0] + r[4] * betas[1] + 2 * r[5] * betas[2] + r[8] * betas[3];
            ra[3] = r[6] * betas[0] + r[7] * betas[1] + r[8] * betas[2] + 2 * r[9] * betas[3];
            b[i] = rho[i] - (r[0] * betas[0] * betas[0] + r[1] * betas[0] * betas[1] + r[2] * betas[1] * betas[1] +
                             r[3] * betas[0] * betas[2] + r[4] * betas[1] * betas[2] + r[5] * betas[2] * betas[2] +
                             r[6] * betas[0] * betas[3] + r[7] * betas[1] * betas[3] + r[8] * betas[2] * betas[3] +
                             r[9] * betas[3] * betas[3]);
        }
        if (!qr_solve(a, b, x)) (*singular)++;
        for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
}

SPSLAM_PNP_HD void betas_approx_1(const double* L, const double* rho, double* betas) {
    double l[24], b4[4];
    for (int i = 0; i < 6; i++) {
        l[i * 4] = L[i * 10]; l[i * 4 + 1] = L[i * 10 + 1]; l[i * 4 + 2] = L[i * 10 + 3]; l[i * 4 + 3] = L[i * 10 + 6];
    }
    svd_solve6(l, 4, rho, b4);
    if (b4[0] < 0) {
        betas[0] = sqrtd(-b4[0]);
        betas[1] = -b4[1] / betas[0]; betas[2] = -b4[2] / betas[0]; betas[3] = -b4[3] / betas[0];
    } else {
        betas[0] = sqrtd(b4[0]);
        betas[1] = b4[1] / betas[0]; betas[2] = b4[2] / betas[0]; betas[3] = b4[3] / betas[0];
    }
}

// approximations 2 (K = 3) and 3 (K = 5)
SPSLAM_PNP_HD void betas_approx_23(const double* L, const double* rho, int K, double* betas) {
    double l[30], b[5];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < K; j++) l[i * K + j] = L[i * 10 + j];
    svd_solve6(l, K, rho, b);
    if (b[0] < 0) {
        betas[0] = sqrtd(-b[0]);
        betas[1] = (b[2] < 0) ? sqrtd(-b[2]) : 0.0;
    } else {
        betas[0] = sqrtd(b[0]);
        betas[1] = (b[2] > 0) ? sqrtd(b[2]) : 0.0;
    }
    if (b[1] < 0) betas[0] = -betas[0];
    betas[2] = K == 5 ? b[3] / betas[0] : 0.0;
    betas[3] = 0.0;
}

SPSLAM_PNP_HD void compute_L_6x10(const double* ut, double* l) {
    const int first[6] = {0, 0, 0, 1, 1, 2}, second[6] = {1, 2, 3, 2, 3, 3};   // the six pairs of control points
    for (int p = 0; p < 6; p++) {
        double d[4][3];   // null vector v's difference over the pair
        for (int v = 0; v < 4; v++)
            for (int k = 0; k < 3; k++) d[v][k] = ut[12 * (11 - v) + 3 * first[p] + k] - ut[12 * (11 - v) + 3 * second[p] + k];
        double* row = l + 10 * p;   // columns: B11 B12 B22 B13 B23 B33 B14 B24 B34 B44
        int q = 0;
        for (int j = 0; j < 4; j++)
            for (int i = 0; i <= j; i++) row[q++] = i == j ? dot3(d[i], d[j]) : 2.0f * dot3(d[i], d[j]);
    }
}

// What a pass needs to make a correspondence's alphas and pcs again
struct Bary {
    double cws0[3], ci[9];
    SPSLAM_PNP_HD void alphas(const double* pi, double* a) const {
        for (int j = 0; j < 3; j++)
            a[1 + j] = ci[3 * j] * (pi[0] - cws0[0]) + ci[3 * j + 1] * (pi[1] - cws0[1]) + ci[3 * j + 2] * (pi[2] - cws0[2]);
        a[0] = 1.0f - a[1] - a[2] - a[3];
    }
};

// compute_R_and_t (:651-662): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error
template <class Src>
SPSLAM_PNP_HD double compute_R_and_t(const Src& src, int n, const Cam& cam, const Bary& B, const double* ut,
                                     const double* betas, double* R, double* t) {
    double ccs[4][3];
    for (int i = 0; i < 4; i++) ccs[i][0] = ccs[i][1] = ccs[i][2] = 0.0f;
    for (int i = 0; i < 4; i++) {
        const double* v = ut + 12 * (11 - i);
        for (int j = 0; j < 4; j++)
            for (int k = 0; k < 3; k++) ccs[j][k] += betas[i] * v[3 * j + k];
    }
    auto pcs = [&](const double* pw, double* pc) {
        double a[4];
        B.alphas(pw, a);
        for (int j = 0; j < 3; j++) pc[j] = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
    };
    double pw1[3], us1[2], pc1[3];
    src.first(pw1, us1);
    pcs(pw1, pc1);
    const bool flip = pc1[2] < 0.0;   // solve_for_sign reads pcs[2]
    auto pcs_signed = [&](const double* pw, double* pc) {
        pcs(pw, pc);
        if (flip) { pc[0] = -pc[0]; pc[1] = -pc[1]; pc[2] = -pc[2]; }
    };
    double pc0[3] = {0.0, 0.0, 0.0}, pw0[3] = {0.0, 0.0, 0.0};
    src.each([&](const double* pw, const double*) {
        double pc[3];
        pcs_signed(pw, pc);
        for (int j = 0; j < 3; j++) { pc0[j] += pc[j]; pw0[j] += pw[j]; }
    });
    for (int j = 0; j < 3; j++) { pc0[j] /= n; pw0[j] /= n; }
    double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    src.each([&](const double* pw, const double*) {
        double pc[3];
        pcs_signed(pw, pc);
        for (int j = 0; j < 3; j++) {
            abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
            abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
            abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
        }
    });
    // cvSVD(ABt, D, U, V): U(i, k) = At[k][i], V(j, k) = Vt[k][j]
    double At[9], W[3], Vt[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) At[i * 3 + j] = abt[j * 3 + i];
    jacobi_svd(At, 3, 3, W, Vt);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = At[i] * Vt[j] + At[3 + i] * Vt[3 + j] + At[6 + i] * Vt[6 + j];
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] -
                       R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
    t[0] = pc0[0] - dot3(R, pw0);
    t[1] = pc0[1] - dot3(R + 3, pw0);
    t[2] = pc0[2] - dot3(R + 6, pw0);
    double sum2 = 0.0;
    src.each([&](const double* pw, const double* us) {
        const double Xc = dot3(R, pw) + t[0], Yc = dot3(R + 3, pw) + t[1];
        const double inv_Zc = 1.0 / (dot3(R + 6, pw) + t[2]);
        const double ue = cam.uc + cam.fu * Xc * inv_Zc, ve = cam.vc + cam.fv * Yc * inv_Zc;
        const double u = us[0], v = us[1];
        sum2 += sqrtd((u - ue) * (u - ue) + (v - ve) * (v - ve));
    });
    return sum2 / n;
}

// compute_pose (:477-525) over the n correspondences of src.  Returns the solution chosen (1, 2 or 3).
template <class Src>
SPSLAM_PNP_HD int compute_pose(const Src& src, int n, const Cam& cam, double* R, double* t, int* singular) {
    // choose_control_points
    double cws[4][3];
    cws[0][0] = cws[0][1] = cws[0][2] = 0;
    src.each([&](const double* pw, const double*) {
        for (int j = 0; j < 3; j++) cws[0][j] += pw[j];
    });
    for (int j = 0; j < 3; j++) cws[0][j] /= n;
    double s3[6] = {0, 0, 0, 0, 0, 0};   // cvMulTransposed(PW0, ., 1): the upper triangle, each sum over the rows in order
    src.each([&](const double* pw, const double*) {
        const double d[3] = {pw[0] - cws[0][0], pw[1] - cws[0][1], pw[2] - cws[0][2]};
        s3[0] += d[0] * d[0]; s3[1] += d[0] * d[1]; s3[2] += d[0] * d[2];
        s3[3] += d[1] * d[1]; s3[4] += d[1] * d[2]; s3[5] += d[2] * d[2];
    });
    double uct[9] = {s3[0], s3[1], s3[2], s3[1], s3[3], s3[4], s3[2], s3[4], s3[5]}, dc[3];
    jacobi_svd(uct, 3, 3, dc, nullptr);
    for (int i = 1; i < 4; i++) {
        const double k = sqrtd(dc[i - 1] / n);
        for (int j = 0; j < 3; j++) cws[i][j] = cws[0][j] + k * uct[3 * (i - 1) + j];
    }
    // compute_barycentric_coordinates
    Bary B;
    double cc[9];
    for (int i = 0; i < 3; i++)
        for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[j][i] - cws[0][i];
    svd_invert3(cc, B.ci);
    for (int j = 0; j < 3; j++) B.cws0[j] = cws[0][j];
    // fill_M and cvMulTransposed(M, MtM, 1): 78 sums over the 2n rows in order, the lower triangle copied
    double ut[144], d12[12];
    for (int i = 0; i < 144; i++) ut[i] = 0;
    src.each([&](const double* pw, const double* us) {
        double a[4], M1[12], M2[12];
        B.alphas(pw, a);
        for (int i = 0; i < 4; i++) {
            M1[3 * i] = a[i] * cam.fu; M1[3 * i + 1] = 0.0; M1[3 * i + 2] = a[i] * (cam.uc - us[0]);
            M2[3 * i] = 0.0; M2[3 * i + 1] = a[i] * cam.fv; M2[3 * i + 2] = a[i] * (cam.vc - us[1]);
        }
        for (int i = 0; i < 12; i++)
            for (int j = i; j < 12; j++) {
                ut[12 * i + j] += M1[i] * M1[j];
                ut[12 * i + j] += M2[i] * M2[j];
            }
    });
    for (int i = 0; i < 12; i++)
        for (int j = 0; j < i; j++) ut[12 * i + j] = ut[12 * j + i];
    jacobi_svd(ut, 12, 12, d12, nullptr);   // MtM is symmetric: its transpose as stored is itself
    double L[60], rho[6];
    compute_L_6x10(ut, L);
    rho[0] = dist2(cws[0], cws[1]); rho[1] = dist2(cws[0], cws[2]); rho[2] = dist2(cws[0], cws[3]);
    rho[3] = dist2(cws[1], cws[2]); rho[4] = dist2(cws[1], cws[3]); rho[5] = dist2(cws[2], cws[3]);
    double betas[4], Rs[4][9], ts[4][3], rep[4];
    betas_approx_1(L, rho, betas);
    gauss_newton(L, rho, betas, singular);
    rep[1] = compute_R_and_t(src, n, cam, B, ut, betas, Rs[1], ts[1]);
    betas_approx_23(L, rho, 3, betas);
    gauss_newton(L, rho, betas, singular);
    rep[2] = compute_R_and_t(src, n, cam, B, ut, betas, Rs[2], ts[2]);
    betas_approx_23(L, rho, 5, betas);
    gauss_newton(L, rho, betas, singular);
    rep[3] = compute_R_and_t(src, n, cam, B, ut, betas, Rs[3], ts[3]);
    int N = 1;
    if (rep[2] < rep[1]) N = 2;
    if (rep[3] < rep[N]) N = 3;
    for (int i = 0; i < 9; i++) R[i] = Rs[N][i];
    for (int i = 0; i < 3; i++) t[i] = ts[N][i];
    return N;
}

// CheckInliers' test (:314-329) with the contractions GCC makes of it on an FMA host: the three
// camera coordinates, ue / ve, and error2.  A NaN error2 is no inlier.
SPSLAM_PNP_HD float inlier_error2(const Corr& c, const double* R, const double* t, const Cam& cam) {
    const double x = c.xw[0], y = c.xw[1], z = c.xw[2];
    const float Xc = (float)(fma(R[2], z, fma(R[1], y, R[0] * x)) + t[0]);
    const float Yc = (float)(fma(R[5], z, fma(R[4], y, R[3] * x)) + t[1]);
    const float invZc = (float)(1 / (fma(R[8], z, fma(R[7], y, R[6] * x)) + t[2]));
    const double ue = fma(cam.fu * (double)Xc, (double)invZc, cam.uc);
    const double ve = fma(cam.fv * (double)Yc, (double)invZc, cam.vc);
    const float distX = (float)((double)c.uv[0] - ue), distY = (float)((double)c.uv[1] - ve);
    return fmaf(distX, distX, distY * distY);
}
SPSLAM_PNP_HD bool check_inlier(const Corr& c, const double* R, const double* t, const Cam& cam) {
    return inlier_error2(c, R, t, cam) < c.max_error;
}

// The four correspondences of a hypothesis, in draw order (add_correspondence widens the floats)
struct Src4 {
    double pw[4][3], us[4][2];
    SPSLAM_PNP_HD void set(int i, const Corr& c) {
        for (int j = 0; j < 3; j++) pw[i][j] = c.xw[j];
        us[i][0] = c.uv[0]; us[i][1] = c.uv[1];
    }
    SPSLAM_PNP_HD void first(double* p, double* u) const {
        for (int j = 0; j < 3; j++) p[j] = pw[0][j];
        u[0] = us[0][0]; u[1] = us[0][1];
    }
    template <class F> SPSLAM_PNP_HD void each(F&& f) const {
        for (int i = 0; i < 4; i++) f(pw[i], us[i]);
    }
};

// Refine's correspondences (:262-281): those of the N kept whose flag in a best mask is set, in order.  The mask
// is either bytes (carried in) or CheckInliers at the pose of the hypothesis that set the best.
struct MaskBytes {
    const uint8_t* m;
    SPSLAM_PNP_HD bool operator()(int i, const Corr&) const { return m[i] != 0; }
};
struct MaskPose {
    const double* R;
    const double* t;
    Cam cam;
    SPSLAM_PNP_HD bool operator()(int, const Corr& c) const { return check_inlier(c, R, t, cam); }
};
template <class Mask> struct SrcMask {
    const Corr* C;
    int N;
    Mask mask;
    SPSLAM_PNP_HD int count() const {
        int n = 0;
        for (int i = 0; i < N; i++) n += mask(i, C[i]) ? 1 : 0;
        return n;
    }
    SPSLAM_PNP_HD void first(double* p, double* u) const {
        for (int i = 0; i < N; i++)
            if (mask(i, C[i])) {
                for (int j = 0; j < 3; j++) p[j] = C[i].xw[j];
                u[0] = C[i].uv[0]; u[1] = C[i].uv[1];
                return;
            }
        p[0] = p[1] = p[2] = u[0] = u[1] = 0;
    }
    template <class F> SPSLAM_PNP_HD void each(F&& f) const {
        for (int i = 0; i < N; i++)
            if (mask(i, C[i])) {
                const double p[3] = {C[i].xw[0], C[i].xw[1], C[i].xw[2]}, u[2] = {C[i].uv[0], C[i].uv[1]};
                f(p, u);
            }
    }
};

// Refine (:260-305) up to its test: EPnP over the mask's correspondences and CheckInliers' count
template <class Mask>
SPSLAM_PNP_HD void refine(const Corr* C, int N, const Mask& mask, const Cam& cam, Hyp* out, int* singular) {
    const SrcMask<Mask> src{C, N, mask};
    out->which = compute_pose(src, src.count(), cam, out->R, out->t, singular);
    int n = 0;
    for (int i = 0; i < N; i++) n += check_inlier(C[i], out->R, out->t, cam) ? 1 : 0;
    out->n = n;
}

// The iterations of a call (:182): [first, first + *n_run), cut where the recorded draws end (*cut).
SPSLAM_PNP_HD int call_range(int iterations_done, int n_iterations, int rand_iterations, int n, int min_n, int max_its_n,
                             int max_iterations, int* n_run, bool* cut) {
    const int first = iterations_done < 0 ? 0 : iterations_done;
    int want = n_iterations < 0 ? 0 : n_iterations;
    if (want > max_iterations) want = max_iterations;
    int its = max_its_n > max_iterations ? max_iterations : max_its_n;
    int full = its - first > want ? its - first : want;   // max(mRansacMaxIts, done + nIterations) - done
    if (n < min_n || n < 4) full = 0;   // n < 4 cannot be drawn from (min_n >= minSet = 4 in a sound table)
    int have = rand_iterations - first;
    if (have < 0) have = 0;
    *cut = have < full;
    *n_run = *cut ? have : full;
    return first;
}

// Where the sequential loop evaluates Refine on a mask it has not tried: candidate number q (from 0) of the call.
// The loop (:182-239) replaces the best mask at every k with n_k >= min and n_k > best (a record setter) and calls
// Refine on the best mask at every k with n_k >= min.  Refine's result depends on the mask only, so after a failed
// Refine every later k governed by the same mask fails too.  The candidates are therefore, in order: the first
// qualifying k when it is no record setter (the mask carried in governs it: *carried), then every record setter.
// Scans from *j with the running best *best; returns the candidate's k - first or -1 when the range is exhausted,
// and leaves *j behind it.
SPSLAM_PNP_HD int next_candidate(const Hyp* hyp, int n_run, int min_n, int* j, int* best, bool* seen_qualifying,
                                 bool* carried) {
    for (; *j < n_run; (*j)++) {
        const int nj = hyp[*j].n;
        if (nj < min_n) continue;
        const bool first_q = !*seen_qualifying;
        *seen_qualifying = true;
        if (nj > *best) {
            *best = nj;
            *carried = false;
            return (*j)++;
        }
        if (first_q) {
            *carried = true;
            return (*j)++;
        }
    }
    return -1;
}

// Refine's test (:292) is strict.
SPSLAM_PNP_HD bool refine_succeeds(int refine_n, int min_n) { return refine_n > min_n; }

// How a call ends, once the candidates are refined: one copy for the kernel and for the host build.  The values of
// status are include/spslam_gpu.h's SPSLAM_PNP_* (the kernel file asserts it).
enum { kRefined = 0, kBestNoMore = 1, kNoMore = 2, kOutOfDraws = 3 };
struct Outcome {
    int status, done, n_inliers, best_out, iteration;
    bool pose;        // a pose is returned: REFINED or BEST_NO_MORE
    bool from_setter; // BEST_NO_MORE's mask is the latest record setter's (else the one carried in)
};
// refined: a candidate succeeded, at iteration ret_j of the call with ret_n inliers.  setter_n: the count of the
// latest record setter at or before the point where the loop stops, -1 when there is none.
SPSLAM_PNP_HD Outcome decide(bool refined, int ret_j, int ret_n, int n, int min_n, bool cut, int setter_n, int best_in,
                             int done_in, int first, int n_run) {
    Outcome o;
    o.best_out = setter_n >= 0 ? setter_n : best_in;
    o.n_inliers = 0;
    o.from_setter = setter_n >= 0;
    if (refined) {
        o.status = kRefined;
        o.done = first + ret_j + 1;
        o.n_inliers = ret_n;
    } else if (n < min_n) {           // iterate returns before its loop: mnIterations is untouched
        o.status = kNoMore;
        o.done = done_in;
    } else if (cut) {
        o.status = kOutOfDraws;
        o.done = first + n_run;
    } else if (o.best_out >= min_n) {  // :241-254; mnIterations >= mRansacMaxIts holds whenever the loop is left
        o.status = kBestNoMore;
        o.done = first + n_run;
        o.n_inliers = o.best_out;
    } else {
        o.status = kNoMore;
        o.done = first + n_run;
    }
    o.iteration = refined ? o.done - 1 : -1;
    o.pose = o.status == kRefined || o.status == kBestNoMore;
    return o;
}

// [R | t] as convertTo(CV_32F) rounds it, into eye(4, 4), row-major
SPSLAM_PNP_HD void pose_to_float(const Hyp& h, float* T) {
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) T[4 * a + b] = (float)h.R[3 * a + b];
        T[4 * a + 3] = (float)h.t[a];
    }
    T[12] = T[13] = T[14] = 0.f;
    T[15] = 1.f;
}

// The result record (a spslam_pnp_result).  setter / refined: null when there is none.
template <class Result>
SPSLAM_PNP_HD void fill_result(Result& r, const Outcome& o, int n, int min_n, int max_its_n, int max_iterations,
                               const Hyp* setter, const float* best_Tcw_in, const Hyp* refined) {
    r.status = o.status;
    r.n = n;
    r.iterations_done = o.done;
    r.best_inliers = o.best_out;
    r.n_inliers = o.n_inliers;
    r.iteration = o.iteration;
    r.min_inliers = min_n;
    r.max_its = n < min_n ? 0 : (max_its_n > max_iterations ? max_iterations : (max_its_n < 0 ? 0 : max_its_n));
    if (setter) pose_to_float(*setter, r.best_Tcw);
    else for (int a = 0; a < 16; a++) r.best_Tcw[a] = best_Tcw_in[a];
    if (refined) pose_to_float(*refined, r.Tcw);
    else for (int a = 0; a < 16; a++) r.Tcw[a] = o.pose ? r.best_Tcw[a] : 0.f;
}

}  // namespace pnp
}  // namespace spslam
