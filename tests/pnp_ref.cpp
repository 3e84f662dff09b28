// The referee of the PnPsolver tests: a sequential restatement, in this project's own structure and names, of what
// src/PnPsolver.cc computes as Tracking::Relocalization drives it (the constructor, SetRansacParameters, iterate with
// Refine and CheckInliers, and EPnP): one object per problem, iterate's while loop with its condition as written,
// Refine where the source calls it, every floating-point operation in the source's order.  The OpenCV calls go through the readings of DESIGN.md
// 3.20 (cvr:: below); DUtils::Random::RandomInt reads the recorded draws.  Written apart from
// sp-slam_amd/csrc/pnp_math.h: nothing is shared with the code under test.  Compiled by tests/pnp_cases.py with
// g++ -ffp-contract=off; the contractions of CheckInliers are written out.
#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace cvr {

struct RNG {
    uint64_t state;
    explicit RNG(uint64_t s) : state(s) {}
    unsigned next() {
        state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
        return (unsigned)state;
    }
};

// what the tests read back: the inputs of the restated calls, a few of each kind
struct Capture {
    bool on = false;
    std::vector<double> svd12, svd3, solve, invert;   // solve: K, then L (6 x K), then b (6)
} capture;
constexpr size_t kCaptureCap = 48;

static void JacobiSVD(double* At, size_t astep, double* _W, double* Vt, size_t vstep, int m, int n, int n1) {
    const double minval = DBL_MIN, eps = DBL_EPSILON * 10;
    std::vector<double> Wbuf(n);
    double* W = Wbuf.data();
    int i, j, k, iter, max_iter = std::max(m, 30);
    double c, s, sd;
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) {
            double t = At[i * astep + k];
            sd += t * t;
        }
        W[i] = sd;
        if (Vt) {
            for (k = 0; k < n; k++) Vt[i * vstep + k] = 0;
            Vt[i * vstep + i] = 1;
        }
    }
    for (iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (i = 0; i < n - 1; i++)
            for (j = i + 1; j < n; j++) {
                double *Ai = At + i * astep, *Aj = At + j * astep;
                double a = W[i], p = 0, b = W[j];
                for (k = 0; k < m; k++) p += Ai[k] * Aj[k];
                if (std::abs(p) <= eps * std::sqrt(a * b)) continue;
                p *= 2;
                double beta = a - b, gamma = std::sqrt(p * p + beta * beta);   // hypot, as + * sqrt
                if (beta < 0) {
                    double delta = (gamma - beta) * 0.5;
                    s = std::sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = std::sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
                for (k = 0; k < m; k++) {
                    double t0 = c * Ai[k] + s * Aj[k];
                    double t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0;
                    Aj[k] = t1;
                    a += t0 * t0;
                    b += t1 * t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
                if (Vt) {
                    double *Vi = Vt + i * vstep, *Vj = Vt + j * vstep;
                    for (k = 0; k < n; k++) {
                        double t0 = c * Vi[k] + s * Vj[k];
                        double t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0;
                        Vj[k] = t1;
                    }
                }
            }
        if (!changed) break;
    }
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) {
            double t = At[i * astep + k];
            sd += t * t;
        }
        W[i] = std::sqrt(sd);
    }
    for (i = 0; i < n - 1; i++) {
        j = i;
        for (k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            std::swap(W[i], W[j]);
            if (Vt) {
                for (k = 0; k < m; k++) std::swap(At[i * astep + k], At[j * astep + k]);
                for (k = 0; k < n; k++) std::swap(Vt[i * vstep + k], Vt[j * vstep + k]);
            }
        }
    }
    for (i = 0; i < n; i++) _W[i] = W[i];
    if (!Vt) return;
    RNG rng(0x12345678);
    for (i = 0; i < n1; i++) {
        sd = i < n ? W[i] : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ii++) {
            const double val0 = 1. / m;
            for (k = 0; k < m; k++) {
                double val = (rng.next() & 256) != 0 ? val0 : -val0;
                At[i * astep + k] = val;
            }
            for (iter = 0; iter < 2; iter++)
                for (j = 0; j < i; j++) {
                    sd = 0;
                    for (k = 0; k < m; k++) sd += At[i * astep + k] * At[j * astep + k];
                    double asum = 0;
                    for (k = 0; k < m; k++) {
                        double t = At[i * astep + k] - sd * At[j * astep + k];
                        At[i * astep + k] = t;
                        asum += std::abs(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (k = 0; k < m; k++) At[i * astep + k] *= asum;
                }
            sd = 0;
            for (k = 0; k < m; k++) {
                double t = At[i * astep + k];
                sd += t * t;
            }
            sd = std::sqrt(sd);
        }
        s = sd > minval ? 1 / sd : 0.;
        for (k = 0; k < m; k++) At[i * astep + k] *= s;
    }
}

// cv::SVD::compute on a square n x n matrix: temp_a is the transpose, whose rows become U's columns; the rotations
// are always accumulated (compute_uv), so the vectors are swapped with the values.  ut: U transposed; vt.
static void svd_square(const double* a, int n, double* w, double* ut, double* vt) {
    if (capture.on) {
        std::vector<double>& to = n == 12 ? capture.svd12 : capture.svd3;
        if ((n == 12 || n == 3) && to.size() < kCaptureCap * n * n) to.insert(to.end(), a, a + n * n);
    }
    std::vector<double> temp_v(n * n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) ut[i * n + j] = a[j * n + i];
    JacobiSVD(ut, n, w, temp_v.data(), n, n, n, n);
    if (vt) std::memcpy(vt, temp_v.data(), sizeof(double) * n * n);
}

// cvMulTransposed(src, dst, 1): dst = src^T * src, MulTransposedR: the upper triangle, each entry one sum over the
// rows from 0, then completeSymm
static void mul_transposed(const double* src, int rows, int cols, double* dst) {
    for (int i = 0; i < cols; i++)
        for (int j = i; j < cols; j++) {
            double s0 = 0;
            for (int k = 0; k < rows; k++) s0 += src[k * cols + i] * src[k * cols + j];
            dst[i * cols + j] = s0;
        }
    for (int i = 0; i < cols; i++)
        for (int j = 0; j < i; j++) dst[i * cols + j] = dst[j * cols + i];
}

// SVBkSb with uT and vT both true unless u_cols: x (n x nb) = v * inv(w) * uT * b; b == NULL is the identity
static void SVBkSb(int m, int n, const double* w, const double* u, int ldu, bool uT, const double* v, int ldv,
                   const double* b, int nb, double* x, int ldx) {
    double threshold = 0, eps = DBL_EPSILON * 2;
    int udelta0 = uT ? ldu : 1, udelta1 = uT ? 1 : ldu;
    int vdelta0 = ldv, vdelta1 = 1;
    int i, j, nm = std::min(m, n);
    std::vector<double> buffer(nb);
    if (!b) nb = m;
    buffer.resize(nb);
    for (i = 0; i < n; i++)
        for (j = 0; j < nb; j++) x[i * ldx + j] = 0;
    for (i = 0; i < nm; i++) threshold += w[i];
    threshold *= eps;
    for (i = 0; i < nm; i++, u += udelta0, v += vdelta0) {
        double wi = w[i];
        if (std::abs(wi) <= threshold) continue;
        wi = 1 / wi;
        if (nb == 1) {
            double s = 0;
            if (b)
                for (j = 0; j < m; j++) s += u[j * udelta1] * b[j];
            else
                s = u[0];
            s *= wi;
            for (j = 0; j < n; j++) x[j * ldx] = x[j * ldx] + s * v[j * vdelta1];
        } else {
            for (j = 0; j < nb; j++) buffer[j] = u[j * udelta1] * wi;   // b == NULL
            for (int r = 0; r < n; r++) {                                // MatrAXPY(n, nb, buffer, 0, v, vdelta1, x, ldx)
                double s = v[r * vdelta1];
                for (j = 0; j < nb; j++) x[r * ldx + j] = x[r * ldx + j] + s * buffer[j];
            }
        }
    }
}

// cvSolve(A, b, x, CV_SVD), A m x n with m >= n, one right-hand side
static void solve_svd(const double* A, int m, int n, const double* b, double* x) {
    if (capture.on && capture.solve.size() < kCaptureCap * 40) {
        capture.solve.push_back(n);
        capture.solve.insert(capture.solve.end(), A, A + m * n);
        capture.solve.insert(capture.solve.end(), b, b + m);
    }
    std::vector<double> a(n * m), w(n), v(n * n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < m; j++) a[i * m + j] = A[j * n + i];
    JacobiSVD(a.data(), m, w.data(), v.data(), n, m, n, n);
    SVBkSb(m, n, w.data(), a.data(), m, true, v.data(), n, b, 1, x, 1);
}

// cvInvert(A, inv, CV_SVD), 3 x 3
static void invert_svd3(const double* A, double* inv) {
    if (capture.on && capture.invert.size() < kCaptureCap * 9) capture.invert.insert(capture.invert.end(), A, A + 9);
    double w[3], ut[9], vt[9], u[9];
    svd_square(A, 3, w, ut, vt);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) u[i * 3 + j] = ut[j * 3 + i];
    SVBkSb(3, 3, w, u, 3, false, vt, 3, nullptr, 3, inv, 3);
}

}  // namespace cvr

namespace {

struct Keypoint { float x, y, size, angle, response; int32_t octave, class_id; };

struct Result {
    int32_t status, n, iterations_done, best_inliers, n_inliers, iteration, min_inliers, max_its;
    float best_Tcw[16], Tcw[16];
};
enum { REFINED = 0, BEST_NO_MORE = 1, NO_MORE = 2, OUT_OF_DRAWS = 3 };

struct Trace {
    int32_t k, idx[4], n, replaced, refine_ran, refine_n, which, refine_which, singular;
    double Rt[12], refine_Rt[12];
};

struct Mat44 {
    bool empty = true;
    float v[16] = {};
};

struct OutOfDraws {};

// A small dense matrix with (row, column) access: the referee indexes, it does not walk pointers.
struct Dense {
    int rows = 0, cols = 0;
    std::vector<double> v;
    Dense() {}
    Dense(int r, int c) : rows(r), cols(c), v((size_t)r * c, 0.0) {}
    double& operator()(int r, int c) { return v[(size_t)r * cols + c]; }
    double operator()(int r, int c) const { return v[(size_t)r * cols + c]; }
};

using Vec3 = std::array<double, 3>;

static double inner(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static double squared_distance(const double* a, const double* b) {
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// the six pairs of control points, in the order the distance constraints are listed, and the ten products
// beta_i * beta_j in the order of the columns of the 6 x 10 system: 11 12 22 13 23 33 14 24 34 44
static const int kPair[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
static const int kProduct[10][2] = {{0, 0}, {0, 1}, {1, 1}, {0, 2}, {1, 2}, {2, 2}, {0, 3}, {1, 3}, {2, 3}, {3, 3}};
static const int kColumnOf[4][4] = {{0, 1, 3, 6}, {1, 2, 4, 7}, {3, 4, 5, 8}, {6, 7, 8, 9}};

// One relocalization candidate's solver: what the reference's PnPsolver object is over its life.  Member functions
// are named for what they do; the comments give the reference's function.  The order of every floating-point
// operation is the reference's.
class RansacEpnp {
public:
    const int32_t* draws = nullptr;   // the recorded rand() values, 4 per iteration
    int draw_iterations = 0, draw_max = 0;
    std::vector<Trace>* trace = nullptr;
    int sign_flips = 0, det_flips = 0;

    // the constructor: keep keypoint i, in order, when it has a point that is not bad
    RansacEpnp(const float* cam, const float* level_sigma2, const Keypoint* keys, const std::vector<int>& point_of,
               const uint8_t* bad, const float* xw)
        : point_of_(point_of) {
        for (size_t i = 0; i < point_of.size(); i++) {
            const int row = point_of[i];
            if (row < 0) continue;
            if (bad && bad[row]) continue;
            Kept k;
            k.pixel[0] = keys[i].x; k.pixel[1] = keys[i].y;
            k.sigma2 = level_sigma2[keys[i].octave];
            for (int a = 0; a < 3; a++) k.world[a] = xw[3 * row + a];
            k.keypoint = (int)i;
            k.limit = 0.f;
            kept_.push_back(k);
        }
        fx_ = cam[0]; fy_ = cam[1]; cx_ = cam[2]; cy_ = cam[3];
        configure(0.99, 8, 300, 4, 0.4f, 5.991f);   // the constructor's own call, overwritten by the caller's
    }

    // SetRansacParameters
    void configure(double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2) {
        const int N = (int)kept_.size();
        min_set_ = min_set;
        int need = N * epsilon;   // an int times a float, truncated
        need = std::max(need, min_inliers);
        need = std::max(need, min_set);
        min_inliers_ = need;
        float eps = epsilon;
        if (eps < (float)need / N) eps = (float)need / N;
        int its = 1;
        if (need != N) {
            // a quotient no int holds counts as max_iterations (the table's rule)
            const double q = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)eps, 3)));
            its = q < (double)max_iterations ? (int)q : max_iterations;
        }
        max_its_ = std::max(1, std::min(its, max_iterations));
        for (Kept& k : kept_) k.limit = k.sigma2 * th2;   // float times float
        flags_.assign(N, false);
    }

    // iterate: the while loop as written
    Mat44 run(int n_iterations, bool& no_more, std::vector<bool>& inliers_out, int& n_inliers_out) {
        const int N = (int)kept_.size();
        no_more = false;
        inliers_out.clear();
        n_inliers_out = 0;
        if (N < min_inliers_) {
            no_more = true;
            return Mat44();
        }
        int this_call = 0;
        while (done_ < max_its_ || this_call < n_iterations) {
            if (done_ >= draw_iterations) throw OutOfDraws();
            this_call++;
            done_++;
            Trace T{};
            T.k = done_ - 1;
            // the minimal set: positions drawn from a list that shrinks by swap-with-back
            std::vector<int> available(N);
            for (int i = 0; i < N; i++) available[i] = i;
            std::vector<int> chosen;
            for (int d = 0; d < min_set_; d++) {
                const int pos = random_position((int)available.size(), 4 * (done_ - 1) + d);
                chosen.push_back(available[pos]);
                T.idx[d] = available[pos];
                available[pos] = available.back();
                available.pop_back();
            }
            load(chosen);
            singular_ = 0;
            T.which = solve_pose();
            T.singular = singular_;
            count_inliers();
            T.n = n_flags_;
            copy_pose(T.Rt);
            bool returned = false;
            if (n_flags_ >= min_inliers_) {
                if (n_flags_ > best_count_) {
                    T.replaced = 1;
                    best_flags_ = flags_;
                    best_count_ = n_flags_;
                    best_T_ = pose_as_float();
                }
                T.refine_ran = 1;
                singular_ = 0;
                returned = refine_on_best(&T.refine_which);
                T.refine_n = refined_count_;
                T.singular += singular_ << 16;
                copy_pose(T.refine_Rt);
            }
            if (trace) trace->push_back(T);
            if (returned) {
                n_inliers_out = refined_count_;
                mark(refined_flags_, inliers_out);
                return refined_T_;
            }
        }
        if (done_ >= max_its_) {
            no_more = true;
            if (best_count_ >= min_inliers_) {
                n_inliers_out = best_count_;
                mark(best_flags_, inliers_out);
                return best_T_;
            }
        }
        return Mat44();
    }

    int iterations_done() const { return done_; }
    int best_count() const { return best_count_; }
    int min_inliers() const { return min_inliers_; }
    int max_its() const { return max_its_; }
    int kept() const { return (int)kept_.size(); }
    const std::vector<bool>& best_flags() const { return best_flags_; }
    const Mat44& best_T() const { return best_T_; }
    const std::vector<int>& point_of() const { return point_of_; }

private:
    struct Kept {
        float world[3], pixel[2], sigma2, limit;
        int keypoint;
    };

    // DUtils::Random::RandomInt(0, size - 1) on a recorded value
    int random_position(int size, int at) const {
        return int(((double)draws[at] / ((double)draw_max + 1.0)) * size);
    }

    // vbInliers: a frame-long vector with the kept keypoints' flags
    void mark(const std::vector<bool>& flags, std::vector<bool>& out) const {
        out = std::vector<bool>(point_of_.size(), false);
        for (size_t i = 0; i < kept_.size(); i++)
            if (flags[i]) out[kept_[i].keypoint] = true;
    }

    void copy_pose(double* Rt) const {
        for (int q = 0; q < 9; q++) Rt[q] = R_[q / 3][q % 3];
        for (int q = 0; q < 3; q++) Rt[9 + q] = t_[q];
    }

    // convertTo(CV_32F) into eye(4, 4)
    Mat44 pose_as_float() const {
        Mat44 T;
        T.empty = false;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) T.v[4 * r + c] = (float)R_[r][c];
            T.v[4 * r + 3] = (float)t_[r];
        }
        T.v[15] = 1.f;
        return T;
    }

    // reset_correspondences and add_correspondence: the floats widened
    void load(const std::vector<int>& which) {
        world_.clear();
        image_.clear();
        for (int i : which) {
            const Kept& k = kept_[i];
            world_.push_back({(double)k.world[0], (double)k.world[1], (double)k.world[2]});
            image_.push_back({(double)k.pixel[0], (double)k.pixel[1]});
        }
        bary_.assign(which.size(), {0, 0, 0, 0});
        camera_.assign(which.size(), {0, 0, 0});
    }

    // Refine: EPnP over the best mask's correspondences, whatever the current hypothesis flagged
    bool refine_on_best(int32_t* which) {
        std::vector<int> members;
        for (size_t i = 0; i < best_flags_.size(); i++)
            if (best_flags_[i]) members.push_back((int)i);
        load(members);
        *which = solve_pose();
        count_inliers();
        refined_count_ = n_flags_;
        refined_flags_ = flags_;
        if (n_flags_ > min_inliers_) {
            refined_T_ = pose_as_float();
            return true;
        }
        return false;
    }

    // CheckInliers, with GCC's contractions on an FMA host written out
    void count_inliers() {
        n_flags_ = 0;
        for (size_t i = 0; i < kept_.size(); i++) {
            const Kept& k = kept_[i];
            const double X = k.world[0], Y = k.world[1], Z = k.world[2];
            const float xc = (float)(std::fma(R_[0][2], Z, std::fma(R_[0][1], Y, R_[0][0] * X)) + t_[0]);
            const float yc = (float)(std::fma(R_[1][2], Z, std::fma(R_[1][1], Y, R_[1][0] * X)) + t_[1]);
            const float inv_z = (float)(1 / (std::fma(R_[2][2], Z, std::fma(R_[2][1], Y, R_[2][0] * X)) + t_[2]));
            const double u = std::fma(fx_ * xc, (double)inv_z, cx_);
            const double v = std::fma(fy_ * yc, (double)inv_z, cy_);
            const float du = (float)(k.pixel[0] - u), dv = (float)(k.pixel[1] - v);
            const float e2 = std::fma(du, du, dv * dv);
            flags_[i] = e2 < k.limit;
            if (flags_[i]) n_flags_++;
        }
    }

    // choose_control_points: the centroid and the principal axes of the loaded points
    void place_control_points() {
        const int n = (int)world_.size();
        for (int a = 0; a < 3; a++) ctrl_world_[0][a] = 0;
        for (const Vec3& p : world_)
            for (int a = 0; a < 3; a++) ctrl_world_[0][a] += p[a];
        for (int a = 0; a < 3; a++) ctrl_world_[0][a] /= n;
        std::vector<double> centred(3 * (size_t)n);
        for (int i = 0; i < n; i++)
            for (int a = 0; a < 3; a++) centred[3 * i + a] = world_[i][a] - ctrl_world_[0][a];
        double scatter[9], spread[3], axes[9];
        cvr::mul_transposed(centred.data(), n, 3, scatter);
        cvr::svd_square(scatter, 3, spread, axes, nullptr);
        for (int c = 1; c < 4; c++) {
            const double length = std::sqrt(spread[c - 1] / n);
            for (int a = 0; a < 3; a++) ctrl_world_[c][a] = ctrl_world_[0][a] + length * axes[3 * (c - 1) + a];
        }
    }

    // compute_barycentric_coordinates
    void barycentric() {
        double edges[9], inverse[9];
        for (int a = 0; a < 3; a++)
            for (int c = 1; c < 4; c++) edges[3 * a + c - 1] = ctrl_world_[c][a] - ctrl_world_[0][a];
        cvr::invert_svd3(edges, inverse);
        for (size_t i = 0; i < world_.size(); i++) {
            const Vec3& p = world_[i];
            std::array<double, 4>& w = bary_[i];
            for (int c = 0; c < 3; c++)
                w[1 + c] = inverse[3 * c] * (p[0] - ctrl_world_[0][0]) + inverse[3 * c + 1] * (p[1] - ctrl_world_[0][1]) +
                           inverse[3 * c + 2] * (p[2] - ctrl_world_[0][2]);
            w[0] = 1.0f - w[1] - w[2] - w[3];
        }
    }

    // compute_pose: returns the solution chosen (1, 2 or 3)
    int solve_pose() {
        const int n = (int)world_.size();
        place_control_points();
        barycentric();
        // fill_M: two rows per correspondence
        Dense M(2 * n, 12);
        for (int i = 0; i < n; i++)
            for (int c = 0; c < 4; c++) {
                const double w = bary_[i][c];
                M(2 * i, 3 * c) = w * fx_;
                M(2 * i, 3 * c + 1) = 0.0;
                M(2 * i, 3 * c + 2) = w * (cx_ - image_[i][0]);
                M(2 * i + 1, 3 * c) = 0.0;
                M(2 * i + 1, 3 * c + 1) = w * fy_;
                M(2 * i + 1, 3 * c + 2) = w * (cy_ - image_[i][1]);
            }
        double gram[144], values[12];
        cvr::mul_transposed(M.v.data(), 2 * n, 12, gram);
        cvr::svd_square(gram, 12, values, null_rows_, nullptr);
        Dense L(6, 10);
        double rho[6];
        distance_system(L, rho);
        double beta[4][4], error[4], Rs[4][3][3], ts[4][3];
        for (int kind = 1; kind <= 3; kind++) {
            starting_betas(kind, L, rho, beta[kind]);
            gauss_newton(L, rho, beta[kind]);
            error[kind] = pose_from_betas(beta[kind], Rs[kind], ts[kind]);
        }
        int pick = 1;
        if (error[2] < error[1]) pick = 2;
        if (error[3] < error[pick]) pick = 3;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) R_[r][c] = Rs[pick][r][c];
            t_[r] = ts[pick][r];
        }
        return pick;
    }

    // the null vector number v (0 is the last row of Ut)
    const double* null_vector(int v) const { return null_rows_ + 12 * (11 - v); }

    // compute_L_6x10 and compute_rho: one row per pair of control points
    void distance_system(Dense& L, double* rho) const {
        double diff[4][6][3];
        for (int v = 0; v < 4; v++)
            for (int p = 0; p < 6; p++)
                for (int a = 0; a < 3; a++)
                    diff[v][p][a] = null_vector(v)[3 * kPair[p][0] + a] - null_vector(v)[3 * kPair[p][1] + a];
        for (int p = 0; p < 6; p++) {
            for (int q = 0; q < 10; q++) {
                const int i = kProduct[q][0], j = kProduct[q][1];
                const double d = inner(diff[i][p], diff[j][p]);
                L(p, q) = i == j ? d : 2.0f * d;
            }
            rho[p] = squared_distance(ctrl_world_[kPair[p][0]], ctrl_world_[kPair[p][1]]);
        }
    }

    // find_betas_approx_1 / 2 / 3: the least-squares solution over a few columns, then the betas from its signs
    void starting_betas(int kind, const Dense& L, const double* rho, double* beta) const {
        static const int cols1[4] = {0, 1, 3, 6}, cols23[5] = {0, 1, 2, 3, 4};
        const int K = kind == 1 ? 4 : kind == 2 ? 3 : 5;
        const int* cols = kind == 1 ? cols1 : cols23;
        std::vector<double> sub(6 * (size_t)K);
        double b[5];
        for (int p = 0; p < 6; p++)
            for (int c = 0; c < K; c++) sub[p * K + c] = L(p, cols[c]);
        cvr::solve_svd(sub.data(), 6, K, rho, b);
        const bool negative = b[0] < 0;
        beta[0] = std::sqrt(negative ? -b[0] : b[0]);
        if (kind == 1) {
            for (int c = 1; c < 4; c++) beta[c] = (negative ? -b[c] : b[c]) / beta[0];
            return;
        }
        if (negative)
            beta[1] = b[2] < 0 ? std::sqrt(-b[2]) : 0.0;
        else
            beta[1] = b[2] > 0 ? std::sqrt(b[2]) : 0.0;
        if (b[1] < 0) beta[0] = -beta[0];
        beta[2] = kind == 3 ? b[3] / beta[0] : 0.0;
        beta[3] = 0.0;
    }

    // gauss_newton with compute_A_and_b_gauss_newton: five steps; the step of a singular system is the one before
    // it, and before the first it is 0 (indeterminate in the reference)
    void gauss_newton(const Dense& L, const double* rho, double* beta) {
        double step[4] = {0, 0, 0, 0};
        for (int it = 0; it < 5; it++) {
            Dense J(6, 4);
            std::vector<double> residual(6);
            for (int p = 0; p < 6; p++) {
                for (int i = 0; i < 4; i++) {
                    double sum = 0;
                    for (int j = 0; j < 4; j++) {
                        const double coefficient = i == j ? 2 * L(p, kColumnOf[i][j]) : L(p, kColumnOf[i][j]);
                        const double term = coefficient * beta[j];
                        sum = j == 0 ? term : sum + term;
                    }
                    J(p, i) = sum;
                }
                double model = 0;
                for (int q = 0; q < 10; q++) {
                    const double term = L(p, q) * beta[kProduct[q][0]] * beta[kProduct[q][1]];
                    model = q == 0 ? term : model + term;
                }
                residual[p] = rho[p] - model;
            }
            householder_solve(J, residual, step);
            for (int i = 0; i < 4; i++) beta[i] += step[i];
        }
    }

    // qr_solve: Householder QR of the 6 x 4 system.  The scan for the column's largest magnitude looks at rows
    // col .. rows - 2 (the reference reads before it advances), and a zero column returns with x untouched.
    void householder_solve(Dense& A, std::vector<double>& rhs, double* x) {
        const int rows = A.rows, cols = A.cols;
        std::vector<double> reflect(cols), diagonal(cols);
        for (int col = 0; col < cols; col++) {
            double largest = std::fabs(A(col, col));
            for (int row = col; row < rows - 1; row++) {
                const double m = std::fabs(A(row, col));
                if (largest < m) largest = m;
            }
            if (largest == 0) {
                singular_++;
                return;
            }
            const double shrink = 1. / largest;
            double squares = 0.0;
            for (int row = col; row < rows; row++) {
                A(row, col) *= shrink;
                squares += A(row, col) * A(row, col);
            }
            double sigma = std::sqrt(squares);
            if (A(col, col) < 0) sigma = -sigma;
            A(col, col) += sigma;
            reflect[col] = sigma * A(col, col);
            diagonal[col] = -largest * sigma;
            for (int other = col + 1; other < cols; other++) {
                double along = 0;
                for (int row = col; row < rows; row++) along += A(row, col) * A(row, other);
                const double tau = along / reflect[col];
                for (int row = col; row < rows; row++) A(row, other) -= tau * A(row, col);
            }
        }
        for (int col = 0; col < cols; col++) {   // Q^T rhs
            double tau = 0;
            for (int row = col; row < rows; row++) tau += A(row, col) * rhs[row];
            tau /= reflect[col];
            for (int row = col; row < rows; row++) rhs[row] -= tau * A(row, col);
        }
        x[cols - 1] = rhs[cols - 1] / diagonal[cols - 1];   // back substitution
        for (int row = cols - 2; row >= 0; row--) {
            double known = 0;
            for (int c = row + 1; c < cols; c++) known += A(row, c) * x[c];
            x[row] = (rhs[row] - known) / diagonal[row];
        }
    }

    // compute_R_and_t: compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error
    double pose_from_betas(const double* beta, double R[3][3], double t[3]) {
        const int n = (int)world_.size();
        for (int c = 0; c < 4; c++)
            for (int a = 0; a < 3; a++) {
                ctrl_camera_[c][a] = 0.0f;
                for (int v = 0; v < 4; v++) ctrl_camera_[c][a] += beta[v] * null_vector(v)[3 * c + a];
            }
        for (int i = 0; i < n; i++)
            for (int a = 0; a < 3; a++)
                camera_[i][a] = bary_[i][0] * ctrl_camera_[0][a] + bary_[i][1] * ctrl_camera_[1][a] +
                                bary_[i][2] * ctrl_camera_[2][a] + bary_[i][3] * ctrl_camera_[3][a];
        if (camera_[0][2] < 0.0) {   // the first point must be in front of the camera
            sign_flips++;
            for (int c = 0; c < 4; c++)
                for (int a = 0; a < 3; a++) ctrl_camera_[c][a] = -ctrl_camera_[c][a];
            for (Vec3& p : camera_)
                for (int a = 0; a < 3; a++) p[a] = -p[a];
        }
        align(R, t);
        // the mean reprojection error
        double total = 0.0;
        for (int i = 0; i < n; i++) {
            const double* p = world_[i].data();
            const double xc = inner(R[0], p) + t[0], yc = inner(R[1], p) + t[1];
            const double inv_z = 1.0 / (inner(R[2], p) + t[2]);
            const double u = cx_ + fx_ * xc * inv_z, v = cy_ + fy_ * yc * inv_z;
            const double du = image_[i][0] - u, dv = image_[i][1] - v;
            total += std::sqrt(du * du + dv * dv);
        }
        return total / n;
    }

    // estimate_R_and_t: the rotation from the SVD of the cross-covariance of the two point sets
    void align(double R[3][3], double t[3]) {
        const int n = (int)world_.size();
        double mean_c[3] = {0.0, 0.0, 0.0}, mean_w[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < n; i++)
            for (int a = 0; a < 3; a++) {
                mean_c[a] += camera_[i][a];
                mean_w[a] += world_[i][a];
            }
        for (int a = 0; a < 3; a++) {
            mean_c[a] /= n;
            mean_w[a] /= n;
        }
        double cross[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, values[3], ut[9], vt[9];
        for (int i = 0; i < n; i++)
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++)
                    cross[3 * r + c] += (camera_[i][r] - mean_c[r]) * (world_[i][c] - mean_w[c]);
        cvr::svd_square(cross, 3, values, ut, vt);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++)   // U(r, k) * V(c, k) over k, U and V as cvSVD returns them
                R[r][c] = ut[r] * vt[c] + ut[3 + r] * vt[3 + c] + ut[6 + r] * vt[6 + c];
        auto along = [&](int a, int b, int c) { return R[0][a] * R[1][b] * R[2][c]; };
        const double det = along(0, 1, 2) + along(1, 2, 0) + along(2, 0, 1) - along(2, 1, 0) - along(1, 0, 2) - along(0, 2, 1);
        if (det < 0) {
            det_flips++;
            for (int c = 0; c < 3; c++) R[2][c] = -R[2][c];
        }
        for (int r = 0; r < 3; r++) t[r] = mean_c[r] - inner(R[r], mean_w);
    }

    // the frame's side
    std::vector<int> point_of_;
    std::vector<Kept> kept_;
    double fx_, fy_, cx_, cy_;
    // RANSAC
    int min_set_ = 4, min_inliers_ = 0, max_its_ = 0, done_ = 0, best_count_ = 0, n_flags_ = 0, refined_count_ = 0;
    std::vector<bool> flags_, best_flags_, refined_flags_;
    Mat44 best_T_, refined_T_;
    double R_[3][3], t_[3];
    int singular_ = 0;
    // EPnP's working set
    std::vector<Vec3> world_, camera_;
    std::vector<std::array<double, 2>> image_;
    std::vector<std::array<double, 4>> bary_;
    double ctrl_world_[4][3], ctrl_camera_[4][3], null_rows_[144];
};

}  // namespace

extern "C" {

// One solver over its life: n_calls calls of iterate(n_iterations[r]).  match: n_frame entries, a keyframe keypoint
// or -1; kf_rows: the keyframe's map points as rows (or -1).  Per call r: results[r]; inliers, best_mask (N bytes
// used) and frame_points at r * n_frame.  counters: sign flips, det flips.  Returns the number of trace records.
int pnp_ref_run(const float* cam, const float* sigma2, const Keypoint* keys_un, int n_frame, const int32_t* match,
                const int32_t* kf_rows, int n_kf, const float* xw, const uint8_t* bad, const int32_t* rnd,
                int rand_iterations, int rand_max, double probability, int min_inliers, int max_iterations, int min_set,
                float epsilon, float th2, int n_calls, const int32_t* n_iterations, Result* results, uint8_t* inliers,
                uint8_t* best_mask, int32_t* frame_points, Trace* trace, int trace_cap, int32_t* counters) {
    std::vector<int> matches(n_frame, -1);
    for (int i = 0; i < n_frame; i++)
        if (match[i] >= 0 && match[i] < n_kf) matches[i] = kf_rows[match[i]];
    RansacEpnp* s = new RansacEpnp(cam, sigma2, keys_un, matches, bad, xw);
    s->configure(probability, min_inliers, max_iterations, min_set, epsilon, th2);
    s->draws = rnd; s->draw_iterations = rand_iterations; s->draw_max = rand_max;
    std::vector<Trace> tr;
    s->trace = &tr;
    for (int r = 0; r < n_calls; r++) {
        Result& o = results[r];
        std::memset(&o, 0, sizeof o);
        uint8_t* in = inliers + (size_t)r * n_frame;
        uint8_t* bm = best_mask + (size_t)r * n_frame;
        int32_t* fp = frame_points + (size_t)r * n_frame;
        std::memset(in, 0, n_frame);
        std::memset(bm, 0, n_frame);
        for (int i = 0; i < n_frame; i++) fp[i] = -1;
        bool no_more = false, cut = false;
        std::vector<bool> flags;
        int n_inliers = 0;
        Mat44 Tcw;
        try {
            Tcw = s->run(n_iterations[r], no_more, flags, n_inliers);
        } catch (const OutOfDraws&) {
            cut = true;
        }
        o.status = cut ? OUT_OF_DRAWS : !Tcw.empty ? (no_more ? BEST_NO_MORE : REFINED) : NO_MORE;
        o.n = s->kept();
        o.iterations_done = s->iterations_done();
        o.best_inliers = s->best_count();
        o.n_inliers = n_inliers;
        o.iteration = o.status == REFINED ? s->iterations_done() - 1 : -1;
        o.min_inliers = s->min_inliers();
        o.max_its = s->kept() < s->min_inliers() ? 0 : s->max_its();
        std::memcpy(o.best_Tcw, s->best_T().v, 64);
        if (!Tcw.empty) {
            std::memcpy(o.Tcw, Tcw.v, 64);
            for (int i = 0; i < n_frame; i++) {
                in[i] = flags[i] ? 1 : 0;
                fp[i] = flags[i] ? s->point_of()[i] : -1;   // Tracking.cc:1661-1670
            }
        }
        for (size_t i = 0; i < s->best_flags().size(); i++) bm[i] = s->best_flags()[i] ? 1 : 0;
    }
    counters[0] = s->sign_flips;
    counters[1] = s->det_flips;
    delete s;
    const int n = (int)std::min(tr.size(), (size_t)trace_cap);
    if (n) std::memcpy(trace, tr.data(), sizeof(Trace) * n);
    return (int)tr.size();
}

// the restated OpenCV calls on their own, for the checks against numpy
void pnp_ref_svd(const double* a, int n, double* w, double* ut, double* vt) { cvr::svd_square(a, n, w, ut, vt); }
void pnp_ref_solve(const double* A, int n, const double* b, double* x) { cvr::solve_svd(A, 6, n, b, x); }
void pnp_ref_invert3(const double* A, double* inv) { cvr::invert_svd3(A, inv); }
void pnp_ref_mul_transposed(const double* src, int rows, int cols, double* dst) { cvr::mul_transposed(src, rows, cols, dst); }

void pnp_ref_capture(int on) {
    cvr::capture = cvr::Capture();
    cvr::capture.on = on != 0;
}
// kind 0: 12 x 12 SVD inputs, 1: 3 x 3 SVD inputs, 2: solve records, 3: invert inputs.  Returns the doubles held.
int pnp_ref_captured(int kind, double* out, int cap) {
    const std::vector<double>& v = kind == 0 ? cvr::capture.svd12 : kind == 1 ? cvr::capture.svd3
                                 : kind == 2 ? cvr::capture.solve : cvr::capture.invert;
    const int n = (int)std::min(v.size(), (size_t)cap);
    if (out && n) std::memcpy(out, v.data(), sizeof(double) * n);
    return (int)v.size();
}

int pnp_ref_sizes(int which) { return which == 0 ? (int)sizeof(Result) : (int)sizeof(Trace); }
}
