// The kernels' arithmetic and selection (sp-slam_amd/csrc/pnp_math.h) built for the host: compiled by
// tests/pnp_cases.py with g++ -ffp-contract=off and held against the referee tests/pnp_ref.cpp bit for bit.  One
// call is one launch of the three kernels of pnp_kernels.hip, done serially: the gather, every hypothesis of the
// call's range, then the candidates' Refine and the selection in the kernels' parallel form (all candidates are
// refined, then the first success is taken).  How the call ends -- Refine's test, the status, the state out, the
// result record -- is pnp_math.h's decide / fill_result, the code the kernel runs; only the loops over the
// correspondences that write the bytes are written here again.
#include <cstring>
#include <vector>

#include "../include/spslam_gpu.h"
#include "../sp-slam_amd/csrc/pnp_math.h"

using namespace spslam::pnp;

extern "C" {

int pnp_host_sizes(int which) { return which == 0 ? (int)sizeof(Corr) : (int)sizeof(Hyp); }

// Q: the state fields and n_iterations / rand_iterations are read.  max_its / min_n: spslam_pnp_ransac_table's.
// hyp_out (may be null): n, which per hypothesis of the range, 2 ints each; n_refines: how many Refine ran.
int pnp_host_call(const float* cam, const float* sigma2, const spslam_keypoint* keys_un, int n_frame, const int32_t* match,
                  const int32_t* kf_rows, int n_kf, const float* xw, const uint8_t* bad, const int32_t* rnd, int rand_max,
                  const int32_t* max_its, const int32_t* min_n, int max_iterations, float th2,
                  const spslam_pnp_problem* Q, spslam_pnp_result* result, uint8_t* inliers, uint8_t* best_mask,
                  int32_t* frame_points, int32_t* hyp_out, int32_t* n_refines) {
    const Cam camd{(double)cam[0], (double)cam[1], (double)cam[2], (double)cam[3]};
    // gather
    std::vector<Corr> C;
    for (int i = 0; i < n_frame; i++) {
        const int m = match[i];
        int row = -1;
        if (m >= 0 && m < n_kf) row = kf_rows[m];
        if (row < 0 || (bad && bad[row])) continue;
        Corr c;
        for (int j = 0; j < 3; j++) c.xw[j] = xw[3 * row + j];
        c.uv[0] = keys_un[i].x; c.uv[1] = keys_un[i].y;
        c.max_error = sigma2[keys_un[i].octave] * th2;
        c.index = i; c.row = row;
        C.push_back(c);
    }
    const int n = (int)C.size();
    const int min_inliers = min_n[n];
    int n_run;
    bool cut;
    const int first = call_range(Q->iterations_done, Q->n_iterations, Q->rand_iterations, n, min_inliers,
                                 max_its[n] < 0 ? 0 : max_its[n], max_iterations, &n_run, &cut);
    // hypotheses
    std::vector<Hyp> hyp(n_run > 0 ? n_run : 1);
    int singular = 0;
    for (int j = 0; j < n_run; j++) {
        int idx[4];
        draw4(rnd + 4 * (size_t)(first + j), rand_max, n, idx);
        Src4 src;
        for (int i = 0; i < 4; i++) src.set(i, C[idx[i]]);
        Hyp& h = hyp[j];
        h.which = compute_pose(src, 4, camd, h.R, h.t, &singular);
        int count = 0;
        for (int i = 0; i < n; i++) count += check_inlier(C[i], h.R, h.t, camd) ? 1 : 0;
        h.n = count;
        if (hyp_out) { hyp_out[2 * j] = h.n; hyp_out[2 * j + 1] = h.which; }
    }
    // candidates, all refined; then the first success
    std::memset(inliers, 0, n_frame);
    std::vector<int> cand_j;
    std::vector<char> cand_carried;
    std::vector<Hyp> ref;
    int scan = 0, best = Q->best_inliers;
    bool seen = false;
    for (;;) {
        bool carried;
        const int j = next_candidate(hyp.data(), n_run, min_inliers, &scan, &best, &seen, &carried);
        if (j < 0) break;
        Hyp r;
        if (carried) refine(C.data(), n, MaskBytes{best_mask}, camd, &r, &singular);
        else refine(C.data(), n, MaskPose{hyp[j].R, hyp[j].t, camd}, camd, &r, &singular);
        cand_j.push_back(j); cand_carried.push_back(carried); ref.push_back(r);
    }
    *n_refines = (int)ref.size();
    int q_ret = -1, ls = -1;
    for (size_t q = 0; q < ref.size(); q++) {
        if (!cand_carried[q]) ls = cand_j[q];
        if (refine_succeeds(ref[q].n, min_inliers)) { q_ret = (int)q; break; }
    }
    const bool refined = q_ret >= 0;
    const Outcome o = decide(refined, refined ? cand_j[q_ret] : 0, refined ? ref[q_ret].n : 0, n, min_inliers, cut,
                             ls >= 0 ? hyp[ls].n : -1, Q->best_inliers, Q->iterations_done, first, n_run);
    if (o.status == kRefined) {
        for (int i = 0; i < n; i++)
            if (check_inlier(C[i], ref[q_ret].R, ref[q_ret].t, camd)) inliers[C[i].index] = 1;
    } else if (o.status == kBestNoMore) {
        for (int i = 0; i < n; i++) {
            const bool is = o.from_setter ? check_inlier(C[i], hyp[ls].R, hyp[ls].t, camd) : best_mask[i] != 0;
            if (is) inliers[C[i].index] = 1;
        }
    }
    if (ls >= 0)
        for (int i = 0; i < n; i++) best_mask[i] = check_inlier(C[i], hyp[ls].R, hyp[ls].t, camd) ? 1 : 0;
    if (o.pose && frame_points)
        for (int i = 0; i < n_frame; i++) frame_points[i] = inliers[i] ? kf_rows[match[i]] : -1;
    spslam_pnp_result r;
    std::memset(&r, 0, sizeof r);
    fill_result(r, o, n, min_inliers, max_its[n], max_iterations, ls >= 0 ? &hyp[ls] : nullptr, Q->best_Tcw,
                refined ? &ref[q_ret] : nullptr);
    *result = r;
    return singular;
}

// the selection alone, on made-up sequences: n[j] per iteration, refine_n[j] = what Refine counts on the mask that
// hypothesis j sets, carried_refine_n = what it counts on the mask carried in.  Returns the candidate that returns
// (its j) or -1; *best_out, *setter_out as the kernel leaves them.
int pnp_host_select(const int32_t* n, const int32_t* refine_n, int n_run, int min_inliers, int best_in,
                    int carried_refine_n, int32_t* best_out, int32_t* setter_out, int32_t* n_refines) {
    std::vector<Hyp> hyp(n_run > 0 ? n_run : 1);
    for (int j = 0; j < n_run; j++) hyp[j].n = n[j];
    int scan = 0, best = best_in, ls = -1, ret = -1, count = 0;
    bool seen = false;
    for (;;) {
        bool carried;
        const int j = next_candidate(hyp.data(), n_run, min_inliers, &scan, &best, &seen, &carried);
        if (j < 0) break;
        count++;
        if (ret >= 0) continue;   // the parallel form refines every candidate; the first success is taken
        if (!carried) ls = j;
        if (refine_succeeds(carried ? carried_refine_n : refine_n[j], min_inliers)) ret = j;
    }
    *best_out = ls >= 0 ? n[ls] : best_in;
    *setter_out = ls;
    *n_refines = count;
    return ret;
}

// the restated OpenCV calls of pnp_math.h on their own
void pnp_host_svd(const double* a, int n, double* w, double* ut, double* vt) {
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) ut[i * n + j] = a[j * n + i];
    jacobi_svd(ut, n, n, w, vt);
}
void pnp_host_solve(const double* A, int K, const double* b, double* x) { svd_solve6(A, K, b, x); }
void pnp_host_invert3(const double* A, double* inv) { svd_invert3(A, inv); }
// CheckInliers' error2 for one correspondence: Rt is R (9, row-major) then t (3)
float pnp_host_error2(const float* xw, const float* uv, const double* Rt, const float* cam) {
    Corr c{};
    for (int j = 0; j < 3; j++) c.xw[j] = xw[j];
    c.uv[0] = uv[0]; c.uv[1] = uv[1];
    return inlier_error2(c, Rt, Rt + 9, Cam{(double)cam[0], (double)cam[1], (double)cam[2], (double)cam[3]});
}
void pnp_host_draw4(const int32_t* r, int rand_max, int n, int32_t* idx) {
    int v[4];
    draw4(r, rand_max, n, v);
    for (int i = 0; i < 4; i++) idx[i] = v[i];
}
}
