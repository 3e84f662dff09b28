// C ABI (include/spslam_gpu.h), Tracking::Relocalization's PnPsolver between SearchByBoW(KeyFrame, Frame) and
// PoseOptimization: spslam_pnp_ransac_table, spslam_pnp_solver[_batch_device].  The host form checks every index,
// octave, parameter and the draw count before anything is staged.
#include "capi_ctx.h"
#include "pnp_launch.h"

#include <cmath>
#include <cstring>

namespace {

const char* pnp_check_params(const spslam_pnp_params* p) {
    if (!p) return "the parameters are missing";
    if (p->min_set != 4) return "min_set is not 4";
    if (p->min_inliers < 1) return "min_inliers below 1";
    if (p->max_iterations < 1 || p->max_iterations > SPSLAM_PNP_MAX_ITERATIONS) return "max_iterations outside 1 .. 4096";
    if (p->rand_max < 1) return "rand_max below 1";
    if (!(p->epsilon > 0.f && p->epsilon <= 1.f)) return "epsilon outside (0, 1]";
    if (!(p->th2 > 0.f)) return "th2 is not positive";
    return nullptr;
}

// what the host form follows: the frame's keypoints, the match list, the keyframe's point rows, the state, the draws
const char* pnp_check_problem(const spslam_keypoint* keys_un, int n_frame, const int32_t* match,
                              const int32_t* kf_match_row, int n_kf, int n_rows, int n_levels, const int32_t* rand,
                              const spslam_pnp_params* p, double probability, const spslam_pnp_problem* q) {
    if (const char* e = pnp_check_params(p)) return e;
    if (n_frame < 0 || n_frame > 8192 || n_kf < 0 || n_kf > 8192) return "n outside 0 .. 8192";
    if (n_frame && (!keys_un || !match)) return "a frame array is missing";
    if (n_kf && !kf_match_row) return "the keyframe's map points are missing";
    if (!(probability > 0.0 && probability < 1.0)) return "probability outside (0, 1)";
    if (!q) return "the problem is missing";
    if (q->n_iterations < 0 || q->n_iterations > p->max_iterations) return "n_iterations outside 0 .. max_iterations";
    if (q->iterations_done < 0 || q->best_inliers < 0) return "the solver's state is negative";
    if (q->rand_iterations < 1 || q->rand_iterations > (1 << 24)) return "too few draws";
    if (!rand) return "the draws are missing";
    for (int i = 0; i < n_kf; i++)
        if (kf_match_row[i] < -1 || kf_match_row[i] >= n_rows) return "a map point outside the table";
    for (int i = 0; i < n_frame; i++) {
        if (match[i] < -1 || match[i] >= n_kf) return "a match entry outside the keyframe's keypoints";
        if (keys_un[i].octave < 0 || keys_un[i].octave >= n_levels) return "an octave outside the configured levels";
    }
    for (int i = 0; i < 4 * q->rand_iterations; i++)
        if (rand[i] < 0 || rand[i] > p->rand_max) return "a draw outside 0 .. rand_max";
    return nullptr;
}

}  // namespace

extern "C" {

int spslam_pnp_ransac_table(double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                            int cap, int32_t* max_its, int32_t* min_inliers_n) {
    if (!max_its || !min_inliers_n || cap < 0 || min_inliers < 1 || max_iterations < 1 || min_set < 1)
        return SPSLAM_ERR_ARG;
    for (int n = 0; n <= cap; n++) {
        int m = n * epsilon;                                                   // :134, an int times a float
        if (m < min_inliers) m = min_inliers;
        if (m < min_set) m = min_set;
        min_inliers_n[n] = m;
        if (n < m) { max_its[n] = 0; continue; }                               // :173
        double its = 1.0;                                                      // :147-148
        if (m != n) {
            float eps = epsilon;
            if (eps < (float)m / n) eps = (float)m / n;                        // :141-142
            its = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)eps, 3)));   // :150
        }
        const int n_iterations = its < (double)max_iterations ? (int)its : max_iterations;
        max_its[n] = std::max(1, n_iterations);                                // :152
    }
    return SPSLAM_OK;
}

int spslam_pnp_solver_batch_device(spslam_ctx* c, int n_problems, const spslam_pnp_problem* d_problems,
                                   const spslam_sim3_map* map, const spslam_keypoint* d_frame_keys_un,
                                   const int* d_frame_counts, int cap, const int32_t* d_match, const int32_t* d_rand,
                                   const int32_t* d_max_its_table, const int32_t* d_min_inliers_table,
                                   const spslam_pnp_params* params, spslam_pnp_result* d_results, uint8_t* d_inliers,
                                   uint8_t* d_best_mask, int32_t* d_frame_points, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    if (n_problems < 1 || n_problems > 65535 || !d_problems || !map || !map->match_off || !map->match_row ||
        !map->points || !d_frame_keys_un || !d_frame_counts || cap < 1 || cap > 8192 || !d_match || !d_rand ||
        !d_max_its_table || !d_min_inliers_table || pnp_check_params(params) || !d_results || !d_inliers ||
        !d_best_mask)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_pnp_solver_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    PnpConsts P{};
    P.fx = c->fg.fx; P.fy = c->fg.fy; P.cx = c->fg.cx; P.cy = c->fg.cy;
    for (int l = 0; l < 8; l++) P.max_error[l] = l < c->p.nlevels ? c->sigma2[l] * params->th2 : 0.f;   // :156, float
    P.max_iterations = params->max_iterations;
    P.rand_max = params->rand_max;
    HIP_CHECK(c, c->d_loop_scratch.reserve(pnp_scratch_bytes(n_problems, cap, params->max_iterations), s));
    HIP_CHECK(c, pnp_solver_launch(n_problems, d_problems, *map, d_frame_keys_un, d_frame_counts, cap, d_match, d_rand,
                                   d_max_its_table, d_min_inliers_table, P, c->d_loop_scratch.p, d_results, d_inliers,
                                   d_best_mask, d_frame_points, s));
    return SPSLAM_OK;
}

int spslam_pnp_solver(spslam_ctx* c, const spslam_keypoint* keys_un, int n_frame, const int32_t* match,
                      const int32_t* kf_match_row, int n_kf, const spslam_local_point* points,
                      const uint8_t* point_bad, int n_rows, const int32_t* rand, const spslam_pnp_params* params,
                      double probability, const spslam_pnp_problem* problem, spslam_pnp_result* result,
                      uint8_t* inliers, uint8_t* best_mask, int32_t* frame_points) {
    if (!c || !result || n_rows < 0 || (n_rows && !points)) return SPSLAM_ERR_ARG;
    if (const char* e = pnp_check_problem(keys_un, n_frame, match, kf_match_row, n_kf, n_rows, c->p.nlevels, rand,
                                          params, probability, problem))
        return fail(c, SPSLAM_ERR_ARG, "spslam_pnp_solver: %s", e);
    if (n_frame && (!inliers || !best_mask)) return fail(c, SPSLAM_ERR_ARG, "spslam_pnp_solver: %s", "an output is missing");
    HIP_CHECK(c, hipSetDevice(c->device));
    // the frame as slot 0 of cap keypoints, the keyframe as keyframe 0 of a one-keyframe map
    const int cap = std::max(n_frame, 1);
    const size_t C = (size_t)cap, R = (size_t)std::max(n_rows, 1), KF = (size_t)std::max(n_kf, 1);
    std::vector<int32_t> max_its(C + 1), min_n(C + 1);
    spslam_pnp_ransac_table(probability, params->min_inliers, params->max_iterations, params->min_set, params->epsilon,
                            cap, max_its.data(), min_n.data());
    const int32_t off[2] = {0, n_kf};
    spslam_pnp_problem Q = *problem;
    Q.kf = 0; Q.frame_slot = 0; Q.match_offset = 0; Q.rand_offset = 0; Q.inlier_offset = 0; Q.best_mask_offset = 0;
    enum { kKun, kCount, kOff, kRows, kBad, kPoints, kProblem, kMatch, kRand, kMaxIts, kMinN, kResult, kInliers, kMask,
           kFramePoints };
    Stage st(c);
    if (int rc = st.open({{keys_un, (size_t)n_frame * sizeof(spslam_keypoint), C * sizeof(spslam_keypoint)},
                          {&n_frame, 4}, {off, 8}, {kf_match_row, (size_t)n_kf * 4, KF * 4},
                          {point_bad, point_bad ? (size_t)n_rows : 0, R},
                          {points, (size_t)n_rows * sizeof(spslam_local_point), R * sizeof(spslam_local_point)},
                          {&Q, sizeof Q}, {match, (size_t)n_frame * 4, C * 4},
                          {rand, (size_t)Q.rand_iterations * 16}, {max_its.data(), max_its.size() * 4},
                          {min_n.data(), min_n.size() * 4}, sizeof(spslam_pnp_result), C,
                          {best_mask, (size_t)n_frame, C}, C * 4}))
        return rc;
    // the uploads read the vectors above: they must be done before those go out of scope
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    spslam_sim3_map M{nullptr, nullptr, st.slot<int32_t>(kOff), st.slot<int32_t>(kRows),
                      point_bad ? st.slot<uint8_t>(kBad) : nullptr, st.slot<spslam_local_point>(kPoints)};
    int rc = spslam_pnp_solver_batch_device(c, 1, st.slot<spslam_pnp_problem>(kProblem), &M,
                                            st.slot<spslam_keypoint>(kKun), st.slot<int>(kCount), cap,
                                            st.slot<int32_t>(kMatch), st.slot<int32_t>(kRand),
                                            st.slot<int32_t>(kMaxIts), st.slot<int32_t>(kMinN), params,
                                            st.slot<spslam_pnp_result>(kResult), st.slot<uint8_t>(kInliers),
                                            st.slot<uint8_t>(kMask), frame_points ? st.slot<int32_t>(kFramePoints) : nullptr,
                                            c->stream);
    if (rc) return rc;
    HIP_CHECK(c, hipMemcpyAsync(result, st.slot<void>(kResult), sizeof *result, hipMemcpyDeviceToHost, c->stream));
    if (n_frame) {
        HIP_CHECK(c, hipMemcpyAsync(inliers, st.slot<void>(kInliers), (size_t)n_frame, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(c, hipMemcpyAsync(best_mask, st.slot<void>(kMask), (size_t)n_frame, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    const bool pose = result->status == SPSLAM_PNP_REFINED || result->status == SPSLAM_PNP_BEST_NO_MORE;
    if (frame_points && n_frame && pose)
        HIP_CHECK(c, hipMemcpyAsync(frame_points, st.slot<void>(kFramePoints), (size_t)n_frame * 4,
                                    hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

}  // extern "C"
