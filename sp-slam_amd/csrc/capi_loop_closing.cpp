// C ABI (include/spslam_gpu.h), LoopClosing's ORBmatcher side (ComputeSim3, SearchAndFuse):
// spslam_search_by_bow_kf[_batch_device] (SearchByBoW(KeyFrame*, KeyFrame*)), spslam_search_by_sim3[_batch_device]
// (SearchBySim3), spslam_search_by_projection_sim3[_batch_device] (SearchByProjection(pKF, Scw, ...)) and
// spslam_fuse_sim3_search[_batch_device] (the search of Fuse(pKF, Scw, ...)), and Sim3Solver between the first two:
// spslam_sim3_ransac_table, spslam_sim3_solver[_batch_device], and Optimizer::OptimizeSim3 with Scw after SearchBySim3:
// spslam_sim3_optimize[_batch_device].  The host forms check their indices with loop_check.h before anything is staged.
#include "capi_ctx.h"
#include "loop_check.h"
#include "sim3_launch.h"
#include "sim3_opt_launch.h"

#include <cmath>
#include <cstring>

namespace {

// The keyframe's geometry and the constants of the three projection searches: KeyFrame's mnMinX .. mnMaxY are ints
// initialised from the Frame's floats (KeyFrame.cc:41, KeyFrame.h:198-201).
MatchGeom keyframe_geom(const spslam_ctx* c) {
    MatchGeom g = match_geom(c);
    g.min_x = (float)(int)g.min_x; g.max_x = (float)(int)g.max_x;
    g.min_y = (float)(int)g.min_y; g.max_y = (float)(int)g.max_y;
    return g;
}

FuseConsts search_consts(const spslam_ctx* c, float th) {
    FuseConsts P{};
    P.th = th;
    P.log_scale_factor = std::log(c->p.scale_factor);  // mfLogScaleFactor, float
    P.n_levels = c->p.nlevels;
    level_table(c, c->inv_sigma2, P.inv_sigma2);
    return P;
}

// the keyframe slots of the projection searches' batch forms: no uright
bool slots_ok(const MatchCurrent& m) {
    return m.kun && m.desc && m.grid_off && m.grid_idx && m.counts && m.cap >= 1 && m.cap <= (1 << 20);
}

// One keyframe of a host form as slot 0 of the batch layouts, cap = max(n_kp, 1): slots first .. first + 4 of a
// stage are keys_un, desc, grid_off, grid_idx, count.
struct SlotStage {
    const spslam_keypoint* keys_un;
    const uint8_t* desc;
    int n_kp;
    const int32_t* grid_off;
    const int32_t* grid_idx;
    int cap() const { return std::max(n_kp, 1); }
    void slots(std::vector<StageSlot>& out) const {
        const size_t K = (size_t)n_kp, C = (size_t)cap();
        out.insert(out.end(), {{keys_un, K * sizeof(spslam_keypoint), C * sizeof(spslam_keypoint)},
                               {desc, K * 32, C * 32},
                               {grid_off, (kLoopGridCells + 1) * 4},
                               {grid_idx, (size_t)grid_off[kLoopGridCells] * 4, C * 4},
                               {&n_kp, sizeof(int)}});
    }
    MatchCurrent current(const Stage& st, int first) const {
        return {st.slot<spslam_keypoint>(first), st.slot<uint8_t>(first + 1), nullptr, st.slot<int32_t>(first + 2),
                st.slot<int32_t>(first + 3), st.slot<int>(first + 4), cap()};
    }
};

}  // namespace

extern "C" {

// ---------------------------------------------------------------- SearchByBoW(KeyFrame*, KeyFrame*)
int spslam_search_by_bow_kf_batch_device(spslam_ctx* c, int n_pairs, const int32_t* d_pairs,
                                         const spslam_bow_side* kf1, const spslam_bow_side* kf2,
                                         const spslam_bow_params* params, int32_t* d_match12, int* d_nmatches,
                                         void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    auto side_ok = [](const spslam_bow_side* b) {
        return b && b->desc && b->keys && b->has_point && b->counts && b->fv_nodes && b->fv_start && b->fv_features &&
               b->n_fv && b->cap >= 1 && b->cap <= 8192;
    };
    if (n_pairs < 1 || !d_pairs || !side_ok(kf1) || !side_ok(kf2) || !params || !d_match12 || !d_nmatches)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_search_by_bow_kf_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    auto side = [](const spslam_bow_side* b) {
        return BowSide{b->desc, b->keys, b->has_point, b->counts, b->fv_nodes, b->fv_start, b->fv_features, b->n_fv,
                       b->cap};
    };
    HIP_CHECK(c, bow_search_kf_launch(n_pairs, (const int2*)d_pairs, side(kf1), side(kf2), params->nn_ratio,
                                      params->check_orientation, d_match12, d_nmatches, (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_search_by_bow_kf(spslam_ctx* c, const spslam_bow_keyframe* kf1, const spslam_bow_keyframe* kf2,
                            const spslam_bow_params* params, int32_t* match12, int* nmatches) {
    if (!c || !params || !nmatches) return SPSLAM_ERR_ARG;
    const spslam_bow_keyframe* k[2] = {kf1, kf2};
    for (int s = 0; s < 2; s++)
        if (const char* e = loop_check_bow_keyframe(k[s])) return fail(c, SPSLAM_ERR_ARG, "spslam_search_by_bow_kf: %s", e);
    if (kf1->n && !match12) return fail(c, SPSLAM_ERR_ARG, "spslam_search_by_bow_kf: %s", "match12 is missing");
    HIP_CHECK(c, hipSetDevice(c->device));
    // each keyframe is slot 0 of a side of its own capacity; one pair (0, 0)
    const int32_t pair[2] = {0, 0};
    constexpr size_t kKp = sizeof(spslam_keypoint);
    std::vector<StageSlot> slots;
    for (int s = 0; s < 2; s++) {
        const spslam_bow_keyframe& q = *k[s];
        const size_t n = (size_t)q.n, C = (size_t)std::max(q.n, 1), nf = (size_t)q.n_fv, m = (size_t)q.fv_start[q.n_fv];
        slots.insert(slots.end(), {{q.desc, n * 32, C * 32}, {q.keys_un, n * kKp, C * kKp}, {q.has_point, n, C},
                                   {&q.n, 4}, {q.fv_nodes, nf * 4, C * 4}, {q.fv_start, (nf + 1) * 4, (C + 1) * 4},
                                   {q.fv_features, m * 4, C * 4}, {&q.n_fv, 4}});
    }
    const size_t C1 = (size_t)std::max(kf1->n, 1);
    slots.insert(slots.end(), {{pair, 8}, C1 * 4, 4});
    enum { kPair = 16, kMatch, kCount };
    Stage st(c);
    if (int rc = st.open(slots.data(), (int)slots.size(), &c->d_bow_stage)) return rc;
    spslam_bow_side S[2];
    for (int s = 0; s < 2; s++)
        S[s] = spslam_bow_side{st.slot<uint8_t>(8 * s), st.slot<spslam_keypoint>(8 * s + 1), st.slot<uint8_t>(8 * s + 2),
                               st.slot<int>(8 * s + 3), st.slot<uint32_t>(8 * s + 4), st.slot<int32_t>(8 * s + 5),
                               st.slot<int32_t>(8 * s + 6), st.slot<int>(8 * s + 7), std::max(k[s]->n, 1), 0};
    int rc = spslam_search_by_bow_kf_batch_device(c, 1, st.slot<int32_t>(kPair), &S[0], &S[1], params,
                                                  st.slot<int32_t>(kMatch), st.slot<int>(kCount), c->stream);
    if (rc) return rc;
    if (kf1->n)
        HIP_CHECK(c, hipMemcpyAsync(match12, st.slot<int32_t>(kMatch), (size_t)kf1->n * 4, hipMemcpyDeviceToHost,
                                    c->stream));
    HIP_CHECK(c, hipMemcpyAsync(nmatches, st.slot<int>(kCount), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

// ---------------------------------------------------------------- SearchBySim3
int spslam_search_by_sim3_batch_device(spslam_ctx* c, int n_pairs, const spslam_sim3_pair* d_pairs,
                                       const spslam_sim3_map* map, const spslam_keypoint* d_keys_un,
                                       const uint8_t* d_desc, const int32_t* d_grid_off, const int32_t* d_grid_idx,
                                       const int* d_counts, int cap, const uint8_t* d_already2,
                                       const spslam_sim3_params* params, int32_t* d_match12, int* d_n_found,
                                       void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    const MatchCurrent cur{d_keys_un, d_desc, nullptr, d_grid_off, d_grid_idx, d_counts, cap};
    if (n_pairs < 1 || n_pairs > 65535 || !d_pairs || !map || !map->kf_Tcw || !map->kf_slot || !map->match_off ||
        !map->match_row || !map->points || !slots_ok(cur) || !params || !d_match12 || !d_n_found)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_search_by_sim3_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    // vnMatch1 / vnMatch2 (2 * cap ints per pair), then vbAlreadyMatched2 (cap bytes per pair)
    const size_t vn_bytes = (size_t)n_pairs * 2 * cap * 4;
    HIP_CHECK(c, c->d_loop_scratch.reserve(vn_bytes + (size_t)n_pairs * cap, s));
    HIP_CHECK(c, sim3_search_launch(n_pairs, d_pairs, *map, cur, keyframe_geom(c), search_consts(c, params->th),
                                    d_already2, (int32_t*)c->d_loop_scratch.p, c->d_loop_scratch + vn_bytes, d_match12,
                                    d_n_found, s));
    return SPSLAM_OK;
}

int spslam_search_by_sim3(spslam_ctx* c, const spslam_sim3_keyframe* kf1, const spslam_sim3_keyframe* kf2,
                          const spslam_local_point* points, const uint8_t* point_bad, int n_rows,
                          const spslam_sim3_pair* pair, const uint8_t* already2, const spslam_sim3_params* params,
                          int32_t* match12, int* n_found) {
    if (!c || !pair || !params || !n_found || n_rows < 0 || (n_rows && !points)) return SPSLAM_ERR_ARG;
    const spslam_sim3_keyframe* k[2] = {kf1, kf2};
    for (int s = 0; s < 2; s++)
        if (const char* e = loop_check_sim3_keyframe(k[s], n_rows)) return fail(c, SPSLAM_ERR_ARG, "spslam_search_by_sim3: %s", e);
    if (const char* e = loop_check_match12(match12, kf1->n, kf2->n)) return fail(c, SPSLAM_ERR_ARG, "spslam_search_by_sim3: %s", e);
    HIP_CHECK(c, hipSetDevice(c->device));
    // the two keyframes as slots 0 and 1 of cap keypoints, keyframes 0 and 1 of a two-keyframe map
    const int cap = std::max(std::max(kf1->n, kf2->n), 1);
    const size_t C = (size_t)cap, kKp = sizeof(spslam_keypoint), R = (size_t)std::max(n_rows, 1);
    std::vector<uint8_t> kun(2 * C * kKp, 0), desc(2 * C * 32, 0), already(C, 0);
    std::vector<int32_t> go(2 * (kLoopGridCells + 1), 0), gi(2 * C, 0), rows(2 * C, -1);
    float Tcw[32];
    const int32_t counts[2] = {kf1->n, kf2->n}, slot[2] = {0, 1}, off[3] = {0, cap, 2 * cap};
    for (int s = 0; s < 2; s++) {
        const spslam_sim3_keyframe& q = *k[s];
        const size_t n = (size_t)q.n;
        if (n) {
            std::memcpy(kun.data() + s * C * kKp, q.keys_un, n * kKp);
            std::memcpy(desc.data() + s * C * 32, q.desc, n * 32);
            std::memcpy(rows.data() + s * C, q.match_row, n * 4);
        }
        std::memcpy(go.data() + s * (kLoopGridCells + 1), q.grid_off, (kLoopGridCells + 1) * 4);
        if (q.grid_off[kLoopGridCells]) std::memcpy(gi.data() + s * C, q.grid_idx, (size_t)q.grid_off[kLoopGridCells] * 4);
        std::memcpy(Tcw + 16 * s, q.Tcw, 64);
    }
    if (already2 && kf2->n) std::memcpy(already.data(), already2, (size_t)kf2->n);
    spslam_sim3_pair P = *pair;
    P.kf1 = 0; P.kf2 = 1; P.match_offset = 0; P.result_offset = 0;
    enum { kKun, kDesc, kGo, kGi, kCounts, kTcw, kSlot, kOff, kRows, kBad, kPoints, kPair, kAlready, kMatch, kFound };
    Stage st(c);
    if (int rc = st.open({{kun.data(), kun.size()}, {desc.data(), desc.size()}, {go.data(), go.size() * 4},
                          {gi.data(), gi.size() * 4}, {counts, 8}, {Tcw, 128}, {slot, 8}, {off, 12},
                          {rows.data(), rows.size() * 4}, {point_bad, point_bad ? (size_t)n_rows : 0, R},
                          {points, (size_t)n_rows * sizeof(spslam_local_point), R * sizeof(spslam_local_point)},
                          {&P, sizeof P}, {already.data(), C}, {match12, (size_t)kf1->n * 4, C * 4}, 4}))
        return rc;
    // the uploads read the vectors above: they must be done before those go out of scope
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    spslam_sim3_map M{st.slot<float>(kTcw), st.slot<int32_t>(kSlot), st.slot<int32_t>(kOff), st.slot<int32_t>(kRows),
                      point_bad ? st.slot<uint8_t>(kBad) : nullptr, st.slot<spslam_local_point>(kPoints)};
    int rc = spslam_search_by_sim3_batch_device(c, 1, st.slot<spslam_sim3_pair>(kPair), &M, st.slot<spslam_keypoint>(kKun),
                                                st.slot<uint8_t>(kDesc), st.slot<int32_t>(kGo), st.slot<int32_t>(kGi),
                                                st.slot<int>(kCounts), cap, already2 ? st.slot<uint8_t>(kAlready) : nullptr,
                                                params, st.slot<int32_t>(kMatch), st.slot<int>(kFound), c->stream);
    if (rc) return rc;
    if (kf1->n)
        HIP_CHECK(c, hipMemcpyAsync(match12, st.slot<void>(kMatch), (size_t)kf1->n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(n_found, st.slot<int>(kFound), 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

// ---------------------------------------------------------------- Sim3Solver
int spslam_sim3_ransac_table(double probability, int min_inliers, int max_iterations, int cap, int32_t* table) {
    if (!table || cap < 0 || min_inliers < 1 || max_iterations < 1) return SPSLAM_ERR_ARG;
    for (int n = 0; n <= cap; n++) {
        if (n < min_inliers) { table[n] = 0; continue; }
        double its = 1.0;                                                      // :130-131
        if (n != min_inliers) {
            const float epsilon = (float)min_inliers / n;                      // :125
            its = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3)));   // :133
        }
        const int n_iterations = its < (double)max_iterations ? (int)its : max_iterations;   // min(nIterations, mRansacMaxIts)
        table[n] = std::max(1, n_iterations);
    }
    return SPSLAM_OK;
}

int spslam_sim3_solver_batch_device(spslam_ctx* c, int n_problems, const spslam_sim3_problem* d_problems,
                                    const spslam_sim3_map* map, const spslam_keypoint* d_keys_un, const int* d_counts,
                                    int cap, const int32_t* d_match12, const int32_t* d_rand,
                                    const int32_t* d_max_its_table, const spslam_sim3_solver_params* params,
                                    spslam_sim3_result* d_results, uint8_t* d_inliers, spslam_sim3_pair* d_pairs_out,
                                    int32_t* d_match12_out, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    if (n_problems < 1 || n_problems > 65535 || !d_problems || !map || !map->kf_Tcw || !map->kf_slot ||
        !map->match_off || !map->match_row || !map->points || !d_keys_un || !d_counts || cap < 1 || cap > 8192 ||
        !d_match12 || !d_rand || !d_max_its_table || !params || params->min_inliers < 3 ||
        params->max_iterations < 1 || params->max_iterations > SPSLAM_SIM3_MAX_ITERATIONS || params->rand_max < 1 ||
        !d_results || !d_inliers)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_sim3_solver_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    SolverConsts P{};
    P.fx = c->fg.fx; P.fy = c->fg.fy; P.cx = c->fg.cx; P.cy = c->fg.cy;
    for (int l = 0; l < 8; l++)  // mvnMaxError is a vector<size_t>: the double product truncated (:87-88)
        P.max_error[l] = l < c->p.nlevels ? (float)(size_t)(9.210 * c->sigma2[l]) : 0.f;
    P.min_inliers = params->min_inliers; P.max_iterations = params->max_iterations;
    P.rand_max = params->rand_max; P.fix_scale = params->fix_scale;
    HIP_CHECK(c, c->d_loop_scratch.reserve(sim3_scratch_bytes(n_problems, cap, params->max_iterations), s));
    HIP_CHECK(c, sim3_solver_launch(n_problems, d_problems, *map, d_keys_un, d_counts, cap, d_match12, d_rand,
                                    d_max_its_table, P, c->d_loop_scratch.p, d_results, d_inliers, d_pairs_out,
                                    d_match12_out, s));
    return SPSLAM_OK;
}

int spslam_sim3_solver(spslam_ctx* c, const spslam_sim3_keyframe* kf1, const spslam_sim3_keyframe* kf2,
                       const spslam_local_point* points, const uint8_t* point_bad, int n_rows,
                       const int32_t* match12, const int32_t* rand, const spslam_sim3_solver_params* params,
                       double probability, int n_iterations, int* iterations_done, int* best_inliers,
                       spslam_sim3_result* result, uint8_t* inliers, int32_t* match12_out) {
    if (!c || !result || n_rows < 0 || (n_rows && !points)) return SPSLAM_ERR_ARG;
    const spslam_sim3_keyframe* k[2] = {kf1, kf2};
    for (int s = 0; s < 2; s++)
        if (const char* e = loop_check_solver_keyframe(k[s], n_rows, c->p.nlevels)) return fail(c, SPSLAM_ERR_ARG, "spslam_sim3_solver: %s", e);
    if (const char* e = loop_check_match12(match12, kf1->n, kf2->n)) return fail(c, SPSLAM_ERR_ARG, "spslam_sim3_solver: %s", e);
    if (const char* e = loop_check_solver_call(params, probability, n_iterations, iterations_done, best_inliers, rand))
        return fail(c, SPSLAM_ERR_ARG, "spslam_sim3_solver: %s", e);
    if (kf1->n && !inliers) return fail(c, SPSLAM_ERR_ARG, "spslam_sim3_solver: %s", "inliers is missing");
    HIP_CHECK(c, hipSetDevice(c->device));
    // the two keyframes as slots 0 and 1 of cap keypoints, keyframes 0 and 1 of a two-keyframe map
    const int cap = std::max(std::max(kf1->n, kf2->n), 1);
    const size_t C = (size_t)cap, R = (size_t)std::max(n_rows, 1);
    std::vector<spslam_keypoint> kun(2 * C);
    std::vector<int32_t> rows(2 * C, -1), table(C + 1);
    float Tcw[32];
    const int32_t counts[2] = {kf1->n, kf2->n}, slot[2] = {0, 1}, off[3] = {0, cap, 2 * cap};
    for (int s = 0; s < 2; s++) {
        if (k[s]->n) {
            std::memcpy(kun.data() + s * C, k[s]->keys_un, (size_t)k[s]->n * sizeof(spslam_keypoint));
            std::memcpy(rows.data() + s * C, k[s]->match_row, (size_t)k[s]->n * 4);
        }
        std::memcpy(Tcw + 16 * s, k[s]->Tcw, 64);
    }
    spslam_sim3_ransac_table(probability, params->min_inliers, params->max_iterations, cap, table.data());
    spslam_sim3_problem Q{};
    Q.kf1 = 0; Q.kf2 = 1;
    Q.iterations_done = *iterations_done; Q.best_inliers = *best_inliers; Q.n_iterations = n_iterations;
    enum { kKun, kCounts, kTcw, kSlot, kOff, kRows, kBad, kPoints, kProblem, kMatch, kRand, kTable, kResult, kInliers,
           kMatchOut };
    Stage st(c);
    if (int rc = st.open({{kun.data(), kun.size() * sizeof(spslam_keypoint)}, {counts, 8}, {Tcw, 128}, {slot, 8},
                          {off, 12}, {rows.data(), rows.size() * 4}, {point_bad, point_bad ? (size_t)n_rows : 0, R},
                          {points, (size_t)n_rows * sizeof(spslam_local_point), R * sizeof(spslam_local_point)},
                          {&Q, sizeof Q}, {match12, (size_t)kf1->n * 4, C * 4},
                          {rand, (size_t)params->max_iterations * 12}, {table.data(), table.size() * 4},
                          sizeof(spslam_sim3_result), C, C * 4}))
        return rc;
    // the uploads read the vectors above: they must be done before those go out of scope
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    spslam_sim3_map M{st.slot<float>(kTcw), st.slot<int32_t>(kSlot), st.slot<int32_t>(kOff), st.slot<int32_t>(kRows),
                      point_bad ? st.slot<uint8_t>(kBad) : nullptr, st.slot<spslam_local_point>(kPoints)};
    int rc = spslam_sim3_solver_batch_device(c, 1, st.slot<spslam_sim3_problem>(kProblem), &M,
                                             st.slot<spslam_keypoint>(kKun), st.slot<int>(kCounts), cap,
                                             st.slot<int32_t>(kMatch), st.slot<int32_t>(kRand), st.slot<int32_t>(kTable),
                                             params, st.slot<spslam_sim3_result>(kResult), st.slot<uint8_t>(kInliers),
                                             nullptr, match12_out ? st.slot<int32_t>(kMatchOut) : nullptr, c->stream);
    if (rc) return rc;
    HIP_CHECK(c, hipMemcpyAsync(result, st.slot<void>(kResult), sizeof *result, hipMemcpyDeviceToHost, c->stream));
    if (kf1->n)
        HIP_CHECK(c, hipMemcpyAsync(inliers, st.slot<void>(kInliers), (size_t)kf1->n, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    if (match12_out && kf1->n && result->status == SPSLAM_SIM3_FOUND)
        HIP_CHECK(c, hipMemcpyAsync(match12_out, st.slot<void>(kMatchOut), (size_t)kf1->n * 4, hipMemcpyDeviceToHost,
                                    c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    *iterations_done = result->iterations_done;
    *best_inliers = result->best_inliers;
    return SPSLAM_OK;
}

// ---------------------------------------------------------------- Optimizer::OptimizeSim3 and Scw
int spslam_sim3_optimize_batch_device(spslam_ctx* c, int n_pairs, const spslam_sim3_pair* d_pairs,
                                      const spslam_sim3_map* map, const spslam_keypoint* d_keys_un, const int* d_counts,
                                      int cap, const spslam_sim3_opt_params* params, int32_t* d_match12,
                                      spslam_sim3_opt_result* d_results, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    // fix_scale = 0 needs a correctly rounded exp (include/spslam_gpu.h): refused before anything is launched
    if (n_pairs < 1 || n_pairs > 65535 || !d_pairs || !map || !map->kf_Tcw || !map->kf_slot || !map->match_off ||
        !map->match_row || !map->points || !d_keys_un || !d_counts || cap < 1 || cap > 8192 || !params ||
        params->fix_scale != 1 || !(params->th2 > 0.f) || !d_match12 || !d_results)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_sim3_optimize_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    Sim3OptConsts P{};
    P.fx = c->fg.fx; P.fy = c->fg.fy; P.cx = c->fg.cx; P.cy = c->fg.cy;
    level_table(c, c->inv_sigma2, P.inv_sigma2);
    P.th2 = params->th2;
    P.min_inliers = params->min_inliers;
    HIP_CHECK(c, c->d_loop_scratch.reserve(sim3_opt_scratch_bytes(n_pairs, cap), s));
    HIP_CHECK(c, sim3_opt_launch(n_pairs, d_pairs, *map, d_keys_un, d_counts, cap, P, c->d_loop_scratch.p, d_match12,
                                 d_results, s));
    return SPSLAM_OK;
}

int spslam_sim3_optimize(spslam_ctx* c, const spslam_sim3_keyframe* kf1, const spslam_sim3_keyframe* kf2,
                         const spslam_local_point* points, const uint8_t* point_bad, int n_rows,
                         const spslam_sim3_pair* pair, const spslam_sim3_opt_params* params, int32_t* match12,
                         spslam_sim3_opt_result* result) {
    if (!c || !result || n_rows < 0 || (n_rows && !points)) return SPSLAM_ERR_ARG;
    const spslam_sim3_keyframe* k[2] = {kf1, kf2};
    for (int s = 0; s < 2; s++)
        if (const char* e = loop_check_solver_keyframe(k[s], n_rows, c->p.nlevels)) return fail(c, SPSLAM_ERR_ARG, "spslam_sim3_optimize: %s", e);
    if (const char* e = loop_check_match12(match12, kf1->n, kf2->n)) return fail(c, SPSLAM_ERR_ARG, "spslam_sim3_optimize: %s", e);
    if (const char* e = loop_check_opt_call(params, pair)) return fail(c, SPSLAM_ERR_ARG, "spslam_sim3_optimize: %s", e);
    HIP_CHECK(c, hipSetDevice(c->device));
    // the two keyframes as slots 0 and 1 of cap keypoints, keyframes 0 and 1 of a two-keyframe map
    const int cap = std::max(std::max(kf1->n, kf2->n), 1);
    const size_t C = (size_t)cap, R = (size_t)std::max(n_rows, 1);
    std::vector<spslam_keypoint> kun(2 * C);
    std::vector<int32_t> rows(2 * C, -1);
    float Tcw[32];
    const int32_t counts[2] = {kf1->n, kf2->n}, slot[2] = {0, 1}, off[3] = {0, cap, 2 * cap};
    for (int s = 0; s < 2; s++) {
        if (k[s]->n) {
            std::memcpy(kun.data() + s * C, k[s]->keys_un, (size_t)k[s]->n * sizeof(spslam_keypoint));
            std::memcpy(rows.data() + s * C, k[s]->match_row, (size_t)k[s]->n * 4);
        }
        std::memcpy(Tcw + 16 * s, k[s]->Tcw, 64);
    }
    spslam_sim3_pair Q = *pair;
    Q.kf1 = 0; Q.kf2 = 1; Q.match_offset = 0; Q.result_offset = 0;
    enum { kKun, kCounts, kTcw, kSlot, kOff, kRows, kBad, kPoints, kPair, kMatch, kResult };
    Stage st(c);
    if (int rc = st.open({{kun.data(), kun.size() * sizeof(spslam_keypoint)}, {counts, 8}, {Tcw, 128}, {slot, 8},
                          {off, 12}, {rows.data(), rows.size() * 4}, {point_bad, point_bad ? (size_t)n_rows : 0, R},
                          {points, (size_t)n_rows * sizeof(spslam_local_point), R * sizeof(spslam_local_point)},
                          {&Q, sizeof Q}, {match12, (size_t)kf1->n * 4, C * 4}, sizeof(spslam_sim3_opt_result)}))
        return rc;
    // the uploads read the vectors above: they must be done before those go out of scope
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    spslam_sim3_map M{st.slot<float>(kTcw), st.slot<int32_t>(kSlot), st.slot<int32_t>(kOff), st.slot<int32_t>(kRows),
                      point_bad ? st.slot<uint8_t>(kBad) : nullptr, st.slot<spslam_local_point>(kPoints)};
    int rc = spslam_sim3_optimize_batch_device(c, 1, st.slot<spslam_sim3_pair>(kPair), &M, st.slot<spslam_keypoint>(kKun),
                                               st.slot<int>(kCounts), cap, params, st.slot<int32_t>(kMatch),
                                               st.slot<spslam_sim3_opt_result>(kResult), c->stream);
    if (rc) return rc;
    HIP_CHECK(c, hipMemcpyAsync(result, st.slot<void>(kResult), sizeof *result, hipMemcpyDeviceToHost, c->stream));
    if (kf1->n)
        HIP_CHECK(c, hipMemcpyAsync(match12, st.slot<void>(kMatch), (size_t)kf1->n * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

int spslam_debug_fill_loop_scratch(spslam_ctx* c, int value) {
    if (!c) return SPSLAM_ERR_ARG;
    HIP_CHECK(c, hipSetDevice(c->device));
    if (c->d_loop_scratch.cap) {
        HIP_CHECK(c, hipMemsetAsync(c->d_loop_scratch.p, value, c->d_loop_scratch.cap, c->stream));
        HIP_CHECK(c, hipStreamSynchronize(c->stream));
    }
    return SPSLAM_OK;
}

// ---------------------------------------------------------------- Fuse(pKF, Scw, ...), the search
int spslam_fuse_sim3_search_batch_device(spslam_ctx* c, int n_problems, const spslam_fuse_problem* d_problems,
                                         const spslam_local_point* d_points, int max_points,
                                         const spslam_keypoint* d_keys_un, const uint8_t* d_desc,
                                         const int32_t* d_grid_off, const int32_t* d_grid_idx, const int* d_counts,
                                         int cap, const uint8_t* d_skip, const spslam_fuse_params* params,
                                         spslam_fuse_result* d_results, int* d_nfused, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    const MatchCurrent cur{d_keys_un, d_desc, nullptr, d_grid_off, d_grid_idx, d_counts, cap};
    if (n_problems < 1 || n_problems > 65535 || !d_problems || max_points < 0 ||
        (max_points > 0 && (!d_points || !d_results)) || !slots_ok(cur) || !params || !d_nfused)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_fuse_sim3_search_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, fuse_sim3_search_launch(n_problems, d_problems, d_points, max_points, cur, keyframe_geom(c),
                                         search_consts(c, params->th), d_skip, d_results, d_nfused,
                                         (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_fuse_sim3_search(spslam_ctx* c, const float* Scw, const spslam_local_point* points, int n_points,
                            const spslam_keypoint* keys_un, const uint8_t* desc, int n_kp, const int32_t* grid_off,
                            const int32_t* grid_idx, const uint8_t* skip, const spslam_fuse_params* params,
                            spslam_fuse_result* results, int* nfused) {
    if (!c || !params || !nfused || (n_points > 0 && !results)) return SPSLAM_ERR_ARG;
    if (const char* e = loop_check_scw_problem(Scw, points, n_points, keys_un, desc, n_kp, grid_off, grid_idx))
        return fail(c, SPSLAM_ERR_ARG, "spslam_fuse_sim3_search: %s", e);
    HIP_CHECK(c, hipSetDevice(c->device));
    spslam_fuse_problem F{};
    std::memcpy(F.Tcw, Scw, sizeof F.Tcw);
    F.n_points = n_points;
    const int np = n_points;
    const size_t N = (size_t)std::max(np, 1);
    const SlotStage kf{keys_un, desc, n_kp, grid_off, grid_idx};
    std::vector<StageSlot> slots;
    kf.slots(slots);
    enum { kProblem = 5, kPoints, kSkip, kResults, kNFused };
    slots.insert(slots.end(), {{&F, sizeof F}, {points, np * sizeof(spslam_local_point), N * sizeof(spslam_local_point)},
                               {skip, skip ? (size_t)np : 0, N}, N * sizeof(spslam_fuse_result), sizeof(int)});
    Stage st(c);
    if (int rc = st.open(slots.data(), (int)slots.size())) return rc;
    const MatchCurrent d = kf.current(st, 0);
    int rc = spslam_fuse_sim3_search_batch_device(
        c, 1, st.slot<spslam_fuse_problem>(kProblem), st.slot<spslam_local_point>(kPoints), np, d.kun, d.desc, d.grid_off,
        d.grid_idx, d.counts, d.cap, skip ? st.slot<uint8_t>(kSkip) : nullptr, params,
        st.slot<spslam_fuse_result>(kResults), st.slot<int>(kNFused), c->stream);
    if (rc) return rc;
    if (np)
        HIP_CHECK(c, hipMemcpyAsync(results, st.slot<void>(kResults), (size_t)np * sizeof(spslam_fuse_result),
                                    hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(nfused, st.slot<int>(kNFused), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

// ---------------------------------------------------------------- SearchByProjection(pKF, Scw, ...)
int spslam_search_by_projection_sim3_batch_device(spslam_ctx* c, int n_problems,
                                                  const spslam_fuse_problem* d_problems,
                                                  const spslam_local_point* d_points, int max_points,
                                                  const spslam_keypoint* d_keys_un, const uint8_t* d_desc,
                                                  const int32_t* d_grid_off, const int32_t* d_grid_idx,
                                                  const int* d_counts, int cap, const uint8_t* d_skip,
                                                  const uint8_t* d_taken, const spslam_fuse_params* params,
                                                  int32_t* d_match, int* d_nmatches, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    const MatchCurrent cur{d_keys_un, d_desc, nullptr, d_grid_off, d_grid_idx, d_counts, cap};
    if (n_problems < 1 || n_problems > 65535 || !d_problems || max_points < 0 || (max_points > 0 && !d_points) ||
        !slots_ok(cur) || cap > 36000 || !params || !d_match || !d_nmatches)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_search_by_projection_sim3_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_CHECK(c, c->d_loop_scratch.reserve((size_t)n_problems * std::max(max_points, 1) * sizeof(Sim3Window), s));
    HIP_CHECK(c, proj_sim3_launch(n_problems, d_problems, d_points, max_points, cur, keyframe_geom(c),
                                  search_consts(c, params->th), d_skip, d_taken, (Sim3Window*)c->d_loop_scratch.p,
                                  d_match, d_nmatches, s));
    return SPSLAM_OK;
}

int spslam_search_by_projection_sim3(spslam_ctx* c, const float* Scw, const spslam_local_point* points,
                                     int n_points, const spslam_keypoint* keys_un, const uint8_t* desc, int n_kp,
                                     const int32_t* grid_off, const int32_t* grid_idx, const uint8_t* skip,
                                     const uint8_t* taken, const spslam_fuse_params* params, int32_t* match,
                                     int* nmatches) {
    if (!c || !params || !nmatches || (n_kp > 0 && !match)) return SPSLAM_ERR_ARG;
    if (const char* e = loop_check_scw_problem(Scw, points, n_points, keys_un, desc, n_kp, grid_off, grid_idx))
        return fail(c, SPSLAM_ERR_ARG, "spslam_search_by_projection_sim3: %s", e);
    HIP_CHECK(c, hipSetDevice(c->device));
    spslam_fuse_problem F{};
    std::memcpy(F.Tcw, Scw, sizeof F.Tcw);
    F.n_points = n_points;
    const int np = n_points;
    const size_t N = (size_t)std::max(np, 1);
    const SlotStage kf{keys_un, desc, n_kp, grid_off, grid_idx};
    const size_t C = (size_t)kf.cap();
    std::vector<StageSlot> slots;
    kf.slots(slots);
    enum { kProblem = 5, kPoints, kSkip, kTaken, kMatch, kCount };
    slots.insert(slots.end(), {{&F, sizeof F}, {points, np * sizeof(spslam_local_point), N * sizeof(spslam_local_point)},
                               {skip, skip ? (size_t)np : 0, N}, {taken, taken ? (size_t)n_kp : 0, C}, C * 4,
                               sizeof(int)});
    Stage st(c);
    if (int rc = st.open(slots.data(), (int)slots.size())) return rc;
    const MatchCurrent d = kf.current(st, 0);
    int rc = spslam_search_by_projection_sim3_batch_device(
        c, 1, st.slot<spslam_fuse_problem>(kProblem), st.slot<spslam_local_point>(kPoints), np, d.kun, d.desc, d.grid_off,
        d.grid_idx, d.counts, d.cap, skip ? st.slot<uint8_t>(kSkip) : nullptr, taken ? st.slot<uint8_t>(kTaken) : nullptr,
        params, st.slot<int32_t>(kMatch), st.slot<int>(kCount), c->stream);
    if (rc) return rc;
    if (n_kp)
        HIP_CHECK(c, hipMemcpyAsync(match, st.slot<void>(kMatch), (size_t)n_kp * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(nmatches, st.slot<int>(kCount), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

}  // extern "C"
