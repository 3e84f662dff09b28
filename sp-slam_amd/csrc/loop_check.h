// The index checks of the loop-closing entries' host forms (capi_loop_closing.cpp): every index the kernels follow
// through a FeatureVector, a keyframe grid, a match list or a point list.  Plain C++ without a HIP call, so that they
// run, and are checked, on a CPU (tools/loop_check_main.cpp).  Each returns NULL when the tables are sound, else
// what is wrong.
#pragma once
#include <cstdint>

#include "../../include/spslam_gpu.h"

namespace spslam {

constexpr int kLoopGridCells = SPSLAM_GRID_COLS * SPSLAM_GRID_ROWS;

// one keyframe of SearchByBoW(KF, KF): n keypoints and its FeatureVector
inline const char* loop_check_bow_keyframe(const spslam_bow_keyframe* k) {
    if (!k) return "a keyframe is missing";
    if (k->n < 0 || k->n > 8192) return "n outside 0 .. 8192";
    if (k->n_fv < 0 || k->n_fv > k->n) return "a FeatureVector with more nodes than keypoints";
    if (!k->fv_start) return "fv_start is missing";
    if (k->n && (!k->desc || !k->keys_un || !k->has_point)) return "a keypoint array is missing";
    if (k->n_fv && (!k->fv_nodes || !k->fv_features)) return "a FeatureVector array is missing";
    if (k->fv_start[0] != 0) return "fv_start does not begin at 0";
    for (int a = 0; a < k->n_fv; a++) {
        if (k->fv_start[a + 1] < k->fv_start[a]) return "fv_start descends";
        if (a && k->fv_nodes[a - 1] >= k->fv_nodes[a]) return "the FeatureVector's nodes do not ascend";
    }
    const int m = k->fv_start[k->n_fv];
    if (m > k->n) return "the FeatureVector lists more features than keypoints";
    for (int q = 0; q < m; q++)
        if (k->fv_features[q] < 0 || k->fv_features[q] >= k->n) return "a FeatureVector feature outside the keypoints";
    return nullptr;
}

// a keyframe's grid CSR over n_kp keypoints
inline const char* loop_check_grid(const int32_t* grid_off, const int32_t* grid_idx, int n_kp) {
    if (n_kp < 0 || n_kp > (1 << 20)) return "n_kp outside 0 .. 2^20";
    if (!grid_off) return "grid_off is missing";
    if (grid_off[0] != 0) return "grid_off does not begin at 0";
    for (int c = 0; c < kLoopGridCells; c++)
        if (grid_off[c + 1] < grid_off[c]) return "grid_off descends";
    const int m = grid_off[kLoopGridCells];
    if (m > n_kp) return "the grid lists more keypoints than there are";
    if (m && !grid_idx) return "grid_idx is missing";
    for (int j = 0; j < m; j++)
        if (grid_idx[j] < 0 || grid_idx[j] >= n_kp) return "a grid entry outside the keypoints";
    return nullptr;
}

// the keyframe of the Scw searches: its arrays, its grid and the point list
inline const char* loop_check_scw_problem(const float* Scw, const spslam_local_point* points, int n_points,
                                          const spslam_keypoint* keys_un, const uint8_t* desc, int n_kp,
                                          const int32_t* grid_off, const int32_t* grid_idx) {
    if (!Scw) return "Scw is missing";
    if (n_points < 0 || n_points > (1 << 24)) return "n_points outside 0 .. 2^24";
    if (n_points && !points) return "the points are missing";
    if (const char* e = loop_check_grid(grid_off, grid_idx, n_kp)) return e;
    if (n_kp && (!keys_un || !desc)) return "a keypoint array is missing";
    return nullptr;
}

// one keyframe of SearchBySim3: its arrays, its grid, and its map points as rows of an n_rows table
inline const char* loop_check_sim3_keyframe(const spslam_sim3_keyframe* k, int n_rows) {
    if (!k) return "a keyframe is missing";
    if (!k->Tcw) return "Tcw is missing";
    if (const char* e = loop_check_grid(k->grid_off, k->grid_idx, k->n)) return e;
    if (k->n && (!k->keys_un || !k->desc || !k->match_row)) return "a keypoint array is missing";
    for (int i = 0; i < k->n; i++)
        if (k->match_row[i] < -1 || k->match_row[i] >= n_rows) return "a map point outside the table";
    return nullptr;
}

// vpMatches12 on entry: n1 entries, each -1 or a keypoint of KF2
inline const char* loop_check_match12(const int32_t* match12, int n1, int n2) {
    if (n1 && !match12) return "match12 is missing";
    for (int i = 0; i < n1; i++)
        if (match12[i] < -1 || match12[i] >= n2) return "a match12 entry outside KF2's keypoints";
    return nullptr;
}

// one keyframe of Sim3Solver: its pose, keypoints (the octave indexes mvLevelSigma2) and map points; the grid and
// the descriptors are not read
inline const char* loop_check_solver_keyframe(const spslam_sim3_keyframe* k, int n_rows, int n_levels) {
    if (!k) return "a keyframe is missing";
    if (!k->Tcw) return "Tcw is missing";
    if (k->n < 0 || k->n > 8192) return "n outside 0 .. 8192";
    if (k->n && (!k->keys_un || !k->match_row)) return "a keypoint array is missing";
    for (int i = 0; i < k->n; i++) {
        if (k->match_row[i] < -1 || k->match_row[i] >= n_rows) return "a map point outside the table";
        if (k->keys_un[i].octave < 0 || k->keys_un[i].octave >= n_levels) return "an octave outside the configured levels";
    }
    return nullptr;
}

// SetRansacParameters' and iterate's arguments, the solver's state and the recorded draws
inline const char* loop_check_solver_call(const spslam_sim3_solver_params* p, double probability, int n_iterations,
                                          const int* iterations_done, const int* best_inliers, const int32_t* rand) {
    if (!p) return "the parameters are missing";
    if (p->min_inliers < 3) return "min_inliers below 3";
    if (p->max_iterations < 1 || p->max_iterations > SPSLAM_SIM3_MAX_ITERATIONS) return "max_iterations outside 1 .. 4096";
    if (p->rand_max < 1) return "rand_max below 1";
    if (!(probability > 0.0 && probability < 1.0)) return "probability outside (0, 1)";
    if (n_iterations < 0) return "n_iterations is negative";
    if (!iterations_done || !best_inliers) return "the solver's state is missing";
    if (*iterations_done < 0 || *best_inliers < 0) return "the solver's state is negative";
    if (!rand) return "the draws are missing";
    for (int i = 0; i < 3 * p->max_iterations; i++)
        if (rand[i] < 0 || rand[i] > p->rand_max) return "a draw outside 0 .. rand_max";
    return nullptr;
}

// OptimizeSim3's parameters and the pair record whose s12, R12, t12 are gScm
inline const char* loop_check_opt_call(const spslam_sim3_opt_params* p, const spslam_sim3_pair* pair) {
    if (!p) return "the parameters are missing";
    if (p->fix_scale != 1) return "fix_scale is not 1 (a free scale needs a correctly rounded exp)";
    if (!(p->th2 > 0.f)) return "th2 is not positive";
    if (!pair) return "the pair is missing";
    return nullptr;
}

}  // namespace spslam
