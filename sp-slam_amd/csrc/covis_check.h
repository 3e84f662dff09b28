// The index checks of the covisibility entries' host forms (capi_local_mapping.cpp): every index the kernels of
// covis_kernels.hip follow.  Plain C++ without a HIP call, so that they run, and are checked, on a CPU.
// Each returns NULL when the tables are sound, else what is wrong.
#pragma once
#include <cstdint>

#include "../../include/spslam_gpu.h"

namespace spslam {

// a CSR's offsets: n + 1 entries from 0, not decreasing
inline const char* covis_check_offsets(const int32_t* off, int n) {
    if (!off || off[0] != 0) return "a CSR does not start at 0";
    for (int i = 0; i < n; i++)
        if (off[i] > off[i + 1]) return "a CSR's offsets decrease";
    return nullptr;
}

// The match and observer CSRs of n_kf keyframes and n_rows rows.  culling: obs_kp, kf_slot and points are read
// too, with n_slots keyframe slots of cap keypoints, and no match list is longer than cap.
inline const char* covis_check_map(const spslam_covis_map& m, int n_kf, int n_rows, bool culling, int cap,
                                   int n_slots) {
    if (n_kf < 1 || n_kf > SPSLAM_COVIS_MAX_KF || n_rows < 0) return "n_kf outside 1 .. 1024 or n_rows < 0";
    if (const char* e = covis_check_offsets(m.match_off, n_kf)) return e;
    if (const char* e = covis_check_offsets(m.obs_off, n_rows)) return e;
    const int n_match = m.match_off[n_kf], n_obs = m.obs_off[n_rows];
    if ((n_match && !m.match_row) || (n_obs && !m.obs_kf)) return "a CSR lacks its array";
    for (int e = 0; e < n_match; e++)
        if (m.match_row[e] < -1 || m.match_row[e] >= n_rows) return "a match row outside the point table";
    for (int o = 0; o < n_obs; o++)
        if (m.obs_kf[o] < 0 || m.obs_kf[o] >= n_kf) return "an observer outside the keyframes";
    if (!culling) return nullptr;
    if (cap < 1 || n_slots < 0 || !m.kf_slot || (n_obs && !m.obs_kp) || (n_rows && !m.points))
        return "a culling table is missing";
    for (int k = 0; k < n_kf; k++) {
        if (m.kf_slot[k] < 0 || m.kf_slot[k] >= n_slots) return "a keyframe slot outside the frame arrays";
        if (m.match_off[k + 1] - m.match_off[k] > cap) return "a match list longer than cap";
    }
    for (int o = 0; o < n_obs; o++)
        if (m.obs_kp[o] < 0 || m.obs_kp[o] >= cap) return "an observation's keypoint outside cap";
    return nullptr;
}

// The graph arrays of one sequence at base 0.
inline const char* covis_check_graph(const spslam_covis_graph& g, int n_kf) {
    if (!g.weights || !g.ordered || !g.ordered_w || !g.n_ordered || !g.covis || !g.parent || !g.first_connection)
        return "a graph array is missing";
    if (g.stride < n_kf) return "the graph's stride is below n_kf";
    return nullptr;
}

// A candidate list (GetVectorCovisibleKeyFrames) of n entries.
inline const char* covis_check_candidates(const int32_t* ordered, int n, int n_kf) {
    if (n < 0 || n > SPSLAM_COVIS_MAX_KF || (n && !ordered)) return "the candidate list is missing or too long";
    for (int q = 0; q < n; q++)
        if (ordered[q] < 0 || ordered[q] >= n_kf) return "a candidate outside the keyframes";
    return nullptr;
}

// The list of MapPointCulling: n absolute rows of a table of n_rows.
inline const char* covis_check_rows(const int32_t* rows, int n, int n_rows) {
    if (n < 0 || n_rows < 0 || (n && !rows)) return "the row list is missing";
    for (int k = 0; k < n; k++)
        if (rows[k] < 0 || rows[k] >= n_rows) return "a listed row outside the point table";
    return nullptr;
}

}  // namespace spslam
