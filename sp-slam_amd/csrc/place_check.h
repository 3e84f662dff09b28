// The index checks of the place-recognition entries' host forms (capi_place.cpp): every index the kernels of
// place_kernels.hip follow.  Plain C++ without a HIP call, so that they run, and are checked, on a CPU.
// Each returns NULL when the tables are sound, else what is wrong.
#pragma once
#include <cstdint>

#include "../../include/spslam_gpu.h"

namespace spslam {

// one BowVector: n words in 0 .. cap, ascending and unique
inline const char* place_check_vector(const uint32_t* words, const double* values, int n, int cap) {
    if (n < 0 || n > cap) return "a BowVector longer than cap";
    if (n && (!words || !values)) return "a BowVector lacks its arrays";
    for (int i = 1; i < n; i++)
        if (words[i - 1] >= words[i]) return "a BowVector's words do not ascend";
    return nullptr;
}

// The database of one sequence at base 0 (the score tables are the entries' own to check).
inline const char* place_check_db(const spslam_place_db& db, int n_kf) {
    if (n_kf < 1 || n_kf > SPSLAM_COVIS_MAX_KF) return "n_kf outside 1 .. 1024";
    if (db.cap < 1 || db.cap > SPSLAM_PLACE_MAX_WORDS) return "cap outside 1 .. 8192";
    if (!db.bow_words || !db.bow_values || !db.n_bow || !db.in_db) return "a database array is missing";
    for (int k = 0; k < n_kf; k++)
        if (const char* e = place_check_vector(db.bow_words + (size_t)k * db.cap, db.bow_values + (size_t)k * db.cap,
                                               db.n_bow[k], db.cap))
            return e;
    return nullptr;
}

// GetBestCovisibilityKeyFrames(10) of every keyframe: -1 or a keyframe
inline const char* place_check_covis(const int32_t* covis, int n_kf) {
    if (!covis) return "the covis table is missing";
    for (int e = 0; e < n_kf * SPSLAM_COVIS_BEST; e++)
        if (covis[e] < -1 || covis[e] >= n_kf) return "a covis neighbour outside the keyframes";
    return nullptr;
}

// the loop and min-score entries' query keyframe and the graph rows they read
inline const char* place_check_query(const spslam_covis_graph& g, int n_kf, int query) {
    if (query < 0 || query >= n_kf) return "query outside the keyframes";
    if (g.stride < n_kf) return "the graph's stride is below n_kf";
    return nullptr;
}

// GetVectorCovisibleKeyFrames of the query keyframe
inline const char* place_check_ordered(const spslam_covis_graph& g, int n_kf, int query) {
    if (!g.ordered || !g.n_ordered) return "the ordered lists are missing";
    const int n = g.n_ordered[query];
    if (n < 0 || n > g.stride || n > SPSLAM_COVIS_MAX_KF) return "the ordered list is longer than its row";
    const int32_t* row = g.ordered + (size_t)query * g.stride;
    for (int q = 0; q < n; q++)
        if (row[q] < 0 || row[q] >= n_kf) return "an ordered keyframe outside the keyframes";
    return nullptr;
}

}  // namespace spslam
