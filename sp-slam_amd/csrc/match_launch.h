// Host-side entry points of match_kernels.hip (ORBmatcher::SearchByProjection).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/spslam_gpu.h"
#include "orb_launch.h"

namespace spslam {

struct MatchGeom {
    float fx, fy, cx, cy, bf;          // mK, mbf
    float min_x, max_x, min_y, max_y;  // ComputeImageBounds
    float ginv_x, ginv_y;              // mfGridElementWidthInv / HeightInv
    float scale[8];                    // mvScaleFactors
};

struct MatchCurrent {
    const spslam_keypoint* kun;
    const uint8_t* desc;
    const float* uright;
    const int32_t* grid_off;
    const int32_t* grid_idx;
    const int* counts;
    int cap;
};

// Per-point search state between the two kernels (scratch, n_frames * max_points entries), with the K smallest
// keys per point: the in-order walks re-scan a point's window only when in-loop assignments took (all but one of)
// them.  Small batches keep kProjKeys / kLocalKeys = 6 (with 3, a B = 1 frame re-scanned 2.6 last-frame and 12.5
// local windows of ~10 us each); large batches keep 3, whose window kernels cost less (kSmallBatchKeys).  The
// results do not depend on K.
constexpr int kProjKeys = 6, kLocalKeys = 6, kFewKeys = 3, kSmallBatchKeys = 16;
template <int K>
struct MatchWindowK {
    float u, v, r, invzc;
    int16_t x0, x1, y0, y1;   // GetFeaturesInArea cell range (x0 > x1: empty)
    int8_t min_level, max_level, valid, pad;
    uint32_t best[K];          // the smallest (distance << 20) | CSR position over the window; ~0u: none
    int32_t kp[K];             // their keypoints (grid_idx of the CSR position), -1: none
    float kang[K];             // and those keypoints' angles
};
using MatchWindow = MatchWindowK<kProjKeys>;  // (the scratch is sized for the larger K)

// Local-map search state per point (SearchLocalPoints).
template <int K>
struct LocalWindowK {
    float u, v, rs, ur;      // mTrackProjX / Y, r * mvScaleFactors[level], mTrackProjXR
    int16_t x0, x1, y0, y1;
    int8_t level, in_view, pad[2];
    uint32_t best[K];        // smallest keys over the window without the initially taken keypoints
    int32_t kp[K];           // their keypoints, -1: none
    int8_t oct[K];           // and those keypoints' octaves
    int8_t pad2[(8 - K % 8) % 8];
};
using LocalWindow = LocalWindowK<kLocalKeys>;

struct LocalConsts {
    float th, nn_ratio, view_cos_limit, log_scale_factor;
    int n_levels;
    const int32_t* seen;  // per-frame seen stamps (spslam_local_frame.seen_offset / stamp), may be NULL
};

hipError_t local_match_launch(int n_frames, const spslam_local_frame* frames, const spslam_local_point* points,
                              int max_points, const MatchCurrent& cur, const MatchGeom& g, const LocalConsts& P,
                              const uint8_t* taken_in, LocalWindow* win, int32_t* match, int* nmatches,
                              uint8_t* in_view, hipStream_t s, KernelTimer* timer);

// ORBmatcher::Fuse's search (fuse_search_kernel).  g: the KeyFrame's geometry, its bounds truncated to ints.
struct FuseConsts {
    float th, log_scale_factor;
    int n_levels;
    float inv_sigma2[8];  // mvInvLevelSigma2
};

hipError_t fuse_search_launch(int n_problems, const spslam_fuse_problem* problems, const spslam_local_point* points,
                              int max_points, const MatchCurrent& cur, const MatchGeom& g, const FuseConsts& P,
                              const uint8_t* skip, spslam_fuse_result* results, int* nfused, hipStream_t s);

// LoopClosing's Sim3 matchers.  g: the KeyFrame's geometry, as for fuse_search_launch; P.inv_sigma2 is not read.
// Fuse(pKF, Scw, ...)'s search: fuse_search_launch's records, the problems' Tcw fields holding Scw; cur.uright is
// not read (may be null).
hipError_t fuse_sim3_search_launch(int n_problems, const spslam_fuse_problem* problems,
                                   const spslam_local_point* points, int max_points, const MatchCurrent& cur,
                                   const MatchGeom& g, const FuseConsts& P, const uint8_t* skip,
                                   spslam_fuse_result* results, int* nfused, hipStream_t s);

// Per-point search state of SearchByProjection(pKF, Scw, ...) between its two kernels (scratch, n_problems *
// max_points entries): the window and the kSim3Keys smallest keys among the keypoints not taken on entry.  The
// in-order walk re-scans a window only when in-loop assignments took all of them.
constexpr int kSim3Keys = SPSLAM_PROJ_SIM3_KEYS;
struct Sim3Window {
    float u, v, r;
    int16_t x0, x1, y0, y1;  // GetFeaturesInArea cell range (x0 > x1: empty)
    int8_t level, valid, pad[2];
    uint32_t best[kSim3Keys];  // (distance << 20) | CSR position, ascending; ~0u: none
    int32_t kp[kSim3Keys];     // their keypoints, -1: none
};

// taken_in (may be null) and match at problem * cur.cap; nmatches one int per problem.
hipError_t proj_sim3_launch(int n_problems, const spslam_fuse_problem* problems, const spslam_local_point* points,
                            int max_points, const MatchCurrent& cur, const MatchGeom& g, const FuseConsts& P,
                            const uint8_t* skip, const uint8_t* taken_in, Sim3Window* win, int32_t* match,
                            int* nmatches, hipStream_t s);

// SearchBySim3: vn (2 * cur.cap ints per pair) and flags (cur.cap bytes per pair) are scratch; already2 (may be
// null) at pair * cur.cap.
hipError_t sim3_search_launch(int n_pairs, const spslam_sim3_pair* pairs, const spslam_sim3_map& map,
                              const MatchCurrent& cur, const MatchGeom& g, const FuseConsts& P,
                              const uint8_t* already2, int32_t* vn, uint8_t* flags, int32_t* match12, int* n_found,
                              hipStream_t s);

hipError_t match_launch(int n_frames, const spslam_proj_frame* frames, const spslam_proj_point* points,
                        int max_points, const MatchCurrent& cur, const MatchGeom& g, const spslam_match_params& P,
                        MatchWindow* win, int2* pushes, int32_t* match, int* nmatches, hipStream_t s,
                        KernelTimer* timer);

}  // namespace spslam
