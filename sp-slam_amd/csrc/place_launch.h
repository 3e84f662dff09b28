// Host-side entry points of place_kernels.hip (KeyFrameDatabase::DetectRelocalizationCandidates,
// KeyFrameDatabase::DetectLoopCandidates and the reference score of LoopClosing::DetectLoop).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/spslam_gpu.h"

namespace spslam {

// graph: covis is read
hipError_t place_reloc_launch(int n_problems, const spslam_place_problem* problems, const spslam_place_db& db,
                              const spslam_place_frames& frames, const spslam_covis_graph& graph,
                              spslam_place_result* results, int32_t* candidates, hipStream_t s);

// graph: covis, weights and stride are read
hipError_t place_loop_launch(int n_problems, const spslam_place_problem* problems, const spslam_place_db& db,
                             const spslam_covis_graph& graph, const float* min_score, spslam_place_result* results,
                             int32_t* candidates, hipStream_t s);

// graph: ordered, n_ordered and stride are read
hipError_t place_min_score_launch(int n_problems, const spslam_place_problem* problems, const spslam_place_db& db,
                                  const spslam_covis_graph& graph, const uint8_t* kf_bad, float* min_score,
                                  hipStream_t s);

}  // namespace spslam
