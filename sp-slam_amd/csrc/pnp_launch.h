// Host-side entry points of pnp_kernels.hip (PnPsolver, src/PnPsolver.cc).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/spslam_gpu.h"

namespace spslam {

struct PnpConsts {
    float fx, fy, cx, cy;    // the Frame's calibration: the context's camera
    float max_error[8];      // per octave: mvLevelSigma2 * th2 in float (:156)
    int max_iterations, rand_max;
};

// bytes of scratch the three kernels share for one call
size_t pnp_scratch_bytes(int n_problems, int cap, int max_iterations);

// gather, hypotheses, refinement and selection on stream s.  frame_points may be null.
hipError_t pnp_solver_launch(int n_problems, const spslam_pnp_problem* problems, const spslam_sim3_map& map,
                             const spslam_keypoint* kun, const int* counts, int cap, const int32_t* match,
                             const int32_t* rnd, const int32_t* max_its, const int32_t* min_n, const PnpConsts& P,
                             uint8_t* scratch, spslam_pnp_result* results, uint8_t* inliers, uint8_t* best_mask,
                             int32_t* frame_points, hipStream_t s);

}  // namespace spslam
