// Host-side entry points of sim3_kernels.hip (Sim3Solver, src/Sim3Solver.cc).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/spslam_gpu.h"

namespace spslam {

struct SolverConsts {
    float fx, fy, cx, cy;    // mK1 = mK2: the context's camera
    float max_error[8];      // per octave: (float)(size_t)(9.210 * mvLevelSigma2), the bound as `err < bound` sees it
    int min_inliers, max_iterations, rand_max, fix_scale;
};

// bytes of scratch the three kernels share for one call
size_t sim3_scratch_bytes(int n_problems, int cap, int max_iterations);

// gather, hypotheses, selection on stream s.  pairs_out / match12_out may be null.
hipError_t sim3_solver_launch(int n_problems, const spslam_sim3_problem* problems, const spslam_sim3_map& map,
                              const spslam_keypoint* kun, const int* counts, int cap, const int32_t* match12,
                              const int32_t* rnd, const int32_t* table, const SolverConsts& P, uint8_t* scratch,
                              spslam_sim3_result* results, uint8_t* inliers, spslam_sim3_pair* pairs_out,
                              int32_t* match12_out, hipStream_t s);

}  // namespace spslam
