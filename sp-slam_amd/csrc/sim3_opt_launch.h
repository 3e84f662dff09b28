// Host-side entry points of sim3_opt_kernels.hip (Optimizer::OptimizeSim3, src/Optimizer.cc:2279-2474).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/spslam_gpu.h"

namespace spslam {

struct Sim3OptConsts {
    float fx, fy, cx, cy;    // K1 = K2: the context's camera
    float inv_sigma2[8];     // mvInvLevelSigma2 per octave
    float th2;
    int min_inliers;
};

// bytes of scratch of one call: 16 + 104 * cap per problem
size_t sim3_opt_scratch_bytes(int n_pairs, int cap);

// gather, both optimize calls, the two checks and Scw: one workgroup per pair on stream s
hipError_t sim3_opt_launch(int n_pairs, const spslam_sim3_pair* pairs, const spslam_sim3_map& map,
                           const spslam_keypoint* kun, const int* counts, int cap, const Sim3OptConsts& P,
                           uint8_t* scratch, int32_t* match12, spslam_sim3_opt_result* results, hipStream_t s);

}  // namespace spslam
