// Host-side entry point of map_point_kernels.hip (MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/spslam_gpu.h"

namespace spslam {

struct RefreshConsts {
    float scale[8];  // mvScaleFactors
    int n_levels;    // mnScaleLevels
};

hipError_t map_points_refresh_launch(const spslam_point_refresh_map& map, const int32_t* rows, int n, int what,
                                     const spslam_keypoint* keys_un, const uint8_t* desc, int cap,
                                     const RefreshConsts& P, uint8_t* status, hipStream_t s);

}  // namespace spslam
