// Host-side entry points of covis_kernels.hip (KeyFrame::UpdateConnections, LocalMapping::KeyFrameCulling and
// LocalMapping::MapPointCulling).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/spslam_gpu.h"

namespace spslam {

struct CullFrames {  // the frame stage's layouts, slot s at s * cap
    const spslam_keypoint* keys_un;
    const float* uright;
    const float* depth;
    int cap;
};

hipError_t covis_update_connections_launch(int n_problems, const spslam_covis_problem* problems,
                                           const spslam_covis_map& map, const spslam_covis_graph& graph, int th,
                                           spslam_covis_result* results, hipStream_t s);

hipError_t keyframe_culling_launch(int n_problems, const spslam_cull_problem* problems, const spslam_covis_map& map,
                                   const spslam_covis_graph& graph, const CullFrames& frames,
                                   const uint8_t* new_plane, const uint8_t* not_erase, const spslam_cull_params& params,
                                   spslam_cull_record* records, spslam_cull_summary* summaries, hipStream_t s);

hipError_t map_point_culling_launch(const spslam_point_cull_map& map, const int32_t* rows, const int32_t* cur_kf_id,
                                    int n, int th_obs, uint8_t* verdict, hipStream_t s);

}  // namespace spslam
