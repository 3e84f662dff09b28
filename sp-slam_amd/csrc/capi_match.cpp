// C ABI (include/spslam_gpu.h), Tracking's ORBmatcher searches: spslam_search_by_projection[_batch_device]
// (TrackWithMotionModel) and spslam_search_local_points[_batch_device] (SearchLocalPoints).
#include "capi_ctx.h"

#include <cmath>

extern "C" {

int spslam_search_by_projection_batch_device(spslam_ctx* c, int n_frames, const spslam_proj_frame* d_frames,
                                             const spslam_proj_point* d_points, int max_points,
                                             const spslam_keypoint* d_keys_un, const uint8_t* d_desc,
                                             const float* d_uright, const int32_t* d_grid_off,
                                             const int32_t* d_grid_idx, const int* d_counts, int cap,
                                             const spslam_match_params* params, int32_t* d_match, int* d_nmatches,
                                             void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    const MatchCurrent cur{d_keys_un, d_desc, d_uright, d_grid_off, d_grid_idx, d_counts, cap};
    if (n_frames < 1 || !d_frames || max_points < 0 || (max_points > 0 && !d_points) || !match_current_ok(cur) ||
        !params || !d_match || !d_nmatches)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_search_by_projection_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the default stream (header)
    const size_t n = (size_t)n_frames * std::max(max_points, 1);
    const size_t need = n * sizeof(MatchWindow) + 256 + n * sizeof(int2);
    HIP_CHECK(c, c->d_match_scratch.reserve(need, s));
    auto* win = (MatchWindow*)c->d_match_scratch.p;
    auto* pushes = (int2*)(c->d_match_scratch + ((n * sizeof(MatchWindow) + 255) & ~(size_t)255));
    HIP_CHECK(c, match_launch(n_frames, d_frames, d_points, max_points, cur, match_geom(c), *params, win, pushes,
                              d_match, d_nmatches, s, c->timer));
    return SPSLAM_OK;
}

int spslam_search_by_projection(spslam_ctx* c, const spslam_proj_frame* frame, const spslam_proj_point* points,
                                const spslam_keypoint* keys_un, const uint8_t* desc, const float* uright, int n_kp,
                                const int32_t* grid_off, const int32_t* grid_idx, const spslam_match_params* params,
                                int32_t* match, int* nmatches) {
    const CurrentFrame cf{keys_un, desc, uright, n_kp, grid_off, grid_idx};
    if (!c || !frame || !params || !nmatches || !cf.args_ok() || frame->n_points < 0 ||
        (frame->n_points && !points) || (n_kp && !match))
        return SPSLAM_ERR_ARG;
    if (int rc = cf.check_grid(c)) return rc;
    HIP_CHECK(c, hipSetDevice(c->device));
    spslam_proj_frame F = *frame;
    F.point_offset = 0;
    const int np = F.n_points;
    const size_t C = (size_t)cf.cap();
    enum { kFrame = CurrentFrame::kFirst, kPoints, kMatch, kNMatches };
    Stage st(c);
    if (int rc = cf.open(st, {{&F, sizeof F},
                              {points, np * sizeof(spslam_proj_point), std::max(np, 1) * sizeof(spslam_proj_point)},
                              C * 4, sizeof(int)}))
        return rc;
    const MatchCurrent d = cf.current(st);
    int rc = spslam_search_by_projection_batch_device(
        c, 1, st.slot<spslam_proj_frame>(kFrame), st.slot<spslam_proj_point>(kPoints), np, d.kun, d.desc, d.uright,
        d.grid_off, d.grid_idx, d.counts, d.cap, params, st.slot<int32_t>(kMatch), st.slot<int>(kNMatches), c->stream);
    if (rc) return rc;
    if (n_kp)
        HIP_CHECK(c, hipMemcpyAsync(match, st.slot<int32_t>(kMatch), (size_t)n_kp * 4, hipMemcpyDeviceToHost,
                                    c->stream));
    HIP_CHECK(c, hipMemcpyAsync(nmatches, st.slot<int>(kNMatches), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

int spslam_search_local_points_batch_device(spslam_ctx* c, int n_frames, const spslam_local_frame* d_frames,
                                            const spslam_local_point* d_points, int max_points,
                                            const spslam_keypoint* d_keys_un, const uint8_t* d_desc,
                                            const float* d_uright, const int32_t* d_grid_off,
                                            const int32_t* d_grid_idx, const int* d_counts, int cap,
                                            const uint8_t* d_taken, const spslam_local_params* params,
                                            int32_t* d_match, int* d_nmatches, uint8_t* d_in_view,
                                            const int32_t* d_seen, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    const MatchCurrent cur{d_keys_un, d_desc, d_uright, d_grid_off, d_grid_idx, d_counts, cap};
    if (n_frames < 1 || !d_frames || max_points < 0 || (max_points > 0 && !d_points) || !match_current_ok(cur) ||
        !params || !d_match || !d_nmatches)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_search_local_points_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the default stream (header)
    const size_t need = (size_t)n_frames * std::max(max_points, 1) * sizeof(LocalWindow) + 256;
    HIP_CHECK(c, c->d_match_scratch.reserve(need, s));
    LocalConsts P{params->th, params->nn_ratio, params->view_cos_limit,
                  std::log(c->p.scale_factor),  // Frame::mfLogScaleFactor = log(mfScaleFactor), float
                  c->p.nlevels, d_seen};
    HIP_CHECK(c, local_match_launch(n_frames, d_frames, d_points, max_points, cur, match_geom(c), P, d_taken,
                                    (LocalWindow*)c->d_match_scratch.p, d_match, d_nmatches, d_in_view, s, c->timer));
    return SPSLAM_OK;
}

int spslam_search_local_points(spslam_ctx* c, const spslam_local_frame* frame, const spslam_local_point* points,
                               const spslam_keypoint* keys_un, const uint8_t* desc, const float* uright, int n_kp,
                               const int32_t* grid_off, const int32_t* grid_idx, const uint8_t* taken,
                               const spslam_local_params* params, int32_t* match, int* nmatches, uint8_t* in_view) {
    const CurrentFrame cf{keys_un, desc, uright, n_kp, grid_off, grid_idx};
    if (!c || !frame || !params || !nmatches || !cf.args_ok() || frame->n_points < 0 ||
        (frame->n_points && !points) || (n_kp && !match))
        return SPSLAM_ERR_ARG;
    if (int rc = cf.check_grid(c)) return rc;
    HIP_CHECK(c, hipSetDevice(c->device));
    spslam_local_frame F = *frame;
    F.point_offset = 0;
    const int np = F.n_points;
    const size_t K = (size_t)n_kp, C = (size_t)cf.cap();
    enum { kFrame = CurrentFrame::kFirst, kPoints, kTaken, kMatch, kNMatches, kInView };
    Stage st(c);
    if (int rc = cf.open(st, {{&F, sizeof F},
                              {points, np * sizeof(spslam_local_point), std::max(np, 1) * sizeof(spslam_local_point)},
                              {taken, taken ? K : 0, C}, C * 4, sizeof(int), (size_t)std::max(np, 1)}))
        return rc;
    const MatchCurrent d = cf.current(st);
    int rc = spslam_search_local_points_batch_device(
        c, 1, st.slot<spslam_local_frame>(kFrame), st.slot<spslam_local_point>(kPoints), np, d.kun, d.desc, d.uright,
        d.grid_off, d.grid_idx, d.counts, d.cap, taken ? st.slot<uint8_t>(kTaken) : nullptr, params,
        st.slot<int32_t>(kMatch), st.slot<int>(kNMatches), st.slot<uint8_t>(kInView), nullptr, c->stream);
    if (rc) return rc;
    if (n_kp) HIP_CHECK(c, hipMemcpyAsync(match, st.slot<int32_t>(kMatch), K * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(nmatches, st.slot<int>(kNMatches), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (in_view && np)
        HIP_CHECK(c, hipMemcpyAsync(in_view, st.slot<uint8_t>(kInView), (size_t)np, hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

}  // extern "C"
