// C ABI (include/spslam_gpu.h): projection, local-point and Fuse search, the map-point refresh, the tracking graph,
// masked copies and bag of words.
#include "capi_ctx.h"
#include "triangulate_launch.h"

#include <cmath>
#include <cstring>
#include <sstream>
#include <vector>

namespace {

// camera, image bounds, grid and level scales of the configured frame stage
MatchGeom match_geom(const spslam_ctx* c) {
    MatchGeom g{};
    g.fx = c->fg.fx; g.fy = c->fg.fy; g.cx = c->fg.cx; g.cy = c->fg.cy; g.bf = c->fg.bf;
    g.min_x = c->fg.min_x; g.max_x = c->fg.max_x; g.min_y = c->fg.min_y; g.max_y = c->fg.max_y;
    g.ginv_x = c->fg.ginv_x; g.ginv_y = c->fg.ginv_y;
    for (int l = 0; l < 8; l++) g.scale[l] = l < c->p.nlevels ? c->scale[l] : 0.f;
    return g;
}

}  // namespace

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
    if (n_frames < 1 || !d_frames || max_points < 0 || (max_points > 0 && !d_points) || !d_keys_un || !d_desc ||
        !d_uright || !d_grid_off || !d_grid_idx || !d_counts || cap < 1 || cap > (1 << 20) || !params ||
        !d_match || !d_nmatches)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_search_by_projection_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the default stream (header)
    const size_t n = (size_t)n_frames * std::max(max_points, 1);
    const size_t need = n * sizeof(MatchWindow) + 256 + n * sizeof(int2);
    HIP_CHECK(c, c->d_match_scratch.reserve(need, s));
    auto* win = (MatchWindow*)c->d_match_scratch.p;
    auto* pushes = (int2*)(c->d_match_scratch + ((n * sizeof(MatchWindow) + 255) & ~(size_t)255));
    MatchCurrent cur{d_keys_un, d_desc, d_uright, d_grid_off, d_grid_idx, d_counts, cap};
    HIP_CHECK(c, match_launch(n_frames, d_frames, d_points, max_points, cur, match_geom(c), *params, win, pushes,
                              d_match, d_nmatches, s, c->timer));
    return SPSLAM_OK;
}

int spslam_search_by_projection(spslam_ctx* c, const spslam_proj_frame* frame, const spslam_proj_point* points,
                                const spslam_keypoint* keys_un, const uint8_t* desc, const float* uright, int n_kp,
                                const int32_t* grid_off, const int32_t* grid_idx, const spslam_match_params* params,
                                int32_t* match, int* nmatches) {
    if (!c || !frame || !params || !grid_off || !nmatches || n_kp < 0 || frame->n_points < 0 ||
        (frame->n_points && !points) || (n_kp && (!keys_un || !desc || !uright || !grid_idx || !match)))
        return SPSLAM_ERR_ARG;
    constexpr int kCells = SPSLAM_GRID_COLS * SPSLAM_GRID_ROWS;
    if (grid_off[0] != 0 || grid_off[kCells] > n_kp)
        return fail(c, SPSLAM_ERR_ARG, "grid CSR does not fit the keypoints%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    spslam_proj_frame F = *frame;
    F.point_offset = 0;
    const int np = F.n_points, cap = std::max(n_kp, 1);
    const size_t K = (size_t)n_kp, C = (size_t)cap;
    Stage st(c);
    if (int rc = st.open({{&F, sizeof F},
                           {points, np * sizeof(spslam_proj_point), std::max(np, 1) * sizeof(spslam_proj_point)},
                           {keys_un, K * sizeof(spslam_keypoint), C * sizeof(spslam_keypoint)},
                           {desc, K * 32, C * 32}, {uright, K * 4, C * 4},
                           {grid_off, (kCells + 1) * 4}, {grid_idx, (size_t)grid_off[kCells] * 4, C * 4},
                           {&n_kp, sizeof(int)}, C * 4, sizeof(int)}))
        return rc;
    int rc = spslam_search_by_projection_batch_device(
        c, 1, st.slot<spslam_proj_frame>(0), st.slot<spslam_proj_point>(1), np, st.slot<spslam_keypoint>(2),
        st.slot<uint8_t>(3), st.slot<float>(4), st.slot<int32_t>(5), st.slot<int32_t>(6), st.slot<int>(7), cap,
        params, st.slot<int32_t>(8), st.slot<int>(9), c->stream);
    if (rc) return rc;
    if (n_kp) HIP_CHECK(c, hipMemcpyAsync(match, st.slot<int32_t>(8), K * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(nmatches, st.slot<int>(9), sizeof(int), hipMemcpyDeviceToHost, c->stream));
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
    if (n_frames < 1 || !d_frames || max_points < 0 || (max_points > 0 && !d_points) || !d_keys_un || !d_desc ||
        !d_uright || !d_grid_off || !d_grid_idx || !d_counts || cap < 1 || cap > (1 << 20) || !params ||
        !d_match || !d_nmatches)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_search_local_points_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the default stream (header)
    const size_t need = (size_t)n_frames * std::max(max_points, 1) * sizeof(LocalWindow) + 256;
    HIP_CHECK(c, c->d_match_scratch.reserve(need, s));
    LocalConsts P{params->th, params->nn_ratio, params->view_cos_limit,
                  std::log(c->p.scale_factor),  // Frame::mfLogScaleFactor = log(mfScaleFactor), float
                  c->p.nlevels, d_seen};
    MatchCurrent cur{d_keys_un, d_desc, d_uright, d_grid_off, d_grid_idx, d_counts, cap};
    HIP_CHECK(c, local_match_launch(n_frames, d_frames, d_points, max_points, cur, match_geom(c), P, d_taken,
                                    (LocalWindow*)c->d_match_scratch.p, d_match, d_nmatches, d_in_view, s, c->timer));
    return SPSLAM_OK;
}

int spslam_search_local_points(spslam_ctx* c, const spslam_local_frame* frame, const spslam_local_point* points,
                               const spslam_keypoint* keys_un, const uint8_t* desc, const float* uright, int n_kp,
                               const int32_t* grid_off, const int32_t* grid_idx, const uint8_t* taken,
                               const spslam_local_params* params, int32_t* match, int* nmatches, uint8_t* in_view) {
    if (!c || !frame || !params || !grid_off || !nmatches || n_kp < 0 || frame->n_points < 0 ||
        (frame->n_points && !points) || (n_kp && (!keys_un || !desc || !uright || !grid_idx || !match)))
        return SPSLAM_ERR_ARG;
    constexpr int kCells = SPSLAM_GRID_COLS * SPSLAM_GRID_ROWS;
    if (grid_off[0] != 0 || grid_off[kCells] > n_kp)
        return fail(c, SPSLAM_ERR_ARG, "grid CSR does not fit the keypoints%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    spslam_local_frame F = *frame;
    F.point_offset = 0;
    const int np = F.n_points, cap = std::max(n_kp, 1);
    const size_t K = (size_t)n_kp, C = (size_t)cap;
    Stage st(c);
    if (int rc = st.open({{&F, sizeof F},
                           {points, np * sizeof(spslam_local_point), std::max(np, 1) * sizeof(spslam_local_point)},
                           {keys_un, K * sizeof(spslam_keypoint), C * sizeof(spslam_keypoint)},
                           {desc, K * 32, C * 32}, {uright, K * 4, C * 4},
                           {grid_off, (kCells + 1) * 4}, {grid_idx, (size_t)grid_off[kCells] * 4, C * 4},
                           {&n_kp, sizeof(int)}, {taken, taken ? K : 0, C}, C * 4, sizeof(int),
                           (size_t)std::max(np, 1)}))
        return rc;
    int rc = spslam_search_local_points_batch_device(
        c, 1, st.slot<spslam_local_frame>(0), st.slot<spslam_local_point>(1), np, st.slot<spslam_keypoint>(2),
        st.slot<uint8_t>(3), st.slot<float>(4), st.slot<int32_t>(5), st.slot<int32_t>(6), st.slot<int>(7), cap,
        taken ? st.slot<uint8_t>(8) : nullptr, params, st.slot<int32_t>(9), st.slot<int>(10), st.slot<uint8_t>(11),
        nullptr, c->stream);
    if (rc) return rc;
    if (n_kp) HIP_CHECK(c, hipMemcpyAsync(match, st.slot<int32_t>(9), K * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(nmatches, st.slot<int>(10), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (in_view && np) HIP_CHECK(c, hipMemcpyAsync(in_view, st.slot<uint8_t>(11), (size_t)np, hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

int spslam_fuse_search_batch_device(spslam_ctx* c, int n_problems, const spslam_fuse_problem* d_problems,
                                    const spslam_local_point* d_points, int max_points,
                                    const spslam_keypoint* d_keys_un, const uint8_t* d_desc, const float* d_uright,
                                    const int32_t* d_grid_off, const int32_t* d_grid_idx, const int* d_counts,
                                    int cap, const uint8_t* d_skip, const spslam_fuse_params* params,
                                    spslam_fuse_result* d_results, int* d_nfused, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    if (n_problems < 1 || !d_problems || max_points < 0 || (max_points > 0 && (!d_points || !d_results)) ||
        !d_keys_un || !d_desc || !d_uright || !d_grid_off || !d_grid_idx || !d_counts || cap < 1 ||
        cap > (1 << 20) || !params || !d_nfused)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_fuse_search_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    // KeyFrame's mnMinX .. mnMaxY are ints initialised from the Frame's floats (KeyFrame.cc:41, KeyFrame.h:198-201)
    MatchGeom g = match_geom(c);
    g.min_x = (float)(int)g.min_x; g.max_x = (float)(int)g.max_x;
    g.min_y = (float)(int)g.min_y; g.max_y = (float)(int)g.max_y;
    FuseConsts P{};
    P.th = params->th;
    P.log_scale_factor = std::log(c->p.scale_factor);  // mfLogScaleFactor, float
    P.n_levels = c->p.nlevels;
    for (int l = 0; l < 8; l++) P.inv_sigma2[l] = l < c->p.nlevels ? c->inv_sigma2[l] : 0.f;
    MatchCurrent cur{d_keys_un, d_desc, d_uright, d_grid_off, d_grid_idx, d_counts, cap};
    HIP_CHECK(c, fuse_search_launch(n_problems, d_problems, d_points, max_points, cur, g, P, d_skip, d_results,
                                    d_nfused, (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_fuse_search(spslam_ctx* c, const float* Tcw, const spslam_local_point* points, int n_points,
                       const spslam_keypoint* keys_un, const uint8_t* desc, const float* uright, int n_kp,
                       const int32_t* grid_off, const int32_t* grid_idx, const uint8_t* skip,
                       const spslam_fuse_params* params, spslam_fuse_result* results, int* nfused) {
    if (!c || !Tcw || !params || !grid_off || !nfused || n_kp < 0 || n_points < 0 ||
        (n_points && (!points || !results)) || (n_kp && (!keys_un || !desc || !uright || !grid_idx)))
        return SPSLAM_ERR_ARG;
    constexpr int kCells = SPSLAM_GRID_COLS * SPSLAM_GRID_ROWS;
    if (grid_off[0] != 0 || grid_off[kCells] > n_kp)
        return fail(c, SPSLAM_ERR_ARG, "grid CSR does not fit the keypoints%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    spslam_fuse_problem F{};
    std::memcpy(F.Tcw, Tcw, sizeof F.Tcw);
    F.n_points = n_points;
    const int np = n_points, cap = std::max(n_kp, 1);
    const size_t K = (size_t)n_kp, C = (size_t)cap, N = (size_t)std::max(np, 1);
    Stage st(c);
    if (int rc = st.open({{&F, sizeof F}, {points, np * sizeof(spslam_local_point), N * sizeof(spslam_local_point)},
                           {keys_un, K * sizeof(spslam_keypoint), C * sizeof(spslam_keypoint)},
                           {desc, K * 32, C * 32}, {uright, K * 4, C * 4},
                           {grid_off, (kCells + 1) * 4}, {grid_idx, (size_t)grid_off[kCells] * 4, C * 4},
                           {&n_kp, sizeof(int)}, {skip, skip ? (size_t)np : 0, N},
                           N * sizeof(spslam_fuse_result), sizeof(int)}))
        return rc;
    int rc = spslam_fuse_search_batch_device(
        c, 1, st.slot<spslam_fuse_problem>(0), st.slot<spslam_local_point>(1), np, st.slot<spslam_keypoint>(2),
        st.slot<uint8_t>(3), st.slot<float>(4), st.slot<int32_t>(5), st.slot<int32_t>(6), st.slot<int>(7), cap,
        skip ? st.slot<uint8_t>(8) : nullptr, params, st.slot<spslam_fuse_result>(9), st.slot<int>(10), c->stream);
    if (rc) return rc;
    if (np)
        HIP_CHECK(c, hipMemcpyAsync(results, st.slot<void>(9), (size_t)np * sizeof(spslam_fuse_result),
                                    hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(nfused, st.slot<int>(10), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

int spslam_map_points_refresh_batch_device(spslam_ctx* c, const spslam_point_refresh_map* map, const int32_t* d_rows,
                                           int n, int what, const spslam_keypoint* d_keys_un, const uint8_t* d_desc,
                                           int cap, uint8_t* d_status, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    constexpr int kAll = SPSLAM_REFRESH_DESCRIPTOR | SPSLAM_REFRESH_NORMAL_DEPTH;
    if (!map || n < 0 || (n && (!d_rows || !d_status)) || what < 1 || (what & ~kAll) || cap < 1 || cap > (1 << 20))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_map_points_refresh_batch_device");
    const spslam_point_refresh_map& m = *map;
    if (!m.obs_off || !m.obs_kf || !m.obs_kp || !m.kf_slot || !m.points ||
        ((what & SPSLAM_REFRESH_DESCRIPTOR) && !d_desc) ||
        ((what & SPSLAM_REFRESH_NORMAL_DEPTH) && (!m.kf_Tcw || !m.ref_kf || !d_keys_un)))
        return fail(c, SPSLAM_ERR_ARG, "missing buffer for spslam_map_points_refresh_batch_device%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    RefreshConsts P{};
    P.n_levels = c->p.nlevels;
    for (int l = 0; l < 8; l++) P.scale[l] = l < c->p.nlevels ? c->scale[l] : 0.f;
    HIP_CHECK(c, map_points_refresh_launch(m, d_rows, n, what, d_keys_un, d_desc, cap, P, d_status,
                                           (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_map_points_refresh(spslam_ctx* c, const spslam_point_refresh_map* map, int n_kf, int n_rows,
                              const int32_t* rows, int n, int what, const spslam_keypoint* keys_un,
                              const uint8_t* desc, int cap, int n_slots, uint8_t* status) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!map || n_kf < 0 || n_rows < 0 || n < 0 || (n && (!rows || !status)) || cap < 1 || n_slots < 0 ||
        !map->obs_off || (n_rows && !map->points) || (n_kf && (!map->kf_Tcw || !map->kf_slot)) ||
        (n_rows && !map->ref_kf) || ((size_t)n_slots * cap && (!keys_un || !desc)))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_map_points_refresh");
    const spslam_point_refresh_map& m = *map;
    const int n_obs = m.obs_off[n_rows];
    if (m.obs_off[0] != 0 || n_obs < 0 || (n_obs && (!m.obs_kf || !m.obs_kp)))
        return fail(c, SPSLAM_ERR_ARG, "spslam_map_points_refresh: the CSR does not start at 0 or lacks its arrays%s", "");
    // every index the kernel follows, checked here: the device form trusts its tables
    bool ok = true;
    for (int r = 0; r < n_rows; r++) ok = ok && m.obs_off[r] <= m.obs_off[r + 1];
    for (int k = 0; k < n; k++) ok = ok && rows[k] >= 0 && rows[k] < n_rows;
    for (int k = 0; k < n_kf; k++) ok = ok && m.kf_slot[k] >= 0 && m.kf_slot[k] < n_slots;
    for (int o = 0; o < n_obs && ok; o++)
        ok = m.obs_kf[o] >= 0 && m.obs_kf[o] < n_kf && m.obs_kp[o] >= 0 && m.obs_kp[o] < cap;
    if (!ok) return fail(c, SPSLAM_ERR_ARG, "spslam_map_points_refresh: an index outside its table%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    const size_t R = (size_t)n_rows, K = (size_t)n_kf, O = (size_t)n_obs, S = (size_t)n_slots * cap,
                 Pt = sizeof(spslam_local_point), Kp = sizeof(spslam_keypoint);
    const auto one = [](size_t x) { return std::max(x, (size_t)1); };
    Stage st(c);
    if (int rc = st.open({{m.kf_Tcw, K * 64, one(K) * 64}, {m.kf_slot, K * 4, one(K) * 4},
                           {m.kf_bad, m.kf_bad ? K : 0, one(K)}, {m.obs_off, (R + 1) * 4},
                           {m.obs_kf, O * 4, one(O) * 4}, {m.obs_kp, O * 4, one(O) * 4},
                           {m.ref_kf, R * 4, one(R) * 4}, {m.point_bad, m.point_bad ? R : 0, one(R)},
                           {m.points, R * Pt, one(R) * Pt}, {rows, (size_t)n * 4, one((size_t)n) * 4},
                           {keys_un, S * Kp, one(S) * Kp}, {desc, S * 32, one(S) * 32}, one((size_t)n)}))
        return rc;
    spslam_point_refresh_map dm{};
    dm.kf_Tcw = st.slot<float>(0);
    dm.kf_slot = st.slot<int32_t>(1);
    dm.kf_bad = m.kf_bad ? st.slot<uint8_t>(2) : nullptr;
    dm.obs_off = st.slot<int32_t>(3);
    dm.obs_kf = st.slot<int32_t>(4);
    dm.obs_kp = st.slot<int32_t>(5);
    dm.ref_kf = st.slot<int32_t>(6);
    dm.point_bad = m.point_bad ? st.slot<uint8_t>(7) : nullptr;
    dm.points = st.slot<spslam_local_point>(8);
    int rc = spslam_map_points_refresh_batch_device(c, &dm, st.slot<int32_t>(9), n, what, st.slot<spslam_keypoint>(10),
                                                    st.slot<uint8_t>(11), cap, st.slot<uint8_t>(12), c->stream);
    if (rc) return rc;
    if (n) {
        HIP_CHECK(c, hipMemcpyAsync(m.points, dm.points, R * Pt, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(c, hipMemcpyAsync(status, st.slot<uint8_t>(12), (size_t)n, hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < n; k++)
        if (status[k] == SPSLAM_REFRESH_CAPACITY)
            return fail(c, SPSLAM_ERR_CAPACITY, "spslam_map_points_refresh: a row has more than %s observers", "128");
    return SPSLAM_OK;
}

int spslam_track_graph_batch_device(spslam_ctx* c, int n_frames, int stage, const spslam_track_batch* batch,
                                    void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_frames < 1 || !batch || stage < SPSLAM_TRACK_MOTION_MODEL || stage > SPSLAM_TRACK_LAST_FRAME)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_track_graph_batch_device");
    const spslam_track_batch& b = *batch;
    const bool common = b.kp_counts && b.cap >= 1 && b.cap <= (1 << 20) && b.proj_frames && b.proj_match &&
                        b.proj_points && b.edge_of_kp;
    bool ok = common;
    if (stage == SPSLAM_TRACK_MOTION_PRIOR) {
        ok = b.proj_frames && b.velocity;
    } else if (stage == SPSLAM_TRACK_LAST_FRAME) {
        ok = common && b.keys_un && b.local_frames && b.local_points && b.local_match && b.results &&
             b.point_outlier && b.point_outlier_local && b.next_frames && b.next_points && b.velocity;
    } else if (stage == SPSLAM_TRACK_DISCARD) {
        ok = ok && b.taken && b.local_frames && b.results && b.point_outlier;
        if (b.next_match)  // the plane-outlier discard needs the first association and its edge flags
            ok = ok && b.next_parallel && b.next_vertical && b.plane_outlier && b.assoc_match && b.assoc_parallel &&
                 b.assoc_vertical && b.cap_a >= 0 && b.cap_b >= 0 && (b.cap_a == 0 || b.count_a) &&
                 (b.cap_b == 0 || b.count_b);
    } else {
        ok = ok && b.keys_un && b.uright && b.problems && b.points && b.cap_a >= 0 && b.cap_b >= 0 &&
             (b.cap_a == 0 || (b.planes_a && b.count_a && b.stride_a >= 16)) &&
             (b.cap_b == 0 || (b.planes_b && b.count_b && b.stride_b >= 16)) &&
             (b.cap_a + b.cap_b == 0 || (b.planes && b.map && b.assoc_match && b.assoc_parallel && b.assoc_vertical));
        if (stage == SPSLAM_TRACK_LOCAL_MAP)
            ok = ok && b.local_frames && b.local_points && b.local_match && b.results && b.point_outlier;
    }
    static const char* names[5] = {"MOTION_MODEL", "DISCARD", "LOCAL_MAP", "MOTION_PRIOR", "LAST_FRAME"};
    if (!ok) return fail(c, SPSLAM_ERR_ARG, "missing buffer for stage %s of spslam_track_graph_batch_device",
                         names[stage]);
    HIP_CHECK(c, hipSetDevice(c->device));
    TrackArgs a{};
    a.b = b;
    if (b.cap_b == 0) a.b.count_b = nullptr;
    for (int l = 0; l < kMaxLevels; l++)
        a.inv_sigma2[l] = c->inv_sigma2[std::min<int>(l, (int)c->inv_sigma2.size() - 1)];
    HIP_CHECK(c, track_launch(n_frames, stage, a, (hipStream_t)hip_stream, c->timer));
    return SPSLAM_OK;
}

int spslam_track_refkf_batch_device(spslam_ctx* c, int n_frames, int stage, const spslam_track_batch* mm,
                                    const spslam_refkf_batch* rk, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_frames < 1 || !mm || !rk || (stage != SPSLAM_REFKF_PREPARE && stage != SPSLAM_REFKF_SELECT))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_track_refkf_batch_device");
    const spslam_track_batch& b = *mm;
    const spslam_refkf_batch& r = *rk;
    bool ok = b.kp_counts && b.cap >= 1 && b.cap <= (1 << 20) && b.proj_frames && b.proj_points && b.proj_match &&
              b.edge_of_kp && b.point_outlier && r.nmatches && r.fallback;
    if (stage == SPSLAM_REFKF_PREPARE)
        ok = ok && b.problems && b.planes && b.plane_outlier && r.refkf_counts;
    else
        ok = ok && r.bow_nmatches && r.bow_match && r.refkf_rows && r.refkf_index && r.rows_stride >= 1 &&
             r.refkf_sets && r.assoc_frames && r.apply && r.refkf_match && r.refkf_frames && r.refkf_assoc &&
             (!b.seen || b.local_frames);
    if (!ok)
        return fail(c, SPSLAM_ERR_ARG, "missing buffer for spslam_track_refkf_batch_device stage %s",
                    stage == SPSLAM_REFKF_PREPARE ? "PREPARE" : "SELECT");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, refkf_launch(n_frames, stage, b, r, (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_track_refkf_vote_batch_device(spslam_ctx* c, int n_frames, const spslam_track_batch* mm,
                                         const spslam_refkf_vote* vote, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_frames < 1 || !mm || !vote)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_track_refkf_vote_batch_device");
    const spslam_track_batch& b = *mm;
    const spslam_refkf_vote& v = *vote;
    if (v.n_kf < 1 || v.n_kf > 1024 || v.ids_per_kf < 1 || v.new_kf >= v.n_kf)
        return fail(c, SPSLAM_ERR_ARG, "spslam_track_refkf_vote_batch_device: n_kf outside 1 .. 1024, ids_per_kf < 1 "
                    "or new_kf >= n_kf%s", "");
    const bool ok = b.kp_counts && b.cap >= 1 && b.cap <= (1 << 20) && b.proj_frames && b.proj_points &&
                    b.proj_match && b.edge_of_kp && b.point_outlier && v.kf_base && v.kf_sets && v.refkf_index &&
                    v.refkf_sets;
    if (!ok) return fail(c, SPSLAM_ERR_ARG, "missing buffer for spslam_track_refkf_vote_batch_device%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, refkf_vote_launch(n_frames, b, v, (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_track_update_local_map_batch_device(spslam_ctx* c, int n_frames, const spslam_track_batch* mm,
                                               const spslam_local_map* map, const spslam_local_map_out* out,
                                               void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_frames < 1 || !map || !out)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_track_update_local_map_batch_device");
    const spslam_local_map& m = *map;
    const spslam_local_map_out& o = *out;
    if (m.n_kf < 1 || m.n_kf > 1024)
        return fail(c, SPSLAM_ERR_ARG, "spslam_track_update_local_map_batch_device: n_kf outside 1 .. 1024%s", "");
    if (o.capacity < 0 || o.kf_cap < 0 || o.scratch_stride < 0 || o.kf_cap < m.n_kf)
        return fail(c, SPSLAM_ERR_ARG, "spslam_track_update_local_map_batch_device: negative capacity, kf_cap or "
                    "scratch_stride, or kf_cap < n_kf%s", "");
    bool ok = m.kf_base && m.row_base && m.obs_off && m.obs_kf && m.covis && m.child_off && m.child && m.parent &&
              m.match_off && m.match_row && o.local_kfs && o.n_local_kfs && o.kf_max && o.local_rows && o.n_local &&
              o.status && o.scratch && (!o.records || m.points);
    if (m.frame_rows)
        ok = ok && m.kp_counts && m.cap >= 1 && m.cap <= (1 << 20);
    else
        ok = ok && mm && mm->kp_counts && mm->cap >= 1 && mm->cap <= (1 << 20) && mm->proj_frames &&
             mm->proj_points && mm->proj_match && mm->edge_of_kp && mm->point_outlier;
    if (!ok) return fail(c, SPSLAM_ERR_ARG, "missing buffer for spslam_track_update_local_map_batch_device%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, update_local_map_launch(n_frames, m.frame_rows ? nullptr : mm, m, o, (hipStream_t)hip_stream,
                                         c->timer));
    return SPSLAM_OK;
}

int spslam_track_update_local_map(spslam_ctx* c, const spslam_local_map* map, int n_rows, int n_kp,
                                  const spslam_local_map_out* out) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!map || !out || n_rows < 0 || n_kp < 0)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_track_update_local_map");
    const spslam_local_map& m = *map;
    const spslam_local_map_out& o = *out;
    if (m.n_kf < 1 || m.n_kf > 1024)
        return fail(c, SPSLAM_ERR_ARG, "spslam_track_update_local_map: n_kf outside 1 .. 1024%s", "");
    if (o.capacity < 0) return fail(c, SPSLAM_ERR_ARG, "spslam_track_update_local_map: negative capacity%s", "");
    if ((n_kp && !m.frame_rows) || !m.obs_off || !m.covis || !m.child_off || !m.parent || !m.match_off ||
        !o.local_kfs || !o.n_local_kfs || !o.kf_max || !o.n_local || !o.status || (o.capacity && !o.local_rows) ||
        (o.records && !m.points && n_rows))
        return fail(c, SPSLAM_ERR_ARG, "missing buffer for spslam_track_update_local_map%s", "");
    const int nk = m.n_kf, n_obs = m.obs_off[n_rows], n_child = m.child_off[nk], n_match = m.match_off[nk];
    if (m.obs_off[0] != 0 || m.child_off[0] != 0 || m.match_off[0] != 0 || n_obs < 0 || n_child < 0 || n_match < 0 ||
        (n_obs && !m.obs_kf) || (n_child && !m.child) || (n_match && !m.match_row) || *o.n_local_kfs < 0 ||
        *o.n_local_kfs > nk)
        return fail(c, SPSLAM_ERR_ARG, "spslam_track_update_local_map: a CSR does not start at 0 or lacks its "
                    "array, or n_local_kfs outside 0 .. n_kf%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    const size_t R = (size_t)n_rows, K = (size_t)nk, C = (size_t)o.capacity, P = sizeof(spslam_local_point);
    const int cap = std::max(n_kp, 1);
    // {keypoints, base 0, n_local_kfs, kf_max, n_local, status}
    int32_t hdr[6] = {n_kp, 0, *o.n_local_kfs, -1, 0, 0};
    spslam_local_frame lf{};
    const bool with_frame = o.records && o.local_frames;
    if (with_frame) lf = *o.local_frames;
    Stage st(c);
    if (int rc = st.open({{hdr, sizeof hdr},
                           {m.frame_rows, (size_t)n_kp * 4, (size_t)cap * 4},
                           {m.obs_off, (R + 1) * 4}, {m.obs_kf, (size_t)n_obs * 4, std::max(n_obs, 1) * (size_t)4},
                           {m.point_bad, m.point_bad ? R : 0, std::max(R, (size_t)1)},
                           {m.kf_bad, m.kf_bad ? K : 0, K}, {m.covis, K * 40}, {m.child_off, (K + 1) * 4},
                           {m.child, (size_t)n_child * 4, std::max(n_child, 1) * (size_t)4}, {m.parent, K * 4},
                           {m.match_off, (K + 1) * 4},
                           {m.match_row, (size_t)n_match * 4, std::max(n_match, 1) * (size_t)4},
                           {m.points, o.records ? R * P : 0, std::max(R, (size_t)1) * P},
                           {o.local_kfs, (size_t)*o.n_local_kfs * 4, K * 4}, std::max(C, (size_t)1) * 4,
                           std::max(R, (size_t)1) * 4, std::max(C, (size_t)1) * P, {&lf, sizeof lf}}))
        return rc;
    int32_t* d_hdr = st.slot<int32_t>(0);
    spslam_local_map dm{};
    dm.frame_rows = st.slot<int32_t>(1);
    dm.kp_counts = d_hdr;
    dm.kf_base = dm.row_base = d_hdr + 1;
    dm.cap = cap;
    dm.n_kf = nk;
    dm.obs_off = st.slot<int32_t>(2);
    dm.obs_kf = st.slot<int32_t>(3);
    dm.point_bad = m.point_bad ? st.slot<uint8_t>(4) : nullptr;
    dm.points = st.slot<spslam_local_point>(12);
    dm.kf_bad = m.kf_bad ? st.slot<uint8_t>(5) : nullptr;
    dm.covis = st.slot<int32_t>(6);
    dm.child_off = st.slot<int32_t>(7);
    dm.child = st.slot<int32_t>(8);
    dm.parent = st.slot<int32_t>(9);
    dm.match_off = st.slot<int32_t>(10);
    dm.match_row = st.slot<int32_t>(11);
    spslam_local_map_out dout{};
    dout.local_kfs = st.slot<int32_t>(13);
    dout.n_local_kfs = d_hdr + 2;
    dout.kf_max = d_hdr + 3;
    dout.n_local = d_hdr + 4;
    dout.status = d_hdr + 5;
    dout.local_rows = st.slot<int32_t>(14);
    dout.scratch = st.slot<int32_t>(15);  // deliberately not cleared: the kernel does not read what it held
    dout.kf_cap = nk;
    dout.capacity = o.capacity;
    dout.scratch_stride = n_rows;
    dout.records = o.records ? st.slot<spslam_local_point>(16) : nullptr;
    dout.local_frames = with_frame ? st.slot<spslam_local_frame>(17) : nullptr;
    int rc = spslam_track_update_local_map_batch_device(c, 1, nullptr, &dm, &dout, c->stream);
    if (rc) return rc;
    HIP_CHECK(c, hipMemcpyAsync(hdr, d_hdr, sizeof hdr, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    *o.n_local_kfs = hdr[2];
    *o.kf_max = hdr[3];
    *o.n_local = hdr[4];
    *o.status = hdr[5];
    if (hdr[2]) HIP_CHECK(c, hipMemcpyAsync(o.local_kfs, dout.local_kfs, (size_t)hdr[2] * 4, hipMemcpyDeviceToHost, c->stream));
    if (hdr[4]) {
        HIP_CHECK(c, hipMemcpyAsync(o.local_rows, dout.local_rows, (size_t)hdr[4] * 4, hipMemcpyDeviceToHost, c->stream));
        if (o.records)
            HIP_CHECK(c, hipMemcpyAsync(o.records, dout.records, (size_t)hdr[4] * P, hipMemcpyDeviceToHost, c->stream));
    }
    if (with_frame)
        HIP_CHECK(c, hipMemcpyAsync(o.local_frames, dout.local_frames, sizeof lf, hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

int spslam_masked_frame_copy_device(spslam_ctx* c, int n_frames, const uint8_t* flags, int n_regions,
                                    const spslam_frame_region* regions, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_frames < 1 || !flags || n_regions < 0 || n_regions > kMaxFrameRegions || (n_regions && !regions))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_masked_frame_copy_device");
    FrameRegions G{};
    G.n = n_regions;
    for (int k = 0; k < n_regions; k++) {
        const spslam_frame_region& r = regions[k];
        if (!r.dst || !r.src || r.frame_bytes < 0 || r.frame_bytes % 4 || r.dst_stride % 4 || r.src_stride % 4 ||
            ((uintptr_t)r.dst | (uintptr_t)r.src) % 4 || r.frame_bytes > r.dst_stride || r.frame_bytes > r.src_stride)
            return fail(c, SPSLAM_ERR_ARG, "bad region of %s", "spslam_masked_frame_copy_device");
        G.r[k] = r;
    }
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, masked_frame_copy_launch(n_frames, flags, G, (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

// ---------------------------------------------------------------- bag of words
// TemplatedVocabulary::loadFromTextFile (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1424), host side,
// then one HBM blob: descriptors, children CSR, weights, word ids.
int spslam_bow_load_vocabulary(spslam_ctx* c, const char* text, size_t len, int* k_out, int* L_out, int* n_nodes_out,
                               int* n_words_out) {
    if (!c || (!text && len)) return SPSLAM_ERR_ARG;
    std::istringstream f(std::string(text ? text : "", len));
    std::string line;
    std::getline(f, line);
    std::stringstream ss;
    ss << line;
    int k = 0, L = 0, n1 = 0, n2 = 0;
    ss >> k >> L >> n1 >> n2;
    if (k < 0 || k > 20 || L < 1 || L > 10 || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3)
        return fail(c, SPSLAM_ERR_ARG, "vocabulary header is not DBoW2 text%s", "");
    std::vector<int> parent(1, 0);
    std::vector<std::vector<int>> children(1);
    std::vector<uint8_t> desc(32, 0);
    std::vector<double> weight(1, 0.0);
    std::vector<uint32_t> word(1, 0);
    uint32_t n_words = 0;
    while (!f.eof()) {  // the reference's loop: an empty last line still makes a node
        std::string sn;
        std::getline(f, sn);
        std::stringstream sl;
        sl << sn;
        const int nid = (int)parent.size();
        int pid = 0, leaf = 0;
        sl >> pid;
        if (pid < 0 || pid >= nid) return fail(c, SPSLAM_ERR_ARG, "vocabulary node with a bad parent%s", "");
        sl >> leaf;
        std::stringstream sd;
        for (int i = 0; i < 32; i++) {
            std::string e;
            sl >> e;
            sd << e << " ";
        }
        uint8_t d[32] = {0};  // FORB::fromString leaves unparsed bytes unset (uninitialised there, zero here)
        for (int i = 0; i < 32; i++) {
            int v;
            sd >> v;
            if (!sd.fail()) d[i] = (uint8_t)v;
        }
        double w = 0.0;
        sl >> w;
        parent.push_back(pid);
        children.emplace_back();
        children[pid].push_back(nid);
        desc.insert(desc.end(), d, d + 32);
        weight.push_back(w);
        word.push_back(leaf > 0 ? n_words++ : 0u);
    }
    const int n = (int)parent.size();
    std::vector<int> cbeg(n), ccnt(n), cids;
    cids.reserve(n);
    for (int i = 0; i < n; i++) {
        cbeg[i] = (int)cids.size();
        ccnt[i] = (int)children[i].size();
        cids.insert(cids.end(), children[i].begin(), children[i].end());
    }
    if (cids.empty()) cids.push_back(0);
    const size_t sz[] = {(size_t)n * 32, (size_t)n * 4, (size_t)n * 4, cids.size() * 4, (size_t)n * 8, (size_t)n * 4};
    size_t off[6], bytes = 0;
    for (int i = 0; i < 6; i++) { off[i] = bytes; bytes += (sz[i] + 255) / 256 * 256; }
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    c->vocab = VocabDev{};
    HIP_CHECK(c, c->d_vocab.alloc(bytes));
    const void* src[] = {desc.data(), cbeg.data(), ccnt.data(), cids.data(), weight.data(), word.data()};
    for (int i = 0; i < 6; i++) HIP_CHECK(c, hipMemcpy(c->d_vocab + off[i], src[i], sz[i], hipMemcpyHostToDevice));
    VocabDev& V = c->vocab;
    V.n_nodes = n; V.k = k; V.L = L; V.scoring = n1; V.weighting = n2;
    V.desc = (const uint4*)(c->d_vocab + off[0]);
    V.child_begin = (const int*)(c->d_vocab + off[1]);
    V.child_count = (const int*)(c->d_vocab + off[2]);
    V.child_ids = (const int*)(c->d_vocab + off[3]);
    V.weight = (const double*)(c->d_vocab + off[4]);
    V.word_id = (const uint32_t*)(c->d_vocab + off[5]);
    if (k_out) *k_out = k;
    if (L_out) *L_out = L;
    if (n_nodes_out) *n_nodes_out = n;
    if (n_words_out) *n_words_out = (int)n_words;
    return SPSLAM_OK;
}

int spslam_bow_transform_batch_device(spslam_ctx* c, int n_frames, const uint8_t* d_desc, const int* d_counts,
                                      int cap, int levelsup, uint32_t* d_bow_words, double* d_bow_values,
                                      int* d_n_bow, uint32_t* d_fv_nodes, int32_t* d_fv_start,
                                      int32_t* d_fv_features, int* d_n_fv, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->d_vocab) return fail(c, SPSLAM_ERR_NOT_READY, "no vocabulary loaded (spslam_bow_load_vocabulary)%s", "");
    if (n_frames < 1 || !d_desc || !d_counts || cap < 1 || cap > 8192 || !d_bow_words || !d_bow_values || !d_n_bow ||
        !d_fv_nodes || !d_fv_start || !d_fv_features || !d_n_fv)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_bow_transform_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;
    if (c->vocab.n_nodes < 2) {  // empty vocabulary: transform clears both vectors
        HIP_CHECK(c, hipMemsetAsync(d_n_bow, 0, (size_t)n_frames * sizeof(int), s));
        HIP_CHECK(c, hipMemsetAsync(d_n_fv, 0, (size_t)n_frames * sizeof(int), s));
        return SPSLAM_OK;
    }
    const size_t n = (size_t)n_frames * cap;
    const size_t need = n * 16 + 512;
    HIP_CHECK(c, c->d_bow_scratch.reserve(need, s));
    auto* s_weight = (double*)c->d_bow_scratch.p;
    auto* s_word = (uint32_t*)(c->d_bow_scratch + ((n * 8 + 255) & ~(size_t)255));
    auto* s_node = s_word + ((n + 63) & ~(size_t)63);
    BowOut out{d_bow_words, d_bow_values, d_n_bow, d_fv_nodes, d_fv_start, d_fv_features, d_n_fv};
    HIP_CHECK(c, bow_transform_launch(c->vocab, n_frames, d_desc, d_counts, cap, levelsup, s_word, s_weight, s_node,
                                      out, s, c->timer));
    return SPSLAM_OK;
}

int spslam_bow_transform(spslam_ctx* c, const uint8_t* desc, int n, int levelsup, uint32_t* bow_words,
                         double* bow_values, int* n_bow, uint32_t* fv_nodes, int32_t* fv_start,
                         int32_t* fv_features, int* n_fv) {
    if (!c || n < 0 || (n && !desc) || !n_bow || !n_fv || n > 8192 || !fv_start ||
        (n && (!bow_words || !bow_values || !fv_nodes || !fv_features)))
        return SPSLAM_ERR_ARG;
    if (!c->d_vocab) return fail(c, SPSLAM_ERR_NOT_READY, "no vocabulary loaded (spslam_bow_load_vocabulary)%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    const int cap = std::max(n, 1);
    const size_t C = (size_t)cap;
    Stage st(c);
    if (int rc = st.open({{desc, (size_t)n * 32, C * 32}, {&n, 4}, C * 4, C * 8, 4, C * 4, (C + 1) * 4, C * 4, 4},
                         &c->d_bow_stage))
        return rc;
    int rc = spslam_bow_transform_batch_device(c, 1, st.slot<uint8_t>(0), st.slot<int>(1), cap, levelsup,
                                               st.slot<uint32_t>(2), st.slot<double>(3), st.slot<int>(4),
                                               st.slot<uint32_t>(5), st.slot<int32_t>(6), st.slot<int32_t>(7),
                                               st.slot<int>(8), c->stream);
    if (rc) return rc;
    HIP_CHECK(c, hipMemcpyAsync(n_bow, st.slot<int>(4), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(n_fv, st.slot<int>(8), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    if (*n_bow) {
        HIP_CHECK(c, hipMemcpy(bow_words, st.slot<void>(2), (size_t)*n_bow * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(c, hipMemcpy(bow_values, st.slot<void>(3), (size_t)*n_bow * 8, hipMemcpyDeviceToHost));
    }
    if (*n_fv) {
        HIP_CHECK(c, hipMemcpy(fv_nodes, st.slot<void>(5), (size_t)*n_fv * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(c, hipMemcpy(fv_start, st.slot<void>(6), (size_t)(*n_fv + 1) * 4, hipMemcpyDeviceToHost));
        int m = 0;
        std::memcpy(&m, fv_start + *n_fv, 4);
        if (m) HIP_CHECK(c, hipMemcpy(fv_features, st.slot<void>(7), (size_t)m * 4, hipMemcpyDeviceToHost));
    } else {
        fv_start[0] = 0;
    }
    return SPSLAM_OK;
}

int spslam_search_by_bow_batch_device(spslam_ctx* c, int n_pairs, const int32_t* d_pairs,
                                      const spslam_bow_side* kf, const spslam_bow_side* fr,
                                      const spslam_bow_params* params, int32_t* d_match, int* d_nmatches,
                                      void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    auto side_ok = [](const spslam_bow_side* b, bool keyframe) {
        return b && b->desc && b->keys && b->counts && b->fv_nodes && b->fv_start && b->fv_features && b->n_fv &&
               b->cap >= 1 && b->cap <= 8192 && (!keyframe || b->has_point);
    };
    if (n_pairs < 1 || !d_pairs || !side_ok(kf, true) || !side_ok(fr, false) || !params || !d_match || !d_nmatches)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_search_by_bow_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    BowSide K{kf->desc, kf->keys, kf->has_point, kf->counts, kf->fv_nodes, kf->fv_start, kf->fv_features, kf->n_fv,
              kf->cap};
    BowSide F{fr->desc, fr->keys, nullptr, fr->counts, fr->fv_nodes, fr->fv_start, fr->fv_features, fr->n_fv, fr->cap};
    HIP_CHECK(c, bow_search_launch(n_pairs, (const int2*)d_pairs, K, F, params->nn_ratio, params->check_orientation,
                                   d_match, d_nmatches, (hipStream_t)hip_stream, c->timer));
    return SPSLAM_OK;
}

int spslam_search_by_bow(spslam_ctx* c, const uint8_t* kf_desc, const spslam_keypoint* kf_keys,
                         const uint8_t* kf_has_point, int kf_n, const uint32_t* kf_fv_nodes,
                         const int32_t* kf_fv_start, const int32_t* kf_fv_features, int kf_n_fv,
                         const uint8_t* f_desc, const spslam_keypoint* f_keys, int f_n, const uint32_t* f_fv_nodes,
                         const int32_t* f_fv_start, const int32_t* f_fv_features, int f_n_fv,
                         const spslam_bow_params* params, int32_t* match, int* nmatches) {
    if (!c || !params || !nmatches || kf_n < 0 || f_n < 0 || kf_n > 8192 || f_n > 8192 || kf_n_fv < 0 ||
        f_n_fv < 0 || kf_n_fv > std::max(kf_n, 1) || f_n_fv > std::max(f_n, 1) || !kf_fv_start || !f_fv_start ||
        (kf_n && (!kf_desc || !kf_keys || !kf_has_point)) || (f_n && (!f_desc || !f_keys || !match)) ||
        (kf_n_fv && (!kf_fv_nodes || !kf_fv_features)) || (f_n_fv && (!f_fv_nodes || !f_fv_features)))
        return SPSLAM_ERR_ARG;
    const int kc = std::max(kf_n, 1), fc = std::max(f_n, 1);
    const int km = kf_fv_start[kf_n_fv], fm = f_fv_start[f_n_fv];
    if (km < 0 || km > kf_n || fm < 0 || fm > f_n)
        return fail(c, SPSLAM_ERR_ARG, "FeatureVector does not fit the features%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    // keyframe slot 0 and frame slot 0 of a one-pair batch
    const size_t kn = (size_t)kf_n, fn = (size_t)f_n, KC = (size_t)kc, FC = (size_t)fc;
    const int32_t pair[2] = {0, 0};
    Stage st(c);
    constexpr size_t kKp = sizeof(spslam_keypoint);
    if (int rc = st.open({{kf_desc, kn * 32, KC * 32}, {kf_keys, kn * kKp, KC * kKp}, {kf_has_point, kn, KC},
                           {&kf_n, 4}, {kf_fv_nodes, (size_t)kf_n_fv * 4, KC * 4},
                           {kf_fv_start, (size_t)(kf_n_fv + 1) * 4, (KC + 1) * 4},
                           {kf_fv_features, (size_t)km * 4, KC * 4}, {&kf_n_fv, 4},
                           {f_desc, fn * 32, FC * 32}, {f_keys, fn * kKp, FC * kKp}, {&f_n, 4},
                           {f_fv_nodes, (size_t)f_n_fv * 4, FC * 4},
                           {f_fv_start, (size_t)(f_n_fv + 1) * 4, (FC + 1) * 4},
                           {f_fv_features, (size_t)fm * 4, FC * 4}, {&f_n_fv, 4}, {pair, 8}, FC * 4, 4},
                         &c->d_bow_stage))
        return rc;
    spslam_bow_side K{st.slot<uint8_t>(0), st.slot<spslam_keypoint>(1), st.slot<uint8_t>(2), st.slot<int>(3),
                      st.slot<uint32_t>(4), st.slot<int32_t>(5), st.slot<int32_t>(6), st.slot<int>(7), kc, 0};
    spslam_bow_side F{st.slot<uint8_t>(8), st.slot<spslam_keypoint>(9), nullptr, st.slot<int>(10),
                      st.slot<uint32_t>(11), st.slot<int32_t>(12), st.slot<int32_t>(13), st.slot<int>(14), fc, 0};
    int rc = spslam_search_by_bow_batch_device(c, 1, st.slot<int32_t>(15), &K, &F, params, st.slot<int32_t>(16),
                                               st.slot<int>(17), c->stream);
    if (rc) return rc;
    if (f_n) HIP_CHECK(c, hipMemcpyAsync(match, st.slot<int32_t>(16), fn * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(nmatches, st.slot<int>(17), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- CreateNewMapPoints
namespace {

// Frame.cc:118-124 (invfx = 1.0f/fx, mb = mbf/fx), LocalMapping.cc:245 (ratioFactor = 1.5f*mfScaleFactor)
TriConsts tri_consts(const spslam_ctx* c) {
    TriConsts C{};
    C.fx = c->fg.fx; C.fy = c->fg.fy; C.cx = c->fg.cx; C.cy = c->fg.cy; C.bf = c->fg.bf;
    C.invfx = 1.0f / C.fx;
    C.invfy = 1.0f / C.fy;
    C.mb = C.bf / C.fx;
    C.ratio_factor = 1.5f * (float)c->p.scale_factor;
    for (int l = 0; l < 8; l++) {
        C.scale[l] = l < c->p.nlevels ? c->scale[l] : 0.f;
        C.sigma2[l] = l < c->p.nlevels ? c->sigma2[l] : 0.f;
    }
    return C;
}

bool tri_side_ok(const spslam_tri_side* s) {
    return s && s->keys && s->keys_un && s->uright && s->depth && s->desc && s->has_point && s->counts &&
           s->fv_nodes && s->fv_start && s->fv_features && s->n_fv && s->cap >= 1 && s->cap <= 8192;
}

bool tri_keyframe_ok(const spslam_tri_keyframe* k) {
    if (!k || k->n < 0 || k->n > 8192 || k->n_fv < 0 || k->n_fv > std::max(k->n, 1) || !k->fv_start) return false;
    if (k->n && (!k->keys || !k->keys_un || !k->uright || !k->depth || !k->desc || !k->has_point)) return false;
    if (k->n_fv && (!k->fv_nodes || !k->fv_features)) return false;
    const int m = k->fv_start[k->n_fv];
    return k->fv_start[0] == 0 && m >= 0 && m <= k->n;
}

// The two keyframes of a drop-in call as slots 0 and 1 of a batch of cap keypoints, with one pair record.
struct TriStage {
    Stage st;
    spslam_tri_side side{};
    int cap = 1;
    explicit TriStage(spslam_ctx* c) : st(c) {}
    // slots: 0 pair, 1..10 the side's arrays, 11 match12, 12 results, 13 {nmatches, n_new}
    int open(spslam_ctx* c, const spslam_tri_keyframe* k[2], const float* F12, const int32_t* match12) {
        cap = std::max(std::max(k[0]->n, k[1]->n), 1);
        const size_t C = (size_t)cap, kKp = sizeof(spslam_keypoint);
        std::vector<uint8_t> h[10];
        const size_t unit[10] = {kKp, kKp, 4, 4, 32, 1, 4, 4, 4, 4};
        const size_t per_slot[10] = {C, C, C, C, C, C, 1, C, C + 1, C};
        for (int a = 0; a < 10; a++) h[a].assign(2 * per_slot[a] * unit[a], 0);
        for (int s = 0; s < 2; s++) {
            const spslam_tri_keyframe& q = *k[s];
            const size_t n = (size_t)q.n, nf = (size_t)q.n_fv, m = (size_t)q.fv_start[q.n_fv];
            const void* src[10] = {q.keys, q.keys_un, q.uright, q.depth, q.desc, q.has_point, &q.n, q.fv_nodes,
                                   q.fv_start, q.fv_features};
            const size_t cnt[10] = {n, n, n, n, n, n, 1, nf, nf + 1, m};
            for (int a = 0; a < 10; a++)
                if (cnt[a]) std::memcpy(h[a].data() + s * per_slot[a] * unit[a], src[a], cnt[a] * unit[a]);
        }
        const int32_t nfv[2] = {k[0]->n_fv, k[1]->n_fv};
        spslam_tri_pair P{};
        P.kf1 = 0; P.kf2 = 1;
        std::memcpy(P.Tcw1, k[0]->Tcw, sizeof P.Tcw1);
        std::memcpy(P.Tcw2, k[1]->Tcw, sizeof P.Tcw2);
        std::memcpy(P.Ow1, k[0]->Ow, sizeof P.Ow1);
        std::memcpy(P.Ow2, k[1]->Ow, sizeof P.Ow2);
        if (F12) std::memcpy(P.F12, F12, sizeof P.F12);
        if (int rc = st.open({{&P, sizeof P}, {h[0].data(), h[0].size()}, {h[1].data(), h[1].size()},
                              {h[2].data(), h[2].size()}, {h[3].data(), h[3].size()}, {h[4].data(), h[4].size()},
                              {h[5].data(), h[5].size()}, {h[6].data(), h[6].size()}, {h[7].data(), h[7].size()},
                              {h[8].data(), h[8].size()}, {h[9].data(), h[9].size()},
                              {match12, match12 ? C * 4 : 0, C * 4}, C * sizeof(spslam_tri_result), 8,
                              {nfv, sizeof nfv}}))
            return rc;
        // the uploads read the vectors above: they must be done before those go out of scope
        HIP_CHECK(c, hipStreamSynchronize(c->stream));
        side.keys = st.slot<spslam_keypoint>(1);
        side.keys_un = st.slot<spslam_keypoint>(2);
        side.uright = st.slot<float>(3);
        side.depth = st.slot<float>(4);
        side.desc = st.slot<uint8_t>(5);
        side.has_point = st.slot<uint8_t>(6);
        side.counts = st.slot<int>(7);
        side.fv_nodes = st.slot<uint32_t>(8);
        side.fv_start = st.slot<int32_t>(9);
        side.fv_features = st.slot<int32_t>(10);
        side.n_fv = st.slot<int>(14);
        side.cap = cap;
        return SPSLAM_OK;
    }
};

}  // namespace

extern "C" {

int spslam_search_for_triangulation_batch_device(spslam_ctx* c, int n_pairs, const spslam_tri_pair* d_pairs,
                                                 const spslam_tri_side* side, int only_stereo,
                                                 int check_orientation, int32_t* d_match12, int* d_nmatches,
                                                 void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_pairs < 1 || !d_pairs || !tri_side_ok(side) || !d_match12 || !d_nmatches)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_search_for_triangulation_batch_device");
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, triangulation_search_launch(n_pairs, d_pairs, *side, tri_consts(c), only_stereo != 0,
                                             check_orientation != 0, 0, d_match12, d_nmatches, nullptr,
                                             (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_triangulate_batch_device(spslam_ctx* c, int n_pairs, const spslam_tri_pair* d_pairs,
                                    const spslam_tri_side* side, const int32_t* d_match12, int mark,
                                    spslam_tri_result* d_results, int* d_n_new, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_pairs < 1 || !d_pairs || !tri_side_ok(side) || !d_match12 || !d_results || !d_n_new)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_triangulate_batch_device");
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, triangulate_launch(n_pairs, d_pairs, *side, tri_consts(c), d_match12, mark != 0, d_results, d_n_new,
                                    (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_create_new_points_batch_device(spslam_ctx* c, int n_pairs, const spslam_tri_pair* d_pairs,
                                          const spslam_tri_side* side, int32_t* d_match12, int* d_nmatches,
                                          spslam_tri_result* d_results, int* d_n_new, uint8_t* d_pair_status,
                                          void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_pairs < 1 || !d_pairs || !tri_side_ok(side) || !d_match12 || !d_nmatches || !d_results || !d_n_new ||
        !d_pair_status)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_create_new_points_batch_device");
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    const TriConsts C = tri_consts(c);
    hipStream_t s = (hipStream_t)hip_stream;
    // matcher(0.6, false).SearchForTriangulation(..., bOnlyStereo = false) (LocalMapping.cc:228, :283)
    HIP_CHECK(c, triangulation_search_launch(n_pairs, d_pairs, *side, C, 0, 0, 1, d_match12, d_nmatches,
                                             d_pair_status, s));
    HIP_CHECK(c, triangulate_launch(n_pairs, d_pairs, *side, C, d_match12, 1, d_results, d_n_new, s));
    return SPSLAM_OK;
}

int spslam_search_for_triangulation(spslam_ctx* c, const spslam_tri_keyframe* kf1, const spslam_tri_keyframe* kf2,
                                    const float* F12, int32_t* matched_pairs, int only_stereo,
                                    int check_orientation) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!tri_keyframe_ok(kf1) || !tri_keyframe_ok(kf2) || !F12 || (kf1->n && !matched_pairs))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_search_for_triangulation");
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    TriStage ts(c);
    const spslam_tri_keyframe* k[2] = {kf1, kf2};
    if (int rc = ts.open(c, k, F12, nullptr)) return rc;
    int rc = spslam_search_for_triangulation_batch_device(c, 1, ts.st.slot<spslam_tri_pair>(0), &ts.side, only_stereo,
                                                          check_orientation, ts.st.slot<int32_t>(11),
                                                          ts.st.slot<int>(13), c->stream);
    if (rc) return rc;
    std::vector<int32_t> match((size_t)ts.cap);
    int nmatches = 0;
    HIP_CHECK(c, hipMemcpyAsync(match.data(), ts.st.slot<int32_t>(11), match.size() * 4, hipMemcpyDeviceToHost,
                                c->stream));
    HIP_CHECK(c, hipMemcpyAsync(&nmatches, ts.st.slot<int>(13), 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = ts.st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    int n = 0;
    for (int i = 0; i < kf1->n; i++)  // vMatchedPairs: idx1 order (:811-816)
        if (match[i] >= 0) {
            matched_pairs[2 * n] = i;
            matched_pairs[2 * n + 1] = match[i];
            n++;
        }
    if (n != nmatches) return fail(c, SPSLAM_ERR_HIP, "spslam_search_for_triangulation: count mismatch%s", "");
    return nmatches;
}

int spslam_triangulate(spslam_ctx* c, const spslam_tri_keyframe* kf1, const spslam_tri_keyframe* kf2,
                       const int32_t* matched_pairs, int n_matches, spslam_tri_result* results, int* n_new) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!tri_keyframe_ok(kf1) || !tri_keyframe_ok(kf2) || n_matches < 0 || !n_new ||
        (n_matches && (!matched_pairs || !results)))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_triangulate");
    const int cap = std::max(std::max(kf1->n, kf2->n), 1);
    std::vector<int32_t> match((size_t)cap, -1);
    for (int k = 0; k < n_matches; k++) {
        const int i1 = matched_pairs[2 * k], i2 = matched_pairs[2 * k + 1];
        if (i1 < 0 || i1 >= kf1->n || i2 < 0 || i2 >= kf2->n || match[i1] >= 0)
            return fail(c, SPSLAM_ERR_ARG, "spslam_triangulate: a pair outside the keyframes or idx1 twice%s", "");
        match[i1] = i2;
    }
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    TriStage ts(c);
    const spslam_tri_keyframe* k[2] = {kf1, kf2};
    if (int rc = ts.open(c, k, nullptr, match.data())) return rc;
    int rc = spslam_triangulate_batch_device(c, 1, ts.st.slot<spslam_tri_pair>(0), &ts.side, ts.st.slot<int32_t>(11), 0,
                                             ts.st.slot<spslam_tri_result>(12), ts.st.slot<int>(13) + 1, c->stream);
    if (rc) return rc;
    std::vector<spslam_tri_result> rec((size_t)cap);
    HIP_CHECK(c, hipMemcpyAsync(rec.data(), ts.st.slot<void>(12), rec.size() * sizeof(spslam_tri_result),
                                hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(n_new, ts.st.slot<int>(13) + 1, 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = ts.st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    for (int q = 0; q < n_matches; q++) results[q] = rec[matched_pairs[2 * q]];
    return SPSLAM_OK;
}

}  // extern "C"
