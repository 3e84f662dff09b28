// C ABI (include/spslam_gpu.h): ORB extraction, the RGB-D frame stage and the grab stage.
#include "capi_ctx.h"

#include <cmath>

namespace {

// Point level 0 at the caller's frames and levels >= 1 at the context pyramid.
void bind_frames(spslam_ctx* c, const uint8_t* d_gray, size_t frame_stride, int stride) {
    OrbGeom& g = c->geom;
    g.lv[0].img = d_gray;
    g.lv[0].stride = stride;
    g.lv[0].frame_stride = (long long)frame_stride;
}

// cv::undistortPoints(point, K, D, noArray(), K), OpenCV 3.4 (frame_kernels.hip restates it for the device).
void undistort_host(const FrameGeom& g, float u, float v, float* ou, float* ov) {
    const double fx = g.fx, fy = g.fy, cx = g.cx, cy = g.cy, ifx = 1. / fx, ify = 1. / fy;
    const double k0 = g.dist[0], k1 = g.dist[1], k2 = g.dist[2], k3 = g.dist[3], k4 = g.dist[4];
    const double k5 = 0, k6 = 0, k7 = 0, k8 = 0, k9 = 0, k10 = 0, k11 = 0;
    double x = ((double)u - cx) * ifx, y = ((double)v - cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k7 * r2 + k6) * r2 + k5) * r2) / (1 + ((k4 * r2 + k1) * r2 + k0) * r2);
        const double deltaX = 2 * k2 * x * y + k3 * (r2 + 2 * x * x) + k8 * r2 + k9 * r2 * r2;
        const double deltaY = k2 * (r2 + 2 * y * y) + 2 * k3 * x * y + k10 * r2 + k11 * r2 * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    *ou = (float)((fx * x + 0. * y + cx) * (1. / (0. * x + 0. * y + 1.)));
    *ov = (float)((0. * x + fy * y + cy) * (1. / (0. * x + 0. * y + 1.)));
}

}  // namespace

extern "C" {

int spslam_orb_extract_batch_device(spslam_ctx* c, const uint8_t* d_gray, int n_frames, size_t frame_stride,
                                    int stride, spslam_keypoint* d_kps, uint8_t* d_desc, int* d_counts,
                                    int cap_per_frame, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!d_gray || !d_kps || !d_desc || !d_counts || n_frames < 1 || n_frames > c->p.max_batch ||
        stride < c->p.width || (n_frames > 1 && frame_stride < (size_t)stride * c->p.height) || cap_per_frame < 1)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_orb_extract_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the default stream (header)
    bind_frames(c, d_gray, frame_stride, stride);
    if (!c->orb_aux) {  // the small levels' chain (orb_launch)
        HIP_CHECK(c, hipStreamCreateWithFlags(&c->orb_aux, hipStreamNonBlocking));
        HIP_CHECK(c, hipEventCreateWithFlags(&c->orb_fork, hipEventDisableTiming));
        HIP_CHECK(c, hipEventCreateWithFlags(&c->orb_join, hipEventDisableTiming));
    }
    HIP_CHECK(c, orb_launch(c->geom, c->b, n_frames, c->p.ini_th_fast, c->p.min_th_fast, d_kps, d_desc, d_counts,
                            cap_per_frame, s, c->timer, c->orb_aux, c->orb_fork, c->orb_join));
    c->last_gray = d_gray;
    c->last_frame_stride = frame_stride;
    c->last_stride = stride;
    c->last_frames = n_frames;
    return SPSLAM_OK;
}

int spslam_orb_extract(spslam_ctx* c, const uint8_t* gray, int w, int h, int stride, spslam_keypoint* kps,
                       uint8_t* desc, int cap, int* n) {
    if (!c || !n) return SPSLAM_ERR_ARG;
    if (w == 0 || h == 0 || !gray) {  // reference: empty image -> return, outputs untouched
        *n = 0;
        return SPSLAM_OK;
    }
    if (w != c->p.width || h != c->p.height || stride < w)
        return fail(c, SPSLAM_ERR_ARG, "image size does not match the context%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, hipMemcpy2DAsync(c->d_in, w, gray, stride, w, h, hipMemcpyHostToDevice, c->stream));
    int rc = spslam_orb_extract_batch_device(c, c->d_in, 1, (size_t)w * h, w, c->d_kps, c->d_desc, c->d_cnt,
                                             c->max_kp, c->stream);
    if (rc) return rc;
    int cnt = 0;
    HIP_CHECK(c, hipMemcpyAsync(&cnt, c->d_cnt, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    *n = cnt;
    if (cnt > cap) return fail(c, SPSLAM_ERR_CAPACITY, "keypoint buffer too small%s", "");
    if (cnt > 0) {
        if (kps) HIP_CHECK(c, hipMemcpy(kps, c->d_kps, cnt * sizeof(spslam_keypoint), hipMemcpyDeviceToHost));
        if (desc) HIP_CHECK(c, hipMemcpy(desc, c->d_desc, (size_t)cnt * 32, hipMemcpyDeviceToHost));
    }
    return SPSLAM_OK;
}

int spslam_frame_configure(spslam_ctx* c, const spslam_frame_params* p, float* bounds, float* grid_inv) {
    if (!c || !p || p->fx == 0.f || p->fy == 0.f || p->width < 1 || p->height < 1) return SPSLAM_ERR_ARG;
    FrameGeom& g = c->fg;
    g.fx = p->fx; g.fy = p->fy; g.cx = p->cx; g.cy = p->cy;
    for (int k = 0; k < 5; k++) g.dist[k] = p->dist[k];
    g.bf = p->bf;
    g.undistort = p->dist[0] != 0.0f;
    // Frame::ComputeImageBounds (Frame.cc:536-564)
    if (g.undistort) {
        float cu[4], cv[4];
        const float px[4] = {0.f, (float)p->width, 0.f, (float)p->width};
        const float py[4] = {0.f, 0.f, (float)p->height, (float)p->height};
        for (int i = 0; i < 4; i++) undistort_host(g, px[i], py[i], &cu[i], &cv[i]);
        g.min_x = std::min(cu[0], cu[2]); g.max_x = std::max(cu[1], cu[3]);
        g.min_y = std::min(cv[0], cv[1]); g.max_y = std::max(cv[2], cv[3]);
    } else {
        g.min_x = 0.f; g.max_x = (float)p->width; g.min_y = 0.f; g.max_y = (float)p->height;
    }
    g.ginv_x = (float)SPSLAM_GRID_COLS / (g.max_x - g.min_x);
    g.ginv_y = (float)SPSLAM_GRID_ROWS / (g.max_y - g.min_y);
    if (bounds) { bounds[0] = g.min_x; bounds[1] = g.max_x; bounds[2] = g.min_y; bounds[3] = g.max_y; }
    if (grid_inv) { grid_inv[0] = g.ginv_x; grid_inv[1] = g.ginv_y; }
    HIP_CHECK(c, hipSetDevice(c->device));
    if (!c->d_frame1) {
        const size_t cap = (size_t)c->max_kp;
        const size_t bytes = cap * (2 * sizeof(spslam_keypoint) + 3 * 4) + (SPSLAM_GRID_COLS * SPSLAM_GRID_ROWS + 1) * 4 +
                             4096;
        HIP_CHECK(c, c->d_frame1.alloc(bytes));
    }
    c->frame_ready = true;
    return SPSLAM_OK;
}

int spslam_frame_rgbd_batch_device(spslam_ctx* c, const spslam_keypoint* d_kps, const int* d_counts,
                                   int cap_per_frame, const float* d_depth, int n_frames, size_t frame_stride,
                                   int stride_floats, spslam_keypoint* d_keys_un, float* d_mv_depth,
                                   float* d_mv_uright, int32_t* d_grid_off, int32_t* d_grid_idx,
                                   int* d_plane_counts, int* d_supp_counts, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    if (!d_kps || !d_counts || !d_depth || !d_keys_un || !d_mv_depth || !d_mv_uright || !d_grid_off || !d_grid_idx ||
        n_frames < 1 || cap_per_frame < 1 || cap_per_frame > 32767 || stride_floats < 1)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_frame_rgbd_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the default stream (header)
    HIP_CHECK(c, frame_launch(c->fg, n_frames, d_kps, d_counts, cap_per_frame, d_depth, (long long)frame_stride,
                              stride_floats, d_keys_un, d_mv_depth, d_mv_uright, d_grid_off, d_grid_idx,
                              d_plane_counts, d_supp_counts, s, c->timer));
    return SPSLAM_OK;
}

int spslam_frame_rgbd(spslam_ctx* c, const spslam_keypoint* kps, int n, const float* depth, int w, int h,
                      int stride_floats, spslam_keypoint* keys_un, float* mv_depth, float* mv_uright,
                      int32_t* grid_off, int32_t* grid_idx) {
    if (!c || n < 0 || (n && (!kps || !keys_un || !mv_depth || !mv_uright || !grid_idx)) || !grid_off || !depth ||
        w < 1 || h < 1 || stride_floats < w)
        return SPSLAM_ERR_ARG;
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    if (n > c->max_kp) return fail(c, SPSLAM_ERR_CAPACITY, "more keypoints than the context holds%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    const size_t cap = (size_t)std::max(n, 1), K = (size_t)c->max_kp;
    constexpr size_t kGridOff = (SPSLAM_GRID_COLS * SPSLAM_GRID_ROWS + 1) * 4;
    // slots sized for the context's most keypoints: they fit the block of spslam_frame_configure
    Stage st(c);
    if (int rc = st.open({{kps, n * sizeof(spslam_keypoint), K * sizeof(spslam_keypoint)}, K * sizeof(spslam_keypoint),
                          K * 4, K * 4, K * 4, kGridOff, {&n, sizeof(int)}},
                         &c->d_frame1))
        return rc;
    auto *d_k = st.slot<spslam_keypoint>(0), *d_u = st.slot<spslam_keypoint>(1);
    auto *d_d = st.slot<float>(2), *d_r = st.slot<float>(3);
    auto *d_gi = st.slot<int32_t>(4), *d_go = st.slot<int32_t>(5);
    // the depth image is staged in a stream-ordered temporary
    Stage dep(c);
    if (int rc = dep.open({(size_t)w * h * 4})) return rc;
    float* d_depth = dep.slot<float>(0);
    HIP_CHECK(c, hipMemcpy2DAsync(d_depth, (size_t)w * 4, depth, (size_t)stride_floats * 4, (size_t)w * 4, h,
                                  hipMemcpyHostToDevice, c->stream));
    int rc = spslam_frame_rgbd_batch_device(c, d_k, st.slot<int>(6), (int)cap, d_depth, 1, (size_t)w * h, w, d_u, d_d,
                                            d_r, d_go, d_gi, nullptr, nullptr, c->stream);
    if (rc) return rc;
    if (n) {
        HIP_CHECK(c, hipMemcpyAsync(keys_un, d_u, n * sizeof(spslam_keypoint), hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(c, hipMemcpyAsync(mv_depth, d_d, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(c, hipMemcpyAsync(mv_uright, d_r, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_CHECK(c, hipMemcpyAsync(grid_off, d_go, kGridOff, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    const int ng = grid_off[SPSLAM_GRID_COLS * SPSLAM_GRID_ROWS];
    if (ng) HIP_CHECK(c, hipMemcpy(grid_idx, d_gi, (size_t)ng * 4, hipMemcpyDeviceToHost));
    if ((rc = dep.close())) return rc;
    return SPSLAM_OK;
}

int spslam_grab_rgbd_batch_device(spslam_ctx* c, int n_frames, const uint8_t* d_color, size_t color_frame_stride,
                                  int color_stride, const void* d_depth, size_t depth_frame_stride, int depth_stride,
                                  int w, int h, const spslam_grab_params* params, uint8_t* d_gray, float* d_depth_out,
                                  void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_frames < 1 || !d_color || !d_depth || !params || !d_gray || !d_depth_out || w < 1 || h < 1 ||
        (params->channels != 1 && params->channels != 3 && params->channels != 4) ||
        color_stride < w * params->channels || depth_stride < w ||
        (n_frames > 1 && (color_frame_stride < (size_t)color_stride * h || depth_frame_stride < (size_t)depth_stride * h)))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_grab_rgbd_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    GrabArgs a{d_color, color_frame_stride, color_stride, d_depth, depth_frame_stride, depth_stride, w, h, *params,
               d_gray, d_depth_out, nullptr, 0, 1, 0, 0, 0.f, 0.f, 0.f, 0.f};
    // a CV_32F depth with |factor - 1| <= 1e-5 is used as is (Tracking.cc:228)
    if (!params->depth_u16 && std::fabs(params->depth_scale - 1.0f) <= 1e-5f) a.p.depth_scale = 1.0f;
    // the organized cloud of the plane stage in the same pass (spslam_grab_fuse_cloud)
    const bool cloud = c->grab_cloud && c->planes_ready && w == c->pg.w && h == c->pg.h && n_frames <= c->p.max_batch;
    if (cloud) {
        const PlaneGeom& g = c->pg;
        a.cloud = c->pb.cloud; a.cloud_fs = c->pb.cloud_fs;
        a.ds = g.ds; a.cW = g.W; a.cN = g.N;
        a.fx = g.fx; a.fy = g.fy; a.cx = g.cx; a.cy = g.cy;
    }
    HIP_CHECK(c, grab_launch(n_frames, a, (hipStream_t)hip_stream, c->timer));
    if (cloud) c->cloud_tag[c->cloud_set] = {d_depth_out, n_frames};
    return SPSLAM_OK;
}

int spslam_grab_fuse_cloud(spslam_ctx* c, int enable) {
    if (!c) return SPSLAM_ERR_ARG;
    c->grab_cloud = enable != 0;
    if (!enable) c->cloud_tag[0] = c->cloud_tag[1] = {};
    return SPSLAM_OK;
}

int spslam_grab_rgbd(spslam_ctx* c, const uint8_t* color, int color_stride, const void* depth, int depth_stride,
                     int w, int h, const spslam_grab_params* params, uint8_t* gray, float* depth_out) {
    if (!c || !color || !depth || !params || !gray || !depth_out || w < 1 || h < 1 ||
        (params->channels != 1 && params->channels != 3 && params->channels != 4) ||
        color_stride < w * params->channels || depth_stride < w)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_grab_rgbd");
    HIP_CHECK(c, hipSetDevice(c->device));
    const size_t de = params->depth_u16 ? 2 : 4;
    const size_t cb = (size_t)color_stride * h, db = (size_t)depth_stride * h * de, gb = (size_t)w * h;
    Stage st(c);
    if (int rc = st.open({{color, cb}, {depth, db}, gb, gb * 4})) return rc;
    int rc = spslam_grab_rgbd_batch_device(c, 1, st.slot<uint8_t>(0), cb, color_stride, st.slot<void>(1),
                                           (size_t)depth_stride * h, depth_stride, w, h, params, st.slot<uint8_t>(2),
                                           st.slot<float>(3), c->stream);
    if (rc) return rc;
    HIP_CHECK(c, hipMemcpyAsync(gray, st.slot<uint8_t>(2), gb, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(depth_out, st.slot<float>(3), gb * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

int spslam_orb_debug_stage(spslam_ctx* c, int frame, int level, int stage, void* out, int cap, int* n) {
    if (!c || !out || level < 0 || level >= c->p.nlevels) return SPSLAM_ERR_ARG;
    if (!c->last_frames || frame < 0 || frame >= c->last_frames)
        return fail(c, SPSLAM_ERR_NOT_READY, "no such frame in the last call%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    HIP_CHECK(c, hipDeviceSynchronize());
    const LevelGeom& L = c->geom.lv[level];
    if (stage == 0 || stage == 1) {
        const uint8_t* src;
        size_t pitch;
        if (stage == 0) {
            src = (level == 0 ? c->last_gray : L.img) +
                  (size_t)frame * (level == 0 ? c->last_frame_stride : (size_t)L.frame_stride);
            pitch = level == 0 ? c->last_stride : L.stride;
        } else {
            src = L.blur + (size_t)frame * L.blur_frame_stride;
            pitch = L.bpitch;
        }
        HIP_CHECK(c, hipMemcpy2D(out, L.w, src, pitch, L.w, L.h, hipMemcpyDeviceToHost));
        if (n) *n = L.w * L.h;
        return SPSLAM_OK;
    }
    spslam_keypoint* o = (spslam_keypoint*)out;
    if (stage == 2) {
        const int ncells = L.nRows * L.nCols;
        std::vector<uint16_t> cnt(ncells);
        std::vector<uint32_t> cand((size_t)ncells * kCellCap);
        const size_t cell0 = (size_t)frame * c->geom.cells_per_frame + L.cell_base;
        HIP_CHECK(c, hipMemcpy(cnt.data(), c->b.cand_cnt + cell0, ncells * sizeof(uint16_t), hipMemcpyDeviceToHost));
        HIP_CHECK(c, hipMemcpy(cand.data(), c->b.cand + cell0 * kCellCap, cand.size() * 4, hipMemcpyDeviceToHost));
        int k = 0;
        for (int ci = 0; ci < ncells; ci++)
            for (int j = 0; j < cnt[ci]; j++, k++) {
                if (k >= cap) continue;
                const uint32_t v = cand[(size_t)ci * kCellCap + j];
                o[k] = spslam_keypoint{(float)(v & 0xFFF), (float)((v >> 12) & 0xFFF), 7.f, -1.f, (float)(v >> 24), 0, -1};
            }
        *n = k;
        return k > cap ? SPSLAM_ERR_CAPACITY : SPSLAM_OK;
    }
    if (stage == 3) {
        int cnt = 0;
        HIP_CHECK(c, hipMemcpy(&cnt, c->b.lvl_cnt + frame * kMaxLevels + level, sizeof(int), hipMemcpyDeviceToHost));
        std::vector<LevelKp> v(cnt);
        if (cnt)
            HIP_CHECK(c, hipMemcpy(v.data(), c->b.lvl_kp + (size_t)frame * c->geom.lvl_kp_per_frame + L.kp_base,
                                   cnt * sizeof(LevelKp), hipMemcpyDeviceToHost));
        for (int i = 0; i < cnt && i < cap; i++)
            o[i] = spslam_keypoint{(float)v[i].x, (float)v[i].y, (float)L.patch_size, -1.f, (float)v[i].response,
                                   level, -1};
        *n = cnt;
        return cnt > cap ? SPSLAM_ERR_CAPACITY : SPSLAM_OK;
    }
    return fail(c, SPSLAM_ERR_ARG, "unknown stage%s", "");
}

}  // extern "C"
