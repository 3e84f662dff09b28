// C ABI (include/spslam_gpu.h): plane extraction, supposed planes, plane association and the plane debug entries.
#include "capi_ctx.h"

#include <cmath>
#include <cstring>
#include <random>
#include <string>

namespace {

// GeneratePlanesFromBoundries constants and scratch (supposed_kernels.hip).
hipError_t configure_supposed(spslam_ctx* c, const spslam_plane_params* p) {
    const PlaneGeom& g = c->pg;
    SuppParams& sp = c->sp;
    sp.line_ratio = p->line_ratio;
    // (double)s < (double)th * th  <=>  s <= sqr_th_f
    const double T = (double)p->line_distance_threshold * (double)p->line_distance_threshold;
    float f = (float)T;
    while ((double)f >= T && f > 0.f) f = std::nextafter(f, 0.f);
    while ((double)std::nextafter(f, 1.f) < T) f = std::nextafter(f, 1.f);
    sp.sqr_th_f = f;
    const bool nob = p->image_bounds[0] == 0.f && p->image_bounds[1] == 0.f && p->image_bounds[2] == 0.f &&
                     p->image_bounds[3] == 0.f;
    sp.min_x = nob ? 0.f : p->image_bounds[0];
    sp.max_x = nob ? (float)p->width : p->image_bounds[1];
    sp.min_y = nob ? 0.f : p->image_bounds[2];
    sp.max_y = nob ? (float)p->height : p->image_bounds[3];
    sp.supp_cap = kMaxSuppPerFrame;
    sp.line_cap = g.contour_cap;
    // CaculatePlanes' loop: for (float i = -0.25; i < 0.25;) { ...; i = i + 0.01; } (double step)
    int ns = 0;
    for (float v = -0.25f; v < 0.25f; v = (float)((double)v + 0.01)) {
        if (ns >= kMaxPatchSteps) return hipErrorInvalidValue;
        sp.steps[ns++] = v;
    }
    sp.n_steps = ns;
    const size_t F = (size_t)c->p.max_batch, CC = (size_t)g.contour_cap;
    SuppBuffers& b = c->sb;
    const size_t bytes = (size_t)kSuppRndTable * 4 +
                         F * kMaxPlanesPerFrame * kMaxLinesPerBoundary * sizeof(LineCand) +
                         F * kMaxPlanesPerFrame * sizeof(int) + F * CC * (4 + 16 + 4 + 1) +
                         F * kMaxPlanesPerFrame * 8 * sizeof(long long) + 9 * 256;
    hipError_t e = c->d_supp_scratch.alloc(bytes);
    if (e != hipSuccess) return e;
    uint8_t* q = c->d_supp_scratch;
    auto carve = [&](size_t n) { uint8_t* r = q; q += (n + 255) / 256 * 256; return r; };
    b.rnd = (const uint32_t*)carve((size_t)kSuppRndTable * 4);
    b.cand = (LineCand*)carve(F * kMaxPlanesPerFrame * kMaxLinesPerBoundary * sizeof(LineCand));
    b.n_cand = (int*)carve(F * kMaxPlanesPerFrame * sizeof(int));
    b.line_idx = (int32_t*)carve(F * CC * 4);
    b.big = (float4*)carve(F * CC * 16);
    b.big_sh = (int*)carve(F * CC * 4);
    b.big_flag = (uint8_t*)carve(F * CC);
    b.prof = (long long*)carve(F * kMaxPlanesPerFrame * 8 * sizeof(long long));
    e = hipMemset(b.prof, 0, F * kMaxPlanesPerFrame * 8 * sizeof(long long));
    if (e != hipSuccess) return e;
    // every SACSegmentation::segment() seeds boost::mt19937(12345u); rnd() = uniform_int<>(0, INT_MAX) = mt() >> 1
    std::vector<uint32_t> tab(kSuppRndTable);
    std::mt19937 mt(12345u);
    for (auto& v : tab) v = (uint32_t)mt() >> 1;
    e = hipMemcpy((void*)b.rnd, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    const size_t patch = (size_t)sp.n_steps * sp.n_steps;
    if ((e = c->d_supp1.alloc(sp.supp_cap * sizeof(spslam_supposed_plane))) != hipSuccess) return e;
    if ((e = c->d_supp_cnt1.alloc(16)) != hipSuccess) return e;
    if ((e = c->d_line1.alloc(CC * 4)) != hipSuccess) return e;
    return c->d_patch1.alloc(sp.supp_cap * patch * 12);
}

// The limits a frame's status word (PlaneBuffers::ts[14]) names, if it is of extraction call `epoch`.
int plane_status_flags(long long word, int epoch) { return (word >> 8) == epoch ? (int)(word & 0xFF) : 0; }

}  // namespace

extern "C" {

int spslam_planes_configure(spslam_ctx* c, const spslam_plane_params* p) {
    if (!c || !p) return SPSLAM_ERR_ARG;
    if (p->cloud_dis < 1 || p->width < 1 || p->height < 1 || p->fx == 0.f || p->fy == 0.f)
        return fail(c, SPSLAM_ERR_ARG, "bad plane parameters%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    PlaneGeom g = c->pg;  // (a refused geometry leaves the context's configuration as it was)
    g.w = p->width;
    g.h = p->height;
    g.ds = p->cloud_dis;
    g.W = (int)std::ceil(p->width / (float)p->cloud_dis);
    g.H = (int)std::ceil(p->height / (float)p->cloud_dis);
    g.N = g.W * g.H;
    if (g.H > 512) return fail(c, SPSLAM_ERR_ARG, "organized cloud taller than 512 rows%s", "");
    if (g.N > 160000) return fail(c, SPSLAM_ERR_ARG, "organized cloud larger than the LDS state map%s", "");
    if (3 * 10 * g.W * 4 > 65536) return fail(c, SPSLAM_ERR_ARG, "organized cloud wider than the LDS row band%s", "");
    // whatever plane_launch would refuse at extraction time is refused here
    if (plane_launch_shape(g, 1, nullptr) != hipSuccess)
        return fail(c, SPSLAM_ERR_ARG, "no kernel instance takes the organized cloud%s",
                    g.W > 512 ? ": wider than 512 columns" : ": past the segmentation's LDS or index budget");
    g.fx = p->fx; g.fy = p->fy; g.cx = p->cx; g.cy = p->cy;
    g.min_size = p->min_size;
    g.ang_cos = std::cos((float)(0.017453 * p->angle_threshold));  // cosf(static_cast<float>(0.017453*AngTh))
    g.dist_th = p->distance_threshold;
    g.inlier_cap = g.N;
    g.contour_cap = 4 * g.N;
    c->pg = g;
    const long long N = g.N, F = c->p.max_batch, IWH = (long long)(g.W + 1) * (g.H + 1);
    PlaneBuffers& b = c->pb;
    // nothing of the old configuration stays reachable until every buffer of the new one exists
    c->planes_ready = false;
    c->plane_last_frames = c->supp_last_frames = 0;
    c->plane_cloud[0] = c->plane_cloud[1] = nullptr;
    c->sb = SuppBuffers{};
    const int keep_labels = b.keep_labels;  // spslam_debug_plane_labels outlives a re-configure
    b = PlaneBuffers{};
    b.keep_labels = keep_labels;
    const long long SH = wave_size(g.W, g.H);
    b.cloud_fs = 3 * N; b.wave_fs = SH; b.dist_fs = N; b.integral_fs = 6 * (IWH + g.W + 1); b.normal_fs = 3 * N; b.pd_fs = N;
    b.labels_fs = N; b.work_fs = 4 * N; b.grown_fs = N; b.maps_fs = 2 * N;
    const size_t bytes = F * (sizeof(float) * (2 * b.cloud_fs + b.wave_fs + b.dist_fs + b.normal_fs + b.pd_fs) +
                              sizeof(double) * b.integral_fs + sizeof(uint32_t) * b.labels_fs +
                              sizeof(int) * (b.work_fs + b.grown_fs) + b.maps_fs + 16 * sizeof(long long)) + 8192;
    HIP_CHECK(c, c->d_plane_scratch.alloc(bytes));
    uint8_t* q = c->d_plane_scratch;
    auto carve = [&](size_t n) { uint8_t* r = q; q += (n + 255) / 256 * 256; return r; };
    b.integral = (double*)carve(F * b.integral_fs * sizeof(double));
    c->plane_cloud[0] = (float*)carve(F * b.cloud_fs * 4);
    c->plane_cloud[1] = (float*)carve(F * b.cloud_fs * 4);
    b.cloud = c->plane_cloud[0];
    c->cloud_set = 0;
    c->cloud_tag[0] = c->cloud_tag[1] = {};
    b.wave = (float*)carve(F * b.wave_fs * 4);
    b.dist = (float*)carve(F * b.dist_fs * 4);
    b.normal = (float*)carve(F * b.normal_fs * 4);
    b.pd = (float*)carve(F * b.pd_fs * 4);
    b.labels = (uint32_t*)carve(F * b.labels_fs * 4);
    b.work = (int*)carve(F * b.work_fs * 4);
    b.grown = (int*)carve(F * b.grown_fs * 4);
    b.maps = (uint8_t*)carve(F * b.maps_fs);
    b.ts = (long long*)carve(F * 16 * sizeof(long long));
    HIP_CHECK(c, hipMemset(b.ts, 0, F * 16 * sizeof(long long)));  // no frame has crossed a limit (ts[14])
    HIP_CHECK(c, c->d_depth_in.alloc((size_t)g.w * g.h * sizeof(float)));
    HIP_CHECK(c, c->d_planes1.alloc(kMaxPlanesPerFrame * sizeof(spslam_plane)));
    HIP_CHECK(c, c->d_plane_cnt1.alloc(16));
    HIP_CHECK(c, c->d_inl1.alloc((size_t)g.inlier_cap * 4));
    HIP_CHECK(c, c->d_con1.alloc((size_t)g.contour_cap * 4));
    HIP_CHECK(c, configure_supposed(c, p));
    c->planes_ready = true;
    return SPSLAM_OK;
}

int spslam_planes_capacity(const spslam_ctx* c, int* planes_cap, int* inlier_cap, int* contour_cap) {
    if (!c || !c->planes_ready) return SPSLAM_ERR_NOT_READY;
    if (planes_cap) *planes_cap = kMaxPlanesPerFrame;
    if (inlier_cap) *inlier_cap = c->pg.inlier_cap;
    if (contour_cap) *contour_cap = c->pg.contour_cap;
    return SPSLAM_OK;
}

int spslam_planes_extract_batch_device(spslam_ctx* c, const float* d_depth, int n_frames, size_t frame_stride,
                                       int stride_floats, spslam_plane* d_planes, int* d_counts,
                                       int32_t* d_inliers, int32_t* d_contours, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->planes_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_planes_configure not called%s", "");
    if (!d_depth || !d_planes || !d_counts || !d_inliers || !d_contours || n_frames < 1 ||
        n_frames > c->p.max_batch || stride_floats < c->pg.w)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_planes_extract_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the default stream (header)
    // a fused grab already wrote this depth's cloud into the selected set (spslam_grab_fuse_cloud)
    auto& tag = c->cloud_tag[c->cloud_set];
    const bool have_cloud = tag.depth == d_depth && n_frames <= tag.n &&
                            frame_stride == (size_t)c->pg.w * c->pg.h && stride_floats == c->pg.w;
    tag = {};
    c->pb.epoch++;
    HIP_CHECK(c, plane_launch(c->pg, c->pb, n_frames, d_depth, (long long)frame_stride, stride_floats, d_planes,
                              d_counts, kMaxPlanesPerFrame, d_inliers, d_contours, s, c->timer, have_cloud));
    c->plane_last_frames = n_frames;
    return SPSLAM_OK;
}

int spslam_planes_extract(spslam_ctx* c, const float* depth, int w, int h, int stride_floats, spslam_plane* planes,
                          int planes_cap, int* n_planes, int32_t* inliers, int32_t* contours) {
    if (!c || !n_planes) return SPSLAM_ERR_ARG;
    if (!c->planes_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_planes_configure not called%s", "");
    if (!depth || w != c->pg.w || h != c->pg.h || stride_floats < w)
        return fail(c, SPSLAM_ERR_ARG, "depth size does not match the plane configuration%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, hipMemcpy2DAsync(c->d_depth_in, (size_t)w * 4, depth, (size_t)stride_floats * 4, (size_t)w * 4, h,
                                  hipMemcpyHostToDevice, c->stream));
    int rc = spslam_planes_extract_batch_device(c, c->d_depth_in, 1, (size_t)w * h, w, c->d_planes1, c->d_plane_cnt1,
                                                c->d_inl1, c->d_con1, c->stream);
    if (rc) return rc;
    int n = 0;
    long long word = 0;
    spslam_plane tmp[kMaxPlanesPerFrame];
    HIP_CHECK(c, hipMemcpyAsync(&n, c->d_plane_cnt1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(&word, c->pb.ts + 14, sizeof word, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(tmp, c->d_planes1, sizeof tmp, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    *n_planes = n;
    if (n > planes_cap) return fail(c, SPSLAM_ERR_CAPACITY, "plane buffer too small%s", "");
    const int over = plane_status_flags(word, c->pb.epoch);
    int ni = 0, nc = 0;
    for (int k = 0; k < n; k++) {
        planes[k] = tmp[k];
        ni = std::max(ni, tmp[k].inlier_offset + tmp[k].n_inliers);
        nc = std::max(nc, tmp[k].contour_offset + tmp[k].n_contour);
    }
    if (inliers && ni) HIP_CHECK(c, hipMemcpy(inliers, c->d_inl1, (size_t)ni * 4, hipMemcpyDeviceToHost));
    if (contours && nc) HIP_CHECK(c, hipMemcpy(contours, c->d_con1, (size_t)nc * 4, hipMemcpyDeviceToHost));
    if (over) {
        std::string what;
        if (over & SPSLAM_PLANES_OVER_COMPONENTS) what += " more than 255 components over Plane.MinSize;";
        if (over & SPSLAM_PLANES_OVER_MODELS) what += " more than 64 plane models;";
        if (over & SPSLAM_PLANES_OVER_KEPT) what += " more than 64 kept planes;";
        return fail(c, SPSLAM_ERR_CAPACITY, "plane extraction limit crossed:%s", what.c_str());
    }
    return SPSLAM_OK;
}

int spslam_planes_status(spslam_ctx* c, int frame, int* flags) {
    if (!c || !flags) return SPSLAM_ERR_ARG;
    if (!c->planes_ready || frame < 0 || frame >= c->plane_last_frames)
        return fail(c, SPSLAM_ERR_NOT_READY, "no plane data for that frame%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    long long word = 0;
    HIP_CHECK(c, hipMemcpy(&word, c->pb.ts + (size_t)frame * 16 + 14, sizeof word, hipMemcpyDeviceToHost));
    *flags = plane_status_flags(word, c->pb.epoch);
    return SPSLAM_OK;
}

int spslam_debug_plane_launch_shape(spslam_ctx* c, int n_frames, spslam_plane_launch_shape* shape) {
    if (!c || !shape || n_frames < 1) return SPSLAM_ERR_ARG;
    if (!c->planes_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_planes_configure not called%s", "");
    if (plane_launch_shape(c->pg, n_frames, shape) != hipSuccess)
        return fail(c, SPSLAM_ERR_ARG, "no kernel instance takes the configured cloud%s", "");
    return SPSLAM_OK;
}

int spslam_supposed_capacity(const spslam_ctx* c, int* supp_cap, int* line_cap, int* patch_points) {
    if (!c || !c->planes_ready) return SPSLAM_ERR_NOT_READY;
    if (supp_cap) *supp_cap = c->sp.supp_cap;
    if (line_cap) *line_cap = c->sp.line_cap;
    if (patch_points) *patch_points = c->sp.n_steps * c->sp.n_steps;
    return SPSLAM_OK;
}

int spslam_planes_select_cloud_set(spslam_ctx* c, int set) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->planes_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_planes_configure not called%s", "");
    if (set < 0 || set > 1) return fail(c, SPSLAM_ERR_ARG, "cloud set not 0 or 1%s", "");
    c->pb.cloud = c->plane_cloud[set];
    c->cloud_set = set;
    return SPSLAM_OK;
}

int spslam_planes_generate_from_boundaries_batch_device(spslam_ctx* c, const float* d_depth, int n_frames,
                                                        size_t frame_stride, int stride_floats,
                                                        const spslam_plane* d_planes, const int* d_counts,
                                                        const int32_t* d_contours, spslam_supposed_plane* d_out,
                                                        int* d_out_counts, int32_t* d_line_idx, float* d_patch,
                                                        void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->planes_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_planes_configure not called%s", "");
    if (!d_depth || !d_planes || !d_counts || !d_contours || !d_out || !d_out_counts || !d_line_idx || !d_patch ||
        n_frames < 1 || stride_floats < c->pg.w)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_planes_generate_from_boundaries_batch_device");
    if (n_frames > c->plane_last_frames)
        return fail(c, SPSLAM_ERR_NOT_READY, "%s", "more frames than the last plane extraction holds");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the default stream (header)
    HIP_CHECK(c, supp_launch(c->pg, c->pb, c->sp, c->sb, n_frames, d_depth, (long long)frame_stride, stride_floats,
                             d_planes, d_counts, d_contours, d_out, d_out_counts, d_line_idx, d_patch, s, c->timer));
    c->supp_last_frames = n_frames;
    return SPSLAM_OK;
}

int spslam_planes_generate_from_boundaries(spslam_ctx* c, const float* depth, int w, int h, int stride_floats,
                                           spslam_supposed_plane* out, int cap, int* n, int32_t* line_idx,
                                           float* patch_xyz) {
    if (!c || !n) return SPSLAM_ERR_ARG;
    if (!c->planes_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_planes_configure not called%s", "");
    if (!depth || w != c->pg.w || h != c->pg.h || stride_floats < w)
        return fail(c, SPSLAM_ERR_ARG, "depth size does not match the plane configuration%s", "");
    if (c->plane_last_frames < 1) return fail(c, SPSLAM_ERR_NOT_READY, "%s", "spslam_planes_extract not called");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, hipMemcpy2DAsync(c->d_depth_in, (size_t)w * 4, depth, (size_t)stride_floats * 4, (size_t)w * 4, h,
                                  hipMemcpyHostToDevice, c->stream));
    int rc = spslam_planes_generate_from_boundaries_batch_device(c, c->d_depth_in, 1, (size_t)w * h, w, c->d_planes1,
                                                                 c->d_plane_cnt1, c->d_con1, c->d_supp1,
                                                                 c->d_supp_cnt1, c->d_line1, c->d_patch1, c->stream);
    if (rc) return rc;
    int m = 0;
    std::vector<spslam_supposed_plane> tmp(c->sp.supp_cap);
    HIP_CHECK(c, hipMemcpyAsync(&m, c->d_supp_cnt1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(tmp.data(), c->d_supp1, tmp.size() * sizeof(spslam_supposed_plane),
                                hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    *n = m;
    const int stored = std::min(m, c->sp.supp_cap);
    if (m > cap || m > c->sp.supp_cap) return fail(c, SPSLAM_ERR_CAPACITY, "supposed-plane buffer too small%s", "");
    int nl = 0;
    for (int k = 0; k < stored; k++) {
        out[k] = tmp[k];
        nl = std::max(nl, tmp[k].line_offset + tmp[k].n_line);
    }
    const size_t patch = (size_t)c->sp.n_steps * c->sp.n_steps;
    if (line_idx && nl) HIP_CHECK(c, hipMemcpy(line_idx, c->d_line1, (size_t)nl * 4, hipMemcpyDeviceToHost));
    if (patch_xyz && stored)
        HIP_CHECK(c, hipMemcpy(patch_xyz, c->d_patch1, stored * patch * 12, hipMemcpyDeviceToHost));
    return SPSLAM_OK;
}

int spslam_planes_associate_batch_device(spslam_ctx* c, int n_frames, const spslam_assoc_frame* d_frames,
                                         const void* d_planes_a, int stride_a, const int* d_count_a, int cap_a,
                                         const void* d_planes_b, int stride_b, const int* d_count_b, int cap_b,
                                         const spslam_map_plane* d_map, const float* d_boundary_xyz, int max_map,
                                         const spslam_assoc_params* params, int32_t* d_match, int32_t* d_parallel,
                                         int32_t* d_vertical, int* d_new_plane, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_frames < 1 || !d_frames || !params || !d_match || !d_parallel || !d_vertical || max_map < 0 ||
        (cap_a > 0 && (!d_planes_a || !d_count_a || stride_a < 16)) || cap_a < 0 || cap_b < 0 ||
        (cap_b > 0 && (!d_planes_b || !d_count_b || stride_b < 16)) || (max_map > 0 && (!d_map || !d_boundary_xyz)))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_planes_associate_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the default stream (header)
    const size_t need = std::max<size_t>((size_t)n_frames * (cap_a + cap_b) * max_map * sizeof(float), 256);
    HIP_CHECK(c, c->d_assoc_dist.reserve(need, s));
    AssocSources S{(const uint8_t*)d_planes_a, cap_b > 0 ? (const uint8_t*)d_planes_b : nullptr, stride_a,
                   stride_b, d_count_a, cap_b > 0 ? d_count_b : nullptr, cap_a, cap_b};
    HIP_CHECK(c, assoc_launch(n_frames, d_frames, S, d_map, d_boundary_xyz, max_map, *params, c->d_assoc_dist,
                              d_match, d_parallel, d_vertical, d_new_plane, s, c->timer));
    return SPSLAM_OK;
}

int spslam_planes_associate(spslam_ctx* c, const spslam_assoc_frame* frame, const float* coefs, int n_planes,
                            const spslam_map_plane* map_planes, int n_map, const float* boundary_xyz,
                            int n_boundary, const spslam_assoc_params* params, int32_t* match, int32_t* parallel,
                            int32_t* vertical, int* new_plane) {
    if (!c || !frame || !params || n_planes < 0 || n_map < 0 || n_boundary < 0 ||
        (n_planes && (!coefs || !match || !parallel || !vertical)) || (n_map && !map_planes) ||
        (n_boundary && !boundary_xyz))
        return SPSLAM_ERR_ARG;
    for (int j = 0; j < n_map; j++)
        if (map_planes[j].n_boundary < 0 || map_planes[j].boundary_offset < 0 ||
            (long long)map_planes[j].boundary_offset + map_planes[j].n_boundary > n_boundary)
            return fail(c, SPSLAM_ERR_ARG, "map plane boundary range outside the boundary array%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    spslam_assoc_frame F = *frame;
    F.map_offset = 0;
    F.n_map = n_map;
    const int cap = std::max(n_planes, 1);
    Stage st(c);
    if (int rc = st.open({{&F, sizeof F}, {coefs, (size_t)n_planes * 16, (size_t)cap * 16}, {&n_planes, sizeof(int)},
                           {map_planes, n_map * sizeof(spslam_map_plane), std::max(n_map, 1) * sizeof(spslam_map_plane)},
                           {boundary_xyz, (size_t)n_boundary * 12, (size_t)std::max(n_boundary, 1) * 12},
                           (size_t)cap * 4 * 3, sizeof(int)}))
        return rc;
    auto* d_out = st.slot<int32_t>(5);
    if (F.carry && n_planes) {  // the frame's current associations are the starting state
        HIP_CHECK(c, hipMemcpyAsync(d_out, match, (size_t)n_planes * 4, hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(c, hipMemcpyAsync(d_out + cap, parallel, (size_t)n_planes * 4, hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(c, hipMemcpyAsync(d_out + 2 * cap, vertical, (size_t)n_planes * 4, hipMemcpyHostToDevice, c->stream));
    }
    int rc = spslam_planes_associate_batch_device(
        c, 1, st.slot<spslam_assoc_frame>(0), st.slot<void>(1), 16, st.slot<int>(2), cap, nullptr, 0, nullptr, 0,
        st.slot<spslam_map_plane>(3), st.slot<float>(4), n_map, params, d_out, d_out + cap, d_out + 2 * cap,
        st.slot<int>(6), c->stream);
    if (rc) return rc;
    int np = 0;
    if (n_planes) {
        HIP_CHECK(c, hipMemcpyAsync(match, d_out, (size_t)n_planes * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(c, hipMemcpyAsync(parallel, d_out + cap, (size_t)n_planes * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(c, hipMemcpyAsync(vertical, d_out + 2 * cap, (size_t)n_planes * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_CHECK(c, hipMemcpyAsync(&np, st.slot<int>(6), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    if (new_plane) *new_plane = np;
    return SPSLAM_OK;
}

int spslam_debug_plane_not_seen(spslam_ctx* c, const float* planes, int n_planes, const float* coefs, int n_coefs,
                                int* not_seen) {
    if (!c || n_planes < 0 || n_coefs < 0 || (n_planes && !planes) || (n_coefs && (!coefs || !not_seen)))
        return SPSLAM_ERR_ARG;
    if (!n_coefs) return SPSLAM_OK;
    HIP_CHECK(c, hipSetDevice(c->device));
    const size_t cb = (size_t)n_coefs * 16;
    Stage st(c);
    if (int rc = st.open({{planes, (size_t)n_planes * 16, (size_t)std::max(n_planes, 1) * 16}, {coefs, cb},
                          (size_t)n_coefs * 4}))
        return rc;
    HIP_CHECK(c, plane_not_seen_debug_launch(st.slot<float>(0), n_planes, st.slot<float>(1), n_coefs,
                                             st.slot<int>(2), c->stream));
    HIP_CHECK(c, hipMemcpyAsync(not_seen, st.slot<int>(2), (size_t)n_coefs * 4, hipMemcpyDeviceToHost, c->stream));
    if (int rc = st.close()) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

int spslam_debug_plane_labels(spslam_ctx* c, int keep) {
    if (!c) return SPSLAM_ERR_ARG;
    c->pb.keep_labels = keep ? 1 : 0;
    return SPSLAM_OK;
}

int spslam_supposed_debug(spslam_ctx* c, int frame, int plane, spslam_line_candidate* cand, int* n_cand,
                          int32_t* idx, int idx_cap) {
    static_assert(sizeof(spslam_line_candidate) == sizeof(LineCand), "candidate layout");
    if (!c || !cand || !n_cand) return SPSLAM_ERR_ARG;
    if (frame < 0 || frame >= c->supp_last_frames || plane < 0 || plane >= kMaxPlanesPerFrame)
        return fail(c, SPSLAM_ERR_NOT_READY, "no supposed-plane data for that frame%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, hipDeviceSynchronize());
    int nc = 0;
    HIP_CHECK(c, hipMemcpy(&nc, c->sb.n_cand + frame * kMaxPlanesPerFrame + plane, sizeof(int), hipMemcpyDeviceToHost));
    nc = std::min(std::max(nc, 0), kMaxLinesPerBoundary);
    LineCand lc[kMaxLinesPerBoundary];
    if (nc)
        HIP_CHECK(c, hipMemcpy(lc, c->sb.cand + ((size_t)frame * kMaxPlanesPerFrame + plane) * kMaxLinesPerBoundary,
                               nc * sizeof(LineCand), hipMemcpyDeviceToHost));
    *n_cand = nc;
    int lo = 0;
    for (int k = 0; k < nc; k++) {
        std::memcpy(&cand[k], &lc[k], sizeof(LineCand));
        if (lc[k].flags & 1) {
            const int m = lc[k].n_inliers;
            if (idx && lo + m <= idx_cap && m)
                HIP_CHECK(c, hipMemcpy(idx + lo, c->sb.line_idx + (size_t)frame * c->pg.contour_cap + lc[k].idx_off,
                                       (size_t)m * 4, hipMemcpyDeviceToHost));
            cand[k].idx_offset = lo;
            lo += m;
        } else {
            cand[k].idx_offset = -1;
        }
    }
    return lo > idx_cap ? SPSLAM_ERR_CAPACITY : SPSLAM_OK;
}

int spslam_planes_debug(spslam_ctx* c, int frame, int what, void* out, int* n_points) {
    if (!c || !out) return SPSLAM_ERR_ARG;
    if (!c->planes_ready || frame < 0 || frame >= c->plane_last_frames)
        return fail(c, SPSLAM_ERR_NOT_READY, "no plane data for that frame%s", "");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, hipDeviceSynchronize());
    const PlaneBuffers& b = c->pb;
    const long long N = c->pg.N;
    if (n_points) *n_points = (int)N;
    if (what == 0 || what == 1) {  // SoA on device -> AoS x,y,z
        const float* src = what == 0 ? b.cloud + frame * b.cloud_fs : b.normal + frame * b.normal_fs;
        std::vector<float> soa(3 * N);
        HIP_CHECK(c, hipMemcpy(soa.data(), src, 3 * N * 4, hipMemcpyDeviceToHost));
        float* o = (float*)out;
        for (long long i = 0; i < N; i++) { o[3 * i] = soa[i]; o[3 * i + 1] = soa[N + i]; o[3 * i + 2] = soa[2 * N + i]; }
        return SPSLAM_OK;
    }
    if (what == 2) {
        HIP_CHECK(c, hipMemcpy(out, b.dist + frame * b.dist_fs, N * 4, hipMemcpyDeviceToHost));
        return SPSLAM_OK;
    }
    if (what == 3) {
        bool in_lds = false;
        plane_segment_lds_bytes(c->pg, &in_lds);
        if (in_lds && !b.keep_labels)
            return fail(c, SPSLAM_ERR_NOT_READY, "labels are kept only after spslam_debug_plane_labels(ctx, 1)%s", "");
        HIP_CHECK(c, hipMemcpy(out, b.labels + frame * b.labels_fs, N * 4, hipMemcpyDeviceToHost));
        return SPSLAM_OK;
    }
    if (what == 4) {
        HIP_CHECK(c, hipMemcpy(out, b.ts + frame * 16, 16 * sizeof(long long), hipMemcpyDeviceToHost));
        return SPSLAM_OK;
    }
    if (what == 5) {  // supp_lines phase clocks (SPSLAM_SUPP_PROF build), [kMaxPlanesPerFrame][8]
        HIP_CHECK(c, hipMemcpy(out, c->sb.prof + (size_t)frame * kMaxPlanesPerFrame * 8,
                               kMaxPlanesPerFrame * 8 * sizeof(long long), hipMemcpyDeviceToHost));
        return SPSLAM_OK;
    }
    return fail(c, SPSLAM_ERR_ARG, "unknown debug stage%s", "");
}

}  // extern "C"
