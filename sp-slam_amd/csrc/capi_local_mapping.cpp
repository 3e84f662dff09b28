// C ABI (include/spslam_gpu.h), LocalMapping's ORBmatcher side: spslam_fuse_search[_batch_device] (SearchInNeighbors'
// Fuse), spslam_map_points_refresh[_batch_device] (ComputeDistinctiveDescriptors, UpdateNormalAndDepth) and
// CreateNewMapPoints: spslam_search_for_triangulation[_batch_device], spslam_triangulate[_batch_device],
// spslam_create_new_points_batch_device, with TriStage, the staging of their host forms; and the covisibility side:
// spslam_covis_update_connections[_batch_device] (KeyFrame::UpdateConnections), spslam_keyframe_culling[_batch_device]
// and spslam_map_point_culling[_batch_device], whose host forms check their indices with covis_check.h.
#include "capi_ctx.h"
#include "covis_check.h"

#include <cmath>
#include <cstring>

namespace {

// Frame.cc:118-124 (invfx = 1.0f/fx, mb = mbf/fx), LocalMapping.cc:245 (ratioFactor = 1.5f*mfScaleFactor)
TriConsts tri_consts(const spslam_ctx* c) {
    TriConsts C{};
    C.fx = c->fg.fx; C.fy = c->fg.fy; C.cx = c->fg.cx; C.cy = c->fg.cy; C.bf = c->fg.bf;
    C.invfx = 1.0f / C.fx;
    C.invfy = 1.0f / C.fy;
    C.mb = C.bf / C.fx;
    C.ratio_factor = 1.5f * (float)c->p.scale_factor;
    level_table(c, c->scale, C.scale);
    level_table(c, c->sigma2, C.sigma2);
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

int spslam_fuse_search_batch_device(spslam_ctx* c, int n_problems, const spslam_fuse_problem* d_problems,
                                    const spslam_local_point* d_points, int max_points,
                                    const spslam_keypoint* d_keys_un, const uint8_t* d_desc, const float* d_uright,
                                    const int32_t* d_grid_off, const int32_t* d_grid_idx, const int* d_counts,
                                    int cap, const uint8_t* d_skip, const spslam_fuse_params* params,
                                    spslam_fuse_result* d_results, int* d_nfused, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!c->frame_ready) return fail(c, SPSLAM_ERR_NOT_READY, "spslam_frame_configure not called%s", "");
    const MatchCurrent cur{d_keys_un, d_desc, d_uright, d_grid_off, d_grid_idx, d_counts, cap};
    if (n_problems < 1 || !d_problems || max_points < 0 || (max_points > 0 && (!d_points || !d_results)) ||
        !match_current_ok(cur) || !params || !d_nfused)
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
    level_table(c, c->inv_sigma2, P.inv_sigma2);
    HIP_CHECK(c, fuse_search_launch(n_problems, d_problems, d_points, max_points, cur, g, P, d_skip, d_results,
                                    d_nfused, (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_fuse_search(spslam_ctx* c, const float* Tcw, const spslam_local_point* points, int n_points,
                       const spslam_keypoint* keys_un, const uint8_t* desc, const float* uright, int n_kp,
                       const int32_t* grid_off, const int32_t* grid_idx, const uint8_t* skip,
                       const spslam_fuse_params* params, spslam_fuse_result* results, int* nfused) {
    const CurrentFrame cf{keys_un, desc, uright, n_kp, grid_off, grid_idx};
    if (!c || !Tcw || !params || !nfused || !cf.args_ok() || n_points < 0 || (n_points && (!points || !results)))
        return SPSLAM_ERR_ARG;
    if (int rc = cf.check_grid(c)) return rc;
    HIP_CHECK(c, hipSetDevice(c->device));
    spslam_fuse_problem F{};
    std::memcpy(F.Tcw, Tcw, sizeof F.Tcw);
    F.n_points = n_points;
    const int np = n_points;
    const size_t N = (size_t)std::max(np, 1);
    enum { kProblem = CurrentFrame::kFirst, kPoints, kSkip, kResults, kNFused };
    Stage st(c);
    if (int rc = cf.open(st, {{&F, sizeof F}, {points, np * sizeof(spslam_local_point), N * sizeof(spslam_local_point)},
                              {skip, skip ? (size_t)np : 0, N}, N * sizeof(spslam_fuse_result), sizeof(int)}))
        return rc;
    const MatchCurrent d = cf.current(st);
    int rc = spslam_fuse_search_batch_device(
        c, 1, st.slot<spslam_fuse_problem>(kProblem), st.slot<spslam_local_point>(kPoints), np, d.kun, d.desc, d.uright,
        d.grid_off, d.grid_idx, d.counts, d.cap, skip ? st.slot<uint8_t>(kSkip) : nullptr, params,
        st.slot<spslam_fuse_result>(kResults), st.slot<int>(kNFused), c->stream);
    if (rc) return rc;
    if (np)
        HIP_CHECK(c, hipMemcpyAsync(results, st.slot<void>(kResults), (size_t)np * sizeof(spslam_fuse_result),
                                    hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipMemcpyAsync(nfused, st.slot<int>(kNFused), sizeof(int), hipMemcpyDeviceToHost, c->stream));
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
    level_table(c, c->scale, P.scale);
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

// ---------------------------------------------------------------- CreateNewMapPoints
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

// ---------------------------------------------------------------- covisibility graph, the cullings
int spslam_covis_update_connections_batch_device(spslam_ctx* c, int n_problems, const spslam_covis_problem* d_problems,
                                                 const spslam_covis_map* map, const spslam_covis_graph* graph, int th,
                                                 spslam_covis_result* d_results, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_problems < 1 || !d_problems || !map || !graph || th < 1 || !d_results || !map->match_off ||
        !map->match_row || !map->obs_off || !map->obs_kf)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_covis_update_connections_batch_device");
    if (const char* e = covis_check_graph(*graph, 1))
        return fail(c, SPSLAM_ERR_ARG, "spslam_covis_update_connections_batch_device: %s", e);
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, covis_update_connections_launch(n_problems, d_problems, *map, *graph, th, d_results,
                                                 (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_covis_update_connections(spslam_ctx* c, const spslam_covis_map* map, int n_kf, int n_rows, int kf, int th,
                                    const spslam_covis_graph* graph, spslam_covis_result* result) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!map || !graph || !result || th < 1)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_covis_update_connections");
    const char* e = covis_check_map(*map, n_kf, n_rows, false, 0, 0);
    if (!e) e = covis_check_graph(*graph, n_kf);
    if (!e && (kf < 0 || kf >= n_kf)) e = "kf outside the keyframes";
    if (e) return fail(c, SPSLAM_ERR_ARG, "spslam_covis_update_connections: %s", e);
    HIP_CHECK(c, hipSetDevice(c->device));
    const spslam_covis_map& m = *map;
    const spslam_covis_graph& g = *graph;
    const size_t K = (size_t)n_kf, R = (size_t)n_rows, NM = (size_t)m.match_off[n_kf], NO = (size_t)m.obs_off[n_rows],
                 W = K * (size_t)g.stride * 4;
    const auto one = [](size_t x) { return std::max(x, (size_t)1); };
    const spslam_covis_problem P{0, 0, kf, n_kf};
    enum { kMatchOff, kMatchRow, kObsOff, kObsKf, kBad, kWeights, kOrdered, kOrderedW, kNOrdered, kCovis, kParent,
           kFirst, kProblem, kResult };
    Stage st(c);
    if (int rc = st.open({{m.match_off, (K + 1) * 4}, {m.match_row, NM * 4, one(NM) * 4}, {m.obs_off, (R + 1) * 4},
                           {m.obs_kf, NO * 4, one(NO) * 4}, {m.point_bad, m.point_bad ? R : 0, one(R)},
                           {g.weights, W}, {g.ordered, W}, {g.ordered_w, W}, {g.n_ordered, K * 4},
                           {g.covis, K * SPSLAM_COVIS_BEST * 4}, {g.parent, K * 4}, {g.first_connection, K},
                           {&P, sizeof P}, sizeof(spslam_covis_result)}))
        return rc;
    spslam_covis_map dm{};
    dm.match_off = st.slot<int32_t>(kMatchOff);
    dm.match_row = st.slot<int32_t>(kMatchRow);
    dm.obs_off = st.slot<int32_t>(kObsOff);
    dm.obs_kf = st.slot<int32_t>(kObsKf);
    dm.point_bad = m.point_bad ? st.slot<uint8_t>(kBad) : nullptr;
    spslam_covis_graph dg{};
    dg.weights = st.slot<int32_t>(kWeights);
    dg.ordered = st.slot<int32_t>(kOrdered);
    dg.ordered_w = st.slot<int32_t>(kOrderedW);
    dg.n_ordered = st.slot<int32_t>(kNOrdered);
    dg.covis = st.slot<int32_t>(kCovis);
    dg.parent = st.slot<int32_t>(kParent);
    dg.first_connection = st.slot<uint8_t>(kFirst);
    dg.stride = g.stride;
    int rc = spslam_covis_update_connections_batch_device(c, 1, st.slot<spslam_covis_problem>(kProblem), &dm, &dg, th,
                                                          st.slot<spslam_covis_result>(kResult), c->stream);
    if (rc) return rc;
    void* const host[] = {g.weights, g.ordered, g.ordered_w, g.n_ordered, g.covis, g.parent, g.first_connection,
                          result};
    const int slot[] = {kWeights, kOrdered, kOrderedW, kNOrdered, kCovis, kParent, kFirst, kResult};
    const size_t bytes[] = {W, W, W, K * 4, K * SPSLAM_COVIS_BEST * 4, K * 4, K, sizeof(spslam_covis_result)};
    for (int a = 0; a < 8; a++)
        HIP_CHECK(c, hipMemcpyAsync(host[a], st.slot<void>(slot[a]), bytes[a], hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

int spslam_keyframe_culling_batch_device(spslam_ctx* c, int n_problems, const spslam_cull_problem* d_problems,
                                         const spslam_covis_map* map, const spslam_covis_graph* graph,
                                         const spslam_keypoint* d_keys_un, const float* d_uright, const float* d_depth,
                                         int cap, const uint8_t* d_new_plane, const uint8_t* d_not_erase,
                                         const spslam_cull_params* params, spslam_cull_record* d_records,
                                         spslam_cull_summary* d_summaries, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_problems < 1 || !d_problems || !map || !graph || !d_keys_un || !d_uright || !d_depth || cap < 1 ||
        cap > (1 << 20) || !d_new_plane || !params || params->th_obs < 1 || !d_records || !d_summaries ||
        !map->match_off || !map->match_row || !map->obs_off || !map->obs_kf || !map->obs_kp || !map->kf_slot ||
        !map->points || !graph->ordered || !graph->n_ordered || graph->stride < 1)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_keyframe_culling_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, keyframe_culling_launch(n_problems, d_problems, *map, *graph, CullFrames{d_keys_un, d_uright, d_depth, cap},
                                         d_new_plane, d_not_erase, *params, d_records, d_summaries,
                                         (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_keyframe_culling(spslam_ctx* c, const spslam_covis_map* map, int n_kf, int n_rows, int kf,
                            const int32_t* ordered, int n_ordered, const spslam_keypoint* keys_un, const float* uright,
                            const float* depth, int cap, int n_slots, const uint8_t* new_plane,
                            const uint8_t* not_erase, const spslam_cull_params* params, spslam_cull_record* records,
                            spslam_cull_summary* summary) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!map || !new_plane || !params || !summary || (n_ordered > 0 && !records) ||
        ((size_t)std::max(n_slots, 0) * std::max(cap, 0) && (!keys_un || !uright || !depth)))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_keyframe_culling");
    const char* e = covis_check_map(*map, n_kf, n_rows, true, cap, n_slots);
    if (!e) e = covis_check_candidates(ordered, n_ordered, n_kf);
    if (!e && (kf < 0 || kf >= n_kf)) e = "kf outside the keyframes";
    if (e) return fail(c, SPSLAM_ERR_ARG, "spslam_keyframe_culling: %s", e);
    HIP_CHECK(c, hipSetDevice(c->device));
    const spslam_covis_map& m = *map;
    const size_t K = (size_t)n_kf, R = (size_t)n_rows, NM = (size_t)m.match_off[n_kf], NO = (size_t)m.obs_off[n_rows],
                 S = (size_t)n_slots * cap, NC = (size_t)n_ordered, Pt = sizeof(spslam_local_point),
                 Kp = sizeof(spslam_keypoint);
    const auto one = [](size_t x) { return std::max(x, (size_t)1); };
    // the graph as the kernel reads it: keyframe kf's list in row kf of a table of stride max(n_ordered, 1)
    const size_t stride = one(NC);
    std::vector<int32_t> ord((size_t)(kf + 1) * stride, -1), n_ord(K, 0);
    std::copy(ordered, ordered + NC, ord.begin() + (size_t)kf * stride);
    n_ord[kf] = n_ordered;
    const spslam_cull_problem P{0, 0, kf, n_kf, 0, {0, 0, 0}};
    enum { kMatchOff, kMatchRow, kObsOff, kObsKf, kObsKp, kSlot, kBad, kPoints, kOrdered, kNOrdered, kKeys, kURight,
           kDepth, kNewPlane, kNotErase, kProblem, kRecords, kSummary };
    Stage st(c);
    if (int rc = st.open({{m.match_off, (K + 1) * 4}, {m.match_row, NM * 4, one(NM) * 4}, {m.obs_off, (R + 1) * 4},
                           {m.obs_kf, NO * 4, one(NO) * 4}, {m.obs_kp, NO * 4, one(NO) * 4}, {m.kf_slot, K * 4},
                           {m.point_bad, m.point_bad ? R : 0, one(R)}, {m.points, R * Pt, one(R) * Pt},
                           {ord.data(), ord.size() * 4}, {n_ord.data(), K * 4}, {keys_un, S * Kp, one(S) * Kp},
                           {uright, S * 4, one(S) * 4}, {depth, S * 4, one(S) * 4}, {new_plane, K},
                           {not_erase, not_erase ? K : 0, K}, {&P, sizeof P}, one(NC) * sizeof(spslam_cull_record),
                           sizeof(spslam_cull_summary)}))
        return rc;
    spslam_covis_map dm{};
    dm.match_off = st.slot<int32_t>(kMatchOff);
    dm.match_row = st.slot<int32_t>(kMatchRow);
    dm.obs_off = st.slot<int32_t>(kObsOff);
    dm.obs_kf = st.slot<int32_t>(kObsKf);
    dm.obs_kp = st.slot<int32_t>(kObsKp);
    dm.kf_slot = st.slot<int32_t>(kSlot);
    dm.point_bad = m.point_bad ? st.slot<uint8_t>(kBad) : nullptr;
    dm.points = st.slot<spslam_local_point>(kPoints);
    spslam_covis_graph dg{};
    dg.ordered = st.slot<int32_t>(kOrdered);
    dg.n_ordered = st.slot<int32_t>(kNOrdered);
    dg.stride = (int32_t)stride;
    int rc = spslam_keyframe_culling_batch_device(
        c, 1, st.slot<spslam_cull_problem>(kProblem), &dm, &dg, st.slot<spslam_keypoint>(kKeys),
        st.slot<float>(kURight), st.slot<float>(kDepth), cap, st.slot<uint8_t>(kNewPlane),
        not_erase ? st.slot<uint8_t>(kNotErase) : nullptr, params, st.slot<spslam_cull_record>(kRecords),
        st.slot<spslam_cull_summary>(kSummary), c->stream);
    if (rc) return rc;
    HIP_CHECK(c, hipMemcpyAsync(summary, st.slot<void>(kSummary), sizeof *summary, hipMemcpyDeviceToHost, c->stream));
    // the uploads read the vectors above, and the record count is the device's
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    if (summary->n_candidates > 0)
        HIP_CHECK(c, hipMemcpyAsync(records, st.slot<void>(kRecords),
                                    (size_t)summary->n_candidates * sizeof(spslam_cull_record), hipMemcpyDeviceToHost,
                                    c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

int spslam_map_point_culling_batch_device(spslam_ctx* c, const spslam_point_cull_map* map, const int32_t* d_rows,
                                          const int32_t* d_cur_kf_id, int n, int th_obs, uint8_t* d_verdict,
                                          void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!map || n < 0 || (n && (!d_rows || !d_cur_kf_id || !d_verdict || !map->found || !map->visible ||
                                !map->first_kf || !map->points)))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_map_point_culling_batch_device");
    HIP_CHECK(c, hipSetDevice(c->device));
    HIP_CHECK(c, map_point_culling_launch(*map, d_rows, d_cur_kf_id, n, th_obs, d_verdict, (hipStream_t)hip_stream));
    return SPSLAM_OK;
}

int spslam_map_point_culling(spslam_ctx* c, const spslam_point_cull_map* map, int n_rows, const int32_t* rows, int n,
                             int cur_kf_id, int th_obs, uint8_t* verdict) {
    if (!c) return SPSLAM_ERR_ARG;
    if (!map || (n > 0 && !verdict) ||
        (n_rows > 0 && (!map->found || !map->visible || !map->first_kf || !map->points)))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_map_point_culling");
    if (const char* e = covis_check_rows(rows, n, n_rows))
        return fail(c, SPSLAM_ERR_ARG, "spslam_map_point_culling: %s", e);
    if (n == 0) return SPSLAM_OK;
    HIP_CHECK(c, hipSetDevice(c->device));
    const spslam_point_cull_map& m = *map;
    const size_t R = (size_t)n_rows, N = (size_t)n, Pt = sizeof(spslam_local_point);
    const std::vector<int32_t> ids(N, cur_kf_id);
    enum { kFound, kVisible, kFirstKf, kBad, kPoints, kRows, kIds, kVerdict };
    Stage st(c);
    if (int rc = st.open({{m.found, R * 4}, {m.visible, R * 4}, {m.first_kf, R * 4},
                           {m.point_bad, m.point_bad ? R : 0, R}, {m.points, R * Pt}, {rows, N * 4},
                           {ids.data(), N * 4}, N}))
        return rc;
    spslam_point_cull_map dm{};
    dm.found = st.slot<int32_t>(kFound);
    dm.visible = st.slot<int32_t>(kVisible);
    dm.first_kf = st.slot<int32_t>(kFirstKf);
    dm.point_bad = m.point_bad ? st.slot<uint8_t>(kBad) : nullptr;
    dm.points = st.slot<spslam_local_point>(kPoints);
    int rc = spslam_map_point_culling_batch_device(c, &dm, st.slot<int32_t>(kRows), st.slot<int32_t>(kIds), n, th_obs,
                                                   st.slot<uint8_t>(kVerdict), c->stream);
    if (rc) return rc;
    HIP_CHECK(c, hipMemcpyAsync(verdict, st.slot<void>(kVerdict), N, hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.close())) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));  // also: the uploads have read `ids`
    return SPSLAM_OK;
}

}  // extern "C"
