// C ABI (include/spslam_gpu.h), Tracking's device graph and its local map: spslam_track_graph_batch_device,
// spslam_track_refkf_batch_device, spslam_track_refkf_vote_batch_device,
// spslam_track_update_local_map[_batch_device] (UpdateLocalMap) and spslam_masked_frame_copy_device.
#include "capi_ctx.h"

extern "C" {

int spslam_track_graph_batch_device(spslam_ctx* c, int n_frames, int stage, const spslam_track_batch* batch,
                                    void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n_frames < 1 || !batch || stage < SPSLAM_TRACK_MOTION_MODEL || stage > SPSLAM_TRACK_LAST_FRAME)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_track_graph_batch_device");
    const spslam_track_batch& b = *batch;
    const bool common = track_batch_ok(b);
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
    bool ok = track_batch_ok(b) && b.point_outlier && r.nmatches && r.fallback;
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
    const bool ok = track_batch_ok(b) && b.point_outlier && v.kf_base && v.kf_sets && v.refkf_index && v.refkf_sets;
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
        ok = ok && mm && track_batch_ok(*mm) && mm->point_outlier;
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

}  // extern "C"
