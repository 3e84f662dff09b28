// C ABI (include/spslam_gpu.h): PoseOptimization, LocalBundleAdjustment and the solver debug entries.
#include "capi_ctx.h"

#include <chrono>
#include <cmath>
#include <thread>

namespace {
// the Schur layout's team threshold (measurement knob; the results do not depend on it)
int lba_rows_max_team() {
    static const int v = [] {
        const char* e = getenv("SPSLAM_LBG_ROWS_MAX_TEAM");
        return e ? atoi(e) : 4;
    }();
    return v;
}

// g2o order: one launch runs every problem's whole schedule
int lba_g2o_order(spslam_ctx* c, int n, const LbaIo& io, const LbaConsts& C, int pw, hipStream_t s) {
    HIP_CHECK(c, c->d_lba_ctl.reserve(lbg_ctl_ints(n) * sizeof(int), s));
    // workgroups per problem: the context's setting, else as many as fill the chip's CUs (one each), at most 8
    int team = c->lba_team;
    if (team <= 0) team = std::max(1, std::min(8, c->num_cus / n));
    LbgBatch B{n, c->d_lba_off, c->d_lba_scratch, io, c->lba_stop_after, team, c->solve_fail_mask, c->d_lba_ctl, pw,
               lba_rows_max_team()};
    HIP_CHECK(c, lba_run_g2o(B, C, s, c->timer));
    return SPSLAM_OK;
}

// host-buffer entry: mirror the caller's bool into the device-visible flag while the work on `s` runs
int mirror_stop_flag(spslam_ctx* c, hipStream_t s, const volatile uint8_t* stop_src, volatile int32_t* stop_mirror) {
    hipEvent_t ev;
    HIP_CHECK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_CHECK(c, hipEventRecord(ev, s));
    for (;;) {
        if (*stop_src) *stop_mirror = 1;
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) {
            (void)hipEventDestroy(ev);
            HIP_CHECK(c, q);
        }
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    HIP_CHECK(c, hipEventDestroy(ev));
    return SPSLAM_OK;
}

// fast order: phase kernels step by step over (problem, first index) work tables, polled by the host
int lba_fast_order(spslam_ctx* c, int n, const spslam_lba_problem* problems, const LbaIo& io, const LbaConsts& C,
                   int max_kf, hipStream_t s, const volatile uint8_t* stop_src, volatile int32_t* stop_mirror) {
    // work tables: edge chunks, landmark chunks, keyframe tasks, pose-pair (+ bs) tasks per problem
    std::vector<int2> ec, lc, kt, pt, qt, sg, pm;
    const int seg_own = lba_seg_own(std::min(std::max(max_kf, 1), kLbaMaxKeyframes));
    for (int i = 0; i < n; i++) {
        const spslam_lba_problem& p = problems[i];
        const int E = p.n_point_obs + p.n_plane_obs, L = p.n_points + p.n_planes;
        if (p.n_kf > kLbaMaxKeyframes) continue;  // rejected on the device (status -2)
        for (int e = 0; e < E; e += kLbaChunk) ec.push_back(int2{i, e});
        for (int l = 0; l < L; l += kLbaChunk) lc.push_back(int2{i, l});
        for (int k = 0; k < p.n_kf; k++) kt.push_back(int2{i, k});
        const int npmax = p.n_kf;  // bound on the free poses; surplus tasks exit on the device
        // pose-pair and right-hand-side Schur tasks (the latter encoded -(p + 1)) only where the reduced system
        // may exceed the matrix-core path (6 np > 16 x kLbaMfmaTiles rows), which forms both
        if (6 * npmax > 16 * kLbaMfmaTiles) {
            for (int q = 0; q < npmax * (npmax + 1) / 2; q++) pt.push_back(int2{i, q});
            for (int q = 0; q < npmax; q++) pt.push_back(int2{i, -(q + 1)});
        }
        for (int q = 0; q < p.n_plane_obs; q += kLbaPlaneEdgesPerTask) qt.push_back(int2{i, p.n_point_obs + q});
        for (int e = 0; e < p.n_point_obs; e += seg_own) sg.push_back(int2{i, e});
        for (int q = 0; q < p.n_planes; q += kLbaChunk / 64) pm.push_back(int2{i, p.n_points + q});
    }
    const std::vector<int2>* tables[] = {&ec, &lc, &kt, &pt, &qt, &sg, &pm};
    size_t n_work = 1;  // the tables back to back, then the active counter
    for (const auto* t : tables) n_work += t->size();
    HIP_CHECK(c, c->d_lba_work.reserve(n_work * sizeof(int2), s));
    std::vector<int2> work;
    work.reserve(n_work);
    const int2* w[7];  // each table's start in the device copy
    for (int t = 0; t < 7; t++) {
        w[t] = c->d_lba_work + work.size();
        work.insert(work.end(), tables[t]->begin(), tables[t]->end());
    }
    work.push_back(int2{0, 0});  // active counter
    HIP_CHECK(c, hipMemcpyAsync(c->d_lba_work, work.data(), work.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    LbaWork W{w[0], (int)ec.size(), w[1], (int)lc.size(), w[2], (int)kt.size(), w[3], (int)pt.size(),
              w[4], (int)qt.size(), w[5], (int)sg.size(), w[6], (int)pm.size(), seg_own};
    LbaBatch B{n, c->d_lba_off, c->d_lba_scratch, io, (int*)(c->d_lba_work + work.size() - 1), c->lba_stop_after};
    // optimize(5) + optimize(10), at most 10 trials per iteration, plus the two structure steps
    HIP_CHECK(c, lba_run(B, W, C, 15 * 10 + 4, s, c->timer, nullptr, stop_src, stop_mirror));
    return SPSLAM_OK;
}

int lba_batch(spslam_ctx* c, int n, const spslam_lba_problem* problems, const LbaIo& io,
              const spslam_plane_config* cfg, void* hip_stream, const volatile uint8_t* stop_src,
              volatile int32_t* stop_mirror) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n < 1 || !problems || !io.probs || !io.kfs || !cfg || !io.kf_out || !io.res)
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_lba_optimize_batch_device");
    LbaConsts C{};
    C.angle_info = 3282.8 / (cfg->angle_info * cfg->angle_info);
    C.dis_info = cfg->distance_info * cfg->distance_info;
    C.par_info = 3282.8 / (cfg->parallel_info * cfg->parallel_info);
    C.ver_info = 3282.8 / (cfg->vertical_info * cfg->vertical_info);
    C.plane_chi = cfg->chi;
    C.vp_chi = cfg->vp_chi;
    C.delta_mono = (float)std::sqrt(5.991);     // const float thHuberMono = sqrt(5.991)
    C.delta_stereo = (float)std::sqrt(7.815);
    C.delta_plane = (float)std::sqrt(cfg->chi);  // const float deltaPlane = sqrt(planeChi)
    C.delta_vp = (float)std::sqrt(cfg->vp_chi);
    std::vector<long long> off(n);
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the default stream (header)
    if (!c->lba_done) HIP_CHECK(c, hipEventCreateWithFlags(&c->lba_done, hipEventDisableTiming));
    // the previous LBA call of this context (on any stream) has finished reading the offsets, ctl and scratch
    // before this one's copies on `s` rewrite them (recorded below after every launch; a never-recorded event
    // is complete)
    HIP_CHECK(c, hipStreamWaitEvent(s, c->lba_done, 0));
    const bool g2o = c->lba_order == SPSLAM_LBA_G2O_ORDER;
    // the g2o instance: pose masks of one word (up to 64 free poses) unless a window has more keyframes than that
    int max_kf = 0;
    for (int i = 0; i < n; i++) max_kf = std::max(max_kf, problems[i].n_kf);
    const int pw = lbg_pw_for(max_kf);
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        const spslam_lba_problem& p = problems[i];
        if (p.n_kf < 0 || p.n_points < 0 || p.n_planes < 0 || p.n_point_obs < 0 || p.n_plane_obs < 0)
            return fail(c, SPSLAM_ERR_ARG, "negative count in LBA problem%s", "");
        if ((p.n_points && (!io.pts || !io.pobs || !io.pt_out || !io.pobs_out)) ||
            (p.n_planes && (!io.pls || !io.plobs || !io.pl_out || !io.plobs_out)))
            return fail(c, SPSLAM_ERR_ARG, "missing LBA buffers%s", "");
        const int E = p.n_point_obs + p.n_plane_obs;
        off[i] = (long long)total;
        total += g2o ? lbg_layout(std::min(p.n_kf, kLbgMaxKeyframes), p.n_points, p.n_planes, E, pw).bytes
                     : lba_layout(p.n_kf, p.n_points, p.n_planes, E).bytes;
    }
    HIP_CHECK(c, c->d_lba_scratch.reserve(total, s));
    HIP_CHECK(c, c->d_lba_off.reserve((size_t)n * sizeof(long long), s));
    HIP_CHECK(c, hipMemcpyAsync(c->d_lba_off, off.data(), (size_t)n * sizeof(long long), hipMemcpyHostToDevice, s));
    const int rc = g2o ? lba_g2o_order(c, n, io, C, pw, s)
                       : lba_fast_order(c, n, problems, io, C, max_kf, s, stop_src, stop_mirror);
    if (rc) return rc;
    HIP_CHECK(c, hipEventRecord(c->lba_done, s));
    // the fast order's host loop mirrors the flag itself
    return g2o && stop_src ? mirror_stop_flag(c, s, stop_src, stop_mirror) : SPSLAM_OK;
}
}  // namespace

extern "C" {

int spslam_pose_optimize_batch_device(spslam_ctx* c, int n, const spslam_pose_problem* d_problems,
                                      const spslam_point_obs* d_points, const spslam_plane_obs* d_planes,
                                      const spslam_plane_config* cfg, const spslam_pose_result* d_init_from,
                                      spslam_pose_result* d_results, uint8_t* d_point_outlier,
                                      uint8_t* d_plane_outlier, void* hip_stream) {
    if (!c) return SPSLAM_ERR_ARG;
    if (n < 0 || !cfg || (n > 0 && (!d_problems || !d_points || !d_results || !d_point_outlier)))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_pose_optimize_batch_device");
    if (n == 0) return SPSLAM_OK;
    HIP_CHECK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)hip_stream;  // NULL = the default stream (header)
    PoseConsts K = make_pose_consts(*cfg);
    if (c->pose_spin_cap != 0) K.spin_cap = c->pose_spin_cap;
    K.fail_mask = c->solve_fail_mask;
    if (c->timer) c->timer->begin(kKindPose, s);
    HIP_CHECK(c, pose_launch(n, d_problems, d_points, d_planes, K, d_init_from, d_results, d_point_outlier,
                             d_plane_outlier, s));
    if (c->timer) c->timer->end(kKindPose, s);
    return SPSLAM_OK;
}

int spslam_pose_optimize(spslam_ctx* c, const spslam_pose_problem* problem, const spslam_point_obs* points,
                         const spslam_plane_obs* planes, const spslam_plane_config* cfg, spslam_pose_result* result,
                         uint8_t* point_outlier, uint8_t* plane_outlier) {
    if (!c || !problem || !cfg || !result) return SPSLAM_ERR_ARG;
    const int np = problem->n_points, nl = problem->n_planes;
    if (np < 0 || nl < 0 || (np && (!points || !point_outlier)) || (nl && (!planes || !plane_outlier)))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_pose_optimize");
    HIP_CHECK(c, hipSetDevice(c->device));
    spslam_pose_problem prob = *problem;
    prob.point_offset = 0;
    prob.plane_offset = 0;
    const size_t pts_bytes = (size_t)np * sizeof(spslam_point_obs), pls_bytes = (size_t)nl * sizeof(spslam_plane_obs);
    Stage st(c);  // a need above the capacity allocates twice that need: slowly growing frames reallocate rarely
    if (int rc = st.open({{&prob, sizeof prob}, sizeof(spslam_pose_result), {points, pts_bytes}, {planes, pls_bytes},
                          (size_t)np + 1, (size_t)nl + 1},
                         &c->d_pose_scratch, 2))
        return rc;
    auto* d_res = st.slot<spslam_pose_result>(1);
    auto *d_po = st.slot<uint8_t>(4), *d_plo = st.slot<uint8_t>(5);
    int rc = spslam_pose_optimize_batch_device(c, 1, st.slot<spslam_pose_problem>(0), st.slot<spslam_point_obs>(2),
                                               st.slot<spslam_plane_obs>(3), cfg, nullptr, d_res, d_po, d_plo,
                                               c->stream);
    if (rc) return rc;
    HIP_CHECK(c, hipMemcpyAsync(result, d_res, sizeof *result, hipMemcpyDeviceToHost, c->stream));
    if (np) HIP_CHECK(c, hipMemcpyAsync(point_outlier, d_po, np, hipMemcpyDeviceToHost, c->stream));
    if (nl) HIP_CHECK(c, hipMemcpyAsync(plane_outlier, d_plo, nl, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

int spslam_lba_set_team(spslam_ctx* c, int workgroups) {
    if (!c || workgroups < 0 || workgroups > kLbgTeamMax) return SPSLAM_ERR_ARG;
    c->lba_team = workgroups;
    return SPSLAM_OK;
}

int spslam_lba_set_order(spslam_ctx* c, int order) {
    if (!c || (order != SPSLAM_LBA_G2O_ORDER && order != SPSLAM_LBA_FAST_ORDER)) return SPSLAM_ERR_ARG;
    c->lba_order = order;
    return SPSLAM_OK;
}

int spslam_lba_debug_stop_after(spslam_ctx* c, int trials) {
    if (!c || trials < -1) return SPSLAM_ERR_ARG;
    c->lba_stop_after = trials;
    return SPSLAM_OK;
}

int spslam_lba_optimize_batch_device(spslam_ctx* c, int n, const spslam_lba_problem* problems,
                                     const spslam_lba_problem* d_problems, const spslam_lba_keyframe* d_kfs,
                                     const spslam_lba_point* d_points, const spslam_lba_point_obs* d_point_obs,
                                     const spslam_lba_plane* d_planes, const spslam_lba_plane_obs* d_plane_obs,
                                     const spslam_plane_config* cfg, float* d_kf_out, float* d_pt_out,
                                     float* d_pl_out, uint8_t* d_point_obs_outlier, uint8_t* d_plane_obs_outlier,
                                     spslam_lba_result* d_results, const int32_t* d_stop_flags, void* hip_stream) {
    const LbaIo io{d_problems, d_kfs, d_points, d_point_obs, d_planes, d_plane_obs, d_kf_out, d_pt_out, d_pl_out,
                   d_point_obs_outlier, d_plane_obs_outlier, d_results, d_stop_flags};
    return lba_batch(c, n, problems, io, cfg, hip_stream, nullptr, nullptr);
}

int spslam_lba_optimize(spslam_ctx* c, const spslam_lba_problem* problem, const spslam_lba_keyframe* kfs,
                        const spslam_lba_point* points, const spslam_lba_point_obs* point_obs,
                        const spslam_lba_plane* planes, const spslam_lba_plane_obs* plane_obs,
                        const spslam_plane_config* cfg, float* kf_out, float* pt_out, float* pl_out,
                        uint8_t* point_obs_outlier, uint8_t* plane_obs_outlier, spslam_lba_result* result,
                        const volatile uint8_t* stop_flag) {
    if (!c || !problem || !cfg || !result) return SPSLAM_ERR_ARG;
    spslam_lba_problem P = *problem;
    P.kf_offset = P.point_offset = P.plane_offset = 0;
    const size_t nk = P.n_kf, np = P.n_points, nq = P.n_planes, npo = P.n_point_obs, nqo = P.n_plane_obs;
    if ((nk && (!kfs || !kf_out)) || (np && (!points || !pt_out)) || (nq && (!planes || !pl_out)) ||
        (npo && (!point_obs || !point_obs_outlier)) || (nqo && (!plane_obs || !plane_obs_outlier)))
        return fail(c, SPSLAM_ERR_ARG, "bad argument%s", " to spslam_lba_optimize");
    HIP_CHECK(c, hipSetDevice(c->device));
    // six inputs, then the six outputs in the order of `dst` below
    const size_t in[] = {sizeof P, nk * sizeof(spslam_lba_keyframe), np * sizeof(spslam_lba_point),
                         npo * sizeof(spslam_lba_point_obs), nq * sizeof(spslam_lba_plane),
                         nqo * sizeof(spslam_lba_plane_obs)};
    const size_t out[] = {nk * 64, np * 12, nq * 16, npo, nqo, sizeof(spslam_lba_result)};
    Stage st(c);
    if (int rc = st.open({{&P, in[0]}, {kfs, in[1]}, {points, in[2]}, {point_obs, in[3]}, {planes, in[4]},
                          {plane_obs, in[5]}, out[0], out[1], out[2], out[3], out[4], out[5]},
                         &c->d_lba_stage))
        return rc;
    if (stop_flag && !c->h_lba_stop) {
        HIP_CHECK(c, hipHostMalloc((void**)&c->h_lba_stop, sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent));
        HIP_CHECK(c, hipHostGetDevicePointer((void**)&c->d_lba_stop, c->h_lba_stop, 0));
    }
    if (stop_flag) *(volatile int32_t*)c->h_lba_stop = *stop_flag ? 1 : 0;
    const LbaIo io{st.slot<spslam_lba_problem>(0), st.slot<spslam_lba_keyframe>(1), st.slot<spslam_lba_point>(2),
                   st.slot<spslam_lba_point_obs>(3), st.slot<spslam_lba_plane>(4), st.slot<spslam_lba_plane_obs>(5),
                   st.slot<float>(6), st.slot<float>(7), st.slot<float>(8), st.slot<uint8_t>(9),
                   st.slot<uint8_t>(10), st.slot<spslam_lba_result>(11), stop_flag ? c->d_lba_stop : nullptr};
    int rc = lba_batch(c, 1, &P, io, cfg, c->stream, stop_flag, stop_flag ? c->h_lba_stop : nullptr);
    if (rc) return rc;
    void* dst[] = {kf_out, pt_out, pl_out, point_obs_outlier, plane_obs_outlier, result};
    for (int i = 0; i < 6; i++)
        if (out[i]) HIP_CHECK(c, hipMemcpyAsync(dst[i], st.slot<void>(6 + i), out[i], hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return result->status == 0 ? SPSLAM_OK : fail(c, SPSLAM_ERR_ARG, "LBA problem rejected (status %s)", "< 0");
}

int spslam_debug_force_solve_failures(spslam_ctx* c, unsigned trial_mask) {
    if (!c) return SPSLAM_ERR_ARG;
    c->solve_fail_mask = trial_mask;
    return SPSLAM_OK;
}

int spslam_debug_pose_spin_cap(spslam_ctx* c, int cap) {
    if (!c || cap < -1) return SPSLAM_ERR_ARG;
    c->pose_spin_cap = cap;
    return SPSLAM_OK;
}

int spslam_debug_libm64(spslam_ctx* c, int kind, const double* a, const double* b, int n, double* out) {
    if (!c || n < 0 || kind < 0 || kind > 3 || (n && (!a || !out || (kind == 2 && !b)))) return SPSLAM_ERR_ARG;
    if (!n) return SPSLAM_OK;
    HIP_CHECK(c, hipSetDevice(c->device));
    const size_t nb = (size_t)n * 8;
    Stage st(c);
    if (int rc = st.open({{a, nb}, {b, kind == 2 ? nb : 0, nb}, nb})) return rc;
    HIP_CHECK(c, libm64_debug_launch(kind, st.slot<double>(0), st.slot<double>(1), n, st.slot<double>(2), c->stream));
    HIP_CHECK(c, hipMemcpyAsync(out, st.slot<double>(2), nb, hipMemcpyDeviceToHost, c->stream));
    if (int rc = st.close()) return rc;
    HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return SPSLAM_OK;
}

}  // extern "C"
