// ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) on gfx950
// (src/ORBmatcher.cc:1328-1470, Frame::GetFeaturesInArea src/Frame.cc:427-480,
// DescriptorDistance :1647-1662, ComputeThreeMaxima :1601-1642) for a batch of
// frame pairs, with TrackWithMotionModel's second search at 2*th when fewer
// than retry_below matches (src/Tracking.cc:968-975).  Semantics:
// oracle/match_oracle.cpp.
//
//   match_window_kernel  grid (frame, 16 last-frame points), 16 lanes per point:
//                        projection and search window (redundantly per lane),
//                        the window's grid cells spread over the lanes, every
//                        candidate's Hamming distance (v_bcnt over the XOR of 8
//                        dwords); keeps the kProjKeys (6) best as (distance << 20 | CSR
//                        position), which orders ties like the reference's
//                        cell-by-cell scan, merged over the lanes (keys are
//                        unique, so the merge is the serial scan's result);
//   match_assign_kernel  grid (frame), one wave: the reference's loop is
//                        sequential only through `mvpMapPoints[i2] taken`, so
//                        the wave walks the points in order, accepts each
//                        point's precomputed best unless an earlier point took
//                        that keypoint, and only then re-scans the window
//                        cooperatively (64 lanes, min over keys) excluding the
//                        taken keypoints (LDS bitmap); then the rotation
//                        histogram check.
//   fuse_search_kernel   ORBmatcher::Fuse(pKF, vpMapPoints, th), the search (:842-949): the window kernel's
//                        shape, 4 lanes per point, with Fuse's own candidate test; no in-order walk (below).
//   sim3_search_kernel, sim3_agree_kernel; proj_sim3_window_kernel, proj_sim3_assign_kernel;
//   fuse_sim3_search_kernel   LoopClosing's Sim3 matchers: SearchBySim3 (:1102-1326), SearchByProjection(pKF, Scw,
//                        ...) (:290-403) and the search of Fuse(pKF, Scw, ...) (:977-1079), described at the kernels.
// Float expressions follow the reference build's contraction pattern; the
// cv::Mat products are accumulated in double and rounded once (oracle header).
#include <hip/hip_runtime.h>

#include "wave_priority.h"

#include "match_launch.h"
#include "orb_match_device.h"
#include "wave_ops.h"

namespace spslam {
namespace match {

using namespace orb_match;

constexpr int kThreads = 256, kCols = SPSLAM_GRID_COLS, kRows = SPSLAM_GRID_ROWS, kThHigh = 100;
constexpr uint32_t kNone = 0xffffffffu;
// lanes per last-frame point in match_window_kernel: the serial chain of dependent loads (cell bounds,
// grid index, keypoint, descriptor) per candidate is what the in-step time of the window search is made of
// when the extraction streams load the memory system, so the window's cells are split over the lanes
constexpr int kGrp = 16, kPtsPerBlock = kThreads / kGrp;
// local-map windows are a few cells (radius 2.5-4 px x scale): 4 lanes per local point
constexpr int kLGrp = 4, kLPtsPerBlock = kThreads / kLGrp;

// insert a key into the ascending K smallest (keys unique; kNone = +inf)
template <int K>
__device__ __forceinline__ void insk(uint32_t (&b)[K], uint32_t x) {
#pragma unroll
    for (int q = 0; q < K; q++) {
        const uint32_t lo = min(b[q], x);
        x = max(b[q], x);
        b[q] = lo;
    }
}

__device__ __forceinline__ void mat3_mul(const float* T, const float* x, const float* c, bool transpose, double sign,
                                         float* y) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++)
            s = __dadd_rn(s, __dmul_rn((double)(transpose ? T[4 * k + r] : T[4 * r + k]), (double)x[k]));
        s = __dmul_rn(s, sign);
        if (c) s = __dadd_rn(s, (double)c[r]);
        y[r] = (float)s;
    }
}

// bForward / bBackward of one frame pair (src/ORBmatcher.cc:1336-1349)
__device__ __forceinline__ void direction(const spslam_proj_frame& F, const MatchGeom& g, bool mono, bool* fwd,
                                          bool* bwd) {
    const float tcw[3] = {F.Tcw[3], F.Tcw[7], F.Tcw[11]};
    const float tlw[3] = {F.Tlw[3], F.Tlw[7], F.Tlw[11]};
    float twc[3], tlc[3];
    mat3_mul(F.Tcw, tcw, nullptr, true, -1.0, twc);
    mat3_mul(F.Tlw, twc, tlw, false, 1.0, tlc);
    const float mb = __fdiv_rn(g.bf, g.fx);
    *fwd = tlc[2] > mb && !mono;
    *bwd = -tlc[2] > mb && !mono;
}

// The current frame's arrays of batch entry f: the grid as CSR (cell offsets, keypoints by position), the
// undistorted keypoints, their descriptors and right coordinates.
struct FrameView {
    const int32_t *GO, *GI;
    const spslam_keypoint* kun;
    const uint8_t* desc;
    const float* uright;
};
__device__ __forceinline__ FrameView frame_view(const MatchCurrent& C, int f) {
    return {C.grid_off + (size_t)f * (kCols * kRows + 1), C.grid_idx + (size_t)f * C.cap,
            C.kun + (size_t)f * C.cap, C.desc + (size_t)f * C.cap * 32, C.uright + (size_t)f * C.cap};
}

// GetFeaturesInArea cell range of the window (u, v, r); false: the reference returns no candidates
__device__ __forceinline__ bool cell_range(float u, float v, float r, const MatchGeom& g, int* x0, int* x1, int* y0,
                                           int* y1) {
    *x0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(u, g.min_x), r), g.ginv_x)));
    *x1 = min(kCols - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(u, g.min_x), r), g.ginv_x)));
    *y0 = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(v, g.min_y), r), g.ginv_y)));
    *y1 = min(kRows - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(v, g.min_y), r), g.ginv_y)));
    return !(*x0 >= kCols || *x1 < 0 || *y0 >= kRows || *y1 < 0);
}

// What a window's candidates are tested against: the projection, the radius, the projected right coordinate
// (mTrackProjXR; ur = fma(-mbf, invz, u)), the octave range and the point's descriptor.
struct Probe {
    float u, v, r, ur;
    int min_level, max_level;
    uint4 d0, d1;
};
template <int K>
__device__ __forceinline__ Probe probe_of(const MatchWindowK<K>& w, const MatchGeom& g, const uint8_t* desc) {
    return {w.u, w.v, w.r, __fmaf_rn(-g.bf, w.invzc, w.u), w.min_level, w.max_level,
            *(const uint4*)desc, *(const uint4*)(desc + 16)};
}
template <int K>
__device__ __forceinline__ Probe probe_of(const LocalWindowK<K>& w, const uint8_t* desc) {
    return {w.u, w.v, w.rs, w.ur, w.level - 1, w.level, *(const uint4*)desc, *(const uint4*)(desc + 16)};
}

// Candidate test of GetFeaturesInArea + the stereo check on keypoint k at CSR position j; returns the key or kNone.
__device__ __forceinline__ uint32_t candidate_key(const Probe& p, const FrameView& V, int j, int k) {
    const spslam_keypoint kp = V.kun[k];
    const bool check = (p.min_level > 0) || (p.max_level >= 0);
    if (check) {
        if (kp.octave < p.min_level) return kNone;
        if (p.max_level >= 0 && kp.octave > p.max_level) return kNone;
    }
    const float dx = __fsub_rn(kp.x, p.u), dy = __fsub_rn(kp.y, p.v);
    if (!(fabsf(dx) < p.r && fabsf(dy) < p.r)) return kNone;
    const float urk = V.uright[k];
    if (urk > 0) {
        const float er = fabsf(__fsub_rn(p.ur, urk));
        if (er > p.r) return kNone;
    }
    return ((uint32_t)hamming(p.d0, p.d1, V.desc + 32 * (size_t)k) << 20) | (uint32_t)j;
}

// The K smallest keys over the cells x0 .. x1, y0 .. y1, left in every one of the point's G lanes (sub: this
// lane's index among them): the cells (column-major, as the reference scans them) are dealt round-robin to the
// lanes and the lanes' smallest keys merged (unique keys, so the merge is the serial scan's result); x1 < x0 or
// y1 < y0 (an empty range) gives no cells.  taken: one byte per keypoint, set ones are passed over; may be null.
template <int K, int G>
__device__ __forceinline__ void window_keys(const Probe& p, const FrameView& V, int x0, int x1, int y0, int y1,
                                            const uint8_t* taken, int sub, uint32_t (&bk)[K]) {
#pragma unroll
    for (int q = 0; q < K; q++) bk[q] = kNone;
    const int nrows = y1 - y0 + 1, ncells = x1 >= x0 && nrows > 0 ? (x1 - x0 + 1) * nrows : 0;
    for (int cell = sub; cell < ncells; cell += G) {
        const int cx = cell / nrows, c = (x0 + cx) * kRows + y0 + (cell - cx * nrows);
        const int j0 = V.GO[c], j1 = V.GO[c + 1];
        for (int j = j0; j < j1; j++) {
            const int k = V.GI[j];
            if (taken && taken[k]) continue;
            insk(bk, candidate_key(p, V, j, k));
        }
    }
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) {
        uint32_t pk[K];
#pragma unroll
        for (int q = 0; q < K; q++) pk[q] = (uint32_t)__shfl_xor((int)bk[q], o);
#pragma unroll
        for (int q = 0; q < K; q++) insk(bk, pk[q]);
    }
}

// The window w again by the whole wave, without the keypoints taken by now (LDS bitmap): *m1 / *m2 are the
// smallest and second smallest key among the candidates this lane tested (every 64th of each cell).
template <class Win>
__device__ __forceinline__ void rescan_window(const Probe& p, const FrameView& V, const Win& w, const uint32_t* taken,
                                              int lane, uint32_t* m1, uint32_t* m2) {
    uint32_t a = kNone, b = kNone;
    for (int ix = w.x0; ix <= w.x1; ix++)
        for (int iy = w.y0; iy <= w.y1; iy++) {
            const int c = ix * kRows + iy;
            for (int j = V.GO[c] + lane; j < V.GO[c + 1]; j += 64) {
                const int k = V.GI[j];
                if (bit_test(taken, k)) continue;
                const uint32_t key = candidate_key(p, V, j, k);
                if (key < a) { b = a; a = key; }
                else if (key < b) b = key;
            }
        }
    *m1 = a;
    *m2 = b;
}

template <int K>
__global__ __launch_bounds__(kThreads) void match_window_kernel(const spslam_proj_frame* __restrict__ frames,
                                                                const spslam_proj_point* __restrict__ points,
                                                                int max_points, MatchCurrent C, MatchGeom g, float th,
                                                                int mono, int retry_below, int pass,
                                                                const int* __restrict__ nmatches,
                                                                MatchWindowK<K>* __restrict__ win) {
    tail_wave_priority();
    const int f = blockIdx.x, sub = threadIdx.x & (kGrp - 1);
    const int i = blockIdx.y * kPtsPerBlock + (int)(threadIdx.x / kGrp);
    const spslam_proj_frame& F = frames[f];
    if (pass == 1 && !(retry_below > 0 && nmatches[f] < retry_below)) return;
    if (i >= F.n_points || i >= max_points) return;  // uniform over the point's lanes, as every return below
    MatchWindowK<K> w{};
#pragma unroll
    for (int q = 0; q < K; q++) {
        w.best[q] = kNone;
        w.kp[q] = -1;
    }
    w.valid = 0;
    w.x0 = 1;
    w.x1 = 0;
    const spslam_proj_point p = points[F.point_offset + i];
    bool fwd, bwd;
    direction(F, g, mono != 0, &fwd, &bwd);
    const float tcw[3] = {F.Tcw[3], F.Tcw[7], F.Tcw[11]};
    float x3Dc[3];
    mat3_mul(F.Tcw, p.xw, tcw, false, 1.0, x3Dc);
    const float invzc = (float)__ddiv_rn(1.0, (double)x3Dc[2]);
    MatchWindowK<K>* W = win + (size_t)f * max_points + i;
    if (invzc < 0) { if (sub == 0) *W = w; return; }
    const float u = __fmaf_rn(__fmul_rn(g.fx, x3Dc[0]), invzc, g.cx);
    const float v = __fmaf_rn(__fmul_rn(g.fy, x3Dc[1]), invzc, g.cy);
    if (u < g.min_x || u > g.max_x || v < g.min_y || v > g.max_y) { if (sub == 0) *W = w; return; }
    const int oct = p.octave;
    const float th_eff = pass == 1 ? __fmul_rn(2.0f, th) : th;
    const float r = __fmul_rn(th_eff, g.scale[oct]);
    w.u = u; w.v = v; w.r = r; w.invzc = invzc;
    if (fwd) { w.min_level = oct; w.max_level = -1; }
    else if (bwd) { w.min_level = 0; w.max_level = oct; }
    else { w.min_level = oct - 1; w.max_level = oct + 1; }
    w.valid = 1;
    int x0, x1, y0, y1;
    if (!cell_range(u, v, r, g, &x0, &x1, &y0, &y1)) { if (sub == 0) *W = w; return; }
    w.x0 = (int16_t)x0; w.x1 = (int16_t)x1; w.y0 = (int16_t)y0; w.y1 = (int16_t)y1;
    const FrameView V = frame_view(C, f);
    uint32_t bk[K];
    window_keys<K, kGrp>(probe_of(w, g, p.desc), V, x0, x1, y0, y1, nullptr, sub, bk);
    // lanes 0 .. K-1 resolve best[sub]'s keypoint and angle (read by the in-order walk)
    static_assert(K <= kGrp, "a lane per key");
    uint32_t mine = kNone;
#pragma unroll
    for (int q = 0; q < K; q++)
        if (sub == q) mine = bk[q];
    if (sub < K && mine != kNone) {
        const int k = V.GI[mine & 0xfffff];
        W->kp[sub] = k;
        W->kang[sub] = V.kun[k].angle;
    }
    if (sub == 0) {
        // kp / kang: written by lanes 0 .. K-1
        W->u = w.u; W->v = w.v; W->r = w.r; W->invzc = w.invzc;
        W->x0 = w.x0; W->x1 = w.x1; W->y0 = w.y0; W->y1 = w.y1;
        W->min_level = w.min_level; W->max_level = w.max_level; W->valid = w.valid; W->pad = 0;
#pragma unroll
        for (int q = 0; q < K; q++) W->best[q] = bk[q];
    }
    if (sub < K && mine == kNone) W->kp[sub] = -1;
}

template <int K>
__global__ __launch_bounds__(64) void match_assign_kernel(const spslam_proj_frame* __restrict__ frames,
                                                          const spslam_proj_point* __restrict__ points, int max_points,
                                                          MatchCurrent C, MatchGeom g, int check_ori, int retry_below,
                                                          int pass, const MatchWindowK<K>* __restrict__ win,
                                                          int2* __restrict__ pushes, int32_t* __restrict__ match,
                                                          int* __restrict__ nmatches) {
    tail_wave_priority();
    extern __shared__ uint32_t taken[];  // [ceil(cap / 32)], then claim[cap]
    __shared__ int hist[kHisto];
    __shared__ int ind[3];
    const int f = blockIdx.x, lane = threadIdx.x;
    const spslam_proj_frame& F = frames[f];
    if (pass == 1 && !(retry_below > 0 && nmatches[f] < retry_below)) return;
    const int n_kp = min(C.counts[f], C.cap), np = min(F.n_points, max_points);
    int32_t* M = match + (size_t)f * C.cap;
    const int words = (C.cap + 31) / 32;
    // claim[k]: per pass, first the earliest blocking acceptance of keypoint k, then the last committed one
    // (~0u / 0: none) -- one LDS atomic per lane instead of a 64-step shuffle scan per pass
    uint32_t* claim = taken + words;
    for (int k = lane; k < n_kp; k += 64) claim[k] = ~0u;
    for (int k = lane; k < n_kp; k += 64) M[k] = -1;  // fill(mvpMapPoints, NULL)
    for (int k = lane; k < words; k += 64) taken[k] = 0;
    if (lane < kHisto) hist[lane] = 0;
    __syncthreads();
    const MatchWindowK<K>* Wf = win + (size_t)f * max_points;
    const FrameView V = frame_view(C, f);
    const spslam_proj_point* P = points + F.point_offset;
    int2* PU = pushes + (size_t)f * max_points;
    int n_push = 0;
#ifdef SPSLAM_LA_DIAG  // diagnostic build: passes, serial stops and window re-scans per frame (device printf)
    int d_pass = 0, d_stop = 0, d_rescan = 0;
    const long long d_t0 = wall_clock64();
#endif
    // every lane fetches its point's precomputed state, one round of loads per 64 points, issued one chunk
    // ahead (in flight during the previous chunk's walk) ...
    MatchWindowK<K> wn{};
    int nobs_n = 0;
    float pang_n = 0.f;
    if (lane < np) { wn = Wf[lane]; nobs_n = P[lane].n_obs; pang_n = P[lane].angle; }
    for (int c0 = 0; c0 < np; c0 += 64) {
        const int i = c0 + lane;
        int valid = 0, blocking = 0;
        uint32_t best[K];
        int b[K];
        float kang[K];
#pragma unroll
        for (int q = 0; q < K; q++) {
            best[q] = kNone;
            b[q] = -1;
            kang[q] = 0.f;
        }
        float pangle = 0.f;
        const MatchWindowK<K> w = wn;
        const int nobs = nobs_n;
        const float pang = pang_n;
        if (i + 64 < np) { wn = Wf[i + 64]; nobs_n = P[i + 64].n_obs; pang_n = P[i + 64].angle; }
        if (i < np) {
            valid = w.valid;
#pragma unroll
            for (int q = 0; q < K; q++) {
                best[q] = w.best[q];
                if (valid && best[q] != kNone) {
                    b[q] = w.kp[q];  // resolved by the window kernel
                    kang[q] = w.kang[q];
                }
            }
            blocking = nobs > 0;
            pangle = pang;
        }
        // ... then the reference's loop over the 64 points, in passes: every point still to do takes the first of
        // its smallest keys whose keypoint is free; the points before the first one that cannot be decided
        // that way -- all K keys taken (a window re-scan), or its keypoint taken by an earlier point of the pass
        // that blocks it (a map point with observations) -- are committed together, in order; that point is
        // then walked alone (the reference's step with the updated taken set) and the next pass starts after it.
        const int m = min(64, np - c0);
        int start = 0;
        while (start < m) {
#ifdef SPSLAM_LA_DIAG
            d_pass++;
#endif
            uint32_t keyl = kNone;
            int bl = -1;
            float kangl = 0.f;
            bool rescanl = false;
            const bool act = lane >= start && lane < m && valid;
            if (act) {
#pragma unroll
                for (int q = 0; q < K; q++) {
                    if (keyl != kNone || rescanl || best[q] == kNone) continue;
                    if (!bit_test(taken, b[q])) { keyl = best[q]; bl = b[q]; kangl = kang[q]; }
                    else if (q == K - 1) rescanl = true;
                }
            }
            const bool acc = act && !rescanl && keyl != kNone && (int)(keyl >> 20) <= kThHigh;
            const bool accb = acc && blocking;
            // conflicts with earlier blocking acceptances (the earliest blocking lane per keypoint)
            if (accb) atomicMin(&claim[bl], (uint32_t)lane);
            wave_sync();
            const bool conflict = acc && claim[bl] < (uint32_t)lane;
            wave_sync();
            if (acc) claim[bl] = 0u;  // reused below as "last committed lane + 1" (0: none)
            wave_sync();
            const bool stop = act && (rescanl || (acc && conflict));
            const unsigned long long sm = __ballot(stop);
            const int first = sm ? __ffsll((long long)sm) - 1 : m;
            const bool commit = acc && lane < first;
            const unsigned long long cm = __ballot(commit);
            // the last committed assignment of a keypoint wins, as in the reference's order
            if (commit) atomicMax(&claim[bl], (uint32_t)lane + 1u);
            wave_sync();
            const bool last = commit && claim[bl] == (uint32_t)lane + 1u;
            wave_sync();
            if (acc) claim[bl] = ~0u;
            int bin = 0;
            if (commit) {
                if (last) M[bl] = c0 + lane;
                if (blocking) bit_set_atomic(taken, bl);
                if (check_ori) {
                    bin = rotation_bin(pangle, kangl);
                    atomicAdd(&hist[bin], 1);
                }
                PU[n_push + __popcll(cm & ((1ull << lane) - 1ull))] = make_int2(bl, bin);
            }
            n_push += __popcll(cm);
            wave_sync();
            if (first >= m) break;
#ifdef SPSLAM_LA_DIAG
            d_stop++;
#endif
            // the point that stopped the pass, alone (the reference's step for it)
            const int L = first;
            uint32_t bestL = kNone;
            int bL = -1;
            float kangL = 0.f;
            bool rescan = false;
#pragma unroll
            for (int q = 0; q < K; q++) {
                const uint32_t kq = (uint32_t)__shfl((int)best[q], L);
                const int bq = __shfl(b[q], L);
                const float aq = __shfl(kang[q], L);
                if (bestL != kNone || rescan || kq == kNone) continue;  // sorted: kNone ends the list
                if (!bit_test(taken, bq)) { bestL = kq; bL = bq; kangL = aq; }
                else if (q == K - 1) rescan = true;
            }
            if (rescan) {
#ifdef SPSLAM_LA_DIAG
                d_rescan++;
#endif
                // an earlier point holds this keypoint: search the window again without the taken ones
                const MatchWindowK<K> w = Wf[c0 + L];
                uint32_t m1, m2;
                rescan_window(probe_of(w, g, P[c0 + L].desc), V, w, taken, lane, &m1, &m2);
                bestL = wave_min(m1);
                if (bestL != kNone) {
                    bL = V.GI[bestL & 0xfffff];
                    kangL = V.kun[bL].angle;
                }
            }
            start = L + 1;
            if (bestL == kNone || (int)(bestL >> 20) > kThHigh) continue;
            const int blockL = __shfl(blocking, L);
            const float pangL = __shfl(pangle, L);
            if (lane == 0) {
                M[bL] = c0 + L;
                if (blockL) bit_set(taken, bL);
                int binL = 0;
                if (check_ori) {
                    binL = rotation_bin(pangL, kangL);
                    hist[binL]++;
                }
                PU[n_push] = make_int2(bL, binL);
            }
            n_push++;
            wave_sync();
        }
    }
    __syncthreads();
    int n = n_push;
    if (check_ori) {
        if (lane == 0) three_maxima(hist, &ind[0], &ind[1], &ind[2]);
        __syncthreads();
        const int i1 = ind[0], i2 = ind[1], i3 = ind[2];
        int removed = 0;
        for (int q = lane; q < n_push; q += 64) {
            const int2 e = PU[q];
            if (e.y != i1 && e.y != i2 && e.y != i3) {
                M[e.x] = -1;
                removed++;
            }
        }
        n -= wave_sum(removed);
    }
    if (lane == 0) nmatches[f] = n;
#ifdef SPSLAM_LA_DIAG
    if (lane == 0)
        printf("MA pass %d np %d nkp %d passes %d stops %d rescans %d matches %d us %.1f\n", pass, np, n_kp, d_pass,
               d_stop, d_rescan, n, (double)(wall_clock64() - d_t0) * 0.01);
#endif
}

// MapPoint::PredictScale: ceil(log(max_dist / dist) / mfLogScaleFactor), clamped to the levels; the correctly
// rounded logf gives the same level as glibc's for every float ratio (tests/test_libm_restated.py)
__device__ __forceinline__ int predict_scale(float max_dist, float dist, float log_scale_factor, int n_levels) {
    const float ratio = __fdiv_rn(max_dist, dist);
    const int n = (int)ceilf(__fdiv_rn((float)log((double)ratio), log_scale_factor));
    return n < 0 ? 0 : (n >= n_levels ? n_levels - 1 : n);
}

// ---------------------------------------------------------------------------
// Tracking::SearchLocalPoints: isInFrustum + PredictScale per local point,
// then ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:
// 45-130).  Same two-kernel shape: the window kernel keeps the kLocalKeys (6)
// smallest keys over the window (initially taken keypoints excluded); the
// in-order walk needs the best AND the second best among the keypoints still
// free (the ratio test), which the keys give unless in-loop assignments took
// all but one of them -- then the wave re-scans for both.
template <int K>
__global__ __launch_bounds__(kThreads) void local_window_kernel(const spslam_local_frame* __restrict__ frames,
                                                                const spslam_local_point* __restrict__ points,
                                                                int max_points, MatchCurrent C, MatchGeom g,
                                                                LocalConsts P, const uint8_t* __restrict__ taken_in,
                                                                LocalWindowK<K>* __restrict__ win,
                                                                uint8_t* __restrict__ in_view) {
    tail_wave_priority();
    const int f = blockIdx.x, sub = threadIdx.x & (kLGrp - 1);
    const int i = blockIdx.y * kLPtsPerBlock + (int)(threadIdx.x / kLGrp);
    const spslam_local_frame& F = frames[f];
    if (i >= F.n_points || i >= max_points) return;  // uniform over the point's lanes, as every return below
    LocalWindowK<K> w{};
#pragma unroll
    for (int q = 0; q < K; q++) {
        w.best[q] = kNone;
        w.kp[q] = -1;
        w.oct[q] = -1;
    }
    w.x0 = 1;
    w.x1 = 0;
    LocalWindowK<K>* W = win + (size_t)f * max_points + i;
    const spslam_local_point& p = points[F.point_offset + i];
    // points the frame already tracks (mnLastFrameSeen == the frame) are skipped before isInFrustum
    // (Tracking.cc:1396-1401); their mbTrackInView stays false
    if (P.seen && P.seen[F.seen_offset + p.id] == F.stamp) {
        if (sub == 0) {
            if (in_view) in_view[F.point_offset + i] = 0;
            *W = w;
        }
        return;
    }
    bool in = false;
    // Frame::isInFrustum(pMP, 0.5)
    const float tcw[3] = {F.Tcw[3], F.Tcw[7], F.Tcw[11]};
    float Pc[3], Ow[3];
    mat3_mul(F.Tcw, p.xw, tcw, false, 1.0, Pc);
    float u = 0.f, v = 0.f, invz = 0.f, viewCos = 0.f;
    int level = 0;
    do {
        if (Pc[2] < 0.0f) break;
        invz = __fdiv_rn(1.0f, Pc[2]);
        u = __fmaf_rn(__fmul_rn(g.fx, Pc[0]), invz, g.cx);
        v = __fmaf_rn(__fmul_rn(g.fy, Pc[1]), invz, g.cy);
        if (u < g.min_x || u > g.max_x || v < g.min_y || v > g.max_y) break;
        const float maxD = __fmul_rn(1.2f, p.max_dist), minD = __fmul_rn(0.8f, p.min_dist);
        mat3_mul(F.Tcw, tcw, nullptr, true, -1.0, Ow);
        const float PO[3] = {__fsub_rn(p.xw[0], Ow[0]), __fsub_rn(p.xw[1], Ow[1]), __fsub_rn(p.xw[2], Ow[2])};
        float sq = __fmul_rn(PO[0], PO[0]);
        sq = __fadd_rn(sq, __fmul_rn(PO[1], PO[1]));
        sq = __fadd_rn(sq, __fmul_rn(PO[2], PO[2]));
        const float dist = (float)__dsqrt_rn((double)sq);  // cv::norm
        if (dist < minD || dist > maxD) break;
        double dot = __dmul_rn((double)PO[0], (double)p.normal[0]);
        dot = __dadd_rn(dot, __dmul_rn((double)PO[1], (double)p.normal[1]));
        dot = __dadd_rn(dot, __dmul_rn((double)PO[2], (double)p.normal[2]));
        viewCos = (float)__ddiv_rn(dot, (double)dist);
        if (viewCos < P.view_cos_limit) break;
        level = predict_scale(p.max_dist, dist, P.log_scale_factor, P.n_levels);
        in = true;
    } while (false);
    if (in_view && sub == 0) in_view[F.point_offset + i] = in;
    if (!in) { if (sub == 0) *W = w; return; }
    float r = viewCos > 0.998f ? 2.5f : 4.0f;  // RadiusByViewingCos
    if (P.th != 1.0f) r = __fmul_rn(r, P.th);
    const float rs = __fmul_rn(r, g.scale[level]);
    w.u = u; w.v = v; w.rs = rs; w.ur = __fmaf_rn(-g.bf, invz, u);
    w.level = (int8_t)level;
    w.in_view = 1;
    int x0, x1, y0, y1;
    if (!cell_range(u, v, rs, g, &x0, &x1, &y0, &y1)) { if (sub == 0) *W = w; return; }
    w.x0 = (int16_t)x0; w.x1 = (int16_t)x1; w.y0 = (int16_t)y0; w.y1 = (int16_t)y1;
    // the frame-to-frame candidate test with this window, the initially taken keypoints passed over
    const FrameView V = frame_view(C, f);
    uint32_t bk[K];
    window_keys<K, kLGrp>(probe_of(w, p.desc), V, x0, x1, y0, y1, taken_in ? taken_in + (size_t)f * C.cap : nullptr,
                          sub, bk);
    // the keypoint and octave of each key (read by the in-order walk), resolved here
#pragma unroll
    for (int q = 0; q < K; q++) {
        w.best[q] = bk[q];
        if (bk[q] != kNone) {
            w.kp[q] = V.GI[bk[q] & 0xfffff];
            w.oct[q] = (int8_t)V.kun[w.kp[q]].octave;
        }
    }
    if (sub == 0) *W = w;
}

template <int K>
__global__ __launch_bounds__(64) void local_assign_kernel(const spslam_local_frame* __restrict__ frames,
                                                          const spslam_local_point* __restrict__ points,
                                                          int max_points, MatchCurrent C, MatchGeom g, LocalConsts P,
                                                          const uint8_t* __restrict__ taken_in,
                                                          const LocalWindowK<K>* __restrict__ win,
                                                          int32_t* __restrict__ match, int* __restrict__ nmatches) {
    tail_wave_priority();
    extern __shared__ uint32_t taken[];  // [ceil(cap / 32)], then claim[cap]
    const int f = blockIdx.x, lane = threadIdx.x;
    const spslam_local_frame& F = frames[f];
    const int n_kp = min(C.counts[f], C.cap), np = min(F.n_points, max_points);
    int32_t* M = match + (size_t)f * C.cap;
    const int words = (C.cap + 31) / 32;
    // claim[k]: the first lane of the current pass whose acceptance takes keypoint k (~0u: none); replaces a
    // 64-step shuffle scan per pass with one LDS atomic and two reads
    uint32_t* claim = taken + words;
    for (int k = lane; k < n_kp; k += 64) claim[k] = ~0u;
    const uint8_t* tk = taken_in ? taken_in + (size_t)f * C.cap : nullptr;
    for (int k = lane; k < n_kp; k += 64) M[k] = -1;
    // the taken bits: 8 coalesced byte loads in flight per lane, two words per ballot (a lane building its own
    // word byte by byte waited out 32 dependent loads per word)
    const int wset = tk ? 2 * ((n_kp + 63) / 64) : 0;  // words written from the flags (the rest are zero)
    for (int wd = wset + lane; wd < words; wd += 64) taken[wd] = 0u;
    for (int base = 0; base < n_kp && tk; base += 64 * 8) {
        uint8_t v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int k = base + 64 * u + lane;
            v[u] = tk[min(k, n_kp - 1)] & (uint8_t)(k < n_kp);  // unconditional load: no wait at a branch join
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const unsigned long long m = __ballot(v[u] != 0);
            const int wd = (base >> 5) + 2 * u;
            if (lane < 2 && wd + lane < min(words, wset)) taken[wd + lane] = (uint32_t)(m >> (32 * lane));
        }
    }
    __syncthreads();
    const LocalWindowK<K>* Wf = win + (size_t)f * max_points;
    const FrameView V = frame_view(C, f);
    const spslam_local_point* Pp = points + F.point_offset;
    int nm = 0;
#ifdef SPSLAM_LA_DIAG  // diagnostic build: passes, serial stops and window re-scans per frame (device printf)
    int d_pass = 0, d_stop = 0, d_rescan = 0;
    const long long d_t0 = wall_clock64();
#endif
    LocalWindowK<K> wn{};  // the next chunk's window states, loaded one chunk ahead
    if (lane < np) wn = Wf[lane];
    for (int c0 = 0; c0 < np; c0 += 64) {
        const int i = c0 + lane;
        int valid = 0;
        uint32_t best[K];
        int b[K], oc[K];
#pragma unroll
        for (int q = 0; q < K; q++) {
            best[q] = kNone;
            b[q] = -1;
            oc[q] = -1;
        }
        const LocalWindowK<K> w = wn;
        if (i + 64 < np) wn = Wf[i + 64];
        if (i < np) {
            valid = w.in_view;
#pragma unroll
            for (int q = 0; q < K; q++) {
                best[q] = w.best[q];
                if (valid && best[q] != kNone) {
                    b[q] = w.kp[q];  // resolved by the window kernel
                    oc[q] = w.oct[q];
                }
            }
        }
        // the reference's loop in passes (as in match_assign_kernel): every point still to do evaluates its best
        // and second best free keys from its smallest keys; the points before the first one that cannot be decided
        // that way -- a re-scan, or one of its two keypoints taken by an earlier acceptance of the pass -- are
        // committed together; that point is walked alone and the next pass starts after it.
        const int m = min(64, np - c0);
        auto ratio_ok = [&](uint32_t k1, uint32_t k2, int o1, int o2) {
            const int bestDist = (int)(k1 >> 20), bestDist2 = k2 != kNone ? (int)(k2 >> 20) : 256;
            const int bestLevel2 = k2 != kNone ? o2 : -1;
            if (bestDist > kThHigh) return false;
            return !(o1 == bestLevel2 && (float)bestDist > __fmul_rn(P.nn_ratio, (float)bestDist2));
        };
        int start = 0;
        while (start < m) {
#ifdef SPSLAM_LA_DIAG
            d_pass++;
#endif
            const bool act = lane >= start && lane < m && valid;
            uint32_t k1 = kNone, k2 = kNone;
            int b1 = -1, b2 = -1, o1 = -1, o2 = -1, nk = 0;
            if (act) {
#pragma unroll
                for (int q = 0; q < K; q++) {
                    if (best[q] == kNone) continue;
                    nk++;
                    if (bit_test(taken, b[q])) continue;
                    if (k1 == kNone) { k1 = best[q]; b1 = b[q]; o1 = oc[q]; }
                    else if (k2 == kNone) { k2 = best[q]; b2 = b[q]; o2 = oc[q]; }
                }
            }
            const bool rescanl = act && nk == K && k2 == kNone;
            const bool acc = act && !rescanl && k1 != kNone && ratio_ok(k1, k2, o1, o2);
            // conflict: an earlier accepting lane of this pass takes my best or second-best keypoint
            if (acc) atomicMin(&claim[b1], (uint32_t)lane);
            wave_sync();
            const bool conflict = act && k1 != kNone &&
                                  (claim[b1] < (uint32_t)lane || (b2 >= 0 && claim[b2] < (uint32_t)lane));
            wave_sync();
            if (acc) claim[b1] = ~0u;
            const bool stop = act && (rescanl || (k1 != kNone && conflict));
            const unsigned long long sm = __ballot(stop);
            const int first = sm ? __ffsll((long long)sm) - 1 : m;
            const bool commit = acc && lane < first;
            if (commit) {
                M[b1] = c0 + lane;
                bit_set_atomic(taken, b1);
            }
            nm += __popcll(__ballot(commit));
            wave_sync();
            if (first >= m) break;
            const int L = first;
            start = L + 1;
#ifdef SPSLAM_LA_DIAG
            d_stop++;
#endif
            k1 = kNone; k2 = kNone; b1 = -1; o1 = -1; o2 = -1; nk = 0;
#pragma unroll
            for (int q = 0; q < K; q++) {
                const uint32_t kq = (uint32_t)__shfl((int)best[q], L);
                const int bq = __shfl(b[q], L), oq = __shfl(oc[q], L);
                if (kq == kNone) continue;
                nk++;
                if (bit_test(taken, bq)) continue;
                if (k1 == kNone) { k1 = kq; b1 = bq; o1 = oq; }
                else if (k2 == kNone) { k2 = kq; o2 = oq; }
            }
            if (nk == K && k2 == kNone) {
                // in-loop assignments took all but one of the keys: best and second best over the window again
#ifdef SPSLAM_LA_DIAG
                d_rescan++;
#endif
                const LocalWindowK<K> w = Wf[c0 + L];
                uint32_t m1, m2;
                rescan_window(probe_of(w, Pp[c0 + L].desc), V, w, taken, lane, &m1, &m2);
                // wave top-2: the smallest key, then the smallest key above it
                k1 = wave_min(m1);
                k2 = wave_min(m1 == k1 ? m2 : m1);
                b1 = k1 != kNone ? V.GI[k1 & 0xfffff] : -1;
                o1 = b1 >= 0 ? V.kun[b1].octave : -1;
                o2 = k2 != kNone ? V.kun[V.GI[k2 & 0xfffff]].octave : -1;
            }
            if (k1 == kNone || !ratio_ok(k1, k2, o1, o2)) continue;
            if (lane == 0) {
                M[b1] = c0 + L;
                bit_set(taken, b1);
            }
            nm++;
            wave_sync();
        }
    }
    if (lane == 0) nmatches[f] = nm;
#ifdef SPSLAM_LA_DIAG
    if (lane == 0)
        printf("LA np %d nkp %d passes %d stops %d rescans %d matches %d us %.1f\n", np, n_kp, d_pass, d_stop,
               d_rescan, nm, (double)(wall_clock64() - d_t0) * 0.01);
#endif
}

// ---------------------------------------------------------------------------
// ORBmatcher::Fuse(pKF, vpMapPoints, th), the search (src/ORBmatcher.cc:842-949): one point per kLGrp lanes, no
// in-order walk -- with every point at most once in the list the search of point i does not depend on the map
// mutation (:951-971) of the points before it (include/spslam_gpu.h), so the kernel is the window kernel alone.
// Its float expressions are Fuse's own, with the contractions GCC emits for them (tests/test_fuse_host.py).
constexpr int kFusePtsPerBlock = kThreads / kLGrp;
constexpr int kThLow = 50;

struct FuseProbe {
    float u, v, ur, r;
    int level;
    uint4 d0, d1;
};

// Fuse's loop body for keypoint k at CSR position j (:903-949): the key, or kNone when the keypoint is not in
// vIndices or fails the level or chi-square test; *in_area: it is in vIndices (KeyFrame::GetFeaturesInArea's test).
__device__ __forceinline__ uint32_t fuse_candidate_key(const FuseProbe& p, const FrameView& V, const FuseConsts& P,
                                                       int j, int k, bool* in_area) {
    const spslam_keypoint kp = V.kun[k];
    const float dx = __fsub_rn(kp.x, p.u), dy = __fsub_rn(kp.y, p.v);
    if (!(fabsf(dx) < p.r && fabsf(dy) < p.r)) return kNone;
    *in_area = true;
    if (kp.octave < p.level - 1 || kp.octave > p.level) return kNone;
    const float ex = __fsub_rn(p.u, kp.x), ey = __fsub_rn(p.v, kp.y);
    float e2 = __fmaf_rn(ex, ex, __fmul_rn(ey, ey));  // ex*ex+ey*ey
    const float kpr = V.uright[k];
    double limit = 5.99;
    if (kpr >= 0) {  // the stereo branch: >= 0 here, 0.0f included (:914)
        const float er = __fsub_rn(p.ur, kpr);
        e2 = __fmaf_rn(er, er, e2);  // ex*ex+ey*ey+er*er
        limit = 7.8;
    }
    if ((double)__fmul_rn(e2, level_entry(P.inv_sigma2, kp.octave)) > limit) return kNone;
    return ((uint32_t)hamming(p.d0, p.d1, V.desc + 32 * (size_t)k) << 20) | (uint32_t)j;
}

// One point: the status; *level once PredictScale is reached; *best the smallest key, in every lane of the point.
// Every return is uniform over the point's lanes.
__device__ __forceinline__ int fuse_point(const spslam_fuse_problem& F, const spslam_local_point& p,
                                          const MatchCurrent& C, const MatchGeom& g, const FuseConsts& P, int sub,
                                          int* level, uint32_t* best) {
    const float tcw[3] = {F.Tcw[3], F.Tcw[7], F.Tcw[11]};
    float Pc[3], Ow[3];
    mat3_mul(F.Tcw, p.xw, tcw, false, 1.0, Pc);  // Rcw*p3Dw + tcw
    if (Pc[2] < 0.0f) return SPSLAM_FUSE_BEHIND;
    const float invz = __fdiv_rn(1.0f, Pc[2]);
    const float x = __fmul_rn(Pc[0], invz), y = __fmul_rn(Pc[1], invz);
    const float u = __fmaf_rn(g.fx, x, g.cx), v = __fmaf_rn(g.fy, y, g.cy);  // fx*x+cx (:863)
    // KeyFrame::IsInImage: half open (KeyFrame.cc:627-630); z == 0 makes u / v inf or NaN, which fail it
    if (!(u >= g.min_x && u < g.max_x && v >= g.min_y && v < g.max_y)) return SPSLAM_FUSE_OUTSIDE_IMAGE;
    const float ur = __fmaf_rn(-g.bf, invz, u);  // u-bf*invz (:870)
    const float maxD = __fmul_rn(1.2f, p.max_dist), minD = __fmul_rn(0.8f, p.min_dist);
    mat3_mul(F.Tcw, tcw, nullptr, true, -1.0, Ow);
    const float PO[3] = {__fsub_rn(p.xw[0], Ow[0]), __fsub_rn(p.xw[1], Ow[1]), __fsub_rn(p.xw[2], Ow[2])};
    float sq = __fmul_rn(PO[0], PO[0]);
    sq = __fadd_rn(sq, __fmul_rn(PO[1], PO[1]));
    sq = __fadd_rn(sq, __fmul_rn(PO[2], PO[2]));
    const float dist = (float)__dsqrt_rn((double)sq);  // cv::norm, local_window_kernel's reading
    if (dist < minD || dist > maxD) return SPSLAM_FUSE_OUT_OF_RANGE;
    double dot = __dmul_rn((double)PO[0], (double)p.normal[0]);
    dot = __dadd_rn(dot, __dmul_rn((double)PO[1], (double)p.normal[1]));
    dot = __dadd_rn(dot, __dmul_rn((double)PO[2], (double)p.normal[2]));
    if (dot < __dmul_rn(0.5, (double)dist)) return SPSLAM_FUSE_VIEW_ANGLE;  // doubles, no division (:884)
    *level = predict_scale(p.max_dist, dist, P.log_scale_factor, P.n_levels);  // PredictScale(dist3D, pKF)
    const FuseProbe q{u, v, ur, __fmul_rn(P.th, level_entry(g.scale, *level)), *level,
                      *(const uint4*)p.desc, *(const uint4*)(p.desc + 16)};
    int x0, x1, y0, y1;
    if (!cell_range(u, v, q.r, g, &x0, &x1, &y0, &y1)) return SPSLAM_FUSE_NO_CANDIDATES;
    // the window's cells (column-major, as KeyFrame::GetFeaturesInArea scans them) dealt to the point's lanes
    const FrameView V = frame_view(C, F.kf_slot);
    uint32_t bk[1] = {kNone};
    bool any = false;
    const int nrows = y1 - y0 + 1, ncells = (x1 - x0 + 1) * nrows;
    for (int cell = sub; cell < ncells; cell += kLGrp) {
        const int cx = cell / nrows, c = (x0 + cx) * kRows + y0 + (cell - cx * nrows);
        const int j0 = V.GO[c], j1 = V.GO[c + 1];
        for (int j = j0; j < j1; j++) insk(bk, fuse_candidate_key(q, V, P, j, V.GI[j], &any));
    }
    int anyi = any;
#pragma unroll
    for (int o = kLGrp / 2; o >= 1; o >>= 1) {
        insk(bk, (uint32_t)__shfl_xor((int)bk[0], o));
        anyi |= __shfl_xor(anyi, o);
    }
    *best = bk[0];
    return anyi ? SPSLAM_FUSE_SEARCHED : SPSLAM_FUSE_NO_CANDIDATES;
}

__global__ __launch_bounds__(kThreads) void fuse_search_kernel(const spslam_fuse_problem* __restrict__ problems,
                                                               const spslam_local_point* __restrict__ points,
                                                               int max_points, MatchCurrent C, MatchGeom g,
                                                               FuseConsts P, const uint8_t* __restrict__ skip,
                                                               spslam_fuse_result* __restrict__ results,
                                                               int* __restrict__ nfused) {
    const int f = blockIdx.x, sub = threadIdx.x & (kLGrp - 1);
    const int i = blockIdx.y * kFusePtsPerBlock + (int)(threadIdx.x / kLGrp);
    const spslam_fuse_problem& F = problems[f];
    const bool live = i < F.n_points && i < max_points;  // uniform over the point's lanes
    int status = SPSLAM_FUSE_SKIPPED, level = 0;
    uint32_t best = kNone;
    if (live && !(skip && skip[F.out_offset + i]))
        status = fuse_point(F, points[F.point_offset + i], C, g, P, sub, &level, &best);
    const int dist = best != kNone ? (int)(best >> 20) : 256;
    if (live && sub == 0) {
        spslam_fuse_result r;
        r.best_idx = best != kNone ? frame_view(C, F.kf_slot).GI[best & 0xfffff] : -1;
        r.best_dist = (int16_t)dist;
        r.level = (uint8_t)level;
        r.status = (uint8_t)status;
        results[F.out_offset + i] = r;
    }
    // nFused: the points with bestDist <= TH_LOW (:952), one atomic per wave that has any
    const int n = wave_sum(live && sub == 0 && dist <= kThLow);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&nfused[f], n);
}

// ---------------------------------------------------------------------------
// LoopClosing's Sim3 matchers: SearchBySim3 (src/ORBmatcher.cc:1102-1326), SearchByProjection(pKF, Scw, ...)
// (:290-403) and the search of Fuse(pKF, Scw, ...) (:977-1079).  One point per kLGrp lanes, as fuse_search_kernel;
// the three share the projection, the window and the candidate test below: KeyFrame::IsInImage / GetFeaturesInArea
// over the truncated bounds, the octave filter [level - 1, level], no chi-square test, no view of uright.  They are
// siblings of fuse_point and not a parameter of it: as a template parameter they moved fuse_search_kernel's
// registers (profiles/r15/disassembly.md).
struct Sim3Probe {
    float u, v, r;
    int level;
    uint4 d0, d1;
};

// keypoint k at CSR position j: the key, or kNone outside vIndices or the octave range; *in_area: it is in vIndices
__device__ __forceinline__ uint32_t sim3_candidate_key(const Sim3Probe& p, const FrameView& V, int j, int k,
                                                       bool* in_area) {
    const spslam_keypoint kp = V.kun[k];
    const float dx = __fsub_rn(kp.x, p.u), dy = __fsub_rn(kp.y, p.v);
    if (!(fabsf(dx) < p.r && fabsf(dy) < p.r)) return kNone;
    *in_area = true;
    if (kp.octave < p.level - 1 || kp.octave > p.level) return kNone;
    return ((uint32_t)hamming(p.d0, p.d1, V.desc + 32 * (size_t)k) << 20) | (uint32_t)j;
}

// The K smallest keys of the window over the cells x0 .. x1, y0 .. y1 (column-major, as GetFeaturesInArea scans
// them, dealt to the point's kLGrp lanes and merged), in every lane of the point; taken (may be null): one byte per
// keypoint, set ones are passed over.  Returns whether any keypoint, taken or not, is in vIndices.
template <int K>
__device__ __forceinline__ bool sim3_window_keys(const Sim3Probe& p, const FrameView& V, int x0, int x1, int y0, int y1,
                                                 const uint8_t* taken, int sub, uint32_t (&bk)[K]) {
#pragma unroll
    for (int q = 0; q < K; q++) bk[q] = kNone;
    bool any = false;
    const int nrows = y1 - y0 + 1, ncells = x1 >= x0 && nrows > 0 ? (x1 - x0 + 1) * nrows : 0;
    for (int cell = sub; cell < ncells; cell += kLGrp) {
        const int cx = cell / nrows, c = (x0 + cx) * kRows + y0 + (cell - cx * nrows);
        const int j0 = V.GO[c], j1 = V.GO[c + 1];
        for (int j = j0; j < j1; j++) {
            const int k = V.GI[j];
            const uint32_t key = sim3_candidate_key(p, V, j, k, &any);
            if (taken && taken[k]) continue;
            insk(bk, key);
        }
    }
    int anyi = any;
#pragma unroll
    for (int o = kLGrp / 2; o >= 1; o >>= 1) {
        uint32_t pk[K];
#pragma unroll
        for (int q = 0; q < K; q++) pk[q] = (uint32_t)__shfl_xor((int)bk[q], o);
#pragma unroll
        for (int q = 0; q < K; q++) insk(bk, pk[q]);
        anyi |= __shfl_xor(anyi, o);
    }
    return anyi != 0;
}

// cv::norm of a 3-vector: the squares summed in float, the root in double (local_window_kernel's reading)
__device__ __forceinline__ float norm3f(const float* a) {
    float sq = __fmul_rn(a[0], a[0]);
    sq = __fadd_rn(sq, __fmul_rn(a[1], a[1]));
    sq = __fadd_rn(sq, __fmul_rn(a[2], a[2]));
    return (float)__dsqrt_rn((double)sq);
}

// The camera-frame point Pc into the keyframe: SPSLAM_FUSE_BEHIND, SPSLAM_FUSE_OUTSIDE_IMAGE or SPSLAM_FUSE_SEARCHED
// with (u, v).  invz is 1/z in float (:331) or 1.0/z in double, rounded (:1019, :1166, :1246): the same bits, a
// quotient rounded to 53 bits and then to 24 being the correctly rounded float.  u = fx*x+cx with GCC's contraction
// (tests/test_loop_match_host.py).
__device__ __forceinline__ int sim3_project(const float* Pc, const MatchGeom& g, float* u, float* v) {
    if (Pc[2] < 0.0f) return SPSLAM_FUSE_BEHIND;
    const float invz = __fdiv_rn(1.0f, Pc[2]);
    const float x = __fmul_rn(Pc[0], invz), y = __fmul_rn(Pc[1], invz);
    *u = __fmaf_rn(g.fx, x, g.cx);
    *v = __fmaf_rn(g.fy, y, g.cy);
    // KeyFrame::IsInImage: half open (KeyFrame.cc:627-630); z == 0 makes u / v inf or NaN, which fail it
    if (!(*u >= g.min_x && *u < g.max_x && *v >= g.min_y && *v < g.max_y)) return SPSLAM_FUSE_OUTSIDE_IMAGE;
    return SPSLAM_FUSE_SEARCHED;
}

__device__ __forceinline__ bool sim3_in_range(const spslam_local_point& p, float dist) {
    const float maxD = __fmul_rn(1.2f, p.max_dist), minD = __fmul_rn(0.8f, p.min_dist);
    return !(dist < minD || dist > maxD);
}

// PredictScale, the radius and GetFeaturesInArea's cell range; false: the reference's vIndices is empty
__device__ __forceinline__ bool sim3_window(const spslam_local_point& p, float dist, float u, float v, const MatchGeom& g,
                                            const FuseConsts& P, Sim3Probe* q, int* x0, int* x1, int* y0, int* y1) {
    const int level = predict_scale(p.max_dist, dist, P.log_scale_factor, P.n_levels);
    *q = Sim3Probe{u, v, __fmul_rn(P.th, level_entry(g.scale, level)), level, *(const uint4*)p.desc,
                   *(const uint4*)(p.desc + 16)};
    return cell_range(u, v, q->r, g, x0, x1, y0, y1);
}

// The decomposition of Scw (:298-303, :985-990) into the rows [Rcw | tcw] of T: scw = sqrt(sRcw.row(0).dot(sRcw.row(0)))
// with Mat::dot summed in double and the root rounded to the float scw; Rcw = sRcw / scw and tcw = col3 / scw as
// OpenCV's Mat / double, a scale by 1.0 / scw: the product with the double reciprocal, rounded once.
__device__ __forceinline__ void sim3_decompose(const float* S, float* T) {
    double d = __dmul_rn((double)S[0], (double)S[0]);
    d = __dadd_rn(d, __dmul_rn((double)S[1], (double)S[1]));
    d = __dadd_rn(d, __dmul_rn((double)S[2], (double)S[2]));
    const float scw = (float)__dsqrt_rn(d);
    const double inv = __ddiv_rn(1.0, (double)scw);
#pragma unroll
    for (int q = 0; q < 12; q++) T[q] = (float)__dmul_rn((double)S[q], inv);
}

// One point of SearchByProjection(pKF, Scw, ...) / Fuse(pKF, Scw, ...) up to its window (:312-362, :1000-1051, the
// same statements): SPSLAM_FUSE_SEARCHED with the probe and the cell range, or the status of the test that ended it.
// Ow = -Rcw.t()*tcw as fuse_point makes it.
__device__ __forceinline__ int scw_window(const float* Scw, const spslam_local_point& p, const MatchGeom& g,
                                          const FuseConsts& P, Sim3Probe* q, int* x0, int* x1, int* y0, int* y1) {
    float T[12];
    sim3_decompose(Scw, T);
    const float tcw[3] = {T[3], T[7], T[11]};
    float Pc[3], Ow[3], u, v;
    mat3_mul(T, p.xw, tcw, false, 1.0, Pc);  // Rcw*p3Dw+tcw
    q->level = 0;
    const int st = sim3_project(Pc, g, &u, &v);
    if (st != SPSLAM_FUSE_SEARCHED) return st;
    mat3_mul(T, tcw, nullptr, true, -1.0, Ow);
    const float PO[3] = {__fsub_rn(p.xw[0], Ow[0]), __fsub_rn(p.xw[1], Ow[1]), __fsub_rn(p.xw[2], Ow[2])};
    const float dist = norm3f(PO);
    if (!sim3_in_range(p, dist)) return SPSLAM_FUSE_OUT_OF_RANGE;
    double dot = __dmul_rn((double)PO[0], (double)p.normal[0]);
    dot = __dadd_rn(dot, __dmul_rn((double)PO[1], (double)p.normal[1]));
    dot = __dadd_rn(dot, __dmul_rn((double)PO[2], (double)p.normal[2]));
    if (dot < __dmul_rn(0.5, (double)dist)) return SPSLAM_FUSE_VIEW_ANGLE;  // doubles, no division
    return sim3_window(p, dist, u, v, g, P, q, x0, x1, y0, y1) ? SPSLAM_FUSE_SEARCHED : SPSLAM_FUSE_NO_CANDIDATES;
}

// The search of Fuse(pKF, Scw, vpPoints, th, vpReplacePoint): fuse_search_kernel's records; the problem's Tcw field
// holds Scw.  The walk :1082-1096 stays with the caller.
__global__ __launch_bounds__(kThreads) void fuse_sim3_search_kernel(const spslam_fuse_problem* __restrict__ problems,
                                                                    const spslam_local_point* __restrict__ points,
                                                                    int max_points, MatchCurrent C, MatchGeom g,
                                                                    FuseConsts P, const uint8_t* __restrict__ skip,
                                                                    spslam_fuse_result* __restrict__ results,
                                                                    int* __restrict__ nfused) {
    const int f = blockIdx.x, sub = threadIdx.x & (kLGrp - 1);
    const int i = blockIdx.y * kFusePtsPerBlock + (int)(threadIdx.x / kLGrp);
    const spslam_fuse_problem& F = problems[f];
    const bool live = i < F.n_points && i < max_points;  // uniform over the point's lanes
    int status = SPSLAM_FUSE_SKIPPED, level = 0;
    uint32_t bk[1] = {kNone};
    const FrameView V = frame_view(C, F.kf_slot);
    if (live && !(skip && skip[F.out_offset + i])) {
        Sim3Probe q;
        int x0, x1, y0, y1;
        status = scw_window(F.Tcw, points[F.point_offset + i], g, P, &q, &x0, &x1, &y0, &y1);
        level = q.level;
        if (status == SPSLAM_FUSE_SEARCHED && !sim3_window_keys(q, V, x0, x1, y0, y1, nullptr, sub, bk))
            status = SPSLAM_FUSE_NO_CANDIDATES;
    }
    const uint32_t best = bk[0];
    const int dist = best != kNone ? (int)(best >> 20) : 256;
    if (live && sub == 0) {
        spslam_fuse_result r;
        r.best_idx = best != kNone ? V.GI[best & 0xfffff] : -1;
        r.best_dist = (int16_t)dist;
        r.level = (uint8_t)level;
        r.status = (uint8_t)status;
        results[F.out_offset + i] = r;
    }
    const int n = wave_sum(live && sub == 0 && dist <= kThLow);  // nFused (:1082, :1095)
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&nfused[f], n);
}

// SearchByProjection(pKF, Scw, vpPoints, vpMatched, th), the window kernel: per point the kSim3Keys smallest keys
// among the keypoints that pass the octave filter and are not taken on entry, with the window for a re-scan.
__global__ __launch_bounds__(kThreads) void proj_sim3_window_kernel(const spslam_fuse_problem* __restrict__ problems,
                                                                    const spslam_local_point* __restrict__ points,
                                                                    int max_points, MatchCurrent C, MatchGeom g,
                                                                    FuseConsts P, const uint8_t* __restrict__ skip,
                                                                    const uint8_t* __restrict__ taken_in,
                                                                    Sim3Window* __restrict__ win) {
    const int f = blockIdx.x, sub = threadIdx.x & (kLGrp - 1);
    const int i = blockIdx.y * kFusePtsPerBlock + (int)(threadIdx.x / kLGrp);
    const spslam_fuse_problem& F = problems[f];
    if (i >= F.n_points || i >= max_points) return;  // uniform over the point's lanes
    Sim3Window w{};
#pragma unroll
    for (int q = 0; q < kSim3Keys; q++) {
        w.best[q] = kNone;
        w.kp[q] = -1;
    }
    w.x0 = 1;  // an empty range
    if (!(skip && skip[F.out_offset + i])) {
        Sim3Probe q;
        int x0, x1, y0, y1;
        if (scw_window(F.Tcw, points[F.point_offset + i], g, P, &q, &x0, &x1, &y0, &y1) == SPSLAM_FUSE_SEARCHED) {
            const FrameView V = frame_view(C, F.kf_slot);
            uint32_t bk[kSim3Keys];
            sim3_window_keys(q, V, x0, x1, y0, y1, taken_in ? taken_in + (size_t)f * C.cap : nullptr, sub, bk);
            w.u = q.u; w.v = q.v; w.r = q.r;
            w.level = (int8_t)q.level;
            w.valid = 1;
            w.x0 = (int16_t)x0; w.x1 = (int16_t)x1; w.y0 = (int16_t)y0; w.y1 = (int16_t)y1;
#pragma unroll
            for (int k = 0; k < kSim3Keys; k++) {
                w.best[k] = bk[k];
                if (bk[k] != kNone) w.kp[k] = V.GI[bk[k] & 0xfffff];
            }
        }
    }
    if (sub == 0) win[(size_t)f * max_points + i] = w;
}

// ... and its in-order walk, one wave per problem (:312-400): point i takes the best of its keypoints still free, if
// that distance is <= TH_LOW.  The lanes hold 64 consecutive points; in passes, every point not yet decided picks the
// first of its keys that is free, the accepting ones claim their keypoint (LDS atomicMin of the lane), and the points
// before the first one that lost a claim, or whose keys are all taken, are committed together.  A loser starts the
// next pass (its key is taken by then); a point out of keys is re-scanned by the whole wave, and only when its last
// key could still be accepted: the keys ascend, so past a distance above TH_LOW nothing can.
__global__ __launch_bounds__(64) void proj_sim3_assign_kernel(const spslam_fuse_problem* __restrict__ problems,
                                                              const spslam_local_point* __restrict__ points,
                                                              int max_points, MatchCurrent C,
                                                              const uint8_t* __restrict__ taken_in,
                                                              const Sim3Window* __restrict__ win,
                                                              int32_t* __restrict__ match, int* __restrict__ nmatches) {
    extern __shared__ uint32_t taken[];  // [ceil(cap / 32)], then claim[cap]
    const int f = blockIdx.x, lane = threadIdx.x;
    const spslam_fuse_problem& F = problems[f];
    const int n_kp = min(C.counts[F.kf_slot], C.cap), np = min(F.n_points, max_points);
    int32_t* M = match + (size_t)f * C.cap;
    const int words = (C.cap + 31) / 32;
    uint32_t* claim = taken + words;
    const uint8_t* tk = taken_in ? taken_in + (size_t)f * C.cap : nullptr;
    for (int k = lane; k < n_kp; k += 64) {
        claim[k] = ~0u;
        M[k] = -1;
    }
    for (int wd = lane; wd < words; wd += 64) {
        uint32_t bits = 0u;
        if (tk)
            for (int b = 0; b < 32; b++) {
                const int k = 32 * wd + b;
                if (k < n_kp && tk[k]) bits |= 1u << b;
            }
        taken[wd] = bits;
    }
    __syncthreads();
    const Sim3Window* Wf = win + (size_t)f * max_points;
    const FrameView V = frame_view(C, F.kf_slot);
    const spslam_local_point* Pp = points + F.point_offset;
    int nm = 0;
    for (int c0 = 0; c0 < np; c0 += 64) {
        const int i = c0 + lane, m = min(64, np - c0);
        uint32_t best[kSim3Keys];
        int b[kSim3Keys];
#pragma unroll
        for (int q = 0; q < kSim3Keys; q++) {
            best[q] = kNone;
            b[q] = -1;
        }
        if (i < np) {
            const Sim3Window w = Wf[i];
#pragma unroll
            for (int q = 0; q < kSim3Keys; q++) {
                best[q] = w.valid ? w.best[q] : kNone;
                b[q] = best[q] != kNone ? w.kp[q] : -1;
            }
        }
        int start = 0;
        while (start < m) {
            const bool act = lane >= start && lane < m;
            uint32_t k1 = kNone;
            int b1 = -1;
            if (act) {
#pragma unroll
                for (int q = kSim3Keys - 1; q >= 0; q--)
                    if (best[q] != kNone && !bit_test(taken, b[q])) { k1 = best[q]; b1 = b[q]; }
            }
            // out of keys: all kSim3Keys were there, all are taken, and the last could still have been accepted
            const bool out = act && k1 == kNone && best[kSim3Keys - 1] != kNone &&
                             (int)(best[kSim3Keys - 1] >> 20) <= kThLow;
            const bool acc = act && k1 != kNone && (int)(k1 >> 20) <= kThLow;  // :394
            if (acc) atomicMin(&claim[b1], (uint32_t)lane);
            wave_sync();
            const bool lost = acc && claim[b1] < (uint32_t)lane;
            wave_sync();
            if (acc) claim[b1] = ~0u;
            const unsigned long long sm = __ballot(out || lost);
            const int first = sm ? __ffsll((long long)sm) - 1 : m;
            const bool commit = acc && lane < first;
            if (commit) {
                M[b1] = c0 + lane;  // vpMatched[bestIdx] = pMP (:396)
                bit_set_atomic(taken, b1);
            }
            nm += __popcll(__ballot(commit));
            wave_sync();
            if (first >= m) break;
            start = first;
            if (!__shfl((int)out, first)) continue;  // lost a claim: decided by the next pass
            start = first + 1;
            const Sim3Window w = Wf[c0 + first];
            const uint8_t* d = Pp[c0 + first].desc;
            const Sim3Probe q{w.u, w.v, w.r, w.level, *(const uint4*)d, *(const uint4*)(d + 16)};
            uint32_t k = kNone;
            bool any = false;
            for (int ix = w.x0; ix <= w.x1; ix++)
                for (int iy = w.y0; iy <= w.y1; iy++) {
                    const int c = ix * kRows + iy;
                    for (int j = V.GO[c] + lane; j < V.GO[c + 1]; j += 64) {
                        const int kk = V.GI[j];
                        if (bit_test(taken, kk)) continue;
                        k = min(k, sim3_candidate_key(q, V, j, kk, &any));
                    }
                }
            k = wave_min(k);
            if (k == kNone || (int)(k >> 20) > kThLow) continue;
            if (lane == 0) {
                const int kk = V.GI[k & 0xfffff];
                M[kk] = c0 + first;
                bit_set(taken, kk);
            }
            nm++;
            wave_sync();
        }
    }
    if (lane == 0) nmatches[f] = nm;
}

// SearchBySim3, the two searches (:1148-1305) in one launch: blockIdx.z = 0 sends KF1's map points into KF2 by
// sR21 / t21 (vnMatch1), 1 sends KF2's into KF1 by sR12 / t12 (vnMatch2).  sR12 = s12*R12 (a float product in
// double, rounded: the float product), sR21 = (1.0/s12)*R12.t() (the double reciprocal times the element, rounded
// once) and t21 = -sR21*t12 (rows summed in double, negated, rounded) are made here.  The distance
// is cv::norm of the camera-frame point; no view-angle test.  A point is passed over without a map point, with a
// bad one, or (side 1) already matched on entry; side 2's vbAlreadyMatched2 is applied by the agreement pass,
// which is all that reads vnMatch2.  vn at pair * 2 * cap: vnMatch1, then vnMatch2.
__global__ __launch_bounds__(kThreads) void sim3_search_kernel(const spslam_sim3_pair* __restrict__ pairs,
                                                               spslam_sim3_map map, MatchCurrent C, MatchGeom g,
                                                               FuseConsts P, const int32_t* __restrict__ match12,
                                                               int32_t* __restrict__ vn) {
    const int p = blockIdx.x, side = blockIdx.z, sub = threadIdx.x & (kLGrp - 1);
    const int i = blockIdx.y * kFusePtsPerBlock + (int)(threadIdx.x / kLGrp);
    const spslam_sim3_pair& S = pairs[p];
    const int kf_from = side ? S.kf2 : S.kf1, kf_to = side ? S.kf1 : S.kf2;
    const int slot_from = map.kf_slot[kf_from], slot_to = map.kf_slot[kf_to];
    const int n_from = min(min(C.counts[slot_from], C.cap), map.match_off[kf_from + 1] - map.match_off[kf_from]);
    if (i >= n_from) return;  // uniform over the point's lanes
    uint32_t bk[1] = {kNone};
    const FrameView V = frame_view(C, slot_to);
    const int row = map.match_row[map.match_off[kf_from] + i];
    do {
        if (row < 0 || (map.point_bad && map.point_bad[row])) break;       // :1152-1156
        if (side == 0 && match12[S.match_offset + i] >= 0) break;         // vbAlreadyMatched1
        const spslam_local_point& pt = map.points[row];
        // the transform between the cameras, rows [sR | t] at stride 4
        float A[12];
        if (side == 0) {
            const double inv = __ddiv_rn(1.0, (double)S.s12);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) A[4 * r + c] = (float)__dmul_rn((double)S.R12[3 * c + r], inv);
            float t21[3];
            mat3_mul(A, S.t12, nullptr, false, -1.0, t21);
            A[3] = t21[0]; A[7] = t21[1]; A[11] = t21[2];
        } else {
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) A[4 * r + c] = __fmul_rn(S.s12, S.R12[3 * r + c]);
                A[4 * r + 3] = S.t12[r];
            }
        }
        const float* Tw = map.kf_Tcw + 16 * (size_t)kf_from;
        const float tw[3] = {Tw[3], Tw[7], Tw[11]}, ta[3] = {A[3], A[7], A[11]};
        float Pa[3], Pb[3], u, v;
        mat3_mul(Tw, pt.xw, tw, false, 1.0, Pa);   // R1w*p3Dw + t1w
        mat3_mul(A, Pa, ta, false, 1.0, Pb);       // sR21*p3Dc1 + t21
        if (sim3_project(Pb, g, &u, &v) != SPSLAM_FUSE_SEARCHED) break;
        const float dist = norm3f(Pb);
        if (!sim3_in_range(pt, dist)) break;
        Sim3Probe q;
        int x0, x1, y0, y1;
        if (!sim3_window(pt, dist, u, v, g, P, &q, &x0, &x1, &y0, &y1)) break;
        sim3_window_keys(q, V, x0, x1, y0, y1, nullptr, sub, bk);
    } while (false);
    if (sub == 0) {
        const uint32_t best = bk[0];
        const bool ok = best != kNone && (int)(best >> 20) <= kThHigh;     // :1221
        vn[((size_t)p * 2 + side) * C.cap + i] = ok ? V.GI[best & 0xfffff] : -1;
    }
}

// ... and the agreement pass (:1307-1323), one workgroup per pair: vbAlreadyMatched2 from match12 as it came in (or
// the caller's override), then match12[i1] = idx2 where vnMatch1[i1] = idx2 and vnMatch2[idx2] = i1 with idx2 not
// already matched.  flags: cap bytes per pair.
__global__ __launch_bounds__(kThreads) void sim3_agree_kernel(const spslam_sim3_pair* __restrict__ pairs,
                                                              spslam_sim3_map map, MatchCurrent C,
                                                              const uint8_t* __restrict__ already2,
                                                              const int32_t* __restrict__ vn,
                                                              uint8_t* __restrict__ flags, int32_t* __restrict__ match12,
                                                              int* __restrict__ n_found) {
    __shared__ int found;
    const int p = blockIdx.x, t = threadIdx.x;
    const spslam_sim3_pair& S = pairs[p];
    const int n1 = min(min(C.counts[map.kf_slot[S.kf1]], C.cap), map.match_off[S.kf1 + 1] - map.match_off[S.kf1]);
    const int n2 = min(min(C.counts[map.kf_slot[S.kf2]], C.cap), map.match_off[S.kf2 + 1] - map.match_off[S.kf2]);
    const int32_t* vn1 = vn + (size_t)p * 2 * C.cap;
    const int32_t* vn2 = vn1 + C.cap;
    uint8_t* fl = flags + (size_t)p * C.cap;
    int32_t* M = match12 + S.match_offset;
    if (t == 0) found = 0;
    for (int k = t; k < n2; k += kThreads) fl[k] = already2 ? already2[(size_t)p * C.cap + k] : 0;
    __syncthreads();
    if (!already2)
        for (int i = t; i < n1; i += kThreads) {
            const int idx2 = M[i];
            if (idx2 >= 0 && idx2 < n2) fl[idx2] = 1;                      // :1138-1140
        }
    __syncthreads();
    int n = 0;
    for (int i = t; i < n1; i += kThreads) {
        const int idx2 = vn1[i];
        if (idx2 >= 0 && idx2 < n2 && !fl[idx2] && vn2[idx2] == i) {
            M[i] = idx2;
            n++;
        }
    }
    if (n) atomicAdd(&found, n);
    __syncthreads();
    if (t == 0) n_found[S.result_offset] = found;
}

}  // namespace match

// Dynamic LDS beyond the default 64 KB needs the per-kernel opt-in: both instantiations (K keys per point) of a walk.
static hipError_t lds_opt_in(const void* small_batch_kernel, const void* few_keys_kernel, int bytes) {
    const hipError_t a = hipFuncSetAttribute(small_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return a != hipSuccess ? a : hipFuncSetAttribute(few_keys_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

hipError_t local_match_launch(int n_frames, const spslam_local_frame* frames, const spslam_local_point* points,
                              int max_points, const MatchCurrent& cur, const MatchGeom& g, const LocalConsts& P,
                              const uint8_t* taken_in, LocalWindow* win, int32_t* match, int* nmatches,
                              uint8_t* in_view, hipStream_t s, KernelTimer* timer) {
    // taken bits + the claim table in dynamic LDS (opted in up to 160 KB: caps up to ~39K keypoints)
    const size_t lds = (size_t)((cur.cap + 31) / 32) * 4 + (size_t)cur.cap * 4;
    if (n_frames < 1 || max_points < 0 || cur.cap < 1 || lds > 160 * 1024) return hipErrorInvalidValue;
    static const hipError_t lds_attr = lds_opt_in((const void*)match::local_assign_kernel<kLocalKeys>,
                                                  (const void*)match::local_assign_kernel<kFewKeys>, 160 * 1024);
    if (lds_attr != hipSuccess) return lds_attr;
    if (timer) timer->begin(kKindLocalMatch, s);
    auto run = [&](auto* w) {
        constexpr int K = sizeof(w->best) / sizeof(w->best[0]);
        if (max_points > 0)
            hipLaunchKernelGGL(match::local_window_kernel<K>,
                               dim3(n_frames, (max_points + match::kLPtsPerBlock - 1) / match::kLPtsPerBlock),
                               dim3(match::kThreads), 0, s, frames, points, max_points, cur, g, P, taken_in, w, in_view);
        hipLaunchKernelGGL(match::local_assign_kernel<K>, dim3(n_frames), dim3(64), lds, s,
                           frames, points, max_points, cur, g, P, taken_in, w, match, nmatches);
    };
    if (n_frames <= kSmallBatchKeys) run(win);
    else run(reinterpret_cast<LocalWindowK<kFewKeys>*>(win));
    if (timer) timer->end(kKindLocalMatch, s);
    return hipGetLastError();
}

hipError_t fuse_search_launch(int n_problems, const spslam_fuse_problem* problems, const spslam_local_point* points,
                              int max_points, const MatchCurrent& cur, const MatchGeom& g, const FuseConsts& P,
                              const uint8_t* skip, spslam_fuse_result* results, int* nfused, hipStream_t s) {
    if (n_problems < 1 || max_points < 0 || cur.cap < 1) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(nfused, 0, (size_t)n_problems * sizeof(int), s);
    if (e != hipSuccess) return e;
    if (max_points > 0)
        hipLaunchKernelGGL(match::fuse_search_kernel,
                           dim3(n_problems, (max_points + match::kFusePtsPerBlock - 1) / match::kFusePtsPerBlock),
                           dim3(match::kThreads), 0, s, problems, points, max_points, cur, g, P, skip, results, nfused);
    return hipGetLastError();
}

hipError_t fuse_sim3_search_launch(int n_problems, const spslam_fuse_problem* problems,
                                   const spslam_local_point* points, int max_points, const MatchCurrent& cur,
                                   const MatchGeom& g, const FuseConsts& P, const uint8_t* skip,
                                   spslam_fuse_result* results, int* nfused, hipStream_t s) {
    if (n_problems < 1 || max_points < 0 || cur.cap < 1) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(nfused, 0, (size_t)n_problems * sizeof(int), s);
    if (e != hipSuccess) return e;
    if (max_points > 0)
        hipLaunchKernelGGL(match::fuse_sim3_search_kernel,
                           dim3(n_problems, (max_points + match::kFusePtsPerBlock - 1) / match::kFusePtsPerBlock),
                           dim3(match::kThreads), 0, s, problems, points, max_points, cur, g, P, skip, results, nfused);
    return hipGetLastError();
}

hipError_t proj_sim3_launch(int n_problems, const spslam_fuse_problem* problems, const spslam_local_point* points,
                            int max_points, const MatchCurrent& cur, const MatchGeom& g, const FuseConsts& P,
                            const uint8_t* skip, const uint8_t* taken_in, Sim3Window* win, int32_t* match,
                            int* nmatches, hipStream_t s) {
    // taken bits + the claim table in dynamic LDS (opted in up to 150 KB: caps up to ~36K keypoints)
    const size_t lds = (size_t)((cur.cap + 31) / 32) * 4 + (size_t)cur.cap * 4;
    if (n_problems < 1 || max_points < 0 || cur.cap < 1 || lds > 150 * 1024) return hipErrorInvalidValue;
    static const hipError_t lds_attr = hipFuncSetAttribute((const void*)match::proj_sim3_assign_kernel,
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (lds_attr != hipSuccess) return lds_attr;
    if (max_points > 0)
        hipLaunchKernelGGL(match::proj_sim3_window_kernel,
                           dim3(n_problems, (max_points + match::kFusePtsPerBlock - 1) / match::kFusePtsPerBlock),
                           dim3(match::kThreads), 0, s, problems, points, max_points, cur, g, P, skip, taken_in, win);
    hipLaunchKernelGGL(match::proj_sim3_assign_kernel, dim3(n_problems), dim3(64), lds, s, problems, points,
                       max_points, cur, taken_in, win, match, nmatches);
    return hipGetLastError();
}

hipError_t sim3_search_launch(int n_pairs, const spslam_sim3_pair* pairs, const spslam_sim3_map& map,
                              const MatchCurrent& cur, const MatchGeom& g, const FuseConsts& P,
                              const uint8_t* already2, int32_t* vn, uint8_t* flags, int32_t* match12, int* n_found,
                              hipStream_t s) {
    if (n_pairs < 1 || cur.cap < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(match::sim3_search_kernel,
                       dim3(n_pairs, (cur.cap + match::kFusePtsPerBlock - 1) / match::kFusePtsPerBlock, 2),
                       dim3(match::kThreads), 0, s, pairs, map, cur, g, P, match12, vn);
    hipLaunchKernelGGL(match::sim3_agree_kernel, dim3(n_pairs), dim3(match::kThreads), 0, s, pairs, map, cur,
                       already2, vn, flags, match12, n_found);
    return hipGetLastError();
}

hipError_t match_launch(int n_frames, const spslam_proj_frame* frames, const spslam_proj_point* points,
                        int max_points, const MatchCurrent& cur, const MatchGeom& g, const spslam_match_params& P,
                        MatchWindow* win, int2* pushes, int32_t* match, int* nmatches, hipStream_t s,
                        KernelTimer* timer) {
    // taken bits + the claim table in dynamic LDS (opted in up to 150 KB: caps up to ~36K keypoints)
    const size_t lds = (size_t)((cur.cap + 31) / 32) * 4 + (size_t)cur.cap * 4;
    if (n_frames < 1 || max_points < 0 || cur.cap < 1 || lds > 150 * 1024) return hipErrorInvalidValue;
    static const hipError_t lds_attr = lds_opt_in((const void*)match::match_assign_kernel<kProjKeys>,
                                                  (const void*)match::match_assign_kernel<kFewKeys>, 150 * 1024);
    if (lds_attr != hipSuccess) return lds_attr;
    if (timer) timer->begin(kKindMatch, s);
    const int passes = P.retry_below > 0 ? 2 : 1;
    auto run = [&](auto* w) {
        constexpr int K = sizeof(w->best) / sizeof(w->best[0]);
        for (int pass = 0; pass < passes; pass++) {
            if (max_points > 0)
                hipLaunchKernelGGL(match::match_window_kernel<K>,
                                   dim3(n_frames, (max_points + match::kPtsPerBlock - 1) / match::kPtsPerBlock),
                                   dim3(match::kThreads), 0, s, frames, points, max_points, cur, g, P.th, P.mono,
                                   P.retry_below, pass, nmatches, w);
            hipLaunchKernelGGL(match::match_assign_kernel<K>, dim3(n_frames), dim3(64), lds, s, frames, points,
                               max_points, cur, g, P.check_orientation, P.retry_below, pass, w, pushes, match, nmatches);
        }
    };
    if (n_frames <= kSmallBatchKeys) run(win);
    else run(reinterpret_cast<MatchWindowK<kFewKeys>*>(win));
    if (timer) timer->end(kKindMatch, s);
    return hipGetLastError();
}

}  // namespace spslam
