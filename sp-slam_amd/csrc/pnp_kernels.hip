// PnPsolver on gfx950 (src/PnPsolver.cc as Tracking::Relocalization drives it, src/Tracking.cc:1623-1675): the
// constructor, iterate with Refine, and the outputs Relocalization reads.  Semantics: tests/pnp_ref.cpp (DESIGN.md
// 3.20); the arithmetic is pnp_math.h, shared with a host build.
//
//   pnp_gather_kernel      the constructor (:67-110), one workgroup per problem: the frame's keypoints in chunks of
//                          256, kept ones compacted in order (ballot within a wave, the waves' counts prefixed
//                          through LDS), each kept one's mvP3Dw, mvP2D, mvMaxError, index and point row written to
//                          the problem's scratch with N.
//   pnp_hypothesis_kernel  one wave per (problem, 64 iterations), one lane per iteration of the call's range: the
//                          draws, the 4-point EPnP and CheckInliers over the N correspondences, which every lane
//                          reads at the same address.  EPnP's matrices (the 12 x 12 MtM that becomes Ut, and the
//                          small systems) are indexed at run time and live in the lane's private memory.
//   pnp_select_kernel      one wave per problem: Refine for the masks the sequential loop would try, 64 at a time,
//                          one lane each; the iteration at which the loop returns; the result record, the state
//                          out, vbInliers and, when asked, the frame's map points.
//
// Selection.  The reference's loop (:182-239), with min = mRansacMinInliers and the running best B (mnBestInliers,
// best_in on entry): at every k with n_k >= min it first replaces the best mask when n_k > B (k is a *record
// setter*), then calls Refine, which reads the best mask and nothing else of the iteration (:260-271), and returns
// when Refine counts more than min inliers.
// (a) Refine is a function of the best mask alone.  Between two record setters the mask does not change, so every
//     qualifying k (n_k >= min) of such a stretch gets the same answer: if the first fails, all fail.
// (b) The mask in force at a qualifying k is that of the latest record setter at or before k, or the mask carried
//     in when there is none.  A record setter qualifies by definition.
// (c) So the loop's outcome is decided by one Refine per *candidate*: the first qualifying k of the call when it is
//     no record setter (mask carried in), then every record setter in order.  The loop returns at the first
//     candidate whose Refine succeeds, at that candidate's own k (it is the first k its mask governs).
// (d) B before k is max(best_in, n_j for qualifying j < k), a prefix maximum: the record setters are known once the
//     n_k are, without any Refine.  pnp_math.h's next_candidate walks them; tests/test_pnp_host.py holds it
//     against a literal trace of the loop on random sequences.
// State out: iterations_done = k + 1 of the returning candidate, else the end of the range; best_inliers, the best
// mask and best_Tcw are those of the latest record setter at or before that point, else what was carried in.
#include <hip/hip_runtime.h>

#include "orb_match_device.h"
#include "pnp_launch.h"
#include "pnp_math.h"

namespace spslam {
namespace pnp {

using orb_match::level_entry;

constexpr int kThreads = 256, kWaves = kThreads / 64, kLanes = 64;

struct Header { int32_t n, pad[3]; };

__device__ __forceinline__ size_t problem_bytes(int cap, int max_its) {
    return sizeof(Header) + (size_t)cap * sizeof(Corr) + (size_t)max_its * sizeof(Hyp);
}
__device__ __forceinline__ Header* header_of(uint8_t* scratch, int p, int cap, int max_its) {
    return (Header*)(scratch + (size_t)p * problem_bytes(cap, max_its));
}
__device__ __forceinline__ Corr* corr_of(Header* h) { return (Corr*)(h + 1); }
__device__ __forceinline__ Hyp* hyp_of(Header* h, int cap) { return (Hyp*)((uint8_t*)(h + 1) + (size_t)cap * sizeof(Corr)); }

__device__ __forceinline__ int frame_n(const int* counts, int cap, int slot) { return max(min(counts[slot], cap), 0); }

__device__ __forceinline__ Cam cam_of(const PnpConsts& P) { return Cam{(double)P.fx, (double)P.fy, (double)P.cx, (double)P.cy}; }

__device__ __forceinline__ int range_of(const spslam_pnp_problem& Q, const PnpConsts& P, const int32_t* max_its,
                                        const int32_t* min_n, int n, int* n_run, bool* cut, int* min_inliers) {
    *min_inliers = min_n[n];
    return call_range(Q.iterations_done, Q.n_iterations, Q.rand_iterations, n, *min_inliers, max(max_its[n], 0),
                      P.max_iterations, n_run, cut);
}

__global__ __launch_bounds__(kThreads) void pnp_gather_kernel(const spslam_pnp_problem* __restrict__ problems,
                                                              spslam_sim3_map map,
                                                              const spslam_keypoint* __restrict__ kun,
                                                              const int* __restrict__ counts, int cap,
                                                              const int32_t* __restrict__ match, PnpConsts P,
                                                              uint8_t* __restrict__ scratch) {
    __shared__ int wave_n[kWaves];
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const spslam_pnp_problem Q = problems[p];
    const int nf = frame_n(counts, cap, Q.frame_slot);
    const int row0 = map.match_off[Q.kf], n_kf = map.match_off[Q.kf + 1] - row0;
    const size_t s = (size_t)Q.frame_slot * cap;
    Header* H = header_of(scratch, p, cap, P.max_iterations);
    Corr* out = corr_of(H);
    int base = 0;
    for (int c0 = 0; c0 < nf; c0 += kThreads) {
        const int i = c0 + t;
        int row = -1;
        if (i < nf) {
            const int m = match[Q.match_offset + i];
            if (m >= 0 && m < n_kf) row = map.match_row[row0 + m];   // vpMapPointMatches[i]
        }
        bool keep = row >= 0;
        if (keep && map.point_bad) keep = !map.point_bad[row];       // :85
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_n[wave] = __popcll(m);
        __syncthreads();
        int before = base, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            before += w < wave ? wave_n[w] : 0;
            total += wave_n[w];
        }
        if (keep) {
            const spslam_keypoint kp = kun[s + i];
            Corr c;
            c.xw[0] = map.points[row].xw[0]; c.xw[1] = map.points[row].xw[1]; c.xw[2] = map.points[row].xw[2];
            c.uv[0] = kp.x; c.uv[1] = kp.y;
            c.max_error = level_entry(P.max_error, kp.octave);
            c.index = i;
            c.row = row;
            out[before + __popcll(m & ((1ull << lane) - 1ull))] = c;
        }
        base += total;
        __syncthreads();  // wave_n is rewritten by the next chunk
    }
    if (t == 0) {
        H->n = base;
        H->pad[0] = H->pad[1] = H->pad[2] = 0;
    }
}

__global__ __launch_bounds__(kLanes) void pnp_hypothesis_kernel(const spslam_pnp_problem* __restrict__ problems,
                                                                int cap, const int32_t* __restrict__ rnd,
                                                                const int32_t* __restrict__ max_its,
                                                                const int32_t* __restrict__ min_n, PnpConsts P,
                                                                uint8_t* __restrict__ scratch) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const spslam_pnp_problem Q = problems[p];
    Header* H = header_of(scratch, p, cap, P.max_iterations);
    const int n = H->n;
    int n_run, min_inliers;
    bool cut;
    const int first = range_of(Q, P, max_its, min_n, n, &n_run, &cut, &min_inliers);
    const int j = blockIdx.y * kLanes + lane;
    if (j >= n_run) return;   // n_run <= P.max_iterations: inside the hypothesis records; n >= min_inliers >= 4
    const int k = first + j;  // < rand_iterations: inside the draws
    const Corr* C = corr_of(H);
    int idx[4];
    draw4(rnd + Q.rand_offset + 4 * (size_t)k, P.rand_max, n, idx);
    Src4 src;
#pragma unroll
    for (int i = 0; i < 4; i++) src.set(i, C[idx[i]]);
    const Cam cam = cam_of(P);
    Hyp h;
    int singular = 0;
    h.which = compute_pose(src, 4, cam, h.R, h.t, &singular);
    int count = 0;
    for (int i = 0; i < n; i++) count += check_inlier(C[i], h.R, h.t, cam) ? 1 : 0;
    h.n = count;
    hyp_of(H, cap)[j] = h;
}

__global__ __launch_bounds__(kLanes) void pnp_select_kernel(const spslam_pnp_problem* __restrict__ problems,
                                                            spslam_sim3_map map, const int* __restrict__ counts,
                                                            int cap, const int32_t* __restrict__ match,
                                                            const int32_t* __restrict__ max_its,
                                                            const int32_t* __restrict__ min_n, PnpConsts P,
                                                            uint8_t* __restrict__ scratch,
                                                            spslam_pnp_result* __restrict__ results,
                                                            uint8_t* __restrict__ inliers,
                                                            uint8_t* __restrict__ best_mask,
                                                            int32_t* __restrict__ frame_points) {
    __shared__ Hyp ref[kLanes];
    __shared__ int cand_j[kLanes];
    __shared__ int cand_carried[kLanes];
    __shared__ int s_ncand, s_ret, s_setter;
    const int p = blockIdx.x, t = threadIdx.x;
    const spslam_pnp_problem Q = problems[p];
    Header* H = header_of(scratch, p, cap, P.max_iterations);
    const Corr* C = corr_of(H);
    const Hyp* hyp = hyp_of(H, cap);
    const int n = H->n, nf = frame_n(counts, cap, Q.frame_slot);
    int n_run, min_inliers;
    bool cut;
    const int first = range_of(Q, P, max_its, min_n, n, &n_run, &cut, &min_inliers);
    const Cam cam = cam_of(P);
    uint8_t* in = inliers + Q.inlier_offset;
    uint8_t* bm = best_mask + Q.best_mask_offset;
    for (int i = t; i < nf; i += kLanes) in[i] = 0;   // vbInliers.clear()
    // thread 0 walks the candidates; every lane refines one
    int scan = 0, best = Q.best_inliers, setter = -1;   // thread 0's
    bool seen = false;
    if (t == 0) s_ret = -1;
    for (;;) {
        if (t == 0) {
            int q = 0;
            for (; q < kLanes; q++) {
                bool carried;
                const int j = next_candidate(hyp, n_run, min_inliers, &scan, &best, &seen, &carried);
                if (j < 0) break;
                cand_j[q] = j;
                cand_carried[q] = carried ? 1 : 0;
            }
            s_ncand = q;
        }
        __syncthreads();
        const int nc = s_ncand;
        if (nc == 0) break;
        if (t < nc) {
            const Hyp& h = hyp[cand_j[t]];
            int singular = 0;
            Hyp r;
            if (cand_carried[t]) refine(C, n, MaskBytes{bm}, cam, &r, &singular);
            else refine(C, n, MaskPose{h.R, h.t, cam}, cam, &r, &singular);
            ref[t] = r;
        }
        __syncthreads();
        if (t == 0) {
            for (int q = 0; q < nc; q++) {
                if (!cand_carried[q]) setter = cand_j[q];
                if (refine_succeeds(ref[q].n, min_inliers)) { s_ret = q; break; }
            }
        }
        __syncthreads();
        if (s_ret >= 0 || nc < kLanes) break;
    }
    if (t == 0) s_setter = setter;
    __syncthreads();   // also: every read of the carried mask is done before it is rewritten below
    const int q_ret = s_ret, ls = s_setter;
    const bool refined = q_ret >= 0;
    const Outcome o = decide(refined, refined ? cand_j[q_ret] : 0, refined ? ref[q_ret].n : 0, n, min_inliers, cut,
                             ls >= 0 ? hyp[ls].n : -1, Q.best_inliers, Q.iterations_done, first, n_run);
    if (o.status == kRefined) {
        for (int i = t; i < n; i += kLanes)
            if (check_inlier(C[i], ref[q_ret].R, ref[q_ret].t, cam)) in[C[i].index] = 1;   // distinct indices: no race
    } else if (o.status == kBestNoMore) {
        for (int i = t; i < n; i += kLanes) {
            const bool is = o.from_setter ? check_inlier(C[i], hyp[ls].R, hyp[ls].t, cam) : bm[i] != 0;
            if (is) in[C[i].index] = 1;
        }
    }
    __syncthreads();   // the carried mask was read above; the inlier bytes are written
    if (ls >= 0)
        for (int i = t; i < n; i += kLanes) bm[i] = check_inlier(C[i], hyp[ls].R, hyp[ls].t, cam) ? 1 : 0;
    if (o.pose && frame_points) {
        int32_t* fp = frame_points + Q.inlier_offset;
        const int row0 = map.match_off[Q.kf];
        for (int i = t; i < nf; i += kLanes) fp[i] = in[i] ? map.match_row[row0 + match[Q.match_offset + i]] : -1;
    }
    if (t == 0) {
        spslam_pnp_result r{};
        fill_result(r, o, n, min_inliers, max_its[n], P.max_iterations, ls >= 0 ? &hyp[ls] : nullptr, Q.best_Tcw,
                    refined ? &ref[q_ret] : nullptr);
        results[p] = r;
    }
}

static_assert(kRefined == SPSLAM_PNP_REFINED && kBestNoMore == SPSLAM_PNP_BEST_NO_MORE && kNoMore == SPSLAM_PNP_NO_MORE &&
                  kOutOfDraws == SPSLAM_PNP_OUT_OF_DRAWS,
              "pnp_math.h's statuses are the header's");

}  // namespace pnp

size_t pnp_scratch_bytes(int n_problems, int cap, int max_iterations) {
    return (size_t)n_problems * (sizeof(pnp::Header) + (size_t)cap * sizeof(pnp::Corr) +
                                 (size_t)max_iterations * sizeof(pnp::Hyp));
}

hipError_t pnp_solver_launch(int n_problems, const spslam_pnp_problem* problems, const spslam_sim3_map& map,
                             const spslam_keypoint* kun, const int* counts, int cap, const int32_t* match,
                             const int32_t* rnd, const int32_t* max_its, const int32_t* min_n, const PnpConsts& P,
                             uint8_t* scratch, spslam_pnp_result* results, uint8_t* inliers, uint8_t* best_mask,
                             int32_t* frame_points, hipStream_t s) {
    if (n_problems < 1 || n_problems > 65535 || cap < 1 || cap > 8192 || P.max_iterations < 1 ||
        P.max_iterations > SPSLAM_PNP_MAX_ITERATIONS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pnp::pnp_gather_kernel, dim3(n_problems), dim3(pnp::kThreads), 0, s, problems, map, kun, counts,
                       cap, match, P, scratch);
    hipLaunchKernelGGL(pnp::pnp_hypothesis_kernel,
                       dim3(n_problems, (P.max_iterations + pnp::kLanes - 1) / pnp::kLanes), dim3(pnp::kLanes), 0, s,
                       problems, cap, rnd, max_its, min_n, P, scratch);
    hipLaunchKernelGGL(pnp::pnp_select_kernel, dim3(n_problems), dim3(pnp::kLanes), 0, s, problems, map, counts, cap,
                       match, max_its, min_n, P, scratch, results, inliers, best_mask, frame_points);
    return hipGetLastError();
}

}  // namespace spslam
