// Sim3Solver on gfx950 (src/Sim3Solver.cc as LoopClosing::ComputeSim3 drives it, src/LoopClosing.cc:276-325): the
// constructor, iterate and GetEstimated*.  Semantics: tests/sim3_solver_ref.py; the arithmetic is
// sim3_math.h, shared with a host build.
//
//   sim3_gather_kernel      the constructor (:37-112), one workgroup per problem: KF1's keypoints in chunks of 256,
//                           kept ones compacted in order (ballot within a wave, the waves' counts prefixed through
//                           LDS), each kept one's X3Dc1 / X3Dc2, image points, error bounds and index written to the
//                           problem's scratch with N.
//   sim3_hypothesis_kernel  one wave per (problem, 64 iterations), one lane per iteration of the call's range: the
//                           draws, ComputeSim3 and CheckInliers over the N correspondences, which every lane reads
//                           at the same address (a broadcast; no LDS staging is needed for that).  The 4x4 Jacobi
//                           indexes its matrix at run time, so each lane keeps it in LDS, word w of lane l at
//                           w * 64 + l: no bank is shared within an access.  Writes mnInliersi, s, R and t.
//   sim3_select_kernel      one workgroup per problem: selects the iteration at which the sequential loop returns,
//                           writes the result record, vbInliers and, when asked, the pair and the filtered match12
//                           that SearchBySim3 takes.
//
// Selection.  The reference (:158-201) keeps mnBestInliers = max over the iterations so far and returns at the
// first iteration k with n_k >= mnBestInliers && n_k > mRansacMinInliers.  With best_in the value of mnBestInliers
// on entry, the running best before iteration k is B_k = max(best_in, n_j for j < k): an n_j below B_j does not
// raise it, any other becomes it.  Let k* be the first k of the call with n_k > min_inliers && n_k >= best_in.
// (a) The reference cannot return before k*: a returning k has n_k >= B_k >= best_in and n_k > min_inliers.
// (b) It returns at k*: every earlier n_j is <= min_inliers < n_k* or < best_in <= n_k*, so B_k* <= n_k*.
// Nothing but the two ints crosses iterations, so all hypotheses of the call are evaluated independently and k* is
// taken; best_out = max(best_in, n_j over the iterations run: up to and including k*, or the whole range).
#include <hip/hip_runtime.h>

#include "orb_match_device.h"
#include "sim3_launch.h"
#include "sim3_math.h"

namespace spslam {
namespace sim3 {

using orb_match::level_entry;

constexpr int kThreads = 256, kWaves = kThreads / 64, kHypLanes = 64;
constexpr int kJacobiWords = 16 + 16 + 4 + 4 + 4;  // A, V, W, indR, indC

struct Header { int32_t n, pad[3]; };

__device__ __forceinline__ size_t problem_bytes(int cap, int max_its) {
    return sizeof(Header) + (size_t)cap * sizeof(Corr) + (size_t)max_its * sizeof(Hyp);
}
__device__ __forceinline__ Header* header_of(uint8_t* scratch, int p, int cap, int max_its) {
    return (Header*)(scratch + (size_t)p * problem_bytes(cap, max_its));
}
__device__ __forceinline__ Corr* corr_of(Header* h) { return (Corr*)(h + 1); }
__device__ __forceinline__ Hyp* hyp_of(Header* h, int cap) { return (Hyp*)((uint8_t*)(h + 1) + (size_t)cap * sizeof(Corr)); }

// the keypoint counts the kernels agree on
__device__ __forceinline__ int keyframe_n(const spslam_sim3_map& map, const int* counts, int cap, int kf) {
    return min(min(counts[map.kf_slot[kf]], cap), map.match_off[kf + 1] - map.match_off[kf]);
}

// the iterations of this call: [first, first + *n_run), and mRansacMaxIts
__device__ __forceinline__ int call_range(const spslam_sim3_problem& Q, const SolverConsts& P, const int32_t* table, int n,
                                          int* n_run, int* max_its) {
    const int first = max(Q.iterations_done, 0);
    *max_its = min(max(table[n], 0), P.max_iterations);
    const int want = min(max(Q.n_iterations, 0), P.max_iterations);
    *n_run = n < P.min_inliers ? 0 : max(min(*max_its - first, want), 0);
    return first;
}

__global__ __launch_bounds__(kThreads) void sim3_gather_kernel(const spslam_sim3_problem* __restrict__ problems,
                                                               spslam_sim3_map map,
                                                               const spslam_keypoint* __restrict__ kun,
                                                               const int* __restrict__ counts, int cap,
                                                               const int32_t* __restrict__ match12, SolverConsts P,
                                                               uint8_t* __restrict__ scratch) {
    __shared__ int wave_n[kWaves];
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const spslam_sim3_problem Q = problems[p];
    const int n1 = keyframe_n(map, counts, cap, Q.kf1), n2 = keyframe_n(map, counts, cap, Q.kf2);
    const size_t s1 = (size_t)map.kf_slot[Q.kf1] * cap, s2 = (size_t)map.kf_slot[Q.kf2] * cap;
    const float* T1 = map.kf_Tcw + 16 * (size_t)Q.kf1;
    const float* T2 = map.kf_Tcw + 16 * (size_t)Q.kf2;
    Header* H = header_of(scratch, p, cap, P.max_iterations);
    Corr* out = corr_of(H);
    int base = 0;
    for (int c0 = 0; c0 < n1; c0 += kThreads) {
        const int i1 = c0 + t;
        int row1 = -1, row2 = -1, i2 = -1;
        if (i1 < n1) {
            i2 = match12[Q.match_offset + i1];
            if (i2 >= 0 && i2 < n2) {                                           // vpMatched12[i1]
                row1 = map.match_row[map.match_off[Q.kf1] + i1];               // vpKeyFrameMP1[i1]
                row2 = map.match_row[map.match_off[Q.kf2] + i2];
            }
        }
        bool keep = row1 >= 0 && row2 >= 0;
        if (keep && map.point_bad) keep = !map.point_bad[row1] && !map.point_bad[row2];   // :72
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
            Corr c;
            const float t1[3] = {T1[3], T1[7], T1[11]}, t2[3] = {T2[3], T2[7], T2[11]};
            mat3_mul(T1, 4, map.points[row1].xw, t1, 1.0, c.X1);                // Rcw1*X3D1w+tcw1
            mat3_mul(T2, 4, map.points[row2].xw, t2, 1.0, c.X2);
            to_image(c.X1, P.fx, P.fy, P.cx, P.cy, c.p1);
            to_image(c.X2, P.fx, P.fy, P.cx, P.cy, c.p2);
            c.b1 = level_entry(P.max_error, kun[s1 + i1].octave);
            c.b2 = level_entry(P.max_error, kun[s2 + i2].octave);
            c.i1 = i1;
            c.pad = 0;
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

// a lane's Jacobi storage in LDS
struct JacobiLds {
    float* f;  // this lane's word 0
    __device__ float& a(int i, int j) { return f[(4 * i + j) * kHypLanes]; }
    __device__ float& v(int i, int j) { return f[(16 + 4 * i + j) * kHypLanes]; }
    __device__ float& w(int i) { return f[(32 + i) * kHypLanes]; }
    __device__ int& ir(int i) { return ((int*)f)[(36 + i) * kHypLanes]; }
    __device__ int& ic(int i) { return ((int*)f)[(40 + i) * kHypLanes]; }
};

__global__ __launch_bounds__(kHypLanes) void sim3_hypothesis_kernel(const spslam_sim3_problem* __restrict__ problems,
                                                                    int cap, const int32_t* __restrict__ rnd,
                                                                    const int32_t* __restrict__ table, SolverConsts P,
                                                                    uint8_t* __restrict__ scratch) {
    __shared__ float jac[kJacobiWords * kHypLanes];
    const int p = blockIdx.x, lane = threadIdx.x;
    const spslam_sim3_problem Q = problems[p];
    Header* H = header_of(scratch, p, cap, P.max_iterations);
    const int n = H->n;
    int n_run, max_its;
    const int first = call_range(Q, P, table, n, &n_run, &max_its);
    const int j = blockIdx.y * kHypLanes + lane;
    if (j >= n_run) return;
    const int k = first + j;  // < max_its <= P.max_iterations: inside the draws and the hypothesis records
    const Corr* C = corr_of(H);
    int idx[3];
    draw3(rnd + Q.rand_offset + 3 * (size_t)k, P.rand_max, n, idx);
    float X1[3][3], X2[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int r = 0; r < 3; r++) {
            X1[i][r] = C[idx[i]].X1[r];
            X2[i][r] = C[idx[i]].X2[r];
        }
    JacobiLds J{jac + lane};
    Hyp h;
    compute_sim3(J, X1, X2, P.fix_scale != 0, &h.s, h.R, h.t);
    float T12[12], T21[12];
    transforms(h.s, h.R, h.t, T12, T21);
    int count = 0;
    for (int i = 0; i < n; i++) count += is_inlier(C[i], T12, T21, P.fx, P.fy, P.cx, P.cy) ? 1 : 0;
    h.n = count;
    h.pad[0] = h.pad[1] = 0;
    hyp_of(H, cap)[k] = h;
}

__global__ __launch_bounds__(kThreads) void sim3_select_kernel(const spslam_sim3_problem* __restrict__ problems,
                                                               spslam_sim3_map map, const int* __restrict__ counts,
                                                               int cap, const int32_t* __restrict__ match12,
                                                               const int32_t* __restrict__ table, SolverConsts P,
                                                               uint8_t* __restrict__ scratch,
                                                               spslam_sim3_result* __restrict__ results,
                                                               uint8_t* __restrict__ inliers,
                                                               spslam_sim3_pair* __restrict__ pairs_out,
                                                               int32_t* __restrict__ match12_out) {
    __shared__ int s_first, s_best;
    const int p = blockIdx.x, t = threadIdx.x;
    const spslam_sim3_problem Q = problems[p];
    Header* H = header_of(scratch, p, cap, P.max_iterations);
    const Corr* C = corr_of(H);
    const Hyp* hyp = hyp_of(H, cap);
    const int n = H->n, n1 = keyframe_n(map, counts, cap, Q.kf1);
    int n_run, max_its;
    const int first = call_range(Q, P, table, n, &n_run, &max_its);
    if (t == 0) { s_first = n_run; s_best = Q.best_inliers; }
    uint8_t* in = inliers + Q.inlier_offset;
    for (int i = t; i < n1; i += kThreads) in[i] = 0;   // vbInliers = vector<bool>(mN1, false)
    __syncthreads();
    for (int j = t; j < n_run; j += kThreads) {
        const int nj = hyp[first + j].n;
        if (nj > P.min_inliers && nj >= Q.best_inliers) atomicMin(&s_first, j);
    }
    __syncthreads();
    const int jf = s_first;
    const bool found = jf < n_run;
    const int ran = found ? jf + 1 : n_run;
    for (int j = t; j < ran; j += kThreads) atomicMax(&s_best, hyp[first + j].n);
    __syncthreads();
    const int done = first + ran;
    if (found) {
        const Hyp h = hyp[first + jf];
        float T12[12], T21[12];
        transforms(h.s, h.R, h.t, T12, T21);
        for (int i = t; i < n; i += kThreads)
            if (is_inlier(C[i], T12, T21, P.fx, P.fy, P.cx, P.cy)) in[C[i].i1] = 1;   // distinct i1: no race
        if (t == 0) {
            spslam_sim3_result r;
            r.status = SPSLAM_SIM3_FOUND;
            r.n = n;
            r.iterations_done = done;
            r.best_inliers = s_best;
            r.n_inliers = h.n;
            r.s12 = h.s;
            for (int q = 0; q < 9; q++) r.R12[q] = h.R[q];
            for (int q = 0; q < 3; q++) r.t12[q] = h.t[q];
            for (int q = 0; q < 12; q++) r.T12[q] = T12[q];
            r.T12[12] = r.T12[13] = r.T12[14] = 0.f;
            r.T12[15] = 1.f;
            results[p] = r;
            if (pairs_out) {
                spslam_sim3_pair o;
                o.kf1 = Q.kf1; o.kf2 = Q.kf2;
                o.match_offset = Q.match_offset;
                o.result_offset = p;
                o.s12 = h.s;
                for (int q = 0; q < 9; q++) o.R12[q] = h.R[q];
                for (int q = 0; q < 3; q++) o.t12[q] = h.t[q];
                o.pad[0] = o.pad[1] = o.pad[2] = 0;
                pairs_out[p] = o;
            }
        }
        if (match12_out) {
            __syncthreads();  // the inlier bytes of this workgroup
            for (int i = t; i < n1; i += kThreads)
                match12_out[Q.match_offset + i] = in[i] ? match12[Q.match_offset + i] : -1;
        }
    } else if (t == 0) {
        spslam_sim3_result r{};
        r.status = n < P.min_inliers || done >= max_its ? SPSLAM_SIM3_NO_MORE : SPSLAM_SIM3_NOT_YET;
        r.n = n;
        r.iterations_done = n < P.min_inliers ? Q.iterations_done : done;
        r.best_inliers = s_best;
        results[p] = r;
    }
}

}  // namespace sim3

size_t sim3_scratch_bytes(int n_problems, int cap, int max_iterations) {
    return (size_t)n_problems * (sizeof(sim3::Header) + (size_t)cap * sizeof(sim3::Corr) +
                                 (size_t)max_iterations * sizeof(sim3::Hyp));
}

hipError_t sim3_solver_launch(int n_problems, const spslam_sim3_problem* problems, const spslam_sim3_map& map,
                              const spslam_keypoint* kun, const int* counts, int cap, const int32_t* match12,
                              const int32_t* rnd, const int32_t* table, const SolverConsts& P, uint8_t* scratch,
                              spslam_sim3_result* results, uint8_t* inliers, spslam_sim3_pair* pairs_out,
                              int32_t* match12_out, hipStream_t s) {
    if (n_problems < 1 || n_problems > 65535 || cap < 1 || cap > 8192 || P.max_iterations < 1 ||
        P.max_iterations > SPSLAM_SIM3_MAX_ITERATIONS || P.min_inliers < 3)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sim3::sim3_gather_kernel, dim3(n_problems), dim3(sim3::kThreads), 0, s, problems, map, kun,
                       counts, cap, match12, P, scratch);
    hipLaunchKernelGGL(sim3::sim3_hypothesis_kernel,
                       dim3(n_problems, (P.max_iterations + sim3::kHypLanes - 1) / sim3::kHypLanes),
                       dim3(sim3::kHypLanes), 0, s, problems, cap, rnd, table, P, scratch);
    hipLaunchKernelGGL(sim3::sim3_select_kernel, dim3(n_problems), dim3(sim3::kThreads), 0, s, problems, map, counts,
                       cap, match12, table, P, scratch, results, inliers, pairs_out, match12_out);
    return hipGetLastError();
}

}  // namespace spslam
