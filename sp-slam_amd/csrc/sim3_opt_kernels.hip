// Optimizer::OptimizeSim3 on gfx950 (src/Optimizer.cc:2279-2474, called at src/LoopClosing.cc:328) and the Scw of
// LoopClosing.cc:335-337.  Semantics: tests/sim3_opt_ref.cpp; the arithmetic and the
// Levenberg-Marquardt driver are sim3_opt_math.h, shared with a host build.
//
// One 256-thread workgroup per pair, one launch, no host round trip:
//   gather     KF1's keypoints in chunks of 256, kept ones compacted in order (ballot within a wave, the waves'
//              counts prefixed through LDS) into the problem's scratch: P3D1c, P3D2c, the two observations, the two
//              information weights, the index.
//   linearize  threads 0..13 make the 14 estimates Sim3(+-delta e_d) * S and their inverses once (they do not
//              depend on the edge) and share them through LDS.  Then kChunk correspondences at a time, one thread
//              per edge (thread 2j is e12 of correspondence j, 2j + 1 its e21: g2o's insertion order): the error,
//              the numeric Jacobian, the robust chi2, the 28 lower terms of B^T W B and the 7 of B^T omega_r, staged
//              in LDS; 36 lanes then add their column edge by edge, removed pairs skipped: the reference's sums,
//              not a tree.
//   trial      the robust chi2 of every active edge at the trial estimate, staged and chained by one lane.
//   driver     every thread runs sim3opt::optimize with the same values (the 7x7 LDLT in registers, the update,
//              the accept / reject walk), so the control flow is uniform and only the edge passes are divided.
//   checks     the chi2 both checks read are those of the last computeActiveErrors, which may belong to a rejected
//              trial: the driver keeps that estimate and the check evaluates the edges at it (the same inputs, the
//              same bits as the cached values).
// Every loop is bounded by a constant (5 / 10 iterations, 10 trials, the LDLT's 7) or by n.
#include <hip/hip_runtime.h>

#include "orb_match_device.h"
#include "sim3_opt_launch.h"
#include "sim3_opt_math.h"

namespace spslam {
namespace sim3opt {

using orb_match::level_entry;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kChunk = kThreads / 2;  // correspondences per pass: one thread per edge
constexpr int kStride = kTerms + 1;   // doubles per staged edge row (odd: the chain lanes' columns spread over the banks)

struct Header { int32_t n, pad[3]; };

struct Shared {
    double terms[kThreads * kStride];
    S3 pert[2][14];  // [0]: Sim3(+-delta e_d) * S, [1]: their inverses
    double red[kTerms];
    int wave_n[kWaves];
    int count;
    uint8_t active[kThreads];
};

__device__ __forceinline__ int keyframe_n(const spslam_sim3_map& map, const int* counts, int cap, int kf) {
    return min(min(counts[map.kf_slot[kf]], cap), map.match_off[kf + 1] - map.match_off[kf]);
}

// the edge passes of sim3opt::optimize / optimize_sim3 on one workgroup
struct DeviceOps {
    Shared& L;
    Corr* C;
    int32_t* match12;
    Cam cam;
    double delta;
    int n, n_removed, t;

    __device__ int n_corr() const { return n; }
    __device__ int n_active() const { return 2 * (n - n_removed); }
    __device__ void note_optimize(int) {}
    __device__ void note_update(int) {}
    __device__ void note_trial(double, double, bool) {}

    __device__ void linearize(const S3& S, double* chi, double* H, double* b) {
        __syncthreads();
        if (t < 14) {
            const S3 P = perturbed(S, t);
            L.pert[0][t] = P;
            L.pert[1][t] = sim3_inverse(P);
        }
        const S3 Sinv = sim3_inverse(S);
        __syncthreads();
        const int kind = t & 1;
        double acc = 0.0;
        for (int c0 = 0; c0 < n; c0 += kChunk) {
            const int j = c0 + (t >> 1);
            bool act = false;
            if (j < n) {
                const Corr c = C[j];
                if (!c.removed) {
                    act = true;
                    double out[kTerms];
                    edge_terms(kind ? Sinv : S, L.pert[kind], kind ? c.X1 : c.X2, kind ? c.o2 : c.o1, kind ? c.w2 : c.w1,
                               cam, delta, out);
#pragma unroll
                    for (int k = 0; k < kTerms; k++) L.terms[t * kStride + k] = out[k];
                }
            }
            L.active[t] = act ? 1 : 0;
            __syncthreads();
            if (t < kTerms) {
                const int rows = min(2 * (n - c0), kThreads);
                for (int r = 0; r < rows; r++)
                    if (L.active[r]) acc += L.terms[r * kStride + t];
            }
            __syncthreads();
        }
        if (t < kTerms) L.red[t] = acc;
        __syncthreads();
        *chi = L.red[0];
#pragma unroll
        for (int k = 0; k < 28; k++) H[k] = L.red[1 + k];
#pragma unroll
        for (int k = 0; k < 7; k++) b[k] = L.red[29 + k];
    }

    __device__ void robust_chi2(const S3& S, double* chi) {
        const S3 Sinv = sim3_inverse(S);
        const int kind = t & 1;
        double acc = 0.0;
        __syncthreads();
        for (int c0 = 0; c0 < n; c0 += kChunk) {
            const int j = c0 + (t >> 1);
            bool act = false;
            if (j < n) {
                const Corr c = C[j];
                if (!c.removed) {
                    act = true;
                    L.terms[t] = edge_robust_chi2(kind ? Sinv : S, kind ? c.X1 : c.X2, kind ? c.o2 : c.o1,
                                                  kind ? c.w2 : c.w1, cam, delta);
                }
            }
            L.active[t] = act ? 1 : 0;
            __syncthreads();
            if (t == 0) {
                const int rows = min(2 * (n - c0), kThreads);
                for (int r = 0; r < rows; r++)
                    if (L.active[r]) acc += L.terms[r];
            }
            __syncthreads();
        }
        if (t == 0) L.red[0] = acc;
        __syncthreads();
        *chi = L.red[0];
    }

    // both checks: the pairs still in the graph whose e12 or e21 has chi2 > th2 at `last`
    __device__ int check(const S3& last, double th2, bool first) {
        const S3 Sinv = sim3_inverse(last);
        __syncthreads();
        if (t == 0) L.count = 0;
        __syncthreads();
        for (int j = t; j < n; j += kThreads) {
            const Corr c = C[j];
            if (c.removed) continue;
            double e[2];
            edge_error(last, c.X2, c.o1, cam, e);
            const double c12 = edge_chi2(c.w1, e);
            edge_error(Sinv, c.X1, c.o2, cam, e);
            const double c21 = edge_chi2(c.w2, e);
            const bool bad = c12 > th2 || c21 > th2;
            if (bad) {
                match12[c.i] = -1;
                if (first) C[j].removed = 1;
            }
            if (bad == first) atomicAdd(&L.count, 1);  // nBad of the first check, nIn of the final one
        }
        __syncthreads();
        return L.count;
    }
    __device__ int check_first(const S3& last, double th2) {
        const int bad = check(last, th2, true);
        n_removed = bad;
        return bad;
    }
    __device__ int check_final(const S3& last, double th2) { return check(last, th2, false); }
};

__global__ __launch_bounds__(kThreads) void sim3_opt_kernel(const spslam_sim3_pair* __restrict__ pairs,
                                                            spslam_sim3_map map,
                                                            const spslam_keypoint* __restrict__ kun,
                                                            const int* __restrict__ counts, int cap, Sim3OptConsts P,
                                                            uint8_t* __restrict__ scratch, int32_t* match12,
                                                            spslam_sim3_opt_result* __restrict__ results) {
    __shared__ Shared L;
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const spslam_sim3_pair Q = pairs[p];
    const int n1 = keyframe_n(map, counts, cap, Q.kf1), n2 = keyframe_n(map, counts, cap, Q.kf2);
    const size_t s1 = (size_t)map.kf_slot[Q.kf1] * cap, s2 = (size_t)map.kf_slot[Q.kf2] * cap;
    const float* T1 = map.kf_Tcw + 16 * (size_t)Q.kf1;
    const float* T2 = map.kf_Tcw + 16 * (size_t)Q.kf2;
    Header* Hd = (Header*)(scratch + (size_t)p * (sizeof(Header) + (size_t)cap * sizeof(Corr)));
    Corr* out = (Corr*)(Hd + 1);
    int32_t* m12 = match12 + Q.match_offset;

    // ---- the gather (:2332-2411)
    int base = 0;
    for (int c0 = 0; c0 < n1; c0 += kThreads) {
        const int i1 = c0 + t;
        int row1 = -1, row2 = -1, i2 = -1;
        if (i1 < n1) {
            i2 = m12[i1];
            if (i2 >= 0 && i2 < n2) {                                           // vpMatches1[i]
                row1 = map.match_row[map.match_off[Q.kf1] + i1];               // vpMapPoints1[i]
                row2 = map.match_row[map.match_off[Q.kf2] + i2];               // i2 = GetIndexInKeyFrame(pKF2)
            }
        }
        bool keep = row1 >= 0 && row2 >= 0;
        if (keep && map.point_bad) keep = !map.point_bad[row1] && !map.point_bad[row2];
        const unsigned long long m = __ballot(keep);
        if (lane == 0) L.wave_n[wave] = __popcll(m);
        __syncthreads();
        int before = base, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            before += w < wave ? L.wave_n[w] : 0;
            total += L.wave_n[w];
        }
        if (keep) {
            Corr c;
            float X1[3], X2[3];
            const float t1[3] = {T1[3], T1[7], T1[11]}, t2[3] = {T2[3], T2[7], T2[11]};
            sim3::mat3_mul(T1, 4, map.points[row1].xw, t1, 1.0, X1);            // R1w*P3D1w + t1w
            sim3::mat3_mul(T2, 4, map.points[row2].xw, t2, 1.0, X2);
            const spslam_keypoint k1 = kun[s1 + i1], k2 = kun[s2 + i2];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                c.X1[r] = (double)X1[r];
                c.X2[r] = (double)X2[r];
            }
            c.o1[0] = (double)k1.x; c.o1[1] = (double)k1.y;
            c.o2[0] = (double)k2.x; c.o2[1] = (double)k2.y;
            c.w1 = (double)level_entry(P.inv_sigma2, k1.octave);
            c.w2 = (double)level_entry(P.inv_sigma2, k2.octave);
            c.i = i1;
            c.removed = 0;
            out[before + __popcll(m & ((1ull << lane) - 1ull))] = c;
        }
        base += total;
        __syncthreads();  // wave_n is rewritten by the next chunk
    }
    if (t == 0) {
        Hd->n = base;
        Hd->pad[0] = Hd->pad[1] = Hd->pad[2] = 0;
    }
    __syncthreads();  // the correspondences are read by other threads from here on

    // ---- optimize(5), the check, optimize(5 or 10), the check (:2413-2473)
    DeviceOps ops{L, out, m12, Cam{(double)P.fx, (double)P.fy, (double)P.cx, (double)P.cy},
                  (double)sqrtf(P.th2), base, 0, t};
    const S3 S0 = sim3_from_float(Q.R12, 3, Q.t12[0], Q.t12[1], Q.t12[2], (double)Q.s12);
    Outcome o;
    optimize_sim3(ops, S0, (double)P.th2, &o);

    if (t == 0) {
        spslam_sim3_opt_result r;
        r.n_in = o.n_in;
        r.n_corr = o.n_corr;
        r.n_bad = o.n_bad;
        r.status = o.too_few ? SPSLAM_SIM3_OPT_TOO_FEW : SPSLAM_SIM3_OPT_OK;
        r.accepted = o.n_in >= P.min_inliers ? 1 : 0;
        r.iterations1 = o.its[0]; r.trials1 = o.trials[0];
        r.iterations2 = o.its[1]; r.trials2 = o.trials[1];
        r.pad = 0;
        r.S12[0] = o.S12.r.x; r.S12[1] = o.S12.r.y; r.S12[2] = o.S12.r.z; r.S12[3] = o.S12.r.w;
        r.S12[4] = o.S12.t.x; r.S12[5] = o.S12.t.y; r.S12[6] = o.S12.t.z; r.S12[7] = o.S12.s;
        scw_of(o.S12, T2, r.Scw, r.mScw);
        results[p] = r;
    }
}

}  // namespace sim3opt

size_t sim3_opt_scratch_bytes(int n_pairs, int cap) {
    return (size_t)n_pairs * (sizeof(sim3opt::Header) + (size_t)cap * sizeof(sim3opt::Corr));
}

hipError_t sim3_opt_launch(int n_pairs, const spslam_sim3_pair* pairs, const spslam_sim3_map& map,
                           const spslam_keypoint* kun, const int* counts, int cap, const Sim3OptConsts& P,
                           uint8_t* scratch, int32_t* match12, spslam_sim3_opt_result* results, hipStream_t s) {
    if (n_pairs < 1 || n_pairs > 65535 || cap < 1 || cap > 8192 || !(P.th2 > 0.f)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sim3opt::sim3_opt_kernel, dim3(n_pairs), dim3(sim3opt::kThreads), 0, s, pairs, map, kun, counts,
                       cap, P, scratch, match12, results);
    return hipGetLastError();
}

}  // namespace spslam
