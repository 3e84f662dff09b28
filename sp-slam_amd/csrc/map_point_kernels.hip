// gfx950 kernel for the map-point refresh of LocalMapping (include/spslam_gpu.h, spslam_map_points_refresh_*):
//   MapPoint::ComputeDistinctiveDescriptors  src/MapPoint.cc:242-307
//   MapPoint::UpdateNormalAndDepth           src/MapPoint.cc:330-371
// for listed rows of the spslam_local_point table, in place.
//
// Observer counts are small (2-10 typically), so a wave takes 8 listed rows, 8 lanes each: lane i of a group owns
// observer i -- its descriptor goes into the wave's LDS region (bad keyframes left out, order kept), it computes
// row i of the distance matrix against the staged descriptors and that row's median, and its term of the normal.
// A row with more than 8 observers (up to SPSLAM_POINT_MAX_OBS = 128) is then taken by the whole wave, lanes
// striding over the observers; more than that is reported, never truncated.
//   median   the element floor(0.5*(N-1)) of the row's sorted distances = the smallest d with at least that index
//            + 1 distances <= d: a 9-step bisection over 0 .. 256, each step one pass over the staged descriptors
//            (v_bcnt over 8 dwords); integers only, so no order to keep.
//   best     the first row with the strictly smallest median: min over (median << 8 | row).
//   normal   an ordered float chain: the per-observer terms are made in parallel, then added in observer order
//            (the same chain in every lane, through shuffles).  Every float step is its own rounding.
// Waves do not talk to each other: no workgroup barrier, no wait.  LDS: 4 KiB per wave.
#include <hip/hip_runtime.h>

#include "map_point_launch.h"
#include "orb_match_device.h"
#include "wave_ops.h"

namespace spslam {

namespace {

using namespace orb_match;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kGrp = 8, kRowsPerWave = 64 / kGrp;
constexpr int kMaxObs = SPSLAM_POINT_MAX_OBS;
constexpr uint32_t kNone = 0xffffffffu;
static_assert(kMaxObs <= 256, "the row index takes the key's low 8 bits");

// One observation's term of UpdateNormalAndDepth (:350-357): Ow = -Rcw^T tcw (KeyFrame.cc:82: the three products
// summed in double in row order, negated, rounded), normali = Pos - Ow, *nv = cv::norm(normali) with the squares
// accumulated in double ((x^2 + y^2) + z^2), t = normali / nv.
__device__ __forceinline__ void observer_term(const float* __restrict__ T, const float (&X)[3], float (&t)[3],
                                              float* nv) {
    const double t0 = T[3], t1 = T[7], t2 = T[11];
    float v[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double s = __dadd_rn(__dmul_rn((double)T[i], t0), __dmul_rn((double)T[4 + i], t1));
        s = __dadd_rn(s, __dmul_rn((double)T[8 + i], t2));
        v[i] = __fsub_rn(X[i], (float)-s);
    }
    const double x = v[0], y = v[1], z = v[2];
    *nv = (float)__dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z)));
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = __fdiv_rn(v[i], *nv);
}

// The median of row r of the distance matrix of the M descriptors staged at D (two uint4 each).
__device__ __forceinline__ int row_median(const uint4* D, int M, int r) {
    const uint4 a0 = D[2 * r], a1 = D[2 * r + 1];
    const int need = (M - 1) / 2 + 1;  // vDists[0.5*(N-1)] is the need-th smallest
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
        for (int k = 0; k < M; k++) cnt += hamming(a0, a1, D[2 * k], D[2 * k + 1]) <= mid;
        if (cnt >= need) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ void stage_descriptor(uint4* D, int r, const uint8_t* __restrict__ desc) {
    D[2 * r] = *(const uint4*)desc;
    D[2 * r + 1] = *(const uint4*)(desc + 16);
}

// mfMaxDistance, mfMinDistance, mNormalVector (:365-370) by one lane
__device__ __forceinline__ void write_normal_depth(spslam_local_point& p, const float (&sum)[3], int N, float dist,
                                                   int octave, const RefreshConsts& P) {
    const float max_d = __fmul_rn(dist, level_entry(P.scale, octave));
    p.max_dist = max_d;
    p.min_dist = __fdiv_rn(max_d, level_entry(P.scale, P.n_levels - 1));
#pragma unroll
    for (int i = 0; i < 3; i++) p.normal[i] = __fdiv_rn(sum[i], (float)N);
}

__global__ __launch_bounds__(kThreads) void map_points_refresh_kernel(spslam_point_refresh_map M,
                                                                      const int32_t* __restrict__ rows, int n,
                                                                      int what,
                                                                      const spslam_keypoint* __restrict__ keys_un,
                                                                      const uint8_t* __restrict__ desc, int cap,
                                                                      RefreshConsts P, uint8_t* __restrict__ status) {
    __shared__ uint4 lds[kWaves][2 * kMaxObs];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane / kGrp, sub = lane & (kGrp - 1);
    uint4* const D = lds[wave];
    const int e = (blockIdx.x * kWaves + wave) * kRowsPerWave + grp;  // this group's entry of the row list
    int row = 0, o0 = 0, N = 0, st = SPSLAM_REFRESH_UNTOUCHED;
    if (e < n) {
        row = rows[e];
        o0 = M.obs_off[row];
        N = M.obs_off[row + 1] - o0;
        const bool bad = M.point_bad && M.point_bad[row];
        if (!bad && N > 0) st = N > kMaxObs ? SPSLAM_REFRESH_CAPACITY : SPSLAM_REFRESH_DONE;
        if (sub == 0) status[e] = (uint8_t)st;
    }
    const bool todo = e < n && st == SPSLAM_REFRESH_DONE;
    const bool small = todo && N <= kGrp, big = todo && N > kGrp;
    const bool do_desc = what & SPSLAM_REFRESH_DESCRIPTOR, do_normal = what & SPSLAM_REFRESH_NORMAL_DEPTH;
    const int g0 = grp * kGrp;  // the group's first lane

    // ---- rows of up to 8 observers: one observer per lane.  Predicated, not branched: the shuffles and the
    //      LDS hand-off below are executed by the whole wave.
    {
        const bool mine = small && sub < N;
        int kf = -1, kp = 0;
        bool valid = false;
        if (mine) {
            kf = M.obs_kf[o0 + sub];
            kp = M.obs_kp[o0 + sub];
            valid = !(M.kf_bad && M.kf_bad[kf]);  // if(!pKF->isBad()) (:265)
        }
        if (do_desc) {
            const uint32_t gm = (uint32_t)(__ballot(mine && valid) >> g0) & 0xffu;
            const int Mv = __popc(gm), r = __popc(gm & ((1u << sub) - 1u));
            uint4* const Dg = D + 2 * g0;
            if (mine && valid) stage_descriptor(Dg, r, desc + ((size_t)M.kf_slot[kf] * cap + kp) * 32);
            wave_sync();
            uint32_t key = kNone;
            if (mine && valid) key = ((uint32_t)row_median(Dg, Mv, r) << 8) | (uint32_t)r;
#pragma unroll
            for (int o = kGrp / 2; o >= 1; o >>= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o));
            // vDescriptors[BestIdx], one dword per lane; no observer left (:269): unchanged
            if (small && Mv > 0)
                ((uint32_t*)M.points[row].desc)[sub] = ((const uint32_t*)(Dg + 2 * (key & 0xffu)))[sub];
            wave_sync();  // the region is staged again below
        }
        if (do_normal) {
            float t[3] = {0.f, 0.f, 0.f}, nv = 0.f;
            float X[3] = {0.f, 0.f, 0.f};
            if (small) { X[0] = M.points[row].xw[0]; X[1] = M.points[row].xw[1]; X[2] = M.points[row].xw[2]; }
            if (mine) observer_term(M.kf_Tcw + 16 * (size_t)kf, X, t, &nv);
            // pRefKF's observation; mpRefKF not among the observers: the first one
            const int ref = small ? M.ref_kf[row] : -2;
            const uint32_t rm = (uint32_t)(__ballot(mine && kf == ref) >> g0) & 0xffu;
            const int rl = g0 + (rm ? __ffs((int)rm) - 1 : 0);
            float sum[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < kGrp; k++) {
                const float a = __shfl(t[0], g0 + k), b = __shfl(t[1], g0 + k), c = __shfl(t[2], g0 + k);
                if (k < N) { sum[0] = __fadd_rn(sum[0], a); sum[1] = __fadd_rn(sum[1], b); sum[2] = __fadd_rn(sum[2], c); }
            }
            const float dist = __shfl(nv, rl);  // cv::norm(Pos - pRefKF->GetCameraCenter()): that lane's nv
            const int rkf = __shfl(kf, rl), rkp = __shfl(kp, rl);
            if (small && sub == 0)
                write_normal_depth(M.points[row], sum, N, dist, keys_un[(size_t)M.kf_slot[rkf] * cap + rkp].octave, P);
        }
    }

    // ---- rows of 9 .. 128 observers: the whole wave, one row after the other (uniform loop)
    if (!__ballot(big)) return;
    for (int g = 0; g < kRowsPerWave; g++) {
        if (!__shfl((int)big, g * kGrp)) continue;
        const int rw = __shfl(row, g * kGrp), ob = __shfl(o0, g * kGrp), Nw = __shfl(N, g * kGrp);
        if (do_desc) {
            int Mv = 0;
            for (int base = 0; base < Nw; base += 64) {
                const bool have = base + lane < Nw;
                bool valid = false;
                int kf = 0, kp = 0;
                if (have) {
                    kf = M.obs_kf[ob + base + lane];
                    kp = M.obs_kp[ob + base + lane];
                    valid = !(M.kf_bad && M.kf_bad[kf]);
                }
                const unsigned long long vm = __ballot(valid);
                if (valid)
                    stage_descriptor(D, Mv + __popcll(vm & ((1ull << lane) - 1ull)),
                                     desc + ((size_t)M.kf_slot[kf] * cap + kp) * 32);
                Mv += __popcll(vm);
            }
            wave_sync();
            uint32_t key = kNone;
            for (int r = lane; r < Mv; r += 64) key = min(key, ((uint32_t)row_median(D, Mv, r) << 8) | (uint32_t)r);
            key = wave_min(key);
            if (Mv > 0 && lane < 8) ((uint32_t*)M.points[rw].desc)[lane] = ((const uint32_t*)(D + 2 * (key & 0xffu)))[lane];
            wave_sync();
        }
        if (do_normal) {
            const float X[3] = {M.points[rw].xw[0], M.points[rw].xw[1], M.points[rw].xw[2]};
            const int ref = M.ref_kf[rw];
            float sum[3] = {0.f, 0.f, 0.f}, dist = 0.f;
            int rkf = 0, rkp = 0;
            bool found = false;
            for (int base = 0; base < Nw; base += 64) {
                const int cnt = min(64, Nw - base);
                const bool have = lane < cnt;
                float t[3] = {0.f, 0.f, 0.f}, nv = 0.f;
                int kf = -1, kp = 0;
                if (have) {
                    kf = M.obs_kf[ob + base + lane];
                    kp = M.obs_kp[ob + base + lane];
                    observer_term(M.kf_Tcw + 16 * (size_t)kf, X, t, &nv);
                }
                for (int k = 0; k < cnt; k++) {
                    sum[0] = __fadd_rn(sum[0], __shfl(t[0], k));
                    sum[1] = __fadd_rn(sum[1], __shfl(t[1], k));
                    sum[2] = __fadd_rn(sum[2], __shfl(t[2], k));
                }
                const unsigned long long rm = __ballot(have && kf == ref);
                // the reference observation, or until it is found the first observation
                if (!found && (rm || base == 0)) {
                    const int rl = rm ? __ffsll((long long)rm) - 1 : 0;
                    dist = __shfl(nv, rl);
                    rkf = __shfl(kf, rl);
                    rkp = __shfl(kp, rl);
                    found = rm != 0;
                }
            }
            if (lane == 0)
                write_normal_depth(M.points[rw], sum, Nw, dist, keys_un[(size_t)M.kf_slot[rkf] * cap + rkp].octave, P);
        }
    }
}

}  // namespace

hipError_t map_points_refresh_launch(const spslam_point_refresh_map& map, const int32_t* rows, int n, int what,
                                     const spslam_keypoint* keys_un, const uint8_t* desc, int cap,
                                     const RefreshConsts& P, uint8_t* status, hipStream_t s) {
    if (n < 0 || cap < 1) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const int per_block = kWaves * kRowsPerWave;
    hipLaunchKernelGGL(map_points_refresh_kernel, dim3((n + per_block - 1) / per_block), dim3(kThreads), 0, s, map,
                       rows, n, what, keys_un, desc, cap, P, status);
    return hipGetLastError();
}

}  // namespace spslam
