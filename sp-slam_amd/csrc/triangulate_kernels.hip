// LocalMapping::CreateNewMapPoints' per-match work on gfx950 (src/LocalMapping.cc:298-443): the parallax test, the
// linear triangulation or KeyFrame::UnprojectStereo (src/KeyFrame.cc:632-648), and the depth, reprojection and
// scale checks.  Semantics: tests/triangulation_ref.py.
//
//   triangulate_kernel  lane per key-1 feature of a pair.  A lane without a match writes SPSLAM_TRI_NO_MATCH.
//                       The 4x4 null vector is a one-sided Jacobi held in registers (every index is a compile-time
//                       constant: the pair loops are unrolled, the sweep loop is not): columns of A and rows of V
//                       in float, squared norms / dot product / rotation parameters in double made of
//                       + - * / sqrt only, so nothing depends on a math library.  With `mark` the has-point bytes
//                       of accepted records are set (idempotent byte stores; the next round's search reads them).
// Every float step is one rounding (the build has -ffp-contract=off); the contractions the reference's compiler
// makes are written as __fmaf_rn.
#include <hip/hip_runtime.h>

#include "libm_restated.h"
#include "orb_match_device.h"
#include "triangulate_launch.h"

namespace spslam {
namespace tri {

using orb_match::level_entry;

constexpr int kThreads = 256;
constexpr int kSweeps = 30;
constexpr double kEps = 0x1p-22;  // 2*FLT_EPSILON, OpenCV's JacobiSVDImpl_ choice for float matrices

// rows i and j of M (floats) rotated by (c, s) in double; returns the new squared norms when asked
template <bool kNorms>
__device__ __forceinline__ void rotate(float (&M)[4][4], int i, int j, double c, double s, double* a, double* b) {
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double x = (double)M[i][k], y = (double)M[j][k];
        const float t0 = (float)(c * x + s * y), t1 = (float)(c * y - s * x);
        M[i][k] = t0;
        M[j][k] = t1;
        if (kNorms) {
            sa += (double)t0 * (double)t0;
            sb += (double)t1 * (double)t1;
        }
    }
    if (kNorms) { *a = sa; *b = sb; }
}

// vt.row(3) of the SVD of A (rows a0..a3): tests/triangulation_ref.py jacobi_null_vector
__device__ void jacobi_null_vector(const float (&A)[4][4], float (&v)[4]) {
    float At[4][4], V[4][4];
    double W[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            At[i][k] = A[k][i];
            V[i][k] = i == k ? 1.f : 0.f;
            s += (double)A[k][i] * (double)A[k][i];
        }
        W[i] = s;
    }
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; sweep++) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = i + 1; j < 4; j++) {
                double a = W[i], b = W[j], p = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) p += (double)At[i][k] * (double)At[j][k];
                if (fabs(p) <= kEps * sqrt(a * b)) continue;
                p *= 2.0;
                const double beta = a - b, gamma = sqrt(p * p + beta * beta);
                double c, s;
                if (beta < 0.0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2.0);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2.0));
                    s = p / (gamma * c * 2.0);
                }
                rotate<true>(At, i, j, c, s, &a, &b);
                W[i] = a;
                W[j] = b;
                rotate<false>(V, i, j, c, s, nullptr, nullptr);
                changed = true;
            }
        }
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) s += (double)At[i][k] * (double)At[i][k];
        W[i] = sqrt(s);
    }
    // stable selection, descending: the first largest of the rest moves up; the last place's row is the answer
    int order[4] = {0, 1, 2, 3};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        int j = i;
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < 4; k++)
            if (wj < W[k]) { j = k; wj = W[k]; }
#pragma unroll
        for (int k = i + 1; k < 4; k++)
            if (k == j) {
                const double tw = W[i]; W[i] = W[k]; W[k] = tw;
                const int to = order[i]; order[i] = order[k]; order[k] = to;
            }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float x = V[0][k];
#pragma unroll
        for (int r = 1; r < 4; r++) x = order[3] == r ? V[r][k] : x;
        v[k] = x;
    }
}

// KeyFrame::UnprojectStereo: mvKeys, mvDepth, Twc = [Rcw^T | Ow]
__device__ __forceinline__ void unproject_stereo(const TriConsts& C, const float* T, const float* Ow, float u,
                                                 float v, float z, float (&X)[3]) {
    const float x = __fmul_rn(__fmul_rn(__fsub_rn(u, C.cx), z), C.invfx);
    const float y = __fmul_rn(__fmul_rn(__fsub_rn(v, C.cy), z), C.invfy);
    X[0] = row3(T[0], T[4], T[8], x, y, z, Ow[0]);
    X[1] = row3(T[1], T[5], T[9], x, y, z, Ow[1]);
    X[2] = row3(T[2], T[6], T[10], x, y, z, Ow[2]);
}

// :374-426 for one keyframe: true when the reprojection error is over its chi-square bound
__device__ __forceinline__ bool reprojection_fails(const TriConsts& C, const float* T, const float (&X)[3], float z,
                                                   float kx, float ky, int octave, float ur, bool stereo) {
    const float x = (float)(dot3(T[0], T[1], T[2], X[0], X[1], X[2]) + (double)T[3]);
    const float y = (float)(dot3(T[4], T[5], T[6], X[0], X[1], X[2]) + (double)T[7]);
    const double sigma2 = (double)level_entry(C.sigma2, octave);
    const float invz = (float)(1.0 / (double)z);
    const float u = __fmaf_rn(__fmul_rn(C.fx, x), invz, C.cx);
    const float v = __fmaf_rn(__fmul_rn(C.fy, y), invz, C.cy);
    const float eX = __fsub_rn(u, kx), eY = __fsub_rn(v, ky);
    const float e2 = __fmaf_rn(eX, eX, __fmul_rn(eY, eY));
    if (!stereo) return (double)e2 > 5.991 * sigma2;
    const float u_r = __fmaf_rn(-C.bf, invz, u);  // the current keyframe's mbf for both (:418)
    const float eR = __fsub_rn(u_r, ur);
    return (double)__fmaf_rn(eR, eR, e2) > 7.8 * sigma2;
}

__device__ void triangulate_match(const TriConsts& C, const spslam_tri_pair* P, const spslam_tri_side& S, int idx1,
                                  int idx2, spslam_tri_result* out) {
    const size_t o1 = (size_t)P->kf1 * S.cap + idx1, o2 = (size_t)P->kf2 * S.cap + idx2;
    const float* T1 = P->Tcw1;
    const float* T2 = P->Tcw2;
    const float k1x = S.keys_un[o1].x, k1y = S.keys_un[o1].y, k2x = S.keys_un[o2].x, k2y = S.keys_un[o2].y;
    const int oct1 = S.keys_un[o1].octave, oct2 = S.keys_un[o2].octave;
    const float ur1 = S.uright[o1], ur2 = S.uright[o2];
    const bool stereo1 = ur1 >= 0.f, stereo2 = ur2 >= 0.f;
    // the parallax between the rays (:313-330)
    const float xn1[2] = {__fmul_rn(__fsub_rn(k1x, C.cx), C.invfx), __fmul_rn(__fsub_rn(k1y, C.cy), C.invfy)};
    const float xn2[2] = {__fmul_rn(__fsub_rn(k2x, C.cx), C.invfx), __fmul_rn(__fsub_rn(k2y, C.cy), C.invfy)};
    const float r1x = row3(T1[0], T1[4], T1[8], xn1[0], xn1[1], 1.f, 0.f);
    const float r1y = row3(T1[1], T1[5], T1[9], xn1[0], xn1[1], 1.f, 0.f);
    const float r1z = row3(T1[2], T1[6], T1[10], xn1[0], xn1[1], 1.f, 0.f);
    const float r2x = row3(T2[0], T2[4], T2[8], xn2[0], xn2[1], 1.f, 0.f);
    const float r2y = row3(T2[1], T2[5], T2[9], xn2[0], xn2[1], 1.f, 0.f);
    const float r2z = row3(T2[2], T2[6], T2[10], xn2[0], xn2[1], 1.f, 0.f);
    const float cos_rays = (float)(dot3(r1x, r1y, r1z, r2x, r2y, r2z) / (norm3(r1x, r1y, r1z) * norm3(r2x, r2y, r2z)));
    float cos_s1 = __fadd_rn(cos_rays, 1.f), cos_s2 = cos_s1;
    if (stereo1 || stereo2) {  // cos(2*atan2(mb/2, depth)): the float overloads
        float sn, cs;
        libm::sincosf_(__fmul_rn(2.f, libm::atan2f_(C.mb / 2.f, S.depth[stereo1 ? o1 : o2])), &sn, &cs);
        if (stereo1) cos_s1 = cs; else cos_s2 = cs;
    }
    const float cos_stereo = cos_s2 < cos_s1 ? cos_s2 : cos_s1;  // std::min
    float X[3] = {0.f, 0.f, 0.f};
    int source = SPSLAM_TRI_FROM_SVD;
    if (cos_rays < cos_stereo && cos_rays > 0.f && (stereo1 || stereo2 || (double)cos_rays < 0.9998)) {
        float A[4][4], v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {  // xn*Tcw.row(2) - Tcw.row(k): a float multiply, a float subtract
            A[0][k] = __fsub_rn(__fmul_rn(xn1[0], T1[8 + k]), T1[k]);
            A[1][k] = __fsub_rn(__fmul_rn(xn1[1], T1[8 + k]), T1[4 + k]);
            A[2][k] = __fsub_rn(__fmul_rn(xn2[0], T2[8 + k]), T2[k]);
            A[3][k] = __fsub_rn(__fmul_rn(xn2[1], T2[8 + k]), T2[4 + k]);
        }
        jacobi_null_vector(A, v);
        if (v[3] == 0.f) { out->status = SPSLAM_TRI_W_ZERO; return; }           // :345
        const double inv_w = 1.0 / (double)v[3];
#pragma unroll
        for (int k = 0; k < 3; k++) X[k] = (float)((double)v[k] * inv_w);
    } else if (stereo1 && cos_s1 < cos_s2) {
        source = SPSLAM_TRI_FROM_STEREO_1;
        unproject_stereo(C, T1, P->Ow1, S.keys[o1].x, S.keys[o1].y, S.depth[o1], X);
    } else if (stereo2 && cos_s2 < cos_s1) {
        source = SPSLAM_TRI_FROM_STEREO_2;
        unproject_stereo(C, T2, P->Ow2, S.keys[o2].x, S.keys[o2].y, S.depth[o2], X);
    } else {
        out->status = SPSLAM_TRI_LOW_PARALLAX;                                   // :360
        return;
    }
    out->x = X[0]; out->y = X[1]; out->z = X[2];
    out->source = (uint8_t)source;
    const float z1 = (float)(dot3(T1[8], T1[9], T1[10], X[0], X[1], X[2]) + (double)T1[11]);
    if (z1 <= 0.f) { out->status = SPSLAM_TRI_BEHIND_1; return; }
    const float z2 = (float)(dot3(T2[8], T2[9], T2[10], X[0], X[1], X[2]) + (double)T2[11]);
    if (z2 <= 0.f) { out->status = SPSLAM_TRI_BEHIND_2; return; }
    if (reprojection_fails(C, T1, X, z1, k1x, k1y, oct1, ur1, stereo1)) { out->status = SPSLAM_TRI_REPROJ_1; return; }
    if (reprojection_fails(C, T2, X, z2, k2x, k2y, oct2, ur2, stereo2)) { out->status = SPSLAM_TRI_REPROJ_2; return; }
    // scale consistency (:428-441)
    const float dist1 = (float)norm3(__fsub_rn(X[0], P->Ow1[0]), __fsub_rn(X[1], P->Ow1[1]), __fsub_rn(X[2], P->Ow1[2]));
    const float dist2 = (float)norm3(__fsub_rn(X[0], P->Ow2[0]), __fsub_rn(X[1], P->Ow2[1]), __fsub_rn(X[2], P->Ow2[2]));
    if (dist1 == 0.f || dist2 == 0.f) { out->status = SPSLAM_TRI_ZERO_DIST; return; }
    const float ratio_dist = dist2 / dist1;
    const float ratio_octave = level_entry(C.scale, oct1) / level_entry(C.scale, oct2);
    if (__fmul_rn(ratio_dist, C.ratio_factor) < ratio_octave || ratio_dist > __fmul_rn(ratio_octave, C.ratio_factor)) {
        out->status = SPSLAM_TRI_SCALE;
        return;
    }
    out->status = SPSLAM_TRI_NEW;
}

__global__ __launch_bounds__(kThreads) void triangulate_kernel(const spslam_tri_pair* __restrict__ pairs,
                                                               spslam_tri_side S, TriConsts C,
                                                               const int32_t* __restrict__ match12, int mark,
                                                               spslam_tri_result* __restrict__ results,
                                                               int* __restrict__ n_new) {
    __shared__ int n_accepted;
    const int p = blockIdx.x, t = threadIdx.x, i = blockIdx.y * kThreads + t;
    const spslam_tri_pair* P = pairs + p;
    const int n1 = min(S.counts[P->kf1], S.cap), n2 = min(S.counts[P->kf2], S.cap);
    if (t == 0) n_accepted = 0;
    __syncthreads();
    if (i < n1) {
        const int m = match12[P->out_offset + i];
        spslam_tri_result r;
        r.x = r.y = r.z = 0.f;
        r.idx2 = m < 0 ? -1 : m;
        r.status = SPSLAM_TRI_NO_MATCH;
        r.source = SPSLAM_TRI_FROM_SVD;
        r.pad = 0;
        if (m >= 0 && m < n2) triangulate_match(C, P, S, i, m, &r);
        results[P->out_offset + i] = r;
        if (r.status == SPSLAM_TRI_NEW) {
            atomicAdd(&n_accepted, 1);
            if (mark) {  // AddMapPoint on both keyframes (:451-452), as the next neighbour's search sees it
                S.has_point[(size_t)P->kf1 * S.cap + i] = 1;
                S.has_point[(size_t)P->kf2 * S.cap + m] = 1;
            }
        }
    }
    __syncthreads();
    if (t == 0 && n_accepted) atomicAdd(&n_new[p], n_accepted);
}

}  // namespace tri

hipError_t triangulate_launch(int n_pairs, const spslam_tri_pair* pairs, const spslam_tri_side& side,
                              const TriConsts& C, const int32_t* match12, int mark, spslam_tri_result* results,
                              int* n_new, hipStream_t s) {
    if (n_pairs < 1 || side.cap < 1 || side.cap > 8192) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(n_new, 0, (size_t)n_pairs * sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tri::triangulate_kernel, dim3(n_pairs, (side.cap + tri::kThreads - 1) / tri::kThreads),
                       dim3(tri::kThreads), 0, s, pairs, side, C, match12, mark, results, n_new);
    return hipGetLastError();
}

}  // namespace spslam
