// LocalBundleAdjustment's g2o edge arithmetic and workgroup primitives, once for both orders (lba_g2o.hip,
// lba_kernels.hip).  The expressions are the oracle's (oracle/lba_oracle.cpp); they decide bit-exactness, so
// neither translation unit restates them.  Functions take their operands as arguments: each file's context struct
// (G, Ctx) gathers them in thin wrappers of its own.  Pointer parameters are templates on the pointee type, so a
// caller's address_space(1) pointer stays a global-memory pointer (a generic one would make every access FLAT).
#pragma once
#include "g2o_device.h"
#include "lba_launch.h"

namespace spslam {
namespace edge_math {

using namespace g2od;

// ---------------------------------------------------------------- workgroup primitives
// kWaves waves of 64; `wsum` / `red` is the caller's LDS scratch (one slot per wave).  Two barriers each.
template <int kWaves>
__device__ __forceinline__ int block_scan(int v, int* total, int (&wsum)[kWaves]) {  // exclusive; *total = sum
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < kWaves; j++) {
        const int q = wsum[j];
        if (j < w) base += q;
        tot += q;
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}
template <int kWaves, int kCols>
__device__ __forceinline__ double block_max(double v, double (&red)[kWaves][kCols]) {  // max of non-negative values
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) red[w][0] = v;
    __syncthreads();
    double m = 0.0;
#pragma unroll
    for (int j = 0; j < kWaves; j++) m = fmax(m, red[j][0]);
    __syncthreads();
    return m;
}

// ---------------------------------------------------------------- edge math (oracle/lba_oracle.cpp)
template <class PD>
__device__ __forceinline__ SE3 load_pose(const PD* p) { return SE3{Q{p[0], p[1], p[2], p[3]}, V3{p[4], p[5], p[6]}}; }
template <class PD>
__device__ __forceinline__ void store_pose(PD* p, const SE3& T) {
    p[0] = T.r.w; p[1] = T.r.x; p[2] = T.r.y; p[3] = T.r.z; p[4] = T.t.x; p[5] = T.t.y; p[6] = T.t.z;
}
template <class PF>
__device__ __forceinline__ P4 plane_from_f(const PF* c) {  // Converter::toPlane3D (flip d < 0) + Plane3D(v)
    P4 p{{c[0], c[1], c[2], c[3]}};
    if (c[3] < 0.0f)
        for (int i = 0; i < 4; i++) p.c[i] = -p.c[i];
    p_normalize(p.c);
    return p;
}
__device__ __forceinline__ P4 plane_transform(const SE3& T, const P4& w) {  // operator*(Isometry3D, Plane3D)
    const M3 R = q_to_rot(T.r);
    const V3 n2 = mv(R, V3{w.c[0], w.c[1], w.c[2]});
    P4 v{{n2.x, n2.y, n2.z, w.c[3] - dot(T.t, n2)}};
    if (v.c[3] < 0.0)
        for (int i = 0; i < 4; i++) v.c[i] = -v.c[i];
    p_normalize(v.c);
    return v;
}
// edge types: 0 mono point, 1 stereo point, 2 plane, 3 parallel plane, 4 vertical plane
__device__ __forceinline__ int edge_dim(int type) { return type == 0 ? 2 : (type <= 2 ? 3 : 2); }
// the information matrix's diagonal; inv_sigma2 is the point observation's (read for t <= 1 only)
__device__ __forceinline__ void info_of(const LbaConsts& C, int t, float inv_sigma2, double* info) {
    if (t <= 1) {
        const double s = (double)inv_sigma2;
        info[0] = info[1] = info[2] = s;
    } else if (t == 2) {
        info[0] = info[1] = C.angle_info; info[2] = C.dis_info;
    } else {
        info[0] = info[1] = t == 3 ? C.par_info : C.ver_info;
        info[2] = 0;
    }
}
template <class PE>
__device__ __forceinline__ double chi2_of(const PE* err, const double* info, int dim) {  // e . (Omega e)
    double s = 0;
    for (int i = 0; i < dim; i++) s += err[i] * (info[i] * err[i]);
    return s;
}
__device__ __forceinline__ double delta_of(const LbaConsts& C, int t) {
    return t == 0 ? C.delta_mono : t == 1 ? C.delta_stereo : t == 2 ? C.delta_plane : C.delta_vp;
}
// A point edge's operands: the keyframe's pose and intrinsics, the point, the observation
struct PointIn {
    SE3 T;
    double X[3];
    float u, v, ur, isg, fx, fy, cx, cy, bf;
};
// EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ::computeError (t = 0 mono: err[2] = 0; t = 1 stereo)
__device__ __forceinline__ void point_edge_error(int t, const PointIn& a, double* err) {
    const V3 p = q_rot(a.T.r, V3{a.X[0], a.X[1], a.X[2]}) + a.T.t;
    if (t == 0) {
        err[0] = (double)a.u - (p.x / p.z * (double)a.fx + (double)a.cx);
        err[1] = (double)a.v - (p.y / p.z * (double)a.fy + (double)a.cy);
        err[2] = 0.0;
    } else {
        const float invz = (float)(1.0f / p.z);
        const double r0 = p.x * invz * (double)a.fx + (double)a.cx, r1 = p.y * invz * (double)a.fy + (double)a.cy;
        const double r2 = r0 - (double)(a.bf * invz);  // cam_project(..., const float& bf)
        err[0] = (double)a.u - r0;
        err[1] = (double)a.v - r1;
        err[2] = (double)a.ur - r2;
    }
}
// EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ::linearizeOplus (types_six_dof_expmap.cpp:103-234): A (landmark,
// 3 x 3) and B (pose, 3 x 6), row 2 zero for a mono edge.  needA false (a uniform branch): only B is formed.
// T: the keyframe's pose, fx, fy, bf: its intrinsics, X: the point (3 doubles).
template <class PD>
__device__ __forceinline__ void point_edge_jacobians(int t, const SE3& T, double fx, double fy, double bf, const PD* X,
                                                     double (&A)[3][3], double (&B)[3][6], bool needA = true) {
    const V3 p = q_rot(T.r, V3{X[0], X[1], X[2]}) + T.t;
    const double x = p.x, y = p.y, z = p.z, z_2 = z * z;
    if (!needA) {
    } else if (t == 0) {
        const M3 R = q_to_rot(T.r);
        const double tmp[2][3] = {{fx, 0, -x / z * fx}, {0, fy, -y / z * fy}};
        const double s = -1. / z;
        for (int r = 0; r < 2; r++) {
            const double t0 = s * tmp[r][0], t1 = s * tmp[r][1], t2 = s * tmp[r][2];
            for (int q = 0; q < 3; q++) A[r][q] = t0 * R.a[q] + t1 * R.a[3 + q] + t2 * R.a[6 + q];
        }
        A[2][0] = A[2][1] = A[2][2] = 0.0;
    } else {
        const M3 R = q_to_rot(T.r);
        for (int q = 0; q < 3; q++) {
            A[0][q] = -fx * R.a[q] / z + fx * x * R.a[6 + q] / z_2;
            A[1][q] = -fy * R.a[3 + q] / z + fy * y * R.a[6 + q] / z_2;
            A[2][q] = A[0][q] - bf * R.a[6 + q] / z_2;
        }
    }
    B[0][0] = x * y / z_2 * fx; B[0][1] = -(1 + (x * x / z_2)) * fx; B[0][2] = y / z * fx;
    B[0][3] = -1. / z * fx; B[0][4] = 0; B[0][5] = x / z_2 * fx;
    B[1][0] = (1 + y * y / z_2) * fy; B[1][1] = -x * y / z_2 * fy; B[1][2] = -x / z * fy;
    B[1][3] = 0; B[1][4] = -1. / z * fy; B[1][5] = y / z_2 * fy;
    if (t == 1) {
        B[2][0] = B[0][0] - bf * y / z_2; B[2][1] = B[0][1] + bf * x / z_2; B[2][2] = B[0][2];
        B[2][3] = B[0][3]; B[2][4] = 0; B[2][5] = B[0][5] - bf / z_2;
    } else {
        for (int q = 0; q < 6; q++) B[2][q] = 0.0;
    }
}
// The relabelling's depth test: the point (st: 3 doubles) in front of the camera at T, or the transformed plane's
// (st: 4 doubles) distance negative
template <class PD>
__device__ __forceinline__ bool depth_positive(const SE3& T, bool point, const PD* st) {
    if (point) return (q_rot(T.r, V3{st[0], st[1], st[2]}) + T.t).z > 0.0;
    return -plane_transform(T, P4{{st[0], st[1], st[2], st[3]}}).c[3] > 0;
}
// Eigen compute_inverse<Matrix3d> (cofactors), r row-major
__device__ __forceinline__ void inverse3(const double (&m)[3][3], double* r) {
    auto cof = [&](int i, int j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
    };
    const double c0 = cof(0, 0), c1 = cof(1, 0), c2 = cof(2, 0);
    const double det = (c0 * m[0][0] + c1 * m[1][0]) + c2 * m[2][0];
    const double invdet = 1.0 / det;
    r[0] = c0 * invdet; r[1] = c1 * invdet; r[2] = c2 * invdet;
    r[3] = cof(0, 1) * invdet; r[4] = cof(1, 1) * invdet; r[5] = cof(2, 1) * invdet;
    r[6] = cof(0, 2) * invdet; r[7] = cof(1, 2) * invdet; r[8] = cof(2, 2) * invdet;
}

}  // namespace edge_math
}  // namespace spslam
