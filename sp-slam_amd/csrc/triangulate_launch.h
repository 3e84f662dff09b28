// Host-side entry point of triangulate_kernels.hip (LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:298-443)
// and the float readings the two CreateNewMapPoints kernels share.
#pragma once
#include <hip/hip_runtime.h>

#include "bow_launch.h"

namespace spslam {
namespace tri {

// one row of a cv::Mat product (+ addend): summed in double, rounded once
__device__ __forceinline__ float row3(float r0, float r1, float r2, float x, float y, float z, float c) {
    double s = (double)r0 * (double)x;
    s += (double)r1 * (double)y;
    s += (double)r2 * (double)z;
    s += (double)c;
    return (float)s;
}

// Mat::dot of three floats: a double
__device__ __forceinline__ double dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    double s = (double)a0 * (double)b0;
    s += (double)a1 * (double)b1;
    s += (double)a2 * (double)b2;
    return s;
}

// cv::norm of three floats: squares accumulated in float, root in double
__device__ __forceinline__ double norm3(float x, float y, float z) {
    float s = __fmul_rn(x, x);
    s = __fadd_rn(s, __fmul_rn(y, y));
    s = __fadd_rn(s, __fmul_rn(z, z));
    return sqrt((double)s);
}

}  // namespace tri

// One record per key-1 feature of every pair; n_new is cleared on the stream first.  mark: set the has-point bytes
// of accepted records.
hipError_t triangulate_launch(int n_pairs, const spslam_tri_pair* pairs, const spslam_tri_side& side,
                              const TriConsts& C, const int32_t* match12, int mark, spslam_tri_result* results,
                              int* n_new, hipStream_t s);

}  // namespace spslam
