// What the ORBmatcher kernels share (match_kernels.hip: SearchByProjection, bow_kernels.hip: SearchByBoW):
// DescriptorDistance, the rotation histogram (src/ORBmatcher.cc:1601-1662) and the LDS bitmap of taken keypoints.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace spslam {
namespace orb_match {

constexpr int kHisto = 30;  // HISTO_LENGTH

// DescriptorDistance (src/ORBmatcher.cc:1647-1662): v_bcnt over the XOR of 8 dwords
__device__ __forceinline__ int hamming(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
__device__ __forceinline__ int hamming(const uint4& a0, const uint4& a1, const uint8_t* b) {
    return hamming(a0, a1, *(const uint4*)b, *(const uint4*)(b + 16));
}

// l-th entry of a per-level table held in kernel arguments (a select chain: no indexed copy of the table)
__device__ __forceinline__ float level_entry(const float (&t)[8], int l) {
    float x = t[0];
#pragma unroll
    for (int q = 1; q < 8; q++) x = l == q ? t[q] : x;
    return x;
}

// the rotation histogram's bin of a match: rot = a - b (+ 360 if negative), round(rot * factor), kHisto -> 0
__device__ __forceinline__ int rotation_bin(float a, float b) {
    const float factor = 1.0f / kHisto;
    float rot = __fsub_rn(a, b);
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    const int bin = (int)roundf(__fmul_rn(rot, factor));
    return bin == kHisto ? 0 : bin;
}

// ComputeThreeMaxima (src/ORBmatcher.cc:1601-1642)
__device__ inline void three_maxima(const int* h, int* i1, int* i2, int* i3) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < kHisto; i++) {
        const int s = h[i];
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            ind3 = ind2; ind2 = ind1; ind1 = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            ind3 = ind2; ind2 = i;
        } else if (s > max3) {
            max3 = s;
            ind3 = i;
        }
    }
    if (max2 < __fmul_rn(0.1f, (float)max1)) { ind2 = -1; ind3 = -1; }
    else if (max3 < __fmul_rn(0.1f, (float)max1)) ind3 = -1;
    *i1 = ind1; *i2 = ind2; *i3 = ind3;
}

// bitmap of taken keypoints, one bit per keypoint; bit_set is for one writer, bit_set_atomic for lanes that
// may share a word
__device__ __forceinline__ bool bit_test(const uint32_t* bits, int k) { return (bits[k >> 5] >> (k & 31)) & 1; }
__device__ __forceinline__ void bit_set(uint32_t* bits, int k) { bits[k >> 5] |= 1u << (k & 31); }
__device__ __forceinline__ void bit_set_atomic(uint32_t* bits, int k) { atomicOr(&bits[k >> 5], 1u << (k & 31)); }

}  // namespace orb_match
}  // namespace spslam
