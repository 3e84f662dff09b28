// Wave-scope helpers shared by the kernels: the in-wave LDS hand-off and the integer xor butterflies.
// Floating-point reductions are not here on purpose: their association order belongs to each kernel's
// bit-exact contract and stays written out where it is used.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace spslam {

__device__ __forceinline__ void wave_sync() {  // LDS written by this wave, visible to this wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum / minimum over the 64 lanes, the result in every lane
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

}  // namespace spslam
