// Fragment of lba_g2o.hip, included inside its namespace; not a standalone header.  Pose masks.
// A set of free poses (Hessian indices) as kPW 64-bit words; with kPW = 1 every operation is the plain uint64_t one.
struct PMask {
    uint64_t w[kPW];
};
__device__ __forceinline__ PMask pm_zero() {
    PMask m;
#pragma unroll
    for (int k = 0; k < kPW; k++) m.w[k] = 0ull;
    return m;
}
__device__ __forceinline__ PMask pm_bit(int i) {
    PMask m;
    if constexpr (kPW == 1) {
        m.w[0] = 1ull << i;
    } else {
#pragma unroll
        for (int k = 0; k < kPW; k++) m.w[k] = (i >> 6) == k ? 1ull << (i & 63) : 0ull;
    }
    return m;
}
__device__ __forceinline__ bool pm_test(const PMask& m, int i) {
    if constexpr (kPW == 1) {
        return (m.w[0] >> i) & 1ull;
    } else {
        uint64_t v = m.w[0];
#pragma unroll
        for (int k = 1; k < kPW; k++) v = (i >> 6) == k ? m.w[k] : v;
        return (v >> (i & 63)) & 1ull;
    }
}
__device__ __forceinline__ void pm_set(PMask& m, int i) {
    if constexpr (kPW == 1) {
        m.w[0] |= 1ull << i;
    } else {
#pragma unroll
        for (int k = 0; k < kPW; k++) m.w[k] |= (i >> 6) == k ? 1ull << (i & 63) : 0ull;
    }
}
__device__ __forceinline__ PMask pm_and(PMask a, const PMask& b) {
#pragma unroll
    for (int k = 0; k < kPW; k++) a.w[k] &= b.w[k];
    return a;
}
__device__ __forceinline__ PMask pm_or(PMask a, const PMask& b) {
#pragma unroll
    for (int k = 0; k < kPW; k++) a.w[k] |= b.w[k];
    return a;
}
__device__ __forceinline__ PMask pm_andnot(PMask a, const PMask& b) {
#pragma unroll
    for (int k = 0; k < kPW; k++) a.w[k] &= ~b.w[k];
    return a;
}
// bits [0, i), 0 <= i < 64 kPW (the narrow instance: (1 << i) - 1, i < 64)
__device__ __forceinline__ PMask pm_below(int i) {
    PMask m;
    if constexpr (kPW == 1) {
        m.w[0] = (1ull << i) - 1ull;
    } else {
#pragma unroll
        for (int k = 0; k < kPW; k++) {
            const int c = i - 64 * k;
            m.w[k] = c >= 64 ? ~0ull : c <= 0 ? 0ull : (1ull << c) - 1ull;
        }
    }
    return m;
}
// bits [0, n), 0 <= n <= 64 kPW
__device__ __forceinline__ PMask pm_first_n(int n) {
    PMask m;
#pragma unroll
    for (int k = 0; k < kPW; k++) {
        const int c = n - 64 * k;
        m.w[k] = c >= 64 ? ~0ull : c <= 0 ? 0ull : (1ull << c) - 1ull;
    }
    return m;
}
__device__ __forceinline__ int pm_popc(const PMask& m) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < kPW; k++) c += __popcll(m.w[k]);
    return c;
}
__device__ __forceinline__ int pm_popc_below(const PMask& m, int i) { return pm_popc(pm_and(m, pm_below(i))); }
__device__ __forceinline__ bool pm_any(const PMask& m) {
    uint64_t v = m.w[0];
#pragma unroll
    for (int k = 1; k < kPW; k++) v |= m.w[k];
    return v != 0ull;
}
__device__ __forceinline__ bool pm_eq(const PMask& a, const PMask& b) {
    bool e = true;
#pragma unroll
    for (int k = 0; k < kPW; k++) e = e && a.w[k] == b.w[k];
    return e;
}
// lowest set bit (the mask must not be empty)
__device__ __forceinline__ int pm_ffs(const PMask& m) {
    if constexpr (kPW == 1) {
        return __ffsll((unsigned long long)m.w[0]) - 1;
    } else {
        int r = -1;
#pragma unroll
        for (int k = kPW - 1; k >= 0; k--)
            if (m.w[k]) r = 64 * k + __ffsll((unsigned long long)m.w[k]) - 1;
        return r;
    }
}
// the mask without its lowest set bit
__device__ __forceinline__ void pm_pop(PMask& m) {
    if constexpr (kPW == 1) {
        m.w[0] &= m.w[0] - 1;
    } else {
        bool done = false;
#pragma unroll
        for (int k = 0; k < kPW; k++)
            if (!done && m.w[k]) {
                m.w[k] &= m.w[k] - 1;
                done = true;
            }
    }
}
// pose masks in global memory (word by word: an address-space-qualified PMask has no copy constructor)
__device__ __forceinline__ PMask pm_ld(const PMask GL* p) {
    const uint64_t GL* q = (const uint64_t GL*)p;
    PMask m;
#pragma unroll
    for (int k = 0; k < kPW; k++) m.w[k] = q[k];
    return m;
}
__device__ __forceinline__ void pm_st(PMask GL* p, const PMask& m) {
    uint64_t GL* q = (uint64_t GL*)p;
#pragma unroll
    for (int k = 0; k < kPW; k++) q[k] = m.w[k];
}
