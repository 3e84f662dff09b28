// Fragment of lba_g2o.hip, included inside its namespace; not a standalone header.  The factorisation and solve.
// LinearSolverEigen::solve: SimplicialLDLT::factorize + solve on wave 0.  Row r of the permuted system lives in
// lane r & 63, register r >> 6.  LD: L column-major (LD[i n + r] = L(r, i)), LB: L's column structures (bitsets),
// RS / RO: the rows' pattern orders, PI: Pinv.
// SP: the reduced system's upper triangle, packed column by column (SP[c (c + 1) / 2 + r] = S(r, c), r <= c) when
// kPacked, else g.S (dense, row-major)
template <int kC, bool kPacked, class PD, class PU, class PI_, class PS>
__device__ __forceinline__ void factor_body(PD* LD, const PU* LB, const PI_* RO, const PI_* RS, const PI_* PI,
                                            const PS* SP, double* PR /* LDS, 64 doubles */,
                                            const double* Dpre = nullptr /* factorised already (factor_dense) */) {
    const G& g = lbg_g;
    Sh& s = lbg_s;
    const int lane = threadIdx.x & 63;
    const int n = 6 * s.np;
    double Dg[kC];
#pragma unroll
    for (int m = 0; m < kC; m++) Dg[m] = 0.0;
    bool ok = true;
    if (Dpre) {  // L and D from factor_dense; s.ok set there
#pragma unroll
        for (int m = 0; m < kC; m++)
            if (64 * m + lane < n) Dg[m] = Dpre[64 * m + lane];
        ok = s.ok;
    }
    for (int k = 0; k < (Dpre ? 0 : n); k++) {
        const int ok_ = PI[k], qk = ok_ / 6;
        double y[kC];
#pragma unroll
        for (int m = 0; m < kC; m++) {
            const int r = 64 * m + lane;
            y[m] = 0.0;
            if (r <= k) {
                const int orr = PI[r];
                if (coupled(s, orr / 6, qk)) {
                    const int lo = min(orr, ok_), hi = max(orr, ok_);
                    y[m] = 0.0 + (kPacked ? SP[(hi * (hi + 1)) / 2 + lo] : SP[(size_t)lo * n + hi]);
                }
            }
        }
        double d = pick(y, k) * 1.0 + 0.0;
        const int t0 = RO[k], t1 = RO[k + 1];
        // The row's pattern order 64 entries at a time in registers (lane q: entry q of the piece), with each
        // entry's LDS byte offsets of its L column and structure word and its lane / register in y precomputed
        // per lane: a step reads them with v_readlane at a loop-counter lane and uses them only in vector
        // address arithmetic and as readlane lane selects, so no scalar instruction waits on a vector result
        // inside the chain.  The columns of L and the structure words of the next kRing steps are in flight
        // while a step runs (a ring of operand sets, each written only by its fetch and read only by its step).
        // Past the piece's end the entries repeat its last one with the structure word LB[n kNW] (zero): masked
        // steps.  A column's rows past n read the next one's (in the LDS layout; unused: masked by r < k).
        // (a divisor of 64: a piece's last ring round ends at step 63 -- with 6, a full piece of 64 entries ran two
        // steps past it, on entry 63's operands refetched and entry 0's lane select).  Global-memory pieces are L2
        // latency bound: a deeper ring where the registers allow it (kC <= 3: 8 operand sets, kC <= 6: 4)
        constexpr int kRing = kPacked ? 8 : kC <= 3 ? 8 : kC <= 6 ? 4 : 2;
        const char* LDc = (const char*)LD;
        const char* LBc = (const char*)LB;
        // rows r < k of register m as a lane mask: a step's update condition is one bit test (a select, no
        // exec-mask branch)
        uint64_t km[kC];
#pragma unroll
        for (int m = 0; m < kC; m++) {
            const int c = k - 64 * m;
            km[m] = c >= 64 ? ~0ull : c <= 0 ? 0ull : (1ull << c) - 1ull;
        }
        auto stepf = [&](int lsel, int rsel, const double (&v)[kC], const uint64_t (&wr)[kC]) __attribute__((always_inline)) {
            // (the structure words opaque until here: otherwise the compiler masks each one as soon as its load is
            // issued -- a wait for the LDS read every step, which defeats the ring)
            uint64_t w[kC];
#pragma unroll
            for (int m = 0; m < kC; m++) {
                w[m] = wr[m];
                asm volatile("" : "+v"(w[m]));
            }
            double yi = rl(y[0], lsel);
#pragma unroll
            for (int m = 1; m < kC; m++) {
                const double q = rl(y[m], lsel);
                yi = rsel == m ? q : yi;
            }
#pragma unroll
            for (int m = 0; m < kC; m++) {
                const double nv = y[m] - v[m] * yi;
                y[m] = (((w[m] & km[m]) >> lane) & 1ull) ? nv : y[m];
            }
        };
#ifdef SPSLAM_LBG_DIAG
        const long long c0 = clock64();
#endif
        for (int p0 = t0; p0 < t1; p0 += 64) {
            const int ns = min(64, t1 - p0);
            const int rsv = RS[p0 + min(lane, ns - 1)];
            const int cofs = rsv * n * 8;                                   // L column, bytes
            const int wofs = (lane < ns ? rsv : n) * (kNW * 8);             // structure words (past the end: zero)
            const int lsel = rsv & 63, rsel = rsv >> 6;                    // y's lane / register of the entry
            auto fetch = [&](int j, double (&v)[kC], uint64_t (&w)[kC]) __attribute__((always_inline)) {
                const int co = __builtin_amdgcn_readlane(cofs, j);
                int wo = __builtin_amdgcn_readlane(wofs, j);
                asm volatile("v_mov_b32 %0, %1" : "=v"(wo) : "s"(wo));  // the address sum in a vector op
#pragma unroll
                for (int m = 0; m < kC; m++) {
                    const int r = 64 * m + lane;
                    v[m] = (kPacked || r < n) ? *(const PD*)(LDc + co + 8 * r) : 0.0;
                    w[m] = *(const PU*)(LBc + wo + 8 * m);
                }
            };
            double v[kRing][kC];
            uint64_t w[kRing][kC];
#pragma unroll
            for (int q = 0; q < kRing; q++) fetch(min(q, 63), v[q], w[q]);
            for (int j = 0; j < ns; j += kRing) {
#pragma unroll
                for (int q = 0; q < kRing; q++) {
                    stepf(__builtin_amdgcn_readlane(lsel, j + q), __builtin_amdgcn_readlane(rsel, j + q), v[q], w[q]);
                    fetch(min(j + q + kRing, 63), v[q], w[q]);
                }
            }
        }
#ifdef SPSLAM_LBG_DIAG
        const long long c1 = clock64();
        if (lane == 0) { s.dg[6] += c1 - c0; s.dg[8] += t1 - t0; }
#endif
        double pr[kC];
#pragma unroll
        for (int m = 0; m < kC; m++) {
            const int r = 64 * m + lane;
            pr[m] = 0.0;
            if (r < k && bit_of(LB + (size_t)r * kNW, k)) {
                const double l = y[m] / Dg[m];
                LD[(size_t)r * n + k] = l;
                pr[m] = l * y[m];
            }
        }
        // d -= l_ki y_i in pattern order: the piece's terms gathered into pattern order across the lanes
        // (ds_bpermute), then subtracted lane by lane (loop-counter readlanes, off the dependent chain)
        for (int p0 = t0; p0 < t1; p0 += 64) {
            const int ns = min(64, t1 - p0);
            const int rsv = RS[p0 + min(lane, ns - 1)];
            const int src = (rsv & 63) * 4;
            double pv = 0.0;
#pragma unroll
            for (int m = 0; m < kC; m++) {
                const int lo = __builtin_amdgcn_ds_bpermute(src, __double2loint(pr[m]));
                const int hi = __builtin_amdgcn_ds_bpermute(src, __double2hiint(pr[m]));
                pv = (rsv >> 6) == m ? __hiloint2double(hi, lo) : pv;
            }
            // lane q's term into LDS slot q, then every lane subtracts the slots in order (broadcast reads:
            // no cross-lane register moves on the chain)
            PR[lane] = pv;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            int j = 0;
            for (; j + 8 <= ns; j += 8) {
                double a[8];
#pragma unroll
                for (int q = 0; q < 8; q++) a[q] = PR[j + q];
#pragma unroll
                for (int q = 0; q < 8; q++) d -= a[q];
            }
            for (; j < ns; j++) d -= PR[j];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
#ifdef SPSLAM_LBG_DIAG
        if (lane == 0) s.dg[7] += clock64() - c1;
#endif
#pragma unroll
        for (int m = 0; m < kC; m++)
            if (64 * m + lane == k) Dg[m] = d;
        if (d == 0.0) {
            ok = false;
            break;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane == 0 && !Dpre) s.ok = ok;
#ifdef SPSLAM_LBG_DIAG
    if (lane == 0) s.dg[4] = wall_clock64();
#endif
    if (!ok) return;
    // x = P b; L x = x; x = D^-1 x; L^T x = x; x = P^-1 x
    const bool haveL = RO[n] > 0;
    double tv[kC];
#pragma unroll
    for (int m = 0; m < kC; m++) {
        const int r = 64 * m + lane;
        tv[m] = r < n ? g.bs[PI[r]] : 0.0;
    }
    if (haveL)
        for (int i = 0; i < n; i++) {
            const double tmp = pick(tv, i);
            if (tmp != 0.0) {
                const auto* cb = LB + (size_t)i * kNW;
#pragma unroll
                for (int m = 0; m < kC; m++) {
                    const int r = 64 * m + lane;
                    if ((cb[m] >> lane) & 1ull) tv[m] = tv[m] - tmp * LD[(size_t)i * n + r];
                }
            }
        }
#pragma unroll
    for (int m = 0; m < kC; m++)
        if (64 * m + lane < n) tv[m] = (1.0 / Dg[m]) * tv[m];
    if (haveL)
        for (int i = n - 1; i >= 0; i--) {
            const auto* cb = LB + (size_t)i * kNW;
            double pr[kC];
#pragma unroll
            for (int m = 0; m < kC; m++) {
                const int r = 64 * m + lane;
                pr[m] = ((cb[m] >> lane) & 1ull) ? LD[(size_t)i * n + r] * tv[m] : 0.0;
            }
            double tmp = pick(tv, i);
#pragma unroll
            for (int m = 0; m < kC; m++) {
                uint64_t bits = (uint64_t)(uint32_t)uni((int)(uint32_t)cb[m]) | ((uint64_t)(uint32_t)uni((int)(cb[m] >> 32)) << 32);
                while (bits) {
                    const int r = __ffsll((unsigned long long)bits) - 1;
                    tmp -= rl(pr[m], r);
                    bits &= bits - 1;
                }
            }
#pragma unroll
            for (int m = 0; m < kC; m++)
                if (64 * m + lane == i) tv[m] = tmp;
        }
#pragma unroll
    for (int m = 0; m < kC; m++) {
        const int r = 64 * m + lane;
        if (r < n) g.x[PI[r]] = tv[m];
    }
}

// byte offsets of the factorisation's LDS copy (n <= kLdsN): L, its column structures, the rows' pattern orders
// (offsets, indices), P^-1, S packed
// (and factor_dense's pivots D and per-row progress PG, + a failure flag)
struct FactorLds { size_t LB, RO, RS, PI, SP, PR, D, PG, end; };
__device__ __forceinline__ FactorLds factor_lds(int n) {
    FactorLds f;
    f.LB = (size_t)n * n * 8;
    f.RO = f.LB + (size_t)(n + 1) * kNW * 8;  // row n: LB[n kNW ..] = 0
    f.RS = f.RO + (size_t)(n + 1) * 4;
    f.PI = f.RS + (size_t)((n * (n + 1)) / 2 + 1) * 4;
    f.SP = (f.PI + (size_t)n * 4 + 7) & ~(size_t)7;
    f.PR = f.SP + (size_t)((n * (n + 1)) / 2) * 8;
    f.D = f.PR + 64 * 8;
    f.PG = f.D + (size_t)n * 8;
    f.end = f.PG + (size_t)(n + 1) * 4;
    return f;
}
static_assert((size_t)kLdsN * kLdsN * 8 + ((kLdsN + 1) * kNW) * 8 + (kLdsN + 1) * 4 + (kLdsN * (kLdsN + 1) / 2 + 1) * 4 +
                  kLdsN * 4 + 8 + (kLdsN * (kLdsN + 1) / 2) * 8 + 64 * 8 + kLdsN * 8 + (kLdsN + 1) * 4 <= (size_t)kDyn,
              "the factorisation's LDS copy");

// SimplicialLDLT::factorize for a fully dense reduced system in the natural order (every pose coupled with every
// other; AMD then returns the identity and the elimination tree is a chain, so row k's pattern order is 0 .. k - 1
// and column i's structure every row below i), pipelined over the workgroup's waves: row k on wave k mod kW.  Row k
// runs Eigen's up-looking steps exactly as factor_body does -- for i = 0 .. k - 1: y_i read, y_r -= L(r, i) y_i for
// i < r < k, then l_ki = y_i / D_i and d -= l_ki y_i (the same pivot-update order as factor_body's pattern-order
// chain) -- and publishes L(k, i) at its step i and D_k when it ends.  Its step i needs L(r, i) for every r < k: row
// k - 1 has passed step i (PG[k - 1] > i) only after row k - 2 had, and so on, so one progress word per row orders
// them.  Same arithmetic, same order, rows overlapped.
template <int kC>
__device__ __noinline__ void factor_dense() {
    Sh& s = lbg_s;
    const int n = 6 * s.np;
    const FactorLds f = factor_lds(n);
    double* LD = (double*)lbg_dyn;
    const double* SP = (const double*)(lbg_dyn + f.SP);
    double* D = (double*)(lbg_dyn + f.D);
    volatile int* PG = (volatile int*)(lbg_dyn + f.PG);
    volatile int* FL = PG + n;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int k = t; k <= n; k += kT) PG[k] = 0;  // (PG[n] = FL)
    __syncthreads();
    for (int k = w; k < n; k += kW) {
        double y[kC];
#pragma unroll
        for (int m = 0; m < kC; m++) {
            const int r = 64 * m + lane;
            y[m] = r <= k ? 0.0 + SP[(k * (k + 1)) / 2 + r] : 0.0;
        }
        double d = pick(y, k) * 1.0 + 0.0;
        int seen = 0;
        bool failed = false;
        for (int i = 0; i < k; i++) {
            while (seen <= i) {  // row k - 1 has published L(k - 1, i)
                seen = __builtin_amdgcn_readfirstlane(PG[k - 1]);
                if (seen <= i) {
                    if (*FL) { failed = true; break; }
                    __builtin_amdgcn_s_sleep(0);
                }
            }
            if (failed) break;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const double yi = pick(y, i);
            const double Di = D[i];
            double v[kC];
#pragma unroll
            for (int m = 0; m < kC; m++) v[m] = LD[(size_t)i * n + 64 * m + lane];  // L(r, i), rows r < k published
            const double l = yi / Di;
#pragma unroll
            for (int m = 0; m < kC; m++) {
                const int r = 64 * m + lane;
                const double nv = y[m] - v[m] * yi;
                y[m] = (r > i && r < k) ? nv : y[m];
            }
            d -= l * yi;
            if (lane == 0) LD[(size_t)i * n + k] = l;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) PG[k] = i + 1;
        }
        if (failed) break;
        if (d == 0.0) {  // Eigen stops at a zero pivot (ok = false); the other rows see the flag and stop
            if (lane == 0) *FL = 1;
            break;
        }
        if (lane == 0) D[k] = d;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) PG[k] = k + 1;
    }
    __syncthreads();
    if (t == 0) s.ok = *FL == 0;
    __syncthreads();
}

// The same pipelined factorisation for dense systems too large for factor_dense's LDS copy (kLdsN < n <= kPackN,
// e.g. a window of 25 free poses, n = 150): L packed column by column in LDS (column i's rows i + 1 .. n - 1, a guard
// in front so that the masked reads of rows <= i stay in range), S read from global memory once per row, D and the
// progress words in LDS.  Then the solve (factor_body's order with every column's structure "all rows below").
constexpr int kPackN = 180;
__host__ __device__ constexpr int pk_col(int i, int n) { return (i * (2 * n - i - 1)) / 2 - i - 1 + n; }  // L(r, i) at + r
__host__ __device__ constexpr size_t pk_words(int n, int kC) { return (size_t)n + (size_t)n * (n - 1) / 2 + 64 * kC; }
static_assert((pk_words(kPackN, 3) + kPackN) * 8 + (kPackN + 1) * 4 <= (size_t)kDyn, "packed dense factorisation");
template <int kC>
__device__ __noinline__ void factor_dense_packed() {
    const G& g = lbg_g;
    Sh& s = lbg_s;
    const int n = 6 * s.np;
    double* LP = (double*)lbg_dyn;
    double* D = LP + pk_words(n, kC);
    volatile int* PG = (volatile int*)(D + n);
    volatile int* FL = PG + n;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int k = t; k <= n; k += kT) PG[k] = 0;  // (PG[n] = FL)
    __syncthreads();
    for (int k = w; k < n; k += kW) {
        double y[kC];
#pragma unroll
        for (int m = 0; m < kC; m++) {
            const int r = 64 * m + lane;
            y[m] = r <= k ? 0.0 + g.S[(size_t)r * n + k] : 0.0;
        }
        double d = pick(y, k) * 1.0 + 0.0;
        int seen = 0;
        bool failed = false;
        for (int i = 0; i < k; i++) {
            while (seen <= i) {  // row k - 1 has published L(k - 1, i)
                seen = __builtin_amdgcn_readfirstlane(PG[k - 1]);
                if (seen <= i) {
                    if (*FL) { failed = true; break; }
                    __builtin_amdgcn_s_sleep(0);
                }
            }
            if (failed) break;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const double yi = pick(y, i);
            const double Di = D[i];
            const double* col = LP + pk_col(i, n);
            double v[kC];
#pragma unroll
            for (int m = 0; m < kC; m++) v[m] = col[64 * m + lane];  // L(r, i): rows i < r < k published
            const double l = yi / Di;
#pragma unroll
            for (int m = 0; m < kC; m++) {
                const int r = 64 * m + lane;
                const double nv = y[m] - v[m] * yi;
                y[m] = (r > i && r < k) ? nv : y[m];
            }
            d -= l * yi;
            if (lane == 0) LP[pk_col(i, n) + k] = l;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) PG[k] = i + 1;
        }
        if (failed) break;
        if (d == 0.0) {  // Eigen stops at a zero pivot (ok = false); the other rows see the flag and stop
            if (lane == 0) *FL = 1;
            break;
        }
        if (lane == 0) D[k] = d;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) PG[k] = k + 1;
    }
    __syncthreads();
    if (t == 0) s.ok = *FL == 0;
    __syncthreads();
}
// x = P b; L x = x; x = D^-1 x; L^T x = x; x = P^-1 x (factor_body's solve, every column's structure the rows below it);
// one wave
template <int kC>
__device__ __noinline__ void solve_dense_packed() {
    const G& g = lbg_g;
    const Sh& s = lbg_s;
    if (!s.ok) return;
    const int n = 6 * s.np, lane = threadIdx.x & 63;
    const double* LP = (const double*)lbg_dyn;
    const double* D = LP + pk_words(n, kC);
    double tv[kC], Dg[kC];
#pragma unroll
    for (int m = 0; m < kC; m++) {
        const int r = 64 * m + lane;
        tv[m] = r < n ? g.bs[g.Pinv[r]] : 0.0;
        Dg[m] = r < n ? D[r] : 0.0;
    }
    if (n > 1)
        for (int i = 0; i < n; i++) {
            const double tmp = pick(tv, i);
            if (tmp != 0.0) {
                const double* col = LP + pk_col(i, n);
#pragma unroll
                for (int m = 0; m < kC; m++) {
                    const int r = 64 * m + lane;
                    if (r > i && r < n) tv[m] = tv[m] - tmp * col[r];
                }
            }
        }
#pragma unroll
    for (int m = 0; m < kC; m++)
        if (64 * m + lane < n) tv[m] = (1.0 / Dg[m]) * tv[m];
    if (n > 1)
        for (int i = n - 1; i >= 0; i--) {
            const double* col = LP + pk_col(i, n);
            double pr[kC];
#pragma unroll
            for (int m = 0; m < kC; m++) {
                const int r = 64 * m + lane;
                pr[m] = (r > i && r < n) ? col[r] * tv[m] : 0.0;
            }
            double tmp = pick(tv, i);
#pragma unroll
            for (int m = 0; m < kC; m++) {
                const int lo = max(i + 1 - 64 * m, 0), hi = min(n - 64 * m, 64);  // lanes of rows i < r < n
                for (int q = lo; q < hi; q++) tmp -= rl(pr[m], q);
            }
#pragma unroll
            for (int m = 0; m < kC; m++)
                if (64 * m + lane == i) tv[m] = tmp;
        }
#pragma unroll
    for (int m = 0; m < kC; m++) {
        const int r = 64 * m + lane;
        if (r < n) g.x[g.Pinv[r]] = tv[m];
    }
}

template <int kC, bool kLds, bool kPre = false>
__device__ __noinline__ void factor_solve() {
    const int n = 6 * lbg_s.np;
    if (kLds) {  // the layout of k_lba_g2o's copy in LDS
        const FactorLds f = factor_lds(n);
        factor_body<kC, true>((double*)lbg_dyn, (const uint64_t*)(lbg_dyn + f.LB), (const int*)(lbg_dyn + f.RO),
                              (const int*)(lbg_dyn + f.RS), (const int*)(lbg_dyn + f.PI),
                              (const double*)(lbg_dyn + f.SP), (double*)(lbg_dyn + f.PR),
                              kPre ? (const double*)(lbg_dyn + f.D) : nullptr);
    } else {
        const G& g = lbg_g;
        factor_body<kC, false>(g.Ld, g.Lbits, g.rs_off, g.rs_idx, g.Pinv, g.S, (double*)lbg_dyn);  // (LDS unused)
    }
}
