// Fragment of lba_g2o.hip, included inside its namespace; not a standalone header.  Errors, chi2 sums, buildSystem.
__device__ __forceinline__ constexpr int upper_idx(int r, int c) { return 6 * r - r * (r - 1) / 2 + (c - r); }  // r <= c < 6

// One edge's quadratic-form terms (BaseBinaryEdge::constructQuadraticForm as Eigen evaluates it, Omega diagonal):
//   Hll += (A^T W) A;  bl += A^T omega_r;  Hpl (6 x 3, pose-major) += (B^T W) A (robust) | B^T (A^T Omega)^T
//   (non-robust);  Hpp upper (r <= c) += (B^T W) B;  bp += B^T omega_r
// W = rho' Omega (robust) or Omega; omega_r = (-(Omega e)) rho' or -(Omega e) (terms_land / terms_pose below).

// ---------------------------------------------------------------- errors + robust chi2
// computeActiveErrors: err of every active edge, its robust chi2 (activeRobustChi2's terms) in echi (+0.0 for
// inactive edges: an exact no-op in the ordered sum)
__device__ __noinline__ void errors() {
    const LbaConsts& C = lbg_c;
    const G& g = lbg_g;
    const Sh& s = lbg_s;
    const int t = threadIdx.x;
    const bool robust = s.robust;
    // this member's share: point edges [p0, p1), plane edges [Ep + q0, Ep + q1)
    const int p0 = split_lo(g.Ep, s.m, s.T), p1 = split_lo(g.Ep, s.m + 1, s.T);
    const int npl = g.E - g.Ep, q0 = split_lo(npl, s.m, s.T), q1 = split_lo(npl, s.m + 1, s.T);
    // point edges, kEU per thread at a time: every edge's records, then every edge's operands, are loaded before
    // any is evaluated (a dependent load chain per group instead of per edge)
    constexpr int kEU = 3;
    for (int e0 = p0 + t; e0 < p1; e0 += kEU * kT) {
        int lv[kEU], ty[kEU], kf[kEU], lm[kEU], src[kEU];
#pragma unroll
        for (int u = 0; u < kEU; u++) {
            const int e = e0 + u * kT, ec = e < p1 ? e : e0;
            lv[u] = e < p1 ? g.e_level[ec] : 1;
            ty[u] = g.e_type[ec];
            kf[u] = g.e_kf[ec];
            lm[u] = g.e_lm[ec];
            src[u] = g.e_src[ec];
        }
        PointIn in[kEU];
#pragma unroll
        for (int u = 0; u < kEU; u++) in[u] = point_in(g, kf[u], lm[u], src[u]);
#pragma unroll
        for (int u = 0; u < kEU; u++) {
            const int e = e0 + u * kT;
            if (e >= p1) break;
            double chi = 0.0;
            if (lv[u] == 0) {
                double err[3];
                point_edge_error(ty[u], in[u], err);
                for (int i = 0; i < 3; i++) g.err[3 * e + i] = err[i];
                const double info[3] = {(double)in[u].isg, (double)in[u].isg, (double)in[u].isg};  // info_of, t <= 1
                double r1;
                huber(chi2_of(err, info, edge_dim(ty[u])), delta_of(C, ty[u]), robust, &chi, &r1);
            }
            g.echi[e] = chi;
        }
    }
    // plane edges: one lane pair per edge (plane_error_pair)
    for (int q = q0 + (t >> 1); q < q0 + ((q1 - q0 + kT / 2 - 1) / (kT / 2)) * (kT / 2); q += kT / 2) {
        const int e = g.Ep + q;
        const bool act = q < q1 && g.e_level[e] == 0;
        E3 r{0, 0, 0};
        if (__any(act)) {
            const int ee = act ? e : g.Ep + (q < q1 ? q : q0);
            if (q < q1) {
                const int ty = g.e_type[ee];
                auto pp = g.P + 4 * (g.e_lm[ee] - g.Np);
                r = plane_error_pair(ty - 2, load_pose(g.pose + 7 * g.e_kf[ee]), P4{{pp[0], pp[1], pp[2], pp[3]}},
                                     plane_from_f(g.plobs[g.e_src[ee]].meas), (t & 1) != 0);
            }
        }
        if (q < q1 && (t & 1) == 0) {
            double chi = 0.0;
            if (act) {
                const int ty = g.e_type[e];
                const double err[3] = {r.e0, r.e1, r.e2};
                for (int i = 0; i < 3; i++) g.err[3 * e + i] = err[i];
                double info[3], r1;
                info_of(g, C, e, ty, info);
                huber(chi2_of(err, info, edge_dim(ty)), delta_of(C, ty), robust, &chi, &r1);
            }
            g.echi[e] = chi;
        }
    }
}

// one lane: sum of v[0 .. n32) in index order (n32 a multiple of 32; two 16-load batches in flight)
template <class PD>
__device__ __forceinline__ double ordered_sum(const PD* v, int n32) {
    double acc = 0.0;
    double A[16], B[16];
#pragma unroll
    for (int u = 0; u < 16; u++) A[u] = n32 > 0 ? v[u] : 0.0;
    for (int e = 0; e < n32; e += 32) {
#pragma unroll
        for (int u = 0; u < 16; u++) B[u] = v[e + 16 + u];
#pragma unroll
        for (int u = 0; u < 16; u++) acc += A[u];
        const bool more = e + 32 < n32;
#pragma unroll
        for (int u = 0; u < 16; u++) A[u] = more ? v[e + 32 + u] : 0.0;
#pragma unroll
        for (int u = 0; u < 16; u++) acc += B[u];
    }
    return acc;
}

// the same over LDS, 16-byte reads: 8 loads per batch of 16 values, so the wait for one batch can leave the next
// batch in flight (the LDS counter holds at most 15 outstanding loads; 16 single loads would force a full wait)
__device__ __forceinline__ double ordered_sum_lds(const double* v, int n32, double acc = 0.0) {
    const double2* w = (const double2*)v;
    double2 A[8], B[8];
    const double2 z = make_double2(0.0, 0.0);
#pragma unroll
    for (int u = 0; u < 8; u++) A[u] = n32 > 0 ? w[u] : z;
    for (int e = 0; e < n32; e += 32) {
        const int q = e >> 1;
#pragma unroll
        for (int u = 0; u < 8; u++) B[u] = w[q + 8 + u];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            acc += A[u].x;
            acc += A[u].y;
        }
        const bool more = e + 32 < n32;
#pragma unroll
        for (int u = 0; u < 8; u++) A[u] = more ? w[q + 16 + u] : z;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            acc += B[u].x;
            acc += B[u].y;
        }
    }
    return acc;
}

// the ordered sums of a computeActiveErrors (activeRobustChi2: the edges' chi2 in edge order) and, for a trial
// (nS > 0), of its scale (x . (lambda x + b), entry order): the operands staged in LDS by the whole workgroup
// (coalesced), then one lane per sum -- the dependent add chains read LDS instead of global memory.  nS == 0:
// currentChi, else tempChi and scale.
__device__ __noinline__ void sums_staged(int nE, int nS) {
    const G& g = lbg_g;
    Sh& s = lbg_s;
    const int t = threadIdx.x;
    double* V = (double*)lbg_dyn;
    if ((size_t)(nE + nS) * 8 <= (size_t)kDyn) {
        for (int i = t; i < nE; i += kT) V[i] = g.echi[i];
        for (int i = t; i < nS; i += kT) V[nE + i] = g.sc[i];
        __syncthreads();
        if (t == 0) {
            const double c = ordered_sum_lds(V, nE);
            if (nS > 0) s.tempChi = c; else s.currentChi = c;
        }
        if (t == 64 && nS > 0) s.scale = ordered_sum_lds(V + nE, nS);
    } else {
        // larger graphs: chunks of kHalf values through two LDS buffers, wave 0's lane 0 adding one chunk (the chain
        // carried across chunks: the same sequence of additions) while the other waves stage the next
        constexpr int kHalf = kDyn / 16;
        auto chain = [&](auto src, int n) __attribute__((always_inline)) {
            double acc = 0.0;
            for (int i = t; i < min(kHalf, n); i += kT) V[i] = src[i];
            __syncthreads();
            for (int c = 0; c * kHalf < n; c++) {
                const int b0 = c * kHalf, nb = min(kHalf, n - b0), n0 = b0 + kHalf, nn = max(0, min(kHalf, n - n0));
                double* nxt = V + ((c + 1) & 1) * kHalf;
                if (t == 0) acc = ordered_sum_lds(V + (c & 1) * kHalf, nb, acc);
                else if (t >= 64)
                    for (int i = t - 64; i < nn; i += kT - 64) nxt[i] = src[n0 + i];
                __syncthreads();
            }
            return acc;
        };
        const double c = chain(g.echi, nE);
        if (t == 0) {
            if (nS > 0) s.tempChi = c; else s.currentChi = c;
        }
        if (nS > 0) {
            const double sc = chain(g.sc, nS);
            if (t == 0) s.scale = sc;
        }
    }
}

// ---------------------------------------------------------------- per iteration: quadratic forms and sums
// BlockSolver::buildSystem in chunks of kCh consecutive edges: (A) every edge's quadratic-form terms into LDS rows
// (every edge on two threads of different waves -- both evaluate the Jacobians, one the landmark side, the other the
// pose side; the plane edges' numeric Jacobians from plane_jacobians); (B) the sums, in edge order: each
// landmark's segment in the chunk as (segment, component) chains (continuing the landmark's partial sums when it
// started in an earlier chunk), each (free pose, term) chain by its own lane over the chunk's edges of that pose
// (LDS bitmasks), the chains' accumulators carried in registers from chunk to chunk.
constexpr int kCh = 256;                    // edges per chunk
constexpr int kSL = 13, kSP = 27, kSB = 19;  // LDS row strides (doubles): Hll + bl (12), Hpp + bp (27), Hpl (18)
constexpr int kPoseSlots = (27 * kMaxK + kT - 1) / kT;

struct EdgeW {  // Omega, robust weights and omega_r of one edge
    int dim;
    double W[3], om[3], info[3];
};
__device__ __forceinline__ EdgeW edge_weights(const LbaConsts& C, bool robust, int ty, const double* err, const double* info) {
    EdgeW w;
    w.dim = edge_dim(ty);
    double r0, wgt;
    huber(chi2_of(err, info, w.dim), delta_of(C, ty), robust, &r0, &wgt);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        w.info[r] = info[r];
        w.W[r] = robust ? wgt * info[r] : info[r];
        w.om[r] = -(info[r] * err[r]);
        if (robust) w.om[r] *= wgt;
    }
    return w;
}
// landmark side: Hll 9, bl 3 (L), Hpl 18 (Bk); see edge_terms
__device__ __forceinline__ void terms_land(const EdgeW& w, bool robust, const double (&A)[3][3], const double (&B)[3][6],
                                           bool pfree, double* L, double* Bk) {
    const bool d3 = w.dim == 3;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double s = A[0][i] * w.om[0] + A[1][i] * w.om[1];
        if (d3) s += A[2][i] * w.om[2];
        L[9 + i] = s;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double h = (A[0][i] * w.W[0]) * A[0][j] + (A[1][i] * w.W[1]) * A[1][j];
            if (d3) h += (A[2][i] * w.W[2]) * A[2][j];
            L[3 * i + j] = h;
        }
    }
    if (!pfree) return;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double h;
            if (robust) {
                h = (B[0][i] * w.W[0]) * A[0][j] + (B[1][i] * w.W[1]) * A[1][j];
                if (d3) h += (B[2][i] * w.W[2]) * A[2][j];
            } else {
                h = B[0][i] * (A[0][j] * w.info[0]) + B[1][i] * (A[1][j] * w.info[1]);
                if (d3) h += B[2][i] * (A[2][j] * w.info[2]);
            }
            Bk[3 * i + j] = h;
        }
}
// pose side: Hpp upper 21, bp 6
__device__ __forceinline__ void terms_pose(const EdgeW& w, const double (&B)[3][6], double* P) {
    const bool d3 = w.dim == 3;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) {
            double h = (B[0][i] * w.W[0]) * B[0][j] + (B[1][i] * w.W[1]) * B[1][j];
            if (d3) h += (B[2][i] * w.W[2]) * B[2][j];
            P[upper_idx(i, j)] = h;
        }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = B[0][i] * w.om[0] + B[1][i] * w.om[1];
        if (d3) s += B[2][i] * w.om[2];
        P[21 + i] = s;
    }
}

// plane / parallel / vertical edges: numeric Jacobians (base_binary_edge.hpp:130-205) into g.terms (A 3x3, then
// B 3x6, per edge), kPJ edges at a time: one lane pair per (edge, evaluation q) -- q < 6: plane perturbed by
// +-1e-9 along q >> 1 (Plane3D::oplus); 6 <= q < 18: pose exp(+-1e-9 e_d) * T, d = (q - 6) >> 1 (free poses
// only) -- the errors into LDS, then one thread per Jacobian entry: (e(+) - e(-)) / 2e-9
// Run by the errors phase on the member's plane edges [e_lo, e_hi): the Jacobians at the state whose errors it
// computes -- the linearisation point of the next buildSystem whenever one follows (a rejected trial's are never
// read: the state is popped and the errors recomputed before the next build).
constexpr int kPJ = 128;
__device__ __noinline__ void plane_jacobians(int e_lo, int e_hi) {
    const G& g = lbg_g;
    const Sh& s = lbg_s;
    double* EV = (double*)lbg_dyn;  // [kPJ][18][3]
    const int t = threadIdx.x, pr = t >> 1;
    const bool half = (t & 1) != 0;
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    __syncthreads();  // the previous phase's LDS use is over
    for (int e0 = e_lo; e0 < e_hi; e0 += kPJ) {
        const int cnt = min(kPJ, e_hi - e0);
        for (int task = pr; task < cnt * 18; task += kT / 2) {  // (both lanes of a pair: the same task)
            const int le = task / 18, q = task - 18 * le, pe = e0 + le;
            if (g.e_level[pe] != 0) continue;
            const bool pfree = s.hidx[g.e_kf[pe]] >= 0;
            if (q >= 6 && !pfree) continue;
            const int ty = g.e_type[pe], lm = g.e_lm[pe];
            SE3 T = load_pose(g.pose + 7 * g.e_kf[pe]);
            auto pp = g.P + 4 * (lm - g.Np);
            P4 P{{pp[0], pp[1], pp[2], pp[3]}};
            const P4 meas = plane_from_f(g.plobs[g.e_src[pe]].meas);
            const double sgn = (q & 1) ? -delta : delta;
            if (q < 6) {
                double add[3] = {0, 0, 0};
                add[q >> 1] = sgn;
                p_oplus(P, add);
            } else {
                double add[6] = {0, 0, 0, 0, 0, 0};
                add[(q - 6) >> 1] = sgn;
                T = se3_mul(se3_exp(add), T);
            }
            const E3 r = plane_error_pair(ty - 2, T, P, meas, half);
            if (!half) {
                double* o = EV + 3 * (18 * le + q);
                o[0] = r.e0; o[1] = r.e1; o[2] = r.e2;
            }
        }
        __syncthreads();
        for (int i = t; i < cnt * 27; i += kT) {
            const int le = i / 27, j = i - 27 * le, pe = e0 + le;
            if (g.e_level[pe] != 0) continue;
            const int dim = edge_dim(g.e_type[pe]);
            const bool pfree = s.hidx[g.e_kf[pe]] >= 0;
            const double* ev = EV + 54 * le;
            double v;
            if (j < 9) {  // A[ii][d]: the plane's evaluations 2d, 2d + 1
                const int ii = j / 3, d = j - 3 * ii;
                v = ii < dim ? scalar * (ev[3 * (2 * d) + ii] - ev[3 * (2 * d + 1) + ii]) : 0.0;
            } else {      // B[ii][d]: the pose's evaluations 6 + 2d, 7 + 2d
                const int ii = (j - 9) / 6, d = (j - 9) - 6 * ii;
                v = pfree && ii < dim ? scalar * (ev[3 * (6 + 2 * d) + ii] - ev[3 * (7 + 2 * d) + ii]) : 0.0;
            }
            g.terms[27 * (size_t)pe + j] = v;
        }
        __syncthreads();
    }
}

// This member's buildSystem share, in steps of kCh rows per side:
//  * the landmark side of the edges [eb0, eb1) (whole landmarks): every edge's Hll / bl / Hpl terms into LDS rows on
//    threads 0 .. kCh - 1, then (B) each landmark's segment summed in edge order as (segment, component) chains
//    (continuing the landmark's partial sums across steps), each Hpl block stored as 0 + its first term and its
//    later terms added in edge order;
//  * the pose side of this member's free poses: R = kCh / P rows of each pose's active edges (in insertion order,
//    g.pe_idx) per step, their Hpp / bp terms into LDS rows on threads kCh .. 2 kCh - 1, then each (pose, term)
//    chain adds its pose's rows of the step in order (one lane per chain, the accumulators in registers across
//    steps).
// Both sides read the plane edges' Jacobians of the errors phase (plane_jacobians).  The partial sums never leave
// their member before they are complete, so every sum keeps g2o's order (sparse_optimizer.cpp:100-114,
// block_solver.hpp:502-561).  Returns this member's largest |diagonal| of Hll and Hpp (computeLambdaInit) in the team
// record.
__device__ __noinline__ void build_system() {
    const LbaConsts& C = lbg_c;
    const G& g = lbg_g;
    Sh& s = lbg_s;
    unsigned char* dyn = lbg_dyn;
    long long tb0 = wall_clock64(), tA = 0, tB = 0;  // diagnostics
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const bool robust = s.robust;
    const int e0 = s.eb0, e1 = s.eb1, P = s.npown;
    const int R = P > 0 ? kCh / P : kCh;  // rows of each owned pose per step
    double* TL = (double*)dyn;
    double* TP = TL + kCh * kSL;
    double* TB = TP + kCh * kSP;
    int* RI = (int*)(TB + kCh * kSB);  // [kCh] per landmark-side row: its Hpl block, -1 none, -2 inactive edge
    // the step's landmark segments, compacted per wave: (first row, end row, landmark, first block | continuing
    // << 30 | complete << 31); per row the Hpl term's kind (0 none, 1 the block's first term: a plain store, 2 a
    // later term of the same block: an addition)
    int4* SG = (int4*)(RI + kCh);                    // [kCh]
    unsigned char* RF = (unsigned char*)(SG + kCh);  // [kCh]
    int* NSW = (int*)(RF + kCh);                     // [kW] segments per wave, [kW]: any addition rows
    int* PS = NSW + kW + 1;                          // [kMaxK] owned pose a: first entry of its edge list in pe_idx
    int* PC = PS + kMaxK;                            //   and its length
    int* NST = PC + kMaxK;                           // steps
    static_assert((size_t)kCh * (kSL + kSP + kSB) * 8 + kCh * (4 + 16 + 1) + 4 * (kW + 2 + 2 * kMaxK) <= (size_t)kDyn,
                  "LDS");
    if (t < P) {
        const int hh = s.pown[t];
        PS[t] = g.pe_off[hh];
        PC[t] = g.pe_off[hh + 1] - g.pe_off[hh];
    }
    __syncthreads();
    if (t == 0) {
        int ns = (e1 - e0 + kCh - 1) / kCh;
        for (int a = 0; a < P; a++) ns = max(ns, (PC[a] + R - 1) / R);
        *NST = ns;
    }
    double acc[kPoseSlots];
    int task[kPoseSlots];
#pragma unroll
    for (int k = 0; k < kPoseSlots; k++) {
        acc[k] = 0.0;
        task[k] = t + k * kT < 27 * P ? t + k * kT : -1;
    }
    double mx = 0.0;
    // this thread's row: landmark side (t < kCh) row t of the step's landmark chunk, pose side (t >= kCh) row i of
    // owned pose a.  Its records (level, type, keyframe, landmark, observation) and, landmark side, its structure
    // record (eseg) are loaded for the next step during the current step's (B)
    const bool land = t < kCh;
    const int q = t - kCh, pa = land ? 0 : q / R, pi = land ? 0 : q - pa * R;
    const bool prow = !land && pa < P;
    auto edge_of = [&](int st) __attribute__((always_inline)) -> int {  // -1: no row
        if (land) {
            const int e = e0 + st * kCh + t;
            return e < e1 ? e : -1;
        }
        if (!prow) return -1;
        const int i = st * R + pi;
        return i < PC[pa] ? g.pe_idx[PS[pa] + i] : -1;
    };
    int nlv = 1, nty = 0, nkf = 0, nlm = 0, nsrc = 0, ne = -1;
    int4 sgn = make_int4(-2, -1, 0, 0);
    auto edge_rec = [&](int e) __attribute__((always_inline)) {
        ne = e;
        if (e >= 0) {
            nlv = g.e_level[e]; nty = g.e_type[e]; nkf = g.e_kf[e]; nlm = g.e_lm[e]; nsrc = g.e_src[e];
            if (land) sgn = ld_i4(g.eseg + 4 * e);
        } else {
            nlv = 1;
        }
    };
    __syncthreads();
    const int nst = *NST;
    edge_rec(edge_of(0));
#ifdef SPSLAM_LBG_DIAG_BUILD
    long long db1 = 0, db2 = 0, db3 = 0;
#endif
    for (int st = 0; st < nst; st++) {
        const int c0 = e0 + st * kCh;
        const int cnt = max(0, min(kCh, e1 - c0));
        const int4 sg = sgn;
        // (B) landmark segments: the rows' Hpl kinds in edge order (head threads), segments compacted per wave
        bool head = false, again = false;
        int end_row = 0, own_h = -1, own_kb = 0;
        PMask touched = pm_zero();
        if (land && t < cnt) {
            RI[t] = sg.x;
            RF[t] = 0;
            const bool first = (sg.w >> 30) & 1;
            if ((first || t == 0) && sg.y >= 0) {
                head = true;
                own_h = sg.y;
                own_kb = sg.w & ((1 << 30) - 1);
                end_row = min(sg.z, c0 + cnt) - c0;
                touched = first ? pm_zero() : s.carry;  // (only row 0 continues a landmark of the previous step)
            }
        }
        {
            const uint64_t hb = __ballot(head);
            if (head) {
                const int li = __popcll(hb & ((1ull << lane) - 1));
                const unsigned fl = (unsigned)own_kb | ((t == 0 && !((sg.w >> 30) & 1)) ? 1u << 30 : 0u) |
                                    (c0 + end_row == sg.z ? 1u << 31 : 0u);
                SG[64 * wv + li] = make_int4(t, end_row, own_h, (int)fl);
            }
            if (lane == 0 && wv < kCh / 64) NSW[wv] = __popcll(hb);
            if (t == 0) NSW[kW] = 0;
        }
        __syncthreads();
        if (head) {
            // (the segment's block indices four at a time: one LDS round trip per four rows, not per row)
            for (int r0 = t; r0 < end_row; r0 += 4) {
                int bkv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) bkv[u] = RI[min(r0 + u, end_row - 1)];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (r0 + u >= end_row) break;
                    const int bk = bkv[u];
                    unsigned char f = 0;
                    if (bk >= 0) {
                        f = pm_test(touched, bk - own_kb) ? 2 : 1;
                        pm_set(touched, bk - own_kb);
                    }
                    RF[r0 + u] = f;
                    again |= f == 2;
                }
            }
            if (c0 + end_row != sg.z) s.carry = touched;  // (the chunk's last segment; read after two barriers)
            if (again) NSW[kW] = 1;
        }
#ifdef SPSLAM_LBG_DIAG_BUILD
        __syncthreads();
        db1 = wall_clock64();
        if (t == 0) s.dg[0] += db1 - tb0;  // segment heads (Hpl kinds, lm_amask)
#endif
        // (A) every row's terms (the plane edges' Jacobians from plane_jacobians)
        {
            const int e = ne;
            const int row = land ? t : q;
            if (e >= 0 && nlv == 0) {
                const int ty = nty;
                const int ph = s.hidx[nkf];
                const bool pfree = ph >= 0;
                double A[3][3], B[3][6], info[3], err[3];
                if (e < g.Ep) {
                    const SE3 T = load_pose(g.pose + 7 * nkf);
                    const auto& k = g.kf[nkf];
                    point_edge_jacobians(ty, T, k.fx, k.fy, k.bf, g.X + 3 * nlm, A, B, land);
                } else {
                    auto J = g.terms + 27 * (size_t)e;
#pragma unroll
                    for (int i = 0; i < 3; i++) {
#pragma unroll
                        for (int d = 0; d < 3; d++) A[i][d] = J[3 * i + d];
#pragma unroll
                        for (int d = 0; d < 6; d++) B[i][d] = J[9 + 6 * i + d];
                    }
                }
                info_of_src(g, C, nsrc, ty, info);
                for (int i = 0; i < 3; i++) err[i] = g.err[3 * e + i];
                const EdgeW w = edge_weights(C, robust, ty, err, info);
                if (land) terms_land(w, robust, A, B, pfree, TL + kSL * row, TB + kSB * row);
                else terms_pose(w, B, TP + kSP * row);
            }
        }
        __syncthreads();
        const long long tb1 = wall_clock64();
        tA += tb1 - tb0;
#ifdef SPSLAM_LBG_DIAG_BUILD
        if (t == 0) s.dg[1] += tb1 - db1;  // (A) terms
#endif
        edge_rec(edge_of(st + 1));  // the next step's records land during (B)
        // (B) landmark segment chains: Hll (9) and bl (3) in edge order, four rows' loads in flight
        {
            int nseg = 0;
#pragma unroll
            for (int w = 0; w < kCh / 64; w++) nseg += NSW[w];
            for (int tk = t; tk < 12 * nseg; tk += kT) {
                const int si = tk / 12, comp = tk - 12 * si;
                int w = 0, li = si;
                while (li >= NSW[w]) li -= NSW[w++];
                const int4 sgm = SG[64 * w + li];
                const unsigned fl = (unsigned)sgm.w;
                const int h = sgm.z;
                auto dst = comp < 9 ? g.Hll + 9 * h + comp : g.bl + 3 * h + (comp - 9);
                // a landmark continuing from the previous step resumes from its partial sums in LDS
                double a = (fl >> 30) & 1 ? s.csum[st & 1][comp] : 0.0;
                int r = sgm.x;
                for (; r + 4 <= sgm.y; r += 4) {
                    double v[4];
                    bool ok[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        ok[u] = RI[r + u] != -2;
                        v[u] = TL[kSL * (r + u) + comp];
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) a = ok[u] ? a + v[u] : a;
                }
                for (; r < sgm.y; r++)
                    if (RI[r] != -2) a += TL[kSL * r + comp];
                if (fl >> 31) {
                    *dst = a;
                    if (comp == 0 || comp == 4 || comp == 8) mx = fmax(mx, fabs(a));
                } else {
                    s.csum[(st + 1) & 1][comp] = a;
                }
            }
#ifdef SPSLAM_LBG_DIAG_BUILD
            __syncthreads();
            db2 = wall_clock64();
            if (t == 0) s.dg[2] += db2 - tb1;  // landmark chains
#endif
            // each block's first term: 0 + term (one entry per task)
            for (int i = t; i < 18 * cnt; i += kT) {
                const int r = i / 18, c = i - 18 * r;
                if (RF[r] == 1) g.blkB[(size_t)18 * RI[r] + c] = 0.0 + TB[kSB * r + c];
            }
            if (NSW[kW]) {  // (block-uniform) the later terms, after every first term is stored
                __syncthreads();
                if (again) {
                    for (int r = t; r < end_row; r++) {
                        if (RF[r] != 2) continue;
                        auto dst = g.blkB + (size_t)18 * RI[r];
                        const double* rb = TB + kSB * r;
#pragma unroll
                        for (int j = 0; j < 18; j++) dst[j] += rb[j];
                    }
                }
            }
        }
#ifdef SPSLAM_LBG_DIAG_BUILD
        __syncthreads();
        db3 = wall_clock64();
        if (t == 0) s.dg[3] += db3 - db2;  // Hpl blocks
#endif
        // (free pose, term) chains over the step's rows of the pose: four rows' loads in flight, then their four adds
        // in edge order (a missing row: a select keeps the sum)
#pragma unroll
        for (int k = 0; k < kPoseSlots; k++) {
            if (task[k] < 0) continue;
            const int a = task[k] / 27, j = task[k] - 27 * a;
            const int n_a = min(R, PC[a] - st * R);
            const double* rows = TP + kSP * (a * R) + j;
            for (int i = 0; i < n_a; i += 4) {
                double v[4];
                bool ok[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    ok[u] = i + u < n_a;
                    v[u] = rows[kSP * (ok[u] ? i + u : i)];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) acc[k] = ok[u] ? acc[k] + v[u] : acc[k];
            }
        }
        __syncthreads();
        tb0 = wall_clock64();
        tB += tb0 - tb1;
#ifdef SPSLAM_LBG_DIAG_BUILD
        if (t == 0) { s.dg[4] += tb0 - db3; s.dg[5] += 1; }  // pose chains, steps
#endif
    }
    if (t == 0) { s.ph[0] += tA; s.tB += tB; }
#pragma unroll
    for (int k = 0; k < kPoseSlots; k++) {
        if (task[k] < 0) continue;
        const int a = task[k] / 27, j = task[k] - 27 * a;
        g.Hps[27 * s.pown[a] + j] = acc[k];
        if (j == 0 || j == 6 || j == 11 || j == 15 || j == 18 || j == 20) mx = fmax(mx, fabs(acc[k]));
    }
    mx = block_max(mx, s.red);
    if (t == 0) g.team->mx[s.m] = mx;
}
