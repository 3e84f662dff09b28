// Fragment of lba_g2o.hip, included inside its namespace; not a standalone header.  The Schur complement.
// ---------------------------------------------------------------- per trial

// setLambda + the Schur complement (block_solver.hpp:367-436), this member's block rows.  Every entry of a pattern
// block (i1, i2) is its own chain in g2o's order: Hschur(6 i1 + r, 6 i2 + c) = 0 + Hpp (+ lambda) then, landmark by
// landmark in landmark (vertex-id) order, -= (BDinv(r, 0) Bj(c, 0) + BDinv(r, 1) Bj(c, 1)) + BDinv(r, 2) Bj(c, 2); and
// Bb(6 i1 + r) = 0 + the landmarks' (Bi db)(r) in the same order.  One wave per block: lane 6 r + c holds entry (r,
// c), lanes 36 + r the diagonal block's Bb(r) (team_plan gives each member whole block rows, each wave up to kBW
// blocks, longest chains dealt first).  Every member stages every landmark in chunks of up to 64: their Hpl blocks
// (one contiguous range, coalesced), masks, Hll and bl -- the chunk's (Hll + lambda)^-1 and Dinv bl formed in place
// (the expressions of update()) -- then BDinv = Bi Dinv and Bi db for the blocks of its own rows (one thread per
// block row) and every free pose's chunk landmarks as a bitmask; then each wave, per block, compacts the chunk's
// landmarks that observe both poses into a list of (BDinv block, Bj block) pairs held one per lane, and walks it with
// the next landmark's operands loading while the current one is subtracted (the list read with v_readlane at the
// loop counter: no load on the chain's critical path).
#ifndef SPSLAM_LBG_SCHUR_BLOCKS
#define SPSLAM_LBG_SCHUR_BLOCKS 8
#endif
constexpr int kBW = SPSLAM_LBG_SCHUR_BLOCKS;  // blocks per wave per round
#ifndef SPSLAM_LBG_SCHUR_TASKS
#define SPSLAM_LBG_SCHUR_TASKS 2
#endif
constexpr int kSchurTasks = SPSLAM_LBG_SCHUR_TASKS;  // schur_rows: chains per lane per round
// (Hll + lambda)^-1 (Eigen's cofactor inverse) and Dinv bl of one landmark
__device__ __forceinline__ void landmark_dinv(const double* H, const double* bv, double lam, double* Di, double* db) {
    double D[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) D[i][j] = H[3 * i + j] + (i == j ? lam : 0.0);
    inverse3(D, Di);
    for (int i = 0; i < 3; i++) db[i] = (Di[3 * i] * bv[0] + Di[3 * i + 1] * bv[1]) + Di[3 * i + 2] * bv[2];
}
__device__ __noinline__ void schur() {
    const G& g = lbg_g;
    Sh& s = lbg_s;
    unsigned char* dyn = lbg_dyn;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int np = s.np, n = 6 * np, nch = s.nch;
    const double lam = s.lambda;
    // LDS: the staged chunk (blocks, Dinv, Dinv bl | masks, block offsets, block -> landmark, block -> pose), its
    // BDinv and Bi db, the poses' landmark masks, the waves' candidate lists
    constexpr int kBufD = kSchurBlk * 18 + kSchurLm * 12;
    double* BUF = (double*)dyn;                          // [kBufD]
    double* SD = BUF + kBufD;                            // [kSchurBlk][18] BDinv
    double* SU = SD + kSchurBlk * 18;                    // [kSchurBlk][6] B row . Dinv bl (Bb's terms)
    PMask* SM = (PMask*)(SU + kSchurBlk * 6);            // [kSchurLm]
    uint64_t* PM = (uint64_t*)(SM + kSchurLm);           // [kMaxK]
    int* SO = (int*)(PM + kMaxK);                        // [kSchurLm + 1]
    unsigned short* OB = (unsigned short*)(SO + kSchurLm + 1);  // [kMaxK][kSchurLm] (pose, landmark) -> its block
    unsigned char* BL = (unsigned char*)(OB + kMaxK * kSchurLm);  // [kSchurBlk] block -> landmark
    unsigned char* BP = BL + kSchurBlk;                  // [kSchurBlk] block -> pose
    using LdsU = __attribute__((address_space(3))) unsigned;
    LdsU* LST = (LdsU*)(unsigned*)(((uintptr_t)(BP + kSchurBlk) + 3) & ~(uintptr_t)3);  // [kW][64]
    const double* SDi = BUF + kSchurBlk * 18;
    const double* Sdb = SDi + kSchurLm * 9;
    static_assert((kBufD + kSchurBlk * 24 + kSchurLm * kPW + kMaxK) * 8 + (kSchurLm + 1) * 4 + kMaxK * kSchurLm * 2 +
                      2 * kSchurBlk + 4 + kW * 64 * 4 <= kDynAlloc, "LDS");
    constexpr int kPer = (kBufD + kT - 1) / kT;          // staged doubles per thread
    const int bo0 = s.bo0, nbm = s.bo1 - s.bo0;
    const PMask rmask = s.rmask;
    // this lane's entry: (r, c) on lanes 0 .. 35, Bb(r) on lanes 36 .. 41 (its operand addresses clamped in range)
    const bool ent = lane < 36;
    const int er = ent ? lane / 6 : min(lane - 36, 5), ec = ent ? lane - 6 * (lane / 6) : 0;
    using LdsD = const __attribute__((address_space(3))) double;
    LdsD* pE = (LdsD*)(SD + 3 * er);   // (LDS address-space pointers: 32-bit address arithmetic, ds_* accesses)
    LdsD* pJ = (LdsD*)(BUF + 3 * ec);
    LdsD* pU = (LdsD*)(SU + er);
    for (int round = 0; round * kW * kBW < nbm; round++) {
        int i1[kBW], i2[kBW];
        double acc[kBW];
#pragma unroll
        for (int k = 0; k < kBW; k++) {
            i1[k] = -1; i2[k] = 0; acc[k] = 0.0;
            const int jb = round * kW * kBW + snake_pick(k, wv, kW);
            if (jb < nbm) {
                const int blk = g.bord[bo0 + jb];
                if (blk < np) {
                    i1[k] = i2[k] = blk;
                } else {
                    int rem = blk - np, a = 0;
                    while (rem >= pm_popc(s.pat[a]) - 1) { rem -= pm_popc(s.pat[a]) - 1; a++; }
                    PMask row = pm_andnot(s.pat[a], pm_bit(a));
                    for (int u = 0; u < rem; u++) pm_pop(row);
                    i1[k] = a;
                    i2[k] = pm_ffs(row);
                }
                i1[k] = uni(i1[k]);
                i2[k] = uni(i2[k]);
                if (i1[k] == i2[k] && ent && ec >= er) {
                    const double h = g.Hps[27 * i1[k] + upper_idx(er, ec)];
                    acc[k] = 0.0 + (ec == er ? h + lam : h);
                }
            }
        }
        // chunk c's records into registers (global loads in flight), later into the staging buffer.  Every load is
        // unconditional (addresses clamped into the chunk; the surplus entries are never read) and nothing loaded is
        // used before the commit, so no wait lands in the chunk loop; the chunk bounds (sch, sch_kb) of the chunk
        // after next load one chunk ahead.
        double pv[kPer];
        PMask pmk = pm_zero();
        int pof = 0, pof1 = 0;
        auto prefetch = [&](int h0, int h1, int kb0, int kb1) __attribute__((always_inline)) {
            const int nbk = kb1 - kb0, nh = h1 - h0;
            const int cb = max(nbk * 18 - 1, 0), ch = max(nh * 9 - 1, 0), cl = max(nh * 3 - 1, 0);
#pragma unroll
            for (int q = 0; q < kPer; q++) {
                const int i = t + q * kT;
                const gdouble* src;
                if ((q + 1) * kT <= kSchurBlk * 18) {  // (compile time) the slice is in the Hpl block range
                    src = g.blkB + (size_t)18 * kb0 + min(i, cb);
                } else {
                    const int j = i - kSchurBlk * 18, j2 = j - kSchurLm * 9;
                    const gdouble* a = g.blkB + (size_t)18 * kb0 + min(i, cb);
                    const gdouble* h = g.Hll + (size_t)9 * h0 + min(max(j, 0), ch);
                    const gdouble* l = g.bl + (size_t)3 * h0 + min(max(j2, 0), cl);
                    src = j < 0 ? a : (j2 < 0 ? h : l);
                }
                pv[q] = *src;
            }
            const int tc = min(t, max(nh - 1, 0));
            pmk = pm_ld(g.lmh_mask + h0 + tc);
            pof = g.lmh_blk[h0 + min(t, nh)];
            pof1 = g.lmh_blk[h0 + tc + 1];
        };
        auto commit = [&](int nh, int kb0) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < kPer; q++)
                if (t + q * kT < kBufD) BUF[t + q * kT] = pv[q];
            if (t < nh) {
                SM[t] = pmk;
                PMask m = pmk;
                for (int bk = pof - kb0; bk < pof1 - kb0; bk++) {  // (the blocks of a landmark are in pose order)
                    BL[bk] = (unsigned char)t;
                    BP[bk] = (unsigned char)pm_ffs(m);
                    pm_pop(m);
                }
            }
            if (t <= nh) SO[t] = pof - kb0;
        };
        __syncthreads();  // the previous phase's LDS use is over
        // chunk bounds: (h0, h1, kb0, kb1) of the current chunk, the next, and the one after (loading)
        int cur_h0 = 0, cur_h1 = 0, cur_k0 = 0, cur_k1 = 0, nx_h1 = 0, nx_k1 = 0, nn_h1 = 0, nn_k1 = 0;
        if (nch > 0) {
            cur_h0 = g.sch[0]; cur_h1 = g.sch[1]; cur_k0 = g.sch_kb[0]; cur_k1 = g.sch_kb[1];
            nx_h1 = g.sch[min(2, nch)]; nx_k1 = g.sch_kb[min(2, nch)];
            prefetch(cur_h0, cur_h1, cur_k0, cur_k1);
            commit(cur_h1 - cur_h0, cur_k0);
            nn_h1 = g.sch[min(3, nch)]; nn_k1 = g.sch_kb[min(3, nch)];
        }
        for (int c = 0; c < nch; c++) {
#ifdef SPSLAM_LBG_DIAG
            long long d0 = wall_clock64();
#endif
            __syncthreads();  // chunk c is staged
#ifdef SPSLAM_LBG_DIAG
            long long d1 = wall_clock64();
            if (t == 0) s.dg[0] += d1 - d0;
#endif
            const int nh = cur_h1 - cur_h0;
            const int nbk = cur_k1 - cur_k0;
            if (t < nh) {  // the staged Hll, bl -> Dinv, Dinv bl, in place
                double* Hd = BUF + kSchurBlk * 18 + 9 * t;
                double* bd = BUF + kSchurBlk * 18 + kSchurLm * 9 + 3 * t;
                double H[9], bv[3], Di[9], db[3];
                for (int j = 0; j < 9; j++) H[j] = Hd[j];
                for (int j = 0; j < 3; j++) bv[j] = bd[j];
                landmark_dinv(H, bv, lam, Di, db);
                for (int j = 0; j < 9; j++) Hd[j] = Di[j];
                for (int j = 0; j < 3; j++) bd[j] = db[j];
            }
            __syncthreads();
            for (int i = t; i < nbk * 6; i += kT) {  // BDinv row by row: (Bi Dinv)(r, q), and Bi(r) . Dinv bl
                const int bk = i / 6, r6 = i - 6 * bk;
                if (!pm_test(rmask, BP[bk])) continue;  // a block row of another member
                const int hb = BL[bk];
                const double* Bi = BUF + 18 * bk + 3 * r6;
                const double* Di = SDi + 9 * hb;
                const double* db = Sdb + 3 * hb;
                double* BD = SD + 18 * bk + 3 * r6;
#pragma unroll
                for (int q = 0; q < 3; q++) BD[q] = (Bi[0] * Di[q] + Bi[1] * Di[3 + q]) + Bi[2] * Di[6 + q];
                SU[i] = (Bi[0] * db[0] + Bi[1] * db[1]) + Bi[2] * db[2];
            }
            for (int i = wv; i < np; i += kW) {  // free pose i's landmarks in the chunk, and their blocks
                const PMask mk = lane < nh ? SM[lane] : pm_zero();
                const bool obs = pm_test(mk, i);
                const uint64_t m = __ballot(obs);
                if (lane == 0) PM[i] = m;
                if (obs) OB[kSchurLm * i + lane] = (unsigned short)(SO[lane] + pm_popc_below(mk, i));
            }
            __syncthreads();
#ifdef SPSLAM_LBG_DIAG
            long long d2 = wall_clock64();
            if (t == 0) s.dg[1] += d2 - d1;
#endif
            if (c + 1 < nch) prefetch(cur_h1, nx_h1, cur_k1, nx_k1);  // lands while chunk c is processed
#ifdef SPSLAM_LBG_DIAG_SCHUR
            const long long wc0 = clock64();
            int wsteps = 0;
#endif
#pragma unroll
            for (int k = 0; k < kBW; k++) {
                if (i1[k] < 0) continue;  // (wave-uniform)
                const uint64_t cand = rl64(PM[i1[k]] & PM[i2[k]], 0);
                if (!cand) continue;
                // the candidates' (BDinv block, Bj block) pairs, compacted in landmark order, one per lane
                const bool in = (cand >> lane) & 1ull;
                const unsigned pos = __builtin_amdgcn_mbcnt_hi((unsigned)(cand >> 32),
                                                               __builtin_amdgcn_mbcnt_lo((unsigned)cand, 0u));
                if (in) LST[64 * wv + pos] = (unsigned)OB[kSchurLm * i1[k] + lane] |
                                             ((unsigned)OB[kSchurLm * i2[k] + lane] << 16);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const unsigned my = LST[64 * wv + lane];
                const int nc = __popcll(cand);

                // operands of list entry q: BDinv row er of its first block, Bj row ec of its second, Bi db (er).  The
                // entry is opaque to the compiler, so the next entry's loads (issued before the current one is
                // subtracted) are not merged with the current one's into loads behind a wait at the loop top.
                auto ld = [&](int q, double (&E)[3], double (&B)[3], double& u) __attribute__((always_inline)) {
                    unsigned bb = __builtin_amdgcn_readlane(my, q);
                    asm volatile("" : "+s"(bb));
                    const unsigned b1 = bb & 0xffffu, b2 = bb >> 16;
                    LdsD* pe = pE + 18 * b1;
                    LdsD* pj = pJ + 18 * b2;
                    LdsD* pu = pU + 6 * b1;
                    E[0] = pe[0]; E[1] = pe[1]; E[2] = pe[2];
                    B[0] = pj[0]; B[1] = pj[1]; B[2] = pj[2];
                    u = pu[0];
                };
                auto step = [&](double a, const double (&E)[3], const double (&B)[3], double u)
                    __attribute__((always_inline)) {
                    const double sub = a - ((E[0] * B[0] + E[1] * B[1]) + E[2] * B[2]);
                    const double add = a + u;
                    return ent ? sub : add;
                };
                double EA[3], BA[3], uA, EB[3], BB[3], uB;
                ld(0, EA, BA, uA);
                double a = acc[k];
                int q = 0;
                for (; q + 2 <= nc; q += 2) {  // two operand sets in turn: one in flight while the other is used
                    ld(q + 1, EB, BB, uB);
                    a = step(a, EA, BA, uA);
                    ld(min(q + 2, nc - 1), EA, BA, uA);
                    a = step(a, EB, BB, uB);
                }
                if (q < nc) a = step(a, EA, BA, uA);
                acc[k] = a;
#ifdef SPSLAM_LBG_DIAG_SCHUR
                wsteps += nc;
#endif
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the list is free again
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
#ifdef SPSLAM_LBG_DIAG_SCHUR  // per wave: chain cycles and steps (summed), the chunk's slowest wave (summed)
            if (lane == 0) {
                const unsigned long long wc = (unsigned long long)(clock64() - wc0);
                atomicAdd((unsigned long long*)&s.dg[10], wc);
                atomicAdd((unsigned long long*)&s.dg[11], (unsigned long long)wsteps);
                atomicMax((unsigned long long*)&s.dg[12], wc);
            }
#endif
            __syncthreads();  // the staging buffer, BDinv and the masks are free again
#ifdef SPSLAM_LBG_DIAG_SCHUR
            if (t == 0) { s.dg[13] += s.dg[12]; s.dg[12] = 0; }
#endif
#ifdef SPSLAM_LBG_DIAG
            long long d3 = wall_clock64();
            if (t == 0) s.dg[2] += d3 - d2;
#endif
            if (c + 1 < nch) commit(nx_h1 - cur_h1, cur_k1);
            // advance the bounds; the chunk after next's load lands during the next chunk
            cur_h0 = cur_h1; cur_h1 = nx_h1; cur_k0 = cur_k1; cur_k1 = nx_k1;
            nx_h1 = nn_h1; nx_k1 = nn_k1;
            nn_h1 = g.sch[min(c + 4, nch)]; nn_k1 = g.sch_kb[min(c + 4, nch)];
#ifdef SPSLAM_LBG_DIAG
            if (t == 0) s.dg[3] += wall_clock64() - d3;
#endif
        }
#pragma unroll
        for (int k = 0; k < kBW; k++) {
            if (i1[k] < 0) continue;
            if (ent) g.S[(size_t)(6 * i1[k] + er) * n + 6 * i2[k] + ec] = acc[k];
            else if (lane < 42 && i1[k] == i2[k]) g.bs[6 * i1[k] + er] = g.Hps[27 * i1[k] + 21 + er] - acc[k];
        }
    }
}

// The same Schur complement with one lane per (block, R rows r0 .. r0 + R - 1) holding those rows' entries (and the
// diagonal block's Bb(r)), each lane walking its own candidate landmarks, TT such tasks per lane: fewer LDS bytes per
// entry than schur()'s lane per entry (a landmark's Bj block is read once for R rows), but a dependent LDS round trip
// per landmark.  The faster of the two when a member holds many blocks (teams of 1 - 4); R and TT are chosen per call
// from the member's block count (schur_rows_pick): every chain keeps g2o's landmark order whatever the split.
template <int R, int TT>
__device__ __noinline__ void schur_rows() {
    constexpr int kG = 6 / R;  // row groups per block
    const G& g = lbg_g;
    Sh& s = lbg_s;
    unsigned char* dyn = lbg_dyn;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int np = s.np, n = 6 * np, nch = s.nch;
    const double lam = s.lambda;
    // LDS: the staged chunk (blocks, Dinv, Dinv bl | masks, block offsets, block -> landmark, block -> pose), its
    // BDinv and Bi db, the poses' landmark masks, the waves' candidate lists
    constexpr int kBufD = kSchurBlk * 18 + kSchurLm * 12;
    double* BUF = (double*)dyn;                          // [kBufD]
    double* SD = BUF + kBufD;                            // [kSchurBlk][18] BDinv
    double* SU = SD + kSchurBlk * 18;                    // [kSchurBlk][6] B row . Dinv bl (Bb's terms)
    PMask* SM = (PMask*)(SU + kSchurBlk * 6);            // [kSchurLm]
    uint64_t* PM = (uint64_t*)(SM + kSchurLm);           // [kMaxK]
    int* SO = (int*)(PM + kMaxK);                        // [kSchurLm + 1]
    unsigned short* OB = (unsigned short*)(SO + kSchurLm + 1);  // [kMaxK][kSchurLm] (pose, landmark) -> its block
    unsigned char* BL = (unsigned char*)(OB + kMaxK * kSchurLm);  // [kSchurBlk] block -> landmark
    unsigned char* BP = BL + kSchurBlk;                  // [kSchurBlk] block -> pose
    const double* SDi = BUF + kSchurBlk * 18;
    const double* Sdb = SDi + kSchurLm * 9;
    static_assert((kBufD + kSchurBlk * 24 + kSchurLm * kPW + kMaxK) * 8 + (kSchurLm + 1) * 4 + kMaxK * kSchurLm * 2 +
                      2 * kSchurBlk + 4 + kW * 64 * 4 <= kDynAlloc, "LDS");
    constexpr int kPer = (kBufD + kT - 1) / kT;          // staged doubles per thread
    const int bo0 = s.bo0, nbm = s.bo1 - s.bo0;
    const PMask rmask = s.rmask;
    using LdsD = const __attribute__((address_space(3))) double;
    for (int round = 0; round * TT * kT < kG * nbm; round++) {
        int i1[TT], i2[TT], rr[TT];
        double acc[TT][R][6], cf[TT][R];
#pragma unroll
        for (int k = 0; k < TT; k++) {
            i1[k] = -1; i2[k] = 0; rr[k] = 0;
            const int task = (round * TT + k) * kT + t;
            if (task < kG * nbm) {
                const int jb = task / kG;
                rr[k] = R * (task - kG * jb);
                const int blk = g.bord[bo0 + jb];
                if (blk < np) {
                    i1[k] = i2[k] = blk;
                } else {
                    int rem = blk - np, a = 0;
                    while (rem >= pm_popc(s.pat[a]) - 1) { rem -= pm_popc(s.pat[a]) - 1; a++; }
                    PMask row = pm_andnot(s.pat[a], pm_bit(a));
                    for (int u = 0; u < rem; u++) pm_pop(row);
                    i1[k] = a;
                    i2[k] = pm_ffs(row);
                }
            }
            const bool diag = i1[k] >= 0 && i1[k] == i2[k];
#pragma unroll
            for (int q = 0; q < R; q++) {
                const int r = rr[k] + q;
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    double base = 0.0;
                    if (diag && c >= r)
                        base = c == r ? g.Hps[27 * i1[k] + upper_idx(r, c)] + lam : g.Hps[27 * i1[k] + upper_idx(r, c)];
                    acc[k][q][c] = 0.0 + base;
                }
                cf[k][q] = 0.0;
            }
        }
        // chunk c's records into registers (global loads in flight), later into the staging buffer.  Every load is
        // unconditional (addresses clamped into the chunk; the surplus entries are never read) and nothing loaded is
        // used before the commit, so no wait lands in the chunk loop; the chunk bounds (sch, sch_kb) of the chunk
        // after next load one chunk ahead.
        double pv[kPer];
        PMask pmk = pm_zero();
        int pof = 0, pof1 = 0;
        auto prefetch = [&](int h0, int h1, int kb0, int kb1) __attribute__((always_inline)) {
            const int nbk = kb1 - kb0, nh = h1 - h0;
            const int cb = max(nbk * 18 - 1, 0), ch = max(nh * 9 - 1, 0), cl = max(nh * 3 - 1, 0);
#pragma unroll
            for (int q = 0; q < kPer; q++) {
                const int i = t + q * kT;
                const gdouble* src;
                if ((q + 1) * kT <= kSchurBlk * 18) {  // (compile time) the slice is in the Hpl block range
                    src = g.blkB + (size_t)18 * kb0 + min(i, cb);
                } else {
                    const int j = i - kSchurBlk * 18, j2 = j - kSchurLm * 9;
                    const gdouble* a = g.blkB + (size_t)18 * kb0 + min(i, cb);
                    const gdouble* h = g.Hll + (size_t)9 * h0 + min(max(j, 0), ch);
                    const gdouble* l = g.bl + (size_t)3 * h0 + min(max(j2, 0), cl);
                    src = j < 0 ? a : (j2 < 0 ? h : l);
                }
                pv[q] = *src;
            }
            const int tc = min(t, max(nh - 1, 0));
            pmk = pm_ld(g.lmh_mask + h0 + tc);
            pof = g.lmh_blk[h0 + min(t, nh)];
            pof1 = g.lmh_blk[h0 + tc + 1];
        };
        auto commit = [&](int nh, int kb0) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < kPer; q++)
                if (t + q * kT < kBufD) BUF[t + q * kT] = pv[q];
            if (t < nh) {
                SM[t] = pmk;
                PMask m = pmk;
                for (int bk = pof - kb0; bk < pof1 - kb0; bk++) {  // (the blocks of a landmark are in pose order)
                    BL[bk] = (unsigned char)t;
                    BP[bk] = (unsigned char)pm_ffs(m);
                    pm_pop(m);
                }
            }
            if (t <= nh) SO[t] = pof - kb0;
        };
        __syncthreads();  // the previous phase's LDS use is over
        // chunk bounds: (h0, h1, kb0, kb1) of the current chunk, the next, and the one after (loading)
        int cur_h0 = 0, cur_h1 = 0, cur_k0 = 0, cur_k1 = 0, nx_h1 = 0, nx_k1 = 0, nn_h1 = 0, nn_k1 = 0;
        if (nch > 0) {
            cur_h0 = g.sch[0]; cur_h1 = g.sch[1]; cur_k0 = g.sch_kb[0]; cur_k1 = g.sch_kb[1];
            nx_h1 = g.sch[min(2, nch)]; nx_k1 = g.sch_kb[min(2, nch)];
            prefetch(cur_h0, cur_h1, cur_k0, cur_k1);
            commit(cur_h1 - cur_h0, cur_k0);
            nn_h1 = g.sch[min(3, nch)]; nn_k1 = g.sch_kb[min(3, nch)];
        }
        for (int c = 0; c < nch; c++) {
#ifdef SPSLAM_LBG_DIAG
            long long d0 = wall_clock64();
#endif
            __syncthreads();  // chunk c is staged
#ifdef SPSLAM_LBG_DIAG
            long long d1 = wall_clock64();
            if (t == 0) s.dg[0] += d1 - d0;
#endif
            const int nh = cur_h1 - cur_h0;
            const int nbk = cur_k1 - cur_k0;
            if (t < nh) {  // the staged Hll, bl -> Dinv, Dinv bl, in place
                double* Hd = BUF + kSchurBlk * 18 + 9 * t;
                double* bd = BUF + kSchurBlk * 18 + kSchurLm * 9 + 3 * t;
                double H[9], bv[3], Di[9], db[3];
                for (int j = 0; j < 9; j++) H[j] = Hd[j];
                for (int j = 0; j < 3; j++) bv[j] = bd[j];
                landmark_dinv(H, bv, lam, Di, db);
                for (int j = 0; j < 9; j++) Hd[j] = Di[j];
                for (int j = 0; j < 3; j++) bd[j] = db[j];
            }
            __syncthreads();
            for (int i = t; i < nbk * 6; i += kT) {  // BDinv row by row: (Bi Dinv)(r, q), and Bi(r) . Dinv bl
                const int bk = i / 6, r6 = i - 6 * bk;
                if (!pm_test(rmask, BP[bk])) continue;  // a block row of another member
                const int hb = BL[bk];
                const double* Bi = BUF + 18 * bk + 3 * r6;
                const double* Di = SDi + 9 * hb;
                const double* db = Sdb + 3 * hb;
                double* BD = SD + 18 * bk + 3 * r6;
#pragma unroll
                for (int q = 0; q < 3; q++) BD[q] = (Bi[0] * Di[q] + Bi[1] * Di[3 + q]) + Bi[2] * Di[6 + q];
                SU[i] = (Bi[0] * db[0] + Bi[1] * db[1]) + Bi[2] * db[2];
            }
            for (int i = wv; i < np; i += kW) {  // free pose i's landmarks in the chunk, and their blocks
                const PMask mk = lane < nh ? SM[lane] : pm_zero();
                const bool obs = pm_test(mk, i);
                const uint64_t m = __ballot(obs);
                if (lane == 0) PM[i] = m;
                if (obs) OB[kSchurLm * i + lane] = (unsigned short)(SO[lane] + pm_popc_below(mk, i));
            }
            __syncthreads();
#ifdef SPSLAM_LBG_DIAG
            long long d2 = wall_clock64();
            if (t == 0) s.dg[1] += d2 - d1;
#endif
            if (c + 1 < nch) prefetch(cur_h1, nx_h1, cur_k1, nx_k1);  // lands while chunk c is processed
#pragma unroll
            for (int k = 0; k < TT; k++) {
                if (i1[k] < 0) continue;
                const int r = rr[k];
                uint64_t cand = PM[i1[k]] & PM[i2[k]];
                // one LDS round trip per landmark: the next landmark's blocks (the chunk's (pose, landmark) block
                // table) load while this one's are subtracted, and the diagonal lanes' Bb term comes staged (SU)
                // with the blocks instead of through a dependent load of Dinv bl
                if (cand) {
                    using LdsU16 = const __attribute__((address_space(3))) unsigned short;
                    LdsU16* O1 = (LdsU16*)(OB + kSchurLm * i1[k]);
                    LdsU16* O2 = (LdsU16*)(OB + kSchurLm * i2[k]);
                    LdsD* SDr = (LdsD*)(SD + 3 * r);
                    LdsD* SUr = (LdsD*)(SU + r);
                    LdsD* BUFl = (LdsD*)BUF;
                    int hl = __ffsll((unsigned long long)cand) - 1;
                    cand &= cand - 1;
                    int b1 = O1[hl], b2 = O2[hl];
                    // (opaque here: otherwise the first landmark's loads and the loop's next-landmark loads are
                    // merged into one load at the top of the loop, behind a wait -- the round trip this loop avoids)
                    asm volatile("" : "+v"(b1), "+v"(b2));
                    for (;;) {
                        LdsD* BD = SDr + __umul24(b1, 18);  // (24-bit products: full-rate multiplies)
                        LdsD* Bj = BUFl + __umul24(b2, 18);
                        double e[3 * R];
#pragma unroll
                        for (int q = 0; q < 3 * R; q++) e[q] = BD[q];  // BDinv rows r .. r + R - 1
                        double bj[18];
#pragma unroll
                        for (int q = 0; q < 18; q++) bj[q] = Bj[q];
                        double u[R];
#pragma unroll
                        for (int q = 0; q < R; q++) u[q] = SUr[__umul24(b1, 6) + q];  // (b1 = b2 on the diagonal)
                        const bool more = cand != 0;
                        const int hn = more ? __ffsll((unsigned long long)cand) - 1 : hl;
                        cand &= cand - 1;
                        const int b1n = O1[hn], b2n = O2[hn];
#pragma unroll
                        for (int q = 0; q < R; q++)
#pragma unroll
                            for (int cc = 0; cc < 6; cc++)
                                acc[k][q][cc] -= (e[3 * q] * bj[3 * cc] + e[3 * q + 1] * bj[3 * cc + 1]) +
                                                 e[3 * q + 2] * bj[3 * cc + 2];
#pragma unroll
                        for (int q = 0; q < R; q++)
                            cf[k][q] += u[q];  // (kept for the diagonal lanes only: unconditional, so the load is not
                                               // sunk into a branch that waits for the next landmark's loads too)
                        if (!more) break;
                        hl = hn;
                        b1 = b1n;
                        b2 = b2n;
                    }
                }
            }
            __syncthreads();  // the staging buffer, BDinv and the masks are free again
#ifdef SPSLAM_LBG_DIAG
            long long d3 = wall_clock64();
            if (t == 0) s.dg[2] += d3 - d2;
#endif
            if (c + 1 < nch) commit(nx_h1 - cur_h1, cur_k1);
            // advance the bounds; the chunk after next's load lands during the next chunk
            cur_h0 = cur_h1; cur_h1 = nx_h1; cur_k0 = cur_k1; cur_k1 = nx_k1;
            nx_h1 = nn_h1; nx_k1 = nn_k1;
            nn_h1 = g.sch[min(c + 4, nch)]; nn_k1 = g.sch_kb[min(c + 4, nch)];
#ifdef SPSLAM_LBG_DIAG
            if (t == 0) s.dg[3] += wall_clock64() - d3;
#endif
        }
#pragma unroll
        for (int k = 0; k < TT; k++) {
            if (i1[k] < 0) continue;
#pragma unroll
            for (int q = 0; q < R; q++) {
                const int r = rr[k] + q;
#pragma unroll
                for (int cc = 0; cc < 6; cc++) g.S[(size_t)(6 * i1[k] + r) * n + 6 * i2[k] + cc] = acc[k][q][cc];
                if (i1[k] == i2[k]) g.bs[6 * i1[k] + r] = g.Hps[27 * i1[k] + 21 + r] - cf[k][q];
            }
        }
    }
}
// the row-group layout for this member's nbm blocks: fewest passes over the landmark chunks first (each pass stages
// every chunk again), then the least time per landmark step -- the largest of one lane's dependent step (an LDS
// round trip, ~120 clocks, then its fp64 work: 4 clocks per wave instruction, 6 per entry + 1 per Bb term), the
// busiest SIMD's fp64 issue and the waves' LDS reads (bytes / 128 per clock).  Measured: 55 blocks per member
// (12-keyframe maps) run fastest with one row per task, 325 (25 free poses) with two rows and two tasks per lane.
__device__ __forceinline__ int schur_rows_pick(int nbm) {
    const int R[4] = {6, 3, 2, 1}, TT[4] = {1, 1, 2, 2};
    int best = 3;
    long long best_cost = -1;
    for (int v = 0; v < 4; v++) {
        const long long tasks = (long long)(6 / R[v]) * nbm, slots = (long long)kT * TT[v];
        const long long rounds = (tasks + slots - 1) / slots;
        const long long per_round = (tasks + rounds - 1) / max(rounds, 1ll);
        const long long waves = (per_round + 64 * TT[v] - 1) / (64 * TT[v]);
        const long long lds = waves * 64 * TT[v] * (4 * R[v] + 18) * 8 / 128;
        const long long step = (long long)TT[v] * (37 * R[v]) * 4;
        const long long issue = (waves + 3) / 4 * step;
        const long long cost = rounds * 1000000 + rounds * max(max(lds, issue), 120 + step);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = v; }
    }
    return best;
}
__device__ __forceinline__ void schur_rows_any() {
    switch (schur_rows_pick(lbg_s.bo1 - lbg_s.bo0)) {
        case 0: schur_rows<6, 1>(); break;
        case 1: schur_rows<3, 1>(); break;
        case 2: schur_rows<2, 2>(); break;
        default: schur_rows<1, kSchurTasks>(); break;
    }
}
