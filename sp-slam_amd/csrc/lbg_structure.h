// Fragment of lba_g2o.hip, included inside its namespace; not a standalone header.  Setup and the per-pass structure.
// ---------------------------------------------------------------- setup (once)
__device__ __noinline__ void setup() {
    const G& g = lbg_g;
    Sh& s = lbg_s;
    int* dyn_i = (int*)lbg_dyn;
    const int t = threadIdx.x;
    for (int k = t; k < g.K; k += kT) {  // Converter::toSE3Quat
        const auto* T = g.kf[k].Tcw;
        M3 Rm;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Rm.a[3 * i + j] = T[4 * i + j];
        SE3 q;
        q.r = q_from_rot(Rm);
        q.t = V3{T[3], T[7], T[11]};
        q_normalize(q.r);
        store_pose(g.pose + 7 * k, q);
    }
    for (int i = t; i < g.Np; i += kT)
        for (int j = 0; j < 3; j++) g.X[3 * i + j] = g.pt[i].xw[j];
    for (int i = t; i < g.Nq; i += kT) {
        const P4 q = plane_from_f(g.pl[i].world);
        for (int j = 0; j < 4; j++) g.P[4 * i + j] = q.c[j];
    }
    // edges in insertion order: point observations (points in list order), then plane observations
    int base_e = 0;
    for (int ch = 0; ch < g.L; ch += kT) {
        const int l = ch + t;
        const int n_obs = l < g.Np ? g.pt[l].n_obs : (l < g.L ? g.pl[l - g.Np].n_obs : 0);
        int tot;
        const int off = block_scan(n_obs, &tot, s.iscan) + base_e;
        if (l < g.L) {
            g.lm_boff[l] = off;
            g.lm_nb[l] = n_obs;
            const int src0 = l < g.Np ? g.pt[l].obs_offset : g.pl[l - g.Np].obs_offset;
            for (int o = 0; o < n_obs; o++) {
                const int e = off + o;
                g.e_lm[e] = l;
                g.e_src[e] = src0 + o;
                g.e_level[e] = 0;
                if (l < g.Np) {
                    const auto& ob = g.pobs[src0 + o];
                    g.e_kf[e] = ob.kf;
                    g.e_type[e] = ob.ur < 0 ? 0 : 1;
                } else {
                    const auto& ob = g.plobs[src0 + o];
                    g.e_kf[e] = ob.kf;
                    g.e_type[e] = ob.kind == SPSLAM_PLANE_EDGE ? 2 : (ob.kind == SPSLAM_PARALLEL_EDGE ? 3 : 4);
                }
            }
        }
        base_e += tot;
    }
    for (int e = g.E + t; e < lbg_pad32(g.E); e += kT) g.echi[e] = 0.0;
    // g2o's solution buffer (Solver::_x): written only by successful solves and read by every update, so a failed
    // solve re-applies the previous solution; never written = zeros (update())
    for (int j = t; j < lbg_pad32(6 * lbg_free_cap(g.K, kPW) + 3 * g.L); j += kT) g.x[j] = 0.0;
    // landmark (vertex-id) order: points by id (ids mnId + maxKFid + 1), then planes by id (mnId + maxPointid + 1,
    // above every point id); stable ranks (id, list index)
    for (int grp = 0; grp < 2; grp++) {
        const int n0 = grp ? g.Np : 0, cnt = grp ? g.Nq : g.Np;
        auto id_of = [&](int i) { return grp ? g.pl[i].id : g.pt[i].id; };
        int ok = 1;
        for (int i = t; i + 1 < cnt; i += kT) ok &= id_of(i) <= id_of(i + 1);
        if (block_and(ok, s)) {
            for (int i = t; i < cnt; i += kT) g.lm_sorted[n0 + i] = n0 + i;
            continue;
        }
        // rank counting over LDS tiles of ids; ranks accumulate in lm_hidx (free until the structure phase)
        for (int i = t; i < cnt; i += kT) g.lm_hidx[n0 + i] = 0;
        constexpr int kTile = kDyn / 4;
        for (int b0 = 0; b0 < cnt; b0 += kTile) {
            const int nt = min(kTile, cnt - b0);
            __syncthreads();
            for (int j = t; j < nt; j += kT) dyn_i[j] = id_of(b0 + j);
            __syncthreads();
            for (int i = t; i < cnt; i += kT) {
                const int id = id_of(i);
                int r = 0;
                for (int j = 0; j < nt; j++) {
                    const int v = dyn_i[j];
                    r += v < id || (v == id && b0 + j < i);
                }
                g.lm_hidx[n0 + i] += r;
            }
        }
        __syncthreads();
        for (int i = t; i < cnt; i += kT) g.lm_sorted[n0 + g.lm_hidx[n0 + i]] = n0 + i;
        __syncthreads();
    }
    __syncthreads();
}

__device__ __forceinline__ bool coupled(const Sh& s, int q1, int q2) {  // pose blocks (q1, q2) in the Schur pattern
    return q1 <= q2 ? pm_test(s.pat[q1], q2) : pm_test(s.pat[q2], q1);
}
template <class PU>
__device__ __forceinline__ bool bit_of(const PU* bits, int i) { return (bits[i >> 6] >> (i & 63)) & 1ull; }

// ---------------------------------------------------------------- structure (per optimize() pass)
// initializeOptimization(0) + buildStructure + LinearSolverEigen's symbolic analysis
__device__ __noinline__ void structure() {
    const G& g = lbg_g;
    Sh& s = lbg_s;
    unsigned char* dyn = lbg_dyn;
    const int t = threadIdx.x, lane = t & 63;
    for (int k = t; k < g.K; k += kT) {
        s.kact[k] = 0;
        s.hidx[k] = -1;
    }
    __syncthreads();
    int na = 0;
    for (int e = t; e < g.E; e += kT)
        if (g.e_level[e] == 0) {
            s.kact[g.e_kf[e]] = 1;  // (every writer stores the same value)
            na++;
        }
    int nact;
    block_scan(na, &nact, s.iscan);
    if (t == 0) s.nact = nact;
    __syncthreads();
    if (t == 0) {  // free poses with an active edge, by id (buildIndexMapping over the id-sorted active vertices)
        int np = 0;
        for (int k = 0; k < g.K; k++) {
            const auto& kk = g.kf[k];
            if (!s.kact[k] || kk.fixed || kk.id == 0) continue;
            if (np == kMaxK) { np++; break; }  // more free poses than the pose masks hold: status -2
            int j = np++;
            while (j > 0 && g.kf[s.hpose[j - 1]].id > kk.id) { s.hpose[j] = s.hpose[j - 1]; j--; }
            s.hpose[j] = k;
        }
        s.unsup = np > kMaxK;
        s.dense = 0;
        if (!s.unsup)
            for (int j = 0; j < np; j++) s.hidx[s.hpose[j]] = (short)j;
        s.np = s.unsup ? 0 : np;
    }
    __syncthreads();
    if (s.unsup) return;
    const int np = s.np;
    // landmarks with an active edge in id order; pose masks of their active edges (the Hpl blocks) and of all
    // their edges (buildStructure's Schur pattern walks v->edges(), any level)
    int base = 0;
    for (int ch = 0; ch < g.L; ch += kT) {
        const int j = ch + t;
        const int l = j < g.L ? g.lm_sorted[j] : -1;
        int act = 0;
        PMask mask = pm_zero(), amask = pm_zero();
        if (l >= 0)
            for (int e = g.lm_boff[l]; e < g.lm_boff[l] + g.lm_nb[l]; e++) {
                const int h = s.hidx[g.e_kf[e]];
                if (h >= 0) pm_set(amask, h);
                if (g.e_level[e] == 0) {
                    act = 1;
                    if (h >= 0) pm_set(mask, h);
                }
            }
        int tot;
        const int off = block_scan(act, &tot, s.iscan) + base;
        if (l >= 0) {
            g.lm_hidx[l] = act ? off : -1;
            pm_st(g.lm_amask + l, amask);
            if (act) {
                g.hidx_lm[off] = l;
                pm_st(g.lmh_mask + off, mask);
            }
        }
        base += tot;
    }
    const int nl = base;
    if (t == 0) s.nl = nl;
    // Hpl blocks of landmark h at lmh_blk[h] .. (pose order), contiguous in landmark order
    base = 0;
    for (int ch = 0; ch < nl; ch += kT) {
        const int h = ch + t;
        const int c = h < nl ? pm_popc(pm_ld(g.lmh_mask + h)) : 0;
        int tot;
        const int off = block_scan(c, &tot, s.iscan) + base;
        if (h < nl) g.lmh_blk[h] = off;
        base += tot;
    }
    if (t == 0) g.lmh_blk[nl] = base;
    __syncthreads();
    // the Schur phase's landmark chunks: groups of kSchurLm landmarks, split greedily where a group's Hpl blocks
    // exceed kSchurBlk (a landmark has at most 64 blocks); sch[c] = first landmark of chunk c, sch_kb its first block
    {
        int nc = 0;
        const int ng = (nl + kSchurLm - 1) / kSchurLm;
        for (int pass2 = 0; pass2 < 2; pass2++) {
            int base2 = 0;
            for (int ch = 0; ch < ng; ch += kT) {
                const int gi = ch + t;
                int cntc = 0;
                if (gi < ng) {
                    const int h0 = gi * kSchurLm, h1 = min(nl, h0 + kSchurLm);
                    int k0 = g.lmh_blk[h0];
                    cntc = 1;
                    for (int h = h0 + 1; h < h1; h++) {
                        const int kh = g.lmh_blk[h + 1];
                        if (kh - k0 > kSchurBlk) { k0 = g.lmh_blk[h]; cntc++; }
                    }
                }
                int tot;
                const int off = block_scan(cntc, &tot, s.iscan) + base2;
                if (pass2 == 1 && gi < ng) {
                    const int h0 = gi * kSchurLm, h1 = min(nl, h0 + kSchurLm);
                    int k0 = g.lmh_blk[h0], o = off;
                    g.sch[o] = h0;
                    g.sch_kb[o++] = k0;
                    for (int h = h0 + 1; h < h1; h++) {
                        const int kh = g.lmh_blk[h + 1];
                        if (kh - k0 > kSchurBlk) { k0 = g.lmh_blk[h]; g.sch[o] = h; g.sch_kb[o++] = k0; }
                    }
                }
                base2 += tot;
            }
            nc = base2;
        }
        if (t == 0) {
            g.sch[nc] = nl;
            g.sch_kb[nc] = g.lmh_blk[nl];
            s.nch = nc;
        }
    }
    if (t < np) s.pat[t] = pm_bit(t);
    __syncthreads();
    for (int l = t; l < g.L; l += kT) {
        const int h = g.lm_hidx[l];
        const PMask mask = h >= 0 ? pm_ld(g.lmh_mask + h) : pm_zero();
        const int b0 = g.lm_boff[l], e1 = b0 + g.lm_nb[l], kb = h >= 0 ? g.lmh_blk[h] : 0;
        for (int e = b0; e < e1; e++) {
            int eb = -1;
            const int ph = s.hidx[g.e_kf[e]];
            const bool on = g.e_level[e] == 0;
            if (h >= 0 && on && ph >= 0) eb = kb + pm_popc_below(mask, ph);
            g.e_blk[e] = eb;
            // build_system's row record: RI (the edge's Hpl block, -1 none, -2 inactive), the landmark's segment
            g.eseg[4 * e] = on ? eb : -2;
            g.eseg[4 * e + 1] = h;
            g.eseg[4 * e + 2] = e1;
            g.eseg[4 * e + 3] = kb | (e == b0 ? 1 << 30 : 0);
        }
        if (h >= 0) {
            const PMask am0 = pm_ld(g.lm_amask + l);
            PMask am = am0;
            while (pm_any(am)) {
                const int i1 = pm_ffs(am);
                const PMask row = pm_andnot(am0, pm_below(i1));
                for (int k = 0; k < kPW; k++)
                    if (row.w[k]) atomicOr((unsigned long long*)&s.pat[i1].w[k], (unsigned long long)row.w[k]);
                pm_pop(am);
            }
        }
    }
    // per free pose, its active edges in insertion order: a stable bucketing in one pass over the edges (round 5 ran
    // a block scan over all edges per pose: np x E / 512 scans).  Counts per pose, their prefix = pe_off; then per
    // chunk of kT edges each edge's rank among the chunk's earlier edges of its pose -- within its wave from the
    // lanes that share the pose (one ballot per distinct pose of the wave), across waves from the per-wave counts
    // taken in wave order -- after the edges of earlier chunks (run).
    {
        int* cnt = (int*)dyn;          // [kW][kMaxK] this chunk's per-wave counts
        int* run = cnt + kW * kMaxK;   // [kMaxK] edges placed so far, then (first) the totals
        const int wv = t >> 6;
        auto pose_of = [&](int e) { return e < g.E && g.e_level[e] == 0 ? (int)s.hidx[g.e_kf[e]] : -1; };
        for (int k = t; k < kMaxK; k += kT) run[k] = 0;
        __syncthreads();
        for (int e = t; e < g.E; e += kT) {
            const int h = pose_of(e);
            if (h >= 0) atomicAdd(&run[h], 1);
        }
        __syncthreads();
        if (t == 0) {
            int o = 0;
            for (int hh = 0; hh < np; hh++) {
                g.pe_off[hh] = o;
                o += run[hh];
            }
            g.pe_off[np] = o;
        }
        __syncthreads();
        for (int k = t; k < kMaxK; k += kT) run[k] = 0;
        for (int ch = 0; ch < g.E; ch += kT) {
            for (int k = t; k < kW * kMaxK; k += kT) cnt[k] = 0;
            __syncthreads();
            const int e = ch + t, h = pose_of(e);
            int rank = 0;
            uint64_t rem = __ballot(h >= 0);
            while (rem) {
                const int hq = __builtin_amdgcn_readlane(h, __builtin_ctzll(rem));
                const uint64_t m = __ballot(h == hq);
                if (h == hq) rank = __popcll(m & (lane == 0 ? 0ull : ~0ull >> (64 - lane)));
                if (lane == 0) cnt[wv * kMaxK + hq] = __popcll(m);
                rem &= ~m;
            }
            __syncthreads();
            if (h >= 0) {
                int base = g.pe_off[h] + run[h] + rank;
                for (int w = 0; w < wv; w++) base += cnt[w * kMaxK + h];
                g.pe_idx[base] = e;
            }
            __syncthreads();
            for (int k = t; k < np; k += kT) {
                int a = 0;
                for (int w = 0; w < kW; w++) a += cnt[w * kMaxK + k];
                run[k] += a;
            }
            __syncthreads();  // (the next chunk clears cnt)
        }
    }
    team_plan();
    // ---- LinearSolverEigen::computeSymbolicDecomposition (analyzePattern, Eigen's AMD)
    const int n = 6 * np;
    if (n == 0) {
        if (t == 0) g.rs_off[0] = 0;
        __syncthreads();
        return;
    }
    if (t < np) {
        int c = 0;
        for (int q = 0; q < np; q++) c += coupled(s, t, q);
        s.pdeg[t] = c;
    }
    __syncthreads();
    const int dense = min(n - 2, max(16, (int)(10 * sqrt((double)n))));
    int alld = 1;
    for (int q = t; q < np; q += kT) alld &= 6 * s.pdeg[q] > dense;
    int full = 1;  // every pose coupled with every other
    for (int q = t; q < np; q += kT) full &= pm_eq(s.pat[q], pm_andnot(pm_first_n(np), pm_below(q)));
    full = block_and(full, s);
    if (block_and(alld, s)) {
        if (t == 0) s.dense = full;
        for (int k = t; k < n; k += kT) g.Pinv[k] = k;  // every scalar dense: absorbed in index order (natural)
    } else {
        // full symmetric pattern (diagonal kept), columns sorted; cs_amd's elbow room
        int cnz = 0;
        for (int q = 0; q < np; q++) cnz += 36 * s.pdeg[q];
        const int tcap = cnz + cnz / 5 + 2 * n;
        const bool in_lds = (size_t)(tcap + 10 * (n + 1)) * 4 <= (size_t)kDyn;
        int* Ci = in_lds ? (int*)dyn : (int*)g.amd_Ci;
        int* W = in_lds ? Ci + tcap : (int*)g.amd_W;
        int* perm = W + 8 * (n + 1);
        int* Cp = perm + (n + 1);
        for (int tt = t; tt < n; tt += kT) {
            const int q2 = tt / 6;
            int c0 = 0;
            for (int q = 0; q < q2; q++) c0 += 6 * s.pdeg[q];
            c0 *= 6;
            c0 += (tt - 6 * q2) * 6 * s.pdeg[q2];
            Cp[tt] = c0;
            int c = c0;
            for (int q = 0; q < np; q++)
                if (coupled(s, q, q2))
                    for (int rr = 0; rr < 6; rr++) Ci[c++] = 6 * q + rr;
        }
        if (t == 0) Cp[n] = cnz;
        __syncthreads();
        if (t == 0) amd_order(n, Cp, Ci, tcap, W, perm);
        __syncthreads();
        for (int k = t; k < n; k += kT) g.Pinv[k] = perm[k];
        __syncthreads();
    }
    for (int k = t; k < n; k += kT) g.Pm[g.Pinv[k]] = k;
    __syncthreads();
    // lower structure of each column j of ap = P a P^T: Abits[j] = {i > j : (Pinv j, Pinv i) in the pattern}
    for (int tt = t; tt < n; tt += kT) {
        const int qj = g.Pinv[tt] / 6;
        uint64_t wv[kNW] = {};
        for (int i = tt + 1; i < n; i++)
            if (coupled(s, qj, g.Pinv[i] / 6)) wv[i >> 6] |= 1ull << (i & 63);
#pragma unroll
        for (int w = 0; w < kNW; w++) g.Abits[tt * kNW + w] = wv[w];
    }
    __syncthreads();
    // elimination tree and L's column structures: struct L(:, j) = Abits[j] U (children's structures \ {j});
    // one lane per bitset word
    if (t < 64) {
        uint64_t* acc = (uint64_t*)dyn;  // n x kNW
        for (int i = lane; i < n * kNW; i += 64) acc[i] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int j = 0; j < n; j++) {
            uint64_t S = 0;
            if (lane < kNW) S = g.Abits[j * kNW + lane] | acc[j * kNW + lane];
            const uint64_t nz = __ballot(lane < kNW && S != 0);
            int par = -1;
            if (nz) {
                const int fw = __ffsll((unsigned long long)nz) - 1;
                const uint64_t wv = rl64(S, fw);
                par = 64 * fw + __ffsll((unsigned long long)wv) - 1;
            }
            if (lane < kNW) {
                g.Lbits[j * kNW + lane] = S;
                if (par >= 0) {
                    const uint64_t keep = (par >> 6) == lane ? ~(1ull << (par & 63)) : ~0ull;
                    acc[par * kNW + lane] |= S & keep;
                }
            }
            if (lane == 0) g.parent[j] = par;  // (each lane reads and writes its own word of acc only)
        }
        // the factorisation's masked-step structure words (a ring step past a piece's end reads row n's kC words:
        // all of them zero, not only the first -- the rest would be whatever an earlier call left in the scratch)
        if (lane < kNW) g.Lbits[n * kNW + lane] = 0;
    }
    __syncthreads();
    // each row k of L: its pattern {i : k in struct L(:, i)} in factorize_preordered's order -- ap's column k
    // entries in source order (original index ascending), an elimination-tree walk from each, the walks' paths
    // stacked so that the last path comes first, each path from its start upwards
    int rs_base = 0;
    for (int k0 = 0; k0 < n; k0 += kT) {  // rows k0 .. k0 + kT - 1 (one pass for n <= kT)
        const int k = k0 + t;
        int cnt = 0;
        if (k < n)
            for (int i = 0; i < k; i++) cnt += bit_of(g.Lbits + i * kNW, k);
        int tot;
        const int off = block_scan(cnt, &tot, s.iscan) + rs_base;
        rs_base += tot;
        if (k < n) g.rs_off[k] = off;
        if (k0 + kT >= n && t == 0) g.rs_off[n] = rs_base;
        if (k < n && cnt > 0) {
            const int ok = g.Pinv[k];
            uint64_t vis[kNW] = {};
            vis[k >> 6] |= 1ull << (k & 63);
            auto seg = g.rs_idx + off;
            int wpos = 0;
            for (int o2 = 0; o2 < n; o2++) {
                const int r = g.Pm[o2];
                if (r >= k || !coupled(s, o2 / 6, ok / 6)) continue;
                int i = r;
                while (!((vis[i >> 6] >> (i & 63)) & 1ull)) {
                    vis[i >> 6] |= 1ull << (i & 63);
                    seg[wpos++] = i;
                    i = g.parent[i];
                }
            }
            // paths were written in discovery order: reverse the whole row, then each path back to start-upwards
            for (int a = 0, b2 = cnt - 1; a < b2; a++, b2--) {
                const int v = seg[a];
                seg[a] = seg[b2];
                seg[b2] = v;
            }
            int a = 0;
            while (a < cnt) {  // a reversed path: consecutive entries (prev, next) with parent[next] == prev
                int b2 = a;
                while (b2 + 1 < cnt && g.parent[seg[b2 + 1]] == seg[b2]) b2++;
                for (int x = a, y = b2; x < y; x++, y--) {
                    const int v = seg[x];
                    seg[x] = seg[y];
                    seg[y] = v;
                }
                a = b2 + 1;
            }
        }
    }
    __syncthreads();
}
