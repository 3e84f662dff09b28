// Fragment of lba_g2o.hip, included inside its namespace; not a standalone header.  Update, relabel, outputs.
// this member's landmarks [h0, h1) (Hessian order) and keyframes [k0, k1)
struct Share { int h0, h1, k0, k1; };
__device__ __forceinline__ Share my_share(const Sh& s, int K) {
    return Share{split_lo(s.nl, s.m, s.T), split_lo(s.nl, s.m + 1, s.T), split_lo(K, s.m, s.T), split_lo(K, s.m + 1, s.T)};
}
// landmark increments (xl = Dinv (bl - Hpl^T xp), Dinv as the Schur phase formed it), push, update
// (block_solver.hpp:444-471, oplus); this member's landmarks and keyframes.  After a failed solve nothing of x was
// written (block_solver.hpp:447-457: the landmark part is formed only after a successful pose solve) and g2o still
// applies it: every vertex moves by the previous solution (optimization_algorithm_levenberg.cpp:110-115).
__device__ __noinline__ void update() {
    const G& g = lbg_g;
    const Sh& s = lbg_s;
    const int t = threadIdx.x;
    const int np = s.np, n = 6 * np;
    const bool ok = s.ok;
    const double lam = s.lambda;
    const Share sh = my_share(s, g.K);
    for (int h = sh.h0 + t; h < sh.h1; h += kT) {
        const int l = g.hidx_lm[h];
        if (l < g.Np) for (int j = 0; j < 3; j++) g.X_b[3 * l + j] = g.X[3 * l + j];
        else for (int j = 0; j < 4; j++) g.P_b[4 * (l - g.Np) + j] = g.P[4 * (l - g.Np) + j];
        double xl[3];
        if (ok) {
            double cl[3] = {g.bl[3 * h], g.bl[3 * h + 1], g.bl[3 * h + 2]};
            PMask m = pm_ld(g.lmh_mask + h);
            int bk = g.lmh_blk[h];
            while (pm_any(m)) {
                const int p = pm_ffs(m);
                pm_pop(m);
                auto B = g.blkB + (size_t)18 * bk++;
                for (int i = 0; i < 3; i++) {
                    double sm = 0;
                    for (int r = 0; r < 6; r++) sm += B[3 * r + i] * (-g.x[6 * p + r]);
                    cl[i] += sm;
                }
            }
            double H[9], Di[9], db[3];
            for (int j = 0; j < 9; j++) H[j] = g.Hll[9 * h + j];
            landmark_dinv(H, cl, lam, Di, db);  // (db unused)
            for (int i = 0; i < 3; i++) xl[i] = (Di[3 * i] * cl[0] + Di[3 * i + 1] * cl[1]) + Di[3 * i + 2] * cl[2];
            for (int j = 0; j < 3; j++) g.x[n + 3 * h + j] = xl[j];
        } else {
            for (int j = 0; j < 3; j++) xl[j] = g.x[n + 3 * h + j];
        }
        if (l < g.Np) {
            for (int j = 0; j < 3; j++) g.X[3 * l + j] += xl[j];
        } else {
            auto pp = g.P + 4 * (l - g.Np);
            P4 P{{pp[0], pp[1], pp[2], pp[3]}};
            p_oplus(P, xl);
            for (int j = 0; j < 4; j++) pp[j] = P.c[j];
        }
    }
    for (int k = sh.k0 + t; k < sh.k1; k += kT) {
        for (int j = 0; j < 7; j++) g.pose_b[7 * k + j] = g.pose[7 * k + j];
        const int h = s.hidx[k];
        if (h < 0) continue;
        double u[6];
        for (int j = 0; j < 6; j++) u[j] = g.x[6 * h + j];
        store_pose(g.pose + 7 * k, se3_mul(se3_exp(u), load_pose(g.pose + 7 * k)));
    }
}

__device__ __noinline__ void restore() {  // pop(): this member's landmarks and keyframes
    const G& g = lbg_g;
    const Sh& s = lbg_s;
    const int t = threadIdx.x;
    const Share sh = my_share(s, g.K);
    for (int h = sh.h0 + t; h < sh.h1; h += kT) {
        const int l = g.hidx_lm[h];
        if (l < g.Np) for (int j = 0; j < 3; j++) g.X[3 * l + j] = g.X_b[3 * l + j];
        else for (int j = 0; j < 4; j++) g.P[4 * (l - g.Np) + j] = g.P_b[4 * (l - g.Np) + j];
    }
    for (int k = sh.k0 + t; k < sh.k1; k += kT)
        for (int j = 0; j < 7; j++) g.pose[7 * k + j] = g.pose_b[7 * k + j];
}

// computeScale terms x_j (lambda x_j + b_j), poses then landmarks (Hessian order), zero-padded to 32; this member's
// share of the entries
__device__ __noinline__ void scale_terms() {
    const G& g = lbg_g;
    const Sh& s = lbg_s;
    const int t = threadIdx.x;
    const int n = 6 * s.np, tot = n + 3 * s.nl, pad = lbg_pad32(tot);
    const double lam = s.lambda;
    for (int j = split_lo(pad, s.m, s.T) + t; j < split_lo(pad, s.m + 1, s.T); j += kT) {
        double v = 0.0;
        if (j < tot) {  // (x as update() applied it: after a failed solve, the previous solution)
            const double b = j < n ? g.Hps[27 * (j / 6) + 21 + j % 6] : g.bl[j - n];
            const double x = g.x[j];
            v = x * (lam * x + b);
        }
        g.sc[j] = v;
    }
}

// relabel between the passes with the errors cached by the last computeActiveErrors (Optimizer.cc:1815-1851); this
// member's edges
__device__ __noinline__ void relabel() {
    const LbaConsts& C = lbg_c;
    const G& g = lbg_g;
    const Sh& s = lbg_s;
    for (int e = split_lo(g.E, s.m, s.T) + threadIdx.x; e < split_lo(g.E, s.m + 1, s.T); e += kT) {
        double info[3];
        const int ty = g.e_type[e];
        info_of(g, C, e, ty, info);
        const double chi = chi2_of(g.err + 3 * e, info, edge_dim(ty));
        bool bad;
        if (ty == 0) bad = chi > 5.991 || !depth_positive(g, e);
        else if (ty == 1) bad = chi > 7.815 || !depth_positive(g, e);
        else if (ty == 2) bad = chi > C.plane_chi;
        else bad = chi > C.vp_chi;
        if (bad) g.e_level[e] = 1;
    }
}

// computeActiveErrors (+ the plane edges' Jacobians at the same state): this member's edges
__device__ __noinline__ void errors_phase() {
    const G& g = lbg_g;
    const Sh& s = lbg_s;
    errors();
    const int npl = g.E - g.Ep;
    plane_jacobians(g.Ep + split_lo(npl, s.m, s.T), g.Ep + split_lo(npl, s.m + 1, s.T));
}

// ---------------------------------------------------------------- outputs
__device__ __noinline__ void outputs(const LbgBatch& b, int p) {
    const LbaConsts& C = lbg_c;
    const G& g = lbg_g;
    Sh& s = lbg_s;
    const int t = threadIdx.x;
    const spslam_lba_problem pb = b.io.probs[p];
    if (s.stopped == 1) {  // returned before optimizing: the map is untouched, nothing is erased
        // (setup did not run: the observations are addressed through the input records)
        for (int i = t; i < g.Np; i += kT)
            for (int o = g.pt[i].obs_offset; o < g.pt[i].obs_offset + g.pt[i].n_obs; o++) b.io.pobs_out[o] = 0;
        for (int i = t; i < g.Nq; i += kT)
            for (int o = g.pl[i].obs_offset; o < g.pl[i].obs_offset + g.pl[i].n_obs; o++) b.io.plobs_out[o] = 0;
        for (int i = t; i < 16 * g.K; i += kT) b.io.kf_out[16 * (size_t)pb.kf_offset + i] = g.kf[i / 16].Tcw[i % 16];
        for (int i = t; i < 3 * g.Np; i += kT) b.io.pt_out[3 * (size_t)pb.point_offset + i] = g.pt[i / 3].xw[i % 3];
        for (int i = t; i < 4 * g.Nq; i += kT) b.io.pl_out[4 * (size_t)pb.plane_offset + i] = g.pl[i / 4].world[i % 4];
        if (t == 0) {
            spslam_lba_result* r = b.io.res + p;
            *r = spslam_lba_result{};
            r->stopped = 1;
        }
        return;
    }
    int cnt[2] = {0, 0};
    for (int e = t; e < g.E; e += kT) {
        double info[3];
        const int ty = g.e_type[e];
        info_of(g, C, e, ty, info);
        const double chi = chi2_of(g.err + 3 * e, info, edge_dim(ty));
        if (ty <= 1) {
            const bool bad = chi > (ty == 0 ? 5.991 : 7.815) || !depth_positive(g, e);
            b.io.pobs_out[g.e_src[e]] = bad;
            cnt[0] += bad;
        } else {
            const bool bad = ty == 2 ? chi > C.plane_chi : chi > C.vp_chi;
            b.io.plobs_out[g.e_src[e]] = bad;
            cnt[1] += bad;
        }
    }
    int tot0, tot1;
    block_scan(cnt[0], &tot0, s.iscan);
    block_scan(cnt[1], &tot1, s.iscan);
    for (int k = t; k < g.K; k += kT) {
        float* o = b.io.kf_out + 16 * ((size_t)pb.kf_offset + k);
        if (g.kf[k].fixed) {
            for (int j = 0; j < 16; j++) o[j] = g.kf[k].Tcw[j];
            continue;
        }
        const SE3 T = load_pose(g.pose + 7 * k);
        const M3 Rm = q_to_rot(T.r);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) o[4 * i + j] = (float)Rm.a[3 * i + j];
        o[3] = (float)T.t.x; o[7] = (float)T.t.y; o[11] = (float)T.t.z;
        o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
    }
    for (int i = t; i < g.Np; i += kT)
        for (int j = 0; j < 3; j++) b.io.pt_out[3 * ((size_t)pb.point_offset + i) + j] = (float)g.X[3 * i + j];
    for (int i = t; i < g.Nq; i += kT)
        for (int j = 0; j < 4; j++) b.io.pl_out[4 * ((size_t)pb.plane_offset + i) + j] = (float)g.P[4 * i + j];
    if (t == 0) {
        spslam_lba_result* r = b.io.res + p;
        *r = spslam_lba_result{};
        r->iterations[0] = s.its[0];
        r->iterations[1] = s.its[1];
        r->n_point_outliers = tot0;
        r->n_plane_outliers = tot1;
        r->status = s.fail ? -3 : 0;
        r->trials = s.trials;
        r->stopped = s.stopped;
    }
}
