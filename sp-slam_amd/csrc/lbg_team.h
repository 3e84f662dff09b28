// Fragment of lba_g2o.hip, included inside its namespace; not a standalone header.  Team barrier, lane helpers, shares.
// ---------------------------------------------------------------- the team
// A problem is solved by T workgroups (members; T = b.team), one per CU.  Membership follows arrival: each
// workgroup takes a ticket (ctl[0]) when it starts; tickets p T .. p T + T - 1 form problem p's team, member 0 (the
// leader) being the first.  A member therefore only ever waits for workgroups that already run, or for the next
// workgroup to be dispatched -- never for one queued behind a waiting member -- so teams cannot deadlock however many
// launches share the chip.  Every member runs the same schedule: the serial steps (setup, structure + AMD, the
// factorisation) on the leader, the parallel ones split over the members, the LM control replicated (each member
// computes the same ordered sums from the same global arrays and takes the same decisions).  Phases meet at
// team_sync, the inter-workgroup hand-off of MI355X_MICROARCH.md ("valid forms"): every storing wave drains its
// stores (s_waitcnt vmcnt(0)), a workgroup barrier, one lane releases at agent scope (buffer_wbl2: the XCD's L2
// written back), drains again (the explicit wait the ROCm 7.2 compiler may drop after the release), and adds to the
// team's counter with a relaxed agent atomic; it polls the counter with relaxed agent loads (sc1: L2, not L1), then
// acquires at agent scope (buffer_inv sc1: this CU's L1 invalidated), drains, and a workgroup barrier lets the other
// waves read with plain loads.  The leader also samples the caller's pbStopFlag before it releases; every member
// reads that sample after the barrier, so all members see the flag change at the same barrier.
__device__ __forceinline__ int* team_ctr(const LbgBatch& b, int p) { return b.ctl + 16 * (p + 1); }
__device__ __noinline__ void team_sync(const LbgBatch& b) {
    Sh& s = lbg_s;
    const G& g = lbg_g;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const int gen = ++s.gen;  // this barrier's number
        bool seen = false;
        if (s.m == 0 && b.io.stop && !s.stop)
            seen = __hip_atomic_load(b.io.stop + s.p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
        if (s.T > 1) {
            // the sample is published as the barrier number it belongs to: a member that reads the record late
            // (after the leader has entered a later barrier) still takes the flag at the same barrier as the others
            if (seen) g.team->stop_gen = gen;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            int* ctr = team_ctr(b, s.p);
            __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int target = s.T * gen;
            while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target)
                __builtin_amdgcn_s_sleep(1);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const int sg = g.team->stop_gen;
            seen = sg != 0 && sg <= gen;
        }
        if (seen) s.stop = 1;  // latched (SparseOptimizer::terminate())
    }
    __syncthreads();
}
__device__ __forceinline__ int split_lo(int n, int m, int T) { return (int)(((long long)n * m) / T); }

// ---------------------------------------------------------------- workgroup primitives
__device__ __forceinline__ int block_and(int v, Sh& s) {
    const int w = threadIdx.x >> 6;
    const bool all = __all(v != 0);
    if ((threadIdx.x & 63) == 0) s.iscan[w] = all;
    __syncthreads();
    int r = 1;
#pragma unroll
    for (int j = 0; j < kW; j++) r &= s.iscan[j];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double rl(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ uint64_t rl64(uint64_t v, int l) {
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}
// value of entry i of a vector spread over the wave (entry 64 m + lane in register m)
template <int kC>
__device__ __forceinline__ double pick(const double (&v)[kC], int i) {
    double r = rl(v[0], i & 63);  // (wave-uniform selects, no branches)
#pragma unroll
    for (int m = 1; m < kC; m++) {
        const double q = rl(v[m], i & 63);
        r = (i >> 6) == m ? q : r;
    }
    return r;
}
__device__ __forceinline__ int4 ld_i4(const gint* p) {  // one 16-byte load (p 16-byte aligned)
    typedef int v4i __attribute__((ext_vector_type(4)));
    const v4i v = *(const v4i GL*)p;
    return make_int4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// ---------------------------------------------------------------- the members' shares (leader, per pass)
// Published in the team record with the structure state the members copy (load_team):
//  * the Schur complement by block rows: every pattern block's chain length (the landmarks whose active edges see
//    both of its poses), the rows (pose i1 with its blocks (i1, i2 >= i1)) dealt to the members by work, largest
//    first to the least loaded (LPT), each member's blocks longest first in g.bord[bo[m] .. bo[m + 1]) -- a member
//    then forms BDinv only for its own rows (schur());
//  * buildSystem: the landmarks in list order -- their edges are one contiguous range -- cut into T runs of about
//    equal work (a plane edge weighs kPlaneW point edges: the Jacobians of its landmark side and of its pose side are
//    read back from the numeric-differentiation pass), and the free poses dealt by edge count, largest first,
//    snaking (build_system()).
constexpr int kPlaneW = 4;
__device__ __forceinline__ int snake_pick(int j, int m, int T) { return j * T + ((j & 1) ? T - 1 - m : m); }
__device__ __noinline__ void team_plan() {
    const G& g = lbg_g;
    Sh& s = lbg_s;
    const int t = threadIdx.x;
    const int np = s.np, nl = s.nl, T = s.T;
    LbgTeam GL* R = g.team;
    int* len = (int*)lbg_dyn;                        // [nb]
    int* brow = len + kMaxK * (kMaxK + 1) / 2;       // [nb] block -> its row i1
    int* rowoff = brow + kMaxK * (kMaxK + 1) / 2;    // [np]
    int* prank = rowoff + kMaxK;                     // [np] free poses by edge count
    int* rw = prank + kMaxK;                         // [np] row work
    int* rmem = rw + kMaxK;                          // [np] row -> member
    if (t == 0) {  // block ids: (i, i) -> i; (i1 < i2) -> rowoff[i1] + rank of i2 among row i1's bits above i1
        int o = np;
        for (int a = 0; a < np; a++) {
            rowoff[a] = o;
            o += pm_popc(s.pat[a]) - 1;
        }
        s.nb = o;
    }
    __syncthreads();
    const int nb = s.nb;
    for (int i = t; i < nb; i += kT) len[i] = 0;
    if (t < np) {
        brow[t] = t;
        for (int j = rowoff[t]; j < rowoff[t] + pm_popc(s.pat[t]) - 1; j++) brow[j] = t;
    }
    __syncthreads();
    for (int h = t; h < nl; h += kT) {
        PMask a = pm_ld(g.lmh_mask + h);
        while (pm_any(a)) {
            const int i1 = pm_ffs(a);
            pm_pop(a);
            atomicAdd(&len[i1], 1);
            const PMask row = pm_andnot(s.pat[i1], pm_bit(i1));
            PMask b2 = a;
            while (pm_any(b2)) {
                const int i2 = pm_ffs(b2);
                pm_pop(b2);
                atomicAdd(&len[rowoff[i1] + pm_popc_below(row, i2)], 1);
            }
        }
    }
    if (t < np) {
        const int c = g.pe_off[t + 1] - g.pe_off[t];
        int r = 0;
        for (int q = 0; q < np; q++) {
            const int v = g.pe_off[q + 1] - g.pe_off[q];
            r += v > c || (v == c && q < t);
        }
        prank[r] = t;
    }
    __syncthreads();
    if (t < np) {  // a row's work: its blocks' chains (+1 each: the block's own cost)
        int w = len[t] + 1;
        for (int j = rowoff[t]; j < rowoff[t] + pm_popc(s.pat[t]) - 1; j++) w += len[j] + 1;
        rw[t] = w;
    }
    __syncthreads();
    if (t == 0) {  // LPT: rows by work, each to the least loaded member
        long long load[kLbgTeamMax];
        PMask rm[kLbgTeamMax];
        for (int mm = 0; mm < T; mm++) { load[mm] = 0; rm[mm] = pm_zero(); }
        PMask done = pm_zero();
        for (int q = 0; q < np; q++) {
            int best = -1;
            for (int a = 0; a < np; a++)
                if (!pm_test(done, a) && (best < 0 || rw[a] > rw[best])) best = a;
            pm_set(done, best);
            int mm = 0;
            for (int u = 1; u < T; u++)
                if (load[u] < load[mm]) mm = u;
            load[mm] += rw[best];
            pm_set(rm[mm], best);
            rmem[best] = mm;
        }
        int o = 0;
        for (int mm = 0; mm < T; mm++) {  // blocks per member -> the members' segments of bord
            R->bo[mm] = o;
            for (int k = 0; k < kPW; k++) R->rmask[mm * kPW + k] = rm[mm].w[k];
            for (int a = 0; a < np; a++)
                if (pm_test(rm[mm], a)) o += pm_popc(s.pat[a]);
        }
        R->bo[T] = o;
    }
    __syncthreads();
    for (int i = t; i < nb; i += kT) {  // each member's blocks longest first (ties: block id)
        const int w = len[i], mi = rmem[brow[i]];
        int r = 0;
        for (int j = 0; j < nb; j++) {
            const int v = len[j];
            r += rmem[brow[j]] == mi && (v > w || (v == w && j < i));
        }
        g.bord[R->bo[mi] + r] = i;
    }
    // landmark runs: exclusive prefix of the edge weights in list order; run m ends after the landmark whose weight
    // interval holds W m / T
    int Wt = 0;
    {
        int tot = 0;
        for (int ch = 0; ch < g.L; ch += kT) {
            int tt;
            block_scan(ch + t < g.L ? g.lm_nb[ch + t] * (ch + t < g.Np ? 1 : kPlaneW) : 0, &tt, s.iscan);
            tot += tt;
        }
        Wt = tot;
    }
    if (t <= T) R->eb[t] = t == 0 ? 0 : g.E;
    __syncthreads();
    {
        int base = 0;
        for (int ch = 0; ch < g.L; ch += kT) {
            const int l = ch + t;
            const int w = l < g.L ? g.lm_nb[l] * (l < g.Np ? 1 : kPlaneW) : 0;
            int tt;
            const int ex = block_scan(w, &tt, s.iscan) + base;
            for (int mm = 1; mm < T; mm++) {
                const long long tgt = ((long long)Wt * mm) / T;
                if (w > 0 && ex < tgt && tgt <= ex + w) R->eb[mm] = g.lm_boff[l] + g.lm_nb[l];
            }
            base += tt;
        }
    }
    if (t == 0) {
        int o = 0;
        for (int mm = 0; mm < T; mm++) {
            R->npo[mm] = o;
            for (int j = 0; j * T < np; j++) {
                const int r = snake_pick(j, mm, T);
                if (r < np) R->pown[o++] = prank[r];
            }
        }
        R->npo[T] = o;
        R->np = np; R->nl = nl; R->nact = s.nact; R->nch = s.nch; R->nb = nb; R->unsup = 0;
    }
    if (t < kMaxK)
        for (int k = 0; k < kPW; k++) R->pat[t * kPW + k] = t < np ? s.pat[t].w[k] : 0ull;
    for (int k = t; k < g.K; k += kT) R->hidx[k] = s.hidx[k];
    __syncthreads();
}

// every member (after the team_sync that follows the leader's structure pass): the shared structure state into LDS,
// and this member's shares
__device__ __noinline__ void load_team() {
    const G& g = lbg_g;
    Sh& s = lbg_s;
    const int t = threadIdx.x;
    const LbgTeam GL* R = g.team;
    if (s.m != 0) {
        if (t == 0) {
            s.unsup = R->unsup;
            s.np = R->np; s.nl = R->nl; s.nact = R->nact; s.nch = R->nch; s.nb = R->nb;
        }
        for (int k = t; k < g.K; k += kT) s.hidx[k] = R->hidx[k];
        if (t < kMaxK)
            for (int k = 0; k < kPW; k++) s.pat[t].w[k] = R->pat[t * kPW + k];
    }
    const int o0 = R->npo[s.m], o1 = R->npo[s.m + 1];
    if (t == 0) {
        s.eb0 = R->eb[s.m];
        s.eb1 = R->eb[s.m + 1];
        s.npown = o1 - o0;
        s.bo0 = R->bo[s.m];
        s.bo1 = R->bo[s.m + 1];
        for (int k = 0; k < kPW; k++) s.rmask.w[k] = R->rmask[s.m * kPW + k];
    }
    if (t < o1 - o0) s.pown[t] = R->pown[o0 + t];
    __syncthreads();
}
