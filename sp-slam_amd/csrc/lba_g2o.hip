// gfx950 LocalBundleAdjustment in g2o's own arithmetic (reference: src/Optimizer.cc:1154-1977 on the vendored
// g2o SparseOptimizer + OptimizationAlgorithmLevenberg + BlockSolver_6_3 + LinearSolverEigen, g2oAddition plane
// edges).  Semantics: oracle/lba_oracle.cpp, which this reproduces bit for bit.
//
// One persistent 512-thread workgroup per problem runs the whole schedule -- setup, optimize(5), relabel,
// optimize(10), outputs -- with no host round trip and no cross-workgroup hand-off; many problems (the local maps
// of many sequences) run side by side, one per CU.  Every order-sensitive sum follows g2o:
//   chi2          activeRobustChi2: one lane adds the edges' robust chi2 in edge-insertion order (the others
//                 evaluate the errors first; inactive edges contribute an exact +0.0);
//   Hll, bl, Hpl  per landmark, its edges in insertion order (one thread per landmark);
//   Hpp, bp       per free pose and term, its edges in insertion order (one lane per (pose, term) chain);
//   Schur         Hschur = Hpp (+ lambda), then landmark by landmark in landmark-index (vertex-id) order
//                 Hi1i2 -= BDinv Bj^T and Bb += Bi db (block_solver.hpp:381-431): one lane per (block row of a
//                 pattern block, i.e. (i1, i2, r)) holds the row's six entries and subtracts each landmark's
//                 contribution in order;
//   factor/solve  Eigen SimplicialLDLT<Upper> on g2o's Hschur pattern: AMD ordering (the scalar
//                 minimum_degree_ordering, one lane; every scalar dense -> the natural order at once), elimination
//                 tree and L's column patterns as bitsets, each row's topological pattern order from the same
//                 tree walks, then the up-looking factorisation on one wave (y in registers, one lane per row of
//                 the reduced system, the pattern order's steps as readlane broadcasts), Eigen's triangular solves;
//   scale         computeScale: x . (lambda x + b) over poses then landmarks, one lane.
// The quadratic-form terms of every edge (Jacobians: analytic for points, central differences for planes on lane
// pairs), errors and updates run in parallel.  Floating-point expressions are the oracle's (g2o_restated.h,
// eigen_simplicial_restated.h); DESIGN.md section 3.9.
//
// This file holds the constants, the LDS and global state (Sh, G), the schedule kernel and its launcher; the phases
// are fragments it includes in this order inside its namespace (one translation unit per instance, so the LDS objects
// keep their namespace-scope names; the fragments are not standalone headers):
//   lbg_pmask.h      PMask and the pm_* operations
//   lbg_team.h       team_sync, the lane helpers, team_plan / load_team (the members' shares)
//   lbg_amd.h        amd_order (Eigen's minimum_degree_ordering, one lane)
//   lbg_structure.h  setup, structure (active sets, Schur pattern, symbolic analysis)
//   lbg_build.h      errors and their ordered sums, edge terms, plane_jacobians, build_system
//   lbg_schur.h      landmark_dinv, schur, schur_rows
//   lbg_factor.h     factor_body, factor_dense*, solve_dense_packed, factor_solve
//   lbg_update.h     update, restore, scale_terms, relabel, errors_phase, outputs
// The edge arithmetic itself is lba_edge_math.h, shared with lba_kernels.hip.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "g2o_device.h"
#include "lba_edge_math.h"
#include "lba_launch.h"

// Two instances of this file are compiled (itself and lba_g2o_wide.hip): LBG_PW = 1 (pose masks of one 64-bit
// word: up to 64 free poses, n <= 384) and LBG_PW = 2 (two words: up to 128 free poses, n <= 768).  The narrow one is
// the round-5 kernel unchanged in its arithmetic; the host runs the wide one for windows of more than 64 keyframes.
#ifndef LBG_PW
#define LBG_PW 1
#endif
#if LBG_PW == 1
#define LBG_NS lbag
#define LBG_RUN lba_run_g2o_pw1
#else
#define LBG_NS lbag2
#define LBG_RUN lba_run_g2o_pw2
#endif

namespace spslam {
namespace LBG_NS {

using namespace g2od;
using namespace edge_math;

constexpr int kT = kLbgThreads, kW = kT / 64;
constexpr int kMaxKF = kLbgMaxKeyframes;  // keyframes (local + fixed)
constexpr int kPW = LBG_PW;               // 64-bit words of a pose mask
constexpr int kMaxK = 64 * kPW;           // free poses (Hessian blocks)
constexpr int kNW = 6 * kPW;              // bitset words for up to 6 * kMaxK scalars
constexpr int kDyn = 136 * 1024;        // dynamic LDS (setup tiles, AMD workspace, the factorisation's L)
constexpr int kDynAlloc = (LBG_PW == 1 ? 154 : 152) * 1024;  // allocated: kDyn plus the Schur phase's staged Bb
                                                              //   terms and block tables (static LDS + this <= 160 KB)
                                        //   (every phase but the Schur one sizes itself against kDyn)
constexpr int kLdsN = LBG_PW == 1 ? 96 : 90;  // reduced systems of n <= kLdsN rows factorised in LDS (L, S packed:
                                               //   133 KB; the wide instance's structure words take more)
constexpr int kSchurLm = 64;            // Schur phase: landmarks per staged chunk (one bit each in a 64-bit mask)
constexpr int kSchurBlk = LBG_PW == 1 ? 412 : 360;  //   and Hpl blocks per chunk (the staging buffer, 16 doubles a
                                                    //   thread, + BDinv; the wide instance's tables take more)

// Global-memory pointers typed with the global address space: G lives in LDS and the phase functions are not
// inlined, so a generic pointer would make every access a FLAT instruction (which also counts against the LDS
// wait counter, so LDS reads would wait for every outstanding global load).
#define GL __attribute__((address_space(1)))
typedef double GL gdouble;
typedef int GL gint;
typedef uint64_t GL guint64;

#include "lbg_pmask.h"

struct Sh {
    double red[kW][4];
    int iscan[kW];
    PMask pat[kMaxK];                   // Schur block pattern: row i1, bits i2 >= i1
    short hidx[kMaxKF];                 // keyframe -> free-pose Hessian index (-1: fixed or inactive)
    unsigned char kact[kMaxKF];         // structure: keyframes with an active edge
    int hpose[kMaxK];                   // Hessian index -> keyframe
    int pdeg[kMaxK];                    // poses coupled with each pose (itself included)
    int np, nl, nact, nch, nb, flag, unsup, dense;
    // the team (one workgroup per member, lba_g2o's header): problem, member, size, barrier generation; this
    // member's buildSystem share (landmark-aligned edge range, its free poses)
    int p, m, T, gen, eb0, eb1, npown, bo0, bo1;
    PMask rmask;                        // this member's Schur block rows
    PMask carry;                        // buildSystem: Hpl blocks touched by the landmark continuing into the next step
    double csum[2][12];                 //   and its partial Hll / bl sums (by step parity)
    int pown[kMaxK];
    // LM / schedule state (every member computes it identically between barriers)
    int pass, it, max_it, robust, qmax, nBad, trials, its[2], stop, stopped, ok, need_err, done, accepted, fail;
    double lambda, ni, currentChi, iniChi, tempChi, scale;
    long long ph[8], tlast, tB;  // diagnostics: wall_clock64 ticks per phase (result phase_us[1..7])
    long long dg[14];            // SPSLAM_LBG_DIAG sub-phase ticks
};
// thread 0 charges the time since the previous mark to phase k (called right after a barrier)
#define LBG_MARK(k)                                  \
    if (threadIdx.x == 0) {                          \
        const long long now_ = wall_clock64();       \
        s.ph[k] += now_ - s.tlast;                   \
        s.tlast = now_;                              \
    }

struct G {
    int K, Np, Nq, L, E, Ep;
    const spslam_lba_keyframe GL* kf;
    const spslam_lba_point GL* pt;
    const spslam_lba_plane GL* pl;
    const spslam_lba_point_obs GL* pobs;
    const spslam_lba_plane_obs GL* plobs;
    gdouble *pose, *pose_b, *X, *X_b, *P, *P_b, *err, *echi, *sc, *terms, *Hll, *bl, *Dinv, *db, *blkB, *Hps,
        *S, *bs, *x, *Ld;
    gint *e_lm, *e_kf, *e_type, *e_level, *e_src, *e_blk, *lm_boff, *lm_nb, *lm_sorted, *lm_hidx, *hidx_lm, *lmh_blk,
        *pe_off, *pe_idx, *Pinv, *Pm, *parent, *rs_off, *rs_idx, *amd_Ci, *amd_W, *sch, *sch_kb,
        *eseg,   // per edge: {RI, landmark hidx, segment end, first block | segment start << 30}
        *bord;   // Schur pattern blocks, longest chain first
    PMask GL *lmh_mask, *lm_amask;
    guint64 *Lbits, *Abits;
    LbgTeam GL* team;
};

// The workgroup's LDS objects at namespace scope: the phase functions are not inlined, and a pointer or reference
// argument would reach them as a generic (flat) address -- every LDS access a FLAT instruction, which also waits on
// the outstanding global loads.  Referenced by name, they compile to ds_* instructions.
extern __shared__ __attribute__((aligned(16))) unsigned char lbg_dyn[];
__shared__ Sh lbg_s;
__shared__ G lbg_g;
__shared__ LbaConsts lbg_c;

__device__ G make_g(const LbgBatch& b, int p) {
    const spslam_lba_problem pb = b.io.probs[p];
    G g;
    g.K = pb.n_kf; g.Np = pb.n_points; g.Nq = pb.n_planes;
    g.Ep = pb.n_point_obs; g.E = pb.n_point_obs + pb.n_plane_obs; g.L = g.Np + g.Nq;
    g.kf = (const spslam_lba_keyframe GL*)(b.io.kfs + pb.kf_offset);
    g.pt = (const spslam_lba_point GL*)(b.io.pts + pb.point_offset);
    g.pl = (const spslam_lba_plane GL*)(b.io.pls + pb.plane_offset);
    g.pobs = (const spslam_lba_point_obs GL*)b.io.pobs;
    g.plobs = (const spslam_lba_plane_obs GL*)b.io.plobs;
    const LbgLayout Ly = lbg_layout(g.K, g.Np, g.Nq, g.E, kPW);
    uint8_t* base = b.scratch + b.scratch_off[p];
    auto D = [&](size_t o) { return (double GL*)(base + o); };
    auto I = [&](size_t o) { return (int GL*)(base + o); };
    g.pose = D(Ly.pose); g.pose_b = D(Ly.pose_b); g.X = D(Ly.X); g.X_b = D(Ly.X_b); g.P = D(Ly.P); g.P_b = D(Ly.P_b);
    g.err = D(Ly.err); g.echi = D(Ly.echi); g.sc = D(Ly.sc); g.terms = D(Ly.terms); g.Hll = D(Ly.Hll);
    g.bl = D(Ly.bl); g.Dinv = D(Ly.Dinv); g.db = D(Ly.db); g.blkB = D(Ly.blkB);
    g.Hps = D(Ly.Hps); g.S = D(Ly.S); g.bs = D(Ly.bs); g.x = D(Ly.x); g.Ld = D(Ly.Ld);
    g.e_lm = I(Ly.e_lm); g.e_kf = I(Ly.e_kf); g.e_type = I(Ly.e_type); g.e_level = I(Ly.e_level);
    g.e_src = I(Ly.e_src); g.e_blk = I(Ly.e_blk); g.lm_boff = I(Ly.lm_boff); g.lm_nb = I(Ly.lm_nb);
    g.lm_sorted = I(Ly.lm_sorted); g.lm_hidx = I(Ly.lm_hidx); g.hidx_lm = I(Ly.hidx_lm); g.lmh_blk = I(Ly.lmh_blk);
    g.pe_off = I(Ly.pe_off); g.pe_idx = I(Ly.pe_idx); g.Pinv = I(Ly.Pinv); g.Pm = I(Ly.Pm); g.parent = I(Ly.parent);
    g.rs_off = I(Ly.rs_off); g.rs_idx = I(Ly.rs_idx); g.amd_Ci = I(Ly.amd_Ci); g.amd_W = I(Ly.amd_W);
    g.sch = I(Ly.sch); g.sch_kb = I(Ly.sch_kb); g.eseg = I(Ly.eseg); g.bord = I(Ly.bord);
    g.lmh_mask = (PMask GL*)(base + Ly.lmh_mask); g.lm_amask = (PMask GL*)(base + Ly.lm_amask);
    g.Lbits = (uint64_t GL*)(base + Ly.Lbits); g.Abits = (uint64_t GL*)(base + Ly.Abits);
    g.team = (LbgTeam GL*)(base + Ly.team);
    return g;
}

#include "lbg_team.h"

// ---------------------------------------------------------------- edge math (oracle/lba_oracle.cpp)
__device__ __forceinline__ void info_of_src(const G& g, const LbaConsts& C, int src, int t, double* info) {
    edge_math::info_of(C, t, t <= 1 ? g.pobs[src].inv_sigma2 : 0.0f, info);
}
__device__ __forceinline__ void info_of(const G& g, const LbaConsts& C, int e, int t, double* info) {
    info_of_src(g, C, t <= 1 ? g.e_src[e] : 0, t, info);
}
// A point edge's operands, loaded together (errors() gathers several edges' before evaluating any)
__device__ __forceinline__ PointIn point_in(const G& g, int kf, int lm, int src) {
    PointIn a;
    a.T = load_pose(g.pose + 7 * kf);
    for (int i = 0; i < 3; i++) a.X[i] = g.X[3 * lm + i];
    const auto& o = g.pobs[src];
    a.u = o.u; a.v = o.v; a.ur = o.ur; a.isg = o.inv_sigma2;
    const auto& k = g.kf[kf];
    a.fx = k.fx; a.fy = k.fy; a.cx = k.cx; a.cy = k.cy; a.bf = k.bf;
    return a;
}
__device__ bool depth_positive(const G& g, int e) {
    const SE3 T = load_pose(g.pose + 7 * g.e_kf[e]);
    const int lm = g.e_lm[e];
    if (g.e_type[e] <= 1) return edge_math::depth_positive(T, true, g.X + 3 * lm);
    return edge_math::depth_positive(T, false, g.P + 4 * (lm - g.Np));
}

// SparseOptimizer::terminate(): the caller's flag as the leader sampled it at the last team_sync (latched in s.stop),
// or the deterministic test hook (spslam_lba_debug_stop_after) on the replicated trial count
__device__ __forceinline__ bool stop_requested(const LbgBatch& b, Sh& s) {
    if (!s.stop && b.stop_after >= 0 && s.trials >= b.stop_after) s.stop = 1;
    return s.stop != 0;
}

#include "lbg_amd.h"
#include "lbg_structure.h"
#include "lbg_build.h"
#include "lbg_schur.h"
#include "lbg_factor.h"
#include "lbg_update.h"

// ---------------------------------------------------------------- the schedule
__global__ __launch_bounds__(kT) void k_lba_g2o(LbgBatch b, LbaConsts C) {
    unsigned char* dyn = lbg_dyn;
    Sh& s = lbg_s;
    const int t = threadIdx.x;
    if (t == 0) {  // the team ticket (lba_g2o's header: membership by arrival)
        const int T = b.team;
        const int slot = __hip_atomic_fetch_add(b.ctl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s.p = slot / T;
        s.m = slot - s.p * T;
        s.T = T;
        s.gen = 0;
        lbg_g = make_g(b, s.p);
        lbg_c = C;
    }
    __syncthreads();
    const int p = s.p;
    const bool lead = s.m == 0;
    const G& g = lbg_g;
    const long long t0 = wall_clock64();
    if (g.K > kMaxKF) {  // (every member leaves here)
        if (lead && t == 0) {
            b.io.res[p] = spslam_lba_result{};
            b.io.res[p].status = -2;
        }
        return;
    }
    if (t == 0) {
        s.stop = 0; s.stopped = 0; s.trials = 0; s.its[0] = s.its[1] = 0; s.fail = 0; s.robust = 1; s.done = 0;
        s.unsup = 0;
        for (int i = 0; i < 8; i++) s.ph[i] = 0;
        for (int i = 0; i < 14; i++) s.dg[i] = 0;
        s.tB = 0;
        s.tlast = t0;
        if (lead) g.team->stop_gen = 0;
    }
    team_sync(b);  // the leader's first sample of pbStopFlag
    if (t == 0 && stop_requested(b, s)) {  // if(*pbStopFlag) return; before initializeOptimization
        s.stopped = 1;
        s.done = 1;
    }
    __syncthreads();
#ifdef SPSLAM_LBG_PROBE  // diagnostic: the cost of the building blocks of the ordered chains inside this kernel
    double probe[4] = {0, 0, 0, 0};
    if (t < 64) {
        const double a = (double)g.E * 1e-9;
        const int lane = t & 63;
        double x = 1.0, yv = (double)lane * 1e-3, z = 0.0;
        long long c0 = clock64();
        for (int i = 0; i < 4096; i++) x = x + a;  // (1) dependent v_add_f64
        long long c1 = clock64();
        for (int i = 0; i < 4096; i++) z = z + rl(yv, i & 63);  // (2) + a v_readlane operand
        long long c2 = clock64();
        int k = lane;
        for (int i = 0; i < 4096; i++) k = __builtin_amdgcn_readlane(k, (k + i) & 63) & 63;  // (3) readlane -> lane select
        long long c3 = clock64();
        probe[0] = (double)(c1 - c0) / 4096;
        probe[1] = (double)(c2 - c1) / 4096;
        probe[2] = (double)(c3 - c2) / 4096;
        probe[3] = x + z + k;
    }
#endif
    if (!s.done && lead) setup();  // (the members wait at the structure pass's team_sync)
    if (t == 0 && g.E == 0) s.done = 1;  // no edges: nothing to optimise, the map goes back through the converters
    __syncthreads();
    for (int pass = 0; pass < 2 && !s.done; pass++) {
        if (lead) {
            structure();
            if (t == 0) g.team->unsup = s.unsup;
        }
        team_sync(b);
        load_team();
        if (s.unsup) break;
        LBG_MARK(1);
        const int n = 6 * s.np;
        // the factorisation's operands in LDS for n <= kLdsN: L, its column structures, the rows' pattern orders, P
        const bool lds = n <= kLdsN;
        const FactorLds fl = factor_lds(n);  // (used when lds)
        uint64_t* LB = (uint64_t*)(dyn + fl.LB);
        int* RO = (int*)(dyn + fl.RO);
        int* RS = (int*)(dyn + fl.RS);
        int* PI = (int*)(dyn + fl.PI);
        if (t == 0) {
            s.it = 0; s.max_it = pass ? 10 : 5; s.need_err = 1;
        }
        __syncthreads();
        // SparseOptimizer::optimize on a graph without active edges (every edge relabelled): nothing to do
        const bool empty = s.nact == 0 || (s.np == 0 && s.nl == 0);
        // SparseOptimizer::optimize(max_it) with OptimizationAlgorithmLevenberg
        for (int it = 0; it < (empty ? 0 : pass ? 10 : 5); it++) {
            if (t == 0 && stop_requested(b, s)) {  // for (...; !terminate(); ...)
                s.stopped = pass == 0 && s.trials == 0 ? 1 : 2;
                s.done = 1;
            }
            __syncthreads();
            if (s.done) break;
            if (s.need_err) {
                LBG_MARK(1);
                errors_phase();
                team_sync(b);
                LBG_MARK(2);
                sums_staged(lbg_pad32(g.E), 0);
                __syncthreads();
                LBG_MARK(3);
            }
            if (t == 0) s.iniChi = s.currentChi;
            build_system();
            team_sync(b);
            LBG_MARK(4);
            if (t == 0) {
                double mx = 0.0;  // computeLambdaInit: the members' maxima
                for (int q = 0; q < s.T; q++) mx = fmax(mx, g.team->mx[q]);
                if (it == 0) { s.lambda = 1e-5 * mx; s.ni = 2; s.nBad = 0; }
                s.qmax = 0;
            }
            __syncthreads();
            double rho = 0.0;
            bool more = true;
            while (more) {
                LBG_MARK(1);
                // the row-group layout for teams of up to 4, and for any member with 16 or more blocks: it reads ~3x
                // fewer LDS bytes per block step than schur()'s lane per entry, which wins when the LDS is busy;
                // schur() splits a block's chain over 36 lanes, which wins for a few short chains (measured:
                // profiles/r06/schur_layouts.txt)
                if (s.T <= b.rows_max_team || s.bo1 - s.bo0 >= 16) schur_rows_any();
                else schur();
                team_sync(b);
                LBG_MARK(5);
                const bool forced = s.trials < 32 && ((b.fail_mask >> s.trials) & 1u);  // (test hook)
                if (lead && forced) {
                    if (t == 0) { s.ok = 0; g.team->ok = 0; }
                } else if (lead) {
                    if (lds) {  // the factorisation's symbolic data into LDS (the other phases use the same LDS)
                        for (int i = t; i < (n + 1) * kNW; i += kT) LB[i] = i < n * kNW ? g.Lbits[i] : 0ull;
                        for (int i = t; i <= n; i += kT) RO[i] = g.rs_off[i];
                        const int nz = g.rs_off[n];
                        for (int i = t; i < nz; i += kT) RS[i] = g.rs_idx[i];
                        for (int i = t; i < n; i += kT) PI[i] = g.Pinv[i];
                        double* SP = (double*)(dyn + fl.SP);  // S, packed upper
                        for (int i = t; i < n * n; i += kT) {
                            const int r = i / n, c = i - r * n;
                            if (r <= c) SP[(c * (c + 1)) / 2 + r] = g.S[i];
                        }
                        __syncthreads();
                    }
#ifdef SPSLAM_LBG_DIAG
                    const long long f0 = wall_clock64();
#endif
                    if (lds && s.dense) {  // every pose coupled, natural order: the rows pipelined over the waves
                        if (n <= 64) factor_dense<1>();
                        else factor_dense<2>();
                        if (t < 64) {
                            if (n <= 64) factor_solve<1, true, true>();
                            else factor_solve<2, true, true>();
                        }
                    } else if (s.dense && n <= kPackN) {  // dense, past the LDS copy: L packed in LDS
                        if (n <= 128) factor_dense_packed<2>();
                        else factor_dense_packed<3>();
                        if (t < 64) {
                            if (n <= 128) solve_dense_packed<2>();
                            else solve_dense_packed<3>();
                        }
                    } else if (t < 64) {
                        if (n <= 64) factor_solve<1, true>();
                        else if (n <= kLdsN) factor_solve<2, true>();
                        else if (n <= 128) factor_solve<2, false>();
                        else if (n <= 192) factor_solve<3, false>();
                        else if (n <= 256) factor_solve<4, false>();
                        else if (kPW == 1 || n <= 384) factor_solve<6, false>();
#if LBG_PW > 1
                        else if (n <= 512) factor_solve<8, false>();
                        else factor_solve<12, false>();
#endif
                    }
                    if (n == 0 && t == 0) s.ok = 1;
#ifdef SPSLAM_LBG_DIAG
                    if (t == 0) s.dg[5] += s.dg[4] - f0;
#endif
                    __syncthreads();
                    if (t == 0) g.team->ok = s.ok;
                }
                team_sync(b);
                if (!lead && t == 0) s.ok = g.team->ok;
                __syncthreads();
                LBG_MARK(6);
                update();
                team_sync(b);
                LBG_MARK(1);
                errors_phase();
                scale_terms();
                team_sync(b);
                LBG_MARK(2);
                sums_staged(lbg_pad32(g.E), lbg_pad32(n + 3 * s.nl));
                __syncthreads();
                LBG_MARK(3);
                if (t == 0) {
                    double tempChi = s.ok ? s.tempChi : DBL_MAX;
                    double r = s.currentChi - tempChi;
                    double scale = s.scale;
                    scale += 1e-3;
                    r /= scale;
                    if (r > 0 && isfinite(tempChi)) {
                        double alpha = 1. - libm64cr::cube_(2 * r - 1);
                        alpha = fmin(alpha, 2. / 3.);
                        s.lambda *= fmax(1. / 3., alpha);
                        s.ni = 2;
                        s.currentChi = tempChi;
                        s.accepted = 1;
                    } else {
                        s.lambda *= s.ni;
                        s.ni *= 2;
                        s.accepted = 0;
                    }
                    s.qmax++;
                    s.trials++;
                    s.red[0][2] = r;
                    const bool stop = stop_requested(b, s);
                    s.flag = r < 0 && s.qmax < 10 && !stop;  // do { ... } while (rho < 0 && qmax < max && !terminate())
                }
                __syncthreads();
                if (!s.accepted) {
                    restore();
                    team_sync(b);
                }
                rho = s.red[0][2];
                more = s.flag;
            }
            if (t == 0) {
                s.need_err = !s.accepted;  // an accepted trial's errors are the new state's (same operands, same bits)
                s.its[pass]++;
                bool term = s.qmax == 10 || rho == 0;
                if (!term) {
                    if ((s.iniChi - s.currentChi) * 1e3 < s.iniChi) s.nBad++;
                    else s.nBad = 0;
                    term = s.nBad >= 3;
                }
                s.flag = term;
                if (s.stop && !term && it + 1 < (pass ? 10 : 5)) {  // the next iteration's terminate() check
                    s.stopped = 2;
                    s.done = 1;
                }
            }
            __syncthreads();
            if (s.flag || s.done) break;
        }
        if (s.done) break;
        if (pass == 0) {
            if (t == 0 && stop_requested(b, s)) {  // bDoMore = !*pbStopFlag
                s.stopped = 2;
                s.done = 1;
            }
            __syncthreads();
            if (s.done) break;
            // relabel with the errors cached by the last computeActiveErrors, drop the robust kernels
            relabel();
            if (t == 0) s.robust = 0;
            team_sync(b);
        }
    }
    team_sync(b);  // every member's writes are in before the leader's outputs
    if (!lead) return;
    if (s.unsup) {  // more free poses than kMaxK: nothing written but the status
        if (t == 0) {
            b.io.res[p] = spslam_lba_result{};
            b.io.res[p].status = -2;
        }
        return;
    }
    outputs(b, p);
    if (t == 0) {  // setup / structure / update / decide, errors, ordered chains, terms, Schur, factor + solve, sums
        b.io.res[p].phase_us[0] = (float)((wall_clock64() - t0) * 0.01);
        for (int i = 1; i < 8; i++) b.io.res[p].phase_us[i] = (float)(s.ph[i] * 0.01);
        b.io.res[p].pad = (int)(s.tB * 0.01);  // diagnostic: build phase (B) us
#ifdef SPSLAM_LBG_DIAG_BUILD  // buildSystem: heads, (A) terms, landmark chains, Hpl blocks, pose chains (us); steps
        for (int i = 0; i < 5; i++) b.io.res[p].phase_us[1 + i] = (float)(s.dg[i] * 0.01);
        b.io.res[p].pad = (int)s.dg[5];
#endif
#ifdef SPSLAM_LBG_DIAG  // Schur: staging wait, BDinv, chains, commit; factor-only
        for (int i = 0; i < 4; i++) b.io.res[p].phase_us[1 + i] = (float)(s.dg[i] * 0.01);
        b.io.res[p].phase_us[5] = (float)(s.dg[6] * 1e-3);  // factor: step-loop shader kcycles,
        b.io.res[p].phase_us[6] = (float)(s.dg[7] * 1e-3);  //   pivot-update kcycles,
        b.io.res[p].pad = (int)s.dg[8];                     //   steps
        b.io.res[p].phase_us[7] = (float)(s.dg[5] * 0.01);
#endif
#ifdef SPSLAM_LBG_DIAG_SCHUR  // Schur chains: kcycles summed over waves, steps, cycles per step, sum of chunk maxima
        b.io.res[p].phase_us[1] = (float)(s.dg[10] * 1e-3);
        b.io.res[p].phase_us[2] = (float)s.dg[11];
        b.io.res[p].phase_us[3] = (float)s.dg[10] / (float)max(1ll, s.dg[11]);
        b.io.res[p].phase_us[4] = (float)(s.dg[13] * 1e-3);
#endif
#ifdef SPSLAM_LBG_PROBE  // shader-clock ticks per (1) add, (2) add of a readlane, (3) readlane chain
        for (int i = 0; i < 3; i++) b.io.res[p].phase_us[1 + i] = (float)probe[i];
        if (probe[3] == 12345.0) b.io.res[p].pad = 1;
#endif
    }
}

}  // namespace LBG_NS

hipError_t LBG_RUN(const LbgBatch& b, const LbaConsts& C, hipStream_t s, KernelTimer* timer) {
    using namespace LBG_NS;
    static const hipError_t attr =
        hipFuncSetAttribute((const void*)k_lba_g2o, hipFuncAttributeMaxDynamicSharedMemorySize, kDynAlloc);
    if (attr != hipSuccess) return attr;
    if (b.team < 1 || b.team > kLbgTeamMax) return hipErrorInvalidValue;
    const hipError_t z = hipMemsetAsync(b.ctl, 0, lbg_ctl_ints(b.n) * sizeof(int), s);
    if (z != hipSuccess) return z;
    if (timer) timer->begin(kKindLba, s);
    hipLaunchKernelGGL(k_lba_g2o, dim3(b.n * b.team), dim3(kT), kDynAlloc, s, b, C);
    if (timer) timer->end(kKindLba, s);
    return hipGetLastError();
}

}  // namespace spslam

#if LBG_PW == 1
namespace spslam {
// the instance of a batch: LbgBatch::pw (lbg_pw_for of its largest window)
hipError_t lba_run_g2o(const LbgBatch& b, const LbaConsts& C, hipStream_t s, KernelTimer* timer) {
    return b.pw == 1 ? lba_run_g2o_pw1(b, C, s, timer) : lba_run_g2o_pw2(b, C, s, timer);
}
}  // namespace spslam
#endif
