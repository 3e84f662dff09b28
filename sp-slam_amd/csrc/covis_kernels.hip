// gfx950 kernels for the covisibility graph and the two cullings of LocalMapping (include/spslam_gpu.h):
//   update_connections_kernel  KeyFrame::UpdateConnections   src/KeyFrame.cc:306-396, with AddConnection :128-141
//                                                            and UpdateBestCovisibles :143-162
//   keyframe_culling_kernel    LocalMapping::KeyFrameCulling src/LocalMapping.cc:644-711 (RGB-D branch), with the
//                                                            effect of KeyFrame::SetBadFlag's EraseObservation loop
//   map_point_culling_kernel   LocalMapping::MapPointCulling src/LocalMapping.cc:182-217
//
// update_connections_kernel: one 256-thread workgroup (four wave64) per problem.
//   1. counts: an LDS histogram over the sequence's keyframes (<= 1024), one atomicAdd per (match row, observer);
//   2. the first strict maximum by one LDS atomicMax of (count << 10 | 1023 - index), the number of counts >= th by
//      an LDS atomicAdd; the selected keyframes appended to an LDS list (their order does not matter: each is
//      handled on its own);
//   3. the keyframe's weights row = the histogram;
//   4. one work item per ordered list to write: item 0 the keyframe's own, item 1 + q selected keyframe q's.  A wave
//      takes items wave, wave + 4, ...: it compacts the list's (weight << 10 | index) keys into its own LDS buffer
//      (ballot + popcount) and sorts them descending inside the wave (no workgroup barrier: the waves work on
//      different lists): up to 64 keys, the usual case, one per lane by counting the greater ones; more, padded with
//      zeros to a power of two, by a bitonic network.  The keys are unique, so the order is the reference's
//      whatever the sort.  Nothing the launch writes is read back from memory: the one entry a neighbour's row
//      gains is taken from the histogram.
// LDS: 4 KiB histogram + 4 KiB selected list + 16 KiB keys.  Index work only: latency bound.
//
// keyframe_culling_kernel: one workgroup per problem, the candidates one after the other (each verdict changes
// what the next one sees); per candidate its keypoints over the threads, two LDS counters, the verdict on thread 0,
// the call's culled set as a 1024-bit LDS mask.
#include <hip/hip_runtime.h>

#include "covis_launch.h"
#include "wave_ops.h"

namespace spslam {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxKf = SPSLAM_COVIS_MAX_KF;
constexpr int kBest = SPSLAM_COVIS_BEST;
constexpr int kIdxBits = 10;
constexpr int kIdxMask = kMaxKf - 1;
static_assert(kMaxKf == 1 << kIdxBits, "the sort keys hold the keyframe index in their low bits");

__global__ __launch_bounds__(kThreads) void update_connections_kernel(const spslam_covis_problem* problems,
                                                                      spslam_covis_map M, spslam_covis_graph G,
                                                                      int th, spslam_covis_result* results) {
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    __shared__ int hist[kMaxKf];
    __shared__ int sel[kMaxKf];
    __shared__ int keys[kWaves][kMaxKf];
    __shared__ int best_s, n_over_s, n_sel_s, n_resorted_s, new_parent_s, n_own_s;
    const spslam_covis_problem pr = problems[p];
    const int nk = min(min(max(pr.n_kf, 0), kMaxKf), G.stride);
    const int kf = pr.kf;
    const size_t kfb = (size_t)pr.kf_base, rb = (size_t)pr.row_base;
    const size_t stride = (size_t)G.stride;

    // ---- 1. counts (:319-337)
    for (int j = t; j < nk; j += kThreads) hist[j] = 0;
    if (t == 0) { best_s = 0; n_over_s = 0; n_sel_s = 0; n_resorted_s = 0; new_parent_s = -1; n_own_s = 0; }
    __syncthreads();
    if (kf >= 0 && kf < nk) {
        const int m0 = M.match_off[kfb + kf], m1 = M.match_off[kfb + kf + 1];
        for (int e = m0 + t; e < m1; e += kThreads) {
            const int row = M.match_row[e];
            if (row < 0) continue;                                        // if(!pMP)
            if (M.point_bad && M.point_bad[rb + row]) continue;           // pMP->isBad()
            for (int o = M.obs_off[rb + row]; o < M.obs_off[rb + row + 1]; o++) {
                const int j = M.obs_kf[o];
                if (j != kf && j >= 0 && j < nk) atomicAdd(&hist[j], 1);  // KFcounter[mit->first]++
            }
        }
    }
    __syncthreads();

    // ---- 2. the maximum and the selection (:345-369)
    for (int j = t; j < nk; j += kThreads) {
        const int c = hist[j];
        if (c <= 0) continue;
        atomicMax(&best_s, (c << kIdxBits) | (kIdxMask - j));             // if(mit->second>nmax): the first maximum
        if (c >= th) atomicAdd(&n_over_s, 1);
    }
    __syncthreads();
    const int best = best_s;
    if (best == 0) {                                                      // if(KFcounter.empty()) return;
        if (t == 0) results[p] = spslam_covis_result{SPSLAM_COVIS_EMPTY, 0, -1, 0};
        return;
    }
    const bool by_th = n_over_s > 0;
    const int j_max = kIdxMask - (best & kIdxMask);
    auto selected = [&](int j) { return by_th ? hist[j] >= th : j == j_max; };
    for (int j = t; j < nk; j += kThreads)
        if (selected(j)) sel[atomicAdd(&n_sel_s, 1)] = j;

    // ---- 3. mConnectedKeyFrameWeights = KFcounter (:384)
    int32_t* own_row = G.weights + (kfb + kf) * stride;
    for (int j = t; j < nk; j += kThreads) own_row[j] = hist[j];
    __syncthreads();

    // ---- 4. the ordered lists: item 0 the keyframe's own (:371-386), item 1 + q AddConnection on sel[q] (:128-162)
    const int n_items = 1 + n_sel_s;
    int* key = keys[wave];
    for (int item = wave; item < n_items; item += kWaves) {
        const bool own = item == 0;
        const int x = own ? kf : sel[item - 1];
        const int32_t* row = G.weights + (kfb + x) * stride;
        if (!own) {
            if (row[kf] == hist[x]) continue;                             // the weight is unchanged: return
            if (lane == 0) {
                G.weights[(kfb + x) * stride + kf] = hist[x];
                atomicAdd(&n_resorted_s, 1);
            }
        }
        int m = 0;
        for (int i0 = 0; i0 < nk; i0 += 64) {
            const int i = i0 + lane;
            int w = 0;
            if (i < nk) w = own ? (selected(i) ? hist[i] : 0) : (i == kf ? hist[x] : row[i]);
            const bool keep = w > 0;
            const unsigned long long mask = __ballot(keep);
            if (keep) key[m + __popcll(mask & ((1ull << lane) - 1))] = (w << kIdxBits) | i;
            m += __popcll(mask);
        }
        // sort(vPairs) then push_front: weight descending, the higher index first on equal weight
        if (m <= 64) {
            // one key per lane: its place is the number of greater keys
            wave_sync();
            const int k = lane < m ? key[lane] : 0;
            int rank = 0;
            for (int b = 0; b < m; b++) rank += key[b] > k;
            wave_sync();
            if (lane < m) key[rank] = k;
            wave_sync();
        } else {
            // a bitonic network; the keys are positive, so the zeros that pad the list to a power of two sort
            // behind them
            int n_sort = 128;
            while (n_sort < m) n_sort <<= 1;
            for (int a = m + lane; a < n_sort; a += 64) key[a] = 0;
            wave_sync();
            for (int k = 2; k <= n_sort; k <<= 1)
                for (int j = k >> 1; j >= 1; j >>= 1) {
                    for (int q = lane; q < n_sort / 2; q += 64) {
                        const int a = ((q & ~(j - 1)) << 1) | (q & (j - 1)), b = a | j;  // they differ in bit j
                        const int ka = key[a], kb = key[b];
                        if ((ka < kb) == ((a & k) == 0)) { key[a] = kb; key[b] = ka; }
                    }
                    wave_sync();
                }
        }
        int32_t* ord = G.ordered + (kfb + x) * stride;
        int32_t* ord_w = G.ordered_w + (kfb + x) * stride;
        int32_t* cov = G.covis + (kfb + x) * kBest;
        for (int rank = lane; rank < m; rank += 64) {
            const int k = key[rank];
            const int idx = k & kIdxMask;
            ord[rank] = idx;
            ord_w[rank] = k >> kIdxBits;
            if (rank < kBest) cov[rank] = idx;
            if (own && rank == 0 && kf != 0 && G.first_connection[kfb + kf]) {  // :388-393
                G.parent[kfb + kf] = idx;
                G.first_connection[kfb + kf] = 0;
                new_parent_s = idx;
            }
        }
        if (lane >= m && lane < kBest) cov[lane] = -1;
        if (lane == 0) {
            G.n_ordered[kfb + x] = m;
            if (own) n_own_s = m;
        }
        wave_sync();  // the next item reuses the key buffer
    }
    __syncthreads();
    if (t == 0) results[p] = spslam_covis_result{SPSLAM_COVIS_UPDATED, n_own_s, new_parent_s, n_resorted_s};
}

__global__ __launch_bounds__(kThreads) void keyframe_culling_kernel(const spslam_cull_problem* problems,
                                                                    spslam_covis_map M, spslam_covis_graph G,
                                                                    CullFrames F, const uint8_t* new_plane,
                                                                    const uint8_t* not_erase,
                                                                    spslam_cull_params prm,
                                                                    spslam_cull_record* records,
                                                                    spslam_cull_summary* summaries) {
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63;
    __shared__ int cand[kMaxKf];
    __shared__ uint32_t culled[kMaxKf / 32];
    __shared__ int n_mps_s, n_red_s, n_culled_s;
    const spslam_cull_problem pr = problems[p];
    const int nk = min(max(pr.n_kf, 0), kMaxKf);
    const int kf = pr.kf;
    const size_t kfb = (size_t)pr.kf_base, rb = (size_t)pr.row_base;
    const size_t cap = (size_t)F.cap;
    if (kf < 0 || kf >= nk || new_plane[kfb + kf]) {                      // if(mpCurrentKeyFrame->mbNewPlane) return;
        if (t == 0) summaries[p] = spslam_cull_summary{0, SPSLAM_CULL_NEW_PLANE};
        return;
    }
    // vpLocalKeyFrames = GetVectorCovisibleKeyFrames(): the copy
    const int n = min(min(max(G.n_ordered[kfb + kf], 0), kMaxKf), G.stride);
    for (int q = t; q < n; q += kThreads) cand[q] = G.ordered[(kfb + kf) * (size_t)G.stride + q];
    if (t < kMaxKf / 32) culled[t] = 0;
    if (t == 0) n_culled_s = 0;
    __syncthreads();
    auto is_culled = [&](int j) { return (culled[j >> 5] >> (j & 31)) & 1u; };
    spslam_cull_record* out = records + pr.out_offset;

    for (int q = 0; q < n; q++) {
        const int c = cand[q];
        if (c <= 0 || c >= nk || new_plane[kfb + c]) {                    // if(pKF->mnId==0 || pKF->mbNewPlane) continue;
            if (t == 0) out[q] = spslam_cull_record{c, 0, 0, SPSLAM_CULL_SKIPPED};
            continue;
        }
        if (t == 0) { n_mps_s = 0; n_red_s = 0; }
        __syncthreads();
        const bool any_culled = n_culled_s > 0;
        const size_t slot_c = (size_t)M.kf_slot[kfb + c] * cap;
        const int m0 = M.match_off[kfb + c];
        const int len = min(M.match_off[kfb + c + 1] - m0, F.cap);
        int mps = 0, red = 0;
        for (int i = t; i < len; i += kThreads) {
            const int row = M.match_row[m0 + i];
            if (row < 0) continue;                                        // if(pMP)
            const size_t rr = rb + row;
            const int o0 = M.obs_off[rr], o1 = M.obs_off[rr + 1];
            // Observations() and isBad() after the EraseObservation of every keyframe culled so far
            int n_obs = M.points[rr].n_obs;
            bool touched = false;
            if (any_culled)
                for (int o = o0; o < o1; o++) {
                    const int j = M.obs_kf[o];
                    if (j < 0 || j >= nk || !is_culled(j)) continue;
                    touched = true;
                    n_obs -= F.uright[(size_t)M.kf_slot[kfb + j] * cap + M.obs_kp[o]] >= 0.f ? 2 : 1;
                }
            if ((M.point_bad && M.point_bad[rr]) || (touched && n_obs <= 2)) continue;  // if(!pMP->isBad())
            const float d = F.depth[slot_c + i];
            if (d > prm.th_depth || d < 0.f) continue;                    // mvDepth[i]>mThDepth || mvDepth[i]<0
            mps++;
            if (n_obs > prm.th_obs) {
                const int level = F.keys_un[slot_c + i].octave;
                int cnt = 0;
                for (int o = o0; o < o1; o++) {
                    const int j = M.obs_kf[o];
                    if (j == c || j < 0 || j >= nk || is_culled(j)) continue;
                    const int level_i = F.keys_un[(size_t)M.kf_slot[kfb + j] * cap + M.obs_kp[o]].octave;
                    if (level_i <= level + 1) cnt++;
                }
                if (cnt >= prm.th_obs) red++;
            }
        }
        mps = wave_sum(mps);
        red = wave_sum(red);
        if (lane == 0) {
            atomicAdd(&n_mps_s, mps);
            atomicAdd(&n_red_s, red);
        }
        __syncthreads();
        if (t == 0) {
            const int n_mps = n_mps_s, n_red = n_red_s;
            int status = SPSLAM_CULL_KEPT;
            if ((double)n_red > 0.9 * (double)n_mps) {                    // if(nRedundantObservations>0.9*nMPs)
                if (not_erase && not_erase[kfb + c]) {
                    status = SPSLAM_CULL_DEFERRED;                        // mbToBeErased = true; return;
                } else {
                    status = SPSLAM_CULL_CULLED;
                    culled[c >> 5] |= 1u << (c & 31);
                    n_culled_s = n_culled_s + 1;
                }
            }
            out[q] = spslam_cull_record{c, n_mps, n_red, status};
        }
        // the next candidate's first barrier orders these writes before its reads
    }
    if (t == 0) summaries[p] = spslam_cull_summary{n, SPSLAM_CULL_RAN};
}

__global__ __launch_bounds__(kThreads) void map_point_culling_kernel(spslam_point_cull_map M, const int32_t* rows,
                                                                     const int32_t* cur_kf_id, int n, int th_obs,
                                                                     uint8_t* verdict) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    const size_t r = (size_t)rows[k];
    const int age = cur_kf_id[k] - M.first_kf[r];                         // (int)nCurrentKFid-(int)pMP->mnFirstKFid
    uint8_t v = SPSLAM_POINT_CULL_KEEP;
    if (M.point_bad && M.point_bad[r]) v = SPSLAM_POINT_CULL_DROP;
    else if ((float)M.found[r] / (float)M.visible[r] < 0.25f) v = SPSLAM_POINT_CULL_BAD_RATIO;  // GetFoundRatio()
    else if (age >= 2 && M.points[r].n_obs <= th_obs) v = SPSLAM_POINT_CULL_BAD_OBS;
    else if (age >= 3) v = SPSLAM_POINT_CULL_EXPIRED;
    verdict[k] = v;
}

}  // namespace

hipError_t covis_update_connections_launch(int n_problems, const spslam_covis_problem* problems,
                                           const spslam_covis_map& map, const spslam_covis_graph& graph, int th,
                                           spslam_covis_result* results, hipStream_t s) {
    hipLaunchKernelGGL(update_connections_kernel, dim3(n_problems), dim3(kThreads), 0, s, problems, map, graph, th,
                       results);
    return hipGetLastError();
}

hipError_t keyframe_culling_launch(int n_problems, const spslam_cull_problem* problems, const spslam_covis_map& map,
                                   const spslam_covis_graph& graph, const CullFrames& frames,
                                   const uint8_t* new_plane, const uint8_t* not_erase, const spslam_cull_params& params,
                                   spslam_cull_record* records, spslam_cull_summary* summaries, hipStream_t s) {
    hipLaunchKernelGGL(keyframe_culling_kernel, dim3(n_problems), dim3(kThreads), 0, s, problems, map, graph, frames,
                       new_plane, not_erase, params, records, summaries);
    return hipGetLastError();
}

hipError_t map_point_culling_launch(const spslam_point_cull_map& map, const int32_t* rows, const int32_t* cur_kf_id,
                                    int n, int th_obs, uint8_t* verdict, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(map_point_culling_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, map, rows,
                       cur_kf_id, n, th_obs, verdict);
    return hipGetLastError();
}

}  // namespace spslam
