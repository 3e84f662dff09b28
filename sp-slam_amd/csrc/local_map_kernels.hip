// gfx950 kernel for Tracking::UpdateLocalMap (include/spslam_gpu.h, spslam_track_update_local_map_batch_device):
//   UpdateLocalKeyFrames  src/Tracking.cc:1463-1571 (observer votes, K1, the neighbour pass, pKFmax)
//   UpdateLocalPoints     src/Tracking.cc:1437-1460 (the local keyframes' map points, first occurrence kept)
//
// One 256-thread workgroup (four wave64) per frame, five phases separated by workgroup barriers:
//   1. votes: an LDS histogram over the sequence's keyframes (<= 1024), one atomicAdd per (frame point, observer);
//   2. K1 + neighbours on thread 0: both are order-defined serial walks over <= 1024 keyframes with the membership
//      flags (mnTrackReferenceForFrame == mCurrentFrame.mnId) in LDS;
//   3. the list's GetMapPointMatches() lengths prefix-summed (thread 0), so that entry e of the concatenation is
//      found by a binary search;
//   4. first position per point in the caller's scratch: every touched entry gets a sentinel, barrier, atomicMin
//      of the position, barrier.  Nothing is read before it is stored, so the scratch's contents on entry do not
//      matter;
//   5. ordered compaction in 256-entry chunks (wave ballot + popcount, wave totals in LDS, a running base): an
//      entry is kept where its position is its row's minimum, which is mvpLocalMapPoints' order exactly; then
//      the 80-byte records are gathered word by word.
// LDS: 4 KiB histogram + 4 KiB list + 4 KiB offsets + 1 KiB flags.  Index work only: HBM / latency bound.
#include <hip/hip_runtime.h>

#include "track_launch.h"

namespace spslam {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxKf = 1024;           // as refkf_vote_kernel's kMaxVoteKf
constexpr int kMaxLocalKf = 80;        // if(mvpLocalKeyFrames.size()>80) break;
constexpr int kRecordWords = sizeof(spslam_local_point) / 4;
constexpr int kNone = 0x7fffffff;

// A load served by L2, where this workgroup's atomics and write-through stores are: a line that another frame's
// workgroup on the same compute unit pulled into the vector L1 (slices of neighbouring frames can share one) may
// be stale there, and a workgroup barrier does not invalidate it.
__device__ __forceinline__ int load_l2(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void update_local_map_kernel(spslam_track_batch B, bool use_mm,
                                                                    spslam_local_map M, spslam_local_map_out O) {
    const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (O.state && O.state[f] == 2) return;  // LOST: TrackLocalMap does not run (:406-409)
    __shared__ int hist[kMaxKf];
    __shared__ int list[kMaxKf];
    __shared__ int moff[kMaxKf + 1];
    __shared__ uint8_t in_list[kMaxKf];
    __shared__ int n_list_s, kf_max_s, voted_s;
    __shared__ int wcnt[kThreads / 64];
    const int nk = M.n_kf;
    const size_t kfb = (size_t)M.kf_base[f], rb = (size_t)M.row_base[f];
    const int n_rows = O.scratch_stride;

    // ---- 1. votes (:1466-1483)
    for (int j = t; j < nk; j += kThreads) { hist[j] = 0; in_list[j] = 0; }
    __syncthreads();
    {
        const int cap = use_mm ? B.cap : M.cap;
        const int n = min(use_mm ? B.kp_counts[f] : M.kp_counts[f], cap);
        const size_t ko = (size_t)f * cap;
        for (int i = t; i < n; i += kThreads) {
            int row;
            if (use_mm) {
                const int e = B.edge_of_kp[ko + i];
                if (e < 0 || B.point_outlier[ko + e]) continue;
                const int id = B.proj_points[B.proj_frames[f].point_offset + B.proj_match[ko + i]].id;
                if (id < 0) continue;
                row = M.id_to_row ? M.id_to_row[(size_t)(M.id_base ? M.id_base[f] : 0) + id] : id;
            } else {
                row = M.frame_rows[ko + i];
            }
            if (row < 0 || row >= n_rows) continue;                   // mvpMapPoints[i] == NULL
            if (M.point_bad && M.point_bad[rb + row]) continue;       // pMP->isBad(): no vote
            for (int o = M.obs_off[rb + row]; o < M.obs_off[rb + row + 1]; o++) {
                const int j = M.obs_kf[o];
                if (j >= 0 && j < nk) atomicAdd(&hist[j], 1);        // keyframeCounter[it->first]++
            }
        }
    }
    __syncthreads();

    // ---- 2. K1 (:1485-1510) and the neighbours (:1513-1564), serial
    if (t == 0) {
        bool voted = false;
        int n = 0, mx = 0, best = -1;
        for (int j = 0; j < nk; j++) {
            if (hist[j] <= 0) continue;
            voted = true;
            if (M.kf_bad && M.kf_bad[kfb + j]) continue;
            if (hist[j] > mx) { mx = hist[j]; best = j; }             // if(it->second>max): the first maximum
            list[n++] = j;
            in_list[j] = 1;
        }
        if (voted) {
            const int k1 = n;
            for (int q = 0; q < k1; q++) {
                if (n > kMaxLocalKf) break;
                const size_t kf = kfb + list[q];
                for (int c = 0; c < 10; c++) {
                    const int nb = M.covis[kf * 10 + c];
                    if (nb < 0 || nb >= nk || (M.kf_bad && M.kf_bad[kfb + nb]) || in_list[nb]) continue;
                    list[n++] = nb;
                    in_list[nb] = 1;
                    break;
                }
                for (int o = M.child_off[kf]; o < M.child_off[kf + 1]; o++) {
                    const int ch = M.child[o];
                    if (ch < 0 || ch >= nk || (M.kf_bad && M.kf_bad[kfb + ch]) || in_list[ch]) continue;
                    list[n++] = ch;
                    in_list[ch] = 1;
                    break;
                }
                const int p = M.parent[kf];
                if (p >= 0 && p < nk && !in_list[p]) {                // no isBad() on the parent; break leaves the for
                    list[n++] = p;
                    in_list[p] = 1;
                    break;
                }
            }
        } else {
            n = min(max(O.n_local_kfs[f], 0), min(O.kf_cap, kMaxKf));  // return before clear(): the old list
        }
        n_list_s = n;
        kf_max_s = best;
        voted_s = voted;
    }
    __syncthreads();
    const int nl = n_list_s;
    int32_t* out_kfs = O.local_kfs + (size_t)f * O.kf_cap;
    if (voted_s) {
        for (int q = t; q < nl; q += kThreads) out_kfs[q] = list[q];
    } else {
        for (int q = t; q < nl; q += kThreads) list[q] = out_kfs[q];
    }
    __syncthreads();

    // ---- 3. offsets of the concatenated GetMapPointMatches() lists
    if (t == 0) {
        int s = 0;
        for (int q = 0; q < nl; q++) {
            moff[q] = s;
            const int j = list[q];
            if (j >= 0 && j < nk) s += max(M.match_off[kfb + j + 1] - M.match_off[kfb + j], 0);
        }
        moff[nl] = s;
    }
    __syncthreads();
    const int total = moff[nl];
    // entry e of the concatenation: its point row, or -1 for an empty slot or a bad point
    auto row_of = [&](int e) {
        int lo = 0, hi = nl - 1;  // the last q with moff[q] <= e
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (moff[mid] <= e) lo = mid; else hi = mid - 1;
        }
        const int row = M.match_row[M.match_off[kfb + list[lo]] + (e - moff[lo])];
        if (row < 0 || row >= n_rows) return -1;
        if (M.point_bad && M.point_bad[rb + row]) return -1;
        return row;
    };

    // ---- 4. first position per point
    int32_t* first = O.scratch + (size_t)f * O.scratch_stride;
    for (int e = t; e < total; e += kThreads) {
        const int row = row_of(e);
        if (row >= 0) first[row] = kNone;
    }
    __syncthreads();
    for (int e = t; e < total; e += kThreads) {
        const int row = row_of(e);
        if (row >= 0) atomicMin(&first[row], e);
    }
    __syncthreads();

    // ---- 5. ordered compaction
    int32_t* out_rows = O.local_rows + (size_t)f * O.capacity;
    int base = 0;
    for (int c0 = 0; c0 < total; c0 += kThreads) {
        const int e = c0 + t;
        const int row = e < total ? row_of(e) : -1;
        const bool keep = row >= 0 && load_l2(&first[row]) == e;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int pos = base + __popcll(m & ((1ull << lane) - 1));
        int sum = 0;
        for (int w = 0; w < kThreads / 64; w++) {
            if (w < wave) pos += wcnt[w];
            sum += wcnt[w];
        }
        if (keep && pos < O.capacity) out_rows[pos] = row;
        base += sum;
        __syncthreads();
    }
    const int n_local = min(base, O.capacity);
    if (t == 0) {
        if (voted_s) O.n_local_kfs[f] = nl;
        O.kf_max[f] = kf_max_s;
        O.n_local[f] = n_local;
        O.status[f] = base > O.capacity ? 1 : 0;
        if (O.records && O.local_frames) {
            O.local_frames[f].point_offset = (int32_t)((size_t)f * O.capacity);
            O.local_frames[f].n_points = n_local;
        }
    }
    if (!O.records) return;
    // out_rows was written by this workgroup before the loop's last barrier
    uint32_t* dst = (uint32_t*)(O.records + (size_t)f * O.capacity);
    const uint32_t* src = (const uint32_t*)(M.points + rb);
    for (int w = t; w < n_local * kRecordWords; w += kThreads) {
        const int r = w / kRecordWords;
        dst[w] = src[(size_t)load_l2(&out_rows[r]) * kRecordWords + (w - r * kRecordWords)];
    }
}

}  // namespace

hipError_t update_local_map_launch(int n_frames, const spslam_track_batch* mm, const spslam_local_map& map,
                                   const spslam_local_map_out& out, hipStream_t s, KernelTimer* timer) {
    if (timer) timer->begin(kKindTrack, s);
    hipLaunchKernelGGL(update_local_map_kernel, dim3(n_frames), dim3(kThreads), 0, s,
                       mm ? *mm : spslam_track_batch{}, mm != nullptr, map, out);
    if (timer) timer->end(kKindTrack, s);
    return hipGetLastError();
}

}  // namespace spslam
