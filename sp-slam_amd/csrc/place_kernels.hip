// gfx950 kernels for place recognition on the device-resident BowVectors (include/spslam_gpu.h):
//   place_candidates_kernel<false>  KeyFrameDatabase::DetectRelocalizationCandidates  src/KeyFrameDatabase.cc:199-309
//   place_candidates_kernel<true>   KeyFrameDatabase::DetectLoopCandidates            src/KeyFrameDatabase.cc:76-197
//   place_min_score_kernel          LoopClosing::DetectLoop's reference score         src/LoopClosing.cc:126-140
// with L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).
//
// One 1024-thread workgroup (sixteen wave64) per problem; a sequence has at most 1024 keyframes, so thread j is
// keyframe j in every per-keyframe step.  A dense walk, keyframe-major; the inverted file is not mirrored:
//   1. the query vector into LDS (words and values, 12 bytes a word, at most 96 KiB);
//   2. a wave per keyframe: its words 64 at a time, coalesced, each lane a binary search in the LDS words.  Both
//      lists ascend, so the hits of a chunk ascend with the lane: the first hit of the first chunk that has one is
//      the query position of the first shared word, the popcount of the ballot counts the common words, and the
//      score's double sum takes the hits' terms lane by lane in ballot order -- the serial sum of the reference,
//      term for term, the same in every lane.  It is formed for every sharing keyframe, scored or not: one pass
//      over the vectors instead of two;
//   3. thread j: the counts' maximum and the list length by LDS atomics; the scores of this query written; the
//      walk of the ten covis neighbours from LDS copies of the scores (nothing the launch writes is read back
//      from memory); the maximum acc by a butterfly and one LDS slot per wave;
//   4. the ordered output without a scan over entries: the list order is the key (first shared position << 10 |
//      index), unique per keyframe.  A kept entry takes an LDS atomicMin of its key on its best keyframe; the
//      entry that holds the minimum is that keyframe's first occurrence.  Those are appended to an LDS list in any
//      order, and each one's output place is the number of smaller keys in that list.
// LDS: the query + 20 KiB of per-keyframe words.  Index work and dependent adds: latency bound.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "place_launch.h"
#include "wave_ops.h"

namespace spslam {

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxKf = SPSLAM_COVIS_MAX_KF;
constexpr int kBest = SPSLAM_COVIS_BEST;
constexpr int kMaxWords = SPSLAM_PLACE_MAX_WORDS;
constexpr int kIdxBits = 10;
static_assert(kMaxKf == 1 << kIdxBits && kMaxKf == kThreads, "thread j is keyframe j; the keys hold j in 10 bits");
static_assert(kMaxWords <= 1 << (31 - kIdxBits), "the keys hold a query position above the index");

struct Query {  // in LDS
    const uint32_t* w;
    const double* v;
    int n;
};

// the dynamic LDS: values, then words
__device__ __forceinline__ Query load_query(double* dyn, int P, const uint32_t* words, const double* values, int n,
                                            int t) {
    double* qv = dyn;
    uint32_t* qw = (uint32_t*)(dyn + P);
    for (int i = t; i < n; i += kThreads) {
        qw[i] = words[i];
        qv[i] = values[i];
    }
    return Query{qw, qv, n};
}

// One wave: the words of one vector against the query.  cnt: the common words; first: the query position of the
// first one; sum: the score's sum before the final -sum / 2.0.  The same in every lane.
__device__ __forceinline__ void wave_intersect(const Query& q, const uint32_t* words, const double* values, int n,
                                               int lane, int& cnt, int& first, double& sum) {
    cnt = 0;
    first = 0;
    sum = 0.0;
    if (q.n == 0) return;
    const uint32_t q_first = q.w[0], q_last = q.w[q.n - 1];
    for (int i0 = 0; i0 < n; i0 += 64) {
        if (words[i0] > q_last) break;                                    // ascending: nothing further is shared
        const int i = i0 + lane;
        bool hit = false;
        int pos = 0;
        double term = 0.0;
        if (i < n) {
            const uint32_t w = words[i];
            if (w >= q_first && w <= q_last) {
                int lo = 0, hi = q.n;                                     // lower_bound
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (q.w[mid] < w) lo = mid + 1; else hi = mid;
                }
                if (lo < q.n && q.w[lo] == w) {
                    const double vi = q.v[lo], wi = values[i];
                    hit = true;
                    pos = lo;
                    term = fabs(vi - wi) - fabs(vi) - fabs(wi);           // ScoringObject.cpp:41
                }
            }
        }
        unsigned long long m = __ballot(hit);
        if (!m) continue;
        if (cnt == 0) first = __shfl(pos, __ffsll(m) - 1);
        cnt += __popcll(m);
        while (m) {                                                       // score += ..., in word order
            sum += __shfl(term, __ffsll(m) - 1);
            m &= m - 1;
        }
    }
}

__device__ __forceinline__ float to_score(double sum) { return (float)(-sum / 2.0); }  // :65, then the float

template <bool kLoop>
__global__ __launch_bounds__(kThreads) void place_candidates_kernel(const spslam_place_problem* problems,
                                                                    spslam_place_db D, spslam_place_frames F,
                                                                    const int32_t* covis, const int32_t* weights,
                                                                    int stride, const float* min_score, int P,
                                                                    spslam_place_result* results,
                                                                    int32_t* candidates) {
    extern __shared__ double dyn[];
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    __shared__ int cnt[kMaxKf];      // common words; from step 3 on: 1 = the keyframe contributes as a neighbour
    __shared__ int key[kMaxKf];      // the list order: first shared position << 10 | index
    __shared__ float sc[kMaxKf];     // the score a neighbour contributes
    __shared__ int min_key[kMaxKf];  // per best keyframe: the first kept entry that names it
    __shared__ int out_key[kMaxKf];  // the emitted entries' keys, in any order
    __shared__ float wave_best[kWaves];
    __shared__ int n_sharing_s, max_s, n_scored_s, n_kept_s, n_out_s;
    const spslam_place_problem pr = problems[p];
    const int nk = min(max(pr.n_kf, 0), kMaxKf);
    const size_t kfb = (size_t)pr.kf_base, cap = (size_t)D.cap;

    // ---- 1. the query vector
    const size_t qslot = kLoop ? kfb + pr.query : (size_t)pr.query;
    const int q_cap = kLoop ? D.cap : F.cap;
    const int q_n = min(max((kLoop ? D.n_bow : F.n_bow)[qslot], 0), min(q_cap, P));
    const Query q = load_query(dyn, P, (kLoop ? D.bow_words : F.bow_words) + qslot * q_cap,
                               (kLoop ? D.bow_values : F.bow_values) + qslot * q_cap, q_n, t);
    min_key[t] = INT_MAX;
    if (t == 0) { n_sharing_s = 0; max_s = 0; n_scored_s = 0; n_kept_s = 0; n_out_s = 0; }
    __syncthreads();

    // ---- 2. common words, first shared position and score sum of every keyframe in the inverted file
    for (int j = wave; j < nk; j += kWaves) {
        bool listed = D.in_db[kfb + j] != 0;
        if (kLoop && listed) listed = weights[(kfb + pr.query) * (size_t)stride + j] == 0;  // spConnectedKeyFrames
        int c = 0, first = 0;
        double sum = 0.0;
        if (listed)
            wave_intersect(q, D.bow_words + (kfb + j) * cap, D.bow_values + (kfb + j) * cap,
                           min(max(D.n_bow[kfb + j], 0), D.cap), lane, c, first, sum);
        if (lane == 0) {
            cnt[j] = c;
            key[j] = (first << kIdxBits) | j;
            sc[j] = to_score(sum);
        }
    }
    __syncthreads();

    // ---- 3. thread j is keyframe j
    const int c = t < nk ? cnt[t] : 0;
    const bool sharing = c > 0;                                           // in lKFsSharingWords
    {
        const int n = __popcll(__ballot(sharing));
        if (lane == 0 && n) atomicAdd(&n_sharing_s, n);
        if (sharing) atomicMax(&max_s, c);
    }
    __syncthreads();
    const int n_sharing = n_sharing_s;
    if (n_sharing == 0) {                                                 // if(lKFsSharingWords.empty()) return
        if (t == 0) results[p] = spslam_place_result{SPSLAM_PLACE_EMPTY, 0, 0, 0, 0, 0, 0, 0.f};
        return;
    }
    const int max_common = max_s;
    const int min_common = (int)((float)max_common * 0.8f);               // int minCommonWords = maxCommonWords*0.8f
    const bool scored = sharing && c > min_common;
    const float si = sc[t];
    const float ms = kLoop ? min_score[p] : 0.f;
    const bool entry = scored && (!kLoop || si >= ms);                    // in lScoreAndMatch
    float* table = (kLoop ? D.loop_score : D.reloc_score) + kfb;
    if (scored) table[t] = si;
    // what a neighbour adds: loop, only if scored now (:159); relocalization, any sharing keyframe, an unscored
    // one with the score an earlier query left (:273-276)
    if (!kLoop && sharing && !scored) sc[t] = table[t];
    if (t < nk) cnt[t] = kLoop ? scored : sharing;
    {
        const int n_sc = __popcll(__ballot(scored)), n_en = __popcll(__ballot(entry));
        if (lane == 0 && n_sc) atomicAdd(&n_scored_s, n_sc);
        if (lane == 0 && n_en) atomicAdd(&n_kept_s, n_en);
    }
    __syncthreads();
    const int n_scored = n_scored_s, n_kept = n_kept_s;
    if (n_kept == 0) {                                                    // if(lScoreAndMatch.empty()) return
        if (t == 0)
            results[p] = spslam_place_result{SPSLAM_PLACE_NONE_KEPT, n_sharing, max_common, min_common, n_scored, 0,
                                             0, ms};
        return;
    }
    float acc = -INFINITY;
    int best = t;
    if (entry) {
        float best_score = si;
        acc = si;
        const int32_t* row = covis + (kfb + t) * kBest;                   // GetBestCovisibilityKeyFrames(10)
        for (int r = 0; r < kBest; r++) {
            const int n = row[r];
            if (n < 0 || n >= nk || !cnt[n]) continue;
            const float s2 = sc[n];
            acc += s2;
            if (s2 > best_score) { best = n; best_score = s2; }
        }
    }
    // bestAccScore: the maximum, from 0 / minScore
    float wmax = acc;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float other = __shfl_xor(wmax, o);
        if (other > wmax) wmax = other;
    }
    if (lane == 0) wave_best[wave] = wmax;
    __syncthreads();
    float best_acc = ms;
    for (int w = 0; w < kWaves; w++)
        if (wave_best[w] > best_acc) best_acc = wave_best[w];

    // ---- 4. retention and the ordered, de-duplicated output
    const bool keep = entry && acc > 0.75f * best_acc;
    const int my_key = t < nk ? key[t] : 0;
    if (keep) atomicMin(&min_key[best], my_key);
    __syncthreads();
    const bool emit = keep && min_key[best] == my_key;                    // !spAlreadyAddedKF.count(pKFi)
    if (emit) out_key[atomicAdd(&n_out_s, 1)] = my_key;
    __syncthreads();
    const int n_out = n_out_s;
    if (emit) {
        int rank = 0;
        for (int a = 0; a < n_out; a++) rank += out_key[a] < my_key;
        candidates[(size_t)pr.out_offset + rank] = best;
    }
    if (t == 0)
        results[p] = spslam_place_result{SPSLAM_PLACE_OK, n_sharing, max_common, min_common, n_scored, n_kept, n_out,
                                         best_acc};
}

__global__ __launch_bounds__(kThreads) void place_min_score_kernel(const spslam_place_problem* problems,
                                                                   spslam_place_db D, const int32_t* ordered,
                                                                   const int32_t* n_ordered, int stride,
                                                                   const uint8_t* kf_bad, int P, float* out) {
    extern __shared__ double dyn[];
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    __shared__ float sc[kMaxKf];
    __shared__ int valid[kMaxKf];
    const spslam_place_problem pr = problems[p];
    const int nk = min(max(pr.n_kf, 0), kMaxKf);
    const size_t kfb = (size_t)pr.kf_base, cap = (size_t)D.cap, qslot = kfb + pr.query;
    const int q_n = min(max(D.n_bow[qslot], 0), min(D.cap, P));
    const Query q = load_query(dyn, P, D.bow_words + qslot * cap, D.bow_values + qslot * cap, q_n, t);
    const int n = min(min(max(n_ordered[qslot], 0), kMaxKf), stride);     // GetVectorCovisibleKeyFrames
    const int32_t* list = ordered + qslot * (size_t)stride;
    __syncthreads();
    for (int e = wave; e < n; e += kWaves) {
        const int j = list[e];
        const bool ok = j >= 0 && j < nk && !(kf_bad && kf_bad[kfb + j]);  // if(pKF->isBad()) continue;
        int c = 0, first = 0;
        double sum = 0.0;
        if (ok)
            wave_intersect(q, D.bow_words + (kfb + j) * cap, D.bow_values + (kfb + j) * cap,
                           min(max(D.n_bow[kfb + j], 0), D.cap), lane, c, first, sum);
        if (lane == 0) {
            sc[e] = to_score(sum);
            valid[e] = ok;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    // if(score<minScore) minScore = score, in list order: the smallest, the earliest of equal ones
    float v = 0.f;
    int at = INT_MAX;
    for (int e = lane; e < n; e += 64)
        if (valid[e] && (at == INT_MAX || sc[e] < v)) { v = sc[e]; at = e; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oat = __shfl_xor(at, o);
        if (oat != INT_MAX && (at == INT_MAX || ov < v || (ov == v && oat < at))) { v = ov; at = oat; }
    }
    if (lane == 0) out[p] = at != INT_MAX && v < 1.f ? v : 1.f;           // float minScore = 1;
}

constexpr size_t kMaxLds = (size_t)kMaxWords * 12;

inline bool db_ok(const spslam_place_db& db) { return db.cap >= 1 && db.cap <= kMaxWords; }

}  // namespace

hipError_t place_reloc_launch(int n_problems, const spslam_place_problem* problems, const spslam_place_db& db,
                              const spslam_place_frames& frames, const spslam_covis_graph& graph,
                              spslam_place_result* results, int32_t* candidates, hipStream_t s) {
    if (n_problems < 1 || !db_ok(db) || frames.cap < 1 || frames.cap > kMaxWords) return hipErrorInvalidValue;
    // dynamic LDS beyond the default 64 KiB needs the per-kernel opt-in (set once)
    static const hipError_t lds_attr = hipFuncSetAttribute((const void*)place_candidates_kernel<false>,
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    if (lds_attr != hipSuccess) return lds_attr;
    const int P = frames.cap;
    hipLaunchKernelGGL(place_candidates_kernel<false>, dim3(n_problems), dim3(kThreads), (size_t)P * 12, s, problems,
                       db, frames, graph.covis, (const int32_t*)nullptr, 0, (const float*)nullptr, P, results,
                       candidates);
    return hipGetLastError();
}

hipError_t place_loop_launch(int n_problems, const spslam_place_problem* problems, const spslam_place_db& db,
                             const spslam_covis_graph& graph, const float* min_score, spslam_place_result* results,
                             int32_t* candidates, hipStream_t s) {
    if (n_problems < 1 || !db_ok(db)) return hipErrorInvalidValue;
    static const hipError_t lds_attr = hipFuncSetAttribute((const void*)place_candidates_kernel<true>,
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    if (lds_attr != hipSuccess) return lds_attr;
    const int P = db.cap;
    hipLaunchKernelGGL(place_candidates_kernel<true>, dim3(n_problems), dim3(kThreads), (size_t)P * 12, s, problems,
                       db, spslam_place_frames{}, graph.covis, graph.weights, graph.stride, min_score, P, results,
                       candidates);
    return hipGetLastError();
}

hipError_t place_min_score_launch(int n_problems, const spslam_place_problem* problems, const spslam_place_db& db,
                                  const spslam_covis_graph& graph, const uint8_t* kf_bad, float* min_score,
                                  hipStream_t s) {
    if (n_problems < 1 || !db_ok(db)) return hipErrorInvalidValue;
    static const hipError_t lds_attr = hipFuncSetAttribute((const void*)place_min_score_kernel,
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
    if (lds_attr != hipSuccess) return lds_attr;
    const int P = db.cap;
    hipLaunchKernelGGL(place_min_score_kernel, dim3(n_problems), dim3(kThreads), (size_t)P * 12, s, problems, db,
                       graph.ordered, graph.n_ordered, graph.stride, kf_bad, P, min_score);
    return hipGetLastError();
}

}  // namespace spslam
