// Bag of words on gfx950:
//   Frame::ComputeBoW (src/Frame.cc:495-502) = DBoW2 TemplatedVocabulary::transform
//     (features, BowVector, FeatureVector, levelsup = 4) (TemplatedVocabulary.h:1127-1194,
//     per feature :1217-1259; BowVector.cpp addWeight / addIfNotExist / normalize;
//     FeatureVector.cpp addFeature; FORB::distance);
//   ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:159-288).
// Semantics: oracle/bow_oracle.cpp.
//
//   bow_words_kernel    thread per feature: descend the vocabulary tree (first minimum
//                       of the 256-bit Hamming distance over each node's children, in
//                       the loaded order) -> word id, weight, node at level L - levelsup.
//                       The top of the tree is read by every feature and stays in L2.
//   bow_vectors_kernel  workgroup per frame: bitonic sort of (word, feature) keys in LDS,
//                       one thread per run sums its weights in feature order (the
//                       std::map += order), the L1 / L2 norm in word order by one thread
//                       (the reference's map walk; <= cap dependent fp64 adds), then the
//                       (node, feature) sort gives the FeatureVector as CSR.
//   bow_search_kernel   workgroup per (keyframe, frame) pair: shared FeatureVector nodes
//                       are independent (a frame feature sits in one node), so each wave
//                       takes whole nodes; inside a node the keyframe features run in
//                       order (a match takes the frame feature for the later ones) and the
//                       64 lanes split the node's frame features, reducing (best, first
//                       index, second best) exactly as the sequential `<` scan; rotation
//                       histogram + ComputeThreeMaxima at the end.
//   bow_search_kf_kernel  ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (src/ORBmatcher.cc:522-655),
//                       the same shape, described at the kernel.
//   triangulation_search_kernel  ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-823), described at
//                       the kernel.
// Integer / index work and fp64 sums in the reference's order: bit-exact.
#include <hip/hip_runtime.h>

#include "bow_launch.h"
#include "orb_match_device.h"
#include "triangulate_launch.h"

namespace spslam {
namespace bow {

using namespace orb_match;

constexpr int kThreads = 256;
constexpr int kThLow = 50;

__global__ __launch_bounds__(kThreads) void bow_words_kernel(VocabDev V, const uint8_t* __restrict__ desc,
                                                             const int* __restrict__ counts, int cap, int n_frames,
                                                             int nid_level, uint32_t* __restrict__ s_word,
                                                             double* __restrict__ s_weight,
                                                             uint32_t* __restrict__ s_node) {
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (g >= (long long)n_frames * cap) return;
    const int f = (int)(g / cap), i = (int)(g - (long long)f * cap);
    if (i >= min(counts[f], cap)) return;
    const uint4* p = reinterpret_cast<const uint4*>(desc + g * 32);
    const uint4 a0 = p[0], a1 = p[1];
    int node = 0, level = 0;
    uint32_t nid = 0;
    bool set = nid_level <= 0;
    int cc = V.child_count[0];
    do {
        ++level;
        const int cb = V.child_begin[node];
        int best = V.child_ids[cb];
        int bd = hamming(a0, a1, V.desc[2 * best], V.desc[2 * best + 1]);
        for (int c = 1; c < cc; c++) {
            const int id = V.child_ids[cb + c];
            const int d = hamming(a0, a1, V.desc[2 * id], V.desc[2 * id + 1]);
            if (d < bd) {
                bd = d;
                best = id;
            }
        }
        node = best;
        if (level == nid_level) {
            nid = (uint32_t)node;
            set = true;
        }
        cc = V.child_count[node];
    } while (cc > 0);
    if (!set) nid = (uint32_t)node;  // indeterminate in the reference (oracle header)
    s_word[g] = V.word_id[node];
    s_weight[g] = V.weight[node];
    s_node[g] = nid;
}

// ascending bitonic sort of P (power of two) 64-bit keys in LDS
__device__ void bitonic_sort(unsigned long long* key, int P) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < P; t += kThreads) {
                const int q = t ^ j;
                if (q > t) {
                    const unsigned long long x = key[t], y = key[q];
                    const bool up = (t & k) == 0;
                    if ((x > y) == up) {
                        key[t] = y;
                        key[q] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// exclusive prefix over threads of `v`; returns this thread's offset, *total the sum
__device__ int block_exclusive_scan(int v, int* tmp, int* total) {
    const int t = threadIdx.x;
    tmp[t] = v;
    __syncthreads();
    for (int o = 1; o < kThreads; o <<= 1) {
        const int add = t >= o ? tmp[t - o] : 0;
        __syncthreads();
        tmp[t] += add;
        __syncthreads();
    }
    const int incl = tmp[t];
    *total = tmp[kThreads - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kThreads) void bow_vectors_kernel(int cap, int P, int tf, int must, int l2,
                                                               const int* __restrict__ counts,
                                                               const uint32_t* __restrict__ s_word,
                                                               const double* __restrict__ s_weight,
                                                               const uint32_t* __restrict__ s_node, BowOut out) {
    extern __shared__ unsigned long long lds[];
    unsigned long long* key = lds;                          // [P]
    double* vals = reinterpret_cast<double*>(lds + P);      // [P]
    __shared__ int scan_tmp[kThreads];
    __shared__ double norm_s;
    const int f = blockIdx.x, t = threadIdx.x;
    const size_t fo = (size_t)f * cap;
    const int n = min(counts[f], cap);
    const int per = P / kThreads > 0 ? P / kThreads : 1;   // contiguous elements per thread
    const int lo = min(t * per, P), hi = min(lo + per, P);
    // keys at positions >= n are ~0 (the maximum), so sorting the first power of two >= n gives the full sort's
    // array: a frame with few features (none, when the caller masks it) does not pay for cap
    int Pn = n > 0 ? 1 : 0;
    while (Pn < n) Pn <<= 1;
    Pn = min(Pn, P);

    // ---- BowVector: (word, feature) keys of the features that are not stop words
    int valid = 0;
    for (int q = t; q < P; q += kThreads) {
        const bool ok = q < n && s_weight[fo + q] > 0.0;
        key[q] = ok ? ((unsigned long long)s_word[fo + q] << 32) | (unsigned)q : ~0ull;
        valid += ok;
    }
    int m;
    block_exclusive_scan(valid, scan_tmp, &m);
    bitonic_sort(key, Pn);
    int heads = 0;
    for (int q = lo; q < hi; q++)
        heads += q < m && (q == 0 || (key[q] >> 32) != (key[q - 1] >> 32));
    int nb;
    int u = block_exclusive_scan(heads, scan_tmp, &nb);
    for (int q = lo; q < hi; q++) {
        if (!(q < m && (q == 0 || (key[q] >> 32) != (key[q - 1] >> 32)))) continue;
        const unsigned w = (unsigned)(key[q] >> 32);
        double v = s_weight[fo + (unsigned)key[q]];
        if (tf)  // addWeight: += in feature order; addIfNotExist keeps the first
            for (int r = q + 1; r < m && (unsigned)(key[r] >> 32) == w; r++) v += s_weight[fo + (unsigned)key[r]];
        out.bow_words[fo + u] = w;
        vals[u++] = v;
    }
    __syncthreads();
    if (t == 0) {
        double norm = 0.0;
        if (must) {  // BowVector::normalize: the std::map walk in word order
            if (!l2) {
                for (int q = 0; q < nb; q++) norm += fabs(vals[q]);
            } else {
                for (int q = 0; q < nb; q++) norm += vals[q] * vals[q];
                norm = sqrt(norm);
            }
        }
        norm_s = norm;
        out.n_bow[f] = nb;
    }
    __syncthreads();
    const double norm = norm_s, nd = (double)nb;
    for (int q = t; q < nb; q += kThreads) {
        double v = vals[q];
        if (tf && !must) v /= nd;
        if (must && norm > 0.0) v /= norm;
        out.bow_values[fo + q] = v;
    }
    __syncthreads();

    // ---- FeatureVector: (node, feature) keys of the same features
    for (int q = t; q < P; q += kThreads) {
        const bool ok = q < n && s_weight[fo + q] > 0.0;
        key[q] = ok ? ((unsigned long long)s_node[fo + q] << 32) | (unsigned)q : ~0ull;
    }
    __syncthreads();
    bitonic_sort(key, Pn);
    heads = 0;
    for (int q = lo; q < hi; q++)
        heads += q < m && (q == 0 || (key[q] >> 32) != (key[q - 1] >> 32));
    int nf;
    u = block_exclusive_scan(heads, scan_tmp, &nf);
    int32_t* fv_start = out.fv_start + (size_t)f * (cap + 1);
    for (int q = lo; q < hi; q++) {
        if (q >= m) break;
        out.fv_features[fo + q] = (int32_t)(unsigned)key[q];
        if (q == 0 || (key[q] >> 32) != (key[q - 1] >> 32)) {
            out.fv_nodes[fo + u] = (uint32_t)(key[q] >> 32);
            fv_start[u++] = q;
        }
    }
    if (t == 0) {
        fv_start[nf] = m;
        out.n_fv[f] = nf;
    }
}

// (best distance, its first position, second best) of a strided scan, merged across lanes
struct Best {
    int b1, i1, b2;
};

__device__ __forceinline__ Best merge(const Best& a, const Best& b) {
    Best r;
    if (a.b1 < b.b1 || (a.b1 == b.b1 && a.i1 < b.i1)) {
        r.b1 = a.b1; r.i1 = a.i1; r.b2 = min(a.b2, b.b1);
    } else {
        r.b1 = b.b1; r.i1 = b.i1; r.b2 = min(b.b2, a.b1);
    }
    return r;
}

// position of node `id` in the ascending node list of a FeatureVector, -1 when absent: the shared-node
// intersection of SearchByBoW / SearchForTriangulation (the reference's lower_bound walk)
__device__ __forceinline__ int find_node(const uint32_t* __restrict__ nodes, int n, uint32_t id) {
    int l = 0, h = n;
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (nodes[mid] < id) l = mid + 1; else h = mid;
    }
    return l < n && nodes[l] == id ? l : -1;
}

// The rotation-consistency tail of SearchByBoW and SearchForTriangulation: ComputeThreeMaxima over the histogram,
// then every match among the first n whose bin is none of the three is cleared and counted in *n_removed.  The
// whole workgroup calls it after the barrier that completes hist and bin; it ends with a barrier.
__device__ __forceinline__ void keep_three_maxima(const int* hist, int* ind, const signed char* bin, int32_t* match,
                                                  int n, int* n_removed) {
    const int t = threadIdx.x;
    if (t == 0) three_maxima(hist, &ind[0], &ind[1], &ind[2]);
    __syncthreads();
    int removed = 0;
    for (int i = t; i < n; i += kThreads) {
        const int bn = bin[i];
        if (bn >= 0 && bn != ind[0] && bn != ind[1] && bn != ind[2]) {
            match[i] = -1;
            removed++;
        }
    }
    if (removed) atomicAdd(n_removed, removed);
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void bow_search_kernel(const int2* __restrict__ pairs, BowSide K, BowSide F,
                                                              float nn_ratio, int check_ori,
                                                              int32_t* __restrict__ match_out,
                                                              int* __restrict__ nmatches_out) {
    extern __shared__ int smem[];
    int32_t* match = smem;                                          // [F.cap]
    int2* shared_nodes = reinterpret_cast<int2*>(smem + F.cap);     // [K.cap]
    signed char* bin = reinterpret_cast<signed char*>(shared_nodes + K.cap);  // [F.cap]
    __shared__ int hist[kHisto];
    __shared__ int n_shared, n_total, n_removed;
    __shared__ int ind[3];
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int kf = pairs[p].x, fr = pairs[p].y;
    const int nF = min(F.counts[fr], F.cap);
    for (int i = t; i < F.cap; i += kThreads) {
        match[i] = -1;
        bin[i] = -1;
    }
    if (t < kHisto) hist[t] = 0;
    if (t == 0) { n_shared = 0; n_total = 0; n_removed = 0; }
    __syncthreads();
    // nodes present in both FeatureVectors (processing order is free: the frame features of different
    // nodes are disjoint, so no node's outcome depends on another's)
    const uint32_t* kn = K.fv_nodes + (size_t)kf * K.cap;
    const uint32_t* fn = F.fv_nodes + (size_t)fr * F.cap;
    const int nk = K.n_fv[kf], nfv = F.n_fv[fr];
    for (int a = t; a < nk; a += kThreads) {
        const int l = find_node(fn, nfv, kn[a]);
        if (l >= 0) shared_nodes[atomicAdd(&n_shared, 1)] = make_int2(a, l);
    }
    __syncthreads();
    const int32_t* ks = K.fv_start + (size_t)kf * (K.cap + 1);
    const int32_t* fs = F.fv_start + (size_t)fr * (F.cap + 1);
    const int32_t* kfeat = K.fv_features + (size_t)kf * K.cap;
    const int32_t* ffeat = F.fv_features + (size_t)fr * F.cap;
    const uint4* kdesc = reinterpret_cast<const uint4*>(K.desc + (size_t)kf * K.cap * 32);
    const uint4* fdesc = reinterpret_cast<const uint4*>(F.desc + (size_t)fr * F.cap * 32);
    const uint8_t* has = K.has_point + (size_t)kf * K.cap;
    const spslam_keypoint* kk = K.keys + (size_t)kf * K.cap;
    const spslam_keypoint* fk = F.keys + (size_t)fr * F.cap;
    int count = 0;
    for (int s = wave; s < n_shared; s += kThreads / 64) {
        const int2 nd = shared_nodes[s];
        const int f0 = fs[nd.y], f1 = fs[nd.y + 1];
        for (int q = ks[nd.x]; q < ks[nd.x + 1]; q++) {
            const int ikf = kfeat[q];
            if (!has[ikf]) continue;
            const uint4 a0 = kdesc[2 * ikf], a1 = kdesc[2 * ikf + 1];
            Best b{256, 1 << 30, 256};
            for (int r = f0 + lane; r < f1; r += 64) {
                const int jf = ffeat[r];
                if (bin[jf] != -1) continue;  // vpMapPointMatches[realIdxF] already set
                const int d = hamming(a0, a1, fdesc[2 * jf], fdesc[2 * jf + 1]);
                if (d < b.b1) { b.b2 = b.b1; b.b1 = d; b.i1 = r; }
                else if (d < b.b2) b.b2 = d;
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                Best x{__shfl_xor(b.b1, o), __shfl_xor(b.i1, o), __shfl_xor(b.b2, o)};
                b = merge(b, x);
            }
            if (b.b1 <= kThLow && (float)b.b1 < __fmul_rn(nn_ratio, (float)b.b2)) {
                const int jf = ffeat[b.i1];
                const int bn = check_ori ? rotation_bin(kk[ikf].angle, fk[jf].angle) : 0;
                if (lane == 0) {
                    match[jf] = ikf;
                    bin[jf] = (signed char)bn;
                    if (check_ori) atomicAdd(&hist[bn], 1);
                }
                count++;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (lane == 0 && count) atomicAdd(&n_total, count);
    __syncthreads();
    if (check_ori) keep_three_maxima(hist, ind, bin, match, nF, &n_removed);
    int32_t* mo = match_out + (size_t)p * F.cap;
    for (int i = t; i < nF; i += kThreads) mo[i] = match[i];
    if (t == 0) nmatches_out[p] = n_total - n_removed;
}

// ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (src/ORBmatcher.cc:522-655), bow_search_kernel's shape:
// workgroup per (keyframe 1, keyframe 2) pair, the shared nodes listed in LDS, a wave per node, the node's idx1 in
// list order (vbMatched2 makes them order dependent; a feature sits in one node, so nodes are independent) and the
// 64 lanes over the node's idx2.  What differs from the keyframe-to-frame overload: has_point is read on both sides,
// acceptance is bestDist1 < TH_LOW (:598), the result, the histogram and the bins are indexed by idx1, and vbMatched2
// is a table of its own that a match removed by the histogram leaves set.
__global__ __launch_bounds__(kThreads) void bow_search_kf_kernel(const int2* __restrict__ pairs, BowSide A, BowSide B,
                                                                 float nn_ratio, int check_ori,
                                                                 int32_t* __restrict__ match_out,
                                                                 int* __restrict__ nmatches_out) {
    extern __shared__ int smem[];
    int2* shared_nodes = reinterpret_cast<int2*>(smem);                       // [A.cap]
    int32_t* match = smem + 2 * A.cap;                                        // [A.cap] by idx1
    signed char* bin = reinterpret_cast<signed char*>(match + A.cap);         // [A.cap] by idx1
    uint8_t* matched2 = reinterpret_cast<uint8_t*>(bin + A.cap);              // [B.cap] vbMatched2
    __shared__ int hist[kHisto];
    __shared__ int n_shared, n_total, n_removed;
    __shared__ int ind[3];
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int k1 = pairs[p].x, k2 = pairs[p].y;
    const int n1 = min(A.counts[k1], A.cap), n2 = min(B.counts[k2], B.cap);
    for (int i = t; i < A.cap; i += kThreads) {
        match[i] = -1;
        bin[i] = -1;
    }
    for (int i = t; i < B.cap; i += kThreads) matched2[i] = 0;
    if (t < kHisto) hist[t] = 0;
    if (t == 0) { n_shared = 0; n_total = 0; n_removed = 0; }
    __syncthreads();
    const uint32_t* nodes1 = A.fv_nodes + (size_t)k1 * A.cap;
    const uint32_t* nodes2 = B.fv_nodes + (size_t)k2 * B.cap;
    const int nfv1 = min(A.n_fv[k1], A.cap), nfv2 = min(B.n_fv[k2], B.cap);
    for (int a = t; a < nfv1; a += kThreads) {
        const int l = find_node(nodes2, nfv2, nodes1[a]);
        if (l >= 0) shared_nodes[atomicAdd(&n_shared, 1)] = make_int2(a, l);
    }
    __syncthreads();
    const int32_t* fs1 = A.fv_start + (size_t)k1 * (A.cap + 1);
    const int32_t* fs2 = B.fv_start + (size_t)k2 * (B.cap + 1);
    const int32_t* feat1 = A.fv_features + (size_t)k1 * A.cap;
    const int32_t* feat2 = B.fv_features + (size_t)k2 * B.cap;
    const uint4* desc1 = reinterpret_cast<const uint4*>(A.desc + (size_t)k1 * A.cap * 32);
    const uint4* desc2 = reinterpret_cast<const uint4*>(B.desc + (size_t)k2 * B.cap * 32);
    const uint8_t* has1 = A.has_point + (size_t)k1 * A.cap;
    const uint8_t* has2 = B.has_point + (size_t)k2 * B.cap;
    const spslam_keypoint* kun1 = A.keys + (size_t)k1 * A.cap;
    const spslam_keypoint* kun2 = B.keys + (size_t)k2 * B.cap;
    int count = 0;
    for (int s = wave; s < n_shared; s += kThreads / 64) {
        const int2 nd = shared_nodes[s];
        const int f0 = max(fs2[nd.y], 0), f1 = min(fs2[nd.y + 1], B.cap);
        const int q1 = min(fs1[nd.x + 1], A.cap);
        for (int q = max(fs1[nd.x], 0); q < q1; q++) {
            const int idx1 = feat1[q];
            if ((unsigned)idx1 >= (unsigned)n1 || !has1[idx1]) continue;          // :558-562
            const uint4 a0 = desc1[2 * idx1], a1 = desc1[2 * idx1 + 1];
            Best b{256, 1 << 30, 256};
            for (int r = f0 + lane; r < f1; r += 64) {
                const int idx2 = feat2[r];
                if ((unsigned)idx2 >= (unsigned)n2 || matched2[idx2] || !has2[idx2]) continue;   // :576-580
                const int d = hamming(a0, a1, desc2[2 * idx2], desc2[2 * idx2 + 1]);
                if (d < b.b1) { b.b2 = b.b1; b.b1 = d; b.i1 = r; }
                else if (d < b.b2) b.b2 = d;
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                Best x{__shfl_xor(b.b1, o), __shfl_xor(b.i1, o), __shfl_xor(b.b2, o)};
                b = merge(b, x);
            }
            if (b.b1 < kThLow && (float)b.b1 < __fmul_rn(nn_ratio, (float)b.b2)) {  // :598, strict
                const int idx2 = feat2[b.i1];
                const int bn = check_ori ? rotation_bin(kun1[idx1].angle, kun2[idx2].angle) : 0;
                if (lane == 0) {
                    match[idx1] = idx2;
                    matched2[idx2] = 1;
                    if (check_ori && (unsigned)bn < (unsigned)kHisto) {  // the reference asserts it
                        bin[idx1] = (signed char)bn;
                        atomicAdd(&hist[bn], 1);
                    }
                }
                count++;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (lane == 0 && count) atomicAdd(&n_total, count);
    __syncthreads();
    if (check_ori) keep_three_maxima(hist, ind, bin, match, n1, &n_removed);
    int32_t* mo = match_out + (size_t)p * A.cap;
    for (int i = t; i < n1; i += kThreads) mo[i] = match[i];
    if (t == 0) nmatches_out[p] = n_total - n_removed;
}

// ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-823, CheckDistEpipolarLine :140-157), workgroup per
// (current keyframe, neighbour) pair.  vbMatched2 is never written in the reference, so every key-1 feature without
// a map point is an independent item: the items of the shared nodes are listed in LDS (any order), and a group of
// kTriGroup lanes scans the item's key-2 node list, each lane keeping (distance, list position) of its own
// candidates that pass the has-point, stereo, TH_LOW, epipole and epipolar-line tests.  The reference keeps the
// smallest distance and, on a tie, the later position (`dist > bestDist` lets an equal one through): the minimum
// of (distance << 16 | 0xFFFF - position).  Rotation histogram + ComputeThreeMaxima at the end.
__global__ __launch_bounds__(kThreads) void triangulation_search_kernel(
    const spslam_tri_pair* __restrict__ pairs, spslam_tri_side S, TriConsts C, int only_stereo, int check_ori,
    int check_baseline, int32_t* __restrict__ match_out, int* __restrict__ nmatches_out,
    uint8_t* __restrict__ pair_status) {
    extern __shared__ int smem[];
    int2* items = reinterpret_cast<int2*>(smem);                          // [cap] (idx1, key-2 node position)
    signed char* bin = reinterpret_cast<signed char*>(items + S.cap);     // [cap]
    __shared__ int hist[kHisto];
    __shared__ int n_items, n_total, n_removed;
    __shared__ int ind[3];
    const int p = blockIdx.x, t = threadIdx.x;
    const spslam_tri_pair* P = pairs + p;
    const int k1 = P->kf1, k2 = P->kf2, cap = S.cap;
    const int n1 = min(S.counts[k1], cap), n2 = min(S.counts[k2], cap);
    int32_t* mo = match_out + P->out_offset;
    int status = SPSLAM_TRI_PAIR_SEARCHED;
    if (P->flags & SPSLAM_TRI_PAIR_SKIP) {
        status = SPSLAM_TRI_PAIR_SKIPPED;
    } else if (check_baseline) {  // LocalMapping.cc:258-264: vBaseline = Ow2 - Ow1, baseline < pKF2->mb
        const float baseline = (float)tri::norm3(__fsub_rn(P->Ow2[0], P->Ow1[0]), __fsub_rn(P->Ow2[1], P->Ow1[1]),
                                                 __fsub_rn(P->Ow2[2], P->Ow1[2]));
        if (baseline < C.mb) status = SPSLAM_TRI_PAIR_SHORT_BASELINE;
    }
    for (int i = t; i < n1; i += kThreads) mo[i] = -1;
    for (int i = t; i < cap; i += kThreads) bin[i] = -1;
    if (t < kHisto) hist[t] = 0;
    if (t == 0) {
        n_items = 0; n_total = 0; n_removed = 0;
        if (pair_status) pair_status[p] = (uint8_t)status;
    }
    if (status != SPSLAM_TRI_PAIR_SEARCHED) {  // uniform over the workgroup
        if (t == 0) nmatches_out[p] = 0;
        return;
    }
    __syncthreads();
    const uint32_t* nodes1 = S.fv_nodes + (size_t)k1 * cap;
    const uint32_t* nodes2 = S.fv_nodes + (size_t)k2 * cap;
    const int32_t* fs1 = S.fv_start + (size_t)k1 * (cap + 1);
    const int32_t* fs2 = S.fv_start + (size_t)k2 * (cap + 1);
    const int32_t* feat1 = S.fv_features + (size_t)k1 * cap;
    const int32_t* feat2 = S.fv_features + (size_t)k2 * cap;
    const uint8_t* has1 = S.has_point + (size_t)k1 * cap;
    const uint8_t* has2 = S.has_point + (size_t)k2 * cap;
    const float* ur1 = S.uright + (size_t)k1 * cap;
    const float* ur2 = S.uright + (size_t)k2 * cap;
    const spslam_keypoint* kun1 = S.keys_un + (size_t)k1 * cap;
    const spslam_keypoint* kun2 = S.keys_un + (size_t)k2 * cap;
    const uint4* desc1 = reinterpret_cast<const uint4*>(S.desc + (size_t)k1 * cap * 32);
    const uint4* desc2 = reinterpret_cast<const uint4*>(S.desc + (size_t)k2 * cap * 32);
    const int nfv1 = min(S.n_fv[k1], cap), nfv2 = min(S.n_fv[k2], cap);
    for (int a = t; a < nfv1; a += kThreads) {
        const int l = find_node(nodes2, nfv2, nodes1[a]);
        if (l < 0) continue;
        for (int q = fs1[a]; q < fs1[a + 1]; q++) {
            const int idx1 = feat1[q];
            if ((unsigned)idx1 >= (unsigned)n1 || has1[idx1]) continue;            // :699
            if (only_stereo && !(ur1[idx1] >= 0.f)) continue;
            const int slot = atomicAdd(&n_items, 1);
            if (slot < cap) items[slot] = make_int2(idx1, l);
        }
    }
    __syncthreads();
    // the epipole in the second image (:664-670): C2 = R2w*Cw + t2w
    const float* T2 = P->Tcw2;
    const float c2x = tri::row3(T2[0], T2[1], T2[2], P->Ow1[0], P->Ow1[1], P->Ow1[2], T2[3]);
    const float c2y = tri::row3(T2[4], T2[5], T2[6], P->Ow1[0], P->Ow1[1], P->Ow1[2], T2[7]);
    const float c2z = tri::row3(T2[8], T2[9], T2[10], P->Ow1[0], P->Ow1[1], P->Ow1[2], T2[11]);
    const float invz = 1.0f / c2z;
    const float ex = __fmaf_rn(__fmul_rn(C.fx, c2x), invz, C.cx);
    const float ey = __fmaf_rn(__fmul_rn(C.fy, c2y), invz, C.cy);
    const float* F = P->F12;
    const int g = t & (kTriGroup - 1);
    const int total = min(n_items, cap);
    int count = 0;
    for (int it = t / kTriGroup; it < total; it += kThreads / kTriGroup) {
        const int2 item = items[it];
        const int idx1 = item.x;
        const float x1 = kun1[idx1].x, y1 = kun1[idx1].y;
        // CheckDistEpipolarLine's l = x1'F12 = [a b c]
        const float la = __fadd_rn(__fmaf_rn(x1, F[0], __fmul_rn(y1, F[3])), F[6]);
        const float lb = __fadd_rn(__fmaf_rn(x1, F[1], __fmul_rn(y1, F[4])), F[7]);
        const float lc = __fadd_rn(__fmaf_rn(x1, F[2], __fmul_rn(y1, F[5])), F[8]);
        const float den = __fmaf_rn(la, la, __fmul_rn(lb, lb));
        const bool stereo1 = ur1[idx1] >= 0.f;
        const uint4 a0 = desc1[2 * idx1], a1 = desc1[2 * idx1 + 1];
        const int f0 = fs2[item.y], f1 = fs2[item.y + 1];
        int key = 0x7fffffff;
        for (int r = f0 + g; r < f1; r += kTriGroup) {
            const int idx2 = feat2[r];
            if ((unsigned)idx2 >= (unsigned)n2 || has2[idx2]) continue;            // :722
            const bool stereo2 = ur2[idx2] >= 0.f;
            if (only_stereo && !stereo2) continue;
            const int d = hamming(a0, a1, desc2[2 * idx2], desc2[2 * idx2 + 1]);
            const int cand = (d << 16) | (0xFFFF - (r - f0));
            if (d > kThLow || cand > key) continue;                                 // :736
            const float x2 = kun2[idx2].x, y2 = kun2[idx2].y;
            const int oct = kun2[idx2].octave;
            if (!stereo1 && !stereo2) {                                             // :741
                const float dx = __fsub_rn(ex, x2), dy = __fsub_rn(ey, y2);
                if (__fmaf_rn(dx, dx, __fmul_rn(dy, dy)) < __fmul_rn(100.f, level_entry(C.scale, oct))) continue;
            }
            const float num = __fadd_rn(__fmaf_rn(la, x2, __fmul_rn(lb, y2)), lc);
            if (den == 0.f) continue;
            const float dsqr = __fmul_rn(num, num) / den;
            if (!((double)dsqr < 3.84 * (double)level_entry(C.sigma2, oct))) continue;
            key = cand;
        }
#pragma unroll
        for (int o = 1; o < kTriGroup; o <<= 1) key = min(key, __shfl_xor(key, o));
        if (g == 0 && key != 0x7fffffff) {
            const int idx2 = feat2[f0 + (0xFFFF - (key & 0xFFFF))];
            mo[idx1] = idx2;
            if (check_ori) {
                const int bn = rotation_bin(kun1[idx1].angle, kun2[idx2].angle);
                if ((unsigned)bn < (unsigned)kHisto) {  // the reference asserts it
                    bin[idx1] = (signed char)bn;
                    atomicAdd(&hist[bn], 1);
                }
            }
            count++;
        }
    }
    if (count) atomicAdd(&n_total, count);
    __syncthreads();
    if (check_ori) keep_three_maxima(hist, ind, bin, mo, n1, &n_removed);
    if (t == 0) nmatches_out[p] = n_total - n_removed;
}

}  // namespace bow

hipError_t triangulation_search_launch(int n_pairs, const spslam_tri_pair* pairs, const spslam_tri_side& side,
                                       const TriConsts& C, int only_stereo, int check_ori, int check_baseline,
                                       int32_t* match12, int* nmatches, uint8_t* pair_status, hipStream_t s) {
    if (n_pairs < 1 || side.cap < 1 || side.cap > 8192) return hipErrorInvalidValue;
    const size_t lds = ((size_t)side.cap * 9 + 15) / 16 * 16;  // <= 72 KB
    static const hipError_t lds_attr = hipFuncSetAttribute((const void*)bow::triangulation_search_kernel,
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 9);
    if (lds_attr != hipSuccess) return lds_attr;
    hipLaunchKernelGGL(bow::triangulation_search_kernel, dim3(n_pairs), dim3(bow::kThreads), lds, s, pairs, side, C,
                       only_stereo, check_ori, check_baseline, match12, nmatches, pair_status);
    return hipGetLastError();
}

hipError_t bow_transform_launch(const VocabDev& V, int n_frames, const uint8_t* desc, const int* counts, int cap,
                                int levelsup, uint32_t* s_word, double* s_weight, uint32_t* s_node,
                                const BowOut& out, hipStream_t s, KernelTimer* timer) {
    if (n_frames < 1 || cap < 1 || V.n_nodes < 2) return hipErrorInvalidValue;
    int P = 64;
    while (P < cap) P <<= 1;
    if (P > 8192) return hipErrorInvalidValue;  // 128 KB of LDS keys + values
    // dynamic LDS beyond the default 64 KB needs the per-kernel opt-in (set once)
    static const hipError_t lds_attr = hipFuncSetAttribute((const void*)bow::bow_vectors_kernel,
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 16);
    if (lds_attr != hipSuccess) return lds_attr;
    const int tf = V.weighting == 0 || V.weighting == 1;  // TF_IDF, TF
    const int must = V.scoring != 5;                       // all but DOT_PRODUCT normalise
    const int l2 = V.scoring == 1;
    const long long n = (long long)n_frames * cap;
    if (timer) timer->begin(kKindBowWords, s);
    hipLaunchKernelGGL(bow::bow_words_kernel, dim3((unsigned)((n + bow::kThreads - 1) / bow::kThreads)),
                       dim3(bow::kThreads), 0, s, V, desc, counts, cap, n_frames, V.L - levelsup, s_word, s_weight,
                       s_node);
    if (timer) timer->end(kKindBowWords, s);
    if (timer) timer->begin(kKindBowVectors, s);
    hipLaunchKernelGGL(bow::bow_vectors_kernel, dim3(n_frames), dim3(bow::kThreads), (size_t)P * 16, s, cap, P, tf,
                       must, l2, counts, s_word, s_weight, s_node, out);
    if (timer) timer->end(kKindBowVectors, s);
    return hipGetLastError();
}

hipError_t bow_search_launch(int n_pairs, const int2* pairs, const BowSide& kf, const BowSide& fr, float nn_ratio,
                             int check_ori, int32_t* match, int* nmatches, hipStream_t s, KernelTimer* timer) {
    if (n_pairs < 1 || kf.cap < 1 || fr.cap < 1) return hipErrorInvalidValue;
    const size_t lds = (size_t)fr.cap * 4 + (size_t)kf.cap * 8 + (size_t)fr.cap;
    if (lds > 150 * 1024) return hipErrorInvalidValue;
    static const hipError_t lds_attr = hipFuncSetAttribute((const void*)bow::bow_search_kernel,
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (lds_attr != hipSuccess) return lds_attr;
    if (timer) timer->begin(kKindBowMatch, s);
    hipLaunchKernelGGL(bow::bow_search_kernel, dim3(n_pairs), dim3(bow::kThreads), (lds + 15) / 16 * 16, s, pairs, kf,
                       fr, nn_ratio, check_ori, match, nmatches);
    if (timer) timer->end(kKindBowMatch, s);
    return hipGetLastError();
}

hipError_t bow_search_kf_launch(int n_pairs, const int2* pairs, const BowSide& kf1, const BowSide& kf2, float nn_ratio,
                                int check_ori, int32_t* match12, int* nmatches, hipStream_t s) {
    if (n_pairs < 1 || kf1.cap < 1 || kf2.cap < 1) return hipErrorInvalidValue;
    const size_t lds = (size_t)kf1.cap * 13 + (size_t)kf2.cap;  // match, shared nodes, bins; vbMatched2
    if (lds > 150 * 1024) return hipErrorInvalidValue;
    static const hipError_t lds_attr = hipFuncSetAttribute((const void*)bow::bow_search_kf_kernel,
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (lds_attr != hipSuccess) return lds_attr;
    hipLaunchKernelGGL(bow::bow_search_kf_kernel, dim3(n_pairs), dim3(bow::kThreads), (lds + 15) / 16 * 16, s, pairs,
                       kf1, kf2, nn_ratio, check_ori, match12, nmatches);
    return hipGetLastError();
}

}  // namespace spslam
