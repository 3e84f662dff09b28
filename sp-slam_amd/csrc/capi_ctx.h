// Private to the capi_*.cpp files: the context behind include/spslam_gpu.h, its device-buffer type, the error
// helpers, the host-array staging of the drop-in entries, and the pieces the ORBmatcher entries share: the per-level
// tables, the current frame of the window searches and the argument predicates of the batch forms.
//
// Nothing here falls back to a CPU path: if the HIP runtime or the gfx950 code object is unusable every entry
// point returns SPSLAM_ERR_HIP.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/spslam_gpu.h"
#include "orb_launch.h"
#include "plane_launch.h"
#include "pose_launch.h"
#include "supposed_launch.h"
#include "frame_launch.h"
#include "lba_launch.h"
#include "assoc_launch.h"
#include "bow_launch.h"
#include "match_launch.h"
#include "map_point_launch.h"
#include "track_launch.h"
#include "grab_launch.h"
#include "triangulate_launch.h"
#include "covis_launch.h"

using namespace spslam;

// HIP-event timer per kernel kind; events recorded on the launch stream.
struct EventTimer : KernelTimer {
    struct Pair { int kind; hipEvent_t e0, e1; };
    std::vector<Pair> pending;
    std::vector<hipEvent_t> pool;
    double total_ms[kNumKernelKinds] = {};
    long long count[kNumKernelKinds] = {};
    hipEvent_t cur[kNumKernelKinds] = {};
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    void begin(int kind, hipStream_t s) override { cur[kind] = get(); (void)hipEventRecord(cur[kind], s); }
    void end(int kind, hipStream_t s) override {
        hipEvent_t e1 = get();
        (void)hipEventRecord(e1, s);
        pending.push_back(Pair{kind, cur[kind], e1});
    }
    void collect() {
        for (auto& p : pending) {
            float ms = 0.f;
            if (hipEventSynchronize(p.e1) == hipSuccess && hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
                total_ms[p.kind] += ms;
                count[p.kind] += 1;
            }
            pool.push_back(p.e0);
            pool.push_back(p.e1);
        }
        pending.clear();
    }
    void reset() { collect(); for (int k = 0; k < kNumKernelKinds; k++) { total_ms[k] = 0; count[k] = 0; } }
    ~EventTimer() override {
        for (auto& p : pending) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};

// Owning device buffer: pointer and capacity in bytes.  Reads as its T* wherever a pointer is expected.
template <class T = uint8_t>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;  // bytes
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    operator T*() const { return p; }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // configure time: drop the old block whatever its size, then allocate exactly `bytes`
    hipError_t alloc(size_t bytes) {
        release();
        const hipError_t e = hipMalloc((void**)&p, bytes);
        if (e == hipSuccess) cap = bytes; else p = nullptr;
        return e;
    }
    // grow on demand: nothing when the capacity suffices, else wait for `s` (the work that may still read the
    // old block) and reallocate
    hipError_t reserve(size_t bytes, hipStream_t s) {
        if (bytes <= cap) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(s);
        return e != hipSuccess ? e : alloc(bytes);
    }
};

// Streams, events and the host-mapped stop flag.  A base of the context so that they are destroyed after its
// members: the device buffers are freed while the streams still exist.
struct CtxStreams {
    hipStream_t stream = nullptr;
    hipStream_t orb_aux = nullptr;  // orb_launch's second stream (the small pyramid levels' chain)
    hipEvent_t orb_fork = nullptr, orb_join = nullptr;
    hipEvent_t lba_done = nullptr;    // recorded after each LBA launch: the next call's stream waits on it before it
                                      //   rewrites the offsets, the ctl block or the scratch (one LBA call in flight
                                      //   per context, whatever the streams)
    int32_t* h_lba_stop = nullptr;    // host-mapped coherent pbStopFlag mirror of spslam_lba_optimize
    int32_t* d_lba_stop = nullptr;    // its device alias (hipHostGetDevicePointer)
    CtxStreams() = default;
    CtxStreams(const CtxStreams&) = delete;
    CtxStreams& operator=(const CtxStreams&) = delete;
    ~CtxStreams() {
        if (lba_done) (void)hipEventDestroy(lba_done);
        if (h_lba_stop) (void)hipHostFree(h_lba_stop);
        if (orb_fork) (void)hipEventDestroy(orb_fork);
        if (orb_join) (void)hipEventDestroy(orb_join);
        if (orb_aux) (void)hipStreamDestroy(orb_aux);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct spslam_ctx : CtxStreams {
    int device = 0;
    int num_cus = 256;  // compute units of the device (spslam_create)
    spslam_orb_params p{};
    std::string err;
    // ORBextractor tables
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    std::vector<int> nfeat;
    int umax[16]{};
    OrbGeom geom{};
    long long pyr_frame_stride = 0, blur_frame_stride = 0;
    int max_kp = 0;
    // device buffers
    DevBuf<> d_pyr, d_blur, d_score;
    OrbBuffers b{};  // views of the six buffers below
    DevBuf<uint32_t> d_cand, d_keys;
    DevBuf<uint16_t> d_cand_cnt, d_keynode;
    DevBuf<LevelKp> d_lvl_kp;
    DevBuf<int> d_lvl_cnt;
    DevBuf<> d_in;
    DevBuf<spslam_keypoint> d_kps;
    DevBuf<> d_desc;
    DevBuf<int> d_cnt;
    // last call (debug stage access)
    const uint8_t* last_gray = nullptr;
    size_t last_frame_stride = 0;
    int last_stride = 0, last_frames = 0;
    EventTimer* timer = nullptr;
    // drop-in PoseOptimization staging
    DevBuf<> d_pose_scratch;
    // plane stage
    bool planes_ready = false;
    PlaneGeom pg{};
    PlaneBuffers pb{};
    float* plane_cloud[2] = {nullptr, nullptr};  // organized-cloud sets (spslam_planes_select_cloud_set)
    int cloud_set = 0;
    // the depth output whose cloud a fused grab wrote into each set (spslam_grab_fuse_cloud); null = none
    struct CloudTag { const float* depth = nullptr; int n = 0; } cloud_tag[2];
    bool grab_cloud = [] { const char* e = getenv("SPSLAM_GRAB_CLOUD"); return e && e[0] == '1'; }();
    DevBuf<> d_plane_scratch;
    DevBuf<float> d_depth_in;
    DevBuf<spslam_plane> d_planes1;
    DevBuf<int> d_plane_cnt1;
    DevBuf<int32_t> d_inl1, d_con1;
    int plane_last_frames = 0;
    // supposed-plane stage (GeneratePlanesFromBoundries)
    SuppParams sp{};
    SuppBuffers sb{};
    DevBuf<> d_supp_scratch;
    DevBuf<spslam_supposed_plane> d_supp1;
    DevBuf<int> d_supp_cnt1;
    DevBuf<int32_t> d_line1;
    DevBuf<float> d_patch1;
    int supp_last_frames = 0;
    // RGB-D frame stage (UndistortKeyPoints / ComputeStereoFromRGBD / AssignFeaturesToGrid)
    bool frame_ready = false;
    FrameGeom fg{};
    DevBuf<> d_frame1;  // single-frame staging: kps, keys_un, depth, uR, grid_idx, grid_off, count
    // LocalBundleAdjustment (all grown on demand)
    DevBuf<> d_lba_scratch;
    DevBuf<long long> d_lba_off;
    int lba_stop_after = -1;          // spslam_lba_debug_stop_after
    int lba_order = SPSLAM_LBA_G2O_ORDER;  // spslam_lba_set_order
    int lba_team = 0;                 // spslam_lba_set_team (0: as many workgroups per problem as fill the chip)
    DevBuf<int> d_lba_ctl;            // the g2o-order launch's tickets and team barrier counters
    int pose_spin_cap = 0;            // spslam_debug_pose_spin_cap (0 = the kernel's default)
    unsigned solve_fail_mask = 0;     // spslam_debug_force_solve_failures
    DevBuf<> d_lba_stage;             // drop-in staging
    DevBuf<int2> d_lba_work;          // (problem, first index) work tables + the active counter
    // plane association: per (frame, frame plane, map plane) boundary distances
    DevBuf<float> d_assoc_dist;
    // projection matching: per (frame, last-frame point) windows + accepted-match lists
    DevBuf<> d_match_scratch;
    // bag of words: the vocabulary (one HBM blob), per-feature transform scratch, drop-in staging
    DevBuf<> d_vocab;
    VocabDev vocab{};
    DevBuf<> d_bow_scratch;
    DevBuf<> d_bow_stage;
    // loop closing: SearchByProjection(pKF, Scw)'s windows, SearchBySim3's vnMatch1 / vnMatch2 and flags
    DevBuf<> d_loop_scratch;

    // Call with the context's device current.  The last LBA launch may still read its buffers on a caller stream.
    ~spslam_ctx() {
        if (lba_done) (void)hipEventSynchronize(lba_done);
        delete timer;
    }
};

inline int fail(spslam_ctx* c, int code, const char* fmt, const char* what = "") {
    if (c) {
        char buf[512];
        std::snprintf(buf, sizeof buf, fmt, what);
        c->err = buf;
    }
    return code;
}
#define HIP_CHECK(ctx, expr)                                                                  \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(ctx, SPSLAM_ERR_HIP, #expr ": %s", hipGetErrorString(e_)); \
    } while (0)

// One slot of a drop-in entry's device block: `upload` bytes of the host array `src` go into `bytes` (>= upload)
// bytes.  {src, n} uploads the whole slot; a bare size is an output-only slot.
struct StageSlot {
    const void* src;
    size_t upload, bytes;
    StageSlot(const void* s, size_t up, size_t b) : src(s), upload(up), bytes(b) {}
    StageSlot(const void* s, size_t b) : StageSlot(s, b, b) {}
    StageSlot(size_t b) : StageSlot(nullptr, 0, b) {}
};

// Slot offsets at 256-byte alignment; returns the block size.  No HIP call, so it can be checked on the CPU.
inline size_t stage_layout(const StageSlot* slots, int n, size_t* off) {
    size_t bytes = 0;
    for (int i = 0; i < n; i++) { off[i] = bytes; bytes += (slots[i].bytes + 255) / 256 * 256; }
    return bytes;
}

// The device block of a drop-in entry: laid out by stage_layout, uploaded on the context's stream.  The block is
// either a stream-ordered temporary, returned on close() or when the Stage goes out of scope, or one of the
// context's persistent buffers, which a need above its capacity grows to `grow` times that need.  open() and
// close() return SPSLAM codes and leave the failing HIP call in the context's error string.
struct Stage {
    static constexpr int kMaxSlots = 20;
    spslam_ctx* c;
    uint8_t* q = nullptr;
    bool temporary = false;
    size_t off[kMaxSlots] = {};
    explicit Stage(spslam_ctx* ctx) : c(ctx) {}
    Stage(const Stage&) = delete;
    Stage& operator=(const Stage&) = delete;
    ~Stage() { if (temporary && q) (void)hipFreeAsync(q, c->stream); }
    int open(std::initializer_list<StageSlot> slots, DevBuf<>* persistent = nullptr, size_t grow = 1) {
        return open(slots.begin(), (int)slots.size(), persistent, grow);
    }
    int open(const StageSlot* slots, int n, DevBuf<>* persistent = nullptr, size_t grow = 1) {
        if (n > kMaxSlots) return fail(c, SPSLAM_ERR_ARG, "too many staging slots%s", "");
        const size_t bytes = stage_layout(slots, n, off);
        if (!persistent) {
            HIP_CHECK(c, hipMallocAsync((void**)&q, bytes, c->stream));
            temporary = true;
        } else {
            if (bytes > persistent->cap) HIP_CHECK(c, persistent->reserve(bytes * grow, c->stream));
            q = *persistent;
        }
        for (int i = 0; i < n; i++) {
            const StageSlot& s = slots[i];
            if (s.upload) HIP_CHECK(c, hipMemcpyAsync(q + off[i], s.src, s.upload, hipMemcpyHostToDevice, c->stream));
        }
        return SPSLAM_OK;
    }
    template <class T>
    T* slot(int i) const { return (T*)(q + off[i]); }
    int close() {
        uint8_t* t = temporary ? q : nullptr;
        q = nullptr;
        if (t) HIP_CHECK(c, hipFreeAsync(t, c->stream));
        return SPSLAM_OK;
    }
};

// An 8-entry per-level table of a kernel's constants from one of the context's ORBextractor vectors, zero past
// nlevels.
inline void level_table(const spslam_ctx* c, const std::vector<float>& v, float (&out)[8]) {
    for (int l = 0; l < 8; l++) out[l] = l < c->p.nlevels ? v[l] : 0.f;
}

// camera, image bounds, grid and level scales of the configured frame stage
inline MatchGeom match_geom(const spslam_ctx* c) {
    MatchGeom g{};
    g.fx = c->fg.fx; g.fy = c->fg.fy; g.cx = c->fg.cx; g.cy = c->fg.cy; g.bf = c->fg.bf;
    g.min_x = c->fg.min_x; g.max_x = c->fg.max_x; g.min_y = c->fg.min_y; g.max_y = c->fg.max_y;
    g.ginv_x = c->fg.ginv_x; g.ginv_y = c->fg.ginv_y;
    level_table(c, c->scale, g.scale);
    return g;
}

// The current frame's arrays of a window search's batch-device form (projection, local points, Fuse).
inline bool match_current_ok(const MatchCurrent& m) {
    return m.kun && m.desc && m.uright && m.grid_off && m.grid_idx && m.counts && m.cap >= 1 && m.cap <= (1 << 20);
}

// The spslam_track_batch fields every tracking entry reads; each entry adds what only it needs.
inline bool track_batch_ok(const spslam_track_batch& b) {
    return b.kp_counts && b.cap >= 1 && b.cap <= (1 << 20) && b.proj_frames && b.proj_points && b.proj_match &&
           b.edge_of_kp;
}

// The current frame of a window search's host form: n_kp keypoints and their grid CSR.  open() stages it as slots
// 0 .. 5 (keys_un, desc, uright, grid_off, grid_idx, count), every array padded to cap = max(n_kp, 1) entries, with
// the entry's own slots behind them from kFirst on; current() is the device view of the opened stage.
struct CurrentFrame {
    static constexpr int kCells = SPSLAM_GRID_COLS * SPSLAM_GRID_ROWS, kFirst = 6;
    const spslam_keypoint* keys_un;
    const uint8_t* desc;
    const float* uright;
    int n_kp;
    const int32_t* grid_off;
    const int32_t* grid_idx;
    int cap() const { return std::max(n_kp, 1); }
    bool args_ok() const { return grid_off && n_kp >= 0 && (!n_kp || (keys_un && desc && uright && grid_idx)); }
    // SPSLAM_OK, or the error of a grid CSR that does not fit the keypoints (call after args_ok)
    int check_grid(spslam_ctx* c) const {
        if (grid_off[0] != 0 || grid_off[kCells] > n_kp)
            return fail(c, SPSLAM_ERR_ARG, "grid CSR does not fit the keypoints%s", "");
        return SPSLAM_OK;
    }
    int open(Stage& st, std::initializer_list<StageSlot> entry_slots) const {
        const size_t K = (size_t)n_kp, C = (size_t)cap();
        std::vector<StageSlot> slots{{keys_un, K * sizeof(spslam_keypoint), C * sizeof(spslam_keypoint)},
                                     {desc, K * 32, C * 32}, {uright, K * 4, C * 4},
                                     {grid_off, (kCells + 1) * 4}, {grid_idx, (size_t)grid_off[kCells] * 4, C * 4},
                                     {&n_kp, sizeof(int)}};
        slots.insert(slots.end(), entry_slots.begin(), entry_slots.end());
        return st.open(slots.data(), (int)slots.size());
    }
    MatchCurrent current(const Stage& st) const {
        return {st.slot<spslam_keypoint>(0), st.slot<uint8_t>(1), st.slot<float>(2), st.slot<int32_t>(3),
                st.slot<int32_t>(4), st.slot<int>(5), cap()};
    }
};
