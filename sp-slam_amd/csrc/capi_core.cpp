// C ABI (include/spslam_gpu.h): context create/destroy, ORB tables and geometry, timing.
#include "capi_ctx.h"

#include <cmath>
#include <cstring>
#include <new>

namespace {

int cv_round(float v) { return (int)std::nearbyint(v); }

// ORBextractor::ORBextractor tables, src/ORBextractor.cc:415-469.
void build_tables(spslam_ctx* c) {
    const int nl = c->p.nlevels;
    const double scaleFactor = c->p.scale_factor;  // member is double, ctor arg float
    c->scale.assign(nl, 1.f); c->sigma2.assign(nl, 1.f);
    for (int i = 1; i < nl; i++) {
        c->scale[i] = (float)(c->scale[i - 1] * scaleFactor);
        c->sigma2[i] = c->scale[i] * c->scale[i];
    }
    c->inv_scale.resize(nl); c->inv_sigma2.resize(nl);
    for (int i = 0; i < nl; i++) {
        c->inv_scale[i] = 1.0f / c->scale[i];
        c->inv_sigma2[i] = 1.0f / c->sigma2[i];
    }
    c->nfeat.assign(nl, 0);
    float factor = (float)(1.0f / scaleFactor);
    float nDesired = c->p.nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nl));
    int sum = 0;
    for (int l = 0; l < nl - 1; l++) {
        c->nfeat[l] = cv_round(nDesired);
        sum += c->nfeat[l];
        nDesired *= factor;
    }
    c->nfeat[nl - 1] = std::max(c->p.nfeatures - sum, 0);
    const int HP = 15;
    int v, v0, vmax = (int)std::floor(HP * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(HP * std::sqrt(2.f) / 2);
    const double hp2 = HP * HP;
    for (v = 0; v <= vmax; ++v) c->umax[v] = (int)std::nearbyint(std::sqrt(hp2 - v * v));
    for (v = HP, v0 = 0; v >= vmin; --v) {
        while (c->umax[v0] == c->umax[v0 + 1]) ++v0;
        c->umax[v] = v0;
        ++v0;
    }
}

// Pyramid + FAST-cell geometry (src/ORBextractor.cc:769-787, 1111-1112) and
// scratch layout.  Returns an error string for unsupported shapes.
const char* build_geom(spslam_ctx* c) {
    OrbGeom& g = c->geom;
    std::memset(&g, 0, sizeof g);
    g.nlevels = c->p.nlevels;
    long long pyr = 0, blur = 0;
    int cells = 0, kpb = 0, keyb = 0;
    for (int l = 0; l < g.nlevels; l++) {
        LevelGeom& L = g.lv[l];
        L.w = cv_round((float)c->p.width * c->inv_scale[l]);
        L.h = cv_round((float)c->p.height * c->inv_scale[l]);
        if (L.w > 4095 || L.h > 4095) return "level wider/taller than 4095 px";
        L.maxBorderX = L.w - kEdgeThreshold + 3;
        L.maxBorderY = L.h - kEdgeThreshold + 3;
        const float width = (float)(L.maxBorderX - kMinBorder), height = (float)(L.maxBorderY - kMinBorder);
        L.nCols = (int)(width / 30.f);
        L.nRows = (int)(height / 30.f);
        if (L.nCols < 1 || L.nRows < 1) return "pyramid level smaller than one FAST cell (reference divides by zero)";
        L.wCell = (int)std::ceil(width / L.nCols);
        L.hCell = (int)std::ceil(height / L.nRows);
        if (L.wCell + 6 > kCellWinMax || L.hCell + 6 > kCellWinMax) return "FAST cell window exceeds LDS tile";
        if (((L.wCell + 1) / 2) * ((L.hCell + 1) / 2) > kCellCap) return "FAST cell survivor bound exceeds kCellCap";
        const int nIni = (int)std::round(width / height);
        if (nIni < 1 || 4 * nIni > 64) return "unsupported aspect ratio for DistributeOctTree";
        L.cell_base = cells;
        cells += L.nCols * L.nRows;
        if (L.nCols * L.nRows > 2048) return "too many FAST cells per level";
        L.nfeat = c->nfeat[l];
        L.kp_cap = std::max(L.nfeat + 16, 4 * nIni + 4);
        if (L.kp_cap > kNodeCap) return "nfeatures per level exceeds DistributeOctTree node capacity";
        L.kp_base = kpb;
        kpb += L.kp_cap;
        L.key_base = keyb;
        keyb += L.nCols * L.nRows * kCellCap;
        L.scale = c->scale[l];
        L.patch_size = (int)(31 * c->scale[l]);
        // pitched rows (multiple of 64 bytes): level_kernel writes 4 pixels per dword store, its 64-wide
        // tiles never cross a row's padded end
        L.bpitch = (L.w + kLevelTileW - 1) / kLevelTileW * kLevelTileW;
        if (l > 0) {
            L.stride = L.bpitch;
            L.img = reinterpret_cast<const uint8_t*>(pyr);  // offset, rebased after allocation
            pyr += (long long)L.stride * L.h;
        }
        L.blur = reinterpret_cast<uint8_t*>(blur);
        L.score = reinterpret_cast<uint8_t*>(blur);
        blur += (long long)L.bpitch * L.h;
        L.tiles_x = (L.w + kLevelTileW - 1) / kLevelTileW;
        g.level_tiles[l] = L.tiles_x * ((L.h + kLevelTileH - 1) / kLevelTileH);
        if (l > 0) {
            L.rscale_x = 1. / ((double)L.w / g.lv[l - 1].w);
            L.rscale_y = 1. / ((double)L.h / g.lv[l - 1].h);
        }
    }
    c->pyr_frame_stride = (pyr + 255) / 256 * 256;
    c->blur_frame_stride = (blur + 255) / 256 * 256;
    g.cells_per_frame = cells;
    g.lvl_kp_per_frame = kpb;
    g.keys_per_frame = keyb;
    c->max_kp = kpb;
    return nullptr;
}

}  // namespace

extern "C" {

int spslam_create(int device, const spslam_orb_params* params, spslam_ctx** out) {
    if (!params || !out) return SPSLAM_ERR_ARG;
    *out = nullptr;
    spslam_ctx* c = new (std::nothrow) spslam_ctx();
    if (!c) return SPSLAM_ERR_ARG;
    c->device = device;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            c->num_cus = cus;
    }
    c->p = *params;
    if (c->p.nlevels < 1 || c->p.nlevels > SPSLAM_MAX_LEVELS || c->p.nfeatures < 1 || c->p.scale_factor <= 1.f ||
        c->p.width < 64 || c->p.height < 64 || c->p.max_batch < 1) {
        delete c;
        return SPSLAM_ERR_ARG;
    }
    build_tables(c);
    if (const char* e = build_geom(c)) {
        delete c;
        std::fprintf(stderr, "spslam_create: %s\n", e);
        return SPSLAM_ERR_ARG;
    }
    int rc = SPSLAM_OK;
    auto hip_ok = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == SPSLAM_OK) {
            rc = fail(c, SPSLAM_ERR_HIP, "%s", what);
            c->err += std::string(": ") + hipGetErrorString(e);
        }
        return e == hipSuccess;
    };
    if (!hip_ok(hipSetDevice(device), "hipSetDevice") ||
        !hip_ok(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate") ||
        !hip_ok(orb_upload_tables(c->umax), "upload tables")) {
        std::fprintf(stderr, "spslam_create: %s\n", c->err.c_str());
        delete c;
        return SPSLAM_ERR_HIP;
    }
    const size_t B = (size_t)c->p.max_batch;
    const OrbGeom& g = c->geom;
    hip_ok(c->d_pyr.alloc(B * c->pyr_frame_stride), "alloc pyramid");
    hip_ok(c->d_blur.alloc(B * c->blur_frame_stride), "alloc blur");
    hip_ok(c->d_score.alloc(B * c->blur_frame_stride), "alloc FAST scores");
    hip_ok(c->d_cand.alloc(B * g.cells_per_frame * kCellCap * sizeof(uint32_t)), "alloc cand");
    hip_ok(c->d_cand_cnt.alloc(B * g.cells_per_frame * sizeof(uint16_t)), "alloc cand_cnt");
    hip_ok(c->d_keys.alloc(B * g.keys_per_frame * sizeof(uint32_t)), "alloc keys");
    hip_ok(c->d_keynode.alloc(B * g.keys_per_frame * sizeof(uint16_t)), "alloc keynode");
    hip_ok(c->d_lvl_kp.alloc(B * g.lvl_kp_per_frame * sizeof(LevelKp)), "alloc lvl_kp");
    hip_ok(c->d_lvl_cnt.alloc(B * kMaxLevels * sizeof(int)), "alloc lvl_cnt");
    hip_ok(c->d_in.alloc((size_t)c->p.width * c->p.height), "alloc input");
    hip_ok(c->d_kps.alloc((size_t)c->max_kp * sizeof(spslam_keypoint)), "alloc kps");
    hip_ok(c->d_desc.alloc((size_t)c->max_kp * 32), "alloc desc");
    hip_ok(c->d_cnt.alloc(sizeof(int) * 4), "alloc cnt");
    if (rc != SPSLAM_OK) {
        std::fprintf(stderr, "spslam_create: %s\n", c->err.c_str());
        delete c;
        return rc;
    }
    c->b = OrbBuffers{c->d_cand, c->d_cand_cnt, c->d_keys, c->d_keynode, c->d_lvl_kp, c->d_lvl_cnt};
    // rebase level offsets onto the allocations
    OrbGeom& gm = c->geom;
    for (int l = 0; l < gm.nlevels; l++) {
        LevelGeom& L = gm.lv[l];
        if (l > 0) {
            L.img = c->d_pyr + reinterpret_cast<long long>(L.img);
            L.frame_stride = c->pyr_frame_stride;
        }
        L.blur = c->d_blur + reinterpret_cast<long long>(L.blur);
        L.score = c->d_score + reinterpret_cast<long long>(L.score);
        L.blur_frame_stride = c->blur_frame_stride;
    }
    *out = c;
    return SPSLAM_OK;
}

void spslam_destroy(spslam_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    delete ctx;  // waits for the last LBA launch, frees the buffers, then destroys the events and streams
}

const char* spslam_last_error(const spslam_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int spslam_orb_tables(const spslam_ctx* c, int* nlevels, float* scale, float* inv_scale, float* sigma2,
                      float* inv_sigma2, int* fpl) {
    if (!c) return SPSLAM_ERR_ARG;
    const int nl = c->p.nlevels;
    if (nlevels) *nlevels = nl;
    for (int l = 0; l < nl; l++) {
        if (scale) scale[l] = c->scale[l];
        if (inv_scale) inv_scale[l] = c->inv_scale[l];
        if (sigma2) sigma2[l] = c->sigma2[l];
        if (inv_sigma2) inv_sigma2[l] = c->inv_sigma2[l];
        if (fpl) fpl[l] = c->nfeat[l];
    }
    return SPSLAM_OK;
}

int spslam_orb_max_keypoints(const spslam_ctx* c) { return c ? c->max_kp : SPSLAM_ERR_ARG; }

int spslam_orb_level_size(const spslam_ctx* c, int level, int* w, int* h) {
    if (!c || level < 0 || level >= c->p.nlevels) return SPSLAM_ERR_ARG;
    *w = c->geom.lv[level].w;
    *h = c->geom.lv[level].h;
    return SPSLAM_OK;
}

int spslam_set_timing(spslam_ctx* c, int enable) {
    if (!c) return SPSLAM_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (enable && !c->timer) c->timer = new EventTimer();
    if (!enable && c->timer) { delete c->timer; c->timer = nullptr; }
    if (c->timer) c->timer->reset();
    return SPSLAM_OK;
}

int spslam_kernel_times(spslam_ctx* c, double* total_ms, long long* launches, int max_kinds) {
    if (!c) return SPSLAM_ERR_ARG;
    const int n = std::min(max_kinds, (int)kNumKernelKinds);
    if (c->timer) c->timer->collect();
    for (int k = 0; k < n; k++) {
        if (total_ms) total_ms[k] = c->timer ? c->timer->total_ms[k] : 0.0;
        if (launches) launches[k] = c->timer ? c->timer->count[k] : 0;
    }
    return n;
}

const char* spslam_kernel_name(int kind) { return kernel_kind_name(kind); }

}  // extern "C"
