/* spslam_gpu.h -- C ABI of the MI355X (gfx950) implementation of SP-SLAM's
 * per-frame RGB-D tracking hot path.
 *
 * Plain C: no C++/torch types cross this boundary; every buffer is
 * caller-owned (host pointers for the drop-in entry points, device pointers
 * for the *_device batch entry points).  Errors are returned as negative
 * status codes, the message is kept per context (spslam_last_error); nothing
 * throws across the ABI and nothing calls exit().
 *
 * Threading: one context per calling host thread.  A context owns its device
 * scratch and one HIP stream, mirroring the reference, where Tracking
 * (ORB/planes/pose) and LocalMapping (LBA) run on different threads
 * (src/System.cc:92-106).
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   spslam_orb_*        ORB_SLAM2::ORBextractor (include/ORBextractor.h:45-111,
 *                       src/ORBextractor.cc:410-470, 1043-1132)
 *   spslam_pose_*       Optimizer::PoseOptimization (include/Optimizer.h:47,
 *                       src/Optimizer.cc:519-1152) with g2oAddition plane edges
 *   spslam_planes_extract*  Frame::ComputePlanesFromOrganizedPointCloud
 *                       (include/Frame.h:120, src/Frame.cc:854-936)
 *   spslam_planes_generate_from_boundaries*  Frame::GeneratePlanesFromBoundries
 *                       (include/Frame.h:121, src/Frame.cc:938-1144)
 *   spslam_frame_*      RGB-D Frame constructor keypoint steps (src/Frame.cc:146-181)
 *   spslam_lba_*        Optimizer::LocalBundleAdjustment (include/Optimizer.h:46,
 *                       src/Optimizer.cc:1154-1977)
 *   spslam_planes_associate*  Map::AssociatePlanesByBoundary (include/Map.h:69-74,
 *                       src/Map.cc:196-359)
 */
#ifndef SPSLAM_GPU_H
#define SPSLAM_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPSLAM_OK 0
#define SPSLAM_ERR_ARG (-1)        /* bad argument / shape */
#define SPSLAM_ERR_CAPACITY (-2)   /* caller buffer too small (count still written) */
#define SPSLAM_ERR_HIP (-3)        /* HIP runtime error */
#define SPSLAM_ERR_NOT_READY (-4)  /* stage data requested before it was computed */

typedef struct spslam_ctx spslam_ctx;

/* Bit-compatible with cv::KeyPoint {Point2f pt; float size, angle, response;
 * int octave, class_id;} (28 bytes), the element type of the reference's
 * std::vector<cv::KeyPoint> output (include/ORBextractor.h:59-61). */
typedef struct spslam_keypoint {
    float x, y;
    float size;
    float angle;
    float response;
    int32_t octave;
    int32_t class_id;
} spslam_keypoint;

/* ORBextractor constructor arguments (include/ORBextractor.h:51-52; values
 * come from ORBextractor.* keys of the YAML, src/Tracking.cc:113-119), plus the
 * image geometry and the largest batch the context must hold. */
typedef struct spslam_orb_params {
    int nfeatures;      /* ORBextractor.nFeatures (1000) */
    float scale_factor; /* ORBextractor.scaleFactor (1.2) */
    int nlevels;        /* ORBextractor.nLevels (8), <= SPSLAM_MAX_LEVELS */
    int ini_th_fast;    /* ORBextractor.iniThFAST (20) */
    int min_th_fast;    /* ORBextractor.minThFAST (7) */
    int width, height;  /* input image size */
    int max_batch;      /* frames per batched call */
} spslam_orb_params;

#define SPSLAM_MAX_LEVELS 8

/* Create a context on HIP device `device`.  Replaces `new ORBextractor(...)`
 * (src/Tracking.cc:119). */
int spslam_create(int device, const spslam_orb_params* params, spslam_ctx** out);
void spslam_destroy(spslam_ctx* ctx);
const char* spslam_last_error(const spslam_ctx* ctx);

/* Per-level tables: GetLevels / GetScaleFactor(s) / GetInverseScaleFactors /
 * GetScaleSigmaSquares / GetInverseScaleSigmaSquares
 * (include/ORBextractor.h:63-83).  Any output pointer may be NULL. */
int spslam_orb_tables(const spslam_ctx* ctx, int* nlevels, float* scale, float* inv_scale, float* sigma2,
                      float* inv_sigma2, int* features_per_level);

/* Upper bound on keypoints one frame can produce (size caller buffers with it). */
int spslam_orb_max_keypoints(const spslam_ctx* ctx);

/* Drop-in for ORBextractor::operator()(image, mask, keypoints, descriptors)
 * (include/ORBextractor.h:59-61, src/ORBextractor.cc:1043-1105): host gray
 * u8 image in, keypoints (level order) + n x 32 descriptor bytes out.
 * The mask is ignored by the reference and is not taken here.  An empty
 * image (w == 0 or h == 0) returns SPSLAM_OK with *n = 0 and buffers
 * untouched.  The image size must equal the context's width/height. */
int spslam_orb_extract(spslam_ctx* ctx, const uint8_t* gray, int w, int h, int stride, spslam_keypoint* kps,
                       uint8_t* desc, int cap, int* n);

/* Throughput entry: n_frames gray frames already resident in device memory
 * (frame f at d_gray + f*frame_stride, rows `stride` bytes apart).  Writes,
 * per frame f, counts[f] keypoints to d_kps + f*cap_per_frame and
 * descriptors to d_desc + f*cap_per_frame*32.  Asynchronous on `hip_stream`
 * (a hipStream_t).  In every *_batch_device call NULL means HIP's default
 * (NULL) stream -- the one PyTorch calls its default stream -- so device
 * buffers filled by the caller on that stream are ordered before the work;
 * the host-buffer drop-ins run on the context's own stream. */
int spslam_orb_extract_batch_device(spslam_ctx* ctx, const uint8_t* d_gray, int n_frames, size_t frame_stride,
                                    int stride, spslam_keypoint* d_kps, uint8_t* d_desc, int* d_counts,
                                    int cap_per_frame, void* hip_stream);

/* Stage access for parity tests (valid for frame `frame` of the last call).
 * stage: 0 = pyramid level image (w*h bytes), 1 = blurred level (w*h bytes),
 *        2 = FAST cell candidates of the level, as spslam_keypoint with
 *            coordinates relative to (minBorderX, minBorderY) like
 *            src/ORBextractor.cc:822-824 (count in *n),
 *        3 = DistributeOctTree output of the level (level coordinates, before
 *            orientation; count in *n). */
int spslam_orb_debug_stage(spslam_ctx* ctx, int frame, int level, int stage, void* out, int cap, int* n);
int spslam_orb_level_size(const spslam_ctx* ctx, int level, int* w, int* h);

/* ------------------------------------------------------------------------
 * PoseOptimization (src/Optimizer.cc:519-1152; include/Optimizer.h:47).
 *
 * The reference builds a g2o graph from Frame/MapPoint/MapPlane members; at
 * this boundary the caller passes those members flattened:
 *   - one spslam_point_obs per keypoint i with mvpMapPoints[i] != NULL, in
 *     increasing i (the reference's edge insertion order, :561-647);
 *   - one spslam_plane_obs per plane edge, all kind 0 (mvpMapPlanes) first,
 *     then kind 1 (mvpParallelPlanes), then kind 2 (mvpVerticalPlanes), each
 *     in increasing plane index (:700-859).  world = MapPlane::GetWorldPos(),
 *     meas = Frame::mvPlaneCoefficients[i]; map_plane_id = MapPlane::mnId
 *     (only used for the vertex-id bookkeeping the reference does).
 * Results: the optimized Tcw (what Frame::SetPose receives, :1149-1150), the
 * returned inlier count (:1151; 0 when fewer than 3 point correspondences,
 * :653), and the per-observation outlier flags (mvbOutlier, mvbPlaneOutlier,
 * mvbParPlaneOutlier, mvbVerPlaneOutlier). */
typedef struct spslam_point_obs {
    float u, v;        /* mvKeysUn[i].pt */
    float ur;          /* mvuRight[i]; < 0 -> monocular edge */
    float inv_sigma2;  /* mvInvLevelSigma2[mvKeysUn[i].octave] */
    float xw[3];       /* MapPoint::GetWorldPos() */
    int32_t kp_index;  /* i (informational) */
} spslam_point_obs;

#define SPSLAM_PLANE_EDGE 0      /* g2o::EdgePlane          (3-D error) */
#define SPSLAM_PARALLEL_EDGE 1   /* g2o::EdgeParallelPlane  (2-D error) */
#define SPSLAM_VERTICAL_EDGE 2   /* g2o::EdgeVerticalPlane  (2-D error) */

typedef struct spslam_plane_obs {
    float meas[4];     /* frame plane coefficients (a,b,c,d) */
    float world[4];    /* map plane world coefficients */
    int32_t kind;      /* SPSLAM_*_EDGE */
    int32_t plane_index;
    int32_t map_plane_id;
    int32_t pad;
} spslam_plane_obs;

/* Config keys read by PoseOptimization (src/Optimizer.cc:681-693; YAML
 * Plane.AngleInfo/DistanceInfo/ParallelInfo/VerticalInfo/Chi/VPChi). */
typedef struct spslam_plane_config {
    double angle_info, distance_info, parallel_info, vertical_info, chi, vp_chi;
} spslam_plane_config;

typedef struct spslam_pose_problem {
    float Tcw[16];      /* Frame::mTcw, row-major 4x4 */
    float fx, fy, cx, cy, bf;
    int32_t n_points;   /* observations [point_offset, point_offset + n_points) */
    int32_t n_planes;
    int32_t point_offset;
    int32_t plane_offset;
    int32_t pad;
} spslam_pose_problem;

typedef struct spslam_pose_result {
    float Tcw[16];      /* optimized pose (unchanged input if n_inliers == 0 by the <3 rule) */
    int32_t n_inliers;  /* PoseOptimization return value */
    int32_t lm_iterations;  /* total LM iterations run (diagnostic); -1 = the device gave up on a bounded
                               internal wait (never observed): invalid result, Tcw = input, n_inliers = 0,
                               every point / plane outlier flag set to 1 */
    int32_t trial_passes;   /* edge passes at trial poses (damping trials are evaluated 4 per pass; diagnostic) */
    int32_t trials;         /* damping trials the reference evaluated (computeActiveErrors calls; diagnostic) */
} spslam_pose_result;

/* Drop-in for Optimizer::PoseOptimization(Frame*) on host buffers, one frame.
 * point_outlier / plane_outlier (n_points / n_planes bytes) receive the
 * outlier flags. */
int spslam_pose_optimize(spslam_ctx* ctx, const spslam_pose_problem* problem, const spslam_point_obs* points,
                         const spslam_plane_obs* planes, const spslam_plane_config* cfg, spslam_pose_result* result,
                         uint8_t* point_outlier, uint8_t* plane_outlier);

/* Batched, device resident: n problems, one workgroup each.  Observation
 * arrays are indexed through each problem's point/plane offsets; the outlier
 * flag arrays share those offsets.  If d_init_from is non-NULL, problem p
 * starts from d_init_from[p].Tcw instead of its own Tcw (used to chain the
 * motion-model and local-map optimizations of one frame on the device).
 * Asynchronous on hip_stream (NULL = the default stream). */
int spslam_pose_optimize_batch_device(spslam_ctx* ctx, int n, const spslam_pose_problem* d_problems,
                                      const spslam_point_obs* d_points, const spslam_plane_obs* d_planes,
                                      const spslam_plane_config* cfg, const spslam_pose_result* d_init_from,
                                      spslam_pose_result* d_results, uint8_t* d_point_outlier,
                                      uint8_t* d_plane_outlier, void* hip_stream);

/* ------------------------------------------------------------------------
 * LocalBundleAdjustment (include/Optimizer.h:46, src/Optimizer.cc:1154-1977)
 * from the point where the local graph is known.  The caller (LocalMapping's
 * shim) flattens what the reference collects from the Map:
 *   keyframes  lLocalKeyFrames in list order (fixed = 0; mnId 0 is held fixed
 *              like the reference), then lFixedCameras (fixed = 1);
 *   points     lLocalMapPoints in list order, each with its observations in
 *              MapPoint::GetObservations() order (std::map<KeyFrame*>:
 *              pointer order in the reference, keyframe-id order here --
 *              SURVEY.md Appendix A.9), observations of bad keyframes dropped;
 *   planes     lLocalMapPlanes in list order, each with its GetObservations()
 *              edges (kind SPSLAM_PLANE_EDGE), then GetVerObservations()
 *              (SPSLAM_VERTICAL_EDGE), then GetParObservations()
 *              (SPSLAM_PARALLEL_EDGE), the reference's edge insertion order.
 * Results: poses of the local keyframes (KeyFrame::SetPose), point positions
 * (MapPoint::SetWorldPos), plane coefficients (MapPlane::SetWorldPos), and per
 * observation the outlier flag the reference acts on (point observations:
 * vToErase -> EraseMapPointMatch / EraseObservation; plane observations:
 * chi2 above Plane.Chi / VPChi, informational -- the reference's erase is
 * commented out, Optimizer.cc:1862-1870).  The not-seen plane branches are
 * dead in the reference (SURVEY.md 8 notes) and are not represented. */
typedef struct spslam_lba_keyframe {
    float Tcw[16];            /* KeyFrame::GetPose(), row-major */
    float fx, fy, cx, cy, bf; /* KeyFrame::fx..cy, mbf (edge intrinsics) */
    int32_t id;               /* KeyFrame::mnId (g2o vertex id) */
    int32_t fixed;            /* 1 = fixed camera */
    int32_t pad;
} spslam_lba_keyframe;

typedef struct spslam_lba_point {
    float xw[3];              /* MapPoint::GetWorldPos() */
    int32_t id;               /* MapPoint::mnId */
    int32_t obs_offset;       /* observations [obs_offset, obs_offset + n_obs) */
    int32_t n_obs;
} spslam_lba_point;

typedef struct spslam_lba_point_obs {
    int32_t kf;               /* index into the problem's keyframes */
    float u, v;               /* KeyFrame::mvKeysUn[idx].pt */
    float ur;                 /* KeyFrame::mvuRight[idx]; < 0 -> monocular edge */
    float inv_sigma2;         /* KeyFrame::mvInvLevelSigma2[octave] */
} spslam_lba_point_obs;

typedef struct spslam_lba_plane {
    float world[4];           /* MapPlane::GetWorldPos() */
    int32_t id;               /* MapPlane::mnId */
    int32_t obs_offset;
    int32_t n_obs;
    int32_t pad;
} spslam_lba_plane;

typedef struct spslam_lba_plane_obs {
    int32_t kf;
    int32_t kind;             /* SPSLAM_PLANE_EDGE / SPSLAM_VERTICAL_EDGE / SPSLAM_PARALLEL_EDGE */
    float meas[4];            /* KeyFrame::mvPlaneCoefficients[idx] */
} spslam_lba_plane_obs;

/* One problem of a batch: its keyframes / points / planes start at the given
 * offsets of the batch arrays; observation offsets inside points / planes are
 * absolute indices into the batch observation arrays. */
typedef struct spslam_lba_problem {
    int32_t n_kf, n_points, n_planes;
    int32_t kf_offset, point_offset, plane_offset;
    int32_t n_point_obs, n_plane_obs;   /* total observations of its points / planes */
} spslam_lba_problem;

typedef struct spslam_lba_result {
    int32_t iterations[2];    /* LM iterations of optimize(5) / optimize(10) */
    int32_t n_point_outliers; /* flagged point observations */
    int32_t n_plane_outliers;
    int32_t status;           /* 0 ok, < 0 capacity / numerical failure */
    int32_t trials;           /* LM trials (lambda steps) in total */
    int32_t stopped;          /* pbStopFlag: 0 not seen (or seen after the schedule ended), 1 seen before
                                 optimize(5) -- returned, outputs = inputs, no outliers -- 2 seen at a later
                                 check point: the schedule ended there (trials = trials run) */
    int32_t pad;              /* diagnostics (g2o order: the sums part of buildSystem, microseconds; else 0) */
    float phase_us[8];        /* diagnostics, device microseconds.  g2o order: [0] the whole call (kernel start
                                 to outputs), then the leader's time per phase: [1] setup, structure, update
                                 and the LM decisions, [2] errors, [3] the ordered chi2 / scale sums,
                                 [4] buildSystem (edge terms and block sums), [5] Schur, [6] factorisation
                                 and solve, [7] unused (0).  Fast order: [0] setup to outputs, [1..7] 0.
                                 Diagnostic builds (SPSLAM_LBG_DIAG*) put other figures in [1..7] and pad. */
} spslam_lba_result;

/* Drop-in for Optimizer::LocalBundleAdjustment on host buffers, one problem
 * (offsets inside *problem are ignored; observation offsets index obs arrays).
 * stop_flag = pbStopFlag (NULL allowed): a bool another thread may raise while
 * the call runs (LocalMapping::InterruptBA); it is copied to the device at the
 * call and at every host poll of the schedule and honoured at g2o's check
 * points (result.stopped).
 * kf_out: 16 floats per keyframe (local keyframes optimised, fixed ones
 * copied), pt_out 3 per point, pl_out 4 per plane, outlier flags per
 * observation.  cfg = the Plane.* config keys (as for PoseOptimization). */
int spslam_lba_optimize(spslam_ctx* ctx, const spslam_lba_problem* problem, const spslam_lba_keyframe* kfs,
                        const spslam_lba_point* points, const spslam_lba_point_obs* point_obs,
                        const spslam_lba_plane* planes, const spslam_lba_plane_obs* plane_obs,
                        const spslam_plane_config* cfg, float* kf_out, float* pt_out, float* pl_out,
                        uint8_t* point_obs_outlier, uint8_t* plane_obs_outlier, spslam_lba_result* result,
                        const volatile uint8_t* stop_flag);

/* Summation order of the LocalBundleAdjustment entries (default SPSLAM_LBA_G2O_ORDER):
 *   SPSLAM_LBA_G2O_ORDER  g2o's own arithmetic, bit-exact to the reference-order oracle: edge-insertion-order
 *                         sums, the landmark-ordered Schur complement (block_solver.hpp:381-431), Eigen's
 *                         SimplicialLDLT with its AMD ordering (linear_solver_eigen.h:58-121); one workgroup per
 *                         problem, the whole schedule in one launch;
 *   SPSLAM_LBA_FAST_ORDER the grid-wide phase kernels (tree-ordered reductions, Schur sums on the f64 matrix
 *                         cores, natural-order LDL^T): the same algorithm to rounding (<= 1e-4 on the tested maps),
 *                         a throughput mode for maps that do not need the reference's bits. */
#define SPSLAM_LBA_G2O_ORDER 0
#define SPSLAM_LBA_FAST_ORDER 1
int spslam_lba_set_order(spslam_ctx* ctx, int order);

/* Test hook (deterministic LocalMapping::InterruptBA): the context's following
 * LocalBundleAdjustment calls see pbStopFlag raised once a problem has run
 * `trials` LM trials -- before optimize(5) when 0 -- at the same check points
 * as a raised flag; -1 turns the hook off (default). */
int spslam_lba_debug_stop_after(spslam_ctx* ctx, int trials);

/* Workgroups per problem of the SPSLAM_LBA_G2O_ORDER launch (1 .. 16; 0, the
 * default: as many as fill the device's compute units, at most 8).  Results do
 * not depend on it: every sum keeps g2o's order whatever the split. */
int spslam_lba_set_team(spslam_ctx* ctx, int workgroups);

/* Batched, device resident: n problems (host copy `problems` for sizing, the
 * same records on the device at d_problems), a team of workgroups each
 * (spslam_lba_set_team), the whole optimize(5) / relabel / optimize(10)
 * schedule on the device.  Outputs are indexed like the inputs (keyframe /
 * point / plane offsets of each problem, absolute observation indices).
 * SPSLAM_LBA_G2O_ORDER: at most 1024 keyframes per problem (local + fixed) of
 * which at most 128 free poses (local keyframes, id != 0, with an active
 * edge; batches whose windows all hold <= 64 keyframes run the narrow
 * instance, others the wide one); SPSLAM_LBA_FAST_ORDER: at most 64 keyframes; status -2 otherwise
 * (nothing else written for that problem).  d_stop_flags: one pbStopFlag per
 * problem in device-visible memory (device, or host-mapped coherent memory
 * another thread raises), nonzero = stop; NULL = no flags.  Results are
 * complete on hip_stream (SPSLAM_LBA_G2O_ORDER only enqueues one launch; the
 * fast order polls the device and returns once every problem is done).  One
 * LocalBundleAdjustment call per context is in flight at a time: a call on
 * another stream first waits (on the device) for the context's previous call,
 * whose scratch it reuses. */
int spslam_lba_optimize_batch_device(spslam_ctx* ctx, int n, const spslam_lba_problem* problems,
                                     const spslam_lba_problem* d_problems, const spslam_lba_keyframe* d_kfs,
                                     const spslam_lba_point* d_points, const spslam_lba_point_obs* d_point_obs,
                                     const spslam_lba_plane* d_planes, const spslam_lba_plane_obs* d_plane_obs,
                                     const spslam_plane_config* cfg, float* d_kf_out, float* d_pt_out,
                                     float* d_pl_out, uint8_t* d_point_obs_outlier, uint8_t* d_plane_obs_outlier,
                                     spslam_lba_result* d_results, const int32_t* d_stop_flags, void* hip_stream);

/* ------------------------------------------------------------------------
 * Plane extraction: Frame::ComputePlanesFromOrganizedPointCloud
 * (include/Frame.h:120, src/Frame.cc:854-936) with the PCL 1.8
 * IntegralImageNormalEstimation + OrganizedMultiPlaneSegmentation it calls.
 *
 * Input: the float depth image in meters the RGB-D Frame constructor
 * receives (imDepth, CV_32F, src/Tracking.cc:230-231).  Output per frame:
 * the planes Frame appends to mvPlaneCoefficients (d >= 0, PlaneNotSeen
 * de-duplicated, in the reference's order) with, per plane, the
 * organized-cloud indices of its inliers (mvPlanePoints) and of its contour
 * (mvBoundaryPoints).  The organized cloud itself (points (x, y, z), row-major
 * ceil(h/dis) x ceil(w/dis)) is available through spslam_planes_cloud. */
typedef struct spslam_plane_params {
    int cloud_dis;            /* Cloud.Dis (3) */
    int min_size;             /* Plane.MinSize (500) */
    float angle_threshold;    /* Plane.AngleThreshold, degrees (3.0) */
    float distance_threshold; /* Plane.DistanceThreshold (0.05) */
    float fx, fy, cx, cy;     /* static Frame::fx, fy, cx, cy */
    int width, height;        /* depth image size */
    /* GeneratePlanesFromBoundries (src/Frame.cc:938-998) */
    double line_ratio;             /* Line.Ratio (0.2) */
    float line_distance_threshold; /* Line.DistanceThreshold (0.01) */
    float image_bounds[4];         /* Frame::mnMinX, mnMaxX, mnMinY, mnMaxY; all 0 -> 0, width, 0, height
                                      (Frame::ComputeImageBounds without distortion, src/Frame.cc:557-563) */
} spslam_plane_params;

typedef struct spslam_plane {
    float coef[4];            /* mvPlaneCoefficients entry */
    int32_t n_inliers;        /* mvPlanePoints size */
    int32_t inlier_offset;    /* into the frame's inlier index buffer */
    int32_t n_contour;        /* mvBoundaryPoints size */
    int32_t contour_offset;   /* into the frame's contour index buffer */
} spslam_plane;

/* Configure (and allocate scratch for max_batch frames) the plane stage.
 * SPSLAM_ERR_ARG for a geometry no kernel instance takes, so that an extraction never refuses a configured
 * one.  The organized cloud is W = ceil(width / cloud_dis) columns by H = ceil(height / cloud_dis) rows:
 *   W <= 512 (eight 64-bit row words) and H <= 512 (one lane per row in the distance-map kernels),
 *   N = W * H <= 160000.
 * There is no lower bound: clouds down to 1 x 1 are extracted (a cloud of 20 or fewer rows or columns has
 * no valid normal, IntegralImageNormalEstimation's border being 10, and so no plane). */
int spslam_planes_configure(spslam_ctx* ctx, const spslam_plane_params* params);

/* Capacities the caller must provide per frame: planes, inlier indices,
 * contour indices.
 *
 * Limits the reference does not have (the segmentation kernel's LDS tables rest on them).  Per frame at most
 *   255 connected components larger than Plane.MinSize (in label order; later ones are not fitted),
 *   64 plane models (components passing the curvature test, in label order; later ones are dropped), and
 *   64 kept planes (planes_cap).
 * A frame past a limit still yields well-formed output (counts[f] <= planes_cap, every offset + length
 * within the capacities), but not the reference's planes.  It is reported: see spslam_planes_status. */
int spslam_planes_capacity(const spslam_ctx* ctx, int* planes_cap, int* inlier_cap, int* contour_cap);

/* Limits a frame crossed (spslam_planes_status flags). */
#define SPSLAM_PLANES_OVER_COMPONENTS 1 /* more than 255 components larger than Plane.MinSize */
#define SPSLAM_PLANES_OVER_MODELS 2     /* more than 64 plane models */
#define SPSLAM_PLANES_OVER_KEPT 4       /* more kept planes than planes_cap: reserved.  Every entry passes
                                           planes_cap = 64, the model limit, so today it is never set. */

/* Drop-in for one frame, host buffers.  *n_planes receives the plane count;
 * inliers / contours receive the index lists referenced by planes[].
 * SPSLAM_ERR_CAPACITY (outputs filled as far as the limits go, the message names the limit) when the frame
 * crossed one of the limits above. */
int spslam_planes_extract(spslam_ctx* ctx, const float* depth, int w, int h, int stride_floats,
                          spslam_plane* planes, int planes_cap, int* n_planes, int32_t* inliers, int32_t* contours);

/* Batched, device resident: frame f's depth at d_depth + f*frame_stride
 * floats (rows stride_floats apart).  Per frame f: counts[f] planes at
 * d_planes + f*planes_cap, indices at d_inliers + f*inlier_cap and
 * d_contours + f*contour_cap (capacities from spslam_planes_capacity).
 * Asynchronous: a frame past a limit does not change the return value; ask spslam_planes_status. */
int spslam_planes_extract_batch_device(spslam_ctx* ctx, const float* d_depth, int n_frames, size_t frame_stride,
                                       int stride_floats, spslam_plane* d_planes, int* d_counts,
                                       int32_t* d_inliers, int32_t* d_contours, void* hip_stream);

/* *flags = the SPSLAM_PLANES_OVER_* limits frame `frame` of the last extraction crossed (0: none).  Call it
 * after synchronising the stream the extraction ran on; it copies eight bytes from the device.
 * Only the most recently enqueued extraction can be asked: once the next one is enqueued (as a pipelined
 * caller does before the first has finished), the flags of the earlier call read as 0 and are lost.  A caller
 * that needs them asks between the two calls. */
int spslam_planes_status(spslam_ctx* ctx, int frame, int* flags);

/* ------------------------------------------------------------------------
 * Supposed planes: Frame::GeneratePlanesFromBoundries (include/Frame.h:121,
 * src/Frame.cc:938-1144), run by the RGB-D Frame constructor right after
 * ComputePlanesFromOrganizedPointCloud (src/Frame.cc:186-194).  For each
 * plane boundary (last to first) up to 4 lines are fitted with PCL's
 * SACSegmentation (LINE, RANSAC, 1000 iterations, Line.DistanceThreshold,
 * optimized coefficients); a line that keeps >= Line.Ratio of the boundary,
 * lies >= 50 px inside the image (LineInRange) and runs along a depth border
 * (IsBorderLine) yields the plane through the line perpendicular to the source
 * plane (CaculatePlanes), appended when PlaneNotSeen.  Each appended plane
 * carries: its coefficients, the line, the source plane index, its line
 * points (organized-cloud indices; the new plane's mvBoundaryPoints and the
 * tail of its mvPlanePoints) and its synthetic patch (n_patch xyz points, the
 * head of its mvPlanePoints).  A source plane whose boundary was empty gets
 * mvBoundaryPoints = every 20th of its inliers (GenerateBoundaryPoints,
 * src/Frame.cc:1001-1011) -- an output-formatting step the caller's shim does
 * from the inlier list; it produces no lines. */
typedef struct spslam_supposed_plane {
    float coef[4];            /* appended mvPlaneCoefficients entry (d >= 0) */
    float line[6];            /* SACMODEL_LINE coefficients: point + unit direction */
    int32_t source_plane;     /* index i of the plane whose boundary gave the line */
    int32_t n_line;           /* line points */
    int32_t line_offset;      /* into the frame's line index buffer */
    int32_t n_patch;          /* synthetic patch points */
    int32_t patch_offset;     /* into the frame's patch buffer, in points (3 floats each) */
    int32_t pad;
} spslam_supposed_plane;

/* Per-frame capacities: appended planes, line indices, patch points per plane. */
int spslam_supposed_capacity(const spslam_ctx* ctx, int* supp_cap, int* line_cap, int* patch_points);

/* Drop-in for one frame on host buffers: runs on the planes of the last
 * spslam_planes_extract call of this context (the reference calls both on the
 * same Frame).  depth as passed to spslam_planes_extract.  *n receives the
 * number of appended planes; line_idx (line_cap ints) and patch_xyz
 * (supp_cap * patch_points * 3 floats) the data referenced by out[]. */
int spslam_planes_generate_from_boundaries(spslam_ctx* ctx, const float* depth, int w, int h, int stride_floats,
                                           spslam_supposed_plane* out, int cap, int* n, int32_t* line_idx,
                                           float* patch_xyz);

/* Batched, device resident: must follow spslam_planes_extract_batch_device
 * on the same frames (it reads that call's organized clouds) and takes its
 * outputs.  Per frame f: out_counts[f] appended planes at d_out + f*supp_cap,
 * line indices at d_line_idx + f*line_cap, patches at
 * d_patch + f*supp_cap*patch_points*3.  Counts beyond supp_cap are reported
 * but not stored. */
int spslam_planes_generate_from_boundaries_batch_device(spslam_ctx* ctx, const float* d_depth, int n_frames,
                                                        size_t frame_stride, int stride_floats,
                                                        const spslam_plane* d_planes, const int* d_counts,
                                                        const int32_t* d_contours, spslam_supposed_plane* d_out,
                                                        int* d_out_counts, int32_t* d_line_idx, float* d_patch,
                                                        void* hip_stream);

/* Pipelining (no reference counterpart; the reference runs both calls on one
 * Frame before the next): the organized cloud that
 * spslam_planes_extract_batch_device writes and
 * spslam_planes_generate_from_boundaries_batch_device reads is one of two sets,
 * chosen by this call for the calls enqueued after it (host order).  With
 * alternating sets, batch k+1's extraction may run on one stream while batch
 * k's supposed planes run on another; the caller orders a set's reuse after its
 * last reader (stream events).  Set 0 after spslam_planes_configure. */
int spslam_planes_select_cloud_set(spslam_ctx* ctx, int set);

/* Parity access: the line candidates fitted on boundary `plane` of frame
 * `frame` in the last call, in fit order (<= 4; the last may be the failing
 * one).  Per candidate: line[6], inlier count, RANSAC trials, flags (1 kept
 * >= Line.Ratio, 2 LineInRange, 4 IsBorderLine), offset of its points in idx
 * (organized-cloud indices, only for flag-1 candidates). */
typedef struct spslam_line_candidate {
    float line[6];
    int32_t n_inliers;
    int32_t iterations;
    int32_t flags;
    int32_t idx_offset;
} spslam_line_candidate;
int spslam_supposed_debug(spslam_ctx* ctx, int frame, int plane, spslam_line_candidate* cand, int* n_cand,
                          int32_t* idx, int idx_cap);

/* Stage access for parity tests, frame `frame` of the last batch:
 * what 0 = organized cloud (3*N floats, x,y,z per point), 1 = normals
 * (3*N floats, NaN = invalid), 2 = distance map (N floats), 3 = labels after
 * connected components (N uint32, PCL label ids), 4 = segmentation phase
 * timestamps (16 int64 ticks of the 100 MHz GPU real-time clock). */
int spslam_planes_debug(spslam_ctx* ctx, int frame, int what, void* out, int* n_points);

/* Test hook: keep = 1 makes the following plane extractions also store the connected-component labels that
 * spslam_planes_debug(what = 3) returns.  Off by default: frames whose union-find runs in LDS (16-bit labels)
 * then write no label map at all. */
int spslam_debug_plane_labels(spslam_ctx* ctx, int keep);

/* Test hook: the kernels an extraction of n_frames frames launches under the current configuration, from
 * the functions the launch itself dispatches on (nothing runs). */
typedef struct spslam_plane_launch_shape {
    int32_t seg_maps_in_lds;  /* segmentation: per-frame maps and 16-bit union-find parents in LDS (1) or global (0) */
    int32_t seg_positions;    /* segmentation: row positions per lane of the refinement scans, 4 or 8 */
    int32_t wave_count;       /* distance map / integral images: waves per workgroup, ceil(H / 64) */
    int32_t one_workgroup;    /* 1: one workgroup per frame (plane_wave_kernel), 0: three (plane_wave_roles_kernel) */
    int32_t barrier_rows;     /* 0, or the row bound (192, 320, 512) of the barrier kernel
                                 SPSLAM_PLANE_WAVE_BARRIER=1 selects instead of either */
} spslam_plane_launch_shape;
int spslam_debug_plane_launch_shape(spslam_ctx* ctx, int n_frames, spslam_plane_launch_shape* shape);

/* Test hook: Frame::PlaneNotSeen (src/Frame.cc:1116-1130) of each of n_coefs
 * candidate coefficient vectors against n_planes planes (4 floats each, host
 * buffers), evaluated by the device predicate the plane-extraction and
 * supposed-plane kernels use; not_seen[k] = 1 when candidate k would be kept. */
int spslam_debug_plane_not_seen(spslam_ctx* ctx, const float* planes, int n_planes, const float* coefs, int n_coefs,
                                int* not_seen);

/* Test hook: the device's double elementary functions (PoseOptimization and
 * LocalBundleAdjustment: SE3Quat::exp, Plane3D, AngleAxis -> std::sin /
 * std::cos / std::atan2 / std::pow(x, 3)), correctly rounded.
 * kind 0 sin(a), 1 cos(a), 2 atan2(a, b), 3 a^3; n host doubles each. */
int spslam_debug_libm64(spslam_ctx* ctx, int kind, const double* a, const double* b, int n, double* out);

/* Test hook: bound of PoseOptimization's internal waits (the chain wave and the compute waves hand edge rows over
 * through LDS; every wait gives up after `cap` polls).  0 restores the default (2^20 polls, never reached); -1
 * reports every problem as given up, deterministically.  A problem whose wait gave up reports lm_iterations = -1,
 * n_inliers = 0, Tcw = input, and every point and plane outlier flag set (nothing of it is kept). */
int spslam_debug_pose_spin_cap(spslam_ctx* ctx, int cap);

/* Test hook: the context's following PoseOptimization (spslam_pose_optimize*) and g2o-order
 * LocalBundleAdjustment calls treat the linear solve of LM trial q (0-based, counted over each
 * call) as failed when bit q of trial_mask is set -- what g2o does on a non-positive dense LDLT
 * (linear_solver_dense.h:107-112) or a zero SimplicialLDLT pivot (linear_solver_eigen.h:104-110):
 * the solution vector keeps its previous contents, which the update and computeScale then use
 * (optimization_algorithm_levenberg.cpp:110-127).  0 (default) turns it off. */
int spslam_debug_force_solve_failures(spslam_ctx* ctx, unsigned trial_mask);

/* ------------------------------------------------------------------------
 * RGB-D Frame per-keypoint steps (src/Frame.cc:146-181): UndistortKeyPoints
 * (:504-534, cv::undistortPoints with K and mDistCoef), ComputeStereoFromRGBD
 * (:743-764: mvDepth / mvuRight from the depth at the distorted keypoint) and
 * AssignFeaturesToGrid (:326-341: 64 x 48 cells over ComputeImageBounds).
 * Outputs per frame: mvKeysUn (keypoints with undistorted x, y), mvDepth,
 * mvuRight (-1 where no depth) and mGrid as CSR: cell (x, y) = x * 48 + y owns
 * grid_idx[grid_off[cell] .. grid_off[cell + 1]) in increasing keypoint index. */
#define SPSLAM_GRID_COLS 64
#define SPSLAM_GRID_ROWS 48

typedef struct spslam_frame_params {
    float fx, fy, cx, cy;   /* Camera.fx .. cy (mK) */
    float dist[5];          /* Camera.k1 k2 p1 p2 k3 (mDistCoef) */
    float bf;               /* Camera.bf (mbf) */
    int width, height;      /* image size (ComputeImageBounds) */
} spslam_frame_params;

/* Configure the frame stage; computes mnMinX/mnMaxX/mnMinY/mnMaxY and the grid
 * scale like the reference's first Frame (mbInitialComputations, Frame.cc:162-177).
 * bounds (4 floats) and grid_inv (2 floats) may be NULL. */
int spslam_frame_configure(spslam_ctx* ctx, const spslam_frame_params* params, float* bounds, float* grid_inv);

/* Drop-in for one frame on host buffers: kps = mvKeys (n keypoints), depth =
 * imDepth (float meters).  keys_un, mv_depth, mv_uright receive n entries,
 * grid_off 64*48+1 ints, grid_idx up to n ints. */
int spslam_frame_rgbd(spslam_ctx* ctx, const spslam_keypoint* kps, int n, const float* depth, int w, int h,
                      int stride_floats, spslam_keypoint* keys_un, float* mv_depth, float* mv_uright,
                      int32_t* grid_off, int32_t* grid_idx);

/* Batched, device resident, on the ORB batch outputs (frame f: counts[f]
 * keypoints at d_kps + f*cap_per_frame) and the depth frames.  Per frame f:
 * keys_un / depth / uright / grid_idx at f*cap_per_frame, grid_off at
 * f*(64*48+1).  d_plane_counts / d_supp_counts (may be NULL) are zeroed for
 * frames without keypoints: the reference's constructor returns before plane
 * extraction then (Frame.cc:148-149). */
int spslam_frame_rgbd_batch_device(spslam_ctx* ctx, const spslam_keypoint* d_kps, const int* d_counts,
                                   int cap_per_frame, const float* d_depth, int n_frames, size_t frame_stride,
                                   int stride_floats, spslam_keypoint* d_keys_un, float* d_mv_depth,
                                   float* d_mv_uright, int32_t* d_grid_off, int32_t* d_grid_idx,
                                   int* d_plane_counts, int* d_supp_counts, void* hip_stream);

/* ---------------------------------------------------------------- plane association
 * Map::AssociatePlanesByBoundary (src/Map.cc:196-340) with
 * Map::PointDistanceFromPlane (:343-359) and Frame::ComputePlaneWorldCoeff
 * (src/Frame.cc:1146-1150).  For every frame plane (mvPlaneCoefficients, the
 * extracted planes followed by the supposed planes) against the map planes in
 * mnId order (the reference iterates a std::set<MapPlane*> by pointer; the build
 * fixes id order):
 *   |angle| > angle_th and min boundary distance < running distance threshold
 *      -> mvpMapPlanes[i] (the last such map plane wins, thresholds tighten);
 *   else |angle| < running vertical threshold  -> mvpVerticalPlanes[i];
 *   else |angle| > running parallel threshold  -> mvpParallelPlanes[i].
 * Outputs are map-plane indices into the map-plane array (-1 = none) and
 * mbNewPlane (some frame plane without a match).  The reference never clears
 * mvpMapPlanes / mvpParallelPlanes / mvpVerticalPlanes (they are only
 * overwritten when a candidate is found), so the second call of a frame
 * (TrackLocalMap, src/Tracking.cc:1058) starts from what the first call left
 * after TrackWithMotionModel's plane-outlier discard (:1004-1028): with
 * spslam_assoc_frame.carry != 0 the match / parallel / vertical arrays are
 * read as that starting state and updated in place; with carry == 0 they start
 * at -1 (a new Frame, src/Frame.cc:199-213).  The not-seen branches
 * (:259-337) are dead in the reference and are not provided. */
typedef struct spslam_map_plane {
    float world[4];           /* MapPlane::GetWorldPos (a, b, c, d) */
    int32_t id;               /* mnId (informative: the array order is the iteration order) */
    int32_t boundary_offset;  /* first point of mvBoundaryPoints in the boundary xyz array */
    int32_t n_boundary;
    int32_t pad;
} spslam_map_plane;           /* 32 bytes */

typedef struct spslam_assoc_params {
    float dis_th;    /* Plane.AssociationDisRef (mfDisTh) */
    float angle_th;  /* Plane.AssociationAngRef (mfAngleTh) */
    float ver_th;    /* Plane.VerticalThreshold (mfVerTh) */
    float par_th;    /* Plane.ParallelThreshold (mfParTh) */
} spslam_assoc_params;

typedef struct spslam_assoc_frame {
    float Tcw[16];            /* Frame::mTcw, row-major float */
    int32_t map_offset;       /* this frame's map: planes [map_offset, map_offset + n_map) */
    int32_t n_map;
    int32_t carry;            /* != 0: match / parallel / vertical hold the frame's current associations */
    int32_t pad;
} spslam_assoc_frame;         /* 80 bytes */

/* Drop-in for one frame on host buffers.  coefs: n_planes x 4 floats; boundary_xyz:
 * float x, y, z per boundary point.  match / parallel / vertical: n_planes ints
 * (read first when frame->carry != 0); new_plane (may be NULL) receives mbNewPlane. */
int spslam_planes_associate(spslam_ctx* ctx, const spslam_assoc_frame* frame, const float* coefs, int n_planes,
                            const spslam_map_plane* map_planes, int n_map, const float* boundary_xyz,
                            int n_boundary, const spslam_assoc_params* params, int32_t* match, int32_t* parallel,
                            int32_t* vertical, int* new_plane);

/* Batched, device resident.  Frame f's planes are the first d_count_a[f] records of
 * source A (record r of frame f at d_planes_a + (f * cap_a + r) * stride_a bytes,
 * coefficients = its first 4 floats; spslam_plane / spslam_supposed_plane layouts)
 * followed by the first d_count_b[f] records of source B (may be NULL).  Outputs at
 * f * (cap_a + cap_b) + i; d_new_plane: one int per frame (may be NULL).  max_map
 * bounds every frame's n_map (host-known launch size). */
int spslam_planes_associate_batch_device(spslam_ctx* ctx, int n_frames, const spslam_assoc_frame* d_frames,
                                         const void* d_planes_a, int stride_a, const int* d_count_a, int cap_a,
                                         const void* d_planes_b, int stride_b, const int* d_count_b, int cap_b,
                                         const spslam_map_plane* d_map, const float* d_boundary_xyz, int max_map,
                                         const spslam_assoc_params* params, int32_t* d_match, int32_t* d_parallel,
                                         int32_t* d_vertical, int* d_new_plane, void* hip_stream);

/* ---------------------------------------------------------------- projection matching
 * ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame,
 * th, bMono) (src/ORBmatcher.cc:1328-1470) with Frame::GetFeaturesInArea
 * (src/Frame.cc:427-480), DescriptorDistance (src/ORBmatcher.cc:1647-1662) and
 * the rotation-consistency check (ComputeThreeMaxima, :1601-1642), as
 * Tracking::TrackWithMotionModel calls it (src/Tracking.cc:951-975: matcher
 * (0.9, checkOri = true), mvpMapPoints cleared, and when fewer than 20 matches
 * a second search at 2*th).  The last frame is given as its map points: one
 * spslam_proj_point per keypoint i with mvpMapPoints[i] && !mvbOutlier[i], in
 * increasing i.  The current frame is the frame stage's output (mvKeysUn,
 * mvuRight, mGrid) with the ORB descriptors; camera and grid geometry come
 * from spslam_frame_configure, the scale factors from the ORB tables.
 * Output per current keypoint: the index (into the frame's point list) of the
 * map point assigned to it (mvpMapPoints), -1 if none; and nmatches. */
typedef struct spslam_proj_point {
    float xw[3];          /* MapPoint::GetWorldPos */
    float angle;          /* LastFrame.mvKeysUn[i].angle */
    int32_t octave;       /* LastFrame.mvKeys[i].octave */
    int32_t n_obs;        /* MapPoint::Observations(): 0 (a visual-odometry point) does not block a keypoint */
    int32_t last_index;   /* i (informative) */
    int32_t id;           /* MapPoint::mnId (the caller's bookkeeping: seen stamps, next last frame) */
    uint8_t desc[32];     /* MapPoint::GetDescriptor */
} spslam_proj_point;      /* 64 bytes */

typedef struct spslam_proj_frame {
    float Tcw[16];        /* CurrentFrame.mTcw (motion-model prediction), row-major */
    float Tlw[16];        /* LastFrame.mTcw */
    int32_t point_offset; /* this frame's last-frame map points: [point_offset, point_offset + n_points) */
    int32_t n_points;
    int32_t pad[2];
} spslam_proj_frame;      /* 144 bytes */

typedef struct spslam_match_params {
    float th;                   /* window radius at level 0 (15 for RGB-D, Tracking.cc:963-967) */
    int32_t mono;               /* bMono */
    int32_t check_orientation;  /* ORBmatcher mbCheckOrientation */
    int32_t retry_below;        /* nmatches < retry_below -> clear and search at 2*th (20; 0 = no retry) */
} spslam_match_params;

/* Drop-in for one frame pair on host buffers.  keys_un / desc / uright: the
 * current frame's n_kp keypoints; grid_off (64*48+1) / grid_idx: its mGrid CSR.
 * match: n_kp ints.  *nmatches receives the return value of the (last) search. */
int spslam_search_by_projection(spslam_ctx* ctx, const spslam_proj_frame* frame, const spslam_proj_point* points,
                                const spslam_keypoint* keys_un, const uint8_t* desc, const float* uright, int n_kp,
                                const int32_t* grid_off, const int32_t* grid_idx, const spslam_match_params* params,
                                int32_t* match, int* nmatches);

/* Batched, device resident.  Frame f: d_frames[f]; its current frame at
 * d_keys_un / d_uright / d_match + f*cap, d_desc + f*cap*32, d_grid_off +
 * f*(64*48+1), d_grid_idx + f*cap, d_counts[f] keypoints (the ORB / frame-stage
 * batch layouts).  max_points bounds every frame's n_points (host-known launch
 * size).  d_nmatches: one int per frame. */
int spslam_search_by_projection_batch_device(spslam_ctx* ctx, int n_frames, const spslam_proj_frame* d_frames,
                                             const spslam_proj_point* d_points, int max_points,
                                             const spslam_keypoint* d_keys_un, const uint8_t* d_desc,
                                             const float* d_uright, const int32_t* d_grid_off,
                                             const int32_t* d_grid_idx, const int* d_counts, int cap,
                                             const spslam_match_params* params, int32_t* d_match, int* d_nmatches,
                                             void* hip_stream);

/* Local-map projection matching: Tracking::SearchLocalPoints (src/Tracking.cc:
 * 1375-1425) -- Frame::isInFrustum (src/Frame.cc:369-425, viewing-cosine
 * limit 0.5) with MapPoint::PredictScale (src/MapPoint.cc:402-417), then
 * ORBmatcher(nn_ratio).SearchByProjection(F, vpMapPoints, th)
 * (src/ORBmatcher.cc:45-130, RadiusByViewingCos :131-137).  The local map
 * points are given in mvpLocalMapPoints order without those the caller skips
 * (already matched in this frame, or bad).  d_taken (may be NULL) marks the
 * current keypoints whose mvpMapPoints entry is already set with
 * Observations() > 0.  Output per current keypoint: the index of the local
 * point newly assigned to it, -1 otherwise; nmatches; optionally
 * mbTrackInView per point. */
typedef struct spslam_local_point {
    float xw[3];          /* MapPoint::GetWorldPos */
    float normal[3];      /* MapPoint::GetNormal */
    float min_dist;       /* mfMinDistance (the invariance region is 0.8x .. 1.2x mfMaxDistance) */
    float max_dist;       /* mfMaxDistance */
    int32_t id;           /* mnId: index into the frame's seen-stamp array (batched form) */
    int32_t n_obs;        /* MapPoint::Observations() (carried into the next last frame) */
    int32_t pad[2];
    uint8_t desc[32];     /* MapPoint::GetDescriptor */
} spslam_local_point;     /* 80 bytes */

typedef struct spslam_local_frame {
    float Tcw[16];        /* CurrentFrame.mTcw after the motion-model PoseOptimization */
    int32_t point_offset; /* local points [point_offset, point_offset + n_points) */
    int32_t n_points;
    int32_t seen_offset;  /* batched form with d_seen: point p is skipped when d_seen[seen_offset + p.id] == stamp */
    int32_t stamp;        /*   (mnLastFrameSeen == mCurrentFrame.mnId, Tracking.cc:1380-1395) */
} spslam_local_frame;     /* 80 bytes */

typedef struct spslam_local_params {
    float th;             /* 3 for RGB-D, 5 right after relocalisation (Tracking.cc:1416-1422) */
    float nn_ratio;       /* ORBmatcher mfNNratio (0.8) */
    float view_cos_limit; /* isInFrustum limit (0.5) */
    int32_t pad;
} spslam_local_params;

int spslam_search_local_points(spslam_ctx* ctx, const spslam_local_frame* frame, const spslam_local_point* points,
                               const spslam_keypoint* keys_un, const uint8_t* desc, const float* uright, int n_kp,
                               const int32_t* grid_off, const int32_t* grid_idx, const uint8_t* taken,
                               const spslam_local_params* params, int32_t* match, int* nmatches, uint8_t* in_view);

/* Batched, device resident, same current-frame layout as
 * spslam_search_by_projection_batch_device; d_taken at f*cap (may be NULL),
 * d_in_view at the points' global index (may be NULL).  d_seen (may be NULL):
 * the frames' seen stamps (spslam_local_frame.seen_offset / stamp; the
 * SPSLAM_TRACK_DISCARD stage writes them), so the local map can be passed
 * whole and the points the frame already tracks are skipped on the device. */
int spslam_search_local_points_batch_device(spslam_ctx* ctx, int n_frames, const spslam_local_frame* d_frames,
                                            const spslam_local_point* d_points, int max_points,
                                            const spslam_keypoint* d_keys_un, const uint8_t* d_desc,
                                            const float* d_uright, const int32_t* d_grid_off,
                                            const int32_t* d_grid_idx, const int* d_counts, int cap,
                                            const uint8_t* d_taken, const spslam_local_params* params,
                                            int32_t* d_match, int* d_nmatches, uint8_t* d_in_view,
                                            const int32_t* d_seen, void* hip_stream);

/* ---------------------------------------------------------------- LocalMapping: Fuse search, map-point refresh
 * The search half of ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>&
 * vpMapPoints, float th) (src/ORBmatcher.cc:842-949) as LocalMapping::
 * SearchInNeighbors calls it (src/LocalMapping.cc:466-546): per map point the
 * pre-checks, the projection into pKF, KeyFrame::GetFeaturesInArea
 * (src/KeyFrame.cc:586-625) and the best descriptor among the candidates that
 * pass Fuse's level and chi-square tests.  The map mutation that follows
 * (:951-971: Replace / AddObservation / AddMapPoint) stays with the caller, who
 * walks the results in point order; the reference fuses point i exactly when
 * best_dist <= TH_LOW (50), and d_nfused counts those.
 * CONTRACT: a map point occurs at most once in a problem's point range; then
 * the search of point i does not depend on the mutation done for the points
 * before it, and one call is one parallel search over a snapshot of the map.
 * The points are spslam_local_point records (the table SearchLocalPoints
 * reads); the keyframe is one slot of the frame stage's batch layouts.  The
 * caller's flag per point (isBad() || IsInKeyFrame(pKF), :849) skips it.
 * KeyFrame's image bounds are ints (include/KeyFrame.h:198-201): the configured
 * bounds are truncated as `mnMinX(F.mnMinX)` does. */
typedef struct spslam_fuse_problem {
    float Tcw[16];        /* pKF->GetPose(), row-major */
    int32_t kf_slot;      /* the keyframe's arrays: keys_un / uright / grid_idx at kf_slot*cap, desc at kf_slot*cap*32,
                             grid_off at kf_slot*(64*48+1), d_counts[kf_slot] keypoints */
    int32_t point_offset; /* vpMapPoints: spslam_local_point records [point_offset, point_offset + n_points) */
    int32_t n_points;
    int32_t out_offset;   /* result and skip flag of point i at out_offset + i */
} spslam_fuse_problem;    /* 80 bytes */

#define SPSLAM_FUSE_SEARCHED 0       /* vIndices not empty: best_idx / best_dist hold the loop's result */
#define SPSLAM_FUSE_SKIPPED 1        /* the caller's flag (:849) */
#define SPSLAM_FUSE_BEHIND 2         /* p3Dc.z < 0 (:856) */
#define SPSLAM_FUSE_OUTSIDE_IMAGE 3  /* !pKF->IsInImage(u, v) (:867), z == 0 included */
#define SPSLAM_FUSE_OUT_OF_RANGE 4   /* dist3D outside the scale invariance region (:878) */
#define SPSLAM_FUSE_VIEW_ANGLE 5     /* PO.dot(Pn) < 0.5 * dist3D (:884) */
#define SPSLAM_FUSE_NO_CANDIDATES 6  /* vIndices.empty() (:894) */

typedef struct spslam_fuse_result {
    int32_t best_idx;     /* keypoint of pKF, -1 when no candidate passed */
    int16_t best_dist;    /* 256 when none passed; the caller fuses when <= TH_LOW (50) */
    uint8_t level;        /* nPredictedLevel (0 when PredictScale was not reached) */
    uint8_t status;       /* SPSLAM_FUSE_* */
} spslam_fuse_result;     /* 8 bytes */

typedef struct spslam_fuse_params {
    float th;             /* radius at level 0 (Fuse's default 3.0, include/ORBmatcher.h:80) */
    int32_t pad;
} spslam_fuse_params;

/* Drop-in for one keyframe on host buffers: n_points points into the keyframe
 * (keys_un / desc / uright: n_kp keypoints, grid_off (64*48+1) / grid_idx: its
 * mGrid CSR).  skip: n_points flags, may be NULL.  results: n_points records;
 * *nfused receives Fuse's return value. */
int spslam_fuse_search(spslam_ctx* ctx, const float* Tcw, const spslam_local_point* points, int n_points,
                       const spslam_keypoint* keys_un, const uint8_t* desc, const float* uright, int n_kp,
                       const int32_t* grid_off, const int32_t* grid_idx, const uint8_t* skip,
                       const spslam_fuse_params* params, spslam_fuse_result* results, int* nfused);

/* Batched, device resident.  Problems may share a keyframe slot and may share
 * a point range; only their [out_offset, out_offset + n_points) ranges must be
 * disjoint.  d_skip (may be NULL) and d_results are indexed by out index;
 * max_points bounds every problem's n_points (host-known launch size);
 * d_nfused: one int per problem. */
int spslam_fuse_search_batch_device(spslam_ctx* ctx, int n_problems, const spslam_fuse_problem* d_problems,
                                    const spslam_local_point* d_points, int max_points,
                                    const spslam_keypoint* d_keys_un, const uint8_t* d_desc, const float* d_uright,
                                    const int32_t* d_grid_off, const int32_t* d_grid_idx, const int* d_counts,
                                    int cap, const uint8_t* d_skip, const spslam_fuse_params* params,
                                    spslam_fuse_result* d_results, int* d_nfused, void* hip_stream);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) and
 * MapPoint::UpdateNormalAndDepth (:330-371) for listed rows of the
 * spslam_local_point table, in place: desc, normal, min_dist, max_dist are
 * written; xw, id, n_obs and pad are not.  Several sequences' maps are packed
 * by the caller with absolute offsets and indices (no batch dimension).
 * Descriptor: observers in ascending keyframe order without those in bad
 * keyframes; per observer the element floor(0.5*(N-1)) of its sorted N
 * distances; the first observer with the strictly smallest one gives the
 * descriptor; none left: unchanged.  Normal and depth: every observer (bad
 * keyframes too: the reference does not check), float arithmetic, cv::norm
 * with the squares accumulated in double.
 * CONTRACT: a row occurs at most once in the row list. */
#define SPSLAM_POINT_MAX_OBS 128     /* observers per point; more: SPSLAM_REFRESH_CAPACITY, the record untouched */
#define SPSLAM_REFRESH_DESCRIPTOR 1
#define SPSLAM_REFRESH_NORMAL_DEPTH 2
#define SPSLAM_REFRESH_DONE 0
#define SPSLAM_REFRESH_UNTOUCHED 1   /* a bad point or a point without observers: both functions return early */
#define SPSLAM_REFRESH_CAPACITY 2

typedef struct spslam_point_refresh_map {
    const float* kf_Tcw;        /* n_kf * 16: KeyFrame::GetPose; the camera centre Ow = -Rcw^T tcw (KeyFrame.cc:82) is
                                   made on the device: three products summed in double in row order, negated, rounded */
    const int32_t* kf_slot;     /* n_kf: the keyframe's slot in d_keys_un (octave) / d_desc */
    const uint8_t* kf_bad;      /* n_kf, may be NULL */
    const int32_t* obs_off;     /* n_rows + 1 */
    const int32_t* obs_kf;      /* per row ascending keyframe index (std::map<KeyFrame*> order) */
    const int32_t* obs_kp;      /* that observation's keypoint index */
    const int32_t* ref_kf;      /* n_rows: mpRefKF; not among the row's observers: the first observer */
    const uint8_t* point_bad;   /* n_rows, may be NULL */
    spslam_local_point* points; /* the table */
} spslam_point_refresh_map;

/* Device resident: map's pointers, d_rows (n table rows), d_keys_un / d_desc at
 * slot*cap (the frame stage's layouts) and d_status (n, SPSLAM_REFRESH_*) are
 * device memory; what: a mask of SPSLAM_REFRESH_DESCRIPTOR / _NORMAL_DEPTH.
 * Scale factors and level count are the ORB tables'. */
int spslam_map_points_refresh_batch_device(spslam_ctx* ctx, const spslam_point_refresh_map* map,
                                           const int32_t* d_rows, int n, int what,
                                           const spslam_keypoint* d_keys_un, const uint8_t* d_desc, int cap,
                                           uint8_t* d_status, void* hip_stream);

/* The same on host arrays (map's pointers too): n_kf keyframes, n_rows table
 * rows, n_slots keyframe slots of cap keypoints.  map->points is rewritten in
 * place.  Returns SPSLAM_ERR_CAPACITY when a row reported
 * SPSLAM_REFRESH_CAPACITY (every other row is done and copied back). */
int spslam_map_points_refresh(spslam_ctx* ctx, const spslam_point_refresh_map* map, int n_kf, int n_rows,
                              const int32_t* rows, int n, int what, const spslam_keypoint* keys_un,
                              const uint8_t* desc, int cap, int n_slots, uint8_t* status);

/* ---------------------------------------------------------------- LocalMapping: CreateNewMapPoints
 * LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:219-464) for RGB-D:
 * ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-823 with
 * CheckDistEpipolarLine :140-157) and the per-match triangulation and checks
 * (:298-443).  One pair is (current keyframe, one neighbour).  The map mutation
 * (new MapPoint, AddObservation, AddMapPoint, the refresh :447-459) stays with
 * the caller, who walks the records in idx1 order; the device only marks the
 * has-point bytes so that the next neighbour's search skips what this one took.
 * F12 (ComputeF12, :548-565) is an input, as it is of SearchForTriangulation.
 * Camera, bf, mb = bf/fx, the scale factors and mvLevelSigma2 are the context's
 * (spslam_frame_configure); both keyframes share them (the reference reads the
 * current keyframe's mbf for the neighbour's right-image error, :418).
 * vbMatched2 of the reference is never written, so every key-1 feature is
 * searched on its own: it keeps the candidate of smallest distance among those
 * that pass every test, the later one in the node's list on a tie.
 * The 4x4 cv::SVD of :342 is not vendored with the reference; the null vector
 * here is a one-sided Jacobi with fixed order and double accumulators
 * (DESIGN.md 3.14), not bit-pinned to any OpenCV build.
 * PRECONDITIONS: uright[i] >= 0 implies depth[i] > 0 (KeyFrame::UnprojectStereo
 * returns an empty Mat otherwise and the reference reads it).  A FeatureVector
 * lists a feature in at most one node, as DBoW2 makes it, so that it holds at
 * most `counts` entries; of a malformed one that lists more than cap entries
 * the search takes cap of them and drops the rest without an error. */
typedef struct spslam_tri_side {     /* frame-stage / bow batch layouts, slot s at s*cap (fv_start at s*(cap+1)) */
    const spslam_keypoint* keys;     /* mvKeys   (UnprojectStereo) */
    const spslam_keypoint* keys_un;  /* mvKeysUn */
    const float* uright;
    const float* depth;
    const uint8_t* desc;             /* s*cap*32 */
    uint8_t* has_point;              /* GetMapPoint(i) != NULL; written when mark != 0 */
    const int* counts;
    const uint32_t* fv_nodes;
    const int32_t* fv_start;
    const int32_t* fv_features;
    const int* n_fv;
    int32_t cap;                     /* 1 .. 8192 */
    int32_t pad;
} spslam_tri_side;

typedef struct spslam_tri_pair {     /* one (current keyframe, neighbour) */
    int32_t kf1, kf2;                /* slots */
    float Tcw1[12], Tcw2[12];        /* [R | t], 3x4 row-major */
    float Ow1[3], Ow2[3];            /* GetCameraCenter() */
    float F12[9];
    int32_t out_offset;              /* records; match12 at the same offset */
    int32_t flags;                   /* bit 0: skip (caller's baseline / CheckNewKeyFrames decision) */
} spslam_tri_pair;                   /* 172 bytes */
#define SPSLAM_TRI_PAIR_SKIP 1

#define SPSLAM_TRI_NEW 0             /* triangulation is successful (:443): the caller creates the MapPoint */
#define SPSLAM_TRI_NO_MATCH 1        /* match12 < 0 */
#define SPSLAM_TRI_LOW_PARALLAX 2    /* no stereo and very low parallax (:360) */
#define SPSLAM_TRI_W_ZERO 3          /* x3D(3) == 0 (:345) */
#define SPSLAM_TRI_BEHIND_1 4        /* z1 <= 0 (:367) */
#define SPSLAM_TRI_BEHIND_2 5        /* z2 <= 0 (:371) */
#define SPSLAM_TRI_REPROJ_1 6        /* 5.991 / 7.8 sigma2 in the current keyframe (:386, :397) */
#define SPSLAM_TRI_REPROJ_2 7        /* the same in the neighbour (:412, :423) */
#define SPSLAM_TRI_ZERO_DIST 8       /* dist1 == 0 || dist2 == 0 (:433) */
#define SPSLAM_TRI_SCALE 9           /* scale consistency (:441) */
#define SPSLAM_TRI_FROM_SVD 0
#define SPSLAM_TRI_FROM_STEREO_1 1
#define SPSLAM_TRI_FROM_STEREO_2 2

typedef struct spslam_tri_result {
    float x, y, z;        /* x3D at the exit (0 where none was made) */
    int32_t idx2;         /* match12 of this key-1 feature */
    uint8_t status;       /* SPSLAM_TRI_* */
    uint8_t source;       /* SPSLAM_TRI_FROM_* */
    uint16_t pad;
} spslam_tri_result;      /* 20 bytes */

#define SPSLAM_TRI_PAIR_SEARCHED 0
#define SPSLAM_TRI_PAIR_SKIPPED 1          /* flags bit 0 */
#define SPSLAM_TRI_PAIR_SHORT_BASELINE 2   /* baseline < mb (:263) */

/* Batched, device resident.  Pair p writes match12 of key-1 feature i < counts[kf1]
 * at d_match12[out_offset + i] (-1: none) and d_nmatches[p]; nothing else is
 * written.  A pair with the skip flag gives -1 everywhere and 0.  The out ranges
 * of the pairs must be disjoint; the pairs may share slots (nothing is marked). */
int spslam_search_for_triangulation_batch_device(spslam_ctx* ctx, int n_pairs, const spslam_tri_pair* d_pairs,
                                                 const spslam_tri_side* side, int only_stereo,
                                                 int check_orientation, int32_t* d_match12, int* d_nmatches,
                                                 void* hip_stream);

/* One record per key-1 feature at d_results[out_offset + i], d_n_new[p] = the
 * number of SPSLAM_TRI_NEW.  mark != 0: has_point[idx1] of kf1 and
 * has_point[idx2] of kf2 are set to 1 for every SPSLAM_TRI_NEW record; then
 * the pairs of one call must not share a keyframe slot. */
int spslam_triangulate_batch_device(spslam_ctx* ctx, int n_pairs, const spslam_tri_pair* d_pairs,
                                    const spslam_tri_side* side, const int32_t* d_match12, int mark,
                                    spslam_tri_result* d_results, int* d_n_new, void* hip_stream);

/* One neighbour round of CreateNewMapPoints for n_pairs sequences: the baseline
 * test (:258-264, from Ow1 / Ow2), the search (ORBmatcher(0.6, false): both
 * stereo and mono, no orientation check) and the triangulation with mark = 1.
 * d_pair_status[p]: SPSLAM_TRI_PAIR_*; a pair that is not SEARCHED gives
 * SPSLAM_TRI_NO_MATCH records.  RULE: the pairs of one call must not share a
 * keyframe slot.  Calls on one stream are ordered, so round i+1 sees round i's
 * marks without a host round trip. */
int spslam_create_new_points_batch_device(spslam_ctx* ctx, int n_pairs, const spslam_tri_pair* d_pairs,
                                          const spslam_tri_side* side, int32_t* d_match12, int* d_nmatches,
                                          spslam_tri_result* d_results, int* d_n_new, uint8_t* d_pair_status,
                                          void* hip_stream);

/* Host arrays of one keyframe for the drop-ins below. */
typedef struct spslam_tri_keyframe {
    const spslam_keypoint* keys;
    const spslam_keypoint* keys_un;
    const float* uright;
    const float* depth;
    const uint8_t* desc;
    const uint8_t* has_point;
    const uint32_t* fv_nodes;
    const int32_t* fv_start;        /* n_fv + 1 */
    const int32_t* fv_features;
    int32_t n, n_fv;
    float Tcw[12], Ow[3];
    int32_t pad;
} spslam_tri_keyframe;

/* Drop-in for ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs,
 * bOnlyStereo): matched_pairs receives (idx1, idx2) in idx1 order (room for
 * kf1->n pairs); returns nmatches, or a negative SPSLAM_ERR_*. */
int spslam_search_for_triangulation(spslam_ctx* ctx, const spslam_tri_keyframe* kf1, const spslam_tri_keyframe* kf2,
                                    const float* F12, int32_t* matched_pairs, int only_stereo,
                                    int check_orientation);

/* :298-443 for n_matches pairs (idx1 distinct): results[k] is pair k's record;
 * *n_new the number of SPSLAM_TRI_NEW.  Nothing is marked. */
int spslam_triangulate(spslam_ctx* ctx, const spslam_tri_keyframe* kf1, const spslam_tri_keyframe* kf2,
                       const int32_t* matched_pairs, int n_matches, spslam_tri_result* results, int* n_new);

/* ---------------------------------------------------------------- LocalMapping: covisibility graph, the cullings
 * KeyFrame::UpdateConnections (src/KeyFrame.cc:306-396) with AddConnection
 * (:128-141) and UpdateBestCovisibles (:143-162); LocalMapping::KeyFrameCulling
 * (src/LocalMapping.cc:644-711, RGB-D branch) and LocalMapping::MapPointCulling
 * (:182-217).  Index work on the tables spslam_local_map and
 * spslam_point_refresh_map define.  Keyframe indices and point rows are local to
 * a sequence: keyframe k of a problem is entry kf_base + k of the keyframe
 * tables, row r is entry row_base + r of the point tables, so many sequences
 * share one call.  Keyframes are walked in ascending index where the reference
 * has pointer order, as everywhere at this ABI; index 0 of a sequence is
 * mnId == 0.  The device forms trust their tables: every index must lie inside
 * its table (the host forms check them). */
typedef struct spslam_covis_map {
    const int32_t* match_off;   /* CSR (keyframes + 1), absolute offsets into match_row */
    const int32_t* match_row;   /* GetMapPointMatches in keypoint order: the point's row or -1 */
    const int32_t* obs_off;     /* CSR (rows + 1), absolute offsets */
    const int32_t* obs_kf;      /* observer keyframes, ascending (MapPoint::GetObservations) */
    const int32_t* obs_kp;      /* that observation's keypoint index (KeyFrameCulling only) */
    const int32_t* kf_slot;     /* per keyframe: its slot in d_keys_un / d_uright / d_depth (KeyFrameCulling only) */
    const uint8_t* point_bad;   /* MapPoint::isBad (may be NULL: none) */
    const spslam_local_point* points;  /* n_obs = MapPoint::Observations() (the cullings only) */
} spslam_covis_map;

/* The binding's mirror of the reference's covisibility members, device resident
 * and persistent across calls.  Keyframe k's rows are at (kf_base + k) * stride. */
typedef struct spslam_covis_graph {
    int32_t* weights;           /* stride per keyframe: mConnectedKeyFrameWeights by keyframe index, 0 = absent */
    int32_t* ordered;           /* stride per keyframe: mvpOrderedConnectedKeyFrames; entries past n_ordered are kept */
    int32_t* ordered_w;         /* stride per keyframe: mvOrderedWeights */
    int32_t* n_ordered;         /* per keyframe */
    int32_t* covis;             /* 10 per keyframe: GetBestCovisibilityKeyFrames(10), -1 padded: spslam_local_map.covis.
                                   Rewritten whenever that keyframe's ordered list is rewritten */
    int32_t* parent;            /* per keyframe: mpParent, -1 = none: spslam_local_map.parent */
    uint8_t* first_connection;  /* per keyframe: mbFirstConnection */
    int32_t stride;             /* >= every problem's n_kf */
    int32_t pad;
} spslam_covis_graph;

typedef struct spslam_covis_problem {
    int32_t kf_base, row_base;
    int32_t kf;                 /* the keyframe whose UpdateConnections runs / mpCurrentKeyFrame of the culling */
    int32_t n_kf;               /* keyframes of this sequence, 1 .. 1024 */
} spslam_covis_problem;         /* 16 bytes */

#define SPSLAM_COVIS_MAX_KF 1024
#define SPSLAM_COVIS_BEST 10         /* entries of covis per keyframe */
#define SPSLAM_COVIS_UPDATED 0
#define SPSLAM_COVIS_EMPTY 1         /* KFcounter.empty() (:340): nothing of the graph is written */

typedef struct spslam_covis_result {
    int32_t status;             /* SPSLAM_COVIS_* */
    int32_t n_ordered;          /* the keyframe's ordered list after the call (EMPTY: 0, the list itself is kept) */
    int32_t new_parent;         /* mpParent set by the first connection (:388-393), -1: none set.  AddChild stays
                                   with the caller: it appends kf to new_parent's children */
    int32_t n_resorted;         /* selected keyframes whose weight changed, i.e. UpdateBestCovisibles ran */
} spslam_covis_result;          /* 16 bytes */

/* UpdateConnections of problem p's keyframe, one workgroup per problem:
 *   counts (:319-337): every match row of kf that is not -1 and not bad adds one to each of its observers but kf;
 *   all zero (:340): SPSLAM_COVIS_EMPTY;
 *   selection (:345-369): every keyframe with count >= th (the reference's 15); none: the first strict maximum in
 *     ascending index;
 *   kf's own state (:384-386): its whole weights row becomes the counts (those below th too), its ordered list the
 *     selected keyframes by weight descending, the higher index first on equal weight (sort, then push_front);
 *   every selected keyframe j (AddConnection): weights[j][kf] already equal to the count: nothing of j changes.
 *     Otherwise it is written and j's ordered list is rebuilt from every non-zero entry of its row, in the same
 *     order (UpdateBestCovisibles): that brings in entries below th which j's own UpdateConnections left out;
 *   first connection (:388-393): first_connection[kf] set and kf != 0: parent[kf] = ordered[kf][0], flag cleared.
 * CONTRACT: a call holds at most one problem per sequence (a problem writes other keyframes' rows).  Several
 * keyframes of one sequence are successive calls on one stream. */
int spslam_covis_update_connections_batch_device(spslam_ctx* ctx, int n_problems,
                                                 const spslam_covis_problem* d_problems,
                                                 const spslam_covis_map* map, const spslam_covis_graph* graph, int th,
                                                 spslam_covis_result* d_results, void* hip_stream);

/* One problem on host arrays (map's and graph's pointers too) at bases 0: n_kf keyframes, n_rows point rows.  The
 * graph arrays are rewritten in place.  map: obs_kp, kf_slot and points are not read. */
int spslam_covis_update_connections(spslam_ctx* ctx, const spslam_covis_map* map, int n_kf, int n_rows, int kf, int th,
                                    const spslam_covis_graph* graph, spslam_covis_result* result);

/* KeyFrameCulling for problem p's current keyframe, one workgroup per problem.  The candidates are the keyframe's
 * ordered list in the graph (GetVectorCovisibleKeyFrames), read once at the start and taken in order:
 *   new_plane[kf] set (:650): problem status SPSLAM_CULL_NEW_PLANE, no candidates;
 *   candidate index 0 or new_plane[c] set (:658): SPSLAM_CULL_SKIPPED;
 *   otherwise, over its keypoints with a row that is not (effectively) bad: depth > th_depth || depth < 0: not
 *     counted; n_mps++; effective Observations() > th_obs: the observers other than c and not culled earlier in this
 *     call whose octave at their obs_kp is <= this keypoint's octave + 1 are counted, th_obs or more make the
 *     keypoint redundant;
 *   verdict: (double)n_redundant > 0.9 * (double)n_mps;
 *   a culled candidate with not_erase set: SPSLAM_CULL_DEFERRED (mbToBeErased, KeyFrame.cc:476-480), nothing
 *     changes for later candidates; any other culled candidate: SPSLAM_CULL_CULLED, and it joins the call's
 *     culled set.
 * "Effective" carries KeyFrame::SetBadFlag's EraseObservation loop (KeyFrame.cc:486-488, MapPoint.cc:111-137)
 * forward without writing the map: a point's Observations() is n_obs minus, per observer in the culled set, 2 when
 * that observation's uright >= 0 and else 1; the point is bad when point_bad says so, or when it has a culled
 * observer and that value is <= 2.
 * CONTRACT: the match rows and the observer lists agree with each other; a keyframe's match list is no longer than
 * cap.  Nothing of the map or the graph is written: the caller applies SetBadFlag to the culled ones in order. */
#define SPSLAM_CULL_KEPT 0
#define SPSLAM_CULL_CULLED 1
#define SPSLAM_CULL_DEFERRED 2
#define SPSLAM_CULL_SKIPPED 3
#define SPSLAM_CULL_RAN 0            /* problem status */
#define SPSLAM_CULL_NEW_PLANE 1      /* problem status */

typedef struct spslam_cull_problem {
    int32_t kf_base, row_base;
    int32_t kf;                 /* mpCurrentKeyFrame */
    int32_t n_kf;               /* 1 .. 1024 */
    int32_t out_offset;         /* candidate q's record at d_records[out_offset + q] */
    int32_t pad[3];
} spslam_cull_problem;          /* 32 bytes */

typedef struct spslam_cull_record {
    int32_t kf;                 /* the candidate */
    int32_t n_mps;              /* nMPs */
    int32_t n_redundant;        /* nRedundantObservations */
    int32_t status;             /* SPSLAM_CULL_KEPT / CULLED / DEFERRED / SKIPPED */
} spslam_cull_record;           /* 16 bytes */

typedef struct spslam_cull_summary {
    int32_t n_candidates;       /* records written */
    int32_t status;             /* SPSLAM_CULL_RAN / SPSLAM_CULL_NEW_PLANE */
} spslam_cull_summary;

typedef struct spslam_cull_params {
    float th_depth;             /* mThDepth */
    int32_t th_obs;             /* thObs (3) */
} spslam_cull_params;

/* d_keys_un / d_uright / d_depth: the frame stage's layouts, slot s at s * cap.  d_new_plane: one byte per keyframe
 * (mbNewPlane); d_not_erase: one byte per keyframe (mbNotErase), may be NULL.  Only graph->ordered, n_ordered and
 * stride are read. */
int spslam_keyframe_culling_batch_device(spslam_ctx* ctx, int n_problems, const spslam_cull_problem* d_problems,
                                         const spslam_covis_map* map, const spslam_covis_graph* graph,
                                         const spslam_keypoint* d_keys_un, const float* d_uright, const float* d_depth,
                                         int cap, const uint8_t* d_new_plane, const uint8_t* d_not_erase,
                                         const spslam_cull_params* params, spslam_cull_record* d_records,
                                         spslam_cull_summary* d_summaries, void* hip_stream);

/* One problem on host arrays at bases 0: n_kf keyframes, n_rows rows, n_slots keyframe slots of cap keypoints;
 * ordered / n_ordered: the current keyframe's list.  records: room for n_ordered entries. */
int spslam_keyframe_culling(spslam_ctx* ctx, const spslam_covis_map* map, int n_kf, int n_rows, int kf,
                            const int32_t* ordered, int n_ordered, const spslam_keypoint* keys_un, const float* uright,
                            const float* depth, int cap, int n_slots, const uint8_t* new_plane,
                            const uint8_t* not_erase, const spslam_cull_params* params, spslam_cull_record* records,
                            spslam_cull_summary* summary);

/* MapPointCulling: per entry k of mlpRecentAddedMapPoints (rows[k], an absolute row of the point tables) the first
 * branch of :198-215 that holds, with cur_kf_id[k] = mpCurrentKeyFrame->mnId of the entry's sequence.  Applying the
 * verdicts (SetBadFlag, erase from the list) stays with the caller. */
#define SPSLAM_POINT_CULL_KEEP 0
#define SPSLAM_POINT_CULL_DROP 1        /* isBad(): erased from the list only */
#define SPSLAM_POINT_CULL_BAD_RATIO 2   /* (float)mnFound / mnVisible < 0.25f */
#define SPSLAM_POINT_CULL_BAD_OBS 3     /* id difference >= 2 and Observations() <= th_obs */
#define SPSLAM_POINT_CULL_EXPIRED 4     /* id difference >= 3 */

typedef struct spslam_point_cull_map {  /* per point row */
    const int32_t* found;       /* mnFound */
    const int32_t* visible;     /* mnVisible */
    const int32_t* first_kf;    /* mnFirstKFid */
    const uint8_t* point_bad;   /* may be NULL */
    const spslam_local_point* points;  /* n_obs */
} spslam_point_cull_map;

int spslam_map_point_culling_batch_device(spslam_ctx* ctx, const spslam_point_cull_map* map, const int32_t* d_rows,
                                          const int32_t* d_cur_kf_id, int n, int th_obs, uint8_t* d_verdict,
                                          void* hip_stream);

/* The same on host arrays of n_rows rows; cur_kf_id: one id for the whole list. */
int spslam_map_point_culling(spslam_ctx* ctx, const spslam_point_cull_map* map, int n_rows, const int32_t* rows, int n,
                             int cur_kf_id, int th_obs, uint8_t* verdict);

/* ---------------------------------------------------------------- input images
 * Tracking::GrabImageRGBD's image preparation (src/Tracking.cc:208-229), the
 * first kernel of a step:
 *   gray  = cvtColor(imRGB, RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY by
 *           channels and mbRGB), OpenCV's 8U fixed point
 *           (R*4899 + G*9617 + B*1868 + 8192) >> 14; a 1-channel image is copied;
 *   depth = imD.convertTo(CV_32F, mDepthMapFactor) when the factor is not 1 or
 *           the depth is not CV_32F: float(d) * (float)factor; else copied.
 * mDepthMapFactor is the reciprocal of the YAML DepthMapFactor (Tracking.cc:142-146),
 * i.e. depth_scale = 1.0f / 5000.0f for TUM. */
typedef struct spslam_grab_params {
    int32_t channels;     /* 1, 3 or 4 (interleaved u8) */
    int32_t rgb;          /* mbRGB: 1 = R,G,B(,A) order, 0 = B,G,R(,A) */
    int32_t depth_u16;    /* 1 = CV_16U depth, 0 = CV_32F */
    float depth_scale;    /* mDepthMapFactor */
} spslam_grab_params;

/* Drop-in for one frame on host buffers: color (row stride color_stride bytes),
 * depth (row stride depth_stride elements); gray (w*h u8) and depth_out (w*h f32) dense. */
int spslam_grab_rgbd(spslam_ctx* ctx, const uint8_t* color, int color_stride, const void* depth, int depth_stride,
                     int w, int h, const spslam_grab_params* params, uint8_t* gray, float* depth_out);

/* Batched, device resident: frame f's color at d_color + f * color_frame_stride bytes,
 * depth at d_depth + f * depth_frame_stride elements; outputs dense, frame f at
 * d_gray + f*w*h and d_depth_out + f*w*h (the ORB / plane batch layouts). */
int spslam_grab_rgbd_batch_device(spslam_ctx* ctx, int n_frames, const uint8_t* d_color, size_t color_frame_stride,
                                  int color_stride, const void* d_depth, size_t depth_frame_stride, int depth_stride,
                                  int w, int h, const spslam_grab_params* params, uint8_t* d_gray, float* d_depth_out,
                                  void* hip_stream);

/* Fusion with the plane stage (no reference counterpart: Frame::ComputePlanesFromOrganizedPointCloud,
 * Frame.cc:857-874, samples the converted depth a second time).  With enable = 1 and
 * spslam_planes_configure called on the same context for the same image size, a
 * spslam_grab_rgbd_batch_device call also writes the organized cloud of its depth output into the
 * selected cloud set (spslam_planes_select_cloud_set) and tags the set with that depth output; the
 * set's next spslam_planes_extract_batch_device over exactly that depth (same pointer, dense layout,
 * no more frames) uses the cloud as it is instead of sampling the depth again (bit-identical cloud),
 * and clears the tag.  Any other extraction makes its own cloud.  The caller orders the grab before
 * the extraction (same stream or an event), as it already must for the depth.  Default 0: in the
 * pipelined batch step the grab is on the ORB stream's critical path and the fused pass measured 2 %
 * slower than a separate cloud kernel on the plane stream (profiles/r06/ab_grab_cloud_c2.txt); the
 * environment variable SPSLAM_GRAB_CLOUD=1 makes 1 the default. */
int spslam_grab_fuse_cloud(spslam_ctx* ctx, int enable);

/* ---------------------------------------------------------------- tracking graph glue
 * The Tracking-side bookkeeping between matching / plane association and
 * PoseOptimization, on the device, for a batch of frames (one stage per call):
 *
 * SPSLAM_TRACK_MOTION_MODEL -- TrackWithMotionModel's graph (src/Tracking.cc:
 *   951-981): mvpMapPoints[i] = the SearchByProjection match of keypoint i,
 *   mvpMapPlanes / mvpParallelPlanes / mvpVerticalPlanes = the first
 *   AssociatePlanesByBoundary; then Optimizer::PoseOptimization's edge loops
 *   (src/Optimizer.cc:561-640: one point edge per keypoint with a map point, in
 *   keypoint order, stereo iff mvuRight >= 0, information mvInvLevelSigma2
 *   [octave]; :681-860: plane edges over the frame planes in index order, then
 *   parallel, then vertical).  The initial pose is the motion-model prediction
 *   (proj_frames[f].Tcw).  edge_of_kp[i] receives keypoint i's edge index.
 * SPSLAM_TRACK_DISCARD -- the outlier discard after that PoseOptimization
 *   (src/Tracking.cc:986-1000: mvpMapPoints[i] = NULL where mvbOutlier[i];
 *   :1004-1028: mvpMapPlanes / mvpParallelPlanes / mvpVerticalPlanes[i] = NULL
 *   where the plane / parallel / vertical edge is an outlier -- written to
 *   next_match / next_parallel / next_vertical, the starting state of the
 *   second association (spslam_assoc_frame.carry), when those are given) and
 *   the SearchLocalPoints preconditions: taken[i] = keypoint i keeps a map point
 *   with Observations() > 0 (src/ORBmatcher.cc:95-97); the optimized pose is
 *   written into local_frames[f].Tcw and, if given, assoc_frames_next[f].Tcw
 *   (the second association runs at that pose, src/Tracking.cc:1066).
 *   With `seen` given it also stamps every map point the motion model matched
 *   (inliers and discarded outliers both get mnLastFrameSeen = the frame,
 *   Tracking.cc:997 and :1380-1390): seen[local_frames[f].seen_offset + id] =
 *   local_frames[f].stamp, which spslam_search_local_points_batch_device skips.
 * SPSLAM_TRACK_LOCAL_MAP -- TrackLocalMap's graph (src/Tracking.cc:1062-1068):
 *   mvpMapPoints = the surviving motion-model points, replaced by the
 *   SearchLocalPoints match where it assigned one (it may re-assign a keypoint
 *   whose point has no observations, src/ORBmatcher.cc:115); planes from the
 *   second association; initial pose = the motion-model result.
 *
 * Layouts: current frame f's keypoints / mvuRight / matches / taken /
 * edge_of_kp at f * cap (ORB and frame-stage batch layout); match indices are
 * relative to the frame's proj / local point_offset; plane association outputs
 * at f * (cap_a + cap_b) + i (spslam_planes_associate_batch_device layout) are
 * global map-plane indices.  The graphs are written with point_offset = f * cap
 * and plane_offset = f * 3 * (cap_a + cap_b), so the PoseOptimization outlier
 * flags of frame f are at the same offsets.  The motion model's failure test and the switch to
 * TrackReferenceKeyFrame: spslam_track_refkf_batch_device below; relocalisation is the caller's.
 *
 * Frame-to-frame state of a tracked sequence (Tracking::Track, src/Tracking.cc:
 * 443-505, TrackWithMotionModel :956-958), for batches that are consecutive
 * frames of their sequences:
 * SPSLAM_TRACK_MOTION_PRIOR -- mCurrentFrame.SetPose(mVelocity * mLastFrame.mTcw):
 *   proj_frames[f].Tcw = velocity[f] (4x4 row-major float) * proj_frames[f].Tlw
 *   (cv::Mat float product), also into assoc_frames_first[f].Tcw when given.
 *   The reference re-derives mLastFrame.mTcw through its reference keyframe
 *   (UpdateLastFrame, Tlr * Tref) first; with fixed keyframe poses that is the
 *   last pose up to float rounding, and is not restated.
 * SPSLAM_TRACK_LAST_FRAME -- after the local-map PoseOptimization (results /
 *   point_outlier = that optimisation's): mVelocity = mTcw * LastTwc (LastTwc =
 *   [Rlw^T | -Rlw^T tlw] of proj_frames[f].Tlw), the VO-match clean-up (points
 *   with Observations() < 1 dropped, :456-466) and the outlier drop (:484-488);
 *   the surviving map points (local-map match, else the kept motion-model
 *   match), in keypoint order, become the next frame's last-frame points:
 *   next_points at f * cap (xw, mvKeysUn angle, octave, n_obs, id, descriptor),
 *   next_frames[f] = {Tlw = mTcw, point_offset = f * cap, n_points}, velocity[f]. */
#define SPSLAM_TRACK_MOTION_MODEL 0
#define SPSLAM_TRACK_DISCARD 1
#define SPSLAM_TRACK_LOCAL_MAP 2
#define SPSLAM_TRACK_MOTION_PRIOR 3
#define SPSLAM_TRACK_LAST_FRAME 4

typedef struct spslam_track_batch {
    /* current frames */
    const spslam_keypoint* keys_un;  /* mvKeysUn */
    const float* uright;             /* mvuRight */
    const int* kp_counts;
    int32_t cap;
    /* motion model: last-frame map points and the SearchByProjection matches */
    const spslam_proj_frame* proj_frames;
    const spslam_proj_point* proj_points;
    const int32_t* proj_match;
    /* local map: SearchLocalPoints inputs / matches */
    spslam_local_frame* local_frames;     /* DISCARD writes Tcw */
    const spslam_local_point* local_points;
    const int32_t* local_match;           /* LOCAL_MAP */
    uint8_t* taken;                       /* DISCARD writes */
    /* frame planes (extracted, then supposed) and their association */
    const void* planes_a;
    const void* planes_b;
    const int* count_a;
    const int* count_b;
    int32_t stride_a, stride_b, cap_a, cap_b;
    const spslam_map_plane* map;
    const int32_t* assoc_match;
    const int32_t* assoc_parallel;
    const int32_t* assoc_vertical;
    spslam_assoc_frame* assoc_frames_next;  /* DISCARD writes Tcw (may be NULL) */
    const uint8_t* plane_outlier;           /* motion-model plane edge outlier flags (DISCARD, with next_*) */
    int32_t* next_match;                    /* DISCARD writes the surviving associations (may be NULL) */
    int32_t* next_parallel;
    int32_t* next_vertical;
    /* sequence state (MOTION_PRIOR, DISCARD stamps, LAST_FRAME) */
    spslam_assoc_frame* assoc_frames_first;  /* MOTION_PRIOR writes Tcw (may be NULL) */
    int32_t* seen;                        /* DISCARD stamps (may be NULL) */
    spslam_proj_frame* next_frames;       /* LAST_FRAME writes */
    spslam_proj_point* next_points;       /* LAST_FRAME writes, f * cap */
    float* velocity;                      /* 16 floats per frame: MOTION_PRIOR reads, LAST_FRAME writes */
    const uint8_t* point_outlier_local;   /* LAST_FRAME: the local-map PoseOptimization's point outlier flags */
    /* PoseOptimization graphs */
    spslam_pose_problem* problems;
    spslam_point_obs* points;             /* f * cap */
    spslam_plane_obs* planes;             /* f * 3 * (cap_a + cap_b) */
    int32_t* edge_of_kp;                  /* MOTION_MODEL writes, DISCARD / LOCAL_MAP read */
    const spslam_pose_result* results;    /* the motion-model PoseOptimization (DISCARD, LOCAL_MAP) */
    const uint8_t* point_outlier;         /* its point outlier flags (DISCARD, LOCAL_MAP) */
    float fx, fy, cx, cy, bf;
    int32_t pad;
} spslam_track_batch;

int spslam_track_graph_batch_device(spslam_ctx* ctx, int n_frames, int stage, const spslam_track_batch* batch,
                                    void* hip_stream);

/* TrackWithMotionModel's failure and the switch to TrackReferenceKeyFrame (src/Tracking.cc:318-324: bOK =
 * TrackWithMotionModel(); if (!bOK) bOK = TrackReferenceKeyFrame()), batched.  The motion model fails when
 * SearchByProjection (after the 2*th retry) finds fewer than 10 matches (:977, before the association and
 * PoseOptimization) or when fewer than 5 map points / map planes survive its discard (nmatchesMap, :986-1053).
 * For the frames that fail a caller runs ComputeBoW + SearchByBoW against the reference keyframe
 * (spslam_bow_transform_batch_device / spslam_search_by_bow_batch_device, :796-806); where that finds at least 10
 * matches the frame is re-tracked from the last frame's pose -- association, MOTION_MODEL graph, PoseOptimization
 * and DISCARD over the reference keyframe's map points (:808-882) -- into separate buffers that
 * spslam_masked_frame_copy_device then moves over the motion model's.
 *   SPSLAM_REFKF_PREPARE (after the motion model's DISCARD; mm = its spslam_track_batch): fallback[f], and
 *     refkf_counts[f] = kp_counts[f] where it failed, else 0 (the BoW transform's counts: it skips the others).
 *   SPSLAM_REFKF_SELECT (after SearchByBoW): apply[f] = fallback[f] && bow_nmatches[f] >= 10 (:806);
 *     state[f] = 0 (motion model), 1 (reference keyframe) or 2 (both failed: LOST, the motion model's result is
 *     kept); refkf_match = the BoW matches as rows of the keyframe's point set (-1 elsewhere and where !apply);
 *     refkf_frames[f] = {Tcw = Tlw = proj_frames[f].Tlw (SetPose(mLastFrame.mTcw)), point_offset / n_points =
 *     refkf_sets[2 f], [2 f + 1] (the keyframe's map points inside proj_points), 0 points where !apply};
 *     refkf_assoc[f] = assoc_frames[f] at Tcw = Tlw, n_map = 0 where !apply, carry = 1 (the association starts
 *     from the motion model's surviving planes, which the caller copies into its association arrays) unless the
 *     motion model stopped before associating (< 10 matches: carry = 0); and the seen stamps: the motion model's
 *     DISCARD stamped every one of its matches (mnLastFrameSeen); where the keyframe takes over only its discarded
 *     outliers keep the stamp (:990-997; none when it stopped at < 10 matches), the others get stamp - 1. */
#define SPSLAM_REFKF_PREPARE 0
#define SPSLAM_REFKF_SELECT 1

typedef struct spslam_refkf_batch {
    const int32_t* nmatches;                 /* SearchByProjection's count after the retry, per frame */
    uint8_t* fallback;                       /* PREPARE writes: the motion model failed */
    int32_t* refkf_counts;                   /* PREPARE writes */
    const int32_t* bow_nmatches;             /* SELECT: SearchByBoW's count per frame */
    const int32_t* bow_match;                /* SELECT: SearchByBoW's keyframe feature per keypoint (cap per frame) */
    const int32_t* refkf_rows;               /* SELECT: per keyframe feature its map point's row in the keyframe's
                                                point set or -1 (rows_stride per keyframe) */
    const int32_t* refkf_index;              /* SELECT: each frame's keyframe (row block of refkf_rows) */
    int32_t rows_stride, pad;
    const int32_t* refkf_sets;               /* SELECT: (point_offset, n_points) per frame */
    const spslam_assoc_frame* assoc_frames;  /* SELECT: the motion model's first-association frames */
    uint8_t* apply;                          /* SELECT writes */
    int8_t* state;                           /* SELECT writes (may be NULL) */
    int32_t* refkf_match;                    /* SELECT writes (cap per frame) */
    spslam_proj_frame* refkf_frames;         /* SELECT writes */
    spslam_assoc_frame* refkf_assoc;         /* SELECT writes */
} spslam_refkf_batch;

int spslam_track_refkf_batch_device(spslam_ctx* ctx, int n_frames, int stage, const spslam_track_batch* mm,
                                    const spslam_refkf_batch* rk, void* hip_stream);

/* The reference keyframe TrackReferenceKeyFrame uses (mpReferenceKF), per frame, batched.  TrackLocalMap's
 * UpdateLocalKeyFrames sets it to pKFmax, the keyframe that observes the most of the frame's map points after
 * TrackWithMotionModel's (or TrackReferenceKeyFrame's) discard, first maximum in keyframe order (src/Tracking.cc:
 * 1459-1570; the reference iterates a std::map<KeyFrame*, int> in pointer order: keyframe id order here, as
 * everywhere at this ABI); it is not run on a LOST frame (:406-409); CreateNewKeyFrame then makes the new keyframe
 * the reference (:1258).  mm = the first graph's spslam_track_batch after the discard (and after the masked copy
 * of a TrackReferenceKeyFrame re-tracking): the frame's map points are proj_points[point_offset +
 * proj_match[i]] for every keypoint i with an edge that is not an outlier; a point's keyframe is id / ids_per_kf
 * (each map point counted for the keyframe that created it).  Writes refkf_index[f] (kept where LOST or where no
 * map point remains: pKFmax stays NULL), refkf_sets[2 f .. 2 f + 1] = kf_sets of it and, when refkf_pairs is
 * given, the (keyframe, frame) pair of spslam_search_by_bow_batch_device. */
typedef struct spslam_refkf_vote {
    const int32_t* kf_base;     /* per frame: the index of its sequence's keyframe 0 in the keyframe tables */
    const int32_t* kf_sets;     /* per keyframe: (point_offset, n_points) of its map points inside proj_points */
    int32_t ids_per_kf;         /* map point id / ids_per_kf = the keyframe (of the sequence) that created it */
    int32_t n_kf;               /* keyframes per sequence, 1 .. 1024 */
    int32_t new_kf;             /* >= 0: the frames become keyframe new_kf of their sequence (CreateNewKeyFrame) */
    int32_t pad;
    const int8_t* state;        /* per frame: 2 = LOST (spslam_refkf_batch.state); may be NULL */
    int32_t* refkf_index;       /* in / out: each frame's reference keyframe (kf_base + its keyframe) */
    int32_t* refkf_sets;        /* out: (point_offset, n_points) of it */
    int32_t* refkf_pairs;       /* out (may be NULL): (refkf_index, f) */
} spslam_refkf_vote;

int spslam_track_refkf_vote_batch_device(spslam_ctx* ctx, int n_frames, const spslam_track_batch* mm,
                                         const spslam_refkf_vote* vote, void* hip_stream);
/* Deviation of spslam_refkf_vote: the reference credits every keyframe in pMP->GetObservations() (:1474-1476);
 * this vote credits only the keyframe that created the point.  The two agree while each point has one observer,
 * which stops holding once LocalMapping adds observations.  spslam_track_update_local_map_batch_device below
 * votes over the observer lists. */

/* Tracking::UpdateLocalMap (src/Tracking.cc:1427-1571): UpdateLocalKeyFrames (:1463-1571) then UpdateLocalPoints
 * (:1437-1460), per frame, batched, on a device-resident map that the host maintains.  One workgroup per frame.
 *   Votes (:1466-1483): every current-frame keypoint with a map point that is not bad adds one vote to every
 *     keyframe of that point's observer list.
 *   K1 (:1485-1510): no keyframe with a vote -> return before clear(): local_kfs / n_local_kfs keep what they
 *     held (they are IN / OUT per frame slot) and kf_max = -1.  Otherwise the list is cleared and the voted
 *     keyframes that are not bad are appended in ascending keyframe index; kf_max = the first strict maximum
 *     among them (-1 when all voters are bad: the list is then empty).
 *   Neighbours (:1513-1564): for each of the first K1 entries, in order: stop when the list holds > 80 (checked
 *     before each entry); append the first of the entry's <= 10 best covisible keyframes
 *     (GetBestCovisibilityKeyFrames(10), KeyFrame.cc:179) that is not bad and not yet in the list; append the first
 *     child that is not bad and not in the list; if the parent exists and is not in the list append it (no bad
 *     check, as the reference) and end the whole loop (the break at :1560 leaves the outer for).
 *   Local points (:1437-1460): the local keyframes' GetMapPointMatches() concatenated in list order then keypoint
 *     order, empty slots and bad points dropped, the first occurrence of each point kept.
 * Every index in the tables is local to the frame's sequence: keyframe k of frame f is entry kf_base[f] + k of the
 * keyframe tables, point row r is entry row_base[f] + r of the point tables, so many sequences share one call.
 * Entries outside [0, n_kf) / [0, scratch_stride) are ignored.
 * Deviations from the reference:
 *   - keyframes and children are walked in ascending index where the reference has pointer order
 *     (std::map<KeyFrame*>, std::set<KeyFrame*>), as everywhere at this ABI;
 *   - the neighbour pass iterates the first K1 entries by index.  The reference iterates the vector it appends
 *     to after reserve(3 * K1); K1 + 2 (K1 - 1) + 3 appends can reallocate under the iterator, which is
 *     undefined.  This is the defined reading;
 *   - mCurrentFrame.mvpMapPoints[i] = NULL for a bad point (:1480) is left to the caller: the bad point only
 *     casts no vote;
 *   - mnTrackReferenceForFrame stamps are not written anywhere: membership lives in the workgroup's LDS and
 *     in `scratch`. */
typedef struct spslam_local_map {
    /* the frames' own map points: either frame_rows, or (frame_rows == NULL) the mm batch, read as
     * spslam_track_refkf_vote_batch_device reads it: for every keypoint i with an edge that is not an outlier,
     * id = proj_points[point_offset + proj_match[i]].id, row = id_to_row ? id_to_row[id_base[f] + id] : id */
    const int32_t* frame_rows;    /* f * cap + i: the keypoint's point row, -1 = none (may be NULL) */
    const int* kp_counts;         /* with frame_rows: keypoints per frame */
    const int32_t* id_to_row;     /* mm path: map point id -> row, -1 = none (may be NULL) */
    const int32_t* id_base;       /* mm path, per frame: its sequence's first entry of id_to_row (NULL = 0) */
    const int32_t* kf_base;       /* per frame: its sequence's keyframe 0 in the keyframe tables */
    const int32_t* row_base;      /* per frame: its sequence's row 0 in the point tables */
    int32_t cap;                  /* with frame_rows: keypoint slots per frame */
    int32_t n_kf;                 /* keyframes per sequence, 1 .. 1024 */
    /* per point row */
    const int32_t* obs_off;       /* CSR (rows + 1): the row's observers in obs_kf */
    const int32_t* obs_kf;        /* observer keyframes, ascending (MapPoint::GetObservations) */
    const uint8_t* point_bad;     /* MapPoint::isBad (may be NULL: none) */
    const spslam_local_point* points;  /* the records (required with out->records) */
    /* per keyframe */
    const uint8_t* kf_bad;        /* KeyFrame::isBad (may be NULL: none) */
    const int32_t* covis;         /* 10 per keyframe: GetBestCovisibilityKeyFrames(10), best first, -1 padded */
    const int32_t* child_off;     /* CSR (keyframes + 1) */
    const int32_t* child;         /* GetChilds, ascending */
    const int32_t* parent;        /* GetParent, -1 = none */
    const int32_t* match_off;     /* CSR (keyframes + 1) */
    const int32_t* match_row;     /* GetMapPointMatches in keypoint order: the point's row or -1 */
} spslam_local_map;

typedef struct spslam_local_map_out {
    const int8_t* state;          /* per frame: 2 = LOST (spslam_refkf_batch.state): the frame is skipped entirely,
                                     nothing of it is written (:406-409); may be NULL */
    int32_t* local_kfs;           /* IN / OUT, f * kf_cap: mvpLocalKeyFrames */
    int32_t* n_local_kfs;         /* IN / OUT per frame */
    int32_t* kf_max;              /* out per frame: pKFmax, -1 = none */
    int32_t* local_rows;          /* out, f * capacity: mvpLocalMapPoints as point rows */
    int32_t* n_local;             /* out per frame */
    int32_t* status;              /* out per frame: 0 ok, 1 = the point list exceeded capacity (its first capacity
                                     entries are written, n_local = capacity) */
    int32_t* scratch;             /* f * scratch_stride: the de-duplication's first position per row.  Its contents
                                     on entry do not matter and need no memset between calls */
    int32_t kf_cap;               /* >= n_kf */
    int32_t capacity;             /* >= 0 */
    int32_t scratch_stride;       /* > every row of a sequence */
    int32_t pad;
    spslam_local_point* records;  /* out (may be NULL), f * capacity: points[row_base[f] + local_rows[..]] in order */
    spslam_local_frame* local_frames;  /* with records: point_offset = f * capacity and n_points = n_local are
                                     written, Tcw / seen_offset / stamp are left as they are, so that
                                     spslam_search_local_points_batch_device runs on the output directly */
} spslam_local_map_out;

/* mm may be NULL when map->frame_rows is given. */
int spslam_track_update_local_map_batch_device(spslam_ctx* ctx, int n_frames, const spslam_track_batch* mm,
                                               const spslam_local_map* map, const spslam_local_map_out* out,
                                               void* hip_stream);

/* Drop-in for one frame on host arrays: the same two structs holding host pointers.  map: frame_rows (n_kp
 * entries) is required; kp_counts, id_to_row, id_base, kf_base, row_base and cap are ignored (one sequence at base
 * 0); the tables hold n_rows point rows and map->n_kf keyframes.  out: state, scratch, scratch_stride and kf_cap
 * are ignored (local_kfs holds n_kf entries, IN / OUT as above); local_frames, when given with records, is one
 * frame whose point_offset becomes 0. */
int spslam_track_update_local_map(spslam_ctx* ctx, const spslam_local_map* map, int n_rows, int n_kp,
                                  const spslam_local_map_out* out);

/* dst[f] = src[f] for every frame f with flags[f] != 0, region by region: frame f's bytes at dst + f * dst_stride
 * and src + f * src_stride (sizes and strides multiples of 4; at most 32 regions per call). */
typedef struct spslam_frame_region {
    void* dst;
    const void* src;
    int64_t frame_bytes;
    int64_t dst_stride;
    int64_t src_stride;
} spslam_frame_region;

int spslam_masked_frame_copy_device(spslam_ctx* ctx, int n_frames, const uint8_t* flags, int n_regions,
                                    const spslam_frame_region* regions, void* hip_stream);

/* ---------------------------------------------------------------- bag of words
 * DBoW2 (vendored Thirdparty/DBoW2) as the tracking path uses it:
 *   spslam_bow_load_vocabulary  TemplatedVocabulary::loadFromTextFile
 *                               (DBoW2/TemplatedVocabulary.h:1338-1424; System.cc:64 loads
 *                               ORBvoc.txt this way).  The text is "k L scoring weighting"
 *                               then one "parent isLeaf d0..d31 weight" line per node; an
 *                               empty line after a final newline becomes one more leaf under
 *                               the root with weight 0 (the reference's eof loop), whose
 *                               descriptor the reference leaves uninitialised (zero here).
 *                               One vocabulary per context, resident in HBM.
 *   spslam_bow_transform        Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cc:495-502,
 *                               src/KeyFrame.cc:64-72): TemplatedVocabulary::transform(
 *                               descriptors, mBowVec, mFeatVec, levelsup = 4) (:1127-1194,
 *                               :1217-1259): BowVector = sorted (word id, value) pairs
 *                               (TF-IDF: summed idf weights, then L1-normalised for ORBvoc's
 *                               L1_NORM scoring), FeatureVector = sorted node ids (the node at
 *                               level L - levelsup on each feature's path) with the feature
 *                               indices of each node in increasing order (CSR: fv_start has
 *                               n_fv + 1 entries).  Stop words (weight 0) are in neither.
 *   spslam_search_by_bow        ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)
 *                               (src/ORBmatcher.cc:159-288), as TrackReferenceKeyFrame
 *                               (matcher(0.7, true), Tracking.cc:797-802) and Relocalization
 *                               (0.75, Tracking.cc:1593-1609) call it: per shared FeatureVector
 *                               node, each keyframe feature with a good map point takes the
 *                               closest free frame feature if its distance <= TH_LOW (50) and
 *                               < nn_ratio x the second best; rotation-consistency filter
 *                               (HISTO_LENGTH 30, ComputeThreeMaxima).  Output per frame
 *                               feature: the keyframe feature whose map point it receives
 *                               (vpMapPointMatches), -1 if none; return value nmatches. */
typedef struct spslam_bow_params {
    float nn_ratio;           /* ORBmatcher mfNNratio (0.7 TrackReferenceKeyFrame, 0.75 Relocalization) */
    int32_t check_orientation;/* mbCheckOrientation */
} spslam_bow_params;

/* text: the vocabulary file's bytes (len of them).  Outputs (may be NULL): k, L, node and word counts. */
int spslam_bow_load_vocabulary(spslam_ctx* ctx, const char* text, size_t len, int* k, int* L, int* n_nodes,
                               int* n_words);

/* Drop-in for one frame on host buffers: desc n x 32 bytes.  bow_words / bow_values:
 * >= n entries, *n_bow receives the BowVector size; fv_nodes: >= n, fv_start: >= n + 1,
 * fv_features: >= n entries, *n_fv the FeatureVector size. */
int spslam_bow_transform(spslam_ctx* ctx, const uint8_t* desc, int n, int levelsup, uint32_t* bow_words,
                         double* bow_values, int* n_bow, uint32_t* fv_nodes, int32_t* fv_start,
                         int32_t* fv_features, int* n_fv);

/* Batched, device resident: frame f's d_counts[f] descriptors at d_desc + f*cap*32 (the ORB
 * batch layout).  Outputs of frame f at f*cap (d_fv_start at f*(cap+1), relative to the
 * frame's f*cap); d_n_bow / d_n_fv one int per frame.  cap <= 8192. */
int spslam_bow_transform_batch_device(spslam_ctx* ctx, int n_frames, const uint8_t* d_desc, const int* d_counts,
                                      int cap, int levelsup, uint32_t* d_bow_words, double* d_bow_values,
                                      int* d_n_bow, uint32_t* d_fv_nodes, int32_t* d_fv_start,
                                      int32_t* d_fv_features, int* d_n_fv, void* hip_stream);

/* One side of SearchByBoW in the batch layout of spslam_bow_transform_batch_device:
 * slot f's features at f*cap (descriptors, keypoints -- only .angle is read -- and, on the
 * keyframe side, has_point[i] = GetMapPointMatches()[i] && !isBad()), its FeatureVector at
 * f*cap / f*(cap+1). */
typedef struct spslam_bow_side {
    const uint8_t* desc;
    const spslam_keypoint* keys;     /* keyframe: mvKeysUn; frame: mvKeys */
    const uint8_t* has_point;        /* keyframe side; ignored on the frame side */
    const int* counts;
    const uint32_t* fv_nodes;
    const int32_t* fv_start;
    const int32_t* fv_features;
    const int* n_fv;
    int32_t cap;
    int32_t pad;
} spslam_bow_side;

/* Drop-in for one (keyframe, frame) pair on host buffers (FeatureVectors as spslam_bow_transform
 * returns them).  match: f_n ints. */
int spslam_search_by_bow(spslam_ctx* ctx, const uint8_t* kf_desc, const spslam_keypoint* kf_keys,
                         const uint8_t* kf_has_point, int kf_n, const uint32_t* kf_fv_nodes,
                         const int32_t* kf_fv_start, const int32_t* kf_fv_features, int kf_n_fv,
                         const uint8_t* f_desc, const spslam_keypoint* f_keys, int f_n, const uint32_t* f_fv_nodes,
                         const int32_t* f_fv_start, const int32_t* f_fv_features, int f_n_fv,
                         const spslam_bow_params* params, int32_t* match, int* nmatches);

/* Batched, device resident: pair p = (keyframe slot, frame slot) = d_pairs[2p], d_pairs[2p+1];
 * d_match at p * frame.cap, d_nmatches one int per pair. */
int spslam_search_by_bow_batch_device(spslam_ctx* ctx, int n_pairs, const int32_t* d_pairs,
                                      const spslam_bow_side* keyframe, const spslam_bow_side* frame,
                                      const spslam_bow_params* params, int32_t* d_match, int* d_nmatches,
                                      void* hip_stream);

/* ---------------------------------------------------------------- place recognition: KeyFrameDatabase
 * KeyFrameDatabase::DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:199-309), the first call of
 * Tracking::Relocalization (src/Tracking.cc:1573-1734); KeyFrameDatabase::DetectLoopCandidates (:76-197) and the
 * reference score that LoopClosing::DetectLoop computes before it (src/LoopClosing.cc:126-140).  The candidates
 * they return are the keyframe slots of the pair list of spslam_search_by_bow_batch_device.  PnP, Sim3 and the
 * consistency groups (LoopClosing.cc:154-220) are not here; add() and erase() stay with the caller: they flip
 * in_db.
 *
 * Tables.  All device resident; keyframe indices are local to a sequence, keyframe k of a problem is entry
 * kf_base + k, as in spslam_covis_problem.  The neighbours come from spslam_covis_graph: covis is
 * GetBestCovisibilityKeyFrames(10), weights (non-zero) is GetConnectedKeyFrames, ordered / n_ordered is
 * GetVectorCovisibleKeyFrames.
 *
 * The inverted file is not mirrored: in_db says which keyframes it holds, and the order of every word's list
 * follows from that.  Every add() of the reference is made by LoopClosing::DetectLoop (LoopClosing.cc:118,148)
 * on keyframes it takes from a FIFO that LocalMapping fills in mnId order; erase() removes one element of a
 * list and keeps the order of the rest (KeyFrameDatabase.cc:48-67).  So each word's list is in ascending
 * keyframe index among the keyframes with in_db set, and walking the query's words in ascending word id (a
 * BowVector is a std::map) over such lists meets the keyframes in this order: by the position, in the query
 * vector, of the first word they share with it, then by keyframe index.  That is the order of
 * lKFsSharingWords, and every later list of the two functions is a subsequence of it.
 *
 * reloc_score / loop_score are KeyFrame::mRelocScore / mLoopScore.  They persist across calls, and the
 * relocalization query reads values that earlier queries left (below).  The reference leaves them uninitialised
 * (KeyFrame.cc:35); the caller zero-fills them when a keyframe is created: 0 is a chosen value, the reference
 * has none.
 *
 * Not reproduced: the stamps mnRelocQuery / mnLoopQuery start at 0, so in the reference a query whose id is 0
 * finds every keyframe "already seen" and returns nothing.  Here every query starts with no keyframe seen. */
#define SPSLAM_PLACE_MAX_WORDS 8192  /* a query vector's length at most (the cap of the BoW transform) */
#define SPSLAM_PLACE_OK 0
#define SPSLAM_PLACE_EMPTY 1         /* lKFsSharingWords.empty() (:107, :224): only the result record is written */
#define SPSLAM_PLACE_NONE_KEPT 2     /* loop query, lScoreAndMatch.empty() (:141): the scores stay written */

typedef struct spslam_place_db {
    const uint32_t* bow_words;  /* the layout spslam_bow_transform_batch_device writes: slot kf_base + k at */
    const double* bow_values;   /*   (kf_base + k) * cap, words ascending and unique                        */
    const int* n_bow;           /* per keyframe, 0 .. cap */
    const uint8_t* in_db;       /* per keyframe: set by add(), cleared by erase() */
    float* reloc_score;         /* per keyframe: mRelocScore, written for the keyframes a relocalization query scores */
    float* loop_score;          /* per keyframe: mLoopScore, written for the keyframes a loop query scores */
    int32_t cap;                /* 1 .. SPSLAM_PLACE_MAX_WORDS */
    int32_t pad;
} spslam_place_db;

typedef struct spslam_place_frames {  /* the query frames' BowVectors, frame slot f at f * cap */
    const uint32_t* bow_words;
    const double* bow_values;
    const int* n_bow;
    int32_t cap;                /* 1 .. SPSLAM_PLACE_MAX_WORDS */
    int32_t pad;
} spslam_place_frames;

typedef struct spslam_place_problem {
    int32_t kf_base;
    int32_t n_kf;               /* keyframes of this sequence, 1 .. SPSLAM_COVIS_MAX_KF */
    int32_t query;              /* relocalization: the frame slot; loop and min-score entries: the keyframe index */
    int32_t out_offset;         /* the problem's first candidate in d_candidates; room for n_kf entries */
} spslam_place_problem;         /* 16 bytes */

typedef struct spslam_place_result {
    int32_t status;             /* SPSLAM_PLACE_* */
    int32_t n_sharing;          /* lKFsSharingWords.size() */
    int32_t max_common_words;
    int32_t min_common_words;   /* (int)(max_common_words * 0.8f) */
    int32_t n_scored;           /* nscores */
    int32_t n_kept;             /* lScoreAndMatch.size(): relocalization n_scored, loop those with score >= min_score */
    int32_t n_candidates;
    float best_acc_score;       /* bestAccScore; EMPTY: 0, NONE_KEPT: min_score */
} spslam_place_result;          /* 32 bytes; EMPTY: every field after n_sharing is 0 */

/* The score of two BowVectors is L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68): the sum in
 * double, over the shared words in ascending word id, of fabs(vi - wi) - fabs(vi) - fabs(wi) with vi the query's
 * value; then -sum / 2.0 in double, rounded to float where the reference stores it in one.  The float has the
 * bits of that serial sum.
 *
 * DetectRelocalizationCandidates for problem p's frame, one workgroup per problem:
 *   sharing list (:207-225): every in_db keyframe with at least one word in common with the query, in the order
 *     derived above; c_i its number of common words.  Empty: SPSLAM_PLACE_EMPTY, n_candidates 0, and neither a
 *     score nor a candidate is written;
 *   word threshold (:228-235): max_common_words = max c_i, min_common_words = (int)(max * 0.8f), the product in
 *     float;
 *   scores (:242-253): the keyframes with c_i > min_common_words, in list order; reloc_score[i] is written for
 *     these only;
 *   accumulation (:262-287): per scored keyframe, acc starts as its score (float) and best as the keyframe; its
 *     covis row is walked in order (-1 skipped), and every neighbour that is in the sharing list of this query
 *     adds its reloc_score to acc and takes over best on a strictly greater score.  A neighbour in the list that
 *     this query did not score contributes reloc_score as stored: the value of the last query that scored it, or
 *     the initial 0 (:273-281 test mnRelocQuery only).  best_acc_score is the maximum acc, from 0;
 *   retention (:290-306): acc > 0.75f * best_acc_score; d_candidates + out_offset receives the best keyframes of
 *     the kept entries in list order, each at its first occurrence only.  Entries past n_candidates are not
 *     written.
 * CONTRACT: a call holds at most one problem per sequence (the score tables are shared state).  Successive
 * queries of one sequence are successive calls on one stream.  graph: only covis is read. */
int spslam_place_reloc_candidates_batch_device(spslam_ctx* ctx, int n_problems,
                                               const spslam_place_problem* d_problems, const spslam_place_db* db,
                                               const spslam_place_frames* frames, const spslam_covis_graph* graph,
                                               spslam_place_result* d_results, int32_t* d_candidates,
                                               void* hip_stream);

/* DetectLoopCandidates for problem p's keyframe `query`; the same walk with these differences:
 *   the query vector is the keyframe's own.  CONTRACT: in_db[query] is 0 (DetectLoop adds it after the query,
 *     LoopClosing.cc:148);
 *   a keyframe i with weights[query][i] != 0 is connected (:78, :96): outside the sharing list and every later
 *     step, also where it stands in a neighbour's covis row;
 *   loop_score[i] is written for every scored keyframe (:135); those with score >= min_score become entries
 *     (:136), n_kept of them.  None: SPSLAM_PLACE_NONE_KEPT, n_candidates 0;
 *   a neighbour contributes to acc only if this query scored it: in the list and c > min_common_words (:159);
 *   best_acc_score starts at min_score (:145);
 *   min_score is d_min_score[p], a device float, so that spslam_place_min_score_batch_device chains into this
 *     entry on one stream.
 * graph: covis, weights and stride are read. */
int spslam_place_loop_candidates_batch_device(spslam_ctx* ctx, int n_problems,
                                              const spslam_place_problem* d_problems, const spslam_place_db* db,
                                              const spslam_covis_graph* graph, const float* d_min_score,
                                              spslam_place_result* d_results, int32_t* d_candidates,
                                              void* hip_stream);

/* LoopClosing.cc:126-140: d_min_score[p] = the minimum, in float from 1.0f, of score(query, j) over the
 * keyframes j of query's ordered list that d_kf_bad (per keyframe, may be NULL: none) does not flag.  in_db is
 * not read.  graph: ordered, n_ordered and stride are read; out_offset is not used. */
int spslam_place_min_score_batch_device(spslam_ctx* ctx, int n_problems, const spslam_place_problem* d_problems,
                                        const spslam_place_db* db, const spslam_covis_graph* graph,
                                        const uint8_t* d_kf_bad, float* d_min_score, void* hip_stream);

/* One problem on host arrays (db's and graph's pointers too) at base 0, n_kf keyframes.  Every index is checked
 * (n_kf, cap, n_bow <= cap, ascending words, covis, ordered, query): SPSLAM_ERR_ARG on a violation, nothing
 * launched.  db->reloc_score / db->loop_score are rewritten in place; candidates has room for n_kf entries and
 * is written up to result->n_candidates.  The relocalization query is q_n words (<= SPSLAM_PLACE_MAX_WORDS).
 * The loop form refuses in_db[query] != 0. */
int spslam_place_reloc_candidates(spslam_ctx* ctx, const spslam_place_db* db, int n_kf, const uint32_t* q_words,
                                  const double* q_values, int q_n, const spslam_covis_graph* graph,
                                  spslam_place_result* result, int32_t* candidates);
int spslam_place_loop_candidates(spslam_ctx* ctx, const spslam_place_db* db, int n_kf, int query,
                                 const spslam_covis_graph* graph, float min_score, spslam_place_result* result,
                                 int32_t* candidates);
int spslam_place_min_score(spslam_ctx* ctx, const spslam_place_db* db, int n_kf, int query,
                           const spslam_covis_graph* graph, const uint8_t* kf_bad, float* min_score);

/* ---------------------------------------------------------------- LoopClosing: ComputeSim3 and SearchAndFuse
 * The four ORBmatcher overloads LoopClosing calls after DetectLoop (src/LoopClosing.cc:233-432, :674-715), on the
 * tables the library keeps in HBM: the frame stage's keyframe slots, the FeatureVector CSR of
 * spslam_bow_transform_batch_device, the spslam_local_point table and the match_off / match_row CSR.
 *   SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12)              src/ORBmatcher.cc:522-655   (LoopClosing.cc:267)
 *   SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)    src/ORBmatcher.cc:1102-1326 (LoopClosing.cc:325)
 *   SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)       src/ORBmatcher.cc:290-403   (LoopClosing.cc:393)
 *   Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)                src/ORBmatcher.cc:977-1100  (LoopClosing.cc:700)
 * All four are deterministic, and so is Sim3Solver (src/Sim3Solver.cc, LoopClosing.cc:276-324) once its rand() draws
 * are an input: it sits between the first two.  Optimizer::OptimizeSim3 (src/Optimizer.cc:2279-2474,
 * LoopClosing.cc:328) follows SearchBySim3 and leaves the Scw that SearchByProjection takes, so that a candidate goes
 * from the BoW matches to the Scw search on one stream.  The consistency groups and CorrectLoop's map mutation stay
 * with the caller.  None of these entries has a timing kind, and none is part of the batched step.
 * KeyFrame's image bounds are ints (include/KeyFrame.h:198-201): the configured bounds are truncated, as for
 * spslam_fuse_search.  The host-pointer forms take one problem and check every index before anything is launched
 * (SPSLAM_ERR_ARG on a violation). */

/* ---- SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12).  Both sides are spslam_bow_side with keys = mvKeysUn and
 * has_point[i] = GetMapPointMatches()[i] && !isBad(), read on both sides.  Pair p = (slot 1, slot 2) =
 * d_pairs[2p], d_pairs[2p+1]; d_match12 at p * kf1->cap holds, per KF1 keypoint, the KF2 keypoint index or -1 (the
 * caller maps it through vpMapPoints2), written for the slot's counts[slot 1] keypoints; d_nmatches one int per
 * pair.  Unlike the keyframe-to-frame overload acceptance is bestDist1 < TH_LOW, strict (:598), the result and the
 * rotation histogram are indexed by idx1, and a KF2 keypoint stays blocked (vbMatched2) for a match that the
 * histogram later removes.  kf1->cap * 13 + kf2->cap bytes of LDS: <= 150 KB. */
int spslam_search_by_bow_kf_batch_device(spslam_ctx* ctx, int n_pairs, const int32_t* d_pairs,
                                         const spslam_bow_side* kf1, const spslam_bow_side* kf2,
                                         const spslam_bow_params* params, int32_t* d_match12, int* d_nmatches,
                                         void* hip_stream);

/* One keyframe of the host form: n keypoints, its FeatureVector as spslam_bow_transform returns it. */
typedef struct spslam_bow_keyframe {
    const uint8_t* desc;             /* n * 32 */
    const spslam_keypoint* keys_un;  /* n (only .angle is read) */
    const uint8_t* has_point;        /* n */
    const uint32_t* fv_nodes;        /* n_fv, strictly ascending */
    const int32_t* fv_start;         /* n_fv + 1, from 0, not descending, fv_start[n_fv] <= n */
    const int32_t* fv_features;      /* fv_start[n_fv] entries in [0, n) */
    int32_t n, n_fv;
} spslam_bow_keyframe;

/* Drop-in for one pair on host buffers.  match12: kf1->n ints. */
int spslam_search_by_bow_kf(spslam_ctx* ctx, const spslam_bow_keyframe* kf1, const spslam_bow_keyframe* kf2,
                            const spslam_bow_params* params, int32_t* match12, int* nmatches);

/* ---- SearchBySim3.  The map, as spslam_covis_map / spslam_point_refresh_map point at it: keyframe k has pose
 * kf_Tcw + 16k and its arrays in slot kf_slot[k] of the frame stage's layouts; its GetMapPointMatches are
 * match_row[match_off[k] + i] for keypoint i (the point's row in `points`, or -1), counts[slot] of them. */
typedef struct spslam_sim3_map {
    const float* kf_Tcw;        /* n_kf * 16, row-major: GetRotation / GetTranslation */
    const int32_t* kf_slot;     /* n_kf */
    const int32_t* match_off;   /* n_kf + 1, absolute offsets into match_row */
    const int32_t* match_row;
    const uint8_t* point_bad;   /* per row, may be NULL: none */
    const spslam_local_point* points;
} spslam_sim3_map;

/* One call of SearchBySim3.  sR12 = s12*R12, sR21 = (1.0/s12)*R12.t() and t21 = -sR21*t12 (:1119-1121) are made on
 * the device from s12, R12 and t12, so that their bits are the library's and not the binding's. */
typedef struct spslam_sim3_pair {
    int32_t kf1, kf2;         /* keyframe indices of the map */
    int32_t match_offset;     /* vpMatches12, in and out: N1 ints at d_match12 + match_offset, KF2 keypoint or -1 */
    int32_t result_offset;    /* n_found at d_n_found[result_offset] */
    float s12;
    float R12[9];             /* row-major */
    float t12[3];
    int32_t pad[3];
} spslam_sim3_pair;           /* 80 bytes */

typedef struct spslam_sim3_params {
    float th;                 /* radius at level 0 (7.5 in ComputeSim3) */
    int32_t pad;
} spslam_sim3_params;

/* Batched, device resident.  On entry vbAlreadyMatched1[i] is match12[i] >= 0 and vbAlreadyMatched2[match12[i]] is
 * set for the same entries: the reference's GetIndexInKeyFrame(pKF2) (:1138) whenever the map is consistent, that
 * is, whenever the point that vpMatches12[i] names is observed by pKF2 at the keypoint the caller derived it from.
 * A binding that cannot promise that passes d_already2 (may be NULL): one byte per KF2 keypoint, pair p's at
 * p * cap, which then replaces the derived flags of every pair of the call.  The two searches (:1148-1305) run in one launch and do
 * not depend on order; a second launch does the agreement pass (:1307-1323), which writes match12[i1] = idx2 for
 * the pairs found and leaves every other entry as it was.  Pairs' match12 ranges must be disjoint.  cap: keypoint
 * slots per keyframe slot; the call keeps 9 * cap bytes of scratch per pair in the context, which
 * spslam_search_by_projection_sim3_batch_device uses too: calls that share a context are ordered on one stream. */
int spslam_search_by_sim3_batch_device(spslam_ctx* ctx, int n_pairs, const spslam_sim3_pair* d_pairs,
                                       const spslam_sim3_map* map, const spslam_keypoint* d_keys_un,
                                       const uint8_t* d_desc, const int32_t* d_grid_off, const int32_t* d_grid_idx,
                                       const int* d_counts, int cap, const uint8_t* d_already2,
                                       const spslam_sim3_params* params, int32_t* d_match12, int* d_n_found,
                                       void* hip_stream);

/* One keyframe of the host form. */
typedef struct spslam_sim3_keyframe {
    const float* Tcw;                /* 16 */
    const spslam_keypoint* keys_un;  /* n */
    const uint8_t* desc;             /* n * 32 */
    const int32_t* grid_off;         /* 64*48 + 1: from 0, not descending, grid_off[64*48] <= n */
    const int32_t* grid_idx;         /* grid_off[64*48] entries in [0, n) */
    const int32_t* match_row;        /* n entries in [-1, n_rows) */
    int32_t n, pad;
} spslam_sim3_keyframe;

/* Drop-in for one pair on host buffers: points / point_bad (may be NULL) are n_rows table rows; match12 (kf1->n
 * ints in [-1, kf2->n)) is rewritten in place; already2: kf2->n bytes or NULL.  *n_found receives the return
 * value.  pair->kf1 / kf2 / offsets are ignored. */
int spslam_search_by_sim3(spslam_ctx* ctx, const spslam_sim3_keyframe* kf1, const spslam_sim3_keyframe* kf2,
                          const spslam_local_point* points, const uint8_t* point_bad, int n_rows,
                          const spslam_sim3_pair* pair, const uint8_t* already2, const spslam_sim3_params* params,
                          int32_t* match12, int* n_found);

/* ---- Sim3Solver (src/Sim3Solver.cc), as ComputeSim3 uses it between SearchByBoW and SearchBySim3: the
 * constructor, SetRansacParameters, iterate and GetEstimated*.  Semantics: tests/sim3_solver_ref.py.
 * The solver draws from rand(): the draws are an input here.  The caller records 3 * max_iterations raw rand()
 * values per problem; iteration k, counted from 0 over the solver's life, uses values 3k .. 3k+2 for its three
 * RandomInt(0, size - 1) = int((double)r / ((double)rand_max + 1.0) * size).  All hypotheses of a call are
 * evaluated, then the first one at which the reference's sequential loop returns is selected. */
#define SPSLAM_SIM3_FOUND 0      /* iterate returned a transformation */
#define SPSLAM_SIM3_NOT_YET 1    /* empty Mat, bNoMore false */
#define SPSLAM_SIM3_NO_MORE 2    /* empty Mat, bNoMore true: N < min_inliers, or mRansacMaxIts reached */
#define SPSLAM_SIM3_MAX_ITERATIONS 4096

typedef struct spslam_sim3_problem {
    int32_t kf1, kf2;          /* keyframe indices of the map */
    int32_t match_offset;      /* vpMatched12: the keyframe's N1 ints at d_match12 (and d_match12_out) + match_offset */
    int32_t rand_offset;       /* 3 * max_iterations ints at d_rand + rand_offset */
    int32_t inlier_offset;     /* vbInliers: N1 bytes at d_inliers + inlier_offset */
    int32_t iterations_done;   /* mnIterations on entry (0 for a new solver) */
    int32_t best_inliers;      /* mnBestInliers on entry (0 for a new solver) */
    int32_t n_iterations;      /* iterate's nIterations */
} spslam_sim3_problem;         /* 32 bytes */

typedef struct spslam_sim3_result {
    int32_t status;            /* SPSLAM_SIM3_* */
    int32_t n;                 /* N: the correspondences the constructor kept */
    int32_t iterations_done;   /* mnIterations on exit */
    int32_t best_inliers;      /* mnBestInliers on exit */
    int32_t n_inliers;         /* nInliers (0 unless FOUND) */
    float s12;                 /* GetEstimatedScale; this and what follows are 0 unless FOUND */
    float R12[9];              /* GetEstimatedRotation, row-major */
    float t12[3];              /* GetEstimatedTranslation */
    float T12[16];             /* the returned Mat, row-major */
} spslam_sim3_result;          /* 136 bytes */

typedef struct spslam_sim3_solver_params {
    int32_t min_inliers;       /* mRansacMinInliers (20 in ComputeSim3), >= 3 */
    int32_t max_iterations;    /* SetRansacParameters' maxIterations (300), 1 .. SPSLAM_SIM3_MAX_ITERATIONS */
    int32_t rand_max;          /* the caller's RAND_MAX */
    int32_t fix_scale;         /* mbFixScale (RGB-D: 1) */
} spslam_sim3_solver_params;

/* SetRansacParameters (:114-138) for every N a keyframe can give: table[n] = mRansacMaxIts for N = n, n in
 * [min_inliers, cap], with the reference's expression on the host's libm (epsilon in float, pow and log in double,
 * ceil, 1 when N == min_inliers, max(1, min(., max_iterations))); 0 below min_inliers, where iterate returns at
 * once.  table: cap + 1 ints.  A quotient that no int holds counts as max_iterations. */
int spslam_sim3_ransac_table(double probability, int min_inliers, int max_iterations, int cap, int32_t* table);

/* Batched, device resident.  Problem p reads its keyframes from the map and the slots, d_match12 as
 * spslam_search_by_bow_kf_batch_device left it, and its draws.  The constructor keeps keypoint i1 of KF1, in
 * order, when match12[i1] is a keypoint of KF2, both keypoints have a map point (match_row >= 0) and neither point
 * is bad.  CONTRACT, as for SearchBySim3: the points' GetIndexInKeyFrame are i1 and match12[i1].  d_max_its_table:
 * cap + 1 ints of spslam_sim3_ransac_table for the same min_inliers and max_iterations.  The camera and
 * mvLevelSigma2 are the context's; octaves outside the configured levels read level 0.
 * Outputs: d_results[p]; d_inliers (always written: N1 bytes, zero unless FOUND).  d_pairs_out and d_match12_out
 * may be NULL; given, a FOUND problem p gets d_pairs_out[p] = {kf1, kf2, match_offset, result_offset = p, s12, R12,
 * t12} and, at d_match12_out + match_offset, match12 with every entry that is no inlier set to -1
 * (LoopClosing.cc:315-320): what spslam_search_by_sim3_batch_device takes on the same stream.  Problems that are
 * not FOUND leave both as they were.  A draw outside [0, rand_max] is clamped into the list it indexes.
 * cap <= 8192.  The call keeps 16 + 56 * cap + 64 * max_iterations bytes of scratch per problem in the context,
 * the buffer the other loop-closing searches use: calls that share a context are ordered on one stream. */
int spslam_sim3_solver_batch_device(spslam_ctx* ctx, int n_problems, const spslam_sim3_problem* d_problems,
                                    const spslam_sim3_map* map, const spslam_keypoint* d_keys_un, const int* d_counts,
                                    int cap, const int32_t* d_match12, const int32_t* d_rand,
                                    const int32_t* d_max_its_table, const spslam_sim3_solver_params* params,
                                    spslam_sim3_result* d_results, uint8_t* d_inliers, spslam_sim3_pair* d_pairs_out,
                                    int32_t* d_match12_out, void* hip_stream);

/* Drop-in for one problem on host buffers: the keyframes' Tcw, keys_un, match_row and n are read (the grid and the
 * descriptors are not); match12: kf1->n ints in [-1, kf2->n); rand: 3 * max_iterations values in [0, rand_max];
 * *iterations_done and *best_inliers are the solver's state, read and rewritten; inliers: kf1->n bytes;
 * match12_out (may be NULL): kf1->n ints, written when the status is FOUND.  Every index is checked before anything
 * is launched: match12, match_row, the octaves against the configured levels, min_inliers >= 3, n_iterations >= 0. */
int spslam_sim3_solver(spslam_ctx* ctx, const spslam_sim3_keyframe* kf1, const spslam_sim3_keyframe* kf2,
                       const spslam_local_point* points, const uint8_t* point_bad, int n_rows,
                       const int32_t* match12, const int32_t* rand, const spslam_sim3_solver_params* params,
                       double probability, int n_iterations, int* iterations_done, int* best_inliers,
                       spslam_sim3_result* result, uint8_t* inliers, int32_t* match12_out);

/* ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:2279-2474) as ComputeSim3 calls it between SearchBySim3 and
 * SearchByProjection(pKF, Scw, ...), and mg2oScw / mScw of LoopClosing.cc:335-337.  Semantics: tests/sim3_opt_ref.cpp
 * (DESIGN 3.19): g2o's Levenberg-Marquardt on one VertexSim3Expmap over an EdgeSim3ProjectXYZ and an
 * EdgeInverseSim3ProjectXYZ per correspondence, numeric Jacobians, Huber kernels of delta sqrt(th2), the dense LDLT;
 * optimize(5), the chi2 check that removes pairs, optimize(5 or 10), the final check.  All in fp64 with g2o's
 * summation order; sin / cos are correctly rounded.
 * fix_scale must be 1 (RGB-D, the only sensor this library runs: mbFixScale = mSensor != MONOCULAR).  Under a fixed
 * scale the update's sigma is exactly 0 and exp(0) = 1 in every libm; a free scale needs a correctly rounded exp,
 * which the library does not have, so fix_scale = 0 is refused with SPSLAM_ERR_ARG before anything is launched. */
#define SPSLAM_SIM3_OPT_OK 0       /* both optimize calls ran; n_in is OptimizeSim3's return value */
#define SPSLAM_SIM3_OPT_TOO_FEW 1  /* nCorrespondences - nBad < 10 (:2444): returned 0, S12 is the input */

typedef struct spslam_sim3_opt_params {
    float th2;                 /* 10 in ComputeSim3; > 0 */
    int32_t fix_scale;         /* must be 1 */
    int32_t min_inliers;       /* 20 in ComputeSim3: accepted = n_in >= min_inliers */
    int32_t pad;
} spslam_sim3_opt_params;

typedef struct spslam_sim3_opt_result {
    int32_t n_in;              /*   0  the return value (0 when TOO_FEW) */
    int32_t n_corr;            /*   4  nCorrespondences */
    int32_t n_bad;             /*   8  nBad of the first check */
    int32_t status;            /*  12  SPSLAM_SIM3_OPT_* */
    int32_t accepted;          /*  16  n_in >= min_inliers (LoopClosing.cc:331) */
    int32_t iterations1;       /*  20  LM iterations of optimize(5) */
    int32_t trials1;           /*  24  its damping trials in total */
    int32_t iterations2;       /*  28  the same of the second optimize (0 when TOO_FEW) */
    int32_t trials2;           /*  32 */
    int32_t pad;               /*  36 */
    double S12[8];             /*  40  g2oS12 on return: quaternion x y z w (not normalised), t, s */
    double Scw[8];             /* 104  mg2oScw = S12 * Sim3(R2w, t2w, 1.0), the same order */
    float mScw[16];            /* 168  Converter::toCvMat(mg2oScw): [s*R | t; 0 0 0 1] row-major */
} spslam_sim3_opt_result;      /* 232 bytes */

/* Batched, device resident.  Pair p is the spslam_sim3_pair that spslam_sim3_solver_batch_device leaves and
 * spslam_search_by_sim3_batch_device reads: kf1, kf2, match_offset, and s12, R12, t12 as gScm's input
 * (LoopClosing.cc:327); the three calls chain on one stream over the same buffers.  d_match12 is read and rewritten
 * in place (vpMatches1): keypoint i of KF1 becomes an edge pair, in order, when match12[i] is a keypoint of KF2, both
 * keypoints have a map point (match_row >= 0) and neither point is bad; an entry that is skipped stays as it was, an
 * entry whose pair fails either check becomes -1.  CONTRACT, as for SearchBySim3: the points' GetIndexInKeyFrame are
 * i and match12[i].  The camera and mvInvLevelSigma2 are the context's (one camera: K1 = K2); octaves outside the
 * configured levels read level 0.  d_results[p] is always written whole: S12 is the optimised estimate, or the
 * input when the status is TOO_FEW (n_corr = 0 included, where g2o optimises nothing); Scw and mScw are made from
 * that S12 and KF2's kf_Tcw.  Pairs' match12 ranges must be disjoint.  cap <= 8192.  The call keeps 16 + 104 * cap
 * bytes of scratch per pair in the context, the buffer the other loop-closing entries use: calls that share a
 * context are ordered on one stream.  The result does not depend on what the scratch held. */
int spslam_sim3_optimize_batch_device(spslam_ctx* ctx, int n_pairs, const spslam_sim3_pair* d_pairs,
                                      const spslam_sim3_map* map, const spslam_keypoint* d_keys_un, const int* d_counts,
                                      int cap, const spslam_sim3_opt_params* params, int32_t* d_match12,
                                      spslam_sim3_opt_result* d_results, void* hip_stream);

/* Drop-in for one pair on host buffers: the keyframes' Tcw, keys_un, match_row and n are read (the grid and the
 * descriptors are not); match12: kf1->n ints in [-1, kf2->n), rewritten in place; pair->s12 / R12 / t12 are read,
 * its indices and offsets ignored.  Every index, octave and parameter is checked before anything is launched. */
int spslam_sim3_optimize(spslam_ctx* ctx, const spslam_sim3_keyframe* kf1, const spslam_sim3_keyframe* kf2,
                         const spslam_local_point* points, const uint8_t* point_bad, int n_rows,
                         const spslam_sim3_pair* pair, const spslam_sim3_opt_params* params, int32_t* match12,
                         spslam_sim3_opt_result* result);

/* Test hook: fills the loop-closing scratch of the context with a byte value (results must not depend on it). */
int spslam_debug_fill_loop_scratch(spslam_ctx* ctx, int value);

/* ---- PnPsolver (src/PnPsolver.cc), the third call of Tracking::Relocalization (src/Tracking.cc:1573-1734), between
 * SearchByBoW(KeyFrame, Frame) and PoseOptimization: the constructor, SetRansacParameters and iterate with Refine.
 * Semantics: tests/pnp_ref.cpp: EPnP in fp64 over the readings of OpenCV's SVD written down there.
 * The draws are an input, as for Sim3Solver: 4 raw rand() values per iteration, iteration k (counted from 0 over
 * the solver's life) uses values 4k .. 4k+3.  All hypotheses of a call are evaluated, then Refine once per mask the
 * sequential loop would try, and the iteration at which that loop returns is selected.
 * What crosses calls is the caller's: iterations_done, best_inliers, best_Tcw and the best mask (mvbBestInliers:
 * one byte per kept correspondence, in the constructor's order, which is the same at every call on the same
 * inputs). */
#define SPSLAM_PNP_REFINED 0        /* Refine succeeded: Tcw is mRefinedTcw, bNoMore false */
#define SPSLAM_PNP_BEST_NO_MORE 1   /* bNoMore, mBestTcw returned with the best mask */
#define SPSLAM_PNP_NO_MORE 2        /* bNoMore, empty Mat: N < mRansacMinInliers, or no hypothesis qualified */
#define SPSLAM_PNP_OUT_OF_DRAWS 3   /* the call's range passes rand_iterations: the state as far as it got */
#define SPSLAM_PNP_MAX_ITERATIONS 4096

typedef struct spslam_pnp_problem {
    int32_t kf;                /* keyframe index of the map (its GetMapPointMatches are the match's points) */
    int32_t frame_slot;        /* the frame's slot in d_frame_keys_un / d_frame_counts */
    int32_t match_offset;      /* vpMapPointMatches: frame.cap ints at d_match + match_offset, a keyframe keypoint or -1 */
    int32_t rand_offset;       /* 4 * rand_iterations ints at d_rand + rand_offset */
    int32_t inlier_offset;     /* vbInliers: bytes at d_inliers + inlier_offset, ints at d_frame_points + inlier_offset */
    int32_t best_mask_offset;  /* mvbBestInliers: cap bytes at d_best_mask + best_mask_offset */
    int32_t iterations_done;   /* mnIterations on entry (0 for a new solver) */
    int32_t best_inliers;      /* mnBestInliers on entry (0 for a new solver) */
    int32_t n_iterations;      /* iterate's nIterations, at most params->max_iterations */
    int32_t rand_iterations;   /* the iterations that the draws cover */
    int32_t pad[2];
    float best_Tcw[16];        /* mBestTcw on entry (zeros for a new solver) */
} spslam_pnp_problem;          /* 112 bytes */

typedef struct spslam_pnp_result {
    int32_t status;            /* SPSLAM_PNP_* */
    int32_t n;                 /* N: the correspondences the constructor kept */
    int32_t iterations_done;   /* mnIterations on exit */
    int32_t best_inliers;      /* mnBestInliers on exit */
    int32_t n_inliers;         /* nInliers (0 unless a pose is returned) */
    int32_t iteration;         /* the iteration that returned a refined pose, else -1 */
    int32_t min_inliers;       /* mRansacMinInliers for this N */
    int32_t max_its;           /* mRansacMaxIts for this N (0 when N < min_inliers) */
    float best_Tcw[16];        /* mBestTcw on exit, row-major */
    float Tcw[16];             /* the returned Mat as convertTo(CV_32F) rounds it; zeros when empty */
} spslam_pnp_result;           /* 160 bytes */

typedef struct spslam_pnp_params {
    int32_t min_inliers;       /* SetRansacParameters' minInliers (10 in Relocalization) */
    int32_t max_iterations;    /* maxIterations (300), 1 .. SPSLAM_PNP_MAX_ITERATIONS */
    int32_t min_set;           /* minSet: must be 4 */
    int32_t rand_max;          /* the caller's RAND_MAX */
    float epsilon;             /* 0.5 */
    float th2;                 /* 5.991 */
} spslam_pnp_params;

/* SetRansacParameters (:121-157) for every N a frame can give, N = 0 .. cap, with the reference's expressions on
 * the host's libm: min_inliers_n[N] = max(int(N * epsilon), min_inliers, min_set) (an int times a float);
 * max_its[N] = max(1, min(ceil(log(1-p) / log(1 - pow(eps, 3))), max_iterations)) with eps = max(epsilon,
 * (float)min_inliers_n / N) in float, 1 when min_inliers_n == N, and 0 where N < min_inliers_n (iterate returns at
 * once).  A quotient that no int holds counts as max_iterations.  Both tables: cap + 1 ints. */
int spslam_pnp_ransac_table(double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                            int cap, int32_t* max_its, int32_t* min_inliers_n);

/* Batched, device resident.  Problem p reads d_match as spslam_search_by_bow_batch_device leaves it.  The
 * constructor keeps frame keypoint i, in order, when match[i] is a keypoint of the keyframe whose match_row is a
 * point row that is not bad; mvP2D is d_frame_keys_un's x, y, mvSigma2 the context's mvLevelSigma2 at its octave
 * (octaves outside the configured levels read level 0), the camera the context's.  d_frame_counts[slot] keypoints
 * of cap per slot.  d_max_its_table / d_min_inliers_table: cap + 1 ints each of spslam_pnp_ransac_table.
 * Outputs: d_results[p]; d_inliers (always written: the frame's count of bytes, zero unless a pose is returned);
 * d_best_mask, read when best_inliers qualifies and rewritten when a hypothesis of the call sets a new best;
 * d_frame_points (may be NULL): for a problem that returns a pose, the frame's mvpMapPoints of Tracking.cc:1661-1670
 * as ints -- the match's point row where vbInliers, -1 elsewhere -- and untouched otherwise.
 * Only min_set == 4 is built; a draw outside [0, rand_max] is clamped into the list it indexes.  cap <= 8192.
 * The call keeps 16 + 32 * cap + 104 * max_iterations bytes of scratch per problem in the context, the buffer the
 * loop-closing entries use: calls that share a context are ordered on one stream.  The result does not depend on
 * what the scratch held. */
int spslam_pnp_solver_batch_device(spslam_ctx* ctx, int n_problems, const spslam_pnp_problem* d_problems,
                                   const spslam_sim3_map* map, const spslam_keypoint* d_frame_keys_un,
                                   const int* d_frame_counts, int cap, const int32_t* d_match, const int32_t* d_rand,
                                   const int32_t* d_max_its_table, const int32_t* d_min_inliers_table,
                                   const spslam_pnp_params* params, spslam_pnp_result* d_results, uint8_t* d_inliers,
                                   uint8_t* d_best_mask, int32_t* d_frame_points, void* hip_stream);

/* Drop-in for one problem on host buffers.  keys_un: the frame's n_frame keypoints; match: n_frame ints in
 * [-1, n_kf); kf_match_row: the keyframe's n_kf map points as rows in [-1, n_rows); rand: 4 * problem->rand_iterations
 * values in [0, rand_max]; problem's state fields are read (its indices and offsets ignored); best_mask: n_frame
 * bytes, in and out; inliers: n_frame bytes; frame_points (may be NULL): n_frame ints, written when a pose is
 * returned.  Every index, octave, parameter and the draw count (rand_iterations >= 1, every value in range) is checked
 * before anything is launched.  Draws that end inside the call's range are no error of the arguments: whether the
 * loop needs them depends on where it returns, so the call is launched and reports SPSLAM_PNP_OUT_OF_DRAWS, or
 * REFINED when a success comes first, as the batched form does. */
int spslam_pnp_solver(spslam_ctx* ctx, const spslam_keypoint* keys_un, int n_frame, const int32_t* match,
                      const int32_t* kf_match_row, int n_kf, const spslam_local_point* points,
                      const uint8_t* point_bad, int n_rows, const int32_t* rand, const spslam_pnp_params* params,
                      double probability, const spslam_pnp_problem* problem, spslam_pnp_result* result,
                      uint8_t* inliers, uint8_t* best_mask, int32_t* frame_points);

/* ---- SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) and the search of Fuse(pKF, Scw, vpPoints, th,
 * vpReplacePoint).  Both take spslam_fuse_problem records whose Tcw field holds Scw; the decomposition (:298-303,
 * :985-990: scw, Rcw = sRcw/scw, tcw = col3/scw, Ow) is made on the device.  The keyframe's uright is not read. */

/* Fuse with Scw: the same records, statuses and nfused = the count of best_dist <= TH_LOW as spslam_fuse_search,
 * without the chi-square test.  d_skip[out index] is the caller's flag isBad() || spAlreadyFound.count(pMP)
 * (:1005) as it was on entry; the search never reads GetMapPoint, so one call is a pure search over a snapshot,
 * and the walk :1082-1096 (vpReplacePoint[iMP] or AddObservation / AddMapPoint; a bad pMPinKF is counted with
 * nothing done) stays with the caller.  CONTRACT, as Fuse's: a point occurs at most once in a problem's list. */
int spslam_fuse_sim3_search_batch_device(spslam_ctx* ctx, int n_problems, const spslam_fuse_problem* d_problems,
                                         const spslam_local_point* d_points, int max_points,
                                         const spslam_keypoint* d_keys_un, const uint8_t* d_desc,
                                         const int32_t* d_grid_off, const int32_t* d_grid_idx, const int* d_counts,
                                         int cap, const uint8_t* d_skip, const spslam_fuse_params* params,
                                         spslam_fuse_result* d_results, int* d_nfused, void* hip_stream);
int spslam_fuse_sim3_search(spslam_ctx* ctx, const float* Scw, const spslam_local_point* points, int n_points,
                            const spslam_keypoint* keys_un, const uint8_t* desc, int n_kp, const int32_t* grid_off,
                            const int32_t* grid_idx, const uint8_t* skip, const spslam_fuse_params* params,
                            spslam_fuse_result* results, int* nfused);

/* SearchByProjection with Scw.  d_skip[out index]: isBad() || in spAlreadyFound (:317).  d_taken at problem *
 * cap (may be NULL: none): vpMatched[idx] != NULL on entry, per keyframe keypoint.  d_match at problem * cap, for
 * the keyframe's counts[kf_slot] keypoints: the index (in the problem's list) of the point newly assigned to the
 * keypoint, else -1; d_nmatches one int per problem.  The search of point i skips the keypoints that the points
 * before it took (:375, :396): a window kernel keeps each point's SPSLAM_PROJ_SIM3_KEYS smallest candidates among
 * the keypoints not taken on entry, and one wave per problem walks the points in order.  CONTRACT, as Fuse's: a
 * point occurs at most once in a problem's list (mnLoopPointForKF guarantees it in the reference).  params->th is
 * the reference's int th (10 in ComputeSim3) as a float.  cap <= 36000 (the walk's LDS). */
#define SPSLAM_PROJ_SIM3_KEYS 4
int spslam_search_by_projection_sim3_batch_device(spslam_ctx* ctx, int n_problems,
                                                  const spslam_fuse_problem* d_problems,
                                                  const spslam_local_point* d_points, int max_points,
                                                  const spslam_keypoint* d_keys_un, const uint8_t* d_desc,
                                                  const int32_t* d_grid_off, const int32_t* d_grid_idx,
                                                  const int* d_counts, int cap, const uint8_t* d_skip,
                                                  const uint8_t* d_taken, const spslam_fuse_params* params,
                                                  int32_t* d_match, int* d_nmatches, void* hip_stream);
/* taken: n_kp bytes or NULL; match: n_kp ints. */
int spslam_search_by_projection_sim3(spslam_ctx* ctx, const float* Scw, const spslam_local_point* points,
                                     int n_points, const spslam_keypoint* keys_un, const uint8_t* desc, int n_kp,
                                     const int32_t* grid_off, const int32_t* grid_idx, const uint8_t* skip,
                                     const uint8_t* taken, const spslam_fuse_params* params, int32_t* match,
                                     int* nmatches);

/* ---------------------------------------------------------------- the whole batched step
 * The throughput path as one call per step, for a C / C++ caller: GrabImageRGBD (Tracking.cc:208-229) ->
 * ORB extraction || ComputePlanesFromOrganizedPointCloud + GeneratePlanesFromBoundries (the RGB-D Frame
 * constructor) -> the tracking tail: Frame keypoint steps, SearchByProjection (TrackWithMotionModel,
 * Tracking.cc:951-975), AssociatePlanesByBoundary, the motion-model PoseOptimization graph and optimisation,
 * the outlier discard, SearchLocalPoints, the second association, the local-map graph and PoseOptimization
 * (TrackLocalMap, :1054-1068) -- the batched entry points above, enqueued on streams and events the step
 * object owns (the tail stream at high priority).  pipelined != 0: spslam_step_run(k) enqueues batch k+1's
 * extraction (grab + ORB on one stream, planes on another, into extraction set (k+1) % 2) beside batch k's
 * tail (set k % 2); a set is rewritten only after the tail that read it has finished.  spslam_step_prime
 * enqueues batch 0's extraction once before the first run.  pipelined == 0: each run is grab -> (planes ||
 * ORB) -> tail of `next`, set 0 only.  The context must be configured as for the single stages
 * (spslam_frame_configure, spslam_planes_configure; the vocabulary is not used).
 * Buffers: device memory; NULL members of the sets / tail are allocated by the step object (owned, freed by
 * spslam_step_destroy), others are the caller's; spslam_step_buffers returns all of them. */
typedef struct spslam_step_config {
    int32_t n_frames, width, height, kp_cap;      /* batch, image size, keypoint slots per frame */
    int32_t pipelined, tail_priority, orb_priority, planes_priority;
    spslam_grab_params grab;                      /* GrabImageRGBD: channels, mbRGB, depth type, mDepthMapFactor */
    spslam_match_params match;                    /* TrackWithMotionModel: th 15, checkOri, retry below 20 */
    spslam_local_params local;                    /* SearchLocalPoints: th 3, nn 0.8, viewing cos 0.5 */
    spslam_assoc_params assoc;                    /* Plane.Association* / Vertical / ParallelThreshold */
    spslam_plane_config pose;                     /* PoseOptimization Plane.* keys */
    float fx, fy, cx, cy, bf;                     /* camera (the graph's point edges) */
    int32_t pad;
} spslam_step_config;

typedef struct spslam_step_frames {               /* one batch of input frames (GrabImageRGBD's inputs) */
    const uint8_t* color;                         /* frame f at color + f * color_frame_stride bytes */
    size_t color_frame_stride;
    const void* depth;                            /* frame f at depth + f * depth_frame_stride elements */
    size_t depth_frame_stride;
    int32_t color_stride, depth_stride;           /* row strides: bytes / elements */
} spslam_step_frames;

typedef struct spslam_step_tracking {             /* one batch's tracking inputs (device) */
    const spslam_proj_frame* proj_frames;         /* last frames' map points (spslam_search_by_projection_batch_device) */
    const spslam_proj_point* proj_points;
    spslam_local_frame* local_frames;             /* local maps (spslam_search_local_points_batch_device; DISCARD writes Tcw) */
    const spslam_local_point* local_points;
    const spslam_assoc_frame* assoc_frames1;      /* first association (motion-model pose) */
    spslam_assoc_frame* assoc_frames2;            /* second (DISCARD writes Tcw), carry = 1 */
    const spslam_map_plane* map;
    const float* boundary_xyz;
    int32_t max_proj_points, max_local_points, max_map, pad;
} spslam_step_tracking;

typedef struct spslam_step_set {                  /* extraction outputs of one batch (the batch layouts above) */
    uint8_t* gray;
    float* depth;
    spslam_keypoint* kps;
    uint8_t* desc;
    int* counts;
    spslam_plane* planes;
    int* plane_counts;
    int32_t* inliers;
    int32_t* contours;
    spslam_supposed_plane* supposed;
    int* supposed_counts;
    int32_t* lines;
    float* patch;
} spslam_step_set;

typedef struct spslam_step_tail {                 /* the tracking tail's buffers and outputs */
    spslam_keypoint* keys_un;
    float* mv_depth;
    float* uright;
    int32_t* grid_off;
    int32_t* grid_idx;
    int32_t* match;
    int* nmatches;
    uint8_t* taken;
    int32_t* local_match;
    int* local_nmatches;
    int32_t* edge_of_kp;
    int32_t* assoc[2][3];                         /* [association][match, parallel, vertical] */
    int* new_plane[2];
    spslam_pose_problem* problems[2];             /* [0] motion model, [1] local map */
    spslam_point_obs* points[2];
    spslam_plane_obs* planes[2];
    uint8_t* point_outlier[2];
    uint8_t* plane_outlier[2];
    spslam_pose_result* results[2];
} spslam_step_tail;

typedef struct spslam_step spslam_step;
int spslam_step_create(spslam_ctx* ctx, const spslam_step_config* cfg, const spslam_step_set* sets /* [2], may be NULL */,
                       const spslam_step_tail* tail /* may be NULL */, spslam_step** out);
int spslam_step_buffers(const spslam_step* step, spslam_step_set* sets /* [2] */, spslam_step_tail* tail);
int spslam_step_prime(spslam_step* step, const spslam_step_frames* first);
int spslam_step_run(spslam_step* step, const spslam_step_frames* next, const spslam_step_tracking* tracking);
int spslam_step_sync(spslam_step* step);          /* host waits for every stream of the step */
void* spslam_step_stream(const spslam_step* step); /* the tail stream (hipStream_t) */
void spslam_step_destroy(spslam_step* step);

/* Measurement: when enabled, every kernel kind launched by this context is
 * bracketed by HIP events on its launch stream.  spslam_kernel_times returns,
 * per kind, the summed event time (ms) and number of timed launches since the
 * last spslam_set_timing call (it waits for the recorded events).  Returns the
 * number of kinds written; spslam_kernel_name(kind) names the kernel. */
int spslam_set_timing(spslam_ctx* ctx, int enable);
int spslam_kernel_times(spslam_ctx* ctx, double* total_ms, long long* launches, int max_kinds);
const char* spslam_kernel_name(int kind);

#ifdef __cplusplus
}
#endif

#endif /* SPSLAM_GPU_H */
