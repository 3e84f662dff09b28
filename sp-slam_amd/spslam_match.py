"""ctypes binding of the projection-matching part of include/spslam_gpu.h
(ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono),
src/ORBmatcher.cc:1328-1470, as TrackWithMotionModel calls it, on gfx950)."""
from __future__ import annotations

import ctypes

import numpy as np

import spslam_gpu

PROJ_POINT_DTYPE = np.dtype([("xw", "<f4", 3), ("angle", "<f4"), ("octave", "<i4"), ("n_obs", "<i4"),
                             ("last_index", "<i4"), ("id", "<i4"), ("desc", "u1", 32)])
assert PROJ_POINT_DTYPE.itemsize == 64
PROJ_FRAME_DTYPE = np.dtype([("Tcw", "<f4", 16), ("Tlw", "<f4", 16), ("point_offset", "<i4"), ("n_points", "<i4"),
                             ("pad", "<i4", 2)])
assert PROJ_FRAME_DTYPE.itemsize == 144


def _ptr(a):
    """The address of an array, None for an absent or empty one."""
    return a.ctypes.data if a is not None and a.size else None


def _current_frame(keys_un, desc, uright, grid_off, grid_idx):
    """The current frame of a window search's host form as contiguous arrays of the C types."""
    return (np.ascontiguousarray(keys_un, spslam_gpu.KEYPOINT_DTYPE),
            np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), np.ascontiguousarray(uright, np.float32),
            np.ascontiguousarray(grid_off, np.int32), np.ascontiguousarray(grid_idx, np.int32))


class MatchParams(ctypes.Structure):
    _fields_ = [("th", ctypes.c_float), ("mono", ctypes.c_int), ("check_orientation", ctypes.c_int),
                ("retry_below", ctypes.c_int)]


# Tracking::TrackWithMotionModel for RGB-D: th = 15, not mono, checkOri, retry below 20 matches
MOTION_MODEL = (15.0, 0, 1, 20)

spslam_gpu.EXPORTED += ["spslam_search_by_projection", "spslam_search_by_projection_batch_device"]


def _bind(lib):
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.spslam_search_by_projection.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    lib.spslam_search_by_projection_batch_device.argtypes = [vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp,
                                                             vp, vp]


class Matcher:
    """GPU SearchByProjection on a context configured with spslam_frame_configure."""

    def __init__(self, ex: spslam_gpu.OrbExtractor, params=MOTION_MODEL):
        self.ex = ex
        _bind(ex.lib)
        self.params = MatchParams(*params)

    def __call__(self, frame, points, keys_un, desc, uright, grid_off, grid_idx):
        fr = np.ascontiguousarray(frame, PROJ_FRAME_DTYPE).reshape(())
        pts = np.ascontiguousarray(points, PROJ_POINT_DTYPE)
        k, d, ur, go, gi = _current_frame(keys_un, desc, uright, grid_off, grid_idx)
        n = len(k)
        match = np.zeros(max(n, 1), np.int32)
        nm = ctypes.c_int(0)
        self.ex._check(self.ex.lib.spslam_search_by_projection(
            self.ex.ctx, fr.ctypes.data, _ptr(pts), _ptr(k), _ptr(d), _ptr(ur), n, go.ctypes.data, _ptr(gi),
            ctypes.byref(self.params), match.ctypes.data, ctypes.byref(nm)))
        return match[:n], nm.value

    def batch_device(self, n_frames, d_frames, d_points, max_points, d_keys_un, d_desc, d_uright, d_grid_off,
                     d_grid_idx, d_counts, cap, d_match, d_nmatches, stream=0):
        self.ex._check(self.ex.lib.spslam_search_by_projection_batch_device(
            self.ex.ctx, n_frames, d_frames, d_points, max_points, d_keys_un, d_desc, d_uright, d_grid_off,
            d_grid_idx, d_counts, cap, ctypes.byref(self.params), d_match, d_nmatches, stream or None))


LOCAL_POINT_DTYPE = np.dtype([("xw", "<f4", 3), ("normal", "<f4", 3), ("min_dist", "<f4"), ("max_dist", "<f4"),
                              ("id", "<i4"), ("n_obs", "<i4"), ("pad", "<i4", 2), ("desc", "u1", 32)])
assert LOCAL_POINT_DTYPE.itemsize == 80
LOCAL_FRAME_DTYPE = np.dtype([("Tcw", "<f4", 16), ("point_offset", "<i4"), ("n_points", "<i4"), ("seen_offset", "<i4"),
                              ("stamp", "<i4")])
assert LOCAL_FRAME_DTYPE.itemsize == 80


class LocalParams(ctypes.Structure):
    _fields_ = [("th", ctypes.c_float), ("nn_ratio", ctypes.c_float), ("view_cos_limit", ctypes.c_float),
                ("pad", ctypes.c_int)]


# Tracking::SearchLocalPoints for RGB-D: th = 3, ORBmatcher(0.8), isInFrustum(pMP, 0.5)
SEARCH_LOCAL = (3.0, 0.8, 0.5, 0)

spslam_gpu.EXPORTED += ["spslam_search_local_points", "spslam_search_local_points_batch_device"]


class LocalMatcher:
    """GPU Tracking::SearchLocalPoints on a context configured with spslam_frame_configure."""

    def __init__(self, ex: spslam_gpu.OrbExtractor, params=SEARCH_LOCAL):
        self.ex = ex
        vp, ci = ctypes.c_void_p, ctypes.c_int
        ex.lib.spslam_search_local_points.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp]
        ex.lib.spslam_search_local_points_batch_device.argtypes = [vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci,
                                                                   vp, vp, vp, vp, vp, vp, vp]
        self.params = LocalParams(*params)

    def __call__(self, frame, points, keys_un, desc, uright, grid_off, grid_idx, taken=None):
        fr = np.ascontiguousarray(frame, LOCAL_FRAME_DTYPE).reshape(())
        pts = np.ascontiguousarray(points, LOCAL_POINT_DTYPE)
        k, d, ur, go, gi = _current_frame(keys_un, desc, uright, grid_off, grid_idx)
        tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
        n = len(k)
        match = np.zeros(max(n, 1), np.int32)
        inv = np.zeros(max(len(pts), 1), np.uint8)
        nm = ctypes.c_int(0)
        self.ex._check(self.ex.lib.spslam_search_local_points(
            self.ex.ctx, fr.ctypes.data, _ptr(pts), _ptr(k), _ptr(d), _ptr(ur), n, go.ctypes.data, _ptr(gi), _ptr(tk),
            ctypes.byref(self.params), match.ctypes.data, ctypes.byref(nm), inv.ctypes.data))
        return match[:n], nm.value, inv[:len(pts)].astype(bool)

    def batch_device(self, n_frames, d_frames, d_points, max_points, d_keys_un, d_desc, d_uright, d_grid_off,
                     d_grid_idx, d_counts, cap, d_taken, d_match, d_nmatches, d_in_view=0, stream=0, d_seen=0):
        self.ex._check(self.ex.lib.spslam_search_local_points_batch_device(
            self.ex.ctx, n_frames, d_frames, d_points, max_points, d_keys_un, d_desc, d_uright, d_grid_off,
            d_grid_idx, d_counts, cap, d_taken or None, ctypes.byref(self.params), d_match, d_nmatches,
            d_in_view or None, d_seen or None, stream or None))


# ---------------------------------------------------------------- LocalMapping: Fuse search, map-point refresh
FUSE_PROBLEM_DTYPE = np.dtype([("Tcw", "<f4", 16), ("kf_slot", "<i4"), ("point_offset", "<i4"), ("n_points", "<i4"),
                               ("out_offset", "<i4")])
assert FUSE_PROBLEM_DTYPE.itemsize == 80
FUSE_RESULT_DTYPE = np.dtype([("best_idx", "<i4"), ("best_dist", "<i2"), ("level", "u1"), ("status", "u1")])
assert FUSE_RESULT_DTYPE.itemsize == 8
FUSE_SEARCHED, FUSE_SKIPPED, FUSE_BEHIND, FUSE_OUTSIDE_IMAGE, FUSE_OUT_OF_RANGE, FUSE_VIEW_ANGLE, \
    FUSE_NO_CANDIDATES = range(7)
TH_LOW = 50


class FuseParams(ctypes.Structure):
    _fields_ = [("th", ctypes.c_float), ("pad", ctypes.c_int)]


# LocalMapping::SearchInNeighbors: matcher.Fuse(pKFi, vpMapPointMatches) with the default th = 3.0
FUSE = (3.0, 0)

spslam_gpu.EXPORTED += ["spslam_fuse_search", "spslam_fuse_search_batch_device"]


class FuseSearch:
    """GPU search of ORBmatcher::Fuse(pKF, vpMapPoints, th) on a context configured with spslam_frame_configure;
    the map mutation (Replace / AddObservation) stays with the caller."""

    def __init__(self, ex: spslam_gpu.OrbExtractor, params=FUSE):
        self.ex = ex
        vp, ci = ctypes.c_void_p, ctypes.c_int
        ex.lib.spslam_fuse_search.argtypes = [vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
        ex.lib.spslam_fuse_search_batch_device.argtypes = [vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp,
                                                           vp, vp]
        self.params = FuseParams(*params)

    def __call__(self, Tcw, points, keys_un, desc, uright, grid_off, grid_idx, skip=None):
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        pts = np.ascontiguousarray(points, LOCAL_POINT_DTYPE)
        k, d, ur, go, gi = _current_frame(keys_un, desc, uright, grid_off, grid_idx)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        res = np.zeros(max(len(pts), 1), FUSE_RESULT_DTYPE)
        nf = ctypes.c_int(0)
        self.ex._check(self.ex.lib.spslam_fuse_search(
            self.ex.ctx, T.ctypes.data, _ptr(pts), len(pts), _ptr(k), _ptr(d), _ptr(ur), len(k), go.ctypes.data,
            _ptr(gi), _ptr(sk), ctypes.byref(self.params), res.ctypes.data, ctypes.byref(nf)))
        return res[:len(pts)], nf.value

    def batch_device(self, n_problems, d_problems, d_points, max_points, d_keys_un, d_desc, d_uright, d_grid_off,
                     d_grid_idx, d_counts, cap, d_skip, d_results, d_nfused, stream=0):
        self.ex._check(self.ex.lib.spslam_fuse_search_batch_device(
            self.ex.ctx, n_problems, d_problems, d_points, max_points, d_keys_un, d_desc, d_uright, d_grid_off,
            d_grid_idx, d_counts, cap, d_skip or None, ctypes.byref(self.params), d_results, d_nfused,
            stream or None))


POINT_MAX_OBS = 128
REFRESH_DESCRIPTOR, REFRESH_NORMAL_DEPTH = 1, 2
REFRESH_DONE, REFRESH_UNTOUCHED, REFRESH_CAPACITY = 0, 1, 2
ERR_CAPACITY = -2
# the tables of spslam_point_refresh_map before `points`, in its order
REFRESH_MAP_TABLES = (("kf_Tcw", np.float32), ("kf_slot", np.int32), ("kf_bad", np.uint8), ("obs_off", np.int32),
                      ("obs_kf", np.int32), ("obs_kp", np.int32), ("ref_kf", np.int32), ("point_bad", np.uint8))


class PointRefreshMap(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _ in REFRESH_MAP_TABLES] + [("points", ctypes.c_void_p)]


spslam_gpu.EXPORTED += ["spslam_map_points_refresh", "spslam_map_points_refresh_batch_device"]


class PointRefresh:
    """GPU MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth on rows of the local-point table."""

    def __init__(self, ex: spslam_gpu.OrbExtractor):
        self.ex = ex
        vp, ci = ctypes.c_void_p, ctypes.c_int
        ex.lib.spslam_map_points_refresh.argtypes = [vp, vp, ci, ci, vp, ci, ci, vp, vp, ci, ci, vp]
        ex.lib.spslam_map_points_refresh_batch_device.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, vp, vp]

    def __call__(self, tables, points, rows, what, keys_un, desc, cap):
        """tables: the REFRESH_MAP_TABLES arrays by name (kf_bad / point_bad may be None); points: the table, a copy
        of which is refreshed and returned with the status per listed row and the return code (0, or ERR_CAPACITY
        with every other row done)."""
        a = {name: None if tables.get(name) is None else np.ascontiguousarray(tables[name], dt).reshape(-1)
             for name, dt in REFRESH_MAP_TABLES}
        pts = np.array(points, LOCAL_POINT_DTYPE)
        rw = np.ascontiguousarray(rows, np.int32)
        k = np.ascontiguousarray(keys_un, spslam_gpu.KEYPOINT_DTYPE).reshape(-1)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        assert len(k) % cap == 0 and len(d) == len(k)
        status = np.full(max(len(rw), 1), 0xEE, np.uint8)
        m = PointRefreshMap(points=_ptr(pts), **{name: _ptr(a[name]) for name, _ in REFRESH_MAP_TABLES})
        rc = self.ex.lib.spslam_map_points_refresh(self.ex.ctx, ctypes.byref(m), len(a["kf_slot"]), len(pts), _ptr(rw),
                                                   len(rw), what, _ptr(k), _ptr(d), cap, len(k) // cap,
                                                   status.ctypes.data)
        if rc != ERR_CAPACITY:
            self.ex._check(rc)
        return pts, status[:len(rw)], rc

    def batch_device(self, refresh_map: PointRefreshMap, d_rows, n, what, d_keys_un, d_desc, cap, d_status, stream=0):
        self.ex._check(self.ex.lib.spslam_map_points_refresh_batch_device(
            self.ex.ctx, ctypes.byref(refresh_map), d_rows, n, what, d_keys_un or None, d_desc or None, cap, d_status,
            stream or None))


# ---------------------------------------------------------------- LocalMapping: CreateNewMapPoints
TRI_PAIR_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("Tcw1", "<f4", 12), ("Tcw2", "<f4", 12), ("Ow1", "<f4", 3),
                           ("Ow2", "<f4", 3), ("F12", "<f4", 9), ("out_offset", "<i4"), ("flags", "<i4")])
assert TRI_PAIR_DTYPE.itemsize == 172
TRI_RESULT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("idx2", "<i4"), ("status", "u1"),
                             ("source", "u1"), ("pad", "<u2")])
assert TRI_RESULT_DTYPE.itemsize == 20
TRI_NEW, TRI_NO_MATCH, TRI_LOW_PARALLAX, TRI_W_ZERO, TRI_BEHIND_1, TRI_BEHIND_2, TRI_REPROJ_1, TRI_REPROJ_2, \
    TRI_ZERO_DIST, TRI_SCALE = range(10)
TRI_FROM_SVD, TRI_FROM_STEREO_1, TRI_FROM_STEREO_2 = range(3)
TRI_PAIR_SEARCHED, TRI_PAIR_SKIPPED, TRI_PAIR_SHORT_BASELINE = range(3)
TRI_PAIR_SKIP = 1
TRI_MAX_CAP = 8192
# the arrays of spslam_tri_side before `cap`, in its order
TRI_SIDE_ARRAYS = ("keys", "keys_un", "uright", "depth", "desc", "has_point", "counts", "fv_nodes", "fv_start",
                   "fv_features", "n_fv")


class TriSide(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in TRI_SIDE_ARRAYS] + [("cap", ctypes.c_int32),
                                                                         ("pad", ctypes.c_int32)]


class TriKeyframe(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ("keys", "keys_un", "uright", "depth", "desc", "has_point",
                                                     "fv_nodes", "fv_start", "fv_features")] + \
               [("n", ctypes.c_int32), ("n_fv", ctypes.c_int32), ("Tcw", ctypes.c_float * 12),
                ("Ow", ctypes.c_float * 3), ("pad", ctypes.c_int32)]


spslam_gpu.EXPORTED += ["spslam_search_for_triangulation", "spslam_search_for_triangulation_batch_device",
                        "spslam_triangulate", "spslam_triangulate_batch_device",
                        "spslam_create_new_points_batch_device"]


def _bind_tri(lib):
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.spslam_search_for_triangulation.argtypes = [vp, vp, vp, vp, vp, ci, ci]
    lib.spslam_search_for_triangulation_batch_device.argtypes = [vp, ci, vp, vp, ci, ci, vp, vp, vp]
    lib.spslam_triangulate.argtypes = [vp, vp, vp, vp, ci, vp, vp]
    lib.spslam_triangulate_batch_device.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, vp]
    lib.spslam_create_new_points_batch_device.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp]


class _TriHost:
    """A keyframe dict (keys, kun, ur, depth, desc, has, fv = dict(nodes, start, features), Tcw [3x4 or 4x4], Ow)
    as a spslam_tri_keyframe; holds the arrays alive."""

    def __init__(self, kf):
        n = len(kf["kun"])
        self.a = [np.ascontiguousarray(kf["keys"], spslam_gpu.KEYPOINT_DTYPE),
                  np.ascontiguousarray(kf["kun"], spslam_gpu.KEYPOINT_DTYPE),
                  np.ascontiguousarray(kf["ur"], np.float32), np.ascontiguousarray(kf["depth"], np.float32),
                  np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32),
                  np.ascontiguousarray(kf["has"], np.uint8),
                  np.ascontiguousarray(kf["fv"]["nodes"], np.uint32),
                  np.ascontiguousarray(kf["fv"]["start"], np.int32),
                  np.ascontiguousarray(kf["fv"]["features"], np.int32)]
        T = np.asarray(kf["Tcw"], np.float32).reshape(-1, 4)[:3].reshape(12)
        self.rec = TriKeyframe(*[_ptr(x) for x in self.a], n, len(self.a[6]), (ctypes.c_float * 12)(*T.tolist()),
                               (ctypes.c_float * 3)(*np.asarray(kf["Ow"], np.float32).tolist()), 0)


class SearchForTriangulation:
    """GPU ORBmatcher::SearchForTriangulation on a context configured with spslam_frame_configure."""

    def __init__(self, ex: spslam_gpu.OrbExtractor):
        self.ex = ex
        _bind_tri(ex.lib)

    def __call__(self, kf1, kf2, F12, only_stereo=False, check_orientation=False):
        """Returns (vMatchedPairs [nmatches, 2] in idx1 order, nmatches)."""
        a, b = _TriHost(kf1), _TriHost(kf2)
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        pairs = np.zeros((max(a.rec.n, 1), 2), np.int32)
        rc = self.ex.lib.spslam_search_for_triangulation(self.ex.ctx, ctypes.byref(a.rec), ctypes.byref(b.rec),
                                                         F.ctypes.data, pairs.ctypes.data, int(only_stereo),
                                                         int(check_orientation))
        if rc < 0:
            self.ex._check(rc)
        return pairs[:rc], rc

    def batch_device(self, n_pairs, d_pairs, side: TriSide, only_stereo, check_orientation, d_match12, d_nmatches,
                     stream=0):
        self.ex._check(self.ex.lib.spslam_search_for_triangulation_batch_device(
            self.ex.ctx, n_pairs, d_pairs, ctypes.byref(side), int(only_stereo), int(check_orientation), d_match12,
            d_nmatches, stream or None))


class Triangulate:
    """GPU triangulation and checks of LocalMapping::CreateNewMapPoints (:298-443) per matched pair."""

    def __init__(self, ex: spslam_gpu.OrbExtractor):
        self.ex = ex
        _bind_tri(ex.lib)

    def __call__(self, kf1, kf2, matched_pairs):
        """Returns (one TRI_RESULT_DTYPE record per pair, n_new)."""
        a, b = _TriHost(kf1), _TriHost(kf2)
        mp = np.ascontiguousarray(matched_pairs, np.int32).reshape(-1, 2)
        res = np.zeros(max(len(mp), 1), TRI_RESULT_DTYPE)
        n_new = ctypes.c_int(0)
        self.ex._check(self.ex.lib.spslam_triangulate(self.ex.ctx, ctypes.byref(a.rec), ctypes.byref(b.rec),
                                                      mp.ctypes.data if len(mp) else None, len(mp),
                                                      res.ctypes.data, ctypes.byref(n_new)))
        return res[:len(mp)], n_new.value

    def batch_device(self, n_pairs, d_pairs, side: TriSide, d_match12, mark, d_results, d_n_new, stream=0):
        self.ex._check(self.ex.lib.spslam_triangulate_batch_device(
            self.ex.ctx, n_pairs, d_pairs, ctypes.byref(side), d_match12, int(mark), d_results, d_n_new,
            stream or None))


class CreateNewPoints:
    """One neighbour round of LocalMapping::CreateNewMapPoints for a batch of sequences: baseline test, search,
    triangulation, has-point marks.  The pairs of one call must not share a keyframe slot; calls on one stream are
    ordered.  The map mutation stays with the caller."""

    def __init__(self, ex: spslam_gpu.OrbExtractor):
        self.ex = ex
        _bind_tri(ex.lib)

    def batch_device(self, n_pairs, d_pairs, side: TriSide, d_match12, d_nmatches, d_results, d_n_new,
                     d_pair_status, stream=0):
        self.ex._check(self.ex.lib.spslam_create_new_points_batch_device(
            self.ex.ctx, n_pairs, d_pairs, ctypes.byref(side), d_match12, d_nmatches, d_results, d_n_new,
            d_pair_status, stream or None))


# ---------------------------------------------------------------- LocalMapping: covisibility graph, the cullings
COVIS_MAX_KF, COVIS_BEST = 1024, 10
COVIS_UPDATED, COVIS_EMPTY = 0, 1
COVIS_TH = 15                              # KeyFrame::UpdateConnections' th
CULL_KEPT, CULL_CULLED, CULL_DEFERRED, CULL_SKIPPED = range(4)
CULL_RAN, CULL_NEW_PLANE = 0, 1
POINT_CULL_KEEP, POINT_CULL_DROP, POINT_CULL_BAD_RATIO, POINT_CULL_BAD_OBS, POINT_CULL_EXPIRED = range(5)
COVIS_PROBLEM_DTYPE = np.dtype([("kf_base", "<i4"), ("row_base", "<i4"), ("kf", "<i4"), ("n_kf", "<i4")])
COVIS_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_ordered", "<i4"), ("new_parent", "<i4"), ("n_resorted", "<i4")])
CULL_PROBLEM_DTYPE = np.dtype([("kf_base", "<i4"), ("row_base", "<i4"), ("kf", "<i4"), ("n_kf", "<i4"),
                               ("out_offset", "<i4"), ("pad", "<i4", 3)])
CULL_RECORD_DTYPE = np.dtype([("kf", "<i4"), ("n_mps", "<i4"), ("n_redundant", "<i4"), ("status", "<i4")])
CULL_SUMMARY_DTYPE = np.dtype([("n_candidates", "<i4"), ("status", "<i4")])
assert COVIS_PROBLEM_DTYPE.itemsize == 16 and COVIS_RESULT_DTYPE.itemsize == 16
assert CULL_PROBLEM_DTYPE.itemsize == 32 and CULL_RECORD_DTYPE.itemsize == 16 and CULL_SUMMARY_DTYPE.itemsize == 8
# the tables of spslam_covis_map, spslam_covis_graph (before `stride`) and spslam_point_cull_map, in their order
COVIS_MAP_TABLES = (("match_off", np.int32), ("match_row", np.int32), ("obs_off", np.int32), ("obs_kf", np.int32),
                    ("obs_kp", np.int32), ("kf_slot", np.int32), ("point_bad", np.uint8), ("points", LOCAL_POINT_DTYPE))
COVIS_GRAPH_TABLES = (("weights", np.int32), ("ordered", np.int32), ("ordered_w", np.int32), ("n_ordered", np.int32),
                      ("covis", np.int32), ("parent", np.int32), ("first_connection", np.uint8))
POINT_CULL_TABLES = (("found", np.int32), ("visible", np.int32), ("first_kf", np.int32), ("point_bad", np.uint8),
                     ("points", LOCAL_POINT_DTYPE))


class CovisMap(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _ in COVIS_MAP_TABLES]


class CovisGraph(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _ in COVIS_GRAPH_TABLES] + [("stride", ctypes.c_int32),
                                                                             ("pad", ctypes.c_int32)]


class CullParams(ctypes.Structure):
    _fields_ = [("th_depth", ctypes.c_float), ("th_obs", ctypes.c_int32)]


class PointCullMap(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _ in POINT_CULL_TABLES]


spslam_gpu.EXPORTED += ["spslam_covis_update_connections", "spslam_covis_update_connections_batch_device",
                        "spslam_keyframe_culling", "spslam_keyframe_culling_batch_device",
                        "spslam_map_point_culling", "spslam_map_point_culling_batch_device"]


def _bind_covis(lib):
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.spslam_covis_update_connections.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp]
    lib.spslam_covis_update_connections_batch_device.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp]
    lib.spslam_keyframe_culling.argtypes = [vp, vp, ci, ci, ci, vp, ci, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp]
    lib.spslam_keyframe_culling_batch_device.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    lib.spslam_map_point_culling.argtypes = [vp, vp, ci, vp, ci, ci, ci, vp]
    lib.spslam_map_point_culling_batch_device.argtypes = [vp, vp, vp, vp, ci, ci, vp, vp]


def _tables(tables, spec):
    """The named arrays of a table spec, contiguous in their C types (None stays None)."""
    return {name: None if tables.get(name) is None else np.ascontiguousarray(tables[name], dt).reshape(-1)
            for name, dt in spec}


class CovisUpdateConnections:
    """GPU KeyFrame::UpdateConnections with AddConnection / UpdateBestCovisibles on the device-resident
    spslam_covis_graph.  A call holds at most one problem per sequence; AddChild stays with the caller."""

    def __init__(self, ex: spslam_gpu.OrbExtractor, th=COVIS_TH):
        self.ex, self.th = ex, th
        _bind_covis(ex.lib)

    def __call__(self, tables, graph, stride, kf):
        """One keyframe on host arrays: tables by COVIS_MAP_TABLES name (match / observer CSRs, point_bad), graph by
        COVIS_GRAPH_TABLES name.  Returns (the graph after, as copies; the result record)."""
        a = _tables(tables, COVIS_MAP_TABLES)
        g = {name: np.array(graph[name], dt).reshape(-1) for name, dt in COVIS_GRAPH_TABLES}
        res = np.zeros((), COVIS_RESULT_DTYPE)
        m = CovisMap(**{name: _ptr(a[name]) for name, _ in COVIS_MAP_TABLES})
        G = CovisGraph(stride=stride, **{name: _ptr(g[name]) for name, _ in COVIS_GRAPH_TABLES})
        self.ex._check(self.ex.lib.spslam_covis_update_connections(
            self.ex.ctx, ctypes.byref(m), len(a["match_off"]) - 1, len(a["obs_off"]) - 1, kf, self.th,
            ctypes.byref(G), res.ctypes.data))
        return g, res

    def batch_device(self, n_problems, d_problems, covis_map: CovisMap, graph: CovisGraph, d_results, stream=0):
        self.ex._check(self.ex.lib.spslam_covis_update_connections_batch_device(
            self.ex.ctx, n_problems, d_problems, ctypes.byref(covis_map), ctypes.byref(graph), self.th, d_results,
            stream or None))


# LocalMapping::KeyFrameCulling: thObs = 3; mThDepth is the camera's (bf * ThDepth / fx)
CULL_TH_OBS = 3


class KeyFrameCulling:
    """GPU LocalMapping::KeyFrameCulling (RGB-D): verdicts only, the caller applies SetBadFlag in order."""

    def __init__(self, ex: spslam_gpu.OrbExtractor, th_depth, th_obs=CULL_TH_OBS):
        self.ex = ex
        _bind_covis(ex.lib)
        self.params = CullParams(th_depth, th_obs)

    def __call__(self, tables, kf, ordered, keys_un, uright, depth, cap, new_plane, not_erase=None):
        """One current keyframe on host arrays.  Returns (records, summary)."""
        a = _tables(tables, COVIS_MAP_TABLES)
        k = np.ascontiguousarray(keys_un, spslam_gpu.KEYPOINT_DTYPE).reshape(-1)
        ur = np.ascontiguousarray(uright, np.float32).reshape(-1)
        dp = np.ascontiguousarray(depth, np.float32).reshape(-1)
        assert len(k) % cap == 0 and len(ur) == len(k) == len(dp)
        od = np.ascontiguousarray(ordered, np.int32)
        npl = np.ascontiguousarray(new_plane, np.uint8)
        ne = None if not_erase is None else np.ascontiguousarray(not_erase, np.uint8)
        rec = np.zeros(max(len(od), 1), CULL_RECORD_DTYPE)
        summary = np.zeros((), CULL_SUMMARY_DTYPE)
        m = CovisMap(**{name: _ptr(a[name]) for name, _ in COVIS_MAP_TABLES})
        self.ex._check(self.ex.lib.spslam_keyframe_culling(
            self.ex.ctx, ctypes.byref(m), len(a["match_off"]) - 1, len(a["obs_off"]) - 1, kf, _ptr(od), len(od),
            _ptr(k), _ptr(ur), _ptr(dp), cap, len(k) // cap, _ptr(npl), _ptr(ne), ctypes.byref(self.params),
            rec.ctypes.data, summary.ctypes.data))
        return rec[:int(summary["n_candidates"])], summary

    def batch_device(self, n_problems, d_problems, covis_map: CovisMap, graph: CovisGraph, d_keys_un, d_uright,
                     d_depth, cap, d_new_plane, d_not_erase, d_records, d_summaries, stream=0):
        self.ex._check(self.ex.lib.spslam_keyframe_culling_batch_device(
            self.ex.ctx, n_problems, d_problems, ctypes.byref(covis_map), ctypes.byref(graph), d_keys_un, d_uright,
            d_depth, cap, d_new_plane, d_not_erase or None, ctypes.byref(self.params), d_records, d_summaries,
            stream or None))


class MapPointCulling:
    """GPU LocalMapping::MapPointCulling: one POINT_CULL_* verdict per list entry."""

    def __init__(self, ex: spslam_gpu.OrbExtractor, th_obs=CULL_TH_OBS):
        self.ex, self.th_obs = ex, th_obs
        _bind_covis(ex.lib)

    def __call__(self, tables, rows, cur_kf_id):
        a = _tables(tables, POINT_CULL_TABLES)
        rw = np.ascontiguousarray(rows, np.int32)
        verdict = np.full(max(len(rw), 1), 0xEE, np.uint8)
        m = PointCullMap(**{name: _ptr(a[name]) for name, _ in POINT_CULL_TABLES})
        self.ex._check(self.ex.lib.spslam_map_point_culling(self.ex.ctx, ctypes.byref(m), len(a["points"]), _ptr(rw),
                                                            len(rw), cur_kf_id, self.th_obs, verdict.ctypes.data))
        return verdict[:len(rw)]

    def batch_device(self, point_map: PointCullMap, d_rows, d_cur_kf_id, n, d_verdict, stream=0):
        self.ex._check(self.ex.lib.spslam_map_point_culling_batch_device(
            self.ex.ctx, ctypes.byref(point_map), d_rows or None, d_cur_kf_id or None, n, self.th_obs,
            d_verdict or None, stream or None))
