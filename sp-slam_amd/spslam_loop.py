"""ctypes binding of the loop-closing entries of include/spslam_gpu.h: the four ORBmatcher overloads that
LoopClosing::ComputeSim3 and SearchAndFuse call -- SearchByBoW(KeyFrame*, KeyFrame*), SearchBySim3,
SearchByProjection(pKF, Scw, ...) and the search of Fuse(pKF, Scw, ...) -- on keyframe slots, FeatureVectors and the
map-point table that stay on the device -- and Sim3Solver between the first two (RANSAC over Horn's alignment, the
draws an input), and Optimizer::OptimizeSim3 with Scw after SearchBySim3 (g2o's Levenberg-Marquardt on one Sim3 vertex,
fixed scale).  The consistency groups and the map mutation are the caller's."""
from __future__ import annotations

import ctypes

import numpy as np

import spslam_gpu
from spslam_bow import BowParams, BowSide
from spslam_match import (FUSE_PROBLEM_DTYPE, FUSE_RESULT_DTYPE, LOCAL_POINT_DTYPE, FuseParams, _ptr)

PROJ_SIM3_KEYS = 4           # SPSLAM_PROJ_SIM3_KEYS: keys kept per point by SearchByProjection(pKF, Scw)'s window kernel
POINTS_PER_GROUP = 64        # points per workgroup of the three projection searches (256 threads, 4 lanes per point)
BOW_WAVES = 4                # waves per workgroup of the SearchByBoW kernel: shared nodes in flight
SIM3_PAIR_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("match_offset", "<i4"), ("result_offset", "<i4"),
                            ("s12", "<f4"), ("R12", "<f4", 9), ("t12", "<f4", 3), ("pad", "<i4", 3)])
assert SIM3_PAIR_DTYPE.itemsize == 80
# the tables of spslam_sim3_map, in its order
SIM3_MAP_TABLES = (("kf_Tcw", np.float32), ("kf_slot", np.int32), ("match_off", np.int32), ("match_row", np.int32),
                   ("point_bad", np.uint8), ("points", LOCAL_POINT_DTYPE))
# ComputeSim3: SearchBySim3 at th 7.5 (LoopClosing.cc:325), SearchByProjection at th 10 (:393); SearchAndFuse: th 4 (:700)
TH_SIM3, TH_PROJECTION, TH_FUSE = 7.5, 10.0, 4.0

# Sim3Solver: struct spslam_sim3_problem / spslam_sim3_result, the statuses, glibc's RAND_MAX
SIM3_PROBLEM_DTYPE = np.dtype([("kf1", "<i4"), ("kf2", "<i4"), ("match_offset", "<i4"), ("rand_offset", "<i4"),
                               ("inlier_offset", "<i4"), ("iterations_done", "<i4"), ("best_inliers", "<i4"),
                               ("n_iterations", "<i4")])
SIM3_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("iterations_done", "<i4"), ("best_inliers", "<i4"),
                              ("n_inliers", "<i4"), ("s12", "<f4"), ("R12", "<f4", 9), ("t12", "<f4", 3),
                              ("T12", "<f4", 16)])
assert SIM3_PROBLEM_DTYPE.itemsize == 32 and SIM3_RESULT_DTYPE.itemsize == 136
SIM3_FOUND, SIM3_NOT_YET, SIM3_NO_MORE = 0, 1, 2
SIM3_MAX_ITERATIONS = 4096
RAND_MAX = 2147483647

# OptimizeSim3: struct spslam_sim3_opt_result, the statuses, ComputeSim3's th2 and acceptance count
SIM3_OPT_RESULT_DTYPE = np.dtype([("n_in", "<i4"), ("n_corr", "<i4"), ("n_bad", "<i4"), ("status", "<i4"),
                                  ("accepted", "<i4"), ("iterations1", "<i4"), ("trials1", "<i4"), ("iterations2", "<i4"),
                                  ("trials2", "<i4"), ("pad", "<i4"), ("S12", "<f8", 8), ("Scw", "<f8", 8),
                                  ("mScw", "<f4", 16)])
assert SIM3_OPT_RESULT_DTYPE.itemsize == 232
SIM3_OPT_OK, SIM3_OPT_TOO_FEW = 0, 1
SIM3_OPT_TH2, SIM3_OPT_MIN_INLIERS = 10.0, 20
SIM3_OPT_CORR_BYTES = 104    # scratch per keypoint slot of a pair (plus 16 per pair)

_P = ctypes.c_void_p


class Sim3Map(ctypes.Structure):
    _fields_ = [(name, _P) for name, _ in SIM3_MAP_TABLES]


class Sim3Params(ctypes.Structure):
    _fields_ = [("th", ctypes.c_float), ("pad", ctypes.c_int32)]


class Sim3SolverParams(ctypes.Structure):
    _fields_ = [("min_inliers", ctypes.c_int32), ("max_iterations", ctypes.c_int32), ("rand_max", ctypes.c_int32),
                ("fix_scale", ctypes.c_int32)]


class Sim3OptParams(ctypes.Structure):
    _fields_ = [("th2", ctypes.c_float), ("fix_scale", ctypes.c_int32), ("min_inliers", ctypes.c_int32),
                ("pad", ctypes.c_int32)]


class BowKeyframe(ctypes.Structure):
    """struct spslam_bow_keyframe (host pointers)."""
    _fields_ = [("desc", _P), ("keys_un", _P), ("has_point", _P), ("fv_nodes", _P), ("fv_start", _P),
                ("fv_features", _P), ("n", ctypes.c_int32), ("n_fv", ctypes.c_int32)]


class Sim3Keyframe(ctypes.Structure):
    """struct spslam_sim3_keyframe (host pointers)."""
    _fields_ = [("Tcw", _P), ("keys_un", _P), ("desc", _P), ("grid_off", _P), ("grid_idx", _P), ("match_row", _P),
                ("n", ctypes.c_int32), ("pad", ctypes.c_int32)]


spslam_gpu.EXPORTED += ["spslam_search_by_bow_kf", "spslam_search_by_bow_kf_batch_device", "spslam_search_by_sim3",
                        "spslam_search_by_sim3_batch_device", "spslam_search_by_projection_sim3",
                        "spslam_search_by_projection_sim3_batch_device", "spslam_fuse_sim3_search",
                        "spslam_fuse_sim3_search_batch_device", "spslam_sim3_ransac_table", "spslam_sim3_solver",
                        "spslam_sim3_solver_batch_device", "spslam_debug_fill_loop_scratch", "spslam_sim3_optimize",
                        "spslam_sim3_optimize_batch_device"]


def _bind(lib):
    ci, ip = ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    lib.spslam_search_by_bow_kf_batch_device.argtypes = [_P, ci, _P, ctypes.POINTER(BowSide), ctypes.POINTER(BowSide),
                                                         ctypes.POINTER(BowParams), _P, _P, _P]
    lib.spslam_search_by_bow_kf.argtypes = [_P, ctypes.POINTER(BowKeyframe), ctypes.POINTER(BowKeyframe),
                                            ctypes.POINTER(BowParams), _P, ip]
    lib.spslam_search_by_sim3_batch_device.argtypes = [_P, ci, _P, ctypes.POINTER(Sim3Map), _P, _P, _P, _P, _P, ci, _P,
                                                       ctypes.POINTER(Sim3Params), _P, _P, _P]
    lib.spslam_search_by_sim3.argtypes = [_P, ctypes.POINTER(Sim3Keyframe), ctypes.POINTER(Sim3Keyframe), _P, _P, ci,
                                          _P, _P, ctypes.POINTER(Sim3Params), _P, ip]
    lib.spslam_sim3_ransac_table.argtypes = [ctypes.c_double, ci, ci, ci, _P]
    lib.spslam_sim3_solver_batch_device.argtypes = [_P, ci, _P, ctypes.POINTER(Sim3Map), _P, _P, ci, _P, _P, _P,
                                                    ctypes.POINTER(Sim3SolverParams), _P, _P, _P, _P, _P]
    lib.spslam_sim3_solver.argtypes = [_P, ctypes.POINTER(Sim3Keyframe), ctypes.POINTER(Sim3Keyframe), _P, _P, ci, _P,
                                       _P, ctypes.POINTER(Sim3SolverParams), ctypes.c_double, ci, ip, ip, _P, _P, _P]
    lib.spslam_sim3_optimize_batch_device.argtypes = [_P, ci, _P, ctypes.POINTER(Sim3Map), _P, _P, ci,
                                                      ctypes.POINTER(Sim3OptParams), _P, _P, _P]
    lib.spslam_sim3_optimize.argtypes = [_P, ctypes.POINTER(Sim3Keyframe), ctypes.POINTER(Sim3Keyframe), _P, _P, ci, _P,
                                         ctypes.POINTER(Sim3OptParams), _P, _P]
    lib.spslam_debug_fill_loop_scratch.argtypes = [_P, ci]
    lib.spslam_fuse_sim3_search_batch_device.argtypes = [_P, ci, _P, _P, ci, _P, _P, _P, _P, _P, ci, _P,
                                                         ctypes.POINTER(FuseParams), _P, _P, _P]
    lib.spslam_fuse_sim3_search.argtypes = [_P, _P, _P, ci, _P, _P, ci, _P, _P, _P, ctypes.POINTER(FuseParams), _P, ip]
    lib.spslam_search_by_projection_sim3_batch_device.argtypes = [_P, ci, _P, _P, ci, _P, _P, _P, _P, _P, ci, _P, _P,
                                                                  ctypes.POINTER(FuseParams), _P, _P, _P]
    lib.spslam_search_by_projection_sim3.argtypes = [_P, _P, _P, ci, _P, _P, ci, _P, _P, _P, _P,
                                                     ctypes.POINTER(FuseParams), _P, ip]


def _keyframe(keys_un, desc, grid_off, grid_idx):
    """A keyframe of a projection search's host form as contiguous arrays of the C types."""
    return (np.ascontiguousarray(keys_un, spslam_gpu.KEYPOINT_DTYPE), np.ascontiguousarray(desc, np.uint8).reshape(-1, 32),
            np.ascontiguousarray(grid_off, np.int32), np.ascontiguousarray(grid_idx, np.int32))


class LoopMatcher:
    """GPU loop-closing matchers on a context configured with spslam_frame_configure.  The device forms take device
    pointers as ints; the host forms take one problem on numpy arrays, check every index and return copies."""

    def __init__(self, ex: spslam_gpu.OrbExtractor):
        self.ex = ex
        _bind(ex.lib)

    # ---- SearchByBoW(KeyFrame*, KeyFrame*)
    def search_by_bow_kf_batch_device(self, n_pairs, d_pairs, kf1: BowSide, kf2: BowSide, d_match12, d_nmatches,
                                      nn_ratio=0.75, check_orientation=True, stream=0):
        p = BowParams(nn_ratio, int(check_orientation))
        self.ex._check(self.ex.lib.spslam_search_by_bow_kf_batch_device(
            self.ex.ctx, n_pairs, d_pairs, ctypes.byref(kf1), ctypes.byref(kf2), ctypes.byref(p), d_match12,
            d_nmatches, stream or None))

    def search_by_bow_kf(self, kf1, kf2, nn_ratio=0.75, check_orientation=True):
        """kf: dict(desc, keys_un, has_point, fv=dict(nodes, start, features) as Vocabulary.transform returns it).
        Returns (match12 per KF1 keypoint: KF2 keypoint or -1, nmatches)."""
        keep, rec = [], []
        for k in (kf1, kf2):
            a = [np.ascontiguousarray(k["desc"], np.uint8).reshape(-1, 32),
                 np.ascontiguousarray(k["keys_un"], spslam_gpu.KEYPOINT_DTYPE),
                 np.ascontiguousarray(k["has_point"], np.uint8),
                 np.ascontiguousarray(k["fv"]["nodes"], np.uint32), np.ascontiguousarray(k["fv"]["start"], np.int32),
                 np.ascontiguousarray(k["fv"]["features"], np.int32)]
            keep.append(a)
            rec.append(BowKeyframe(_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), a[4].ctypes.data, _ptr(a[5]),
                                   len(a[0]), len(a[3])))
        n1 = len(keep[0][0])
        match = np.zeros(max(n1, 1), np.int32)
        nm = ctypes.c_int()
        p = BowParams(nn_ratio, int(check_orientation))
        self.ex._check(self.ex.lib.spslam_search_by_bow_kf(self.ex.ctx, ctypes.byref(rec[0]), ctypes.byref(rec[1]),
                                                           ctypes.byref(p), match.ctypes.data, ctypes.byref(nm)))
        return match[:n1], nm.value

    # ---- SearchBySim3
    def search_by_sim3_batch_device(self, n_pairs, d_pairs, smap: Sim3Map, d_keys_un, d_desc, d_grid_off, d_grid_idx,
                                    d_counts, cap, d_already2, d_match12, d_n_found, th=TH_SIM3, stream=0):
        p = Sim3Params(th, 0)
        self.ex._check(self.ex.lib.spslam_search_by_sim3_batch_device(
            self.ex.ctx, n_pairs, d_pairs, ctypes.byref(smap), d_keys_un, d_desc, d_grid_off, d_grid_idx, d_counts,
            cap, d_already2 or None, ctypes.byref(p), d_match12, d_n_found, stream or None))

    def search_by_sim3(self, kf1, kf2, points, point_bad, s12, R12, t12, match12, already2=None, th=TH_SIM3):
        """kf: dict(Tcw, kun, desc, go, gi, match_row).  Returns (match12 after, n_found)."""
        keep, rec = [], []
        for k in (kf1, kf2):
            kun, d, go, gi = _keyframe(k["kun"], k["desc"], k["go"], k["gi"])
            T = np.ascontiguousarray(k["Tcw"], np.float32).reshape(16)
            rows = np.ascontiguousarray(k["match_row"], np.int32)
            keep.append((kun, d, go, gi, T, rows))
            rec.append(Sim3Keyframe(T.ctypes.data, _ptr(kun), _ptr(d), go.ctypes.data, _ptr(gi), _ptr(rows), len(kun), 0))
        pts = np.ascontiguousarray(points, LOCAL_POINT_DTYPE)
        bad = None if point_bad is None else np.ascontiguousarray(point_bad, np.uint8)
        pair = np.zeros((), SIM3_PAIR_DTYPE)
        pair["s12"], pair["R12"], pair["t12"] = s12, np.asarray(R12, np.float32).reshape(9), t12
        m = np.array(match12, np.int32).reshape(-1)
        m = m if len(m) else np.zeros(1, np.int32)
        a2 = None if already2 is None else np.ascontiguousarray(already2, np.uint8)
        nf = ctypes.c_int()
        p = Sim3Params(th, 0)
        self.ex._check(self.ex.lib.spslam_search_by_sim3(
            self.ex.ctx, ctypes.byref(rec[0]), ctypes.byref(rec[1]), _ptr(pts), _ptr(bad), len(pts), pair.ctypes.data,
            _ptr(a2), ctypes.byref(p), m.ctypes.data, ctypes.byref(nf)))
        return m[:len(keep[0][0])], nf.value

    # ---- Sim3Solver
    def sim3_ransac_table(self, cap, probability=0.99, min_inliers=20, max_iterations=300):
        """mRansacMaxIts for N = 0 .. cap (SetRansacParameters): the table the device form looks N up in."""
        table = np.zeros(cap + 1, np.int32)
        self.ex._check(self.ex.lib.spslam_sim3_ransac_table(probability, min_inliers, max_iterations, cap,
                                                            table.ctypes.data))
        return table

    def sim3_solver_batch_device(self, n_problems, d_problems, smap: Sim3Map, d_keys_un, d_counts, cap, d_match12,
                                 d_rand, d_max_its_table, d_results, d_inliers, d_pairs_out=0, d_match12_out=0,
                                 min_inliers=20, max_iterations=300, fix_scale=True, rand_max=RAND_MAX, stream=0):
        p = Sim3SolverParams(min_inliers, max_iterations, rand_max, int(fix_scale))
        self.ex._check(self.ex.lib.spslam_sim3_solver_batch_device(
            self.ex.ctx, n_problems, d_problems, ctypes.byref(smap), d_keys_un, d_counts, cap, d_match12, d_rand,
            d_max_its_table, ctypes.byref(p), d_results, d_inliers, d_pairs_out or None, d_match12_out or None,
            stream or None))

    def sim3_solver(self, kf1, kf2, points, point_bad, match12, rand, n_iterations, state=(0, 0), probability=0.99,
                    min_inliers=20, max_iterations=300, fix_scale=True, rand_max=RAND_MAX):
        """One iterate(n_iterations) of a solver whose state (iterations_done, best_inliers) the caller carries.
        kf: dict(Tcw, kun, match_row).  Returns (result record, inlier bytes, match12 filtered to the inliers or
        None unless FOUND, the state after)."""
        keep, rec = [], []
        for k in (kf1, kf2):
            kun = np.ascontiguousarray(k["kun"], spslam_gpu.KEYPOINT_DTYPE)
            T = np.ascontiguousarray(k["Tcw"], np.float32).reshape(16)
            rows = np.ascontiguousarray(k["match_row"], np.int32)
            keep.append((kun, T, rows))
            rec.append(Sim3Keyframe(T.ctypes.data, _ptr(kun), None, None, None, _ptr(rows), len(kun), 0))
        pts = np.ascontiguousarray(points, LOCAL_POINT_DTYPE)
        bad = None if point_bad is None else np.ascontiguousarray(point_bad, np.uint8)
        n1 = len(keep[0][0])
        m = np.ascontiguousarray(match12, np.int32).reshape(-1)
        r = np.ascontiguousarray(rand, np.int32).reshape(-1)
        if len(r) < 3 * max_iterations:
            raise ValueError("rand holds fewer than 3 * max_iterations values")
        p = Sim3SolverParams(min_inliers, max_iterations, rand_max, int(fix_scale))
        done, best = ctypes.c_int(state[0]), ctypes.c_int(state[1])
        result = np.zeros((), SIM3_RESULT_DTYPE)
        inliers, out = np.zeros(max(n1, 1), np.uint8), np.zeros(max(n1, 1), np.int32)
        self.ex._check(self.ex.lib.spslam_sim3_solver(
            self.ex.ctx, ctypes.byref(rec[0]), ctypes.byref(rec[1]), _ptr(pts), _ptr(bad), len(pts), _ptr(m),
            r.ctypes.data, ctypes.byref(p), probability, n_iterations, ctypes.byref(done), ctypes.byref(best),
            result.ctypes.data, inliers.ctypes.data, out.ctypes.data))
        found = int(result["status"]) == SIM3_FOUND
        return result, inliers[:n1], out[:n1] if found else None, (done.value, best.value)

    # ---- Optimizer::OptimizeSim3 and Scw
    def sim3_optimize_batch_device(self, n_pairs, d_pairs, smap: Sim3Map, d_keys_un, d_counts, cap, d_match12, d_results,
                                   th2=SIM3_OPT_TH2, fix_scale=True, min_inliers=SIM3_OPT_MIN_INLIERS, stream=0):
        """d_pairs: the records the solver leaves and SearchBySim3 reads; d_match12 is rewritten in place;
        d_results: n_pairs records of SIM3_OPT_RESULT_DTYPE."""
        p = Sim3OptParams(th2, int(fix_scale), min_inliers, 0)
        self.ex._check(self.ex.lib.spslam_sim3_optimize_batch_device(
            self.ex.ctx, n_pairs, d_pairs, ctypes.byref(smap), d_keys_un, d_counts, cap, ctypes.byref(p), d_match12,
            d_results, stream or None))

    def sim3_optimize(self, kf1, kf2, points, point_bad, s12, R12, t12, match12, th2=SIM3_OPT_TH2, fix_scale=True,
                      min_inliers=SIM3_OPT_MIN_INLIERS):
        """kf: dict(Tcw, kun, match_row).  Returns (result record, match12 after)."""
        keep, rec = [], []
        for k in (kf1, kf2):
            kun = np.ascontiguousarray(k["kun"], spslam_gpu.KEYPOINT_DTYPE)
            T = np.ascontiguousarray(k["Tcw"], np.float32).reshape(16)
            rows = np.ascontiguousarray(k["match_row"], np.int32)
            keep.append((kun, T, rows))
            rec.append(Sim3Keyframe(T.ctypes.data, _ptr(kun), None, None, None, _ptr(rows), len(kun), 0))
        pts = np.ascontiguousarray(points, LOCAL_POINT_DTYPE)
        bad = None if point_bad is None else np.ascontiguousarray(point_bad, np.uint8)
        pair = np.zeros((), SIM3_PAIR_DTYPE)
        pair["s12"], pair["R12"], pair["t12"] = s12, np.asarray(R12, np.float32).reshape(9), t12
        n1 = len(keep[0][0])
        m = np.array(match12, np.int32).reshape(-1)
        m = m if len(m) else np.zeros(1, np.int32)
        p = Sim3OptParams(th2, int(fix_scale), min_inliers, 0)
        result = np.zeros((), SIM3_OPT_RESULT_DTYPE)
        self.ex._check(self.ex.lib.spslam_sim3_optimize(
            self.ex.ctx, ctypes.byref(rec[0]), ctypes.byref(rec[1]), _ptr(pts), _ptr(bad), len(pts), pair.ctypes.data,
            ctypes.byref(p), m.ctypes.data if n1 else None, result.ctypes.data))
        return result, m[:n1]

    def debug_fill_loop_scratch(self, value):
        self.ex._check(self.ex.lib.spslam_debug_fill_loop_scratch(self.ex.ctx, value))

    # ---- Fuse(pKF, Scw, ...), the search
    def fuse_sim3_search_batch_device(self, n_problems, d_problems, d_points, max_points, d_keys_un, d_desc,
                                      d_grid_off, d_grid_idx, d_counts, cap, d_skip, d_results, d_nfused, th=TH_FUSE,
                                      stream=0):
        p = FuseParams(th, 0)
        self.ex._check(self.ex.lib.spslam_fuse_sim3_search_batch_device(
            self.ex.ctx, n_problems, d_problems, d_points, max_points, d_keys_un, d_desc, d_grid_off, d_grid_idx,
            d_counts, cap, d_skip or None, ctypes.byref(p), d_results, d_nfused, stream or None))

    def fuse_sim3_search(self, Scw, points, keys_un, desc, grid_off, grid_idx, skip=None, th=TH_FUSE):
        S = np.ascontiguousarray(Scw, np.float32).reshape(16)
        pts = np.ascontiguousarray(points, LOCAL_POINT_DTYPE)
        k, d, go, gi = _keyframe(keys_un, desc, grid_off, grid_idx)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        res = np.zeros(max(len(pts), 1), FUSE_RESULT_DTYPE)
        nf = ctypes.c_int(0)
        p = FuseParams(th, 0)
        self.ex._check(self.ex.lib.spslam_fuse_sim3_search(
            self.ex.ctx, S.ctypes.data, _ptr(pts), len(pts), _ptr(k), _ptr(d), len(k), go.ctypes.data, _ptr(gi),
            _ptr(sk), ctypes.byref(p), res.ctypes.data, ctypes.byref(nf)))
        return res[:len(pts)], nf.value

    # ---- SearchByProjection(pKF, Scw, ...)
    def search_by_projection_sim3_batch_device(self, n_problems, d_problems, d_points, max_points, d_keys_un, d_desc,
                                               d_grid_off, d_grid_idx, d_counts, cap, d_skip, d_taken, d_match,
                                               d_nmatches, th=TH_PROJECTION, stream=0):
        p = FuseParams(th, 0)
        self.ex._check(self.ex.lib.spslam_search_by_projection_sim3_batch_device(
            self.ex.ctx, n_problems, d_problems, d_points, max_points, d_keys_un, d_desc, d_grid_off, d_grid_idx,
            d_counts, cap, d_skip or None, d_taken or None, ctypes.byref(p), d_match, d_nmatches, stream or None))

    def search_by_projection_sim3(self, Scw, points, keys_un, desc, grid_off, grid_idx, skip=None, taken=None,
                                  th=TH_PROJECTION):
        """Returns (match per keyframe keypoint: index of the point newly assigned to it or -1, nmatches)."""
        S = np.ascontiguousarray(Scw, np.float32).reshape(16)
        pts = np.ascontiguousarray(points, LOCAL_POINT_DTYPE)
        k, d, go, gi = _keyframe(keys_un, desc, grid_off, grid_idx)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
        match = np.zeros(max(len(k), 1), np.int32)
        nm = ctypes.c_int(0)
        p = FuseParams(th, 0)
        self.ex._check(self.ex.lib.spslam_search_by_projection_sim3(
            self.ex.ctx, S.ctypes.data, _ptr(pts), len(pts), _ptr(k), _ptr(d), len(k), go.ctypes.data, _ptr(gi),
            _ptr(sk), _ptr(tk), ctypes.byref(p), match.ctypes.data, ctypes.byref(nm)))
        return match[:len(k)], nm.value


def compute_sim3_round_robin(first_success, per_turn=5):
    """Which candidate LoopClosing::ComputeSim3's loop (:288-344) reaches first: the candidates take turns of
    per_turn RANSAC iterations in index order, so a candidate whose solver first succeeds at iteration k (counted
    from 0; None: never, or discarded) returns its transformation in round k // per_turn.  first_success is, per
    candidate, result["iterations_done"] - 1 of one device call with n_iterations = max_iterations when its status
    is SIM3_FOUND, else None.  Returns (candidate, round), or (None, None) when every candidate fails."""
    turns = [(k // per_turn, i) for i, k in enumerate(first_success) if k is not None]
    if not turns:
        return None, None
    rnd, i = min(turns)
    return i, rnd


__all__ = ["LoopMatcher", "Sim3SolverParams", "Sim3OptParams", "SIM3_OPT_RESULT_DTYPE", "SIM3_OPT_OK", "SIM3_OPT_TOO_FEW",
           "SIM3_OPT_TH2", "SIM3_OPT_MIN_INLIERS", "SIM3_OPT_CORR_BYTES", "SIM3_PROBLEM_DTYPE", "SIM3_RESULT_DTYPE", "SIM3_FOUND", "SIM3_NOT_YET",
           "SIM3_NO_MORE", "SIM3_MAX_ITERATIONS", "RAND_MAX", "compute_sim3_round_robin", "Sim3Map", "Sim3Params", "BowKeyframe", "Sim3Keyframe", "BowSide", "SIM3_PAIR_DTYPE",
           "SIM3_MAP_TABLES", "FUSE_PROBLEM_DTYPE", "FUSE_RESULT_DTYPE", "LOCAL_POINT_DTYPE", "PROJ_SIM3_KEYS",
           "POINTS_PER_GROUP", "BOW_WAVES", "TH_SIM3", "TH_PROJECTION", "TH_FUSE"]
