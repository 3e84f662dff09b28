"""ctypes binding of the relocalization entries of include/spslam_gpu.h: PnPsolver, the third call of
Tracking::Relocalization, between SearchByBoW(KeyFrame, Frame) (spslam_bow) and PoseOptimization: EPnP RANSAC with
the draws an input.  The candidate loop, SearchByProjection(Frame, KeyFrame, ...) and the map are the caller's."""
from __future__ import annotations

import ctypes

import numpy as np

import spslam_gpu
from spslam_loop import RAND_MAX, Sim3Map
from spslam_match import LOCAL_POINT_DTYPE, _ptr

# struct spslam_pnp_problem / spslam_pnp_result and the statuses
PNP_PROBLEM_DTYPE = np.dtype([("kf", "<i4"), ("frame_slot", "<i4"), ("match_offset", "<i4"), ("rand_offset", "<i4"),
                              ("inlier_offset", "<i4"), ("best_mask_offset", "<i4"), ("iterations_done", "<i4"),
                              ("best_inliers", "<i4"), ("n_iterations", "<i4"), ("rand_iterations", "<i4"),
                              ("pad", "<i4", 2), ("best_Tcw", "<f4", 16)])
PNP_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("iterations_done", "<i4"), ("best_inliers", "<i4"),
                             ("n_inliers", "<i4"), ("iteration", "<i4"), ("min_inliers", "<i4"), ("max_its", "<i4"),
                             ("best_Tcw", "<f4", 16), ("Tcw", "<f4", 16)])
assert PNP_PROBLEM_DTYPE.itemsize == 112 and PNP_RESULT_DTYPE.itemsize == 160
PNP_REFINED, PNP_BEST_NO_MORE, PNP_NO_MORE, PNP_OUT_OF_DRAWS = 0, 1, 2, 3
PNP_MAX_ITERATIONS = 4096
PNP_CORR_BYTES, PNP_HYP_BYTES = 32, 104   # scratch per keypoint slot and per iteration of a problem (plus 16)
# Tracking.cc:1628: SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
PNP_PROBABILITY, PNP_MIN_INLIERS, PNP_MAX_ITS, PNP_MIN_SET, PNP_EPSILON, PNP_TH2 = 0.99, 10, 300, 4, 0.5, 5.991

_P = ctypes.c_void_p


class PnPParams(ctypes.Structure):
    _fields_ = [("min_inliers", ctypes.c_int32), ("max_iterations", ctypes.c_int32), ("min_set", ctypes.c_int32),
                ("rand_max", ctypes.c_int32), ("epsilon", ctypes.c_float), ("th2", ctypes.c_float)]


spslam_gpu.EXPORTED += ["spslam_pnp_ransac_table", "spslam_pnp_solver", "spslam_pnp_solver_batch_device"]


def _bind(lib):
    ci = ctypes.c_int
    lib.spslam_pnp_ransac_table.argtypes = [ctypes.c_double, ci, ci, ci, ctypes.c_float, ci, _P, _P]
    lib.spslam_pnp_solver_batch_device.argtypes = [_P, ci, _P, ctypes.POINTER(Sim3Map), _P, _P, ci, _P, _P, _P, _P,
                                                   ctypes.POINTER(PnPParams), _P, _P, _P, _P, _P]
    lib.spslam_pnp_solver.argtypes = [_P, _P, ci, _P, _P, ci, _P, _P, ci, _P, ctypes.POINTER(PnPParams),
                                      ctypes.c_double, _P, _P, _P, _P, _P]


class PnPSolver:
    """PnPsolver on a context configured with spslam_frame_configure.  batch_device takes device pointers as ints.
    solve takes torch tensors (or numpy arrays) for one problem and keeps the solver's state -- mnIterations,
    mnBestInliers, mBestTcw and the best mask -- between calls, as a PnPsolver object does between iterate calls;
    reset() is a new solver."""

    def __init__(self, ex: spslam_gpu.OrbExtractor, probability=PNP_PROBABILITY, min_inliers=PNP_MIN_INLIERS,
                 max_iterations=PNP_MAX_ITS, min_set=PNP_MIN_SET, epsilon=PNP_EPSILON, th2=PNP_TH2, rand_max=RAND_MAX):
        self.ex = ex
        _bind(ex.lib)
        self.probability = probability
        self.params = PnPParams(min_inliers, max_iterations, min_set, rand_max, epsilon, th2)
        self.reset()

    def reset(self):
        self.state = np.zeros((), PNP_PROBLEM_DTYPE)
        self.best_mask = None

    def ransac_table(self, cap):
        """(mRansacMaxIts, mRansacMinInliers) for N = 0 .. cap: the tables the device form looks N up in."""
        max_its, min_n = np.zeros(cap + 1, np.int32), np.zeros(cap + 1, np.int32)
        p = self.params
        self.ex._check(self.ex.lib.spslam_pnp_ransac_table(self.probability, p.min_inliers, p.max_iterations, p.min_set,
                                                           p.epsilon, cap, max_its.ctypes.data, min_n.ctypes.data))
        return max_its, min_n

    def batch_device(self, n_problems, d_problems, smap: Sim3Map, d_frame_keys_un, d_frame_counts, cap, d_match, d_rand,
                     d_max_its_table, d_min_inliers_table, d_results, d_inliers, d_best_mask, d_frame_points=0,
                     stream=0):
        self.ex._check(self.ex.lib.spslam_pnp_solver_batch_device(
            self.ex.ctx, n_problems, d_problems, ctypes.byref(smap), d_frame_keys_un, d_frame_counts, cap, d_match,
            d_rand, d_max_its_table, d_min_inliers_table, ctypes.byref(self.params), d_results, d_inliers, d_best_mask,
            d_frame_points or None, stream or None))

    def solve(self, keys_un, match, kf_match_row, points, point_bad, rand, n_iterations):
        """One iterate(n_iterations) of this solver.  keys_un: the frame's keypoints; match: per frame keypoint a
        keyframe keypoint or -1; kf_match_row: the keyframe's map points as rows of points; rand: 4 raw rand() values
        per iteration of the solver's life, as far as recorded.  Returns (result record, inlier bytes, the frame's
        map points -- a row or -1 per keypoint -- or None when no pose is returned), tensors where tensors came in."""
        as_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)  # noqa: E731
        tensors = hasattr(match, "detach")
        kun = np.ascontiguousarray(as_np(keys_un)).view(spslam_gpu.KEYPOINT_DTYPE).reshape(-1)
        m = np.ascontiguousarray(as_np(match), np.int32).reshape(-1)
        rows = np.ascontiguousarray(as_np(kf_match_row), np.int32).reshape(-1)
        pts = np.ascontiguousarray(as_np(points)).view(LOCAL_POINT_DTYPE).reshape(-1)
        bad = None if point_bad is None else np.ascontiguousarray(as_np(point_bad), np.uint8)
        r = np.ascontiguousarray(as_np(rand), np.int32).reshape(-1)
        if len(m) != len(kun):
            raise ValueError("match has one entry per frame keypoint")
        n = len(kun)
        q = self.state.copy()
        q["n_iterations"], q["rand_iterations"] = n_iterations, len(r) // 4
        mask = np.zeros(max(n, 1), np.uint8)
        if self.best_mask is not None:
            mask[:n] = self.best_mask[:n]
        result = np.zeros((), PNP_RESULT_DTYPE)
        inliers, fp = np.zeros(max(n, 1), np.uint8), np.full(max(n, 1), -1, np.int32)
        self.ex._check(self.ex.lib.spslam_pnp_solver(
            self.ex.ctx, _ptr(kun), n, _ptr(m), _ptr(rows), len(rows), _ptr(pts), _ptr(bad), len(pts), _ptr(r),
            ctypes.byref(self.params), self.probability, q.ctypes.data, result.ctypes.data, inliers.ctypes.data,
            mask.ctypes.data, fp.ctypes.data))
        self.state["iterations_done"], self.state["best_inliers"] = result["iterations_done"], result["best_inliers"]
        self.state["best_Tcw"] = result["best_Tcw"]
        self.best_mask = mask[:n].copy()
        pose = int(result["status"]) in (PNP_REFINED, PNP_BEST_NO_MORE)
        out = (inliers[:n], fp[:n] if pose else None)
        if tensors:
            import torch
            out = tuple(None if a is None else torch.from_numpy(a.copy()) for a in out)
        return (result,) + out


__all__ = ["PnPSolver", "PnPParams", "PNP_PROBLEM_DTYPE", "PNP_RESULT_DTYPE", "PNP_REFINED", "PNP_BEST_NO_MORE",
           "PNP_NO_MORE", "PNP_OUT_OF_DRAWS", "PNP_MAX_ITERATIONS", "PNP_CORR_BYTES", "PNP_HYP_BYTES", "PNP_PROBABILITY",
           "PNP_MIN_INLIERS", "PNP_MAX_ITS", "PNP_MIN_SET", "PNP_EPSILON", "PNP_TH2"]
