"""ctypes binding of the place-recognition entries of include/spslam_gpu.h: KeyFrameDatabase's
DetectRelocalizationCandidates and DetectLoopCandidates and LoopClosing::DetectLoop's reference score, on BowVectors
and a covisibility graph that stay on the device.  add() / erase() are the caller's: they flip in_db."""
from __future__ import annotations

import ctypes

import numpy as np

import spslam_gpu
from spslam_match import COVIS_BEST, COVIS_MAX_KF, CovisGraph

PLACE_MAX_WORDS = 8192
PLACE_OK, PLACE_EMPTY, PLACE_NONE_KEPT = 0, 1, 2
PLACE_PROBLEM_DTYPE = np.dtype([("kf_base", "<i4"), ("n_kf", "<i4"), ("query", "<i4"), ("out_offset", "<i4")])
PLACE_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_sharing", "<i4"), ("max_common_words", "<i4"),
                               ("min_common_words", "<i4"), ("n_scored", "<i4"), ("n_kept", "<i4"),
                               ("n_candidates", "<i4"), ("best_acc_score", "<f4")])
assert PLACE_PROBLEM_DTYPE.itemsize == 16 and PLACE_RESULT_DTYPE.itemsize == 32
# the tables of spslam_place_db and spslam_place_frames (before `cap`), in their order
PLACE_DB_TABLES = (("bow_words", np.uint32), ("bow_values", np.float64), ("n_bow", np.int32), ("in_db", np.uint8),
                   ("reloc_score", np.float32), ("loop_score", np.float32))
PLACE_FRAME_TABLES = PLACE_DB_TABLES[:3]


class PlaceDb(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _ in PLACE_DB_TABLES] + [("cap", ctypes.c_int32),
                                                                          ("pad", ctypes.c_int32)]


class PlaceFrames(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _ in PLACE_FRAME_TABLES] + [("cap", ctypes.c_int32),
                                                                             ("pad", ctypes.c_int32)]


spslam_gpu.EXPORTED += ["spslam_place_reloc_candidates", "spslam_place_reloc_candidates_batch_device",
                        "spslam_place_loop_candidates", "spslam_place_loop_candidates_batch_device",
                        "spslam_place_min_score", "spslam_place_min_score_batch_device"]


def _bind(lib):
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.spslam_place_reloc_candidates_batch_device.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.spslam_place_loop_candidates_batch_device.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
    lib.spslam_place_min_score_batch_device.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
    lib.spslam_place_reloc_candidates.argtypes = [vp, vp, ci, vp, vp, ci, vp, vp, vp]
    lib.spslam_place_loop_candidates.argtypes = [vp, vp, ci, ci, vp, ctypes.c_float, vp, vp]
    lib.spslam_place_min_score.argtypes = [vp, vp, ci, ci, vp, vp, vp]


def _host_db(db, cap):
    """The database tables of one sequence as contiguous arrays of the C types (copies: the scores are rewritten)."""
    a = {name: np.array(db[name], dt).reshape(-1) for name, dt in PLACE_DB_TABLES}
    return a, PlaceDb(cap=cap, **{name: a[name].ctypes.data for name in a})


def _host_graph(graph, stride):
    g = {name: np.ascontiguousarray(graph[name], np.int32).reshape(-1)
         for name in ("covis", "weights", "ordered", "n_ordered") if graph.get(name) is not None}
    return g, CovisGraph(stride=stride, **{name: g[name].ctypes.data for name in g})


class PlaceRecognition:
    """GPU KeyFrameDatabase queries.  The device forms take a PlaceDb, a PlaceFrames and the CovisGraph of
    spslam_match; a call holds at most one problem per sequence.  The host forms take one sequence's tables by
    PLACE_DB_TABLES name (n_kf rows of cap words) and the graph arrays by name, check every index and return
    copies."""

    def __init__(self, ex: spslam_gpu.OrbExtractor):
        self.ex = ex
        _bind(ex.lib)

    # ---- device resident
    def reloc_candidates_batch_device(self, n_problems, d_problems, db: PlaceDb, frames: PlaceFrames,
                                      graph: CovisGraph, d_results, d_candidates, stream=0):
        self.ex._check(self.ex.lib.spslam_place_reloc_candidates_batch_device(
            self.ex.ctx, n_problems, d_problems, ctypes.byref(db), ctypes.byref(frames), ctypes.byref(graph),
            d_results, d_candidates, stream or None))

    def loop_candidates_batch_device(self, n_problems, d_problems, db: PlaceDb, graph: CovisGraph, d_min_score,
                                     d_results, d_candidates, stream=0):
        self.ex._check(self.ex.lib.spslam_place_loop_candidates_batch_device(
            self.ex.ctx, n_problems, d_problems, ctypes.byref(db), ctypes.byref(graph), d_min_score, d_results,
            d_candidates, stream or None))

    def min_score_batch_device(self, n_problems, d_problems, db: PlaceDb, graph: CovisGraph, d_kf_bad, d_min_score,
                               stream=0):
        self.ex._check(self.ex.lib.spslam_place_min_score_batch_device(
            self.ex.ctx, n_problems, d_problems, ctypes.byref(db), ctypes.byref(graph), d_kf_bad or None,
            d_min_score, stream or None))

    # ---- one problem on host arrays
    def reloc_candidates(self, db, cap, n_kf, q_words, q_values, covis):
        """Returns (result record, candidates, reloc_score after)."""
        a, D = _host_db(db, cap)
        qw, qv = np.ascontiguousarray(q_words, np.uint32), np.ascontiguousarray(q_values, np.float64)
        g, G = _host_graph({"covis": covis}, n_kf)
        res, cand = np.zeros((), PLACE_RESULT_DTYPE), np.zeros(max(n_kf, 1), np.int32)
        self.ex._check(self.ex.lib.spslam_place_reloc_candidates(
            self.ex.ctx, ctypes.byref(D), n_kf, qw.ctypes.data if len(qw) else None,
            qv.ctypes.data if len(qv) else None, len(qw), ctypes.byref(G), res.ctypes.data, cand.ctypes.data))
        return res, cand[:int(res["n_candidates"])].copy(), a["reloc_score"]

    def loop_candidates(self, db, cap, n_kf, query, covis, weights, stride, min_score):
        """Returns (result record, candidates, loop_score after)."""
        a, D = _host_db(db, cap)
        g, G = _host_graph({"covis": covis, "weights": weights}, stride)
        res, cand = np.zeros((), PLACE_RESULT_DTYPE), np.zeros(max(n_kf, 1), np.int32)
        self.ex._check(self.ex.lib.spslam_place_loop_candidates(
            self.ex.ctx, ctypes.byref(D), n_kf, query, ctypes.byref(G), float(min_score), res.ctypes.data,
            cand.ctypes.data))
        return res, cand[:int(res["n_candidates"])].copy(), a["loop_score"]

    def min_score(self, db, cap, n_kf, query, ordered, n_ordered, stride, kf_bad=None):
        a, D = _host_db(db, cap)
        g, G = _host_graph({"ordered": ordered, "n_ordered": n_ordered}, stride)
        bad = None if kf_bad is None else np.ascontiguousarray(kf_bad, np.uint8)
        out = np.zeros((), np.float32)
        self.ex._check(self.ex.lib.spslam_place_min_score(
            self.ex.ctx, ctypes.byref(D), n_kf, query, ctypes.byref(G), None if bad is None else bad.ctypes.data,
            out.ctypes.data))
        return np.float32(out)


__all__ = ["PlaceRecognition", "PlaceDb", "PlaceFrames", "PLACE_PROBLEM_DTYPE", "PLACE_RESULT_DTYPE",
           "PLACE_DB_TABLES", "PLACE_FRAME_TABLES", "PLACE_MAX_WORDS", "PLACE_OK", "PLACE_EMPTY", "PLACE_NONE_KEPT",
           "COVIS_BEST", "COVIS_MAX_KF"]
