"""ctypes binding of the tracking-graph part of include/spslam_gpu.h
(spslam_track_graph_batch_device: TrackWithMotionModel / TrackLocalMap's
bookkeeping between matching and Optimizer::PoseOptimization,
src/Tracking.cc:951-1000, 1055-1068; src/Optimizer.cc:561-640, 681-860;
spslam_track_refkf_batch_device + spslam_masked_frame_copy_device: the
motion model's failure test and the TrackReferenceKeyFrame switch,
src/Tracking.cc:318-324, 791-882; spslam_track_refkf_vote_batch_device: the
reference keyframe, UpdateLocalKeyFrames' pKFmax, :1459-1570;
spslam_track_update_local_map_batch_device / spslam_track_update_local_map:
Tracking::UpdateLocalMap, :1427-1571)."""
from __future__ import annotations

import ctypes

import numpy as np

import spslam_gpu

MOTION_MODEL, DISCARD, LOCAL_MAP, MOTION_PRIOR, LAST_FRAME = 0, 1, 2, 3, 4
REFKF_PREPARE, REFKF_SELECT = 0, 1

spslam_gpu.EXPORTED += ["spslam_track_graph_batch_device", "spslam_track_refkf_batch_device",
                        "spslam_track_refkf_vote_batch_device", "spslam_masked_frame_copy_device",
                        "spslam_track_update_local_map_batch_device", "spslam_track_update_local_map"]

_P = ctypes.c_void_p


class TrackBatch(ctypes.Structure):
    """struct spslam_track_batch (device pointers as ints)."""
    _fields_ = [("keys_un", _P), ("uright", _P), ("kp_counts", _P), ("cap", ctypes.c_int32),
                ("proj_frames", _P), ("proj_points", _P), ("proj_match", _P),
                ("local_frames", _P), ("local_points", _P), ("local_match", _P), ("taken", _P),
                ("planes_a", _P), ("planes_b", _P), ("count_a", _P), ("count_b", _P),
                ("stride_a", ctypes.c_int32), ("stride_b", ctypes.c_int32), ("cap_a", ctypes.c_int32),
                ("cap_b", ctypes.c_int32),
                ("map", _P), ("assoc_match", _P), ("assoc_parallel", _P), ("assoc_vertical", _P),
                ("assoc_frames_next", _P), ("plane_outlier", _P), ("next_match", _P), ("next_parallel", _P),
                ("next_vertical", _P), ("assoc_frames_first", _P), ("seen", _P), ("next_frames", _P),
                ("next_points", _P), ("velocity", _P), ("point_outlier_local", _P),
                ("problems", _P), ("points", _P), ("planes", _P), ("edge_of_kp", _P), ("results", _P),
                ("point_outlier", _P),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("bf", ctypes.c_float), ("pad", ctypes.c_int32)]


class RefkfBatch(ctypes.Structure):
    """struct spslam_refkf_batch (device pointers as ints)."""
    _fields_ = [("nmatches", _P), ("fallback", _P), ("refkf_counts", _P), ("bow_nmatches", _P), ("bow_match", _P),
                ("refkf_rows", _P), ("refkf_index", _P), ("rows_stride", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("refkf_sets", _P), ("assoc_frames", _P), ("apply", _P), ("state", _P), ("refkf_match", _P),
                ("refkf_frames", _P), ("refkf_assoc", _P)]


class RefkfVote(ctypes.Structure):
    """struct spslam_refkf_vote (device pointers as ints)."""
    _fields_ = [("kf_base", _P), ("kf_sets", _P), ("ids_per_kf", ctypes.c_int32), ("n_kf", ctypes.c_int32),
                ("new_kf", ctypes.c_int32), ("pad", ctypes.c_int32), ("state", _P), ("refkf_index", _P),
                ("refkf_sets", _P), ("refkf_pairs", _P)]


class FrameRegion(ctypes.Structure):
    """struct spslam_frame_region."""
    _fields_ = [("dst", _P), ("src", _P), ("frame_bytes", ctypes.c_int64), ("dst_stride", ctypes.c_int64),
                ("src_stride", ctypes.c_int64)]


class LocalMap(ctypes.Structure):
    """struct spslam_local_map (device pointers as ints; host pointers in the single-frame form)."""
    _fields_ = [("frame_rows", _P), ("kp_counts", _P), ("id_to_row", _P), ("id_base", _P), ("kf_base", _P),
                ("row_base", _P), ("cap", ctypes.c_int32), ("n_kf", ctypes.c_int32),
                ("obs_off", _P), ("obs_kf", _P), ("point_bad", _P), ("points", _P),
                ("kf_bad", _P), ("covis", _P), ("child_off", _P), ("child", _P), ("parent", _P),
                ("match_off", _P), ("match_row", _P)]


class LocalMapOut(ctypes.Structure):
    """struct spslam_local_map_out."""
    _fields_ = [("state", _P), ("local_kfs", _P), ("n_local_kfs", _P), ("kf_max", _P), ("local_rows", _P),
                ("n_local", _P), ("status", _P), ("scratch", _P), ("kf_cap", ctypes.c_int32),
                ("capacity", ctypes.c_int32), ("scratch_stride", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("records", _P), ("local_frames", _P)]


# the per-sequence tables of struct spslam_local_map (local_mapping.SeqMap.local_map_tables)
LOCAL_MAP_TABLES = (("obs_off", np.int32), ("obs_kf", np.int32), ("point_bad", np.uint8), ("kf_bad", np.uint8),
                    ("covis", np.int32), ("child_off", np.int32), ("child", np.int32), ("parent", np.int32),
                    ("match_off", np.int32), ("match_row", np.int32))


def _bind(lib):
    lib.spslam_track_update_local_map_batch_device.argtypes = [_P, ctypes.c_int, _P, _P, _P, _P]
    lib.spslam_track_update_local_map.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, _P]
    lib.spslam_track_graph_batch_device.argtypes = [_P, ctypes.c_int, ctypes.c_int, _P, _P]
    lib.spslam_track_refkf_batch_device.argtypes = [_P, ctypes.c_int, ctypes.c_int, _P, _P, _P]
    lib.spslam_masked_frame_copy_device.argtypes = [_P, ctypes.c_int, _P, ctypes.c_int, _P, _P]
    lib.spslam_track_refkf_vote_batch_device.argtypes = [_P, ctypes.c_int, _P, _P, _P]


class TrackGraph:
    """GPU tracking-graph bookkeeping on a context (its ORB tables give mvInvLevelSigma2)."""

    def __init__(self, ex: spslam_gpu.OrbExtractor):
        self.ex = ex
        _bind(ex.lib)

    def batch_device(self, n_frames: int, stage: int, batch: TrackBatch, stream=0):
        self.ex._check(self.ex.lib.spslam_track_graph_batch_device(self.ex.ctx, n_frames, stage,
                                                                    ctypes.byref(batch), stream or None))

    def refkf_device(self, n_frames: int, stage: int, mm: TrackBatch, rk: RefkfBatch, stream=0):
        self.ex._check(self.ex.lib.spslam_track_refkf_batch_device(self.ex.ctx, n_frames, stage, ctypes.byref(mm),
                                                                    ctypes.byref(rk), stream or None))

    def refkf_vote_device(self, n_frames: int, mm: TrackBatch, vote: RefkfVote, stream=0):
        self.ex._check(self.ex.lib.spslam_track_refkf_vote_batch_device(self.ex.ctx, n_frames, ctypes.byref(mm),
                                                                         ctypes.byref(vote), stream or None))

    def update_local_map_device(self, n_frames: int, mm, lmap: LocalMap, out: LocalMapOut, stream=0):
        """mm: the first graph's TrackBatch, or None when lmap.frame_rows is given."""
        self.ex._check(self.ex.lib.spslam_track_update_local_map_batch_device(
            self.ex.ctx, n_frames, ctypes.byref(mm) if mm is not None else None, ctypes.byref(lmap),
            ctypes.byref(out), stream or None))

    def update_local_map(self, tables, frame_rows, local_kfs=(), capacity=None, points=None, local_frame=None):
        """One frame on host arrays.  tables: the LOCAL_MAP_TABLES arrays of one sequence (point_bad / kf_bad may be
        missing or None); frame_rows: the keypoints' point rows (-1 = none); local_kfs: the list the frame slot held
        before; points: the spslam_local_point table when the records are wanted.  Returns a dict: local_kfs,
        kf_max, local_rows, status and, with points, records (and local_frame when one was given)."""
        T = {}
        for name, dt in LOCAL_MAP_TABLES:
            a = tables.get(name)
            T[name] = None if a is None else np.ascontiguousarray(a, dt).reshape(-1)
        nk, n_rows = len(T["parent"]), len(T["obs_off"]) - 1
        fr = np.ascontiguousarray(frame_rows, np.int32).reshape(-1)
        capacity = len(T["match_row"]) if capacity is None else capacity
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        m = LocalMap(frame_rows=ptr(fr), n_kf=nk, **{name: ptr(T[name]) for name, _ in LOCAL_MAP_TABLES})
        kfs = np.full(max(nk, 1), -1, np.int32)
        kfs[:len(local_kfs)] = np.asarray(local_kfs, np.int32)
        scal = np.array([len(local_kfs), -9, -9, -9], np.int32)  # n_local_kfs, kf_max, n_local, status
        rows = np.full(max(capacity, 1), -1, np.int32)
        o = LocalMapOut(local_kfs=kfs.ctypes.data, n_local_kfs=scal.ctypes.data, kf_max=scal.ctypes.data + 4,
                        n_local=scal.ctypes.data + 8, status=scal.ctypes.data + 12, local_rows=rows.ctypes.data,
                        capacity=capacity)
        if points is not None:
            import spslam_match
            pts = np.ascontiguousarray(points, spslam_match.LOCAL_POINT_DTYPE)
            rec = np.zeros(max(capacity, 1), spslam_match.LOCAL_POINT_DTYPE)
            m.points, o.records = ptr(pts), rec.ctypes.data
            if local_frame is not None:
                lf = np.array(local_frame, spslam_match.LOCAL_FRAME_DTYPE).reshape(())
                o.local_frames = lf.ctypes.data
        self.ex._check(self.ex.lib.spslam_track_update_local_map(self.ex.ctx, ctypes.byref(m), n_rows, len(fr),
                                                                  ctypes.byref(o)))
        res = dict(local_kfs=kfs[:scal[0]].copy(), kf_max=int(scal[1]), local_rows=rows[:scal[2]].copy(),
                   status=int(scal[3]))
        if points is not None:
            res["records"] = rec[:scal[2]].copy()
            if local_frame is not None:
                res["local_frame"] = lf
        return res

    def masked_copy_device(self, n_frames: int, flags: int, regions, stream=0):
        """regions: [(dst tensor, src tensor)] of n_frames equal rows each (contiguous, byte sizes multiple of 4)."""
        arr = (FrameRegion * len(regions))()
        for k, (d, sv) in enumerate(regions):
            fb = d.numel() * d.element_size() // n_frames
            assert d.is_contiguous() and sv.is_contiguous() and sv.numel() * sv.element_size() == fb * n_frames
            arr[k] = FrameRegion(d.data_ptr(), sv.data_ptr(), fb, fb, fb)
        self.ex._check(self.ex.lib.spslam_masked_frame_copy_device(self.ex.ctx, n_frames, flags, len(regions), arr,
                                                                    stream or None))
