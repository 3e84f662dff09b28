"""Scalar restatement of MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) and
MapPoint::UpdateNormalAndDepth (:330-371) over the tables of spslam_point_refresh_map, written from the reference:
what spslam_map_points_refresh_batch_device is compared with, exactly.

tables: kf_Tcw [n_kf, 16], kf_slot [n_kf], kf_bad [n_kf] or None, obs_off [n_rows + 1], obs_kf / obs_kp (per row in
ascending keyframe order: the project's standing substitution for std::map<KeyFrame*> order), ref_kf [n_rows],
point_bad [n_rows] or None.  keys_un / desc: [n_slots, cap] keypoint records and [n_slots, cap, 32] bytes.

Float readings: the camera centre's three products summed in double in row order, negated, rounded; cv::norm with
the squares accumulated in double, ((x^2 + y^2) + z^2); every other step a float operation of its own.
"""
import math

import numpy as np

from matcher_ref import descriptor_distance, f32 as _f

DESCRIPTOR, NORMAL_DEPTH = 1, 2
DONE, UNTOUCHED, CAPACITY = 0, 1, 2
MAX_OBS = 128


def camera_center(Tcw):
    """KeyFrame::SetPose: Ow = -Rwc * tcw (KeyFrame.cc:82)."""
    T = [float(x) for x in np.asarray(Tcw, np.float32).reshape(16)]
    return [_f(-((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11])) for i in range(3)]


def norm3(v):
    x, y, z = (float(c) for c in v)
    return math.sqrt((x * x + y * y) + z * z)


def distinctive_descriptor(ds, trace=None):
    """:272-306 on the N gathered descriptors: the index of the one with the least median distance."""
    n = len(ds)
    best_median, best = None, 0
    medians = []
    for i in range(n):
        row = sorted(descriptor_distance(ds[i], ds[j]) for j in range(n))   # :292-293, Distances[i][i] = 0 included
        median = row[int(0.5 * (n - 1))]                                     # :294
        medians.append(median)
        if best_median is None or median < best_median:                      # :296 strict: the first smallest
            best_median, best = median, i
    if trace is not None:
        trace["medians"] = medians
    return best


def refresh_row(t, points, row, what, keys_un, desc, scale, trace=None):
    """Both functions on one table row, in place.  Returns the status."""
    trace = {} if trace is None else trace
    o0, o1 = int(t["obs_off"][row]), int(t["obs_off"][row + 1])
    n = o1 - o0
    if (t.get("point_bad") is not None and t["point_bad"][row]) or n <= 0:   # :251 / :256, :338 / :345
        return UNTOUCHED
    if n > MAX_OBS:
        return CAPACITY
    kfs = [int(k) for k in t["obs_kf"][o0:o1]]
    kps = [int(k) for k in t["obs_kp"][o0:o1]]
    bad = t.get("kf_bad")
    if what & DESCRIPTOR:
        ds = [desc[t["kf_slot"][k], kp] for k, kp in zip(kfs, kps) if bad is None or not bad[k]]   # :261-267
        trace["n_desc"] = len(ds)
        if ds:                                                                # :269
            points[row]["desc"] = ds[distinctive_descriptor(ds, trace)]      # :305
    if what & NORMAL_DEPTH:
        X = [_f(c) for c in points[row]["xw"]]
        normal = [_f(0), _f(0), _f(0)]
        nvs = []
        for k in kfs:                                                         # :350 (no isBad() check)
            Ow = camera_center(t["kf_Tcw"][k])
            v = [_f(X[c] - Ow[c]) for c in range(3)]                          # :354
            nv = _f(norm3(v))
            nvs.append(nv)
            normal = [_f(normal[c] + _f(v[c] / nv)) for c in range(3)]        # :355
        ref = int(t["ref_kf"][row])
        r = kfs.index(ref) if ref in kfs else 0                               # absent: the first observer
        trace["ref_index"] = r if ref in kfs else None
        dist = nvs[r]                                                         # :359-360
        level = int(keys_un[t["kf_slot"][kfs[r]], kps[r]]["octave"])          # :361
        max_d = _f(dist * _f(scale[level]))                                   # :367
        points[row]["max_dist"] = max_d
        points[row]["min_dist"] = _f(max_d / _f(scale[len(scale) - 1]))       # :368
        points[row]["normal"] = [_f(normal[c] / _f(n)) for c in range(3)]     # :369
    return DONE


def refresh(t, points, rows, what, keys_un, desc, scale, traces=None):
    """A copy of the table with the listed rows refreshed, and the status per listed row."""
    out = np.array(points)
    status = np.zeros(len(rows), np.uint8)
    for k, row in enumerate(rows):
        tr = {}
        status[k] = refresh_row(t, out, int(row), what, keys_un, desc, scale, tr)
        if traces is not None:
            traces.append(tr)
    return out, status
