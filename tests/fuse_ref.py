"""Scalar restatement of ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, float th)
(src/ORBmatcher.cc:825-975) with KeyFrame::GetFeaturesInArea / IsInImage (src/KeyFrame.cc:586-630) and
MapPoint::PredictScale (src/MapPoint.cc:385-400), written from the reference: what spslam_fuse_search_batch_device
is compared with, exactly.

Two statements:
  search_point / snapshot_search   :852-949 for one point, and for a list of points over an unchanging map -- the
                                   device kernel's contract (include/spslam_gpu.h)
  fuse                             the whole call over a small dict map model, the mutation :951-971 included
                                   (MapPoint::Replace MapPoint.cc:177-215, AddObservation :98-109,
                                   ComputeDistinctiveDescriptors :242-307), recording what each point's search saw

Map model
  points: {pid: {"rec": a spslam_local_point record (position, normal, distances, descriptor),
                 "obs": {keyframe: keypoint}, "nobs": Observations(), "bad": bool}}
  kfs:    {k: {"points": {keypoint: pid} (GetMapPoint), "desc": [n, 32] uint8, "ur": mvuRight, "bad": bool}}

Float readings: cv::Mat products summed in double and rounded once; cv::norm(PO) with the squares
accumulated in float and the root in double; the scalar float expressions with the contractions g++ -O3
-march=native emits for them (tests/test_fuse_host.py holds them against the compiler): u = fma(fx, X*invz, cx),
ur = fma(-bf, invz, u), e2 = fma(ex, ex, ey*ey) and fma(er, er, that).  KeyFrame's image bounds are ints
(include/KeyFrame.h:198-201, initialised from the Frame's floats: truncation).

geo: [fx, fy, cx, cy, bf, min_x, max_x, min_y, max_y, grid inverse x, y, mvScaleFactors ...] as
test_oracle_match.make_pairs builds it (the Frame's float bounds).
"""
import ctypes

import numpy as np

import point_refresh_ref
from matcher_ref import descriptor_distance, f32 as _f, fma, mat3, round_f32  # noqa: F401 (other files import these from here)

SEARCHED, SKIPPED, BEHIND, OUTSIDE_IMAGE, OUT_OF_RANGE, VIEW_ANGLE, NO_CANDIDATES = range(7)
TH_LOW = 50
RESULT_DTYPE = np.dtype([("best_idx", "<i4"), ("best_dist", "<i2"), ("level", "u1"), ("status", "u1")])

_libm = ctypes.CDLL("libm.so.6")
_libm.logf.restype, _libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]


def inv_level_sigma2(scale):
    """ORBextractor.cc:425-437: mvLevelSigma2 = s*s, mvInvLevelSigma2 = 1.0f / that."""
    return [_f(1.0) / _f(_f(s) * _f(s)) for s in scale]


def projection(geo, X, Y, z):
    """:859-870 on p3Dc = (X, Y, z): invz, u, v, ur."""
    fx, fy, cx, cy, bf = [_f(v) for v in geo[:5]]
    with np.errstate(all="ignore"):
        invz = _f(1.0) / _f(z)
        x, y = _f(_f(X) * invz), _f(_f(Y) * invz)
        u, v = fma(fx, x, cx), fma(fy, y, cy)
        return invz, u, v, fma(-bf, invz, u)


def chi2_passes(u, v, ur, kpx, kpy, kpr, inv_sigma2):
    """:914-938: True when the candidate is kept."""
    ex, ey = _f(u - kpx), _f(v - kpy)
    e2 = fma(ex, ex, _f(ey * ey))
    if kpr >= 0:                                                   # :914
        er = _f(ur - kpr)
        e2 = fma(er, er, e2)
        return not float(_f(e2 * inv_sigma2)) > 7.8                # :925
    return not float(_f(e2 * inv_sigma2)) > 5.99                   # :936


def search_point(Tcw, p, kun, desc, ur, go, gi, geo, th=3.0, trace=None):
    """:852-949 for the point record p.  Returns (status, level, best_idx, best_dist)."""
    trace = {} if trace is None else trace
    minx, maxx, miny, maxy = [_f(int(v)) for v in geo[5:9]]        # KeyFrame.cc:41: const int mnMinX(F.mnMinX)
    gix, giy = _f(geo[9]), _f(geo[10])
    scale = [_f(v) for v in geo[11:]]
    isg2 = inv_level_sigma2(scale)
    Tcw = np.asarray(Tcw, np.float32).reshape(4, 4)
    tcw = Tcw[:3, 3]
    xw = [_f(c) for c in p["xw"]]
    Pc = mat3(Tcw, xw, c=tcw)                                       # :853
    if Pc[2] < _f(0.0):                                             # :856
        return BEHIND, 0, -1, 256
    invz, u, v, urp = projection(geo, Pc[0], Pc[1], Pc[2])
    if not (u >= minx and u < maxx and v >= miny and v < maxy):     # :867, KeyFrame.cc:629
        return OUTSIDE_IMAGE, 0, -1, 256
    maxd, mind = _f(_f(1.2) * p["max_dist"]), _f(_f(0.8) * p["min_dist"])   # MapPoint.cc:373-383
    Ow = mat3(Tcw, tcw, transpose=True, sign=-1.0)
    PO = [_f(xw[k] - Ow[k]) for k in range(3)]                      # :874
    s = _f(PO[0] * PO[0])
    s = _f(s + _f(PO[1] * PO[1]))
    s = _f(s + _f(PO[2] * PO[2]))
    dist = _f(np.sqrt(np.float64(s)))                               # :875
    if dist < mind or dist > maxd:                                  # :878
        return OUT_OF_RANGE, 0, -1, 256
    dot = float(PO[0]) * float(p["normal"][0]) + float(PO[1]) * float(p["normal"][1])
    dot += float(PO[2]) * float(p["normal"][2])
    trace["view"] = (dot, 0.5 * float(dist))
    if dot < 0.5 * float(dist):                                     # :884
        return VIEW_ANGLE, 0, -1, 256
    lsf = _f(_libm.logf(_f(geo[12])))                               # mfLogScaleFactor = log(mfScaleFactor)
    n_levels = len(scale)
    lvl = int(np.ceil(_f(_f(_libm.logf(_f(p["max_dist"] / dist))) / lsf)))   # MapPoint.cc:393
    lvl = 0 if lvl < 0 else (n_levels - 1 if lvl >= n_levels else lvl)
    r = _f(_f(th) * scale[lvl])                                     # :890
    # KeyFrame::GetFeaturesInArea (KeyFrame.cc:586-625)
    x0 = max(0, int(np.floor(_f(_f(_f(u - minx) - r) * gix))))
    x1 = min(63, int(np.ceil(_f(_f(_f(u - minx) + r) * gix))))
    y0 = max(0, int(np.floor(_f(_f(_f(v - miny) - r) * giy))))
    y1 = min(47, int(np.ceil(_f(_f(_f(v - miny) + r) * giy))))
    trace.update(cells=(x0, x1, y0, y1), u=u, v=v, r=r)
    if x0 >= 64 or x1 < 0 or y0 >= 48 or y1 < 0:
        return NO_CANDIDATES, lvl, -1, 256
    cand = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            c = ix * 48 + iy
            for j in range(go[c], go[c + 1]):
                k = int(gi[j])
                if abs(_f(kun[k]["x"] - u)) < r and abs(_f(kun[k]["y"] - v)) < r:
                    cand.append(k)
    if not cand:                                                    # :894
        return NO_CANDIDATES, lvl, -1, 256
    best, bi = 256, -1
    trace.update(n_cand=len(cand), dists=[], rejected_chi2=[], levels=[])
    for k in cand:                                                  # :903
        o = int(kun[k]["octave"])
        trace["levels"].append(o - lvl)
        if o < lvl - 1 or o > lvl:                                  # :911
            continue
        if not chi2_passes(u, v, urp, _f(kun[k]["x"]), _f(kun[k]["y"]), _f(ur[k]), isg2[o]):
            trace["rejected_chi2"].append((k, descriptor_distance(p["desc"], desc[k]), bool(ur[k] >= 0)))
            continue
        d = descriptor_distance(p["desc"], desc[k])                 # :942
        trace["dists"].append(d)
        if d < best:                                                # :944
            best, bi = d, k
    return SEARCHED, lvl, bi, best


def snapshot_search(Tcw, P, kun, desc, ur, go, gi, geo, th=3.0, skip=None, traces=None):
    """Every point of P against the same map state.  Returns (RESULT_DTYPE records, nFused)."""
    out = np.zeros(len(P), RESULT_DTYPE)
    for i in range(len(P)):
        tr = {}
        if skip is not None and skip[i]:                            # :849 (the caller's flag)
            rec = (SKIPPED, 0, -1, 256)
        else:
            rec = search_point(Tcw, P[i], kun, desc, ur, go, gi, geo, th, tr)
        if traces is not None:
            traces.append(tr)
        out[i]["status"], out[i]["level"], out[i]["best_idx"], out[i]["best_dist"] = rec
    return out, int((out["best_dist"] <= TH_LOW).sum())


# ---------------------------------------------------------------- the whole call on a map model
def compute_distinctive_descriptors(points, kfs, pid):
    """MapPoint.cc:242-307."""
    p = points[pid]
    if p["bad"] or not p["obs"]:                                    # :251, :256
        return
    ds = [kfs[k]["desc"][p["obs"][k]] for k in sorted(p["obs"]) if not kfs[k]["bad"]]   # :261-267
    if not ds:                                                      # :269
        return
    p["rec"]["desc"] = ds[point_refresh_ref.distinctive_descriptor(ds)]   # :272-306


def add_observation(points, kfs, pid, k, idx):
    """MapPoint.cc:98-109."""
    p = points[pid]
    if k in p["obs"]:
        return
    p["obs"][k] = idx
    p["nobs"] += 2 if kfs[k]["ur"][idx] >= 0 else 1


def replace(points, kfs, pid, by):
    """points[pid].Replace(points[by]) (MapPoint.cc:177-215)."""
    if pid == by:
        return
    p = points[pid]
    obs, p["obs"], p["bad"] = p["obs"], {}, True                    # :187-189 (nObs is not reset)
    for k in sorted(obs):
        if k not in points[by]["obs"]:                              # :200
            kfs[k]["points"][obs[k]] = by                           # ReplaceMapPointMatch
            add_observation(points, kfs, by, k, obs[k])
        else:
            kfs[k]["points"].pop(obs[k], None)                      # EraseMapPointMatch
    compute_distinctive_descriptors(points, kfs, by)                # :212


def fuse(points, kfs, k, Tcw, pids, kun, go, gi, geo, th=3.0):
    """The whole call on keyframe k, mutating the model.  Returns (nFused, what each point's search saw:
    None when :849 skipped it, else (status, level, best_idx, best_dist), and the actions taken)."""
    kf = kfs[k]
    n_fused, seen, actions = 0, [], []
    for pid in pids:                                                # :842
        p = points[pid]
        if p["bad"] or k in p["obs"]:                               # :849
            seen.append(None)
            continue
        rec = search_point(Tcw, p["rec"], kun, kf["desc"], kf["ur"], go, gi, geo, th)
        seen.append(rec)
        best_idx, best_dist = rec[2], rec[3]
        if best_dist <= TH_LOW:                                     # :952
            in_kf = kf["points"].get(best_idx)                      # :954
            if in_kf is not None:
                if not points[in_kf]["bad"]:                        # :957
                    if points[in_kf]["nobs"] > p["nobs"]:           # :959
                        replace(points, kfs, pid, in_kf)
                        actions.append(("replaced_by_kf_point", pid, in_kf))
                    else:
                        replace(points, kfs, in_kf, pid)
                        actions.append(("replaces_kf_point", pid, in_kf))
                else:
                    actions.append(("kf_point_bad", pid, in_kf))
            else:
                add_observation(points, kfs, pid, k, best_idx)      # :967
                kf["points"][best_idx] = pid                        # :968
                actions.append(("added", pid, best_idx))
            n_fused += 1                                            # :970
    return n_fused, seen, actions
