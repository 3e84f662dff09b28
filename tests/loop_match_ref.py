"""Scalar restatements of the four ORBmatcher overloads LoopClosing calls, written from the reference: what the
loop-closing entries of include/spslam_gpu.h are compared with, exactly.

  search_by_bow_kf            SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12)         src/ORBmatcher.cc:522-655
  search_by_sim3              SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12)   :1102-1326
  search_by_projection_sim3   SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)  :290-403
  fuse_sim3_point / fuse_sim3_snapshot / fuse_sim3
                              Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)           :977-1100: one point's search,
                              every point over an unchanging map (the device kernel's contract), and the whole call
                              over fuse_ref's map model with the walk :1082-1096

Float readings: the matcher family's (tests/matcher_ref.py, tests/fuse_ref.py) -- cv::Mat products
summed in double and rounded once, Mat::dot in double, cv::norm with the squares in float and the root in double,
PredictScale through logf, KeyFrame's int bounds and half-open IsInImage, column-major cells, the first in scan
order winning a tie -- and the new ones of DESIGN 3.17, unpinned (no OpenCV to hold them against):
  scw = sqrt(row0.dot(row0))        the dot in double, the double root rounded to the float scw
  sRcw / scw, col3 / scw            OpenCV's Mat / double is a scale by 1.0 / s: the element times the double
                                    reciprocal, rounded once
  Ow = -Rcw.t() * tcw               rows summed in double, negated, rounded (fuse_ref's reading of the same line)
  s12 * R12                         the product in double, rounded: the float product
  (1.0 / s12) * R12.t()             the element times the double reciprocal, rounded once
  -sR21 * t12                       rows summed in double, negated, rounded
With s12 == 1.0f exactly (RGB-D, mbFixScale) every reading of the three Sim3 products gives the same bits.  The Scw
of LoopClosing.cc:337 carries a scale that is 1 only up to rounding, so the decomposition's reading matters there.
The scalar expressions invz, x, y, u, v carry GCC's contractions (tests/test_loop_match_host.py holds them against
the compiler): u = fma(fx, x, cx); :331 has 1/z in float, :1019 / :1166 1.0/z in double, rounded -- the same bits.
"""
import numpy as np

import fuse_ref as FR
from matcher_ref import descriptor_distance, f32 as _f, mat3, rotation_bin, three_maxima

TH_LOW, TH_HIGH = 50, 100
SEARCHED, SKIPPED, BEHIND, OUTSIDE_IMAGE, OUT_OF_RANGE, VIEW_ANGLE, NO_CANDIDATES = range(7)
RESULT_DTYPE = FR.RESULT_DTYPE


# ---------------------------------------------------------------- SearchByBoW(KeyFrame*, KeyFrame*)
def search_by_bow_kf(d1, a1, has1, fv1, d2, a2, has2, fv2, nn_ratio=0.75, check_ori=True, trace=None):
    """:522-655, literally.  d: descriptors, a: mvKeysUn angles, has: vpMapPoints[i] && !isBad(), fv: dict(nodes,
    start, features).  Returns (vpMatches12 as the KF2 keypoint index or -1, nmatches)."""
    trace = {} if trace is None else trace
    n1, n2 = len(d1), len(d2)
    match12 = np.full(n1, -1, np.int32)                              # :534
    matched2 = np.zeros(n2, bool)                                    # :535
    hist = [[] for _ in range(30)]
    nmatches = 0
    nodes1, nodes2 = [int(x) for x in fv1["nodes"]], [int(x) for x in fv2["nodes"]]
    i1, i2 = 0, 0
    trace.update(shared=0, ratio=[], dists=[], blocked=0, second_changed=0)
    while i1 < len(nodes1) and i2 < len(nodes2):                     # :550
        if nodes1[i1] == nodes2[i2]:
            trace["shared"] += 1
            l2 = [int(fv2["features"][q]) for q in range(fv2["start"][i2], fv2["start"][i2 + 1])]
            for p in range(fv1["start"][i1], fv1["start"][i1 + 1]):  # :554
                idx1 = int(fv1["features"][p])
                if not has1[idx1]:                                   # :559-562
                    continue
                b1, bi, b2 = 256, -1, 256
                unblocked = (256, 256)                               # what the scan would see with nothing blocked
                for idx2 in l2:                                      # :570
                    d = None
                    if has2[idx2]:
                        d = descriptor_distance(d1[idx1], d2[idx2])
                        if d < unblocked[0]:
                            unblocked = (d, unblocked[0])
                        elif d < unblocked[1]:
                            unblocked = (unblocked[0], d)
                    if matched2[idx2] or not has2[idx2]:             # :576-580
                        trace["blocked"] += bool(matched2[idx2])
                        continue
                    if d < b1:                                       # :586
                        b2, b1, bi = b1, d, idx2
                    elif d < b2:
                        b2 = d
                trace["dists"].append(b1)
                if b1 < TH_LOW:                                      # :598, strict
                    trace["ratio"].append((b1, b2))
                    if _f(b1) < _f(_f(nn_ratio) * _f(b2)):           # :600
                        trace["second_changed"] += (b1, b2) != unblocked
                        match12[idx1] = bi
                        matched2[bi] = True
                        if check_ori:
                            hist[rotation_bin(a1[idx1], a2[bi])].append(idx1)   # :607-614
                        nmatches += 1
            i1 += 1
            i2 += 1
        elif nodes1[i1] < nodes2[i2]:                                # lower_bound
            while i1 < len(nodes1) and nodes1[i1] < nodes2[i2]:
                i1 += 1
        else:
            while i2 < len(nodes2) and nodes2[i2] < nodes1[i1]:
                i2 += 1
    trace["removed"] = []
    if check_ori:                                                    # :634-652
        keep = three_maxima([len(h) for h in hist])
        for b in range(30):
            if b in keep:
                continue
            for idx1 in hist[b]:
                trace["removed"].append((idx1, int(match12[idx1])))
                match12[idx1] = -1
                nmatches -= 1
    trace["matched2"] = matched2
    return match12, nmatches


# ---------------------------------------------------------------- shared by the three projection searches
def _geo(geo):
    minx, maxx, miny, maxy = [_f(int(v)) for v in geo[5:9]]          # KeyFrame.cc:41: const int mnMinX(F.mnMinX)
    return (minx, maxx, miny, maxy), (_f(geo[9]), _f(geo[10])), [_f(v) for v in geo[11:]]


def norm3(a):
    """cv::norm: the squares summed in float, the root in double."""
    s = _f(a[0] * a[0])
    s = _f(s + _f(a[1] * a[1]))
    s = _f(s + _f(a[2] * a[2]))
    return _f(np.sqrt(np.float64(s)))


def project(geo, Pc):
    """z < 0, invz, x, y, u, v and KeyFrame::IsInImage: (status, u, v)."""
    bounds = _geo(geo)[0]
    if Pc[2] < _f(0.0):
        return BEHIND, None, None
    _, u, v, _ = FR.projection(geo, Pc[0], Pc[1], Pc[2])
    if not (u >= bounds[0] and u < bounds[1] and v >= bounds[2] and v < bounds[3]):   # KeyFrame.cc:629
        return OUTSIDE_IMAGE, u, v
    return SEARCHED, u, v


def in_range(p, dist):
    maxd, mind = _f(_f(1.2) * p["max_dist"]), _f(_f(0.8) * p["min_dist"])   # MapPoint.cc:373-383
    return not (dist < mind or dist > maxd)


def predict_scale(p, dist, geo):
    scale = _geo(geo)[2]
    lsf = _f(FR._libm.logf(_f(geo[12])))                             # mfLogScaleFactor = log(mfScaleFactor)
    lvl = int(np.ceil(_f(_f(FR._libm.logf(_f(p["max_dist"] / dist))) / lsf)))   # MapPoint.cc:393
    return 0 if lvl < 0 else (len(scale) - 1 if lvl >= len(scale) else lvl)


def features_in_area(kun, go, gi, geo, u, v, r):
    """KeyFrame::GetFeaturesInArea (KeyFrame.cc:586-625): vIndices in scan order."""
    (minx, _, miny, _), (gix, giy), _ = _geo(geo)
    x0 = max(0, int(np.floor(_f(_f(_f(u - minx) - r) * gix))))
    x1 = min(63, int(np.ceil(_f(_f(_f(u - minx) + r) * gix))))
    y0 = max(0, int(np.floor(_f(_f(_f(v - miny) - r) * giy))))
    y1 = min(47, int(np.ceil(_f(_f(_f(v - miny) + r) * giy))))
    if x0 >= 64 or x1 < 0 or y0 >= 48 or y1 < 0:
        return []
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            c = ix * 48 + iy
            for j in range(go[c], go[c + 1]):
                k = int(gi[j])
                if abs(_f(kun[k]["x"] - u)) < r and abs(_f(kun[k]["y"] - v)) < r:
                    out.append(k)
    return out


def best_in_window(desc_p, lvl, cand, kun, desc, blocked=None, trace=None):
    """The candidate loop of all three: the octave filter, the smallest distance, the first of equals."""
    best, bi = 256, -1
    for k in cand:
        if blocked is not None and blocked[k]:
            continue
        o = int(kun[k]["octave"])
        if o < lvl - 1 or o > lvl:
            continue
        d = descriptor_distance(desc_p, desc[k])
        if trace is not None:
            trace.setdefault("dists", []).append(d)
        if d < best:
            best, bi = d, k
    return bi, best


def decompose_scw(Scw):
    """:298-303 / :985-990: ([Rcw | tcw] as a 4x4, scw)."""
    S = np.asarray(Scw, np.float32).reshape(4, 4)
    d = float(S[0, 0]) * float(S[0, 0])
    d += float(S[0, 1]) * float(S[0, 1])
    d += float(S[0, 2]) * float(S[0, 2])
    scw = _f(np.sqrt(np.float64(d)))
    T = np.eye(4, dtype=np.float32)
    with np.errstate(all="ignore"):
        inv = np.float64(1.0) / np.float64(scw)
        for r in range(3):
            for c in range(4):
                T[r, c] = _f(np.float64(S[r, c]) * inv)
    return T, scw


def scw_window(Scw, p, geo, th, trace=None):
    """One point of SearchByProjection(pKF, Scw) / Fuse(pKF, Scw) up to its radius: (status, level, u, v, r)."""
    trace = {} if trace is None else trace
    T, _ = decompose_scw(Scw)
    tcw = T[:3, 3]
    xw = [_f(c) for c in p["xw"]]
    with np.errstate(all="ignore"):
        Pc = mat3(T, xw, c=tcw)                                      # Rcw*p3Dw+tcw
        st, u, v = project(geo, Pc)
        if st != SEARCHED:
            return st, 0, u, v, None
        Ow = mat3(T, tcw, transpose=True, sign=-1.0)
        PO = [_f(xw[k] - Ow[k]) for k in range(3)]
        dist = norm3(PO)
        if not in_range(p, dist):
            return OUT_OF_RANGE, 0, u, v, None
        dot = float(PO[0]) * float(p["normal"][0]) + float(PO[1]) * float(p["normal"][1])
        dot += float(PO[2]) * float(p["normal"][2])
        trace["view"] = (dot, 0.5 * float(dist))
        if dot < 0.5 * float(dist):
            return VIEW_ANGLE, 0, u, v, None
        lvl = predict_scale(p, dist, geo)
    r = _f(_f(th) * _geo(geo)[2][lvl])
    trace.update(u=u, v=v, r=r, dist=dist)
    return SEARCHED, lvl, u, v, r


# ---------------------------------------------------------------- Fuse(pKF, Scw, ...)
def fuse_sim3_point(Scw, p, kun, desc, go, gi, geo, th=4.0, trace=None):
    """:1008-1079 for the point record p.  Returns (status, level, best_idx, best_dist)."""
    trace = {} if trace is None else trace
    st, lvl, u, v, r = scw_window(Scw, p, geo, th, trace)
    if st != SEARCHED:
        return st, 0, -1, 256
    cand = features_in_area(kun, go, gi, geo, u, v, r)
    trace["n_cand"] = len(cand)
    if not cand:                                                     # :1053
        return NO_CANDIDATES, lvl, -1, 256
    trace["cand"] = cand
    bi, best = best_in_window(p["desc"], lvl, cand, kun, desc, trace=trace)
    return SEARCHED, lvl, bi, best


def fuse_sim3_snapshot(Scw, P, kun, desc, go, gi, geo, th=4.0, skip=None, traces=None):
    """Every point of P against the same map state.  Returns (RESULT_DTYPE records, nFused)."""
    out = np.zeros(len(P), RESULT_DTYPE)
    for i in range(len(P)):
        tr = {}
        if skip is not None and skip[i]:                             # :1005 (the caller's flag)
            rec = (SKIPPED, 0, -1, 256)
        else:
            rec = fuse_sim3_point(Scw, P[i], kun, desc, go, gi, geo, th, tr)
        if traces is not None:
            traces.append(tr)
        out[i]["status"], out[i]["level"], out[i]["best_idx"], out[i]["best_dist"] = rec
    return out, int((out["best_dist"] <= TH_LOW).sum())


def fuse_sim3(points, kfs, k, Scw, pids, kun, go, gi, geo, th=4.0):
    """The whole call on keyframe k of fuse_ref's map model, the walk :1082-1096 included.  Returns (nFused, what
    each point's search saw: None when :1005 skipped it, vpReplacePoint as pids or None, the actions)."""
    kf = kfs[k]
    already = {pid for pid in kf["points"].values() if not points[pid]["bad"]}   # GetMapPoints, on entry (:993)
    n_fused, seen, actions = 0, [], []
    replace = [None] * len(pids)
    for i, pid in enumerate(pids):
        p = points[pid]
        if p["bad"] or pid in already:                               # :1005
            seen.append(None)
            continue
        rec = fuse_sim3_point(Scw, p["rec"], kun, kf["desc"], go, gi, geo, th)
        seen.append(rec)
        if rec[3] <= TH_LOW:                                         # :1082
            in_kf = kf["points"].get(rec[2])                         # GetMapPoint
            if in_kf is not None:
                if not points[in_kf]["bad"]:                         # :1087
                    replace[i] = in_kf
                    actions.append(("replace", pid, in_kf))
                else:
                    actions.append(("kf_point_bad", pid, in_kf))
            else:
                FR.add_observation(points, kfs, pid, k, rec[2])      # :1092
                kf["points"][rec[2]] = pid                           # :1093
                actions.append(("added", pid, rec[2]))
            n_fused += 1
    return n_fused, seen, replace, actions


# ---------------------------------------------------------------- SearchByProjection(pKF, Scw, ...)
def search_by_projection_sim3(Scw, P, kun, desc, go, gi, geo, th=10.0, skip=None, taken=None, trace=None):
    """:312-400.  taken: vpMatched[idx] != NULL on entry.  Returns (per keypoint the point newly assigned or -1,
    nmatches)."""
    trace = {} if trace is None else trace
    n = len(kun)
    matched = np.zeros(n, bool) if taken is None else np.asarray(taken).astype(bool).copy()
    initially = matched.copy()
    match = np.full(n, -1, np.int32)
    nmatches = 0
    trace.update(rank=[], statuses=[], views=[])
    for i in range(len(P)):
        if skip is not None and skip[i]:                             # :317
            trace["statuses"].append(SKIPPED)
            continue
        tr = {}
        st, lvl, u, v, r = scw_window(Scw, P[i], geo, th, tr)
        trace["statuses"].append(st)
        trace["views"].append(tr.get("view"))
        if st != SEARCHED:
            continue
        cand = features_in_area(kun, go, gi, geo, u, v, r)
        if not cand:                                                 # :364
            continue
        bi, best = best_in_window(P[i]["desc"], lvl, cand, kun, desc, blocked=matched)   # :375
        if best <= TH_LOW:                                           # :394
            # how many better-or-equal candidates the points before this one took inside the loop
            order = sorted((descriptor_distance(P[i]["desc"], desc[k]), n_, k) for n_, k in enumerate(cand)
                           if not initially[k] and lvl - 1 <= int(kun[k]["octave"]) <= lvl)
            trace["rank"].append([k for _, _, k in order].index(bi))
            matched[bi] = True
            match[bi] = i
            nmatches += 1
    return match, nmatches


# ---------------------------------------------------------------- SearchBySim3
def sim3_transforms(s12, R12, t12):
    """:1119-1121: (sR12, sR21, t21) as 4x4 / 3-vectors of floats."""
    s12 = _f(s12)
    R = np.asarray(R12, np.float32).reshape(3, 3)
    t12 = [_f(c) for c in np.asarray(t12, np.float32).reshape(3)]
    sR12, sR21 = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    with np.errstate(all="ignore"):
        inv = np.float64(1.0) / np.float64(s12)
        for r in range(3):
            for c in range(3):
                sR12[r, c] = _f(s12 * R[r, c])
                sR21[r, c] = _f(np.float64(R[c, r]) * inv)
    t21 = mat3(sR21, t12, sign=-1.0)
    return sR12, sR21, t21, t12


def _sim3_side(src, dst, A, ta, points, point_bad, already, geo, th, trace):
    """One of the two searches (:1148-1225 / :1228-1305): vnMatch of `src`'s keypoints in `dst`."""
    vn = np.full(len(src["kun"]), -1, np.int32)
    for i in range(len(src["kun"])):
        row = int(src["match_row"][i])
        if row < 0 or already[i]:                                    # :1152
            continue
        if point_bad is not None and point_bad[row]:                 # :1155
            continue
        p = points[row]
        xw = [_f(c) for c in p["xw"]]
        Tw = np.asarray(src["Tcw"], np.float32).reshape(4, 4)
        with np.errstate(all="ignore"):
            Pa = mat3(Tw, xw, c=Tw[:3, 3])                           # R1w*p3Dw + t1w
            Pb = mat3(A, Pa, c=ta)                                   # sR21*p3Dc1 + t21
            st, u, v = project(geo, Pb)
            trace["statuses"].append(st)
            if st != SEARCHED:
                continue
            dist = norm3(Pb)                                         # cv::norm(p3Dc2): the camera-frame point
            if not in_range(p, dist):
                trace["statuses"][-1] = OUT_OF_RANGE
                continue
            lvl = predict_scale(p, dist, geo)
        r = _f(_f(th) * _geo(geo)[2][lvl])
        cand = features_in_area(dst["kun"], dst["go"], dst["gi"], geo, u, v, r)
        if not cand:
            trace["statuses"][-1] = NO_CANDIDATES
            continue
        bi, best = best_in_window(p["desc"], lvl, cand, dst["kun"], dst["desc"])
        trace["dists"].append(best)
        if best <= TH_HIGH:                                          # :1221
            vn[i] = bi
    return vn


def search_by_sim3(kf1, kf2, points, point_bad, s12, R12, t12, match12, geo, th=7.5, already2=None, trace=None):
    """kf: dict(Tcw, kun, desc, go, gi, match_row).  match12: KF2 keypoint or -1 per KF1 keypoint, on entry.
    vbAlreadyMatched2 is derived from match12 (GetIndexInKeyFrame on a consistent map) unless already2 is given.
    Returns (match12 after, nFound)."""
    trace = {} if trace is None else trace
    n1, n2 = len(kf1["kun"]), len(kf2["kun"])
    m = np.array(match12, np.int32).reshape(-1).copy()
    a1 = m >= 0                                                      # :1134-1137
    if already2 is None:
        a2 = np.zeros(n2, bool)
        for i in range(n1):
            if m[i] >= 0 and m[i] < n2:                              # :1138-1140
                a2[m[i]] = True
    else:
        a2 = np.asarray(already2).astype(bool)
    sR12, sR21, t21, t12f = sim3_transforms(s12, R12, t12)
    trace.update(statuses=[], dists=[])
    vn1 = _sim3_side(kf1, kf2, sR21, t21, points, point_bad, a1, geo, th, trace)
    vn2 = _sim3_side(kf2, kf1, sR12, t12f, points, point_bad, a2, geo, th, trace)
    found = 0
    trace.update(vn1=vn1, vn2=vn2, disagree=0)
    for i1 in range(n1):                                             # :1310-1323
        idx2 = int(vn1[i1])
        if idx2 >= 0:
            if int(vn2[idx2]) == i1:
                m[i1] = idx2
                found += 1
            else:
                trace["disagree"] += 1
    return m, found
