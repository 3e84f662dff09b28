"""Scalar restatement of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:219-464) with
ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-823), CheckDistEpipolarLine (:140-157),
KeyFrame::UnprojectStereo (src/KeyFrame.cc:632-648) and LocalMapping::ComputeF12 (:548-565), written from the
reference: what spslam_search_for_triangulation_batch_device / spslam_triangulate_batch_device /
spslam_create_new_points_batch_device are compared with, exactly.

A keyframe: dict(keys (mvKeys), kun (mvKeysUn), ur (mvuRight), depth (mvDepth), desc [n, 32], has (GetMapPoint(i) !=
NULL, uint8), fv (dict nodes / start / features: the FeatureVector CSR), Tcw [4, 4] float32, Ow [3]).
A camera: camera(fx, fy, cx, cy, bf, scale) -- invfx = 1.0f/fx, mb = bf/fx as Frame holds them (Frame.cc:118-124),
mvLevelSigma2 = scale*scale (ORBextractor.cc:425-437).  Both keyframes share it: the reference's second right-image
error reads the *current* keyframe's mbf (:418), which is the same number here.

Float readings
  * cv::Mat products (R2w*Cw + t2w, Rwc*xn, Twc.R*x3Dc + Twc.t): each row summed in double, rounded once.
  * Mat::dot: the products summed in double from 0, in element order; the value stays a double.
  * cv::norm of a 3-vector: squares accumulated in float ((x*x + y*y) + z*z, not contracted), root in double, the
    value a double (Fuse's reading).  So cosParallaxRays = float(dot / (norm1*norm2)), all in double.
  * cos(2*atan2(mb/2, depth)) is cosf(2.f*atan2f(mb/2, depth)): Timer.h puts `using namespace std` in front of
    LocalMapping.cc, so the float overloads are taken (tests/test_triangulation_host.py compiles the expression).
  * invz = 1.0/z: divided in double, rounded to float.  5.991*sigma2, 7.8*sigma2, 3.84*sigma2: double products,
    compared in double with the widened float on the other side.
  * scalar float expressions with the contractions g++ -O3 -march=native emits (pinned by the compiler probe):
      ex = fma(fx*C2x, invz, cx); distex*distex + distey*distey = fma(dx, dx, dy*dy);
      a = fma(x1, F00, y1*F10) + F20 (b, c alike); num = fma(a, x2, b*y2) + c; den = fma(a, a, b*b);
      dsqr = num*num/den; u = fma(fx*x, invz, cx); u_r = fma(-mbf, invz, u);
      e2 = fma(eX, eX, eY*eY), e3 = fma(eR, eR, e2).
  * x3D.rowRange(0,3)/x3D(3): the MatExpr scale 1./w is a double, applied in double, rounded once per coordinate
    (unpinned OpenCV arithmetic, like the SVD).
  * the rows of A: xn*Tcw.row(2) - Tcw.row(k), a float multiply then a float subtract.
  * UnprojectStereo reads mvKeys (distorted) and Twc: rotation Rcw transposed, translation Ow (KeyFrame::SetPose,
    KeyFrame.cc:76-89).  Precondition: mvuRight >= 0 implies mvDepth > 0 (the reference returns an empty Mat and
    then reads it otherwise).

The 4x4 SVD (:334-349) is un-vendored third-party arithmetic; its semantics here are chosen:
one-sided Jacobi on the columns of A, see jacobi_null_vector.
"""
import ctypes

import numpy as np

from matcher_ref import (HISTO, descriptor_distance, f32 as _f, fma, mat3,  # noqa: F401 (other files import these
                         rotation_bin, three_maxima)                        # from here)

TH_LOW = 50
NEW, NO_MATCH, LOW_PARALLAX, W_ZERO, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, SCALE = range(10)
FROM_SVD, FROM_STEREO_1, FROM_STEREO_2 = range(3)
SEARCHED, SKIPPED, SHORT_BASELINE = range(3)
RESULT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("idx2", "<i4"), ("status", "u1"),
                         ("source", "u1"), ("pad", "<u2")])
JACOBI_SWEEPS = 30
JACOBI_EPS = 2.0 ** -22          # 2*FLT_EPSILON, OpenCV's choice for float matrices

_libm = ctypes.CDLL("libm.so.6")
_libm.atan2f.restype, _libm.atan2f.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
_libm.cosf.restype, _libm.cosf.argtypes = ctypes.c_float, [ctypes.c_float]


def _d(x):
    return np.float64(x)


def camera(fx, fy, cx, cy, bf, scale):
    fx, fy, cx, cy, bf = (_f(v) for v in (fx, fy, cx, cy, bf))
    scale = [_f(s) for s in scale]
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, invfx=_f(1.0) / fx, invfy=_f(1.0) / fy, mb=bf / fx, scale=scale,
                sigma2=[s * s for s in scale], scale_factor=scale[1] if len(scale) > 1 else _f(1.0))


def camera_centre(Tcw):
    """KeyFrame.cc:82: Ow = -Rwc*tcw."""
    T = np.asarray(Tcw, np.float32).reshape(4, 4)
    return np.array(mat3(T, T[:3, 3], transpose=True, sign=-1.0), np.float32)


def norm3(v):
    """cv::norm of three floats: a double."""
    s = _f(v[0]) * _f(v[0])
    s = s + _f(v[1]) * _f(v[1])
    s = s + _f(v[2]) * _f(v[2])
    with np.errstate(all="ignore"):
        return np.sqrt(_d(s))


def dot3(a, b):
    """Mat::dot of three floats: a double."""
    s = _d(0.0)
    for k in range(3):
        s = s + _d(a[k]) * _d(b[k])
    return s


# ---------------------------------------------------------------- SearchForTriangulation
def epipole(kf1, kf2, cam):
    """:664-670.  C2.z == 0 gives inf / NaN, as in C."""
    C2 = mat3(kf2["Tcw"], kf1["Ow"], c=np.asarray(kf2["Tcw"], np.float32).reshape(4, 4)[:3, 3])
    with np.errstate(all="ignore"):
        invz = _f(1.0) / C2[2]
        ex = fma(cam["fx"] * C2[0], invz, cam["cx"])
        ey = fma(cam["fy"] * C2[1], invz, cam["cy"])
    return ex, ey


def epipolar_line(k1, F12):
    F = np.asarray(F12, np.float32).reshape(3, 3)
    x, y = _f(k1["x"]), _f(k1["y"])
    with np.errstate(all="ignore"):
        a = fma(x, F[0, 0], y * F[1, 0]) + F[2, 0]
        b = fma(x, F[0, 1], y * F[1, 1]) + F[2, 1]
        c = fma(x, F[0, 2], y * F[1, 2]) + F[2, 2]
    return a, b, c


def check_dist_epipolar_line(line, k2, sigma2, trace=None):
    """:140-157 with the line of kp1 already made."""
    a, b, c = line
    with np.errstate(all="ignore"):
        num = fma(a, _f(k2["x"]), b * _f(k2["y"])) + c
        den = fma(a, a, b * b)
        if den == 0:
            return False
        dsqr = num * num / den
    if trace is not None:
        trace.append((float(dsqr), 3.84 * float(sigma2[int(k2["octave"])])))
    return bool(_d(dsqr) < _d(3.84) * _d(sigma2[int(k2["octave"])]))


def search_for_triangulation(kf1, kf2, F12, only_stereo, check_orientation, cam, trace=None):
    """:657-823.  Returns (match12 [n1] with -1 for none, nmatches).  trace (a dict) receives per idx1 the list of
    (idx2, dist, epipole test passed, epipolar test passed) of the candidates that reached :722."""
    n1 = len(kf1["kun"])
    ex, ey = epipole(kf1, kf2, cam)
    match12 = np.full(n1, -1, np.int32)
    hist = [[] for _ in range(HISTO)]
    nmatches = 0
    pos2 = {int(n): j for j, n in enumerate(kf2["fv"]["nodes"])}
    fv1, fv2 = kf1["fv"], kf2["fv"]
    for a, node in enumerate(fv1["nodes"]):
        b = pos2.get(int(node))
        if b is None:
            continue
        for p in range(fv1["start"][a], fv1["start"][a + 1]):
            idx1 = int(fv1["features"][p])
            if kf1["has"][idx1]:                                    # :699
                continue
            stereo1 = kf1["ur"][idx1] >= 0
            if only_stereo and not stereo1:
                continue
            k1 = kf1["kun"][idx1]
            line = epipolar_line(k1, F12)
            best, best2 = TH_LOW, -1
            seen = []
            for q in range(fv2["start"][b], fv2["start"][b + 1]):
                idx2 = int(fv2["features"][q])
                if kf2["has"][idx2]:                                # :722 (vbMatched2 is never set)
                    continue
                stereo2 = kf2["ur"][idx2] >= 0
                if only_stereo and not stereo2:
                    continue
                d = descriptor_distance(kf1["desc"][idx1], kf2["desc"][idx2])
                if d > TH_LOW or d > best:                          # :736
                    continue
                k2 = kf2["kun"][idx2]
                pole_ok = True
                if not stereo1 and not stereo2:                     # :741
                    with np.errstate(all="ignore"):
                        dx, dy = ex - _f(k2["x"]), ey - _f(k2["y"])
                        if fma(dx, dx, dy * dy) < _f(100) * cam["scale"][int(k2["octave"])]:
                            pole_ok = False
                line_ok = pole_ok and check_dist_epipolar_line(line, k2, cam["sigma2"])
                seen.append((idx2, d, pole_ok, line_ok))
                if line_ok:                                         # :749
                    best, best2 = d, idx2
            if trace is not None:
                trace[idx1] = seen
            if best2 >= 0:
                match12[idx1] = best2
                nmatches += 1
                if check_orientation:
                    hist[rotation_bin(k1["angle"], kf2["kun"][best2]["angle"])].append(idx1)
    if check_orientation:
        keep = three_maxima([len(h) for h in hist])
        if trace is not None:
            trace["hist"] = [len(h) for h in hist]
            trace["keep"] = keep
        for i in range(HISTO):
            if i in keep:
                continue
            for idx1 in hist[i]:
                match12[idx1] = -1
                nmatches -= 1
    return match12, nmatches


# ---------------------------------------------------------------- the 4x4 null vector
def jacobi_null_vector(A, info=None):
    """vt.row(3) of A = u w vt by one-sided (Hestenes) Jacobi on the four columns of A, after the model of OpenCV's
    JacobiSVDImpl_: pairs (i, j), i < j, in fixed order; a pair is skipped when |p| <= eps*sqrt(a*b); a sweep that
    rotates nothing ends it, as do 30 sweeps.  Columns and V rows are floats; squared norms, the dot product and
    the rotation parameters are doubles made of + - * / sqrt only.  Singular values sorted descending by a stable
    selection (the first largest of the rest moves up)."""
    A = np.asarray(A, np.float32).reshape(4, 4)
    At = [[_f(A[r, c]) for r in range(4)] for c in range(4)]
    V = [[_f(1.0 if r == c else 0.0) for c in range(4)] for r in range(4)]
    sweeps = 0
    with np.errstate(all="ignore"):
        W = []
        for i in range(4):
            s = _d(0.0)
            for k in range(4):
                s = s + _d(At[i][k]) * _d(At[i][k])
            W.append(s)
        for _ in range(JACOBI_SWEEPS):
            changed = False
            sweeps += 1
            for i in range(3):
                for j in range(i + 1, 4):
                    a, b = W[i], W[j]
                    p = _d(0.0)
                    for k in range(4):
                        p = p + _d(At[i][k]) * _d(At[j][k])
                    if abs(p) <= _d(JACOBI_EPS) * np.sqrt(a * b):
                        continue
                    p = p * _d(2.0)
                    beta = a - b
                    gamma = np.sqrt(p * p + beta * beta)
                    if beta < 0:
                        delta = (gamma - beta) * _d(0.5)
                        s = np.sqrt(delta / gamma)
                        c = p / (gamma * s * _d(2.0))
                    else:
                        c = np.sqrt((gamma + beta) / (gamma * _d(2.0)))
                        s = p / (gamma * c * _d(2.0))
                    a = b = _d(0.0)
                    for k in range(4):
                        x, y = _d(At[i][k]), _d(At[j][k])
                        t0, t1 = _f(c * x + s * y), _f(c * y - s * x)
                        At[i][k], At[j][k] = t0, t1
                        a = a + _d(t0) * _d(t0)
                        b = b + _d(t1) * _d(t1)
                    W[i], W[j] = a, b
                    for k in range(4):
                        x, y = _d(V[i][k]), _d(V[j][k])
                        V[i][k], V[j][k] = _f(c * x + s * y), _f(c * y - s * x)
                    changed = True
            if not changed:
                break
        for i in range(4):
            s = _d(0.0)
            for k in range(4):
                s = s + _d(At[i][k]) * _d(At[i][k])
            W[i] = np.sqrt(s)
    order = [0, 1, 2, 3]
    for i in range(3):
        j = i
        for k in range(i + 1, 4):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            order[i], order[j] = order[j], order[i]
    if info is not None:
        info["sweeps"] = sweeps
        info["w"] = [float(w) for w in W]
    return [V[order[3]][k] for k in range(4)]


def triangulation_matrix(xn1, xn2, T1, T2):
    """:336-340: float multiply, float subtract."""
    A = np.zeros((4, 4), np.float32)
    with np.errstate(all="ignore"):
        for k in range(4):
            A[0, k] = xn1[0] * T1[2, k] - T1[0, k]
            A[1, k] = xn1[1] * T1[2, k] - T1[1, k]
            A[2, k] = xn2[0] * T2[2, k] - T2[0, k]
            A[3, k] = xn2[1] * T2[2, k] - T2[1, k]
    return A


# ---------------------------------------------------------------- one match of :298-443
def unproject_stereo(kf, idx, cam):
    """KeyFrame.cc:632-648."""
    z = _f(kf["depth"][idx])
    u, v = _f(kf["keys"][idx]["x"]), _f(kf["keys"][idx]["y"])
    x = (u - cam["cx"]) * z * cam["invfx"]
    y = (v - cam["cy"]) * z * cam["invfy"]
    return mat3(kf["Tcw"], [x, y, z], c=kf["Ow"], transpose=True)


def reprojection(T, x3D, z, kp, ur, stereo, cam):
    """:374-426 for one keyframe: (u, v, u_r, the squared error, its bound as a double)."""
    x = _f(dot3(T[0, :3], x3D) + _d(T[0, 3]))
    y = _f(dot3(T[1, :3], x3D) + _d(T[1, 3]))
    sigma2 = cam["sigma2"][int(kp["octave"])]
    with np.errstate(all="ignore"):
        invz = _f(_d(1.0) / _d(z))
        u = fma(cam["fx"] * x, invz, cam["cx"])
        v = fma(cam["fy"] * y, invz, cam["cy"])
        u_r = fma(-cam["bf"], invz, u)
        eX, eY = u - _f(kp["x"]), v - _f(kp["y"])
        e2 = fma(eX, eX, eY * eY)
        if not stereo:
            return u, v, u_r, e2, _d(5.991) * _d(sigma2)
        eR = u_r - _f(ur)
        return u, v, u_r, fma(eR, eR, e2), _d(7.8) * _d(sigma2)


def _reprojection_fails(T, x3D, z, kp, ur, stereo, cam):
    _, _, _, e, bound = reprojection(T, x3D, z, kp, ur, stereo, cam)
    return bool(_d(e) > bound)


def triangulate_match(kf1, kf2, idx1, idx2, cam, info=None):
    """:298-443 for the pair (idx1, idx2).  Returns (status, source, x3D as three floats).  x3D is what the
    reference held at the exit (zeros where none was made)."""
    info = {} if info is None else info
    T1 = np.asarray(kf1["Tcw"], np.float32).reshape(4, 4)
    T2 = np.asarray(kf2["Tcw"], np.float32).reshape(4, 4)
    kp1, kp2 = kf1["kun"][idx1], kf2["kun"][idx2]
    ur1, ur2 = _f(kf1["ur"][idx1]), _f(kf2["ur"][idx2])
    stereo1, stereo2 = bool(ur1 >= 0), bool(ur2 >= 0)
    zero = [_f(0.0)] * 3
    with np.errstate(all="ignore"):
        xn1 = [(_f(kp1["x"]) - cam["cx"]) * cam["invfx"], (_f(kp1["y"]) - cam["cy"]) * cam["invfy"], _f(1.0)]
        xn2 = [(_f(kp2["x"]) - cam["cx"]) * cam["invfx"], (_f(kp2["y"]) - cam["cy"]) * cam["invfy"], _f(1.0)]
        ray1 = mat3(T1, xn1, transpose=True)
        ray2 = mat3(T2, xn2, transpose=True)
        cos_rays = _f(dot3(ray1, ray2) / (norm3(ray1) * norm3(ray2)))
        cos_s1 = cos_s2 = cos_rays + _f(1.0)
        if stereo1:
            cos_s1 = _f(_libm.cosf(_f(2.0) * _f(_libm.atan2f(cam["mb"] / _f(2.0), _f(kf1["depth"][idx1])))))
        elif stereo2:
            cos_s2 = _f(_libm.cosf(_f(2.0) * _f(_libm.atan2f(cam["mb"] / _f(2.0), _f(kf2["depth"][idx2])))))
        cos_stereo = cos_s2 if cos_s2 < cos_s1 else cos_s1           # std::min(cos_s1, cos_s2)
        info.update(cos_rays=cos_rays, cos_stereo=cos_stereo, types=(stereo1, stereo2))
        if cos_rays < cos_stereo and cos_rays > 0 and (stereo1 or stereo2 or _d(cos_rays) < _d(0.9998)):
            source = FROM_SVD
            A = triangulation_matrix(xn1, xn2, T1, T2)
            info["A"] = A
            v = jacobi_null_vector(A, info)
            info["v"] = v
            if v[3] == 0:                                            # :345
                return W_ZERO, source, zero
            inv_w = _d(1.0) / _d(v[3])
            x3D = [_f(_d(v[k]) * inv_w) for k in range(3)]
        elif stereo1 and cos_s1 < cos_s2:
            source = FROM_STEREO_1
            x3D = unproject_stereo(kf1, idx1, cam)
        elif stereo2 and cos_s2 < cos_s1:
            source = FROM_STEREO_2
            x3D = unproject_stereo(kf2, idx2, cam)
        else:
            return LOW_PARALLAX, FROM_SVD, zero                      # :360
        z1 = _f(dot3(T1[2, :3], x3D) + _d(T1[2, 3]))
        if z1 <= 0:
            return BEHIND_1, source, x3D
        z2 = _f(dot3(T2[2, :3], x3D) + _d(T2[2, 3]))
        if z2 <= 0:
            return BEHIND_2, source, x3D
        if _reprojection_fails(T1, x3D, z1, kp1, ur1, stereo1, cam):
            return REPROJ_1, source, x3D
        if _reprojection_fails(T2, x3D, z2, kp2, ur2, stereo2, cam):
            return REPROJ_2, source, x3D
        dist1 = _f(norm3([x3D[k] - _f(kf1["Ow"][k]) for k in range(3)]))
        dist2 = _f(norm3([x3D[k] - _f(kf2["Ow"][k]) for k in range(3)]))
        if dist1 == 0 or dist2 == 0:
            return ZERO_DIST, source, x3D
        ratio_dist = dist2 / dist1
        ratio_octave = cam["scale"][int(kp1["octave"])] / cam["scale"][int(kp2["octave"])]
        ratio_factor = _f(1.5) * cam["scale_factor"]
        info.update(ratio_dist=ratio_dist, ratio_octave=ratio_octave)
        if ratio_dist * ratio_factor < ratio_octave or ratio_dist > ratio_octave * ratio_factor:
            return SCALE, source, x3D
    return NEW, source, x3D


def triangulate_all(kf1, kf2, match12, cam, infos=None):
    """One record per key-1 feature (RESULT_DTYPE) and the number of SPSLAM_TRI_NEW."""
    out = np.zeros(len(match12), RESULT_DTYPE)
    for i, m in enumerate(match12):
        if m < 0:
            out[i]["idx2"], out[i]["status"] = -1, NO_MATCH
            continue
        info = {}
        st, src, x = triangulate_match(kf1, kf2, i, int(m), cam, info)
        if infos is not None:
            infos[i] = info
        out[i]["x"], out[i]["y"], out[i]["z"] = x
        out[i]["idx2"], out[i]["status"], out[i]["source"] = m, st, src
    return out, int((out["status"] == NEW).sum())


# ---------------------------------------------------------------- ComputeF12 and the whole call
def _mat33(A, B):
    """3x3 cv::Mat product: each element summed in double, rounded once."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    C = np.zeros((3, 3), np.float32)
    for r in range(3):
        for c in range(3):
            s = 0.0
            for k in range(3):
                s += float(A[r, k]) * float(B[k, c])
            C[r, c] = _f(s)
    return C


def _inv33(M):
    """cv::Mat::inv of a 3x3 (unpinned): adjugate over determinant in double, rounded once."""
    m = np.asarray(M, np.float64)
    det = (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
           + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))
    adj = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            i0, i1 = [k for k in range(3) if k != c]
            j0, j1 = [k for k in range(3) if k != r]
            adj[r, c] = (-1) ** (r + c) * (m[i0, j0] * m[i1, j1] - m[i0, j1] * m[i1, j0])
    return (adj / det).astype(np.float32)


def compute_f12(kf1, kf2, K):
    """:548-565.  The tests' F12; the device entries take F12 as an input, as SearchForTriangulation does."""
    T1 = np.asarray(kf1["Tcw"], np.float32).reshape(4, 4)
    T2 = np.asarray(kf2["Tcw"], np.float32).reshape(4, 4)
    R12 = _mat33(T1[:3, :3], T2[:3, :3].T)
    M = (-R12).astype(np.float32)
    t12 = [_f(sum(float(M[r, k]) * float(T2[k, 3]) for k in range(3)) + float(T1[r, 3])) for r in range(3)]
    z = _f(0.0)
    tx = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], np.float32)
    K = np.asarray(K, np.float32).reshape(3, 3)
    return _mat33(_mat33(_mat33(_inv33(K.T), tx), R12), _inv33(K)).reshape(9)


def baseline_is_short(kf1, kf2, cam):
    """:258-264 (not monocular): baseline < pKF2->mb, floats."""
    return bool(_f(norm3([_f(kf2["Ow"][k]) - _f(kf1["Ow"][k]) for k in range(3)])) < cam["mb"])


def create_new_map_points(model, k1, neighbours, cam, K, skip=()):
    """The whole of :219-464 for keyframe k1 over model = dict(kfs={k: keyframe with "points": {idx: pid}},
    points={pid: dict(x3D, obs={k: idx})}); "has" of a keyframe is derived from its points.  skip: neighbours the
    caller's CheckNewKeyFrames decision drops.  Returns per neighbour (pair status, match12, records) and nnew.
    Two key-1 features may take one idx2: the second AddMapPoint overwrites the first (the first point keeps its
    observation of pKF2)."""
    kfs, points = model["kfs"], model["points"]
    rounds, nnew = [], 0
    for k2 in neighbours:
        kf1, kf2 = kfs[k1], kfs[k2]
        if k2 in skip:
            rounds.append((SKIPPED, None, None))
            continue
        if baseline_is_short(kf1, kf2, cam):                        # :263
            rounds.append((SHORT_BASELINE, None, None))
            continue
        for kf in (kf1, kf2):
            kf["has"] = np.array([i in kf["points"] for i in range(len(kf["kun"]))], np.uint8)
        F12 = compute_f12(kf1, kf2, K)
        match12, _ = search_for_triangulation(kf1, kf2, F12, False, False, cam)   # ORBmatcher(0.6, false)
        rec, _ = triangulate_all(kf1, kf2, match12, cam)
        for idx1 in range(len(match12)):                            # vMatchedPairs is in idx1 order
            if rec[idx1]["status"] != NEW:
                continue
            pid = len(points)
            idx2 = int(match12[idx1])
            points[pid] = dict(x3D=(rec[idx1]["x"], rec[idx1]["y"], rec[idx1]["z"]), obs={k1: idx1, k2: idx2})
            kf1["points"][idx1] = pid                               # AddMapPoint
            kf2["points"][idx2] = pid
            nnew += 1
        rounds.append((SEARCHED, match12, rec))
    return rounds, nnew
