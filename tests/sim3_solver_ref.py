"""Scalar restatement of Sim3Solver (src/Sim3Solver.cc) as LoopClosing::ComputeSim3 drives it, written from the
reference: what spslam_sim3_solver[_batch_device] is compared with, exactly.  The solver keeps its mutable state
and a real mvAllIndices vector, and iterate is the sequential loop with its early return.

The reference draws from DUtils::Random; here the raw rand() values are an input: iteration k of the solver's life
uses rand[3k .. 3k+2], RandomInt(0, size-1) = int(((double)r / ((double)RAND_MAX + 1.0)) * size).

Float readings (those of 3.13-3.17 kept: cv::Mat products with each row summed in double and rounded
once, Mat::dot in double, cv::norm with the squares in float and the root in double, Mat / double and double * Mat
as the element times the double factor rounded once, u = fma(fx, x, cx)).  New here, unpinned (no OpenCV to hold
them against):
  cv::reduce(P, C, 1, SUM)   a row of three summed in float as (c0 + c2) + c1 (OpenCV's reduceC_ keeps two
                             accumulators and joins them last); C / 3 = the sum times the double 1.0/3, rounded
  N11 .. N44                 float sums, left to right
  cv::eigen                  the classical symmetric Jacobi in float on the upper triangle: the pivot is the largest
                             |off-diagonal| entry, tracked per row (indR) and per column (indC), the first of equals;
                             stop at |pivot| <= FLT_EPSILON or after 30*n*n rotations; y = (W[l]-W[k])*0.5,
                             t = |y| + hypot(p, y), s = hypot(p, t), c = t/s, s = p/s, t = (p/t)*p, signs by y < 0;
                             v0 = a0*c - b0*s, v1 = a0*s + b0*c, every step one float rounding; eigenvalues sorted
                             descending by selection (the first largest), eigenvectors as rows; the sign of a row
                             is whatever the rotations leave
  hypot(a, b)                sqrt(a*a + b*b) in double, rounded to float
  atan2, sin, cos            correctly rounded (oracle_ctypes.libm_cr)
  2*ang*vec/norm(vec)        the element times the double (2*ang) * (1.0/norm), rounded
  cv::Rodrigues              in double: theta = sqrt(rx*rx + ry*ry + rz*rz); theta < DBL_EPSILON gives I; else
                             r /= theta (times 1.0/theta), R = (c*I + (1-c)*r*r^T) + s*[r]x, rounded to float
  cv::pow(P3, 2), den        the float square, accumulated in double, row-major; ms12i = (float)(nom/den)
  O1 - ms12i*mR12i*O2        each row of R*O2 summed in double, times the double ms12i, rounded; a float difference
  mvnMaxError                vector<size_t>: 9.210 * sigma2 as a double product, truncated; err < bound compares the
                             float err with the integer converted to float
  err = dist.dot(dist)       the two squares summed in double, rounded to the float err
"""
import numpy as np

import oracle_ctypes
from fuse_ref import projection
from matcher_ref import f32 as _f, mat3

FOUND, NOT_YET, NO_MORE = 0, 1, 2
RESULT_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("iterations_done", "<i4"), ("best_inliers", "<i4"),
                         ("n_inliers", "<i4"), ("s12", "<f4"), ("R12", "<f4", 9), ("t12", "<f4", 3),
                         ("T12", "<f4", 16)])
FLT_EPSILON = _f(1.1920928955078125e-07)
DBL_EPSILON = 2.220446049250313e-16


def ransac_max_its(n, probability=0.99, min_inliers=20, max_iterations=300):
    """SetRansacParameters (:114-138) for N = n >= min_inliers: mRansacMaxIts."""
    import math
    if n == min_inliers:
        its = 1
    else:
        eps = float(_f(_f(min_inliers) / _f(n)))
        its = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(eps, 3)))
    return max(1, min(its, max_iterations))


def sigma2_table(geo):
    return [_f(_f(s) * _f(s)) for s in geo[11:]]                     # mvLevelSigma2 (ORBextractor.cc:425-431)


def atan2_cr(y, x):
    return float(oracle_ctypes.libm_cr(2, [y], [x])[0])


def sincos_cr(x):
    return float(oracle_ctypes.libm_cr(0, [x])[0]), float(oracle_ctypes.libm_cr(1, [x])[0])


def hypot_f(a, b):
    return _f(np.sqrt(np.float64(a) * np.float64(a) + np.float64(b) * np.float64(b)))


def eigen_sym4(N):
    """cv::eigen on a symmetric 4x4 float matrix: (eigenvalues descending, eigenvectors as rows, rotations made)."""
    n = 4
    A = np.array(N, np.float32).reshape(4, 4).copy()
    V = np.eye(4, dtype=np.float32)
    W = np.array([A[i, i] for i in range(n)], np.float32)
    indR, indC = [0] * n, [0] * n

    def row_max(k):
        m, mv = k + 1, abs(A[k, k + 1])
        for i in range(k + 2, n):
            if mv < abs(A[k, i]):
                mv, m = abs(A[k, i]), i
        indR[k] = m

    def col_max(k):
        m, mv = 0, abs(A[0, k])
        for i in range(1, k):
            if mv < abs(A[i, k]):
                mv, m = abs(A[i, k]), i
        indC[k] = m

    for k in range(n):
        if k < n - 1:
            row_max(k)
        if k > 0:
            col_max(k)
    rotations = 0
    with np.errstate(all="ignore"):
        for _ in range(30 * n * n):
            k, mv = 0, abs(A[0, indR[0]])
            for i in range(1, n - 1):
                if mv < abs(A[i, indR[i]]):
                    mv, k = abs(A[i, indR[i]]), i
            l = indR[k]
            for i in range(1, n):
                if mv < abs(A[indC[i], i]):
                    mv, k, l = abs(A[indC[i], i]), indC[i], i
            p = A[k, l]
            if abs(p) <= FLT_EPSILON:
                break
            rotations += 1
            y = _f(np.float64(_f(W[l] - W[k])) * 0.5)
            t = _f(abs(y) + hypot_f(p, y))
            s = hypot_f(p, t)
            c = _f(t / s)
            s = _f(p / s)
            t = _f(_f(p / t) * p)
            if y < 0:
                s, t = -s, -t
            A[k, l] = 0
            W[k] = _f(W[k] - t)
            W[l] = _f(W[l] + t)

            def rotate(M, i0, j0, i1, j1):
                a0, b0 = M[i0, j0], M[i1, j1]
                M[i0, j0] = _f(_f(a0 * c) - _f(b0 * s))
                M[i1, j1] = _f(_f(a0 * s) + _f(b0 * c))

            for i in range(k):
                rotate(A, i, k, i, l)
            for i in range(k + 1, l):
                rotate(A, k, i, i, l)
            for i in range(l + 1, n):
                rotate(A, k, i, l, i)
            for i in range(n):
                rotate(V, k, i, l, i)
            for idx in (k, l):
                if idx < n - 1:
                    row_max(idx)
                if idx > 0:
                    col_max(idx)
    for k in range(n - 1):                                           # the selection sort
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[[m, k]] = W[[k, m]]
            V[[m, k]] = V[[k, m]]
    return W, V, rotations


def rodrigues(vec):
    """cv::Rodrigues of a float 3-vector: the float 3x3."""
    with np.errstate(all="ignore"):
        rx, ry, rz = (np.float64(v) for v in vec)
        theta = np.sqrt(rx * rx + ry * ry + rz * rz)
        if theta < DBL_EPSILON:
            return np.eye(3, dtype=np.float32)
        sn, cs = (np.float64(v) for v in sincos_cr(float(theta)))
        c1, itheta = np.float64(1.0) - cs, np.float64(1.0) / theta
        rx, ry, rz = rx * itheta, ry * itheta, rz * itheta
        rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
        rxm = [np.float64(0.0), -rz, ry, rz, np.float64(0.0), -rx, -ry, rx, np.float64(0.0)]
        eye = [np.float64(1.0 if k % 4 == 0 else 0.0) for k in range(9)]
        return np.array([_f((cs * eye[k] + c1 * rrt[k]) + sn * rxm[k]) for k in range(9)], np.float32).reshape(3, 3)


def mat_mul33(A, B):
    """cv::Mat 3x3 * 3x3: every element summed in double from 0.0, rounded once."""
    out = np.zeros((3, 3), np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                d = np.float64(0.0)
                for k in range(3):
                    d = d + np.float64(A[r, k]) * np.float64(B[k, c])
                out[r, c] = _f(d)
    return out


def compute_sim3(P1, P2, fix_scale, trace=None):
    """:226-337 on the 3x3 float matrices whose columns are the points: (s12, R12, t12, T12, T21)."""
    trace = {} if trace is None else trace
    P1, P2 = np.asarray(P1, np.float32), np.asarray(P2, np.float32)
    with np.errstate(all="ignore"):
        def centroid(P):
            C = [_f(np.float64(_f(_f(P[r, 0] + P[r, 2]) + P[r, 1])) * (np.float64(1.0) / np.float64(3.0)))
                 for r in range(3)]
            Pr = np.array([[_f(P[r, i] - C[r]) for i in range(3)] for r in range(3)], np.float32)
            return Pr, C

        Pr1, O1 = centroid(P1)
        Pr2, O2 = centroid(P2)
        M = mat_mul33(Pr2, Pr1.T)
        N11 = _f(_f(M[0, 0] + M[1, 1]) + M[2, 2])
        N12 = _f(M[1, 2] - M[2, 1])
        N13 = _f(M[2, 0] - M[0, 2])
        N14 = _f(M[0, 1] - M[1, 0])
        N22 = _f(_f(M[0, 0] - M[1, 1]) - M[2, 2])
        N23 = _f(M[0, 1] + M[1, 0])
        N24 = _f(M[2, 0] + M[0, 2])
        N33 = _f(_f(-M[0, 0] + M[1, 1]) - M[2, 2])
        N34 = _f(M[1, 2] + M[2, 1])
        N44 = _f(_f(-M[0, 0] - M[1, 1]) + M[2, 2])
        N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]],
                     np.float32)
        _, evec, rotations = eigen_sym4(N)
        trace.update(N=N, rotations=rotations, quaternion=evec[0].copy())
        q = evec[0]
        sq = _f(q[1] * q[1])
        sq = _f(sq + _f(q[2] * q[2]))
        sq = _f(sq + _f(q[3] * q[3]))
        nrm = np.sqrt(np.float64(sq))
        ang = np.float64(atan2_cr(float(nrm), float(q[0])))
        f = (np.float64(2.0) * ang) * (np.float64(1.0) / nrm)
        vec = [_f(np.float64(q[i]) * f) for i in (1, 2, 3)]
        R = rodrigues(vec)
        if not fix_scale:
            P3 = mat_mul33(R, Pr2)
            nom, den = np.float64(0.0), np.float64(0.0)
            for r in range(3):
                for c in range(3):
                    nom = nom + np.float64(Pr1[r, c]) * np.float64(P3[r, c])
                    den = den + np.float64(_f(P3[r, c] * P3[r, c]))
            trace.update(den=float(den))
            s = _f(nom / den)
        else:
            s = _f(1.0)
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = R
        sRO2 = mat3(T, O2, sign=float(s))
        t = np.array([_f(O1[r] - sRO2[r]) for r in range(3)], np.float32)
        T12, T21 = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
        inv = np.float64(1.0) / np.float64(s)
        for r in range(3):
            for c in range(3):
                T12[r, c] = _f(s * R[r, c])
                T21[r, c] = _f(np.float64(R[c, r]) * inv)
            T12[r, 3] = t[r]
        T21[:3, 3] = mat3(T21, t, sign=-1.0)
    return s, R, t, T12, T21


def _image(geo, X):
    _, u, v, _ = projection(geo, X[0], X[1], X[2])
    return u, v


class Sim3Solver:
    """kf: dict(Tcw, kun, match_row); match12: per KF1 keypoint the KF2 keypoint or -1 (CONTRACT: the points'
    GetIndexInKeyFrame are i1 and match12[i1]); rand: the raw draws; geo: fuse_ref's."""

    def __init__(self, kf1, kf2, points, point_bad, match12, geo, fix_scale, rand, rand_max=2147483647):
        self.geo, self.fix_scale = geo, bool(fix_scale)
        self.rand, self.rand_max = [int(r) for r in rand], int(rand_max)
        self.mN1 = len(match12)
        self.mnIterations, self.mnBestInliers = 0, 0
        self.mvnIndices1, self.mvX3Dc1, self.mvX3Dc2 = [], [], []
        self.mvnMaxError1, self.mvnMaxError2, self.mvAllIndices = [], [], []
        sigma2 = sigma2_table(geo)
        T1 = np.asarray(kf1["Tcw"], np.float32).reshape(4, 4)
        T2 = np.asarray(kf2["Tcw"], np.float32).reshape(4, 4)
        idx = 0
        for i1 in range(self.mN1):                                   # :62
            i2 = int(match12[i1])
            if i2 < 0:                                               # :64
                continue
            row1, row2 = int(kf1["match_row"][i1]), int(kf2["match_row"][i2])
            if row1 < 0:                                             # :69
                continue
            if row2 < 0:                                             # vpMatched12[i1] is KF2's point at match12[i1]
                continue
            if point_bad is not None and (point_bad[row1] or point_bad[row2]):   # :72
                continue
            s1 = sigma2[int(kf1["kun"][i1]["octave"])]               # :81-85, indexKF1 = i1, indexKF2 = i2
            s2 = sigma2[int(kf2["kun"][i2]["octave"])]
            self.mvnMaxError1.append(int(9.210 * float(s1)))         # :87: size_t
            self.mvnMaxError2.append(int(9.210 * float(s2)))
            self.mvnIndices1.append(i1)
            with np.errstate(all="ignore"):
                self.mvX3Dc1.append(mat3(T1, [_f(c) for c in points[row1]["xw"]], c=T1[:3, 3]))   # :95
                self.mvX3Dc2.append(mat3(T2, [_f(c) for c in points[row2]["xw"]], c=T2[:3, 3]))
            self.mvAllIndices.append(idx)
            idx += 1
        self.mvP1im1 = [_image(geo, X) for X in self.mvX3Dc1]        # :108-109
        self.mvP2im2 = [_image(geo, X) for X in self.mvX3Dc2]
        self.N = len(self.mvnIndices1)
        self.set_ransac_parameters()
        self.trace = dict(counts=[], den=[], rotations=[], hyps=[])

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        self.mRansacProb, self.mRansacMinInliers = probability, min_inliers
        self.max_iterations = max_iterations
        if self.N >= min_inliers:                                    # below, iterate returns before it is read
            self.mRansacMaxIts = ransac_max_its(self.N, probability, min_inliers, max_iterations)
        else:
            self.mRansacMaxIts = max_iterations
        self.mnIterations = 0

    def random_int(self, size):
        r = self.rand[self._draw]
        self._draw += 1
        return int((float(r) / (float(self.rand_max) + 1.0)) * size)

    def check_inliers(self, T12, T21):
        """:340-364: (mvbInliersi, mnInliersi)."""
        flags, n = [], 0
        self.errs = []                                               # (err1, err2) per correspondence, for the tests
        with np.errstate(all="ignore"):
            for i in range(self.N):
                P2in1 = mat3(T12, self.mvX3Dc2[i], c=T12[:3, 3])
                P1in2 = mat3(T21, self.mvX3Dc1[i], c=T21[:3, 3])
                a, b = _image(self.geo, P2in1), _image(self.geo, P1in2)
                d1 = (_f(self.mvP1im1[i][0] - a[0]), _f(self.mvP1im1[i][1] - a[1]))
                d2 = (_f(b[0] - self.mvP2im2[i][0]), _f(b[1] - self.mvP2im2[i][1]))
                err1 = _f(np.float64(d1[0]) * np.float64(d1[0]) + np.float64(d1[1]) * np.float64(d1[1]))
                err2 = _f(np.float64(d2[0]) * np.float64(d2[0]) + np.float64(d2[1]) * np.float64(d2[1]))
                ok = bool(err1 < _f(self.mvnMaxError1[i]) and err2 < _f(self.mvnMaxError2[i]))
                self.errs.append((err1, err2))
                flags.append(ok)
                n += ok
        return flags, n

    def iterate(self, n_iterations):
        """:140-207.  Returns (T12 or None, bNoMore, vbInliers, nInliers)."""
        no_more = False
        inliers = np.zeros(self.mN1, np.uint8)
        if self.N < self.mRansacMinInliers:
            return None, True, inliers, 0
        current = 0
        while self.mnIterations < self.mRansacMaxIts and current < n_iterations:
            current += 1
            self._draw = 3 * self.mnIterations
            self.mnIterations += 1
            avail = list(self.mvAllIndices)
            P1, P2 = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32)
            triple = []
            for i in range(3):
                randi = self.random_int(len(avail))
                idx = avail[randi]
                triple.append(idx)
                P1[:, i], P2[:, i] = self.mvX3Dc1[idx], self.mvX3Dc2[idx]
                avail[randi] = avail[-1]
                avail.pop()
            tr = {}
            s, R, t, T12, T21 = compute_sim3(P1, P2, self.fix_scale, tr)
            flags, n = self.check_inliers(T12, T21)
            self.trace["counts"].append(n)
            self.trace["den"].append(tr.get("den"))
            self.trace["rotations"].append(tr["rotations"])
            self.trace["hyps"].append((self.mnIterations - 1, triple, s, R, t, T12, T21, flags))
            if n >= self.mnBestInliers:
                self.mnBestInliers = n
                self.mBestT12, self.mBestRotation, self.mBestTranslation, self.mBestScale = T12, R, t, s
                if n > self.mRansacMinInliers:
                    for i in range(self.N):
                        if flags[i]:
                            inliers[self.mvnIndices1[i]] = 1
                    return self.mBestT12, False, inliers, n
        if self.mnIterations >= self.mRansacMaxIts:
            no_more = True
        return None, no_more, inliers, 0

    def result(self, T12, no_more, n_inliers):
        """The record spslam_sim3_result holds after an iterate."""
        r = np.zeros((), RESULT_DTYPE)
        r["status"] = FOUND if T12 is not None else (NO_MORE if no_more else NOT_YET)
        r["n"], r["iterations_done"], r["best_inliers"] = self.N, self.mnIterations, self.mnBestInliers
        if T12 is not None:
            r["n_inliers"], r["s12"], r["R12"] = n_inliers, self.mBestScale, self.mBestRotation.reshape(9)
            r["t12"], r["T12"] = self.mBestTranslation, T12.reshape(16)
        return r


def filtered_match12(match12, inliers):
    """LoopClosing.cc:315-320."""
    return np.where(np.asarray(inliers) != 0, np.asarray(match12, np.int32), -1).astype(np.int32)


def compute_sim3_round_robin(solvers, per_turn=5):
    """ComputeSim3's loop (:288-344) up to its first Scm: candidates take turns of per_turn iterations until one
    returns a transformation or all are discarded.  Returns (candidate, its iterate's outputs) or (None, None)."""
    discarded = [s is None for s in solvers]
    while not all(discarded):
        for i, s in enumerate(solvers):
            if discarded[i]:
                continue
            T12, no_more, inl, n = s.iterate(per_turn)
            if no_more:
                discarded[i] = True
            if T12 is not None:
                return i, (T12, no_more, inl, n)
    return None, None
