"""The cases of the Sim3Solver tests (tests/test_sim3_solver_host.py guards what each reaches,
tests/test_gpu_sim3_solver.py runs them on the device): pairs of small synthetic keyframes whose matched map points
are related by a known similarity, with outliers, and hand-made draws that pick chosen triples.

A case is dict(name, kf1, kf2, match12, fix_scale, rand, min_inliers, max_iterations, calls, state): a keyframe is
dict(Tcw, kun, match_row) (the solver reads nothing else); calls lists the n_iterations of successive iterate
calls on one solver; state, if given, is (iterations_done, best_inliers) forced before the first call.  All cases
share one point table (points, point_bad).  reference(case) returns, per call, (result record, inlier bytes,
filtered match12 or None) and the solver.
"""
import functools
import math

import numpy as np

import sim3_solver_ref as SR

RAND_MAX = 2147483647
PROBABILITY = 0.99


@functools.lru_cache(maxsize=None)
def geo():
    """fuse_ref's geo for synth.TUM3 without distortion: camera, bf, image bounds, grid inverses, mvScaleFactors."""
    import oracle_ctypes
    import synth
    K = synth.TUM3
    scale = oracle_ctypes.OrbOracle().scale_tables()[0]
    return np.concatenate([[K["fx"], K["fy"], K["cx"], K["cy"], K["bf"], 0, 640, 0, 480, 64 / 640, 48 / 480],
                           scale]).astype(np.float32)


def rand_for(randi, size):
    """A raw rand() value whose RandomInt(0, size - 1) is randi."""
    r = int(math.ceil(randi * (RAND_MAX + 1) / size))
    assert 0 <= r <= RAND_MAX and int((float(r) / (float(RAND_MAX) + 1.0)) * size) == randi, (randi, size, r)
    return r


def draws_for(triple, n):
    """Three raw values that make the solver draw the compacted correspondences `triple` (distinct), in order, from
    n: the positions in vAvailableIndices after the swap-with-back removals."""
    avail = list(range(n))
    out = []
    for idx in triple:
        pos = avail.index(idx)
        out.append(rand_for(pos, len(avail)))
        avail[pos] = avail[-1]
        avail.pop()
    return out


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose(axis, angle, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rotation(axis, angle), t
    return T


class Builder:
    """Collects the point table and the cases."""

    def __init__(self):
        import spslam_match
        self.dtype = spslam_match.LOCAL_POINT_DTYPE
        self.rows, self.bad, self.cases = [], [], []

    def row(self, xw, bad=False):
        p = np.zeros((), self.dtype)
        p["xw"] = xw
        self.rows.append(p)
        self.bad.append(1 if bad else 0)
        return len(self.rows) - 1

    def pair(self, n1, n2, X1, X2, seed, where1=None, where2=None, Tcw1=None, Tcw2=None, octaves=None):
        """Keyframes of n1 / n2 keypoints; correspondence j links KF1 keypoint where1[j] (camera-frame point X1[j])
        with KF2 keypoint where2[j] (X2[j]).  Returns (kf1, kf2, match12)."""
        import spslam_gpu
        rng = np.random.default_rng(seed)
        m = len(X1)
        where1 = sorted(rng.choice(n1, m, replace=False).tolist()) if where1 is None else where1
        where2 = rng.choice(n2, m, replace=False).tolist() if where2 is None else where2
        T1 = pose((1, 2, 3), 0.3, (0.1, -0.2, 0.3)) if Tcw1 is None else Tcw1
        T2 = pose((-2, 1, 1), -0.4, (-0.3, 0.1, 0.2)) if Tcw2 is None else Tcw2
        kfs = []
        for n, T in ((n1, T1), (n2, T2)):
            kun = np.zeros(n, spslam_gpu.KEYPOINT_DTYPE)
            kun["octave"] = rng.integers(0, 8, n) if octaves is None else octaves
            kun["x"], kun["y"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
            kfs.append(dict(Tcw=T.astype(np.float32).reshape(16), kun=kun, match_row=np.full(n, -1, np.int32)))
        match12 = np.full(n1, -1, np.int32)
        for j in range(m):
            for kf, T, X, w in ((kfs[0], T1, X1[j], where1[j]), (kfs[1], T2, X2[j], where2[j])):
                Xw = np.linalg.inv(T) @ np.append(np.asarray(X, np.float64), 1.0)
                kf["match_row"][w] = self.row(Xw[:3])
            match12[where1[j]] = where2[j]
        return kfs[0], kfs[1], match12

    def add(self, name, kf1, kf2, match12, rand, fix_scale=True, min_inliers=6, max_iterations=300, calls=(5,),
            state=None):
        rand = list(rand) + [0] * (3 * max_iterations - len(rand))
        self.cases.append(dict(name=name, kf1=kf1, kf2=kf2, match12=np.asarray(match12, np.int32),
                               fix_scale=fix_scale, rand=np.array(rand[:3 * max_iterations], np.int32),
                               min_inliers=min_inliers, max_iterations=max_iterations, calls=tuple(calls),
                               state=state))


def scene(n_in, n_out, seed, s=1.0, axis=(0.2, 1.0, 0.1), angle=0.25, t=(0.3, -0.1, 0.2), noise=0.0):
    """Camera-frame points: X1 = s*R*X2 + t for the first n_in correspondences, unrelated for the n_out after."""
    rng = np.random.default_rng(seed)
    n = n_in + n_out
    z = rng.uniform(1.0, 4.0, n)
    X1 = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)
    R = rotation(axis, angle)
    X2 = (X1 - np.asarray(t)) @ R / s                                 # R^T (X1 - t) / s, row-wise
    X2[:n_in] += rng.normal(0, noise, (n_in, 3)) if noise else 0
    zo = rng.uniform(1.0, 4.0, n_out)
    X2[n_in:] = np.stack([rng.uniform(-0.5, 0.5, n_out) * zo, rng.uniform(-0.4, 0.4, n_out) * zo, zo], 1)
    return X1, X2


def random_draws(seed, n):
    return np.random.default_rng(seed).integers(0, RAND_MAX + 1, n).tolist()


@functools.lru_cache(maxsize=None)
def build():
    """(points, point_bad, cases)."""
    B = Builder()
    IN = lambda n, k: draws_for(tuple(range(k, k + 3)), n)  # noqa: E731 (three inliers: correspondences k .. k+2)

    # ---- N around the RANSAC bounds
    X1, X2 = scene(5, 0, 1)
    B.add("n_below_min", *B.pair(9, 7, X1, X2, 1), random_draws(1, 30))                      # N = 5 = min - 1
    X1, X2 = scene(6, 0, 2)
    B.add("n_equals_min", *B.pair(9, 7, X1, X2, 2), random_draws(2, 30), calls=(5, 5))       # one iteration, NO_MORE
    X1, X2 = scene(3, 0, 3)
    B.add("n3_min3", *B.pair(4, 5, X1, X2, 3), random_draws(3, 30), min_inliers=3, calls=(5,))
    X1, X2 = scene(4, 0, 4, s=1.5)
    B.add("n4_min3_scale", *B.pair(4, 5, X1, X2, 4), random_draws(4, 900), fix_scale=False, min_inliers=3, calls=(5,))
    # ---- N of 63, 64, 65 among 300 keypoints (two chunks of the gather) and N = cap = 300
    for n in (63, 64, 65):
        X1, X2 = scene(n - 20, 20, 10 + n)
        B.add(f"n{n}_of_300", *B.pair(300, 280, X1, X2, n), random_draws(n, 900), calls=(5,))
    X1, X2 = scene(280, 20, 14)
    B.add("n_cap_300", *B.pair(300, 300, X1, X2, 14, where1=list(range(300))), random_draws(14, 900), calls=(2,))
    # ---- KF1 with one keypoint; KF1 without a match
    X1, X2 = scene(1, 0, 15)
    B.add("kf1_one_keypoint", *B.pair(1, 3, X1, X2, 15), random_draws(15, 30))
    k1, k2, m = B.pair(12, 9, *scene(8, 0, 16), 16)
    B.add("kf1_no_match", k1, k2, np.full(12, -1, np.int32), random_draws(16, 30))

    # ---- the gather: bad points and missing rows on either side, octaves over all levels
    X1, X2 = scene(24, 6, 20)
    k1, k2, m = B.pair(40, 36, X1, X2, 20)
    kept = np.flatnonzero(m >= 0)
    B.bad[k1["match_row"][kept[1]]] = 1                              # pMP1 bad
    B.bad[k2["match_row"][m[kept[2]]]] = 1                           # pMP2 bad
    k1["match_row"][kept[3]] = -1                                    # KF1's keypoint lost its point
    k2["match_row"][m[kept[4]]] = -1                                 # KF2's keypoint lost its point
    k1["kun"]["octave"][kept[:8]] = np.arange(8)
    B.add("gather_bad_and_missing", k1, k2, m, random_draws(20, 900), calls=(5, 5))

    # ---- iterations: the first success at 0, 63, 64, the last, never; calls of 1, 5, 64, 65, 300
    def staged(name, at, n_in=8, n_out=16, min_inliers=3, calls=(300,), seed=30, **kw):
        """Every iteration before `at` draws a triple with an outlier (no more than its three inliers), iteration
        `at` draws three inliers; min_inliers = 3 with N = 24 makes mRansacMaxIts 300."""
        X1, X2 = scene(n_in, n_out, seed)
        n = n_in + n_out
        k1, k2, m = B.pair(n + 6, n + 3, X1, X2, seed)
        rng = np.random.default_rng(seed)
        rand = []
        for k in range(300):
            if at is not None and k == at:
                rand += IN(n, 0)
            else:
                o = rng.choice(np.arange(n_in, n), 2, replace=False).tolist()
                rand += draws_for((int(rng.integers(0, n_in)), o[0], o[1]), n)
        B.add(name, k1, k2, m, rand, min_inliers=min_inliers, calls=calls, **kw)

    staged("first_at_0", 0, calls=(1,))
    staged("first_at_63", 63, calls=(64,), seed=31)
    staged("first_at_64", 64, calls=(65,), seed=32)
    staged("first_at_63_in_300", 63, calls=(300,), seed=33)
    staged("first_at_last", 299, calls=(300,), seed=34)
    staged("never", None, calls=(300, 5), seed=35)
    staged("calls_of_5", 22, calls=(5, 5, 5, 5, 5), seed=36)
    staged("one_call_of_all", 22, calls=(300,), seed=36)
    staged("scale_free_at_7", 7, calls=(5, 5), seed=37, fix_scale=False)
    # best_in above and equal to the qualifying count (8 inliers): above refuses it for good, equal takes it
    staged("best_in_above", 3, calls=(10,), seed=38, state=(0, 9))
    staged("best_in_equal", 3, calls=(10,), seed=38, state=(0, 8))
    # ---- iterations_done + n_iterations short of, equal to and past mRansacMaxIts (N = 8, min 6: 9 iterations)
    for name, calls in (("short_of_max", (3, 3)), ("equal_to_max", (4, 5, 1)), ("past_max", (5, 7))):
        X1, X2 = scene(3, 5, 40)
        k1, k2, m = B.pair(10, 10, X1, X2, 40)
        B.add(name, k1, k2, m, random_draws(40, 900), calls=calls)

    # ---- the draws: 0, RAND_MAX, and the swapped-in last element
    X1, X2 = scene(10, 2, 50)
    k1, k2, m = B.pair(14, 13, X1, X2, 50)
    n = 12
    rand = [0, 0, 0,                                                 # positions 0, 0, 0: 0, then the backs 11 and 10
            RAND_MAX, RAND_MAX, RAND_MAX,                            # the last position each time: 11, 10, 9
            rand_for(3, n), rand_for(3, n - 1), rand_for(3, n - 2),  # 3, the swapped-in 11, the swapped-in 10
            rand_for(n - 2, n), rand_for(4, n - 1), rand_for(4, n - 2),   # 10; then 4 and the back 11 moved to 4...
            rand_for(5, n), rand_for(n - 2, n - 1), rand_for(5, n - 2)]   # 5, 10, the swapped-in 11
    B.add("draw_edges", k1, k2, m, rand + random_draws(50, 900), calls=(5,))

    # ---- the error bounds at the truncation seam: octave 0, bound (size_t)9.21 = 9.  Both poses are the identity;
    # two points of KF1 are moved 2.99 px and 3.03 px in u (err1 8.94 and 9.18; KF2 is 0.3 m farther, so err2 is
    # smaller).  An exactly identical pair of triples (no rotation at all) makes norm(vec) = 0 and R = NaN in the
    # reference's own arithmetic: iteration 0 draws one
    rng = np.random.default_rng(60)
    fx = float(geo()[0])
    z = rng.uniform(1.5, 3.0, 12)
    X1 = np.stack([rng.uniform(-0.4, 0.4, 12) * z, rng.uniform(-0.3, 0.3, 12) * z, z], 1)
    X2 = (X1 - np.array([0.05, 0.0, -0.3])) @ rotation((0.1, 1.0, 0.2), 0.05)
    X1[10, 0] += 2.99 * z[10] / fx
    X1[11, 0] += 3.03 * z[11] / fx
    k1, k2, m = B.pair(12, 12, X1, X2, 60, where1=list(range(12)), where2=list(range(12)), Tcw1=np.eye(4),
                       Tcw2=np.eye(4), octaves=0)
    B.add("bound_seam", k1, k2, m, IN(12, 0) + random_draws(60, 30), calls=(1,))
    k1, k2, m = B.pair(12, 12, X1, X1, 61, where1=list(range(12)), where2=list(range(12)), Tcw1=np.eye(4),
                       Tcw2=np.eye(4), octaves=0)
    B.add("identity_motion_is_nan", k1, k2, m, IN(12, 0) + random_draws(61, 30), calls=(1,))

    # ---- degenerate geometry: collinear and coincident triples, z = 0 and z < 0, den = 0
    X1, X2 = scene(10, 0, 70)
    X1[0:3] = [[0.1, 0.1, 2.0], [0.2, 0.2, 2.5], [0.3, 0.3, 3.0]]   # collinear on both sides
    X2[0:3] = X1[0:3] + 0.05
    X1[3:6] = [0.2, -0.1, 2.0]                                       # coincident on both sides
    X2[3:6] = [0.25, -0.1, 2.1]
    X2[6:9] = 1e-23 * X1[6:9] * [1, -1, -1]                          # a half turn about x at scale 1e-23: N stays
    #                                                                  below FLT_EPSILON (no rotation, q = (0,1,0,0)),
    #                                                                  R is finite and P3's squares underflow: den = 0
    X1[9] = [0.3, 0.2, 0.0]                                          # z = 0
    X2[9] = [0.3, 0.2, -1.0]                                         # z < 0
    for fix in (True, False):
        k1, k2, m = B.pair(10, 10, X1, X2, 70, where1=list(range(10)), where2=list(range(10)), Tcw1=np.eye(4),
                           Tcw2=np.eye(4))
        rand = IN(10, 0) + IN(10, 3) + IN(10, 6) + draws_for((9, 0, 4), 10) + draws_for((7, 9, 2), 10)
        B.add(f"degenerate_{'fixed' if fix else 'scale_free'}", k1, k2, m, rand + random_draws(70, 900),
              fix_scale=fix, min_inliers=4, calls=(5, 5))

    # ---- scale-free and fixed-scale successes at ComputeSim3's own parameters (min 20, max 300), with noise
    for name, s, fix, seed in (("loop_fixed", 1.0, True, 80), ("loop_scale_free", 1.3, False, 81),
                               ("loop_fixed_on_scaled", 1.3, True, 82)):
        X1, X2 = scene(30, 8, seed, s=s, noise=0.002)
        B.add(name, *B.pair(50, 45, X1, X2, seed), random_draws(seed, 900), fix_scale=fix, min_inliers=20,
              calls=(5, 5, 5))
    points = np.array(B.rows, B.dtype)
    return points, np.array(B.bad, np.uint8), B.cases


def new_solver(case, points, bad):
    s = SR.Sim3Solver(case["kf1"], case["kf2"], points, bad, case["match12"], geo(), case["fix_scale"], case["rand"],
                      RAND_MAX)
    s.set_ransac_parameters(PROBABILITY, case["min_inliers"], case["max_iterations"])
    if case["state"] is not None:
        s.mnIterations, s.mnBestInliers = case["state"]
    return s


@functools.lru_cache(maxsize=None)
def references():
    """Per case: ([(result record, inlier bytes, filtered match12 or None) per call], the solver after them)."""
    points, bad, cases = build()
    out = []
    for c in cases:
        s = new_solver(c, points, bad)
        calls = []
        for n_it in c["calls"]:
            T12, no_more, inl, n = s.iterate(n_it)
            calls.append((s.result(T12, no_more, n), inl,
                          SR.filtered_match12(c["match12"], inl) if T12 is not None else None))
        out.append((calls, s))
    return out


@functools.lru_cache(maxsize=None)
def chain_case():
    """The real keyframe pair of loop_match_cases with the BoW matches ComputeSim3 would have: the solver's result
    feeds SearchBySim3.  Returns (points, bad, kf1, kf2, match12, rand, geo)."""
    import loop_match_cases as LC
    points, bad, cases, _ = LC.sim3_cases()
    c = next(q for q in cases if q["name"] == "real_ground_truth")
    return points, bad, c["kf1"], c["kf2"], c["match12"], np.array(random_draws(90, 900), np.int32), LC.geo()
