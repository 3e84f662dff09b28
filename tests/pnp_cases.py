"""The cases of the PnPsolver tests (tests/test_pnp_host.py guards what each reaches, tests/test_gpu_pnp.py runs them
on the device), and the two builds they are held against each other with: the referee tests/pnp_ref.cpp and the host
build of the kernels' arithmetic tests/pnp_host.cpp (g++ -O2 -ffp-contract=off).

A case is dict(name, kun, match, kf_rows, rand, rand_iterations, params, calls, Tcw, kinds, kept): kun the frame's
keypoints, match per frame keypoint a keyframe keypoint or -1 (SearchByBoW's format), kf_rows the keyframe's map
points as rows of the shared table (or -1), calls the n_iterations of successive iterate calls on one solver, Tcw the
true pose, kept the frame keypoints the constructor keeps and kinds their nature in that order: 't' a true
correspondence, 'w' a planted wrong one (at least 20 px off).  params is (min_inliers, max_iterations, epsilon); minSet
is 4, th2 5.991 and the probability 0.99 throughout.

The seams are the kernels' (sp-slam_amd/csrc/pnp_kernels.hip): GATHER frame keypoints per gather chunk, WAVE per
ballot, LANES iterations per wave of the hypothesis kernel and candidates per round of the selection.
"""
import ctypes
import functools
import math
import pathlib
import subprocess
import tempfile

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
GATHER, WAVE, LANES = 256, 64, 64
RAND_MAX = 2147483647
PROBABILITY, MIN_SET, TH2 = 0.99, 4, 5.991
TRACKING = (10, 300, 0.5)      # Tracking.cc:1628
LONG = (4, 300, 0.2)           # mRansacMaxIts = 300 from N = 24 on: every wave of the hypothesis kernel
REFINED, BEST_NO_MORE, NO_MORE, OUT_OF_DRAWS = 0, 1, 2, 3

RESULT_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("iterations_done", "<i4"), ("best_inliers", "<i4"),
                         ("n_inliers", "<i4"), ("iteration", "<i4"), ("min_inliers", "<i4"), ("max_its", "<i4"),
                         ("best_Tcw", "<f4", 16), ("Tcw", "<f4", 16)])
PROBLEM_DTYPE = np.dtype([("kf", "<i4"), ("frame_slot", "<i4"), ("match_offset", "<i4"), ("rand_offset", "<i4"),
                          ("inlier_offset", "<i4"), ("best_mask_offset", "<i4"), ("iterations_done", "<i4"),
                          ("best_inliers", "<i4"), ("n_iterations", "<i4"), ("rand_iterations", "<i4"),
                          ("pad", "<i4", 2), ("best_Tcw", "<f4", 16)])
TRACE_DTYPE = np.dtype([("k", "<i4"), ("idx", "<i4", 4), ("n", "<i4"), ("replaced", "<i4"), ("refine_ran", "<i4"),
                        ("refine_n", "<i4"), ("which", "<i4"), ("refine_which", "<i4"), ("singular", "<i4"),
                        ("Rt", "<f8", 12), ("refine_Rt", "<f8", 12)])
assert RESULT_DTYPE.itemsize == 160 and PROBLEM_DTYPE.itemsize == 112 and TRACE_DTYPE.itemsize == 240


@functools.lru_cache(maxsize=None)
def camera():
    import synth
    K = synth.TUM3
    return np.array([K["fx"], K["fy"], K["cx"], K["cy"]], np.float32)


@functools.lru_cache(maxsize=None)
def sigma2():
    """mvLevelSigma2 of the default pyramid (8 levels of 1.2), as the library's context builds it."""
    scale = np.ones(8, np.float32)
    for i in range(1, 8):
        scale[i] = np.float32(scale[i - 1] * np.float32(1.2))
    return (scale * scale).astype(np.float32)


def rand_for(randi, size):
    """A raw rand() value whose RandomInt(0, size - 1) is randi."""
    r = int(math.ceil(randi * (RAND_MAX + 1) / size))
    assert 0 <= r <= RAND_MAX and int((float(r) / (float(RAND_MAX) + 1.0)) * size) == randi, (randi, size, r)
    return r


def draws_for(quad, n):
    """Four raw values that make the solver draw the kept correspondences `quad` (distinct), in order, from n."""
    avail = list(range(n))
    out = []
    for idx in quad:
        pos = avail.index(idx)
        out.append(rand_for(pos, len(avail)))
        avail[pos] = avail[-1]
        avail.pop()
    return out


def random_draws(seed, n_iterations):
    return np.random.default_rng(seed).integers(0, RAND_MAX + 1, 4 * n_iterations).tolist()


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose(axis=(1, 2, 3), angle=0.3, t=(0.1, -0.2, 0.3)):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rotation(axis, angle), t
    return T


def project(T, Xw):
    Xc = np.asarray(Xw, np.float64) @ T[:3, :3].T + T[:3, 3]
    cam = camera().astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([cam[0] * Xc[:, 0] / Xc[:, 2] + cam[2], cam[1] * Xc[:, 1] / Xc[:, 2] + cam[3]], 1)


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

    def add(self, name, kinds, seed, n_frame=None, n_kf=None, noise=0.0, params=TRACKING, calls=(5,), rand=None,
            rand_iterations=None, T=None, coplanar=False, xw=None, drops=True):
        """kinds: per kept correspondence, in the constructor's order, 't' or 'w'.  xw: {kept index: world point}
        overrides.  drops adds two matched entries the constructor must drop, a keyframe keypoint without a point
        row and one whose row is bad; the frame's other keypoints have a match of -1."""
        import spslam_gpu
        rng = np.random.default_rng(seed)
        N = len(kinds)
        n_frame = N + 7 if n_frame is None else n_frame
        n_kf = N + 5 if n_kf is None else n_kf
        n_drop = 2 if drops and n_frame >= N + 3 and n_kf >= N + 2 else 0
        T = pose() if T is None else T
        Tinv = np.linalg.inv(T)
        where_f = np.sort(rng.choice(n_frame, N + n_drop, replace=False))
        drop_pos = set(rng.choice(N + n_drop, n_drop, replace=False).tolist())
        where_k = rng.choice(n_kf, N + n_drop, replace=False)
        kun = np.zeros(n_frame, spslam_gpu.KEYPOINT_DTYPE)
        kun["octave"] = rng.integers(0, 8, n_frame)
        kun["x"], kun["y"] = rng.uniform(0, 640, n_frame), rng.uniform(0, 480, n_frame)
        match, kf_rows = np.full(n_frame, -1, np.int32), np.full(n_kf, -1, np.int32)
        kept, j, n_dropped = [], 0, 0
        for e in range(N + n_drop):
            f, k = int(where_f[e]), int(where_k[e])
            match[f] = k
            if e in drop_pos:
                kf_rows[k] = -1 if n_dropped == 0 else self.row(rng.uniform(-1, 1, 3), bad=True)
                n_dropped += 1
                continue
            z = rng.uniform(1.0, 4.0)
            Xc = np.array([rng.uniform(-0.5, 0.5) * z, rng.uniform(-0.4, 0.4) * z, 2.5 if coplanar else z])
            if coplanar:
                Xc[:2] = Xc[:2] / z * 2.5
            Xw = (Tinv[:3, :3] @ Xc + Tinv[:3, 3]).astype(np.float32)     # map points are floats
            if xw is not None and j in xw:
                Xw = np.asarray(xw[j], np.float32)
            uv = project(T, Xw[None].astype(np.float64))[0]
            if kinds[j] == "w":
                ang, r = rng.uniform(0, 2 * np.pi), rng.uniform(25.0, 90.0)   # well past sqrt(5.991 * 1.2^14) = 8.8 px
                uv = uv + r * np.array([np.cos(ang), np.sin(ang)])
            elif noise:
                uv = uv + rng.normal(0, noise, 2) * np.sqrt(float(sigma2()[kun["octave"][f]]))
            if np.isfinite(uv).all():
                kun["x"][f], kun["y"][f] = uv
            kf_rows[k] = self.row(Xw)
            kept.append(f)
            j += 1
        if N >= 8:
            kun["octave"][kept[:8]] = np.arange(8)                       # every octave is present
        max_its = params[1]
        n_rand = (max_its + sum(calls)) if rand_iterations is None else rand_iterations
        rand = list(random_draws(seed, n_rand) if rand is None else rand)
        rand = (rand + random_draws(seed + 1000, n_rand))[:4 * n_rand]
        self.cases.append(dict(name=name, kun=kun, match=match, kf_rows=kf_rows, rand=np.array(rand, np.int32),
                               rand_iterations=n_rand, params=params, calls=tuple(calls), Tcw=T, kinds="".join(kinds),
                               kept=np.array(kept, np.int32)))
        return self.cases[-1]


def mixed(n_true, n_wrong, seed):
    k = ["t"] * n_true + ["w"] * n_wrong
    np.random.default_rng(seed).shuffle(k)
    return k


@functools.lru_cache(maxsize=None)
def build():
    """(points, point_bad, cases)."""
    B = Builder()
    # ---- N kept around the RANSAC bounds and the gather's seams; noise-free, so a refined pose is checkable
    B.add("n0", [], 1, n_frame=6, n_kf=5, drops=False)
    B.add("n0_frame_empty", [], 2, n_frame=0, n_kf=3, drops=False)
    B.add("n3", ["t"] * 3, 3, params=LONG)                              # N < min = minSet
    B.add("n4", ["t"] * 4, 4, params=LONG)                              # the four draws exhaust the list; N == min
    B.add("n9", ["t"] * 9, 5)                                           # N < min
    B.add("n10", ["t"] * 10, 6, calls=(5, 5))                           # N == min: one iteration, enters, cannot succeed
    B.add("n11", mixed(11, 0, 7), 7)
    B.add("n14", mixed(12, 2, 8), 8)
    B.add("n15", mixed(12, 3, 9), 9)                                    # Tracking's nmatches threshold: mRansacMaxIts 14
    for n in (63, 64, 65):
        B.add(f"n{n}", mixed(n - 20, 20, 10 + n), 10 + n, n_frame=n + 3, n_kf=n + 9)
    for n in (255, 256, 257):
        B.add(f"n{n}", mixed(n - 100, 100, 20 + n), 20 + n, n_frame=n + 3, n_kf=300, calls=(3,))
    B.add("n300", mixed(200, 100, 30), 30, n_frame=330, n_kf=320, calls=(3,))
    # ---- outcomes.  Noise and wrong matches: the first best's Refine fails, the loop goes on, a later record setter's
    # succeeds (the seeds were searched for with the referee; tests/test_pnp_host.py asserts what each reaches)
    B.add("fail_then_refined", mixed(13, 7, 357), 357, noise=0.9, calls=(5,))                 # fails at 7, returns at 23
    B.add("fail_then_refined_next", mixed(14, 6, 330), 330, noise=1.2, calls=(5,))            # fails at 1, returns at 2
    # N = 15: the best of iteration 4 fails; the calls after it carry its mask, which governs 46, 47 and 50 of the
    # last call until iteration 51 sets a new best and succeeds
    B.add("carried_mask_governs", mixed(11, 4, 301), 301, noise=0.6, calls=(5, 5, 5, 60))
    B.add("all_wrong", ["w"] * 24, 50, calls=(5, 40, 5))                # NO_MORE empty at 35, then exactly 5 more
    B.add("out_of_draws", ["w"] * 24, 51, calls=(5, 5, 40), rand_iterations=12)
    # every wave of the hypothesis kernel: 300 iterations without a success, and a success at iteration 70 and 128
    B.add("long_all_wrong", ["w"] * 30, 52, params=LONG, calls=(300,))
    for at in (63, 64, 70, 128, 299):
        kinds = ["t"] * 12 + ["w"] * 18
        rng = np.random.default_rng(60 + at)
        rand = []
        for k in range(300):
            quad = [0, 1, 2, 3] if k == at else rng.choice(np.arange(12, 30), 4, replace=False).tolist()
            rand += draws_for(quad, 30)
        B.add(f"long_first_at_{at}", kinds, 188, params=LONG, calls=(300,), rand=rand, drops=False)   # one scene
    # ---- re-entries: N = 15, min 10, mRansacMaxIts 14; 11 true and 4 wrong, noise-free.  Four-point EPnP is
    # fragile: of the true quads some give 11 inliers, (0, 1, 2, 5) gives 10 and a quad with a wrong one never 10
    # (found with the referee, asserted in tests/test_pnp_host.py).  Iteration 13 succeeds (done == max); 16 succeeds
    # past it on a hypothesis that only equals the best, so the mask carried in governs; a call of 5 without a
    # qualifying hypothesis runs exactly 5; then n == min enters Refine, does not replace, and the carried mask succeeds
    kinds = ["t"] * 11 + ["w"] * 4
    rng = np.random.default_rng(70)
    good = {13: [0, 1, 2, 4], 16: [0, 1, 2, 10], 22: [0, 1, 2, 5]}
    rand = []
    for k in range(40):
        quad = good.get(k) or rng.choice(11, 3, replace=False).tolist() + [int(rng.integers(11, 15))]
        rand += draws_for(quad, 15)
    B.add("reentry", kinds, 70, calls=(5, 5, 5, 5), rand=rand, rand_iterations=40, drops=False)
    B.add("reentry_below_max", ["t"] * 15, 71, calls=(5, 5, 5))         # REFINED at 0, at 1, at 2
    # ---- geometry
    B.add("coplanar", mixed(20, 6, 80), 80, coplanar=True, calls=(5, 5))
    B.add("coplanar_noisy", mixed(20, 6, 81), 81, coplanar=True, noise=0.7, calls=(5, 5, 30))
    # a 4-set with two coincident points, and one of four coincident points: NaN throughout, 0 inliers
    Tinv = np.linalg.inv(pose())
    P = (Tinv[:3, :3] @ np.array([0.2, -0.1, 2.0]) + Tinv[:3, 3]).astype(np.float32)
    kinds = ["t"] * 16 + ["w"] * 4
    rand = draws_for([0, 1, 2, 3], 20) + draws_for([0, 1, 5, 6], 20) + draws_for([7, 8, 9, 10], 20)
    B.add("coincident", kinds, 82, xw={0: P, 1: P, 2: P, 3: P}, rand=rand, calls=(5, 5), drops=False)
    # a point on the camera's plane under the true pose (Zc = 0): no inlier of any pose near the truth
    Pz = (Tinv[:3, :3] @ np.array([0.3, 0.2, 0.0]) + Tinv[:3, 3]).astype(np.float32)
    B.add("zc_zero", ["t"] * 14, 83, xw={5: Pz}, calls=(5,))
    # behind the camera: the hypotheses' signs and determinants get exercised
    back = {j: (Tinv[:3, :3] @ np.array([0.1 * j - 0.5, 0.2, -1.0 - 0.3 * j]) + Tinv[:3, 3]).astype(np.float32)
            for j in range(6)}
    B.add("behind", ["t"] * 18, 84, xw=back, calls=(5, 5, 30), noise=0.5)
    points = np.array(B.rows, B.dtype)
    return points, np.array(B.bad, np.uint8), B.cases


# ---------------------------------------------------------------- the two builds
@functools.lru_cache(maxsize=None)
def compiled(name, flags=("-O2", "-ffp-contract=off")):
    """tests/<name>.cpp as a shared library: g++ -O2, contraction off."""
    so = pathlib.Path(tempfile.mkdtemp(prefix="pnp_")) / f"{name}.so"
    subprocess.run(["g++", *flags, "-std=c++17", "-shared", "-fPIC", "-o", str(so), str(ROOT / "tests" / f"{name}.cpp")],
                   check=True)
    return ctypes.CDLL(str(so))


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


def ransac_tables(params, cap):
    """spslam_pnp_ransac_table's two tables, from the reference's expressions evaluated here (numpy float32 for the
    float steps, math for libm)."""
    mn, mx, eps = params
    max_its, min_n = np.zeros(cap + 1, np.int32), np.zeros(cap + 1, np.int32)
    for n in range(cap + 1):
        m = max(int(np.float32(n) * np.float32(eps)), mn, MIN_SET)
        min_n[n] = m
        if n < m:
            continue
        its = 1.0
        if m != n:
            e = max(np.float32(eps), np.float32(m) / np.float32(n))
            its = math.ceil(math.log(1 - PROBABILITY) / math.log(1 - math.pow(float(e), 3)))
        max_its[n] = max(1, int(its) if its < mx else mx)
    return max_its, min_n


def reference(case, points, bad, capture=False):
    """The referee over the case's calls: dict(results, inliers, best_mask, frame_points (one row per call), trace,
    counters = (sign flips, det flips))."""
    lib = compiled("pnp_ref")
    nf, nc = len(case["kun"]), len(case["calls"])
    res = np.zeros(nc, RESULT_DTYPE)
    inl, bm = np.zeros((nc, max(nf, 1)), np.uint8), np.zeros((nc, max(nf, 1)), np.uint8)
    fp = np.zeros((nc, max(nf, 1)), np.int32)
    cap = 4096
    trace, counters = np.zeros(cap, TRACE_DTYPE), np.zeros(2, np.int32)
    calls = np.array(case["calls"], np.int32)
    xw = np.ascontiguousarray(points["xw"], np.float32)
    mn, mx, eps = case["params"]
    lib.pnp_ref_capture(1 if capture else 0)
    lib.pnp_ref_run.restype = ctypes.c_int
    lib.pnp_ref_run.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int] + \
        [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_float, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 6 + \
        [ctypes.c_int, ctypes.c_void_p]
    kun = np.ascontiguousarray(case["kun"])
    # the inlier / mask / frame_points rows are n_frame wide in the referee
    inl_c, bm_c, fp_c = (np.zeros((nc, nf), t) for t in (np.uint8, np.uint8, np.int32))
    n = lib.pnp_ref_run(_p(camera()), _p(sigma2()), _p(kun), nf, _p(case["match"]), _p(case["kf_rows"]),
                        len(case["kf_rows"]), _p(xw), _p(bad), _p(case["rand"]), case["rand_iterations"], RAND_MAX,
                        PROBABILITY, mn, mx, MIN_SET, eps, TH2, nc, _p(calls), _p(res), _p(inl_c), _p(bm_c), _p(fp_c),
                        _p(trace), cap, _p(counters))
    assert n <= cap
    inl[:, :nf], bm[:, :nf], fp[:, :nf] = inl_c, bm_c, fp_c
    return dict(results=res, inliers=inl[:, :nf], best_mask=bm[:, :nf], frame_points=fp[:, :nf], trace=trace[:n].copy(),
                counters=counters)


@functools.lru_cache(maxsize=None)
def references():
    points, bad, cases = build()
    return [reference(c, points, bad) for c in cases]


def problem_record(case, r, prev, prev_mask):
    """The problem record of call r: the state is what call r - 1 left (prev: its result record)."""
    q = np.zeros((), PROBLEM_DTYPE)
    q["n_iterations"], q["rand_iterations"] = case["calls"][r], case["rand_iterations"]
    if prev is not None:
        q["iterations_done"], q["best_inliers"], q["best_Tcw"] = prev["iterations_done"], prev["best_inliers"], prev["best_Tcw"]
    return q


def host_call(case, points, bad, q, best_mask):
    """One call of the host build.  Returns (result, inliers, best mask after, frame_points or None, hyp (n, which),
    number of Refine evaluations, qr_solve's singular returns)."""
    lib = compiled("pnp_host")
    nf = len(case["kun"])
    mn, mx, eps = case["params"]
    max_its, min_n = ransac_tables(case["params"], max(nf, 1))
    res = np.zeros((), RESULT_DTYPE)
    inl, fp = np.zeros(max(nf, 1), np.uint8), np.full(max(nf, 1), -7, np.int32)
    bm = np.zeros(max(nf, 1), np.uint8)
    bm[:nf] = best_mask[:nf]
    hyp, nref = np.zeros((mx, 2), np.int32), ctypes.c_int(0)
    xw = np.ascontiguousarray(points["xw"], np.float32)
    kun = np.ascontiguousarray(case["kun"])
    lib.pnp_host_call.restype = ctypes.c_int
    lib.pnp_host_call.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int] + \
        [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_float] + \
        [ctypes.c_void_p] * 7
    sing = lib.pnp_host_call(_p(camera()), _p(sigma2()), _p(kun), nf, _p(case["match"]), _p(case["kf_rows"]),
                             len(case["kf_rows"]), _p(xw), _p(bad), _p(case["rand"]), RAND_MAX, _p(max_its), _p(min_n), mx,
                             TH2, q.ctypes.data, res.ctypes.data, inl.ctypes.data, bm.ctypes.data, fp.ctypes.data,
                             hyp.ctypes.data, ctypes.byref(nref))
    pose_returned = int(res["status"]) in (REFINED, BEST_NO_MORE)
    return res, inl[:nf], bm[:nf], fp[:nf] if pose_returned else None, hyp, nref.value, sing
