"""The cases of the OptimizeSim3 tests (tests/test_sim3_opt_host.py guards what each reaches,
tests/test_gpu_sim3_opt.py runs them on the device) and the binding of their referee (tests/sim3_opt_ref.cpp, compiled
here with g++ -ffp-contract=off): two small synthetic keyframes whose matched map points are related by a known
similarity S12, observed with pixel noise, with planted outliers.

A case is dict(name, cam, kf1, kf2, match12, pair, th2, min_inliers, truth, planted): a keyframe is dict(Tcw, kun,
match_row); pair holds s12, R12, t12 (the start); truth is (R, t, s) in float64; planted lists the KF1 keypoints whose
observation was moved far off.  All cases share one point table (points, point_bad).  One context has one camera, so
K1 = K2 in every case: two different cameras cannot be expressed through the C ABI.

The seams are the kernel's (sp-slam_amd/csrc/sim3_opt_kernels.hip): GATHER keypoints per gather chunk, CHUNK
correspondences per edge pass (one thread per edge), WAVE correspondences per wave of a pass.
"""
import ctypes
import functools
import pathlib
import subprocess
import tempfile

import numpy as np

import sim3_solver_cases as SC

ROOT = pathlib.Path(__file__).resolve().parents[1]
GATHER, CHUNK, WAVE = 256, 128, 32   # kThreads, kChunk, 64 lanes / 2 edges
TH2, MIN_INLIERS = 10.0, 20
MAX_TRIALS, MAX_LIN = 160, 16        # (5 + 10) iterations of at most 10 trials; 15 linearisations

RESULT_DTYPE = np.dtype([("n_in", "<i4"), ("n_corr", "<i4"), ("n_bad", "<i4"), ("status", "<i4"), ("accepted", "<i4"),
                         ("iterations1", "<i4"), ("trials1", "<i4"), ("iterations2", "<i4"), ("trials2", "<i4"),
                         ("pad", "<i4"), ("S12", "<f8", 8), ("Scw", "<f8", 8), ("mScw", "<f4", 16)])
assert RESULT_DTYPE.itemsize == 232
OK, TOO_FEW = 0, 1


def cameras():
    import synth
    return {k: np.array([c["fx"], c["fy"], c["cx"], c["cy"]], np.float32) for k, c in (("TUM3", synth.TUM3), ("ICL", synth.ICL))}


@functools.lru_cache(maxsize=None)
def inv_sigma2():
    """mvInvLevelSigma2 of the default pyramid (8 levels of 1.2), as the library's context builds it."""
    scale = SC.geo()[11:].astype(np.float32)
    sigma2 = (scale * scale).astype(np.float32)
    out = (np.float32(1.0) / sigma2).astype(np.float32)
    assert len(out) == 8
    return out


def project(cam, X):
    X = np.asarray(X, np.float64)
    return np.stack([cam[0] * X[:, 0] / X[:, 2] + cam[2], cam[1] * X[:, 1] / X[:, 2] + cam[3]], 1)


class Builder:
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

    def case(self, name, n_in, n_out=0, seed=0, noise=0.3, start=None, s=1.0, extra=7, th2=TH2, cam="TUM3",
             octaves=None, marginal=(), edit=None, angle=0.25, full=False, identity=False):
        """n_in + n_out correspondences among n_in + n_out + extra KF1 keypoints (full: every keypoint matched); noise:
        pixel sigma on both observations; the last n_out observations in KF1 are moved 40 .. 60 px; marginal: (index,
        du, dv) moves single observations of KF1; start: (axis, angle, dt) composed onto the truth, else the truth;
        edit(kf1, kf2, match12, kept) may damage the tables afterwards."""
        import spslam_gpu
        rng = np.random.default_rng(seed)
        K = cameras()[cam].astype(np.float64)
        n = n_in + n_out
        z = rng.uniform(1.0, 4.0, n)
        X1 = np.stack([rng.uniform(-0.45, 0.45, n) * z, rng.uniform(-0.35, 0.35, n) * z, z], 1)
        R, t = SC.rotation((0.2, 1.0, 0.1), angle), np.array([0.3, -0.1, 0.2])
        if identity:
            R, t = np.eye(3), np.zeros(3)
        X2 = (X1 - t) @ R / s
        n1, n2 = (n, n) if full else (n + extra, n + extra - 2)
        where1 = sorted(rng.choice(n1, n, replace=False).tolist())
        where2 = rng.choice(n2, n, replace=False).tolist()
        T1, T2 = SC.pose((1, 2, 3), 0.3, (0.1, -0.2, 0.3)), SC.pose((-2, 1, 1), -0.4, (-0.3, 0.1, 0.2))
        if identity:
            T1 = T2 = np.eye(4)
        kfs = []
        for m, T in ((n1, T1), (n2, T2)):
            kun = np.zeros(m, spslam_gpu.KEYPOINT_DTYPE)
            kun["octave"] = rng.integers(0, 8, m) if octaves is None else octaves
            kun["x"], kun["y"] = rng.uniform(0, 640, m), rng.uniform(0, 480, m)
            kfs.append(dict(Tcw=T.astype(np.float32).reshape(16), kun=kun, match_row=np.full(m, -1, np.int32)))
        o1 = project(K, X1) + rng.normal(0, noise, (n, 2)) if n else np.zeros((0, 2))
        o2 = project(K, X2) + rng.normal(0, noise, (n, 2)) if n else np.zeros((0, 2))
        for j in range(n_in, n):
            ang = rng.uniform(0, 2 * np.pi)
            o1[j] += rng.uniform(40, 60) * np.array([np.cos(ang), np.sin(ang)])
        for j, du, dv in marginal:
            o1[j] += (du, dv)
        match12 = np.full(n1, -1, np.int32)
        for j in range(n):
            for kf, T, X, w, o in ((kfs[0], T1, X1[j], where1[j], o1[j]), (kfs[1], T2, X2[j], where2[j], o2[j])):
                Xw = np.linalg.inv(T) @ np.append(X, 1.0)
                kf["match_row"][w] = self.row(Xw[:3])
                kf["kun"]["x"][w], kf["kun"]["y"][w] = o
            match12[where1[j]] = where2[j]
        Rs, ts = R, t
        if start is not None:
            D = SC.rotation(start[0], start[1])
            Rs, ts = D @ R, D @ t + np.asarray(start[2])
        pair = np.concatenate([[s], Rs.reshape(9), ts]).astype(np.float32)
        c = dict(name=name, cam=cam, kf1=kfs[0], kf2=kfs[1], match12=match12, pair=pair, th2=np.float32(th2),
                 min_inliers=MIN_INLIERS, truth=(R, t, s), planted=[where1[j] for j in range(n_in, n)],
                 where1=where1, noise=noise, started_at_truth=start is None)
        if edit:
            edit(self, c)
        self.cases.append(c)
        return c


OFF = ((1.0, -0.5, 0.3), 0.04, (0.03, -0.02, 0.04))   # a start 0.04 rad and 5 cm off the truth
FAR = ((0.3, 1.0, -0.2), 0.25, (0.2, -0.15, 0.25))    # a start far off: trials get rejected


@functools.lru_cache(maxsize=None)
def build():
    """(points, point_bad, cases)."""
    B = Builder()
    # ---- correspondence counts: 0, 1, around the ten of :2444, around the wave, chunk and gather seams, 300
    B.case("n0", 0, seed=1)
    B.case("n1", 1, seed=2)
    for n in (9, 10, 11):
        B.case(f"n{n}", n, seed=10 + n, start=OFF)
    for n in (WAVE - 1, WAVE, WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1, GATHER - 1, GATHER, GATHER + 1):
        B.case(f"n{n}", n - 3, 3, seed=100 + n, start=OFF)
    B.case("n300_full", 280, 20, seed=300, start=OFF, full=True)
    # ---- the two checks: n_corr - n_bad at 9 and at 10; n_bad == 0 and n_bad > 0
    B.case("left_9", 9, 3, seed=20, start=OFF)
    B.case("left_10", 10, 3, seed=21, start=OFF)
    B.case("clean_40", 40, 0, seed=22, start=OFF)
    B.case("dirty_40", 34, 6, seed=23, start=OFF)

    # ---- the gather: a missing row and a bad point on either side, match12 = -1; octaves over all levels
    def damage(B, c):
        k1, k2, m = c["kf1"], c["kf2"], c["match12"]
        kept = np.flatnonzero(m >= 0)
        B.bad[k1["match_row"][kept[1]]] = 1
        B.bad[k2["match_row"][m[kept[2]]]] = 1
        k1["match_row"][kept[3]] = -1
        k2["match_row"][m[kept[4]]] = -1
        k1["kun"]["octave"][kept[5:13]] = np.arange(8)
        k2["kun"]["octave"][m[kept[5:13]]] = np.arange(8)[::-1]
        c["dropped"] = [int(i) for i in kept[1:5]]
    B.case("gather_bad_and_missing", 30, 4, seed=30, start=OFF, edit=damage)
    # ---- th2 seams: a clean pair list with one observation 2.4 px off (first check), and one with outliers whose
    # removal moves the estimate between the checks, so that the marginal pair's chi2 grows from 6.36 to 6.52 and a
    # th2 at its final value lets it pass the first check (final check); the seam values come from the referee's
    # trace (all_cases)
    B.case("seam_first_base", 40, 0, seed=40, marginal=((7, 2.0, 1.3),), octaves=0)
    B.case("seam_final_base", 36, 5, seed=41, start=OFF, marginal=((7, 2.2 * np.cos(2.8), 2.2 * np.sin(2.8)),), octaves=0)
    # ---- start and update size
    B.case("far_with_outliers", 40, 12, seed=50, start=FAR)
    B.case("far_more_outliers", 30, 20, seed=51, start=FAR)
    B.case("noise_free_at_truth", 40, 0, seed=52, noise=0.0)
    B.case("noise_free_off", 40, 0, seed=53, noise=0.0, start=OFF)
    # ---- the input scale stays under a fixed scale
    B.case("scale_1_3", 40, 4, seed=60, s=1.3, start=OFF)
    # ---- a negative fy (ICL); every edge an outlier
    B.case("icl_negative_fy", 40, 5, seed=70, start=OFF, cam="ICL")
    B.case("all_outliers", 0, 30, seed=71)

    # ---- degenerate depth: both poses and S12 are the identity, so that the table rows are camera points and
    # S12.map is exact; one point of KF2 has z = 0, and e12 divides by it: inf errors, a NaN chi2
    def flatten(B, c):
        i = int(np.flatnonzero(c["match12"] >= 0)[3])
        B.rows[c["kf2"]["match_row"][c["match12"][i]]]["xw"] = (0.25, -0.125, 0.0)
        c["flat"] = i
    B.case("z_zero", 30, 0, seed=80, edit=flatten, identity=True)
    # the same with planted outliers: n_bad > 0, and since no NaN trial is ever accepted or ends the loop early, the
    # second optimize runs all of its 10 iterations
    B.case("z_zero_dirty", 30, 4, seed=81, edit=flatten, identity=True)
    points = np.array(B.rows, B.dtype)
    return points, np.array(B.bad, np.uint8), B.cases


# ---------------------------------------------------------------- the referee
@functools.lru_cache(maxsize=None)
def _build_dir():
    return pathlib.Path(tempfile.mkdtemp(prefix="sim3_opt_"))


@functools.lru_cache(maxsize=None)
def compiled(name):
    """tests/<name>.cpp as a shared library: g++ -O2, contraction off."""
    so = _build_dir() / f"{name}.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so),
                    str(ROOT / "tests" / f"{name}.cpp"), "-lquadmath"], check=True)
    return ctypes.CDLL(str(so))


def _args(case, points, bad, th2=None):
    """The arguments the referee and the host build share, and the arrays that must stay alive."""
    import spslam_gpu
    k1, k2 = case["kf1"], case["kf2"]
    keep = [cameras()[case["cam"]], inv_sigma2(), np.ascontiguousarray(k1["Tcw"], np.float32),
            np.ascontiguousarray(k1["kun"], spslam_gpu.KEYPOINT_DTYPE), np.ascontiguousarray(k1["match_row"], np.int32),
            np.ascontiguousarray(k2["Tcw"], np.float32), np.ascontiguousarray(k2["kun"], spslam_gpu.KEYPOINT_DTYPE),
            np.ascontiguousarray(k2["match_row"], np.int32), np.ascontiguousarray(points["xw"], np.float32),
            np.ascontiguousarray(bad, np.uint8), np.ascontiguousarray(case["pair"], np.float32),
            np.array(case["match12"], np.int32), np.zeros((), RESULT_DTYPE)]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    cam, inv, T1, kun1, r1, T2, kun2, r2, xw, b, pair, m, res = keep
    args = [p(cam), p(inv), p(T1), p(kun1), p(r1), len(kun1), p(T2), p(kun2), p(r2), len(kun2), p(xw), p(b), p(pair),
            ctypes.c_float(case["th2"] if th2 is None else th2), case["min_inliers"], p(m), p(res)]
    return args, keep


def reference(case, points, bad, th2=None):
    """The referee on one case: dict(result, match12, trials, lin, chi_first, chi_final, kept, flags,
    chi_first_at_estimate, chi_final_at_estimate, errors_at)."""
    L = compiled("sim3_opt_ref")
    args, keep = _args(case, points, bad, th2)
    n1 = len(case["kf1"]["kun"])
    trials, lin = np.zeros((MAX_TRIALS, 8)), np.zeros((MAX_LIN, 10))
    counts, flags = np.zeros(2, np.int32), np.zeros(2, np.int32)
    chi1, chi2, kept = np.zeros((max(n1, 1), 2)), np.zeros((max(n1, 1), 2)), np.zeros(max(n1, 1), np.int32)
    chi1e, chi2e, at = np.zeros((max(n1, 1), 2)), np.zeros((max(n1, 1), 2)), np.zeros((2, 8))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    L.sim3_opt_ref_run.restype = ctypes.c_int
    n_in = L.sim3_opt_ref_run(*args, p(trials), MAX_TRIALS, p(lin), MAX_LIN, p(counts), p(chi1), p(chi2), p(kept), p(flags),
                              p(chi1e), p(chi2e), p(at))
    res, m = keep[-1], keep[-2]
    assert n_in == int(res["n_in"]) and counts[0] < MAX_TRIALS and counts[1] < MAX_LIN
    n = int(res["n_corr"])
    return dict(result=res.copy(), match12=m.copy(), trials=trials[:counts[0]].copy(), lin=lin[:counts[1]].copy(),
                chi_first=chi1[:n].copy(), chi_final=chi2[:n].copy(), kept=kept[:n].copy(), flags=flags.copy(),
                chi_first_at_estimate=chi1e[:n].copy(), chi_final_at_estimate=chi2e[:n].copy(), errors_at=at)


def host_build(case, points, bad, th2=None):
    """sp-slam_amd/csrc/sim3_opt_math.h built for the host on one case: (result, match12, trials of 5 columns, the two
    estimates the checks evaluated the edges at)."""
    L = compiled("sim3_opt_host")
    args, keep = _args(case, points, bad, th2)
    trials, n_trials, at = np.zeros((MAX_TRIALS, 5)), np.zeros(1, np.int32), np.zeros((2, 8))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    L.sim3_opt_host_run(*args, p(trials), MAX_TRIALS, p(n_trials), p(at))
    return keep[-1].copy(), keep[-2].copy(), trials[:n_trials[0]].copy(), at


def seam(case, points, bad, which, edge):
    """Two adjacent floats (below, above) for th2 such that correspondence `edge`'s larger chi2 at check `which`
    ('chi_first' / 'chi_final') exceeds th2 = below and does not exceed th2 = above, each in its own run (th2 also
    sets the Huber delta, so the chi2 is the run's own)."""
    value = lambda r: float(np.max(r[which][edge]))  # noqa: E731
    t = np.float32(value(reference(case, points, bad)))
    for _ in range(6):                                   # th2 -> the chi2 of the run at that th2, to its fixed point
        t_next = np.float32(value(reference(case, points, bad, t)))
        if t_next == t:
            break
        t = t_next
    cand = [t]
    for _ in range(3):
        cand = [np.nextafter(cand[0], np.float32(-np.inf))] + cand + [np.nextafter(cand[-1], np.float32(np.inf))]
    over = [value(reference(case, points, bad, c)) > float(c) for c in cand]
    for a in range(len(cand) - 1):
        if over[a] and not over[a + 1]:
            return cand[a], cand[a + 1]
    raise AssertionError(("no seam", which, edge, cand, over))


@functools.lru_cache(maxsize=None)
def all_cases():
    """(points, bad, cases with the seam cases added)."""
    points, bad, cases = build()
    cases = list(cases)
    by = {c["name"]: c for c in cases}
    base = by["seam_first_base"]
    ref = reference(base, points, bad)
    e = int(np.argmax(ref["chi_first"].max(1)))
    lo, hi = seam(base, points, bad, "chi_first", e)
    cases += [dict(base, name="seam_first_below", th2=lo, seam_edge=e), dict(base, name="seam_first_above", th2=hi, seam_edge=e)]
    base = by["seam_final_base"]
    ref = reference(base, points, bad)
    # a pair still in the graph whose chi2 grew between the checks, so that it passes the first one
    alive = ref["chi_final"].max(1) >= 0
    grow = np.where(alive, ref["chi_final"].max(1) - ref["chi_first"].max(1), -np.inf)
    grow = np.where(ref["chi_final"].max(1) > 1.0, grow, -np.inf)
    e = int(np.argmax(grow))
    assert grow[e] > 1e-3, grow[e]
    lo, hi = seam(base, points, bad, "chi_final", e)
    cases += [dict(base, name="seam_final_below", th2=lo, seam_edge=e), dict(base, name="seam_final_above", th2=hi, seam_edge=e)]
    return points, bad, cases


@functools.lru_cache(maxsize=None)
def references():
    points, bad, cases = all_cases()
    return [reference(c, points, bad) for c in cases]
