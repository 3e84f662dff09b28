"""CPU checks of the OptimizeSim3 referee (tests/sim3_opt_ref.cpp) and its cases (tests/sim3_opt_cases.py):
* every case reaches what it is there for, asserted from the referee's trace;
* the referee's numeric Jacobian agrees with the analytic Jacobian of the two projections over every linearisation;
* the noise-free cases recover the true S12, and exactly the planted outliers are nulled;
* the kernel's arithmetic and driver (sp-slam_amd/csrc/sim3_opt_math.h), built for the host, equal the referee bit for
  bit, and its 7x7 LDLT equals its 6x6 one on embedded systems.
"""
import ctypes

import numpy as np
import pytest

import sim3_opt_cases as C

# The referee's numeric Jacobian (central differences of 1e-9 on errors of up to a few hundred pixels) against the
# analytic one in float64: the largest deviation over the cases' evaluations with |z| >= 0.1, measured here
# (profiles/r18/sim3_opt.md): 2.08e-3, on entries of up to 2e3; the bound is four times that, rounded up to a power
# of two.
TOL_J = 2.0 ** -6
MAX_EXCLUDED = 0.10
# The final S12 of the noise-free cases against the truth (whose map points and poses are rounded to float, 6e-8
# relative): the largest deviation measured here: R 9.23e-9, t 3.54e-8; four times that, rounded up to a power of two.
TOL_R, TOL_T = 2.0 ** -24, 2.0 ** -22


@pytest.fixture(scope="module")
def refs():
    points, bad, cases = C.all_cases()
    return points, bad, cases, C.references()


def named(refs):
    _, _, cases, r = refs
    return {c["name"]: (c, w) for c, w in zip(cases, r)}


def nulled(c, w):
    """The KF1 keypoints whose match the call set to -1."""
    return sorted(np.flatnonzero((c["match12"] >= 0) & (w["match12"] < 0)).tolist())


# ---------------------------------------------------------------- what the cases reach
def test_cases_reach_what_they_are_for(refs):
    N = named(refs)
    res = lambda name: N[name][1]["result"]  # noqa: E731
    # correspondence counts: 0, 1, 9, 10, 11, each seam of the kernel, 300
    want = {"n0": 0, "n1": 1, "n9": 9, "n10": 10, "n11": 11, "n300_full": 300}
    for n in (C.WAVE, C.CHUNK, C.GATHER):
        want.update({f"n{n - 1}": n - 1, f"n{n}": n, f"n{n + 1}": n + 1})
    for name, n in want.items():
        assert int(res(name)["n_corr"]) == n, name
    assert (C.WAVE, C.CHUNK, C.GATHER) == (32, 128, 256)
    assert len(N["n300_full"][0]["kf1"]["kun"]) == 300 and len(N["n257"][0]["kf1"]["kun"]) > C.GATHER
    # g2o optimises nothing without an edge; one pair is optimised and then too few
    assert (int(res("n0")["status"]), int(res("n0")["iterations1"]), int(res("n0")["trials1"])) == (C.TOO_FEW, 0, 0)
    assert int(res("n1")["status"]) == C.TOO_FEW and int(res("n1")["iterations1"]) > 0
    assert int(res("n9")["status"]) == C.TOO_FEW and int(res("n10")["status"]) == C.OK and int(res("n10")["n_in"]) == 10
    # the two checks: n_corr - n_bad at 9 and at 10
    for name, left, status in (("left_9", 9, C.TOO_FEW), ("left_10", 10, C.OK)):
        r = res(name)
        assert int(r["n_corr"]) - int(r["n_bad"]) == left and int(r["n_bad"]) == 3 and int(r["status"]) == status, name
    r = res("left_9")
    assert int(r["n_in"]) == 0 and int(r["iterations2"]) == 0 and len(nulled(*N["left_9"])) == 3   # nulled, then return 0
    assert np.array_equal(r["S12"][4:7], N["left_9"][0]["pair"][10:13].astype(np.float64))        # g2oS12 untouched
    # n_bad == 0: 5 more iterations; n_bad > 0: 10 (no NaN trial is accepted or ends the loop: all of them run)
    assert int(res("clean_40")["n_bad"]) == 0 and int(res("dirty_40")["n_bad"]) == 6
    assert (int(res("z_zero")["n_bad"]), int(res("z_zero")["iterations2"])) == (0, 5)
    assert (int(res("z_zero_dirty")["n_bad"]), int(res("z_zero_dirty")["iterations2"])) == (4, 10)
    # the gather: four entries dropped and left as they were, the unmatched keypoints stay -1, all octaves present
    c, w = N["gather_bad_and_missing"]
    assert int(w["result"]["n_corr"]) == int((c["match12"] >= 0).sum()) - 4
    assert all(w["match12"][i] == c["match12"][i] >= 0 for i in c["dropped"])
    assert not set(c["dropped"]) & set(w["kept"].tolist()) and (w["match12"][c["match12"] < 0] == -1).all()
    assert sorted({int(c["kf1"]["kun"]["octave"][i]) for i in w["kept"]}) == list(range(8))
    assert sorted({int(c["kf2"]["kun"]["octave"][c["match12"][i]]) for i in w["kept"]}) == list(range(8))
    # th2 seams: one float apart, the match flips and nothing else
    for which, chi in (("first", "chi_first"), ("final", "chi_final")):
        (cb, wb), (ca, wa) = N[f"seam_{which}_below"], N[f"seam_{which}_above"]
        assert np.nextafter(cb["th2"], np.float32(np.inf)) == ca["th2"]
        e = cb["seam_edge"]
        assert wb[chi][e].max() > float(cb["th2"]) and 0 <= wa[chi][e].max() <= float(ca["th2"])
        diff = np.flatnonzero(wb["match12"] != wa["match12"])
        assert diff.tolist() == [int(wb["kept"][e])] and wb["match12"][diff[0]] == -1 and wa["match12"][diff[0]] >= 0
        assert int(wa["result"]["n_in"]) == int(wb["result"]["n_in"]) + 1
    (cb, wb), (ca, wa) = N["seam_first_below"], N["seam_first_above"]
    assert (int(wb["result"]["n_bad"]), int(wa["result"]["n_bad"])) == (1, 0)      # and with it 10 or 5 more iterations
    assert (int(wb["result"]["iterations2"]), int(wb["result"]["trials2"])) != \
        (int(wa["result"]["iterations2"]), int(wa["result"]["trials2"]))
    (cb, wb), (ca, wa) = N["seam_final_below"], N["seam_final_above"]
    assert int(wb["result"]["n_bad"]) == int(wa["result"]["n_bad"]) == 5
    e = cb["seam_edge"]
    assert wb["chi_first"][e].max() < float(cb["th2"])                             # it passed the first check
    # rejected trials; a check that reads the errors a rejected trial cached
    w = N["far_with_outliers"][1]
    assert (w["trials"][:, 5] == 0).any() and int(w["result"]["n_bad"]) == 12
    assert N["clean_40"][1]["flags"].tolist() == [1, 1] and N["n11"][1]["flags"].tolist() == [1, 0]
    assert N["n127"][1]["flags"].tolist() == [0, 1] and N["dirty_40"][1]["flags"].tolist() == [0, 0]
    # update size: every real update of the noise-free case started at the truth has theta < 1e-5, the others do not
    assert set(N["noise_free_at_truth"][1]["trials"][:, 6]) == {0.0}
    assert 1.0 in set(N["noise_free_off"][1]["trials"][:, 6]) and 1.0 in set(N["clean_40"][1]["trials"][:, 6])
    assert all(set(w["trials"][:, 6]) <= {0.0, 1.0} for _, w in N.values())        # sigma is 0 under a fixed scale
    # the input scale stays and Scw carries it
    r = res("scale_1_3")
    assert r["S12"][7] == float(np.float32(1.3)) == r["Scw"][7] and int(r["status"]) == C.OK
    s = np.linalg.norm(r["mScw"].reshape(4, 4)[0, :3].astype(np.float64))
    assert abs(s - 1.3) < 1e-6
    # a negative fy; every edge an outlier
    assert C.cameras()["ICL"][1] < 0 and int(res("icl_negative_fy")["status"]) == C.OK
    r = res("all_outliers")
    assert int(r["n_bad"]) == int(r["n_corr"]) == 30 and int(r["status"]) == C.TOO_FEW
    # z = 0: inf errors, a NaN chi2, NaN > th2 is false; the run is bounded and the estimate stays
    for name in ("z_zero", "z_zero_dirty"):
        c, w = N[name]
        e = w["kept"].tolist().index(c["flat"])
        assert np.isnan(w["chi_first"][e][0]) and np.isnan(w["chi_final"][e][0]) and w["match12"][c["flat"]] >= 0
        assert len(w["trials"]) == 15 - (5 if name == "z_zero" else 0) and (w["trials"][:, 7] == 0).all()
        assert np.array_equal(w["result"]["S12"], [0, 0, 0, 1, 0, 0, 0, 1])
    # acceptance: n_in >= 20
    assert int(res("n10")["accepted"]) == 0 and int(res("clean_40")["accepted"]) == 1
    assert {int(w["result"]["status"]) for _, w in N.values()} == {C.OK, C.TOO_FEW}


# ---------------------------------------------------------------- the numeric Jacobian
def camera_points(c, points, kept):
    """P3D1c and P3D2c of the kept correspondences (float products, as the gather makes them)."""
    out = []
    for kf, idx in ((c["kf1"], kept), (c["kf2"], c["match12"][kept])):
        T = kf["Tcw"].reshape(4, 4).astype(np.float64)
        xw = points["xw"][kf["match_row"][idx]].astype(np.float64)
        out.append((xw @ T[:3, :3].T + T[:3, 3]).astype(np.float32).astype(np.float64))
    return out


def analytic_jacobian(S, cam, X, inverse):
    """d error / d update of obs - K project(T X) for T = Sim3(update) * S (e12) or its inverse (e21), update =
    (omega, upsilon, sigma) with sigma fixed: float64."""
    q = S[:4] / np.linalg.norm(S[:4])
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    t, s = S[4:7], S[7]
    skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])  # noqa: E731
    if not inverse:
        p = s * R @ X + t
        dp = np.hstack([-skew(p), np.eye(3)])                 # p + omega x p + upsilon
    else:
        p = R.T @ (X - t) / s
        dp = np.hstack([R.T @ skew(X) / s, -R.T / s])         # S^-1 (X - omega x X - upsilon)
    dproj = np.array([[cam[0] / p[2], 0, -cam[0] * p[0] / p[2] ** 2], [0, cam[1] / p[2], -cam[1] * p[1] / p[2] ** 2]])
    J = np.zeros((2, 7))
    J[:, :6] = -dproj @ dp
    return J, p[2]


def test_numeric_jacobian_agrees_with_the_analytic_one(refs):
    points, bad, cases, r = refs
    L = C.compiled("sim3_opt_ref")
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    worst, total, excluded = 0.0, 0, 0
    for c, w in zip(cases, r):
        if not len(w["kept"]):
            continue
        X1, X2 = camera_points(c, points, w["kept"])
        X = np.ascontiguousarray(np.concatenate([X2, X1]))           # e12 maps X2, e21 maps X1
        kinds = np.repeat([0, 1], len(X1)).astype(np.int32)
        cam = C.cameras()[c["cam"]]
        for lin in w["lin"]:
            S = np.ascontiguousarray(lin[2:])
            J, depth = np.zeros((len(X), 14)), np.zeros(len(X))
            L.sim3_opt_ref_jacobians(p(S), p(cam), len(X), p(X), p(kinds), p(J), p(depth))
            for k in range(len(X)):
                total += 1
                if not abs(depth[k]) >= 0.1:
                    excluded += 1
                    continue
                want, z = analytic_jacobian(S, cam.astype(np.float64), X[k], bool(kinds[k]))
                assert abs(z - depth[k]) < 1e-6
                assert (J[k].reshape(2, 7)[:, 6] == 0).all()          # the scale column is exactly zero
                worst = max(worst, float(np.abs(J[k].reshape(2, 7) - want).max()))
    print(f"numeric Jacobian: {total} evaluations, {excluded} excluded, largest deviation {worst:.3e}")
    assert total > 5000 and excluded <= MAX_EXCLUDED * total
    assert worst <= TOL_J, worst


# ---------------------------------------------------------------- recovery
def test_truth_is_recovered_and_exactly_the_planted_outliers_are_nulled(refs):
    points, bad, cases, r = refs
    worst_R = worst_t = 0.0
    seen = 0
    for c, w in zip(cases, r):
        if c["name"] in ("z_zero", "z_zero_dirty") or not len(w["kept"]):
            continue
        if c["name"].startswith("seam_"):                              # their marginal observation is theirs to judge
            continue
        dropped = set(c.get("dropped", []))
        assert nulled(c, w) == sorted(set(c["planted"]) - dropped), c["name"]
        seen += bool(c["planted"])
        if c["noise"] == 0.0:
            S = w["result"]["S12"]
            q = S[:4] / np.linalg.norm(S[:4])
            x, y, z, qw = q
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * qw), 2 * (x * z + y * qw)],
                          [2 * (x * y + z * qw), 1 - 2 * (x * x + z * z), 2 * (y * z - x * qw)],
                          [2 * (x * z - y * qw), 2 * (y * z + x * qw), 1 - 2 * (x * x + y * y)]])
            worst_R = max(worst_R, float(np.abs(R - c["truth"][0]).max()))
            worst_t = max(worst_t, float(np.abs(S[4:7] - c["truth"][1]).max()))
            assert S[7] == 1.0 and int(w["result"]["n_in"]) == int(w["result"]["n_corr"])
    print(f"recovery: R {worst_R:.3e}, t {worst_t:.3e}")
    assert seen >= 15 and worst_R <= TOL_R and worst_t <= TOL_T, (worst_R, worst_t)


# ---------------------------------------------------------------- the kernel's arithmetic, built for the host
def test_host_build_of_the_kernel_arithmetic_equals_the_referee(refs):
    """sim3_opt_math.h is what the gfx950 kernel runs: the gather, the shared perturbed estimates, the chains with
    removed pairs skipped, the 7x7 LDLT, the LM driver and the checks at the last evaluated estimate.  Built with g++
    (contraction off, as the device build) it must give the referee's result record, match12 and per-trial lambda,
    rho, verdict and Sim3(update) branch bit for bit."""
    points, bad, cases, r = refs
    differs = 0                  # final checks whose estimate is a rejected trial's and is not the accepted one
    for c, w in zip(cases, r):
        res, m, trials, at = C.host_build(c, points, bad)
        assert res.tobytes() == w["result"].tobytes(), (c["name"], res, w["result"])
        assert m.tobytes() == w["match12"].tobytes(), c["name"]
        assert trials.tobytes() == np.ascontiguousarray(w["trials"][:, [0, 3, 4, 5, 6]]).tobytes(), c["name"]
        # the estimate each check evaluates the edges at is the one of the referee's last computeActiveErrors: a
        # rejected trial's where the last trial was rejected.  At convergence the two estimates differ in their last
        # bits only, which no chi2 of the cases carries across th2, so this is where that reading is held
        assert at.tobytes() == w["errors_at"].tobytes(), (c["name"], at, w["errors_at"])
        differs += int(w["flags"][1] == 1 and (w["errors_at"][1] != w["result"]["S12"]).any())
    assert differs >= 2, differs


def test_ldlt_7x7_equals_6x6_on_embedded_systems():
    """A 6x6 system embedded with a unit seventh row and column: the same pivots among the six, the same arithmetic,
    the same bits, wherever the unit pivot falls in the order."""
    L = C.compiled("sim3_opt_host")
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    L.sim3_opt_host_ldlt.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    rng = np.random.default_rng(7)
    tril6, tril7 = np.tril_indices(6), np.tril_indices(7)
    first = last = failed = 0
    for it in range(300):
        A = rng.normal(size=(8, 6)) * 10.0 ** rng.uniform(-2, 2)
        H = A.T @ A * (1.0 if it % 3 else 10.0 ** rng.uniform(-3, 3))
        if it % 50 == 49:
            H = -H                                                       # not positive: both refuse
        if it % 7 == 3:
            H[:, 2] = H[2, :] = 0.0                                      # a zero pivot among the six
        b = rng.normal(size=6)
        H7 = np.zeros((7, 7))
        H7[:6, :6], H7[6, 6] = H, 1.0
        b7 = np.append(b, 0.5)
        x6, x7 = np.full(6, 7.0), np.full(7, 7.0)
        ok6 = L.sim3_opt_host_ldlt(6, p(np.ascontiguousarray(H[tril6])), 0.0, p(b), p(x6))
        ok7 = L.sim3_opt_host_ldlt(7, p(np.ascontiguousarray(H7[tril7])), 0.0, p(b7), p(x7))
        assert ok6 == ok7, it
        failed += not ok6
        if ok6:
            assert x7[:6].tobytes() == x6.tobytes() and x7[6] == 0.5, (it, x6, x7)
            d = np.abs(np.diag(H))
            first += d.max() < 1.0
            last += d.min() > 1.0
        else:
            assert (x6 == 7.0).all() and (x7 == 7.0).all()              # x untouched
    assert first >= 10 and last >= 10 and failed >= 5
