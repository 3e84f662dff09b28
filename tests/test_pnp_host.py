"""CPU checks of the PnPsolver referee (tests/pnp_ref.cpp), its cases (tests/pnp_cases.py) and the host build of the
kernels' arithmetic (sp-slam_amd/csrc/pnp_math.h through tests/pnp_host.cpp):
* every case reaches what it is there for, asserted from the referee's trace;
* the host build, with its parallel-form selection, equals the referee bit for bit on every call of every case;
* the selection rule equals a literal trace of the loop on random sequences;
* the restated OpenCV calls have the properties of an SVD, a least-squares solve and an inverse;
* the noise-free cases recover the true pose and flag exactly the true correspondences;
* the inlier mask is CheckInliers' float expression at the returned pose, and that expression is what GCC makes of
  the reference's lines on an FMA host.
"""
import ctypes
import fractions

import numpy as np
import pytest

import pnp_cases as C

# The restated SVD against its own definition and numpy, over the matrices the referee decomposes in seven of the
# cases (48 of each kind per case: the 12 x 12 MtM, the 3 x 3 PW0tPW0 and ABt), relative to the largest singular value;
# measured here (profiles/r19/pnp.md): orthonormality of U and V 2.78e-15, U^T D V^T against the input 2.65e-15, the
# singular values against numpy.linalg.svd 1.90e-15.  Each bound is four times that, rounded up to a power of two.
TOL_ORTHO, TOL_REBUILD, TOL_D = 2.0 ** -46, 2.0 ** -46, 2.0 ** -46
# cvSolve's restatement against numpy.linalg.lstsq on the full-rank systems, relative to the solution's largest
# entry: 1.83e-13; the inverse against numpy.linalg.inv relative to its largest entry: 3.54e-15.
TOL_SOLVE, TOL_INV = 2.0 ** -40, 2.0 ** -46
# The refined pose of the noise-free cases against the truth (map points rounded to float, 6e-8 relative, and
# keypoints rounded to float, 3e-5 px): R 2.40e-7, t 4.59e-7.
TOL_R, TOL_T = 2.0 ** -19, 2.0 ** -19

NOISE_FREE = ("n11", "n14", "n15", "n63", "n64", "n65", "n255", "n256", "n257", "n300", "reentry_below_max", "coplanar")


@pytest.fixture(scope="module")
def refs():
    points, bad, cases = C.build()
    return points, bad, cases, C.references()


def named(refs):
    _, _, cases, r = refs
    return {c["name"]: (c, w) for c, w in zip(cases, r)}


def statuses(w):
    return [int(r["status"]) for r in w["results"]]


# ---------------------------------------------------------------- what the cases reach
def test_cases_reach_what_they_are_for(refs):
    N = named(refs)
    res = lambda name, r=0: N[name][1]["results"][r]  # noqa: E731
    # the kernels' constants, and N kept around each of them and around the RANSAC bounds
    assert (C.GATHER, C.WAVE, C.LANES) == (256, 64, 64)
    host = C.compiled("pnp_host")
    assert (host.pnp_host_sizes(0), host.pnp_host_sizes(1)) == (32, 104)
    want = {"n0": 0, "n0_frame_empty": 0, "n3": 3, "n4": 4, "n9": 9, "n10": 10, "n11": 11, "n14": 14, "n15": 15, "n300": 300}
    for n in (C.WAVE, C.GATHER):
        want.update({f"n{n - 1}": n - 1, f"n{n}": n, f"n{n + 1}": n + 1})
    for name, n in want.items():
        c, w = N[name]
        assert int(res(name)["n"]) == n == len(c["kept"]), name
    assert len(N["n257"][0]["kun"]) > C.GATHER and len(N["n0_frame_empty"][0]["kun"]) == 0
    # the constructor's drops: a keyframe keypoint without a row, a bad row, matches of -1; every octave
    points, bad = refs[0], refs[1]
    for name in ("n15", "n64", "n300"):
        c = N[name][0]
        matched = np.flatnonzero(c["match"] >= 0)
        dropped = sorted(set(matched.tolist()) - set(c["kept"].tolist()))
        rows = c["kf_rows"][c["match"][dropped]]
        assert len(dropped) == 2 and (rows < 0).sum() == 1 and bad[rows[rows >= 0]].all(), name
        assert (c["match"] < 0).any()
        assert sorted(set(c["kun"]["octave"][c["kept"]].tolist())) == list(range(8)), name
    # mRansacMaxIts 1 (N == min), 14, 35 and the parameter set that crosses every wave of the hypothesis kernel
    assert [int(res(n)["max_its"]) for n in ("n10", "n4", "n15", "n63", "long_all_wrong")] == [1, 1, 14, 35, 300]
    assert [int(res(n)["min_inliers"]) for n in ("n4", "n10", "n15", "n63", "n300")] == [4, 10, 10, 31, 150]
    assert int(res("long_all_wrong")["iterations_done"]) == 300 > 4 * C.LANES
    for at in (63, 64, 70, 128, 299):
        r = res(f"long_first_at_{at}")
        assert (int(r["status"]), int(r["iteration"]), int(r["iterations_done"])) == (C.REFINED, at, at + 1)
    # the first call runs to mRansacMaxIts, not to nIterations: || in the loop condition; N == min runs nIterations
    assert int(res("all_wrong")["iterations_done"]) == 35 and N["all_wrong"][0]["calls"][0] == 5
    assert int(res("n10")["iterations_done"]) == 5 and int(res("n4")["iterations_done"]) == 5
    # outcomes
    assert statuses(N["n11"][1]) == [C.REFINED] and int(res("n11")["iteration"]) == 0          # at the first iteration
    for name in ("n0", "n3", "n9"):                                                               # N < min, at once
        assert (statuses(N[name][1]), int(res(name)["iterations_done"]), len(N[name][1]["trace"])) == ([C.NO_MORE], 0, 0)
    assert statuses(N["all_wrong"][1]) == [C.NO_MORE] * 3 and int(res("all_wrong", 2)["best_inliers"]) == 0
    assert [int(res("all_wrong", r)["iterations_done"]) for r in range(3)] == [35, 75, 80]      # exactly n_iterations more
    assert statuses(N["out_of_draws"][1]) == [C.OUT_OF_DRAWS] * 3
    assert [int(res("out_of_draws", r)["iterations_done"]) for r in range(3)] == [12, 12, 12]
    assert statuses(N["n10"][1]) == [C.BEST_NO_MORE] * 2 and statuses(N["n4"][1]) == [C.BEST_NO_MORE]
    # n == min enters Refine and cannot succeed when N == min; the test in Refine is strict
    tr = N["n10"][1]["trace"]
    assert ((tr["n"] == 10) & (tr["refine_ran"] == 1) & (tr["refine_n"] == 10)).any()
    assert int(res("n10")["n_inliers"]) == 10 == int(res("n10")["best_inliers"])
    # a failed Refine, the loop goes on, a later record setter succeeds
    for name, fail_at, at in (("fail_then_refined", 7, 23), ("fail_then_refined_next", 1, 2)):
        c, w = N[name]
        tr, mn = w["trace"], int(w["results"][0]["min_inliers"])
        k = {int(t["k"]): t for t in tr}
        assert k[fail_at]["replaced"] == 1 and k[fail_at]["refine_ran"] == 1 and k[fail_at]["refine_n"] <= mn, name
        assert k[at]["replaced"] == 1 and k[at]["refine_n"] > mn and statuses(w) == [C.REFINED], name
        assert int(w["results"][0]["iteration"]) == at and len(tr) == at + 1
    # the carried mask: calls 2 .. 4 start with the best of iteration 4, whose Refine fails again at 46, 47 and 50
    # (no record setters: each has n == best == min), until 51 sets a new best
    c, w = N["carried_mask_governs"]
    tr, mn = w["trace"], 10
    k = {int(t["k"]): t for t in tr}
    assert statuses(w) == [C.BEST_NO_MORE] * 3 + [C.REFINED] and int(w["results"][3]["iteration"]) == 51
    assert [int(r["iterations_done"]) for r in w["results"]] == [14, 19, 24, 52]
    assert tr["k"][tr["replaced"] == 1].tolist() == [4, 51]
    for q in (11, 46, 47, 50):
        assert k[q]["refine_ran"] == 1 and k[q]["replaced"] == 0 and k[q]["refine_n"] <= mn and mn <= k[q]["n"] <= k[4]["n"]
    assert all(k[q]["n"] == k[4]["n"] == mn for q in (11, 46, 47, 50))     # n == best (no replacement) and n == min (enters)
    assert w["best_mask"][0].tobytes() == w["best_mask"][2].tobytes() != w["best_mask"][3].tobytes()
    # re-entries with made draws: REFINED at done == max; past it on n == best (not replaced: the carried mask);
    # exactly 5 more; n == min enters and does not replace
    c, w = N["reentry"]
    k = {int(t["k"]): t for t in w["trace"]}
    assert statuses(w) == [C.REFINED, C.REFINED, C.BEST_NO_MORE, C.REFINED]
    assert [int(r["iterations_done"]) for r in w["results"]] == [14, 17, 22, 23] and int(w["results"][0]["max_its"]) == 14
    assert (k[13]["n"], k[13]["replaced"]) == (11, 1) and (k[16]["n"], k[16]["replaced"], k[16]["refine_ran"]) == (11, 0, 1)
    assert (k[22]["n"], k[22]["replaced"], k[22]["refine_ran"]) == (10, 0, 1) and k[22]["refine_n"] == 11
    assert all(k[q]["n"] < 10 and k[q]["refine_ran"] == 0 for q in k if q not in (13, 16, 22))
    assert statuses(N["reentry_below_max"][1]) == [C.REFINED] * 3
    assert [int(r["iterations_done"]) for r in N["reentry_below_max"][1]["results"]] == [1, 3, 5]      # all below 14
    # all three approximations are chosen somewhere; the sign flip and det < 0 happen; qr_solve's singular return
    which = set()
    for c, w in N.values():
        which |= set(w["trace"]["which"].tolist())
    assert which == {1, 2, 3}
    assert all(int(N[n][1]["counters"][0]) > 0 and int(N[n][1]["counters"][1]) > 0 for n in ("n15", "behind", "coplanar"))
    tr = N["coincident"][1]["trace"]
    assert tr["idx"][0].tolist() == [0, 1, 2, 3] and tr["singular"][0] != 0
    # four coincident points: NaN throughout, 0 inliers, and the selection goes on to a refined pose
    assert np.isnan(tr["Rt"][0]).all() and tr["n"][0] == 0 and tr["refine_ran"][0] == 0
    assert tr["idx"][1].tolist() == [0, 1, 5, 6] and statuses(N["coincident"][1])[0] == C.REFINED
    # coplanar map points: the third control axis is near 0
    c = N["coplanar"][0]
    Xw = refs[0]["xw"][c["kf_rows"][c["match"][c["kept"]]]].astype(np.float64)
    assert np.linalg.svd(Xw - Xw.mean(0), compute_uv=False)[2] < 1e-6
    # Zc = 0 under the truth: that point is no inlier of the refined pose, every other is
    c, w = N["zc_zero"]
    assert statuses(w) == [C.REFINED] and w["inliers"][0][c["kept"]].tolist() == [1] * 5 + [0] + [1] * 8
    # Refine fails on masks with points behind the camera: BEST_NO_MORE with the best mask
    c, w = N["behind"]
    assert statuses(w) == [C.BEST_NO_MORE] * 3 and w["inliers"][2].tobytes() == \
        np.isin(np.arange(len(c["kun"])), c["kept"][w["best_mask"][2][:len(c["kept"])] != 0]).astype(np.uint8).tobytes()


# ---------------------------------------------------------------- one copy of the arithmetic
def run_host(c, points, bad):
    out, prev, mask = [], None, np.zeros(max(len(c["kun"]), 1), np.uint8)
    for r in range(len(c["calls"])):
        q = C.problem_record(c, r, prev, mask)
        got = C.host_call(c, points, bad, q, mask)
        out.append(got)
        prev, mask = got[0], got[2]
    return out


def test_host_build_of_the_kernel_arithmetic_equals_the_referee(refs):
    """Every result record, inlier byte, best-mask byte and frame point of every call, the state fed from call to
    call; the hypotheses' counts and chosen solutions against the trace."""
    points, bad, cases, want = refs
    n_refines = 0
    for c, w in zip(cases, want):
        j = 0
        for r, (res, inl, bm, fp, hyp, nref, sing) in enumerate(run_host(c, points, bad)):
            assert res.tobytes() == w["results"][r].tobytes(), (c["name"], r, res, w["results"][r])
            assert inl.tobytes() == w["inliers"][r].tobytes() and bm.tobytes() == w["best_mask"][r].tobytes(), (c["name"], r)
            pose = int(res["status"]) in (C.REFINED, C.BEST_NO_MORE)
            assert (fp is not None) == pose and (fp is None or fp.tobytes() == w["frame_points"][r].tobytes()), (c["name"], r)
            before = int(w["results"][r - 1]["iterations_done"]) if r else 0
            ran = int(res["iterations_done"]) - before
            tr = w["trace"][j:j + ran]                                  # the referee stops where the loop returns
            assert hyp[:ran, 0].tolist() == tr["n"].tolist() and hyp[:ran, 1].tolist() == tr["which"].tolist(), (c["name"], r)
            j += ran
            n_refines += nref
        assert j == len(w["trace"]), c["name"]
    assert n_refines > 40


def test_the_draws_without_the_array_are_the_swap_with_back_draws():
    host = C.compiled("pnp_host")
    host.pnp_host_draw4.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    rng = np.random.default_rng(5)
    for n in (4, 5, 6, 7, 30):
        for _ in range(400):
            pos = [int(rng.integers(0, n - d)) for d in range(4)]
            if rng.random() < 0.5:
                pos = [min(p, n - d - 1) if rng.random() < 0.5 else n - d - 1 for d, p in enumerate(pos)]   # the backs
            avail, want = list(range(n)), []
            for p in pos:
                want.append(avail[p])
                avail[p] = avail[-1]
                avail.pop()
            r = np.array([C.rand_for(p, n - d) for d, p in enumerate(pos)], np.int32)
            got = np.zeros(4, np.int32)
            host.pnp_host_draw4(r.ctypes.data, C.RAND_MAX, n, got.ctypes.data)
            assert got.tolist() == want, (n, pos)


# ---------------------------------------------------------------- the selection rule
def literal_loop(n, refine_n, min_inliers, best_in, carried_refine_n):
    """iterate's loop on made-up counts: mask is the index of the hypothesis that set the best, -1 the carried one."""
    best, mask, refines = best_in, -1, 0
    for j, nj in enumerate(n):
        if nj >= min_inliers:
            if nj > best:
                best, mask = nj, j
            refines += 1
            if (carried_refine_n if mask < 0 else refine_n[mask]) > min_inliers:
                return j, best, mask, refines
    return -1, best, mask, refines


def test_selection_equals_the_literal_loop_on_random_sequences():
    host = C.compiled("pnp_host")
    host.pnp_host_select.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    rng = np.random.default_rng(11)
    outcomes, carried_governs, many = set(), 0, 0
    for trial in range(4000):
        n_run = int(rng.integers(0, 200))
        mn = int(rng.integers(4, 12))
        hi = int(rng.integers(mn - 2, mn + 12))
        n = rng.integers(0, max(hi, 1) + 1, n_run).astype(np.int32)
        if trial % 7 == 0:
            n = np.sort(rng.integers(0, 400, n_run)).astype(np.int32)   # many record setters: more than a round of 64
        p_ok = rng.choice([0.0, 0.1, 0.5]) if trial % 14 else 0.0
        refine_n = np.where(rng.random(n_run) < p_ok, mn + 1 + rng.integers(0, 3, n_run), mn - rng.integers(0, 3, n_run)).astype(np.int32)
        refine_n = np.where(rng.random(n_run) < 0.2, mn, refine_n).astype(np.int32)          # == min fails
        best_in = int(rng.choice([0, 0, mn - 1, mn, mn + 3, hi]))
        carried = int(rng.choice([mn - 1, mn, mn + 1]))
        want = literal_loop(n.tolist(), refine_n.tolist(), mn, best_in, carried)
        b, s, cnt = (np.zeros(1, np.int32) for _ in range(3))
        ret = host.pnp_host_select(n.ctypes.data, refine_n.ctypes.data, n_run, mn, best_in, carried, b.ctypes.data,
                                   s.ctypes.data, cnt.ctypes.data)
        assert (ret, int(b[0]), int(s[0])) == want[:3], (trial, n.tolist(), refine_n.tolist(), mn, best_in, carried)
        outcomes.add((ret >= 0, want[2] < 0))
        carried_governs += ret >= 0 and want[2] < 0
        many += int(cnt[0]) > 64
    assert outcomes == {(True, True), (True, False), (False, True), (False, False)} and carried_governs > 50 and many > 5


# ---------------------------------------------------------------- the readings, whatever the implementation
def captured(cases_wanted=("n15", "n64", "coplanar", "coplanar_noisy", "carried_mask_governs", "behind", "n300")):
    """The inputs the restated OpenCV calls got while the referee ran a few cases."""
    points, bad, cases = C.build()
    lib = C.compiled("pnp_ref")
    out = {}
    take = [c for c in cases if c["name"] in cases_wanted]
    lib.pnp_ref_captured.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    for kind in range(4):
        out[kind] = []
    for c in take:
        C.reference(c, points, bad, capture=True)
        for kind in range(4):
            n = lib.pnp_ref_captured(kind, None, 0)
            buf = np.zeros(max(n, 1))
            lib.pnp_ref_captured(kind, buf.ctypes.data, n)
            out[kind].append(buf[:n].copy())
    lib.pnp_ref_capture(0)
    return out


def svd_deviations(lib_name, fn):
    cap = captured()
    lib = C.compiled(lib_name)
    dev = {"ortho": 0.0, "rebuild": 0.0, "d": 0.0, "n": 0}
    for kind, n in ((0, 12), (1, 3)):
        for buf in cap[kind]:
            for A in buf.reshape(-1, n, n):
                w, ut, vt = np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
                getattr(lib, fn).argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3
                getattr(lib, fn)(A.ctypes.data, n, w.ctypes.data, ut.ctypes.data, vt.ctypes.data)
                s = np.linalg.svd(A, compute_uv=False)
                scale = max(s[0], 1e-300)
                assert (np.diff(w) <= 0).all()
                dev["ortho"] = max(dev["ortho"], np.abs(ut @ ut.T - np.eye(n)).max(), np.abs(vt @ vt.T - np.eye(n)).max())
                dev["rebuild"] = max(dev["rebuild"], np.abs(ut.T @ np.diag(w) @ vt - A).max() / scale)   # A = U D V^T
                dev["d"] = max(dev["d"], np.abs(w - s).max() / scale)
                dev["n"] += 1
    return dev


def solve_deviations(lib_name, fn_solve, fn_inv):
    cap = captured()
    lib = C.compiled(lib_name)
    dev = {"solve": 0.0, "inv": 0.0, "n": 0}
    for buf in cap[2]:
        i = 0
        while i < len(buf):
            K = int(buf[i])
            L, b = buf[i + 1:i + 1 + 6 * K].reshape(6, K).copy(), buf[i + 1 + 6 * K:i + 7 + 6 * K].copy()
            i += 7 + 6 * K
            x = np.zeros(K)
            getattr(lib, fn_solve).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
            getattr(lib, fn_solve)(L.ctypes.data, K, b.ctypes.data, x.ctypes.data)
            s = np.linalg.svd(L, compute_uv=False)
            if not np.isfinite(L).all() or s[-1] <= 1e-10 * s[0]:
                continue                                                # rank-deficient: the thresholds differ by design
            want = np.linalg.lstsq(L, b, rcond=None)[0]
            dev["solve"] = max(dev["solve"], np.abs(x - want).max() / max(np.abs(want).max(), 1e-300))
            dev["n"] += 1
    for buf in cap[3]:
        for A in buf.reshape(-1, 3, 3):
            s = np.linalg.svd(A, compute_uv=False)
            if s[-1] <= 1e-10 * s[0]:
                continue                                                # coplanar: cvInvert gives the pseudo-inverse
            inv = np.zeros((3, 3))
            getattr(lib, fn_inv).argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            getattr(lib, fn_inv)(A.copy().ctypes.data, inv.ctypes.data)
            want = np.linalg.inv(A)
            dev["inv"] = max(dev["inv"], np.abs(inv - want).max() / np.abs(want).max())
            dev["n"] += 1
    return dev


@pytest.mark.parametrize("lib_name,fn", [("pnp_ref", "pnp_ref_svd"), ("pnp_host", "pnp_host_svd")])
def test_restated_svd_is_an_svd(lib_name, fn):
    dev = svd_deviations(lib_name, fn)
    print("svd deviations", lib_name, dev)
    assert dev["n"] > 300
    assert dev["ortho"] <= TOL_ORTHO and dev["rebuild"] <= TOL_REBUILD and dev["d"] <= TOL_D, dev


@pytest.mark.parametrize("lib_name,fn_solve,fn_inv", [("pnp_ref", "pnp_ref_solve", "pnp_ref_invert3"),
                                                      ("pnp_host", "pnp_host_solve", "pnp_host_invert3")])
def test_restated_solve_and_inverse_agree_with_numpy(lib_name, fn_solve, fn_inv):
    dev = solve_deviations(lib_name, fn_solve, fn_inv)
    print("solve deviations", lib_name, dev)
    assert dev["n"] > 300
    assert dev["solve"] <= TOL_SOLVE and dev["inv"] <= TOL_INV, dev


# ---------------------------------------------------------------- the truth
def pose_deviations(refs):
    N = named(refs)
    dev = {"R": 0.0, "t": 0.0, "n": 0}
    for name in NOISE_FREE:
        c, w = N[name]
        for r, res in enumerate(w["results"]):
            if int(res["status"]) != C.REFINED:
                continue
            T = res["Tcw"].reshape(4, 4).astype(np.float64)
            dev["R"] = max(dev["R"], np.abs(T[:3, :3] - c["Tcw"][:3, :3]).max())
            dev["t"] = max(dev["t"], np.abs(T[:3, 3] - c["Tcw"][:3, 3]).max())
            dev["n"] += 1
            true = c["kept"][np.array(list(c["kinds"])) == "t"]
            want = np.zeros(len(c["kun"]), np.uint8)
            want[true] = 1
            assert w["inliers"][r].tobytes() == want.tobytes(), (name, r)   # every true one, no planted one
            assert int(res["n_inliers"]) == len(true)
    return dev


def test_noise_free_cases_recover_the_pose_and_flag_exactly_the_true_correspondences(refs):
    dev = pose_deviations(refs)
    print("pose deviations", dev)
    assert dev["n"] >= len(NOISE_FREE)
    assert dev["R"] <= TOL_R and dev["t"] <= TOL_T, dev
    # the planted ones are at least 20 px from their reprojection
    N = named(refs)
    for name in NOISE_FREE:
        c = N[name][0]
        wrong = c["kept"][np.array(list(c["kinds"])) == "w"]
        if len(wrong):
            Xw = refs[0]["xw"][c["kf_rows"][c["match"][wrong]]].astype(np.float64)
            d = np.linalg.norm(C.project(c["Tcw"], Xw) - np.stack([c["kun"]["x"][wrong], c["kun"]["y"][wrong]], 1), axis=1)
            assert d.min() >= 20.0, name


# ---------------------------------------------------------------- the mask
def fma(a, b, c):
    return float(fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c))   # one rounding, to nearest even


def f32(x):
    return float(np.float32(x))


def error2(xw, uv, Rt, cam):
    """CheckInliers' expression with its contractions, in exact arithmetic rounded where the C++ rounds."""
    x, y, z = (float(v) for v in xw)
    cam = [float(v) for v in cam]
    Xc = f32(fma(Rt[2], z, fma(Rt[1], y, Rt[0] * x)) + Rt[9])
    Yc = f32(fma(Rt[5], z, fma(Rt[4], y, Rt[3] * x)) + Rt[10])
    den = fma(Rt[8], z, fma(Rt[7], y, Rt[6] * x)) + Rt[11]
    if den == 0.0:
        return float("inf")
    invZc = f32(1.0 / den)
    ue, ve = fma(cam[0] * Xc, invZc, cam[2]), fma(cam[1] * Yc, invZc, cam[3])
    dx, dy = f32(float(uv[0]) - ue), f32(float(uv[1]) - ve)
    dy2 = f32(dy * dy)
    exact = fractions.Fraction(dx) * fractions.Fraction(dx) + fractions.Fraction(dy2)
    lo = np.float32(float(exact))                                        # float(exact) is within half a double ulp
    best = min((np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))),
               key=lambda c: (abs(fractions.Fraction(float(c)) - exact), int(np.float32(c).view(np.uint32)) & 1))
    return float(best)


def test_inlier_mask_is_check_inliers_at_the_returned_pose(refs):
    """From the trace's double pose, before the convertTo: the refined pose's mask for REFINED, the best
    hypothesis' for BEST_NO_MORE."""
    points, bad, cases, want = refs
    N = named(refs)
    checked = 0
    for name in ("n15", "n64", "fail_then_refined", "carried_mask_governs", "zc_zero", "behind", "coincident", "reentry"):
        c, w = N[name]
        rows = c["kf_rows"][c["match"][c["kept"]]]
        bound = (C.sigma2()[c["kun"]["octave"][c["kept"]]] * np.float32(C.TH2)).astype(np.float32)
        k = {int(t["k"]): t for t in w["trace"]}
        for r, res in enumerate(w["results"]):
            st = int(res["status"])
            if st == C.REFINED:
                Rt = k[int(res["iteration"])]["refine_Rt"]
            elif st == C.BEST_NO_MORE:
                setters = [t for t in w["trace"] if t["replaced"] == 1 and t["k"] < int(res["iterations_done"])]
                Rt = setters[-1]["Rt"]
            else:
                continue
            mask = np.zeros(len(c["kun"]), np.uint8)
            for i, f in enumerate(c["kept"]):
                e = error2(points["xw"][rows[i]], (c["kun"]["x"][f], c["kun"]["y"][f]), [float(v) for v in Rt], C.camera())
                mask[f] = 1 if e < float(bound[i]) else 0
            assert mask.tobytes() == w["inliers"][r].tobytes(), (name, r)
            assert int(mask.sum()) == int(res["n_inliers"])
            checked += 1
    assert checked >= 12


def test_check_inliers_contractions_are_what_gcc_makes_on_an_fma_host():
    """The reference builds with -O3 -march=native: tests/pnp_probe.cpp states the inlier test's error on the
    reference's types and association; the compiler contracts it, pnp_math.h writes the same contractions out."""
    probe = C.compiled("pnp_probe", ("-O3", "-march=x86-64-v3", "-ffp-contract=fast"))
    host = C.compiled("pnp_host")
    host.pnp_host_error2.restype = ctypes.c_float
    host.pnp_host_error2.argtypes = [ctypes.c_void_p] * 4
    probe.pnp_probe_error2.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5
    rng = np.random.default_rng(1)
    n = 4000
    xw, uv = rng.uniform(-3, 3, (n, 3)).astype(np.float32), rng.uniform(0, 640, (n, 2)).astype(np.float32)
    Rt = np.concatenate([C.rotation((1, 2, 3), 0.3).reshape(9), [0.1, -0.2, 3.3]])
    cam, out = C.camera(), np.zeros(n, np.float32)
    probe.pnp_probe_error2(n, xw.ctypes.data, uv.ctypes.data, Rt.ctypes.data, cam.ctypes.data, out.ctypes.data)
    got = np.array([host.pnp_host_error2(xw[i].ctypes.data, uv[i].ctypes.data, Rt.ctypes.data, cam.ctypes.data)
                    for i in range(n)], np.float32)
    assert got.tobytes() == out.tobytes()
    mine = np.array([error2(xw[i], uv[i], Rt.tolist(), cam) for i in range(200)], np.float32)
    assert mine.tobytes() == out[:200].tobytes()
