"""CPU checks of the Sim3Solver referee (tests/sim3_solver_ref.py) and its cases (tests/sim3_solver_cases.py):
* the sequential loop with its early return agrees with the reformulated selection the kernels use;
* exact rigid and similarity motions are recovered, and the referee agrees with a float64 Horn solution;
* every case reaches what it is there for;
* the restated scalar expressions equal what g++ -O3 -march=native makes of the same arithmetic;
* the kernels' arithmetic (sp-slam_amd/csrc/sim3_math.h), built for the host, equals the referee bit for bit.
"""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import fuse_ref as FR
import sim3_solver_cases as C
import sim3_solver_ref as SR
from matcher_ref import f32 as _f

ROOT = pathlib.Path(__file__).resolve().parents[1]

# Agreement with float64 Horn (numpy.linalg.eigh): the referee's largest deviation over the cases' non-degenerate
# hypotheses, measured here (profiles/r16/sim3_solver.md): R 5.49e-6, t 7.32e-6, s 6.70e-8; the bounds are four times
# that, rounded up to a power of two.
TOL_R, TOL_T, TOL_S = 2.0 ** -15, 2.0 ** -15, 2.0 ** -21
MIN_SHAPE = 0.01       # a triple is degenerate when its triangle's area is below MIN_SHAPE * (longest edge)^2,
MIN_EXTENT = 2.0 ** -63  # or its longest edge is below 2^-63: the squares of such lengths leave float's normal range
MAX_EXCLUDED = 0.10


@pytest.fixture(scope="module")
def refs():
    points, bad, cases = C.build()
    return points, bad, cases, C.references()


def by_name(refs):
    _, _, cases, r = refs
    return {c["name"]: (c, calls, s) for c, (calls, s) in zip(cases, r)}


# ---------------------------------------------------------------- the selection rule
def test_sequential_loop_agrees_with_the_reformulated_selection(refs):
    """Per call: the first k of the call with n_k > min_inliers && n_k >= best_in is where the referee returned,
    no iteration qualifies where it did not, and best_out = max(best_in, n_j over the iterations run)."""
    _, _, cases, r = refs
    found = 0
    for c, (calls, s) in zip(cases, r):
        counts = list(s.trace["counts"])
        done, best = c["state"] if c["state"] is not None else (0, 0)
        for (rec, _, _), n_it in zip(calls, c["calls"]):
            ran = int(rec["iterations_done"]) - done
            assert 0 <= ran <= n_it, c["name"]
            mine, counts = counts[:ran], counts[ran:]
            qualifies = [n > c["min_inliers"] and n >= best for n in mine]
            if int(rec["status"]) == SR.FOUND:
                found += 1
                assert qualifies.index(True) == ran - 1 and int(rec["n_inliers"]) == mine[-1], c["name"]
            else:
                assert not any(qualifies), c["name"]
                want_run = 0 if s.N < c["min_inliers"] else max(min(s.mRansacMaxIts - done, n_it), 0)
                assert ran == want_run, c["name"]
                no_more = s.N < c["min_inliers"] or done + ran >= s.mRansacMaxIts
                assert int(rec["status"]) == (SR.NO_MORE if no_more else SR.NOT_YET), c["name"]
            assert int(rec["best_inliers"]) == max([best] + mine), c["name"]
            done, best = int(rec["iterations_done"]), int(rec["best_inliers"])
        assert not counts
    assert found >= 15


# ---------------------------------------------------------------- what the cases reach
def test_cases_reach_what_they_are_for(refs):
    R = by_name(refs)
    status = lambda name: [int(rec["status"]) for rec, _, _ in R[name][1]]  # noqa: E731
    done = lambda name: [int(rec["iterations_done"]) for rec, _, _ in R[name][1]]  # noqa: E731
    assert R["n_below_min"][2].N == 5 and status("n_below_min") == [SR.NO_MORE] and done("n_below_min") == [0]
    assert R["n_equals_min"][2].N == 6 and done("n_equals_min") == [1, 1] and status("n_equals_min") == [SR.NO_MORE] * 2
    assert R["n3_min3"][2].N == 3 and done("n3_min3") == [1]
    assert R["n4_min3_scale"][2].N == 4 and status("n4_min3_scale") == [SR.FOUND]
    for n in (63, 64, 65):
        c, calls, s = R[f"n{n}_of_300"]
        assert s.N == n and len(c["match12"]) == 300 and max(s.mvnIndices1) >= 256 and status(f"n{n}_of_300") == [SR.FOUND]
    assert R["n_cap_300"][2].N == 300 and status("n_cap_300") == [SR.FOUND]
    assert R["kf1_one_keypoint"][2].mN1 == 1 and R["kf1_no_match"][2].N == 0
    c, calls, s = R["gather_bad_and_missing"]
    assert s.N == int((c["match12"] >= 0).sum()) - 4                   # two bad points, two missing rows
    assert sorted({int(c["kf1"]["kun"]["octave"][i]) for i in s.mvnIndices1}) == list(range(8))
    assert len(set(s.mvnMaxError1)) >= 6 and min(s.mvnMaxError1) == 9   # (size_t)(9.210 * 1.0f)
    for name, at in (("first_at_0", 0), ("first_at_63", 63), ("first_at_64", 64), ("first_at_63_in_300", 63),
                     ("first_at_last", 299), ("one_call_of_all", 22)):
        assert status(name) == [SR.FOUND] and done(name) == [at + 1], name
        assert R[name][2].mRansacMaxIts == 300
    assert status("never") == [SR.NO_MORE, SR.NO_MORE] and done("never") == [300, 300]
    assert status("calls_of_5") == [SR.NOT_YET] * 4 + [SR.FOUND] and done("calls_of_5")[-1] == 23
    a, b = R["calls_of_5"][1][-1], R["one_call_of_all"][1][-1]
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()   # continued = at once
    assert status("scale_free_at_7") == [SR.NOT_YET, SR.FOUND]
    assert status("best_in_above") == [SR.NOT_YET] and int(R["best_in_above"][1][0][0]["best_inliers"]) == 9
    assert status("best_in_equal") == [SR.FOUND] and int(R["best_in_equal"][1][0][0]["n_inliers"]) == 8
    assert R["short_of_max"][2].mRansacMaxIts == 9
    assert status("short_of_max") == [SR.NOT_YET] * 2 and done("short_of_max") == [3, 6]
    assert status("equal_to_max") == [SR.NOT_YET, SR.NO_MORE, SR.NO_MORE] and done("equal_to_max") == [4, 9, 9]
    assert status("past_max") == [SR.NOT_YET, SR.NO_MORE] and done("past_max") == [5, 9]
    # the draws: value 0, RAND_MAX, and positions that hold a swapped-in last element
    s = R["draw_edges"][2]
    triples = [h[1] for h in s.trace["hyps"]]
    assert triples[0] == [0, 11, 10] and triples[1] == [11, 10, 9] and triples[2] == [3, 11, 10], triples
    assert triples[3][0] == 10 and triples[4] == [5, 10, 11], triples
    # the seam: errors of 8.9 and 9.1 .. 9.2 against the bound 9, not 9.21
    c, calls, s = R["bound_seam"]
    assert status("bound_seam") == [SR.FOUND] and s.mvnMaxError1 == [9] * 12
    e10, e11 = float(s.errs[10][0]), float(s.errs[11][0])
    assert 8.8 < e10 < 9.0 and 9.0 < e11 < 9.21, (e10, e11)
    assert calls[0][1].tolist() == [1] * 11 + [0] and int(calls[0][0]["n_inliers"]) == 11
    assert max(float(e[1]) for e in s.errs[10:]) < 9.0                 # err1 alone decides
    # no motion at all: norm(vec) = 0 and the reference's own 0/0
    s = R["identity_motion_is_nan"][2]
    assert np.isnan(s.trace["hyps"][0][3]).all() and s.trace["counts"][0] == 0
    # degenerate triples: NaN or not, nothing faults and NaN errors are no inliers
    for name in ("degenerate_fixed", "degenerate_scale_free"):
        s = R[name][2]
        hy = s.trace["hyps"]
        assert [h[1] for h in hy[:5]] == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 0, 4], [7, 9, 2]]
        assert np.isnan(hy[1][3]).all() and s.trace["counts"][1] == 0   # coincident: M = 0, norm(vec) = 0
        assert not np.isfinite(s.mvP1im1[9][0]) and s.mvX3Dc2[9][2] < 0  # z = 0, z < 0
    hy = R["degenerate_scale_free"][2].trace["hyps"][2]               # den = 0 under a finite R: s12 = nom / 0
    assert R["degenerate_scale_free"][2].trace["den"][2] == 0.0 and np.isfinite(hy[3]).all() and np.isinf(hy[2])
    assert R["degenerate_fixed"][2].trace["hyps"][2][2] == 1.0
    # fixed scale: s12 is exactly 1.0f; scale free recovers 1.3
    for rec, _, _ in R["loop_fixed"][1]:
        assert int(rec["status"]) == SR.FOUND and rec["s12"].tobytes() == _f(1.0).tobytes()
    assert all(abs(float(rec["s12"]) - 1.3) < 0.01 for rec, _, _ in R["loop_scale_free"][1])
    assert status("loop_fixed_on_scaled") == [SR.NOT_YET] * 3
    assert R["loop_fixed"][2].mRansacMaxIts == 30                       # N = 38 at ComputeSim3's 0.99, 20, 300


def test_chain_case_is_found_and_feeds_search_by_sim3():
    import loop_match_ref as LR
    points, bad, kf1, kf2, match12, rand, geo = C.chain_case()
    assert np.array_equal(geo, C.geo())
    s = SR.Sim3Solver(kf1, kf2, points, bad, match12, geo, True, rand)
    s.set_ransac_parameters(0.99, 20, 300)
    T12, no_more, inl, n = s.iterate(5)
    assert T12 is not None and n > 20 and s.N >= 40
    m_in = SR.filtered_match12(match12, inl)
    m, found = LR.search_by_sim3(kf1, kf2, points, bad, s.mBestScale, s.mBestRotation, s.mBestTranslation, m_in, geo)
    assert found > 0 and int((m >= 0).sum()) == n + found


# ---------------------------------------------------------------- rigid motions and float64 Horn
def test_exact_motions_are_recovered():
    rng = np.random.default_rng(3)
    for it in range(40):
        s = 1.0 if it % 2 else float(rng.uniform(0.5, 2.0))
        Rt = C.rotation(rng.normal(size=3), float(rng.uniform(0.05, 3.0)))
        t = rng.uniform(-1, 1, 3)
        X2 = rng.uniform(-1, 1, (3, 3)) + np.array([[0.0], [0.0], [3.0]])
        X1 = s * Rt @ X2 + t[:, None]
        got_s, R, tt, T12, T21 = SR.compute_sim3(X1.astype(np.float32), X2.astype(np.float32), it % 2 == 1)
        assert abs(float(got_s) - s) < 1e-4 and np.abs(R - Rt).max() < 1e-4 and np.abs(tt - t).max() < 1e-3, it
        assert np.abs(T12.astype(np.float64) @ T21.astype(np.float64) - np.eye(4)).max() < 1e-4


def horn64(P1, P2, fix_scale):
    P1, P2 = P1.astype(np.float64), P2.astype(np.float64)
    O1, O2 = P1.mean(1, keepdims=True), P2.mean(1, keepdims=True)
    A, B = P1 - O1, P2 - O2
    M = B @ A.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    a, b, c, d = np.linalg.eigh(N)[1][:, -1]
    R = np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                  [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                  [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])
    P3 = R @ B
    s = 1.0 if fix_scale else (A * P3).sum() / (P3 * P3).sum()
    return s, R, (O1 - s * R @ O2).ravel()


def triangle_shape(P):
    a, b, c = (P[:, i].astype(np.float64) for i in range(3))
    if not np.isfinite(P).all():
        return 0.0
    ext = max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b))
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a)) / ext ** 2 if ext >= MIN_EXTENT else 0.0


def test_referee_agrees_with_float64_horn(refs):
    """Over every hypothesis the cases evaluate, except degenerate triples (on either side: triangle area below
    MIN_SHAPE of the squared longest edge, or a longest edge below MIN_EXTENT, or a point that is not finite) and
    triples identical on both sides (no motion: the reference's 0/0)."""
    _, _, cases, r = refs
    total, excluded, worst = 0, 0, [0.0, 0.0, 0.0]
    for c, (calls, s) in zip(cases, r):
        for (k, triple, sc, R, t, T12, T21, flags) in s.trace["hyps"]:
            P1 = np.array([s.mvX3Dc1[i] for i in triple], np.float32).T
            P2 = np.array([s.mvX3Dc2[i] for i in triple], np.float32).T
            total += 1
            if min(triangle_shape(P1), triangle_shape(P2)) <= MIN_SHAPE or P1.tobytes() == P2.tobytes():
                excluded += 1
                continue
            s64, R64, t64 = horn64(P1, P2, c["fix_scale"])
            d = (np.abs(R - R64).max(), np.abs(t - t64).max(), abs(float(sc) - s64))
            worst = [max(a, b) for a, b in zip(worst, d)]
            assert d[0] <= TOL_R and d[1] <= TOL_T and d[2] <= TOL_S, (c["name"], k, d)
    print(f"float64 Horn: {total} hypotheses, {excluded} excluded, worst dR {worst[0]:.3g} dt {worst[1]:.3g} "
          f"ds {worst[2]:.3g}")
    assert total > 900 and excluded / total <= MAX_EXCLUDED, (excluded, total)


# ---------------------------------------------------------------- the iteration table, the round robin
def test_ransac_table_helper_equals_a_direct_evaluation():
    import spslam_gpu
    import spslam_loop as L
    lib = spslam_gpu.load_library()
    L._bind(lib)
    for prob, mn, mx, cap in ((0.99, 20, 300, 2000), (0.99, 6, 300, 300), (0.99, 3, 300, 64), (0.5, 20, 40, 100),
                              (0.999, 20, 4096, 8192)):
        table = np.full(cap + 2, -7, np.int32)
        assert lib.spslam_sim3_ransac_table(prob, mn, mx, cap, table.ctypes.data) == 0
        assert table[cap + 1] == -7 and not table[:mn].any()
        want = [SR.ransac_max_its(n, prob, mn, mx) for n in range(mn, cap + 1)]
        assert table[mn:cap + 1].tolist() == want, (prob, mn, mx)
        assert table[mn] == 1 and table[mn:cap + 1].min() >= 1 and table[cap] <= mx
    assert lib.spslam_sim3_ransac_table(0.99, 20, 300, 10, None) == -1


def test_round_robin_helper_reproduces_compute_sim3s_loop(refs):
    """The candidate ComputeSim3's 5-iterations-each loop reaches first, from the first-success iterations alone."""
    import spslam_loop as L
    points, bad, cases, r = refs
    R = by_name(refs)
    for names in (("never", "calls_of_5", "first_at_63"), ("first_at_63", "calls_of_5", "loop_fixed"),
                  ("n_below_min", "never", "short_of_max"), ("first_at_64", "first_at_63", "n_below_min"),
                  ("loop_fixed", "first_at_0")):
        solvers = [C.new_solver(R[n][0], points, bad) for n in names]
        want, out = SR.compute_sim3_round_robin(solvers)
        first = []
        for n in names:                                               # one call of everything per candidate
            s = C.new_solver(R[n][0], points, bad)
            T12, _, _, _ = s.iterate(R[n][0]["max_iterations"])
            first.append(s.mnIterations - 1 if T12 is not None else None)
        got, rnd = L.compute_sim3_round_robin(first)
        assert got == want, (names, first, got, want)
        if want is not None:
            assert solvers[want].mnIterations - 1 == first[want] and rnd == first[want] // 5


# ---------------------------------------------------------------- the float expressions against the compiler
PROBE = r"""
extern "C" void sim3_probe(float fx, float fy, float cx, float cy, float X, float Y, float z, float* out) {
    // Sim3Solver::Project / FromCameraToImage: Sim3Solver.cc:396-401, :417-421
    const float invz = 1/(z);
    const float x = X*invz;
    const float y = Y*invz;
    out[0] = invz; out[1] = x; out[2] = y; out[3] = fx*x+cx; out[4] = fy*y+cy;
}
"""


def test_sim3_expressions_match_gcc_march_native(tmp_path):
    if "fma" not in pathlib.Path("/proc/cpuinfo").read_text():
        pytest.skip("host CPU without FMA: -march=native does not contract")
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    so = tmp_path / "probe.so"
    subprocess.run(["g++", "-O3", "-march=native", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    L = ctypes.CDLL(str(so))
    f = ctypes.c_float
    L.sim3_probe.argtypes = [f] * 7 + [ctypes.c_void_p]
    geo = C.geo()
    rng = np.random.default_rng(12)
    out = np.zeros(5, np.float32)
    for it in range(3000):
        X, Y = rng.normal(size=2).astype(np.float32)
        z = _f(rng.uniform(-2.0, 8.0)) if it % 10 else _f(0.0)
        invz, u, v, _ = FR.projection(geo, X, Y, z)
        with np.errstate(all="ignore"):
            want = np.array([invz, _f(X * invz), _f(Y * invz), u, v], np.float32)
        L.sim3_probe(*[_f(g) for g in geo[:4]], X, Y, z, out.ctypes.data)
        assert np.array_equal(out, want, equal_nan=True), (it, out, want)


# ---------------------------------------------------------------- the kernels' arithmetic, built for the host
CORR = np.dtype([("X1", "<f4", 3), ("X2", "<f4", 3), ("p1", "<f4", 2), ("p2", "<f4", 2), ("b1", "<f4"), ("b2", "<f4"),
                 ("i1", "<i4"), ("pad", "<i4")])


def test_host_build_of_the_kernel_arithmetic_equals_the_referee(refs, tmp_path):
    """sim3_math.h is what the gfx950 kernels run; built with g++ (contraction off, as the device build) it must
    give the referee's draws, s, R, t, T12, T21 and inlier flags bit for bit (NaN for NaN)."""
    so = tmp_path / "sim3_math_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so),
                    str(ROOT / "tests" / "sim3_math_host.cpp")], check=True)
    L = ctypes.CDLL(str(so))
    V = ctypes.c_void_p
    L.sim3_host_draw3.argtypes = [V, ctypes.c_int, ctypes.c_int, V]
    L.sim3_host_hypothesis.argtypes = [V, V, ctypes.c_int, V]
    L.sim3_host_inlier.argtypes = [V, V, V, V]
    assert CORR.itemsize == 56
    _, _, cases, r = refs
    cam = np.array(C.geo()[:4], np.float32)
    n_hyp = n_nan = 0
    for c, (calls, s) in zip(cases, r):
        corr = np.zeros(s.N, CORR)
        for i in range(s.N):
            corr[i]["X1"], corr[i]["X2"] = s.mvX3Dc1[i], s.mvX3Dc2[i]
            corr[i]["p1"], corr[i]["p2"] = s.mvP1im1[i], s.mvP2im2[i]
            corr[i]["b1"], corr[i]["b2"], corr[i]["i1"] = s.mvnMaxError1[i], s.mvnMaxError2[i], s.mvnIndices1[i]
        for (k, triple, sc, R, t, T12, T21, flags) in s.trace["hyps"]:
            idx = np.zeros(3, np.int32)
            rnd = np.ascontiguousarray(c["rand"][3 * k:3 * k + 3])
            L.sim3_host_draw3(rnd.ctypes.data, C.RAND_MAX, s.N, idx.ctypes.data)
            assert idx.tolist() == triple, (c["name"], k)
            X1 = np.array([s.mvX3Dc1[i] for i in triple], np.float32)
            X2 = np.array([s.mvX3Dc2[i] for i in triple], np.float32)
            out = np.zeros(37, np.float32)
            L.sim3_host_hypothesis(X1.ctypes.data, X2.ctypes.data, int(c["fix_scale"]), out.ctypes.data)
            want = np.concatenate([[sc], R.reshape(9), t, T12[:3].reshape(12), T21[:3].reshape(12)]).astype(np.float32)
            n_hyp += 1
            if np.isnan(want).any():
                n_nan += 1
                assert np.array_equal(np.isnan(out), np.isnan(want)), (c["name"], k)
                assert np.array_equal(out[~np.isnan(want)], want[~np.isnan(want)]), (c["name"], k)
            else:
                assert out.tobytes() == want.tobytes(), (c["name"], k, out, want)
            T12c, T21c = np.ascontiguousarray(out[13:25]), np.ascontiguousarray(out[25:37])
            got = [bool(L.sim3_host_inlier(corr[i:i + 1].ctypes.data, T12c.ctypes.data, T21c.ctypes.data,
                                           cam.ctypes.data)) for i in range(s.N)]
            assert got == flags, (c["name"], k)
    assert n_hyp > 900 and n_nan >= 5
