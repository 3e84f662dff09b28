"""CPU checks of the CreateNewMapPoints restatement (tests/triangulation_ref.py) and cases
(tests/triangulation_cases.py):

* every case reaches what it is there for (statuses, sources, ties, thresholds, list lengths);
* the restated float expressions equal what g++ -O3 -march=native makes of the reference's lines, and
  `cos(2*atan2(mb/2, depth))` under `using namespace std` is the float overload;
* the chosen 4x4 null-vector semantics agree with a float64 SVD of the same matrix;
* accepted points lie on the scene's surface;
* the whole call over a map model equals per-neighbour rounds of search + triangulation with the has-point masks
  updated in between -- the device entry's contract.
"""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import triangulation_cases as TC
import triangulation_ref as TR
from matcher_ref import f32 as _f

# Largest relative difference |x3D - x3D_64| / |x3D_64| between the restatement's Jacobi (float columns) and the
# float64 numpy.linalg.svd null vector of the same float A, measured over every accepted (SPSLAM_TRI_NEW, SVD) match
# of the cases (89 of them, real pairs of 0.08 m baseline included): 6.2e-7.  Asserted with a 4x margin for inputs
# conditioned differently from these.
SVD_REL_MEASURED = 6.2e-7
SVD_REL_BOUND = 4 * SVD_REL_MEASURED


@pytest.fixture(scope="module")
def searched():
    cam = TC.cam()
    out = {}
    for c in TC.search_cases():
        tr = {}
        m, n = TR.search_for_triangulation(c["kf1"], c["kf2"], c["F12"], c["only_stereo"], c["check_orientation"], cam,
                                           tr)
        out[c["name"]] = (c, m, n, tr)
    return out


@pytest.fixture(scope="module")
def triangulated():
    cam = TC.cam()
    out = {}
    for c in TC.triangulation_cases():
        infos = {}
        rec, nn = TR.triangulate_all(c["kf1"], c["kf2"], c["match12"], cam, infos)
        out[c["name"]] = (c, rec, nn, infos)
    return out


# ---------------------------------------------------------------- what the search cases reach
def test_list_lengths_ties_and_thresholds(searched):
    c, m, n, tr = searched["lists"]
    fv2 = c["kf2"]["fv"]
    lengths = sorted(int(fv2["start"][k + 1] - fv2["start"][k]) for k in range(len(fv2["nodes"])) if
                     fv2["nodes"][k] >= 100)
    assert lengths == sorted(L for L in TC.LIST_LENGTHS if L) and TC.GROUP == 8
    assert m[0] == -1 and (m[1:] >= 0).all() and n == len(TC.LIST_LENGTHS) - 1
    for i in range(1, len(m)):                                      # the minimum recurs in the long lists: the later wins
        d = [s[1] for s in tr[i] if s[3]]
        best = min(d)
        last = max(s[0] for s in tr[i] if s[3] and s[1] == best)
        assert m[i] == last
    assert any(sum(1 for s in tr[i] if s[1] == min(x[1] for x in tr[i])) >= 2 for i in range(4, 7))

    c, m, n, tr = searched["ties_thresholds_has"]
    assert tr[0] == [(0, 12, True, True), (1, 12, True, True)] and m[0] == 1          # tie, both pass: the later
    assert tr[1] == [(2, 12, True, True), (3, 12, True, False)] and m[1] == 2         # the later fails: the earlier
    assert tr[2] == [(4, 50, True, True)] and m[2] == 4 and tr[3] == [] and m[3] == -1  # 50 and 51
    assert m[4] == -1 and 4 not in tr                                # key 1 holds a point
    assert [s[0] for s in tr[5]] == [8] and m[5] == 8                # key 2's nearest holds a point
    assert m[6] == m[7] == 9                                         # two key-1 features, one idx2
    assert n == 6


def test_epipole_octaves_and_degenerate_inputs(searched):
    c, m, n, tr = searched["epipole_radius"]
    ex, ey = TC.epipole_G()
    k2 = c["kf2"]["kun"]
    d2 = [TR.fma(ex - k2[j]["x"], ex - k2[j]["x"], (ey - k2[j]["y"]) * (ey - k2[j]["y"])) for j in range(3)]
    assert d2[0] > 100 and d2[1] == 100 and d2[2] < 100              # outside, exactly on, inside the radius
    assert tr[0] == [(0, 20, True, True), (1, 10, True, True), (2, 5, False, False)] and m[0] == 1
    assert [s[3] for s in tr[1]] == [True, True, True] and m[1] == 2   # a stereo key-1 feature: no epipole test

    c, m, n, tr = searched["octaves"]
    assert m.tolist() == [2 * o for o in range(8)]
    for o in range(8):
        assert [s[3] for s in tr[o]] == [True, False] and c["kf2"]["kun"][2 * o]["octave"] == o

    c, m, n, tr = searched["c2z_zero"]
    ex, ey = TR.epipole(c["kf1"], c["kf2"], TC.cam())
    assert np.isinf(ex) and np.isnan(ey) and n == 6 and all(s[2] for i in range(6) for s in tr[i])
    c, m, n, tr = searched["zero_F12"]
    assert n == 0 and all(not s[3] for i in range(6) for s in tr[i]) and sum(len(tr[i]) for i in range(6)) >= 6
    for name in ("all_key1_hold_points", "key1_empty", "key2_empty", "empty_feature_vectors",
                 "disjoint_feature_vectors"):
        assert searched[name][2] == 0 and (searched[name][1] == -1).all(), name
    assert len(searched["key1_empty"][1]) == 0 and len(searched["key2_empty"][0]["kf2"]["kun"]) == 0
    assert searched["stereo_mix_only0"][2] == 8 and searched["stereo_mix_only1"][2] == 2


def test_orientation_histograms(searched):
    c, m, n, tr = searched["orientation_bins_removed"]
    assert sorted(x for x in tr["hist"] if x) == [2, 3, 5, 10] and n == 18 and (m >= 0).sum() == 18
    c, m, n, tr = searched["orientation_second_below_tenth"]
    assert tr["keep"] == (0, -1, -1) and n == 21
    c, m, n, tr = searched["real0_orientation"]
    assert 0 < n <= searched["real0"][2]


def test_real_pairs_match_and_create_points(searched):
    cam = TC.cam()
    for seq in TC.SEQS:
        c, m, n, _ = searched[f"real{seq}"]
        rec, nn = TR.triangulate_all(c["kf1"], c["kf2"], m, cam)
        assert n >= 20 and nn >= 10, (seq, n, nn)
        assert not TR.baseline_is_short(c["kf1"], c["kf2"], cam)
    assert TR.baseline_is_short(TC.real_keyframes()[(0, 0)], TC.real_keyframes()[(0, 3)], cam)


# ---------------------------------------------------------------- what the triangulation cases reach
def test_every_status_and_source_occurs(triangulated):
    statuses, sources, types = set(), set(), set()
    for name, (c, rec, nn, infos) in triangulated.items():
        if c["want"] is not None:
            assert (rec[0]["status"], rec[0]["source"]) == (c["want"], c["source"]), name
        statuses |= set(rec["status"].tolist())
        sources |= set(rec["source"][rec["status"] == TR.NEW].tolist())
        types |= {i["types"] for i in infos.values()}
    assert statuses == set(range(10)) and sources == {TR.FROM_SVD, TR.FROM_STEREO_1, TR.FROM_STEREO_2}
    assert types == {(True, True), (True, False), (False, True), (False, False)}
    assert triangulated["rays_apart_cos_negative"][3][0]["cos_rays"] <= 0
    c, rec, _, infos = triangulated["w_zero_rank_deficient"]
    assert (infos[0]["A"][:, 2] == 0).all() and infos[0]["w"][3] == 0 and infos[0]["v"] == [0, 0, 1, 0]
    # the sweep limit: a NaN dot product keeps every pair rotating; the match is accepted with a NaN point
    c, rec, nn, infos = triangulated["sweep_limit_overflowing_translation"]
    assert infos[0]["sweeps"] == TR.JACOBI_SWEEPS and np.isinf(infos[0]["A"][:2, 3]).all()
    assert np.isfinite(c["kf1"]["Tcw"]).all() and all(np.isnan(x) for x in infos[0]["v"])
    assert np.isnan([rec[0]["x"], rec[0]["y"], rec[0]["z"]]).all() and nn == 1
    c, rec, _, infos = triangulated["w_zero_one_overflowing_row"]
    assert infos[0]["sweeps"] < TR.JACOBI_SWEEPS and np.isinf(infos[0]["A"][:, 3]).sum() == 1 and infos[0]["v"][3] == 0
    c, rec, _, _ = triangulated["new_stereo1_distorted_keys"]
    assert c["kf1"]["keys"][0]["x"] != c["kf1"]["kun"][0]["x"]
    assert rec[0]["x"] != triangulated["new_stereo1"][1][0]["x"]
    c, rec, nn, _ = triangulated["mixed_70"]
    assert nn >= 30 and (rec["status"] == TR.NO_MATCH).sum() == 10


def test_jacobi_on_identical_rays_and_against_float64(triangulated, searched):
    # identical rays (a rank-deficient A that the parallax test keeps from the device): the two null directions
    T1, T2 = TC.pose(), TC.pose((-0.3, 0, 0))
    info = {}
    v = TR.jacobi_null_vector(TR.triangulation_matrix([_f(0.1), _f(-0.2)], [_f(0.1), _f(-0.2)], T1, T2), info)
    assert info["sweeps"] < TR.JACOBI_SWEEPS and abs(v[3]) < 1e-6 * max(abs(x) for x in v[:3])
    cam = TC.cam()
    worst, count = 0.0, 0
    sets = [(c, rec, infos) for c, rec, _, infos in triangulated.values()]
    for seq in TC.SEQS:
        c, m, _, _ = searched[f"real{seq}"]
        infos = {}
        rec, _ = TR.triangulate_all(c["kf1"], c["kf2"], m, cam, infos)
        sets.append((c, rec, infos))
    for c, rec, infos in sets:
        for i in np.flatnonzero((rec["status"] == TR.NEW) & (rec["source"] == TR.FROM_SVD)):
            A = infos[int(i)]["A"].astype(np.float64)
            if not np.isfinite(A).all():                            # the sweep-limit case: no float64 solution exists
                continue
            v64 = np.linalg.svd(A)[2][3]
            x64 = v64[:3] / v64[3]
            x = np.array([rec[i]["x"], rec[i]["y"], rec[i]["z"]], np.float64)
            worst = max(worst, float(np.linalg.norm(x - x64) / np.linalg.norm(x64)))
            count += 1
            assert infos[int(i)]["sweeps"] < TR.JACOBI_SWEEPS
    print(f"SVD against float64: worst relative difference {worst:.3g} over {count} accepted matches")
    assert count >= 60 and worst <= SVD_REL_BOUND, worst


def test_accepted_points_lie_on_the_surface(searched):
    """x3D's depth in the current keyframe against the rendered depth at the keypoint.  UnprojectStereo points are
    that depth (float rounding of the round trip).  For a triangulated point a reprojection error of e pixels moves
    the depth by z^2/(fx*b)*e, b the baseline; both keyframes passed chi2 = 5.991*sigma2 per image."""
    cam = TC.cam()
    n_svd = n_stereo = 0
    for seq in TC.SEQS:
        c, m, _, _ = searched[f"real{seq}"]
        kf1, kf2 = c["kf1"], c["kf2"]
        rec, _ = TR.triangulate_all(kf1, kf2, m, cam)
        b = float(np.linalg.norm(kf2["Ow"] - kf1["Ow"]))
        T1 = np.asarray(kf1["Tcw"], np.float64)
        for i in np.flatnonzero(rec["status"] == TR.NEW):
            z = float(kf1["depth"][i])
            if z <= 0:
                continue
            zc = float(T1[2, :3] @ np.array([rec[i]["x"], rec[i]["y"], rec[i]["z"]], np.float64) + T1[2, 3])
            if rec[i]["source"] == TR.FROM_STEREO_1:
                assert abs(zc - z) < 1e-5 * z
                n_stereo += 1
            elif rec[i]["source"] == TR.FROM_SVD:
                s1 = float(cam["scale"][int(kf1["kun"][i]["octave"])])
                s2 = float(cam["scale"][int(kf2["kun"][m[i]]["octave"])])
                e = np.sqrt(5.991) * (s1 + s2)
                assert abs(zc - z) < z * z / (float(cam["fx"]) * b) * e + 4 * 0.0012 * z * z, (seq, i, zc, z)
                n_svd += 1
    assert n_svd >= 10 and n_stereo >= 10


# ---------------------------------------------------------------- the whole call against per-neighbour rounds
def test_whole_call_equals_rounds_with_masks_between():
    cam = TC.cam()
    model, k1, neighbours = TC.chained_model(TC.SEQS[0])
    # the rounds, on has-point masks only (what the device does)
    has = {k: model["kfs"][k]["has"].copy() for k in model["kfs"]}
    expect = []
    for k2 in neighbours:
        kf1, kf2 = dict(model["kfs"][k1], has=has[k1]), dict(model["kfs"][k2], has=has[k2])
        if TR.baseline_is_short(kf1, kf2, cam):
            expect.append((TR.SHORT_BASELINE, None, None))
            continue
        m, _ = TR.search_for_triangulation(kf1, kf2, TR.compute_f12(kf1, kf2, TC.Kmat()), False, False, cam)
        rec, _ = TR.triangulate_all(kf1, kf2, m, cam)
        for i in np.flatnonzero(rec["status"] == TR.NEW):
            has[k1][i] = 1
            has[k2][m[i]] = 1
        expect.append((TR.SEARCHED, m, rec))
    rounds, nnew = TR.create_new_map_points(model, k1, neighbours, cam, TC.Kmat())
    assert [r[0] for r in rounds] == [TR.SEARCHED, TR.SHORT_BASELINE, TR.SEARCHED]
    total = 0
    for (st, m, rec), (est, em, erec) in zip(rounds, expect):
        assert st == est
        if st == TR.SEARCHED:
            assert np.array_equal(m, em) and rec.tobytes() == erec.tobytes()
            total += int((rec["status"] == TR.NEW).sum())
    assert nnew == total >= 15 and all((r[2]["status"] == TR.NEW).sum() >= 2 for r in rounds if r[0] == TR.SEARCHED)
    # the second searched round saw the first one's marks: key-1 features taken in round 0 are not matched again
    taken = np.flatnonzero(rounds[0][2]["status"] == TR.NEW)
    assert (rounds[2][1][taken] == -1).all()
    for k in model["kfs"]:
        assert np.array_equal(has[k], np.array([i in model["kfs"][k]["points"]
                                                for i in range(len(has[k]))], np.uint8)), k


def test_two_features_on_one_idx2_overwrite_in_the_model():
    cam = TC.cam()
    c = next(c for c in TC.search_cases() if c["name"] == "ties_thresholds_has")
    kf1, kf2 = dict(c["kf1"], points={4: 0}), dict(c["kf2"], points={7: 1})   # as its has-point flags say
    model = dict(kfs={0: kf1, 1: kf2}, points={0: {}, 1: {}})
    rounds, nnew = TR.create_new_map_points(model, 0, [1], cam, TC.Kmat())
    st, m, rec = rounds[0]
    assert st == TR.SEARCHED and m[6] == m[7] == 9
    assert rec[6]["status"] == rec[7]["status"] == TR.NEW
    first, second = kf1["points"][6], kf1["points"][7]
    assert first != second and kf2["points"][9] == second                      # the second AddMapPoint overwrote
    assert model["points"][first]["obs"] == {0: 6, 1: 9}                        # the first point keeps its observation
    assert model["points"][second]["obs"] == {0: 7, 1: 9}
    assert nnew == int((rec["status"] == TR.NEW).sum()) == len(model["points"]) - 2


# ---------------------------------------------------------------- the float expressions against the compiler
PROBE = r"""
#include <cmath>
using namespace std;   // Timer.h does this in front of LocalMapping.cc
extern "C" float stereo_cos(float mb, float depth) { return cos(2*atan2(mb/2,depth)); }
extern "C" void tri_probe(const float* in, const float* F12, float* out, int* cmp) {
    const float fx = in[0], fy = in[1], cx = in[2], cy = in[3], mbf = in[4];
    const float C2x = in[5], C2y = in[6], C2z = in[7], k1x = in[8], k1y = in[9], k2x = in[10], k2y = in[11];
    const float sigma2 = in[12], scale = in[13], x1 = in[14], y1 = in[15], z1 = in[16], kur = in[17];
    const float invz = 1.0f/C2z;
    const float ex = fx*C2x*invz+cx;
    const float ey = fy*C2y*invz+cy;
    const float distex = ex-k2x;
    const float distey = ey-k2y;
    out[0] = ex; out[1] = ey; out[2] = distex*distex+distey*distey;
    cmp[0] = distex*distex+distey*distey<100*scale;
    const float a = k1x*F12[0]+k1y*F12[3]+F12[6];
    const float b = k1x*F12[1]+k1y*F12[4]+F12[7];
    const float c = k1x*F12[2]+k1y*F12[5]+F12[8];
    const float num = a*k2x+b*k2y+c;
    const float den = a*a+b*b;
    const float dsqr = num*num/den;
    out[3] = a; out[4] = b; out[5] = c; out[6] = dsqr;
    cmp[1] = dsqr<3.84*sigma2;
    const float invz1 = 1.0/z1;
    float u1 = fx*x1*invz1+cx;
    float u1_r = u1 - mbf*invz1;
    float v1 = fy*y1*invz1+cy;
    float errX1 = u1 - k1x;
    float errY1 = v1 - k1y;
    float errX1_r = u1_r - kur;
    out[7] = u1; out[8] = v1; out[9] = u1_r;
    out[10] = errX1*errX1+errY1*errY1;
    out[11] = errX1*errX1+errY1*errY1+errX1_r*errX1_r;
    cmp[2] = (errX1*errX1+errY1*errY1)>5.991*sigma2;
    cmp[3] = (errX1*errX1+errY1*errY1+errX1_r*errX1_r)>7.8*sigma2;
}
"""


def test_expressions_match_gcc_march_native(tmp_path):
    if "fma" not in pathlib.Path("/proc/cpuinfo").read_text():
        pytest.skip("host CPU without FMA: -march=native does not contract")
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    so = tmp_path / "probe.so"
    subprocess.run(["g++", "-O3", "-march=native", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    L = ctypes.CDLL(str(so))
    L.tri_probe.argtypes = [ctypes.c_void_p] * 4
    L.stereo_cos.restype, L.stereo_cos.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    cam = TC.cam()
    rng = np.random.default_rng(12)
    # cos(2*atan2(mb/2, depth)): the float overloads, not the double ones rounded
    differs = 0
    for _ in range(2000):
        d = _f(rng.uniform(0.2, 8.0))
        want = _f(TR._libm.cosf(_f(2.0) * _f(TR._libm.atan2f(cam["mb"] / _f(2.0), d))))
        assert _f(L.stereo_cos(cam["mb"], d)) == want
        differs += want != _f(np.cos(2 * np.arctan2(float(cam["mb"]) / 2, float(d))))
    assert differs > 0
    T = np.eye(4, dtype=np.float32)
    out, cmp = np.zeros(12, np.float32), np.zeros(4, np.int32)
    near = 0
    for it in range(2000):
        o = it % 8
        sigma2, scale = cam["sigma2"][o], cam["scale"][o]
        C2 = rng.normal(size=3).astype(np.float32) * _f(0.3) + np.array([0, 0, 0.5], np.float32)
        F = (rng.normal(size=9) * [1e-6, 1e-5, 1e-3, 1e-5, 1e-6, 1e-3, 1e-3, 1e-3, 1]).astype(np.float32)
        k1 = dict(x=_f(rng.uniform(0, 640)), y=_f(rng.uniform(0, 480)), octave=o)
        kf1 = dict(Ow=C2)
        kf2 = dict(Tcw=T)
        ex, ey = TR.epipole(kf1, kf2, cam)
        line = TR.epipolar_line(k1, F)
        k2 = dict(x=_f(rng.uniform(0, 640)), y=_f(rng.uniform(0, 480)), octave=o)
        if it % 2:                                                   # near the two thresholds of the search
            r = np.sqrt(100.0 * float(scale))
            k2["x"], k2["y"] = _f(ex - _f(r * 0.6)), _f(ey - _f(r * 0.8))
            a, b, c = (float(v) for v in line)
            lim = np.sqrt(3.84 * float(sigma2) * (a * a + b * b))
            if abs(b) > 1e-9:
                k2["y"] = _f(-(a * float(k2["x"]) + c - lim) / b)
            for _ in range(int(rng.integers(0, 4))):
                k2["y"] = np.nextafter(k2["y"], _f(rng.choice([-1e9, 1e9])))
            near += 1
        X = [_f(rng.normal()), _f(rng.normal()), _f(rng.uniform(0.3, 6.0))]
        u, v, u_r, e2, _ = TR.reprojection(T, X, X[2], dict(k1, x=_f(0), y=_f(0)), _f(0), False, cam)
        if it % 2:                                                   # a keypoint near the chi-square bounds
            dx = np.sqrt((5.991 if it % 4 == 1 else 7.8) * float(sigma2) / (2 if it % 4 == 1 else 3))
            k1["x"], k1["y"], kur = _f(u - _f(dx)), _f(v - _f(dx)), _f(u_r - _f(dx))
        else:
            kur = _f(u_r + rng.normal())
        line = TR.epipolar_line(k1, F)
        inp = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["bf"], *C2, k1["x"], k1["y"], k2["x"], k2["y"],
                        sigma2, scale, *X, kur], np.float32)
        L.tri_probe(inp.ctypes.data, F.ctypes.data, out.ctypes.data, cmp.ctypes.data)
        with np.errstate(all="ignore"):
            dx, dy = ex - k2["x"], ey - k2["y"]
            d2 = TR.fma(dx, dx, dy * dy)
        assert (out[0], out[1], out[2]) == (ex, ey, d2), it
        assert bool(cmp[0]) == bool(d2 < _f(100) * scale), it
        tr = []
        ok = TR.check_dist_epipolar_line(line, k2, cam["sigma2"], tr)
        assert (out[3], out[4], out[5]) == line and float(out[6]) == tr[0][0] and bool(cmp[1]) == ok, it
        u, v, u_r, e2, b2 = TR.reprojection(T, X, X[2], k1, kur, False, cam)
        _, _, _, e3, b3 = TR.reprojection(T, X, X[2], k1, kur, True, cam)
        assert (out[7], out[8], out[9], out[10], out[11]) == (u, v, u_r, e2, e3), it
        assert bool(cmp[2]) == bool(np.float64(e2) > b2) and bool(cmp[3]) == bool(np.float64(e3) > b3), it
    assert near == 1000
