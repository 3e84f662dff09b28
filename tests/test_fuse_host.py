"""CPU checks of the Fuse search's restatement (tests/fuse_ref.py) and cases (tests/fuse_cases.py):

* the whole call ORBmatcher::Fuse(pKF, vpMapPoints, th) over a map model -- Replace, AddObservation and the
  recomputed descriptors included -- sees for every point the (bestIdx, bestDist) of the search over the map as it
  was on entry, and returns the number of points with bestDist <= TH_LOW: the device entry's contract;
* every case reaches the branch it is there for;
* the restated float expressions equal what g++ -O3 -march=native makes of the same arithmetic.
"""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import fuse_cases as FC
import fuse_ref as FR
from matcher_ref import f32 as _f


# ---------------------------------------------------------------- the whole call against the snapshot
def _model():
    """A map around problem real0: keyframe 9 is pKF.  The list holds the problem's points, then a second map point
    at the place of every fifth fused one (they collide on its keypoint), then points that are bad or already in
    pKF.  pKF already holds points on some of the keypoints the search will choose: with more observations, with
    fewer, and a bad one."""
    q = FC.real_problems()[0]
    geo = q["geo"]
    P0 = q["LP"][:400]
    kf = FC.keyframe_of(q)
    snap, _ = FR.snapshot_search(q["lfr"]["Tcw"], P0, kf["kun"], kf["desc"], kf["ur"], kf["go"], kf["gi"], geo)
    fused = np.flatnonzero(snap["best_dist"] <= FR.TH_LOW)
    assert len(fused) > 100
    rng = np.random.default_rng(5)
    n_src = 700
    kfs = {k: dict(points={}, desc=rng.integers(0, 256, (n_src, 32), dtype=np.uint8),
                   ur=np.where(rng.uniform(size=n_src) < 0.7, 50.0, -1.0).astype(np.float32), bad=False)
           for k in (0, 1, 2)}
    kfs[9] = dict(points={}, desc=kf["desc"], ur=kf["ur"], bad=False)
    points, pids = {}, []

    def new_point(pid, rec, observers):
        points[pid] = dict(rec=rec.copy(), obs={}, nobs=0, bad=False)
        for k in observers:
            idx = len(kfs[k]["points"])
            kfs[k]["points"][idx] = pid
            FR.add_observation(points, kfs, pid, k, idx)

    for i in range(len(P0)):
        new_point(i, P0[i], (0, 1) if i % 3 else (0,))
        pids.append(i)
    for n, i in enumerate(fused[::5]):                    # a second point at the same place: collides with point i
        new_point(1000 + n, P0[i], (0, 1, 2) if n % 2 else (2,))
        pids.append(1000 + n)
    held = {}
    for n, i in enumerate(fused[1::5]):                   # pKF's keypoint already holds a point
        pid = 2000 + n
        new_point(pid, P0[i], (0, 1, 2) if n % 3 == 0 else ((1,) if n % 3 == 1 else (0, 2)))
        idx = int(snap[i]["best_idx"])
        if idx in kfs[9]["points"]:
            continue
        kfs[9]["points"][idx] = pid
        FR.add_observation(points, kfs, pid, 9, idx)
        if n % 3 == 2:
            points[pid]["bad"] = True
        held[int(i)] = pid
    for n, i in enumerate(fused[2::25]):                  # in the list, but bad or already in pKF
        if n % 2:
            points[int(i)]["bad"] = True
        else:
            free = next(k for k in range(len(kf["kun"])) if k not in kfs[9]["points"])
            kfs[9]["points"][free] = int(i)
            FR.add_observation(points, kfs, int(i), 9, free)
    pids += [2000, 2001]                                  # points pKF holds, listed as well (IsInKeyFrame)
    return q, kf, geo, points, kfs, pids, held


def test_whole_call_sees_the_snapshot_search_and_counts_its_fuses():
    q, kf, geo, points, kfs, pids, held = _model()
    assert len(set(pids)) == len(pids)                    # the contract: a point at most once
    P = FC.stack([points[p]["rec"] for p in pids])
    skip = np.array([points[p]["bad"] or 9 in points[p]["obs"] for p in pids], np.uint8)
    desc_before = {p: points[p]["rec"]["desc"].copy() for p in points}
    snap, n_snap = FR.snapshot_search(q["lfr"]["Tcw"], P, kf["kun"], kf["desc"], kf["ur"], kf["go"], kf["gi"], geo,
                                      skip=skip)
    n_fused, seen, actions = FR.fuse(points, kfs, 9, q["lfr"]["Tcw"], pids, kf["kun"], kf["go"], kf["gi"], geo)
    for n in range(len(pids)):
        if skip[n]:
            assert seen[n] is None and snap[n]["status"] == FR.SKIPPED, n
        else:
            assert seen[n] == (snap[n]["status"], snap[n]["level"], snap[n]["best_idx"], snap[n]["best_dist"]), n
    assert n_fused == n_snap == int((snap["best_dist"] <= FR.TH_LOW).sum())
    # the model went through every branch of :951-971, a bad pMPinKF (counted, nothing done) included
    kinds = {a[0] for a in actions}
    assert kinds == {"added", "replaces_kf_point", "replaced_by_kf_point", "kf_point_bad"}, kinds
    assert 2 < skip.sum() < len(pids) // 4
    added = {a[1] for a in actions if a[0] == "added"}
    collided = [a for a in actions if a[0] != "added" and a[2] in added]
    assert len(collided) >= 10                            # two listed points on one keypoint
    assert any(a[0] == "replaced_by_kf_point" and a[2] in held.values() for a in actions)
    assert any(a[0] == "replaces_kf_point" and a[2] in held.values() for a in actions)
    # and descriptors of listed points were recomputed during the call, after their own turn
    changed = [p for p in pids if not np.array_equal(points[p]["rec"]["desc"], desc_before[p])]
    assert len(changed) >= 5


# ---------------------------------------------------------------- what the cases reach
@pytest.fixture(scope="module")
def ran():
    kfs, problems = FC.build()
    out = {}
    for p in problems:
        traces = []
        res, nf = FC.reference(p, kfs, FC.geo(), traces)
        out[p["name"]] = (p, res, nf, traces)
    return out


def test_statuses_are_reached_by_construction(ran):
    _, res, nf, _ = ran["statuses"]
    assert res["status"].tolist() == [FR.BEHIND, FR.OUTSIDE_IMAGE, FR.OUTSIDE_IMAGE, FR.OUTSIDE_IMAGE,
                                      FR.OUTSIDE_IMAGE, FR.NO_CANDIDATES, FR.OUT_OF_RANGE, FR.OUT_OF_RANGE,
                                      FR.NO_CANDIDATES, FR.VIEW_ANGLE, FR.NO_CANDIDATES, FR.SEARCHED]
    assert nf == 1 and res[11]["best_idx"] == 0 and res[11]["best_dist"] == 0
    _, tr = ran["statuses"][0], ran["statuses"][3]
    assert tr[8]["view"][0] == tr[8]["view"][1] and tr[9]["view"][0] < tr[9]["view"][1]   # either side of 0.5
    assert tr[5]["u"] == np.nextafter(_f(640.0), _f(0.0)) and tr[5]["cells"][1] == 63
    assert res[5]["level"] == 7 and res[0]["level"] == 0
    every = set()
    for _, r, _, _ in ran.values():
        every |= set(r["status"].tolist())
    assert every == set(range(7))


def test_real_problems_fuse_and_sizes_straddle_the_workgroup(ran):
    for name in ("real0", "real1"):
        p, res, nf, _ = ran[name]
        assert nf > 0.3 * len(p["P"]) and len(p["P"]) > 3 * FC.PTS_PER_GROUP, (name, nf, len(p["P"]))
        assert (res["status"] == FR.SEARCHED).sum() > nf > 0
    assert [len(ran[f"real0_n{n}"][0]["P"]) for n in (0, 1, 63, 64, 65)] == [0, 1, 63, 64, 65]
    p, res, nf, _ = ran["real1_skip"]
    assert 0 < (res["status"] == FR.SKIPPED).sum() == p["skip"].sum() < len(p["P"])
    assert nf < ran["real1"][2]
    p, res, nf, _ = ran["keyframe_without_keypoints"]
    assert nf == 0 and set(res["status"].tolist()) <= {FR.NO_CANDIDATES, FR.OUT_OF_RANGE, FR.OUTSIDE_IMAGE,
                                                       FR.VIEW_ANGLE, FR.BEHIND}
    assert (res["status"] == FR.NO_CANDIDATES).any()


def test_windows_are_clipped_and_wide(ran):
    for name, min_cells in (("clipped_th3", 1), ("clipped_th30", 20)):
        _, res, _, tr = ran[name]
        cells = [t["cells"] for t in tr if "cells" in t]
        assert {c[0] for c in cells} >= {0} and {c[1] for c in cells} >= {63}
        assert {c[2] for c in cells} >= {0} and {c[3] for c in cells} >= {47}
        assert max((c[1] - c[0] + 1) * (c[3] - c[2] + 1) for c in cells) >= min_cells
        assert (res["status"] == FR.SEARCHED).sum() >= 6
    _, res, _, tr = ran["real0_th30"]
    assert max((t["cells"][1] - t["cells"][0] + 1) * (t["cells"][3] - t["cells"][2] + 1)
               for t in tr if "cells" in t) > 40          # many cells per lane of a 4-lane group


def test_ties_chi2_stereo_boundary_and_levels(ran):
    _, res, nf, tr = ran["ties_all_zero"]
    tied = [t for t in tr if len(t.get("dists", ())) >= 2]
    assert len(tied) >= 10 and all(set(t["dists"]) == {0} for t in tied) and nf > 50
    for name, stereo in (("chi2_stereo_second_wins", True), ("chi2_mono_second_wins", False)):
        _, res, nf, tr = ran[name]
        assert tr[0]["rejected_chi2"] == [(0, 1, stereo)]                # the nearest descriptor, rejected
        assert (res[0]["best_idx"], res[0]["best_dist"]) == (1, 20) and nf == 1
    _, res, nf, tr = ran["uright_zero_is_stereo"]
    assert res[0]["status"] == FR.SEARCHED and res[0]["best_idx"] == -1 and res[0]["best_dist"] == 256 and nf == 0
    assert tr[0]["rejected_chi2"] == [(0, 2, True)]
    _, res, nf, tr = ran["levels"]
    assert sorted(tr[0]["levels"]) == [-2, -1, 0, 1] and res[0]["level"] == 2
    assert (res[0]["best_idx"], res[0]["best_dist"]) == (3, 25)


def test_keyframe_bounds_are_ints_with_the_second_camera():
    g, kfs, problems = FC.build_distorted()
    p = problems[0]
    traces = []
    res, nf = FC.reference(p, kfs, g, traces)
    assert res["status"].tolist() == [FR.OUTSIDE_IMAGE] * 4 + [FR.SEARCHED] * 2 and nf == 2
    assert all(float(b) != int(b) for b in g[5:9])
    for i in range(4):   # inside the Frame's float bounds, outside the KeyFrame's int bounds
        _, u, v, _ = FR.projection(g, *p["P"][i]["xw"])
        assert g[5] <= u <= g[6] and g[7] <= v <= g[8]
        assert not (int(g[5]) <= u < int(g[6]) and int(g[7]) <= v < int(g[8]))
    assert traces[4]["cells"][0] == 0 and traces[4]["cells"][2] == 0
    assert traces[5]["cells"][1] == 63 and traces[5]["cells"][3] == 47
    assert res[4]["best_idx"] == 1 and res[5]["best_idx"] == 2   # octave 1 is outside level 0's range


# ---------------------------------------------------------------- the float expressions against the compiler
PROBE = r"""
extern "C" void fuse_probe(float fx, float fy, float cx, float cy, float bf, float X, float Y, float z, float kx,
                           float ky, float kr, float s2, float* out, int* over) {
    const float invz = 1 / z;
    const float x = X * invz;
    const float y = Y * invz;
    const float u = fx * x + cx;
    const float v = fy * y + cy;
    const float ur = u - bf * invz;
    const float ex = u - kx;
    const float ey = v - ky;
    const float er = ur - kr;
    const float e3 = ex * ex + ey * ey + er * er;
    const float e2 = ex * ex + ey * ey;
    out[0] = u; out[1] = v; out[2] = ur; out[3] = e3; out[4] = e2;
    over[0] = e3 * s2 > 7.8;
    over[1] = e2 * s2 > 5.99;
}
"""


def test_fuse_expressions_match_gcc_march_native(tmp_path):
    if "fma" not in pathlib.Path("/proc/cpuinfo").read_text():
        pytest.skip("host CPU without FMA: -march=native does not contract")
    import synth
    K = synth.TUM3
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    so = tmp_path / "probe.so"
    subprocess.run(["g++", "-O3", "-march=native", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    L = ctypes.CDLL(str(so))
    f = ctypes.c_float
    L.fuse_probe.argtypes = [f] * 12 + [ctypes.c_void_p, ctypes.c_void_p]
    geo = [_f(K[k]) for k in ("fx", "fy", "cx", "cy", "bf")]
    isg2 = FR.inv_level_sigma2([_f(1.2) ** l for l in range(8)])
    rng = np.random.default_rng(11)
    out, over = np.zeros(5, np.float32), np.zeros(2, np.int32)
    n_near = 0
    for it in range(3000):
        X, Y = rng.normal(size=2).astype(np.float32)
        z = _f(rng.uniform(0.3, 6.0))
        _, u, v, ur = FR.projection(geo, X, Y, z)
        s2 = isg2[it % 8]
        if it % 2:   # a keypoint on the chi-square threshold, a few floats either side
            lim = 7.8 if it % 4 == 1 else 5.99
            dx = np.sqrt(lim / float(s2) / (3 if it % 4 == 1 else 2))
            kx, ky = _f(u - _f(dx)), _f(v - _f(dx))
            kr = _f(ur - _f(dx))
            for _ in range(int(rng.integers(0, 6))):
                kx = np.nextafter(kx, _f(rng.choice([-1e9, 1e9])))
            n_near += 1
        else:
            kx, ky, kr = _f(u + rng.normal() * 2), _f(v + rng.normal() * 2), _f(ur + rng.normal() * 2)
        kr = max(kr, _f(0.0))   # a stereo keypoint (mvuRight >= 0); the two-term form does not read it
        L.fuse_probe(*geo, X, Y, z, kx, ky, kr, s2, out.ctypes.data, over.ctypes.data)
        assert (out[0], out[1], out[2]) == (u, v, ur), it
        ex, ey, er = _f(u - kx), _f(v - ky), _f(ur - kr)
        e2 = FR.fma(ex, ex, _f(ey * ey))
        e3 = FR.fma(er, er, e2)
        assert out[4] == e2 and out[3] == e3, it
        assert bool(over[0]) == (not FR.chi2_passes(u, v, ur, kx, ky, kr, s2)), it
        assert bool(over[1]) == (not FR.chi2_passes(u, v, ur, kx, ky, _f(-1), s2)), it
    assert n_near == 1500
