"""CPU checks of the loop-closing matchers' restatements (tests/loop_match_ref.py) and cases
(tests/loop_match_cases.py):

* every case reaches the branch it is there for, as asserted conditions on what the restatement saw;
* the whole call ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) over fuse_ref's map model -- the walk
  :1082-1096 with vpReplacePoint, AddObservation / AddMapPoint and the bad pMPinKF -- sees for every point the
  search over the map as it was on entry and returns the number of points with bestDist <= TH_LOW: the device
  entry's contract;
* the restated scalar expressions equal what g++ -O3 -march=native makes of the same arithmetic.
"""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import fuse_cases as FC
import fuse_ref as FR
import loop_match_cases as C
import loop_match_ref as LR
from matcher_ref import f32 as _f

G, K = C.PTS_PER_GROUP, C.PROJ_KEYS


# ---------------------------------------------------------------- SearchByBoW(KF, KF)
@pytest.fixture(scope="module")
def bow():
    out = {}
    for c in C.bow_cases():
        tr = {}
        m, n = C.bow_reference(c, tr)
        out[c["name"]] = (c, m, n, tr)
    return out


def test_bow_real_pairs_feed_a_sim3_solver(bow):
    for name in ("real_12_16", "real_16_12", "real_12_16_no_orientation"):
        c, m, n, tr = bow[name]
        assert n >= 20 and n == int((m >= 0).sum()), (name, n)          # LoopClosing.cc:269
        assert tr["shared"] > C.BOW_WAVES and tr["blocked"] > 0 and tr["second_changed"] > 0
    # a cleared has_point on either side loses matches
    assert bow["real_has_point_cleared_on_1"][2] < bow["real_12_16"][2]
    assert bow["real_has_point_cleared_on_2"][2] < bow["real_12_16"][2]
    c, m, n, _ = bow["real_12_16"]
    assert len(np.unique(m[m >= 0])) == n                               # vbMatched2: an idx2 is given once


def test_bow_node_lists_and_shared_node_counts(bow):
    c, m, n, tr = bow["node_lists_0_1_63_64_65"]
    sizes = np.diff(c["kf2"]["fv"]["start"]).tolist()
    assert sizes == [0, 1, 63, 64, 65] and tr["shared"] == 5
    last = [int(c["kf2"]["fv"]["features"][e - 1]) for e in c["kf2"]["fv"]["start"][1:][1:]]
    assert m[2::2].tolist() == last and m[0] == -1                      # the list's last keypoint, at every size
    for shared in (0, 1, C.BOW_WAVES, C.BOW_WAVES + 1):
        assert bow[f"shared_nodes_{shared}"][3]["shared"] == shared == bow[f"shared_nodes_{shared}"][2]
    assert bow["empty_feature_vectors"][2] == 0 and bow["kf2_without_keypoints"][2] == 0


def test_bow_order_thresholds_and_histogram(bow):
    c, m, n, tr = bow["same_idx2_wanted_twice"]
    assert m.tolist() == [0, 1] and tr["blocked"] == 1 and tr["second_changed"] == 1
    assert tr["ratio"] == [(1, 30), (28, 43)]                           # the second sees (28, 43), not (1, 28)
    c, m, n, tr = bow["same_idx2_list_order"]
    assert m.tolist() == [1, 2]                                         # KF1 index 1 is first in the list: it gets idx2 2
    c, m, n, tr = bow["distance_49_and_50"]
    assert tr["dists"] == [49, 50] and m.tolist() == [0, -1]            # 50 < TH_LOW fails; `<=` would take it
    c, m, n, tr = bow["ratio_29_30_31"]
    assert tr["ratio"] == [(29, 40), (30, 40), (31, 40)] and (m >= 0).tolist() == [True, False, False]
    c, m, n, tr = bow["has_point_either_side"]
    assert m.tolist() == [-1, 0, 3]
    c, m, n, tr = bow["equal_distances"]
    assert tr["ratio"] == [(4, 4), (4, 4)] and n == 2
    assert m.tolist() == [int(c["kf2"]["fv"]["features"][0]), int(c["kf2"]["fv"]["features"][3])]
    c, m, n, tr = bow["histogram_removes_and_blocks"]
    first, second = int(c["kf1"]["fv"]["features"][-2]), int(c["kf1"]["fv"]["features"][-1])
    x = tr["removed"][0][1]
    assert tr["removed"] == [(first, x)] and m[first] == -1 and tr["matched2"][x]
    assert m[second] >= 0 and m[second] != x and x not in m             # x stays blocked, and ends unmatched
    assert bow["histogram_off"][2] == n + 1 and bow["histogram_off"][1][first] == x


# ---------------------------------------------------------------- SearchBySim3
@pytest.fixture(scope="module")
def sim3():
    points, bad, cases, S = C.sim3_cases()
    out = {}
    for c in cases:
        tr = {}
        m, n = C.sim3_reference(c, points, bad, tr)
        out[c["name"]] = (c, m, n, tr)
    return out, S, points, bad


def test_sim3_real_pair_finds_more_than_was_put_in(sim3):
    out, _, _, _ = sim3
    c, m, n, tr = out["real_ground_truth"]
    n_in = int((c["match12"] >= 0).sum())
    assert n_in >= 20 and n > n_in and tr["disagree"] > 0
    assert (m[c["match12"] >= 0] == c["match12"][c["match12"] >= 0]).all()       # what came in is kept
    assert int((m >= 0).sum()) == n_in + n
    assert out["real_scale_1p01"][0]["s12"] != 1 and out["real_scale_1p01"][2] > 0
    assert out["real_already2_override"][2] != n
    sizes = {(len(out[k][0]["kf1"]["kun"]), len(out[k][0]["kf2"]["kun"])) for k in out if k.startswith("real_cut")}
    assert sizes == {(0, G + 1), (1, G), (G - 1, 1), (G, 0), (G + 1, G - 1)}
    assert out[f"real_cut_{G + 1}_{G - 1}"][2] > 0


def test_sim3_hand_made_sites(sim3):
    out, S, points, bad = sim3
    c, m, n, tr = out["hand_edges"]
    vn1, vn2 = tr["vn1"], tr["vn2"]
    same = lambda k: S[k]  # noqa: E731  (a site's keypoint has the same index in both keyframes)
    assert m[S["agree"]] == same("agree")
    assert m[S["dist_100"]] == same("dist_100") and 100 in tr["dists"]              # 100 accepted
    assert vn1[S["dist_101"]] == -1 and 101 in tr["dists"] and m[S["dist_101"]] == -1
    assert vn1[S["back_101"]] == same("back_101") and vn2[S["back_101"]] == -1 and m[S["back_101"]] == -1
    for k in ("z_neg", "z_zero", "z_neg_zero", "u_at_max", "too_near", "too_far", "level_filter", "empty_window",
              "bad_point", "no_point_1"):
        assert vn1[S[k]] == -1 and m[S[k]] == -1, k
    st = np.bincount(tr["statuses"], minlength=7)
    assert st[LR.BEHIND] == 1 and st[LR.OUTSIDE_IMAGE] == 3 and st[LR.OUT_OF_RANGE] == 2 and st[LR.NO_CANDIDATES] >= 1
    assert m[S["near_end"]] == same("near_end") and m[S["far_end"]] == same("far_end")   # both ends are inside
    assert m[S["level_ok"]] == same("level_ok")
    assert bad[c["kf1"]["match_row"][S["bad_point"]]] == 1 and c["kf1"]["match_row"][S["no_point_1"]] == -1
    assert vn2[S["no_point_2"]] == -1 and vn1[S["no_point_2"]] == same("no_point_2") and m[S["no_point_2"]] == -1
    assert m[S["already"]] == c["match12"][S["already"]] == same("already") and vn1[S["already"]] == -1
    assert vn2[S["already"]] == -1                                                     # blocked through match12
    assert vn1[S["dis_a"]] == S["dis_b"] and vn2[S["dis_b"]] == S["dis_b"] and m[S["dis_a"]] == -1
    assert tr["disagree"] >= 2 and n == 5
    # u one float inside the half-open bound goes on to the search
    p_in = points[c["kf1"]["match_row"][S["u_inside"]]]
    assert LR.project(C.geo(), [_f(v) for v in p_in["xw"]])[0] == LR.SEARCHED
    # the override: the blocked idx2 is the one the array names, not the one match12 names
    c2, m2, n2, tr2 = out["hand_edges_already2_override"]
    assert m2[S["agree"]] == -1 and tr2["vn2"][S["already"]] == S["already"] and n2 == n - 1
    # a pure scale changes the distances and with them ranges and levels
    assert out["hand_edges_scale_2"][2] != n
    assert out["hand_edges_scale_1_ulp"][0]["s12"] > 1


# ---------------------------------------------------------------- SearchByProjection(pKF, Scw), Fuse(pKF, Scw)
@pytest.fixture(scope="module")
def scw():
    kfs, proj, fuse = C.scw_cases()
    P, F = {}, {}
    for p in proj:
        tr = {}
        m, n = C.proj_reference(p, kfs, tr)
        P[p["name"]] = (p, m, n, tr)
    for p in fuse:
        trs = []
        r, n = C.fuse_reference(p, kfs, trs)
        F[p["name"]] = (p, r, n, trs)
    return kfs, P, F


def test_projection_real_problem_closes_the_loop(scw):
    kfs, P, _ = scw
    p, m, n, tr = P["real"]
    assert n > 40 and n == int((m >= 0).sum())                          # LoopClosing.cc:405
    p, m, n, tr = P["real_skip_taken"]
    assert n > 40 and (m[p["taken"] != 0] == -1).all() and not np.isin(np.flatnonzero(p["skip"]), m).any()
    assert {len(P[f"real_n{k}"][0]["P"]) for k in (0, 1, G - 1, G, G + 1)} == {0, 1, G - 1, G, G + 1}
    assert P[f"real_n{G + 1}"][2] > 0 and P["keyframe_without_keypoints"][2] == 0
    # Scw with a scale: 1, 1 up to a few ulp, 2
    s_ulp = LR.decompose_scw(P["real_scale_ulp"][0]["Scw"])[1]
    assert _f(1) < s_ulp < _f(1.000001) and LR.decompose_scw(P["real_scale_2"][0]["Scw"])[1] == 2
    T_ulp, T_1 = LR.decompose_scw(P["real_scale_ulp"][0]["Scw"])[0], LR.decompose_scw(P["real"][0]["Scw"])[0]
    assert P["real_scale_ulp"][0]["Scw"].tobytes() != P["real"][0]["Scw"].tobytes() and np.allclose(T_ulp, T_1, atol=1e-6)
    assert P["real_scale_ulp"][2] > 40 and P["real_scale_2"][2] > 40


def test_projection_contenders_walk_past_the_kept_keys(scw):
    kfs, P, _ = scw
    for n in (K + 1, 2 * K):
        p, m, nm, tr = P[f"contenders_{n}"]
        assert len(kfs[p["kf"]]["kun"]) == n == nm and sorted(m.tolist()) == list(range(n))
        assert tr["rank"] == list(range(n)) and max(tr["rank"]) >= K    # each takes the next one; past K: a re-scan
        p, m, nm, tr = P[f"contenders_{n}_plus_1"]
        assert nm == n and n not in m                                   # the one too many finds nothing
    p, m, nm, tr = P["keys_taken_last_above_th"]
    assert nm == K and (m[:K] >= 0).all() and m[K] == -1
    p, m, nm, tr = P["ties_all_zero"]
    assert max(tr["rank"]) > K and nm > 100                             # equal descriptors on the real keyframe
    p, m, nm, tr = P["small"]
    assert m.tolist() == [0, 1, 2, -1] and nm == 3                      # 50 accepted, 51 refused, the fifth finds none
    assert P["small_taken"][1].tolist() == [-1, 0, 2, -1]
    assert P["small_skip"][1].tolist() == [1, 4, 2, -1]
    assert P["small_all_taken"][2] == 0
    for tag in ("1", "2", "ulp"):
        p, m, nm, tr = P[f"statuses_scale_{tag}"]
        assert tr["statuses"] == [2, 3, 3, 3, 3, 0, 4, 4, 0, 5, 0, 0] and nm == 1
        eq, below = tr["views"][8], tr["views"][9]
        assert eq[0] == eq[1] and below[0] < below[1]                   # the view-angle test at equality, and below
    assert P["clipped_th4"][2] > 0 and P["clipped_th30"][2] > 0


def test_fuse_sim3_cases_reach_their_branches(scw):
    kfs, _, F = scw
    for tag in ("1", "2", "ulp"):
        p, r, n, _ = F[f"statuses_scale_{tag}"]
        assert r["status"].tolist() == [2, 3, 3, 3, 3, 6, 4, 4, 6, 5, 6, 0] and n == 1
    # what the other Fuse's chi-square test refuses, this one takes; uright is not looked at
    fkfs, fproblems = FC.build()
    for name in ("chi2_stereo_second_wins", "chi2_mono_second_wins"):
        p, r, n, _ = F[name]
        other = FC.reference(next(q for q in fproblems if q["name"] == name), fkfs, FC.geo())[0]
        assert other[0]["best_idx"] == 1 and r[0]["best_idx"] == 0 and r[0]["best_dist"] == 1 and n == 1
    p, r, n, _ = F["uright_zero_is_stereo"]
    other = FC.reference(next(q for q in fproblems if q["name"] == "uright_zero_is_stereo"), fkfs, FC.geo())[0]
    assert other[0]["best_idx"] == -1 and r[0]["best_idx"] == 0 and n == 1
    p, r, n, _ = F["levels"]
    assert r[0]["best_dist"] == 25
    p, r, n, trs = F["ties_all_zero"]
    assert sum(t.get("n_cand", 0) > 1 for t in trs) > 100 and (r["best_dist"][r["best_idx"] >= 0] == 0).all()
    first = [t["cand"][0] for t, q in zip(trs, r) if q["status"] == 0 and t.get("cand")]
    assert any(q["best_idx"] != f for q, f in zip(r[r["status"] == 0], first))      # the octave filter skips some
    assert {F[f"clipped_th{t}"][0]["th"] for t in (4, 30)} == {4.0, 30.0}
    assert max(t.get("n_cand", 0) for t in F["real_th30"][3]) > 20
    for k in (0, 1, G - 1, G, G + 1):
        assert len(F[f"real_n{k}"][0]["P"]) == k
    assert F["real"][2] > 100 and F["real_scale_ulp"][2] > 100 and F["real_scale_2"][2] > 20
    p, r, n, _ = F["small_50_51"]
    assert r["best_dist"].tolist() == [1, 1, 50, 51, 1] and n == 4     # Fuse does not block: both take keypoint 0


def _model():
    """A map around the real problem: keyframe 9 is pKF (frame 16).  The list holds keyframe 1's points, then a
    second map point at the place of every fifth fused one (two listed points on one keypoint), then points that
    are bad or already in pKF.  pKF already holds points on some of the keypoints the search will choose: good
    ones and a bad one."""
    kfs_c, proj, fuse = C.scw_cases()
    p = next(q for q in fuse if q["name"] == "real")
    kf = kfs_c[p["kf"]]
    P0 = p["P"][:400]
    snap, _ = LR.fuse_sim3_snapshot(p["Scw"], P0, kf["kun"], kf["desc"], kf["go"], kf["gi"], C.geo())
    fused = np.flatnonzero(snap["best_dist"] <= LR.TH_LOW)
    assert len(fused) > 100
    kfs = {0: dict(points={}, desc=np.zeros((2000, 32), np.uint8), ur=np.full(2000, -1.0, np.float32), bad=False),
           9: dict(points={}, desc=kf["desc"], ur=kf["ur"], bad=False)}
    points, pids = {}, []

    def new_point(pid, rec, in_kf=None, bad=False):
        points[pid] = dict(rec=rec.copy(), obs={}, nobs=0, bad=False)
        idx = len(kfs[0]["points"])
        kfs[0]["points"][idx] = pid
        FR.add_observation(points, kfs, pid, 0, idx)
        if in_kf is not None:
            kfs[9]["points"][in_kf] = pid
            FR.add_observation(points, kfs, pid, 9, in_kf)
        points[pid]["bad"] = bad

    for i in range(len(P0)):
        new_point(i, P0[i])
        pids.append(i)
    for n, i in enumerate(fused[::5]):                    # a second listed point on the same keypoint
        new_point(1000 + n, P0[i])
        pids.append(1000 + n)
    held = {}
    for n, i in enumerate(fused[1::5]):                   # pKF's keypoint already holds a point: good, or bad
        idx = int(snap[i]["best_idx"])
        if idx in kfs[9]["points"]:
            continue
        new_point(2000 + n, P0[i], in_kf=idx, bad=n % 3 == 0)
        held[i] = 2000 + n
    listed_in_kf = [pid for pid in list(held.values())[:5] if not points[pid]["bad"]]
    pids += listed_in_kf                                  # already found in pKF: skipped
    new_point(3000, P0[0], bad=True)
    pids.append(3000)                                     # bad: skipped
    return p, kf, points, kfs, pids, held, fused


def test_whole_fuse_sim3_call_sees_the_snapshot_search_and_counts_its_fuses():
    p, kf, points, kfs, pids, held, fused = _model()
    skip = np.array([points[pid]["bad"] or 9 in points[pid]["obs"] for pid in pids], np.uint8)
    P = FC.stack([points[pid]["rec"] for pid in pids])
    snap, n_snap = LR.fuse_sim3_snapshot(p["Scw"], P, kf["kun"], kf["desc"], kf["go"], kf["gi"], C.geo(), skip=skip)
    n_fused, seen, replace, actions = LR.fuse_sim3(points, kfs, 9, p["Scw"], pids, kf["kun"], kf["go"], kf["gi"],
                                                   C.geo())
    assert skip.sum() >= 4 and n_fused == n_snap > 100
    for i, rec in enumerate(seen):
        if rec is None:
            assert snap[i]["status"] == LR.SKIPPED
        else:
            assert (snap[i]["status"], snap[i]["level"], snap[i]["best_idx"], snap[i]["best_dist"]) == rec, i
    kinds = [a[0] for a in actions]
    assert kinds.count("added") > 50 and kinds.count("replace") > 20 and kinds.count("kf_point_bad") >= 3
    # two listed points on one keypoint: the first is added, the second gets it as vpReplacePoint
    added = {a[2]: a[1] for a in actions if a[0] == "added"}
    twice = [(a[1], a[2]) for a in actions if a[0] == "replace" and a[2] in added.values()]
    assert len(twice) > 10 and all(replace[pids.index(pid)] == by for pid, by in twice)
    # a keypoint already holding a good point gives vpReplacePoint, a bad one is counted with nothing done
    assert any(a[0] == "replace" and a[2] in held.values() for a in actions)
    assert all(replace[pids.index(a[1])] is None for a in actions if a[0] == "kf_point_bad")
    assert sum(r is not None for r in replace) == kinds.count("replace")


# ---------------------------------------------------------------- the float expressions against the compiler
PROBE = r"""
extern "C" void loop_probe(float fx, float fy, float cx, float cy, float X, float Y, float z, float* out) {
    {   // SearchByProjection(pKF, Scw): ORBmatcher.cc:331-336
        const float invz = 1/z;
        const float x = X*invz;
        const float y = Y*invz;
        const float u = fx*x+cx;
        const float v = fy*y+cy;
        out[0] = invz; out[1] = u; out[2] = v;
    }
    {   // Fuse(pKF, Scw) and SearchBySim3: :1019-1024, :1166-1171
        const float invz = 1.0/z;
        const float x = X*invz;
        const float y = Y*invz;
        const float u = fx*x+cx;
        const float v = fy*y+cy;
        out[3] = invz; out[4] = u; out[5] = v;
    }
}
"""


def test_loop_expressions_match_gcc_march_native(tmp_path):
    if "fma" not in pathlib.Path("/proc/cpuinfo").read_text():
        pytest.skip("host CPU without FMA: -march=native does not contract")
    import synth
    Kc = synth.TUM3
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE)
    so = tmp_path / "probe.so"
    subprocess.run(["g++", "-O3", "-march=native", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    L = ctypes.CDLL(str(so))
    f = ctypes.c_float
    L.loop_probe.argtypes = [f] * 7 + [ctypes.c_void_p]
    geo = [_f(Kc[k]) for k in ("fx", "fy", "cx", "cy", "bf")]
    rng = np.random.default_rng(12)
    out = np.zeros(6, np.float32)
    for it in range(3000):
        X, Y = rng.normal(size=2).astype(np.float32)
        z = _f(rng.uniform(0.05, 8.0)) if it % 10 else _f(np.float32(2.0) ** rng.integers(-3, 3))
        invz, u, v, _ = FR.projection(geo, X, Y, z)
        L.loop_probe(*geo[:4], X, Y, z, out.ctypes.data)
        assert (out[0], out[1], out[2]) == (invz, u, v), it            # 1/z in float
        assert (out[3], out[4], out[5]) == (invz, u, v), it            # 1.0/z in double, rounded: the same bits
