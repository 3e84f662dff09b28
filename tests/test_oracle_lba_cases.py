"""What each case of tests/lba_cases.py reaches, shown without the device: a plain restatement of the branch
conditions of structure() and of k_lba_g2o's factor dispatch (sp-slam_amd/csrc/lbg_structure.h, lba_g2o.hip) over the
case's arrays -- free poses, coupling pattern, pose degrees, class (fully dense / all-dense-not-full / AMD), AMD
workspace size, Schur chunk sizes -- with the kernel's size constants as named conditions, Eigen's AMD order itself
from the oracle's SimplicialLDLT restatement, and the oracle's run of the case (status, and the second-pass outcome a
case was built for).  Every case prints one line naming what it reached."""
import numpy as np
import pytest

import lba_cases as C

FAST = [n for n in C.NAMES if n not in C.SLOW]


def landmarks(P):
    """Per landmark in vertex-id order (points by id, then planes by id; stable): the keyframes of its edges."""
    prob, kfs, pts, pobs, pls, plobs, _ = P
    out = []
    for rows, obs in ((pts, pobs), (pls, plobs)):
        order = sorted(range(len(rows)), key=lambda i: (int(rows[i]["id"]), i))
        out += [obs["kf"][rows[i]["obs_offset"]:rows[i]["obs_offset"] + rows[i]["n_obs"]] for i in order]
    return out


def classify(P):
    prob, kfs, pts, pobs, pls, plobs, _ = P
    K = len(kfs)
    lms = landmarks(P)
    seen = set(int(k) for ks in lms for k in ks)
    free = [k for k in range(K) if k in seen and not kfs[k]["fixed"] and kfs[k]["id"] != 0]
    rank = {k: j for j, k in enumerate(free)}                                       # list order
    hidx = {k: j for j, k in enumerate(sorted(free, key=lambda k: int(kfs[k]["id"])))}  # Hessian (id) order
    n_free = len(free)
    pat_h, pat_l = np.eye(n_free, dtype=bool), np.eye(n_free, dtype=bool)
    blocks = []
    for ks in lms:
        hs = sorted({hidx[int(k)] for k in ks if int(k) in hidx})
        ls = sorted({rank[int(k)] for k in ks if int(k) in rank})
        pat_h[np.ix_(hs, hs)] = True
        pat_l[np.ix_(ls, ls)] = True
        if len(ks):
            blocks.append(len(hs))
    n = 6 * n_free
    pdeg = pat_h.sum(1)
    dense = C.dense_threshold(n) if n else 0
    alld = bool((6 * pdeg > dense).all())
    full = bool(pat_h.all())
    cls = "none" if n == 0 else "dense" if alld and full else "alld" if alld else "amd"
    cnz = 36 * int(pdeg.sum())
    tcap = cnz + cnz // 5 + 2 * n
    amd_bytes = (tcap + 10 * (n + 1)) * 4
    pw = 1 if K <= C.K_MAX_FREE else 2
    lds = n <= C.K_LDS_N[pw]
    if n == 0:
        branch = "no reduced system"
    elif lds and cls == "dense":
        branch = f"factor_dense<{1 if n <= 64 else 2}>"
    elif cls == "dense" and n <= C.K_PACK_N:
        branch = "factor_dense_packed"
    else:
        regs = 1 if n <= 64 else 2 if n <= 128 else 3 if n <= 192 else 4 if n <= 256 else \
            6 if (pw == 1 or n <= 384) else 8 if n <= 512 else 12
        branch = f"factor_solve<{regs},{'true' if lds else 'false'}>"
    groups = [sum(blocks[g:g + C.K_SCHUR_LM]) for g in range(0, len(blocks), C.K_SCHUR_LM)]
    return dict(np=n_free, n=n, pat=pat_h, pat_list=pat_l, pdeg=pdeg, cls=cls, amd_bytes=amd_bytes,
                amd_global=cls == "amd" and amd_bytes > C.K_DYN, pw=pw, branch=branch, n_landmarks=len(blocks),
                n_edges=int(prob["n_point_obs"] + prob["n_plane_obs"]), groups=groups,
                natural=cls in ("dense", "alld"), pdeg_sum=int(pdeg.sum()))


def amd_perm(pat):
    import oracle_lba
    n = 6 * len(pat)
    S = np.kron(pat, np.ones((6, 6), bool))
    A = np.where(S, 0.01, 0.0) + n * np.eye(n)
    x, perm = oracle_lba.eigen_ldlt(np.triu(S), A, np.zeros(n))
    assert x is not None and sorted(perm) == list(range(n))
    return perm


@pytest.mark.parametrize("name", FAST)
def test_case_reaches_what_it_was_built_for(name):
    c = C.case(name)
    P, want = c["P"], c["want"]
    k = classify(P)
    print(f"\n{name}: free poses {k['np']} (n = {k['n']}), instance pw{k['pw']}, class {k['cls']}, {k['branch']}, "
          f"pose degrees {k['pdeg'].min() if k['np'] else 0}..{k['pdeg'].max() if k['np'] else 0}, "
          f"AMD workspace {k['amd_bytes']} B ({'global memory' if k['amd_global'] else 'LDS'}: kDyn = {C.K_DYN}), "
          f"{k['n_landmarks']} landmarks, {k['n_edges']} edges, Schur group blocks {k['groups'][:3]}")
    assert k["np"] == want["np"] and k["cls"] == want["cls"] and k["pw"] == want["pw"], (k["np"], k["cls"], k["pw"])
    if "pattern" in want:
        assert np.array_equal(k["pat_list"], C.expected_pattern(want["pattern"], k["np"]))
    if want["cls"] == "alld":
        assert not k["pat"][0, -1] and k["natural"] and (6 * k["pdeg"] > C.dense_threshold(k["n"])).all()
    if want.get("amd_global"):
        assert k["amd_global"] and k["pdeg_sum"] >= 800 and (6 * k["pdeg"] <= C.dense_threshold(k["n"])).any()
    if "landmarks" in want:
        assert k["n_landmarks"] == want["landmarks"]
    if "edges" in want:
        assert k["n_edges"] == want["edges"]
    if "schur_blocks" in want:  # one side of kSchurBlk each: a group at the limit is one chunk, one past it is split
        assert k["groups"][0] == want["schur_blocks"] and len(k["groups"]) == 2
        assert (k["groups"][0] > C.K_SCHUR_BLK[k["pw"]]) == (want["schur_blocks"] > C.K_SCHUR_BLK[k["pw"]])
    # Eigen's order: the identity exactly where the class says natural
    if k["n"]:
        perm = amd_perm(k["pat"])
        ident = list(perm) == list(range(k["n"]))
        assert ident == k["natural"], (name, k["cls"])
        if not ident:
            print(f"{name}: AMD order is not the identity at n = {k['n']}")


SEAMS = {  # what the list must reach, by the restated dispatch
    "free10-band(2)": "factor_solve<1,true>", "free11-band(2)": "factor_solve<2,true>",
    "free16-band(3)+hub": "factor_solve<2,true>", "free17-band(3)+hub": "factor_solve<2,false>",
    "free21-band(2)": "factor_solve<2,false>", "free22-band(2)": "factor_solve<3,false>",
    "free32-band(2)": "factor_solve<3,false>", "free33-band(2)": "factor_solve<4,false>",
    "free42-band(2)": "factor_solve<4,false>", "free43-band(2)": "factor_solve<6,false>",
    "free64-band(3)+hub": "factor_solve<6,false>", "wide65-two": "factor_solve<8,false>",
    "wide85-two": "factor_solve<8,false>", "wide86-two": "factor_solve<12,false>",
    "wide128-band(3)+hub": "factor_solve<12,false>", "wide66-free15-band(2)": "factor_solve<2,true>",
    "wide66-free16-band(2)": "factor_solve<2,false>", "wide66-free15-full": "factor_dense<2>",
    "wide66-free16-full": "factor_dense_packed", "free16-full": "factor_dense<2>", "free17-full": "factor_dense_packed",
    "free30-full": "factor_dense_packed", "free31-full": "factor_solve<3,false>", "free10-full": "factor_dense<1>",
    "free11-full": "factor_dense<2>", "free25-alld": "factor_solve<3,false>", "free62-alld": "factor_solve<6,false>",
    "wide120-band(8)-amd-global": "factor_solve<12,false>",
}


def test_dispatch_seams_are_reached():
    for name, branch in SEAMS.items():
        assert classify(C.case(name)["P"])["branch"] == branch, name


def _chi2(P, o):
    """Point-edge chi2 at the oracle's result, in float64."""
    prob, kfs, pts, pobs, pls, plobs, _ = P
    lm = np.repeat(np.arange(len(pts)), pts["n_obs"])
    T = o["Tcw"].astype(np.float64).reshape(-1, 4, 4)[pobs["kf"]]
    Xc = np.einsum("nij,nj->ni", T[:, :3, :3], o["points"].astype(np.float64)[lm]) + T[:, :3, 3]
    kf = kfs[pobs["kf"]]
    u = kf["fx"] * Xc[:, 0] / Xc[:, 2] + kf["cx"]
    v = kf["fy"] * Xc[:, 1] / Xc[:, 2] + kf["cy"]
    st = pobs["ur"] >= 0
    e2 = (u - pobs["u"]) ** 2 + (v - pobs["v"]) ** 2 + np.where(st, (u - kf["bf"] / Xc[:, 2] - pobs["ur"]) ** 2, 0.0)
    return e2 * pobs["inv_sigma2"] / np.where(st, 7.815, 5.991)


@pytest.mark.parametrize("name", FAST)
def test_oracle_runs_case_as_tagged(name):
    c = C.case(name)
    P, want = c["P"], c["want"]
    prob, kfs, pts, pobs, pls, plobs, _ = P
    o = C.oracle(name)
    r = o["result"]
    assert r["status"] == 0 and r["stopped"] == 0
    fixed = (kfs["fixed"] == 1) | (kfs["id"] == 0)
    assert np.array_equal(o["Tcw"][fixed], kfs["Tcw"][fixed])
    seen_by = lambda i: list(pobs["kf"][pts[i]["obs_offset"]:][:pts[i]["n_obs"]])  # noqa: E731
    if want.get("all_outliers"):
        assert r["iterations"][0] > 0 and r["iterations"][1] == 0 and o["point_outlier"].all()
    elif want["np"] == 0:  # the landmarks alone move; every pose goes back as it came
        assert np.array_equal(o["Tcw"], kfs["Tcw"]) and r["iterations"][0] > 0
        assert not np.array_equal(o["points"], pts["xw"])
    else:
        assert r["iterations"][0] > 0 and r["iterations"][1] > 0 and r["trials"] >= 2
        free = ~fixed
        if "unobserved" in want:
            free[want["unobserved"]] = False
            assert np.abs(o["Tcw"][want["unobserved"]] - kfs["Tcw"][want["unobserved"]]).max() < 1e-6
        assert (np.abs(o["Tcw"][free] - kfs["Tcw"][free]).max(1) > 0).all()  # every free pose with an edge moved
    if "bridge" in want:
        i, k = want["bridge"]
        flags = o["point_outlier"][pts[i]["obs_offset"]:][:pts[i]["n_obs"]]
        assert list(flags) == [0, 0, 1], flags
        others = [j for j in range(len(pts)) if j != i and {8, 9} <= set(seen_by(j))]
        assert not others and o["point_outlier"][int(pts[i]["obs_offset"]) + seen_by(i).index(k)] == 1
    if "dead_pose" in want:
        mine = pobs["kf"] == want["dead_pose"]
        assert mine.sum() >= 20 and o["point_outlier"][mine].all()
        assert o["point_outlier"][~mine].sum() < 0.1 * (~mine).sum()
    if want.get("fast"):  # nothing flagged and no chi2 near its threshold: the fast order takes the same decisions
        assert not o["point_outlier"].any() and not o["plane_outlier"].any()
        assert _chi2(P, o).max() < 0.5
    if want.get("lonely"):
        n = want["lonely"]
        assert not np.array_equal(o["points"][-n:], pts["xw"][-n:])


def test_rank_tile_case():
    """The 34,817-point case: one id more than a tile of setup()'s rank counting, ids out of order (the sorted
    shortcut is not taken); the oracle's time for it is printed."""
    import time
    c = C.case("rank-tiles-34817")
    prob, kfs, pts, pobs, pls, plobs, _ = c["P"]
    assert len(pts) == C.K_TILE + 1 and (np.diff(pts["id"]) < 0).any() and (np.diff(kfs["id"]) < 0).any()
    assert len(pobs) == 2 * len(pts) and (pobs["ur"] >= 0).all() and classify(c["P"])["np"] == 2
    t0 = time.perf_counter()
    o = C.oracle("rank-tiles-34817")
    print(f"\nrank-tiles-34817: oracle {time.perf_counter() - t0:.2f} s")
    assert o["result"]["status"] == 0 and o["result"]["iterations"][1] > 0
