"""The cases of the loop-closing matcher tests (tests/test_loop_match_host.py guards what each reaches,
tests/test_gpu_loop_match.py runs them on the device): two keyframes of a synthetic sequence four frames apart with
the ground-truth relative pose and map points from the depth, and hand-made keyframes of a few keypoints with
Tcw / Scw = identity or a pure scale, as tests/fuse_cases.py builds them.

  bow_cases()      SearchByBoW(KF, KF): dict(name, kf1, kf2, nn_ratio, check_ori); a keyframe is dict(desc, keys_un,
                   has_point, fv = dict(nodes, start, features))
  sim3_cases()     SearchBySim3: (points, point_bad, cases); a case is dict(name, kf1, kf2, s12, R12, t12, match12,
                   already2 or None, th); a keyframe is dict(Tcw, kun, desc, go, gi, match_row)
  scw_cases()      SearchByProjection(pKF, Scw) and Fuse(pKF, Scw): (keyframes, projection problems, fuse problems);
                   a problem is dict(name, Scw, P, kf, th, skip or None) plus taken or None for the projection
"""
import functools

import numpy as np

import fuse_cases as FC
import loop_match_ref as LR
from matcher_ref import f32 as _f

# the kernels' grouping constants (sp-slam_amd/spslam_loop.py states the same)
PTS_PER_GROUP = 64   # points per workgroup of the three projection searches (256 threads, 4 lanes per point)
PROJ_KEYS = 4        # keys kept per point by SearchByProjection(pKF, Scw)'s window kernel
BOW_WAVES = 4        # waves per workgroup of the SearchByBoW kernel
EYE = FC.EYE
bits = FC.bits


# ---------------------------------------------------------------- the real pair
@functools.lru_cache(maxsize=None)
def real_pair():
    """Frames 12 and 16 of synthetic sequence 0 as keyframes 1 and 2 of a small map.  Returns (geo, [kf1, kf2],
    points, T12 as a 4x4 double): a keyframe is dict(Tcw, kun, desc, ur, go, gi, match_row, fv); the map points of
    keyframe k are rows of `points`, made from its keypoints and the depth as synth.local_problem makes them."""
    import oracle_bow
    import spslam_match
    import synth
    import bow_common as BC
    from test_oracle_match import make_pairs
    K = synth.TUM3
    qs = [FC.real_problems()[0], make_pairs(((0, 10, 16),), seed=18)[0]]
    assert qs[0]["c"] == 12 and qs[1]["c"] == 16
    voc = oracle_bow.Vocabulary(BC.vocab_text())
    rng = np.random.default_rng(41)
    sf = np.float32(1.2) ** np.arange(8, dtype=np.float32)
    kfs, rows = [], []
    for q in qs:
        sc, c = q["sc"], q["c"]
        depth = sc.render(sc.pose(c), noise_seed=c)[1]
        Twc = sc.pose(c)
        match_row = np.full(len(q["kun"]), -1, np.int32)
        for i, kp in enumerate(q["kun"]):
            x, y = int(kp["x"]), int(kp["y"])
            if rng.uniform() > 0.85 or not (0 <= x < 640 and 0 <= y < 480):
                continue
            z = float(depth[y, x]) / K["depth_factor"]
            if z <= 0:
                continue
            Xw = (Twc @ np.array([(kp["x"] - K["cx"]) * z / K["fx"], (kp["y"] - K["cy"]) * z / K["fy"], z, 1.0]))[:3]
            PC = Xw - Twc[:3, 3]
            dist = np.linalg.norm(PC)
            maxd = np.float32(dist) * sf[int(kp["octave"])]
            b = np.unpackbits(np.array(q["desc"][i], np.uint8))
            b[rng.choice(256, size=4, replace=False)] ^= 1
            p = np.zeros((), spslam_match.LOCAL_POINT_DTYPE)
            p["xw"], p["normal"], p["min_dist"], p["max_dist"], p["id"] = Xw, PC / dist, maxd / sf[-1], maxd, len(rows)
            p["desc"] = np.packbits(b)
            match_row[i] = len(rows)
            rows.append(p)
        fv = voc.transform(q["desc"])
        kfs.append(dict(Tcw=np.linalg.inv(Twc).astype(np.float32).reshape(16), kun=q["kun"], desc=q["desc"],
                        ur=q["ur"], go=q["go"], gi=q["gi"], match_row=match_row,
                        fv={k: np.asarray(fv[k]) for k in ("nodes", "start", "features")}))
    T12 = np.linalg.inv(qs[0]["sc"].pose(12)) @ qs[1]["sc"].pose(16)
    return qs[0]["geo"], kfs, np.array(rows, spslam_match.LOCAL_POINT_DTYPE), T12


def geo():
    return FC.geo()


def cut_keyframe(kf, n):
    """The keyframe's first n keypoints, its grid rebuilt over them."""
    keep = kf["gi"] < n
    cell = np.repeat(np.arange(64 * 48), np.diff(kf["go"]))
    go = np.zeros(64 * 48 + 1, np.int32)
    go[1:] = np.cumsum(np.bincount(cell[keep], minlength=64 * 48))
    out = dict(kf, kun=kf["kun"][:n], desc=kf["desc"][:n], go=go, gi=kf["gi"][keep].astype(np.int32))
    for k in ("ur", "match_row"):
        if k in kf:
            out[k] = kf[k][:n]
    return out


# ---------------------------------------------------------------- SearchByBoW(KF, KF)
def bow_keyframe(nodes, reverse_index=False):
    """nodes: [(node id, [(descriptor, angle, has_point)])] in ascending node order.  Keypoints are numbered in
    list order, or from the last one down (list order is then not index order)."""
    import spslam_gpu
    n = sum(len(f) for _, f in nodes)
    desc, keys = np.zeros((n, 32), np.uint8), np.zeros(n, spslam_gpu.KEYPOINT_DTYPE)
    has = np.zeros(n, np.uint8)
    start, feats, q = [0], [], 0
    for _, fl in nodes:
        for d, a, h in fl:
            i = n - 1 - q if reverse_index else q
            desc[i], keys[i]["angle"], has[i] = d, a, h
            feats.append(i)
            q += 1
        start.append(q)
    return dict(desc=desc, keys_un=keys, has_point=has,
                fv=dict(nodes=np.array([i for i, _ in nodes], np.uint32), start=np.array(start, np.int32),
                        features=np.array(feats, np.int32)))


def real_bow_keyframe(kf):
    return dict(desc=kf["desc"], keys_un=kf["kun"], has_point=(kf["match_row"] >= 0).astype(np.uint8), fv=kf["fv"])


@functools.lru_cache(maxsize=None)
def bow_cases():
    _, kfs, _, _ = real_pair()
    r1, r2 = real_bow_keyframe(kfs[0]), real_bow_keyframe(kfs[1])
    cases = []

    def add(name, kf1, kf2, nn_ratio=0.75, check_ori=True):
        cases.append(dict(name=name, kf1=kf1, kf2=kf2, nn_ratio=nn_ratio, check_ori=check_ori))

    # ---- the real pair, both ways, with LoopClosing's matcher (0.75, orientation checked) and without the check
    add("real_12_16", r1, r2)
    add("real_16_12", r2, r1)
    add("real_12_16_no_orientation", r1, r2, check_ori=False)
    rng = np.random.default_rng(5)
    thin = lambda k, f: dict(k, has_point=(k["has_point"] & (rng.uniform(size=len(k["has_point"])) < f)).astype(np.uint8))  # noqa: E731
    add("real_has_point_cleared_on_1", thin(r1, 0.5), r2)
    add("real_has_point_cleared_on_2", r1, thin(r2, 0.5))
    add("real_12_12", r1, r1)                                        # every node shared, every distance 0

    Z = np.zeros(32, np.uint8)
    one = lambda d, a=0.0, h=1: (d, a, h)  # noqa: E731

    # ---- KF2 node lists of 0, 1, 63, 64 and 65 features: the 64-lane strided scan.  The wanted keypoint is the
    # list's last, so a scan that stops at 64 misses it
    n1, n2 = [], []
    for node, m in enumerate((0, 1, 63, 64, 65)):
        n1.append((node, [one(Z), one(bits(2))]))
        n2.append((node, [one(bits(60 + (j % 7))) for j in range(m - 1)] + ([one(bits(1))] if m else [])))
    add("node_lists_0_1_63_64_65", bow_keyframe(n1), bow_keyframe(n2))

    # ---- 0, 1, W and W + 1 shared nodes; no shared node at all
    for shared in (0, 1, BOW_WAVES, BOW_WAVES + 1):
        a = [(2 * k, [one(Z, 10.0 * k)]) for k in range(6)]                       # nodes 0, 2, 4, 6, 8, 10
        b = [(2 * k if k < shared else 2 * k + 1, [one(bits(3), 5.0 * k), one(bits(40))]) for k in range(6)]
        add(f"shared_nodes_{shared}", bow_keyframe(a), bow_keyframe(b), check_ori=False)
    add("empty_feature_vectors", bow_keyframe([]), bow_keyframe([]))
    add("kf2_without_keypoints", bow_keyframe([(3, [one(Z)])]), bow_keyframe([]))

    # ---- two idx1 of one node want the same idx2: the second takes its runner-up, and its ratio test sees a changed
    # second best (unblocked: 1 then 28, refused; blocked: 28 then 43, accepted)
    add("same_idx2_wanted_twice", bow_keyframe([(7, [one(Z), one(bits(2))])]),
        bow_keyframe([(7, [one(bits(1)), one(bits(30)), one(bits(45))])]), check_ori=False)
    # ... with KF1's indices against list order: list order decides who gets it
    add("same_idx2_list_order", bow_keyframe([(7, [one(Z), one(bits(2))])], reverse_index=True),
        bow_keyframe([(7, [one(bits(1)), one(bits(30)), one(bits(45))])], reverse_index=True), check_ori=False)

    # ---- TH_LOW is strict here: 49 accepted, 50 refused (the keyframe-to-frame overload accepts 50)
    add("distance_49_and_50", bow_keyframe([(1, [one(Z)]), (2, [one(Z)])]),
        bow_keyframe([(1, [one(bits(49)), one(bits(200))]), (2, [one(bits(50)), one(bits(200))])]), check_ori=False)
    # ---- the ratio test on either side of equality: 0.75 * 40 = 30
    add("ratio_29_30_31", bow_keyframe([(k, [one(Z)]) for k in (1, 2, 3)]),
        bow_keyframe([(k, [one(bits(40)), one(bits(b))]) for k, b in ((1, 29), (2, 30), (3, 31))]), check_ori=False)
    # ---- has_point cleared on either side
    add("has_point_either_side", bow_keyframe([(1, [one(Z, h=0), one(Z)]), (2, [one(Z)])]),
        bow_keyframe([(1, [one(bits(1)), one(bits(90))]), (2, [one(bits(1), h=0), one(bits(5)), one(bits(90))])]),
        check_ori=False)
    # ---- equal distances: the first in list order wins, and the ratio test fails on a tie of the two best
    add("equal_distances", bow_keyframe([(1, [one(Z)]), (2, [one(Z)])]),
        bow_keyframe([(1, [one(bits(4)), one(bits(4))]),
                      (2, [one(bits(70)), one(bits(4)), one(bits(80)), one(bits(4) ^ bits(8))])],
                     reverse_index=True), nn_ratio=1.5, check_ori=False)
    # ---- the rotation histogram: bins 0 (3 matches, 4 with node 9's second), 3 (2) and 6 (2) stay, bin 9 (1) goes;
    # the match it removes is the first of its node, and the idx2 it took stays blocked for the node's second idx1,
    # which wanted it too
    nodes1, nodes2 = [], []
    for k, rot in enumerate((0.0, 0.0, 0.0, 90.0, 90.0, 180.0, 180.0)):
        nodes1.append((k, [one(Z, rot)]))
        nodes2.append((k, [one(bits(1)), one(bits(90))]))
    nodes1.append((9, [one(Z, 270.0), one(bits(2), 0.0)]))
    nodes2.append((9, [one(bits(1)), one(bits(30)), one(bits(45))]))
    add("histogram_removes_and_blocks", bow_keyframe(nodes1), bow_keyframe(nodes2))
    add("histogram_off", bow_keyframe(nodes1), bow_keyframe(nodes2), check_ori=False)
    return cases


def bow_reference(case, trace=None):
    a, b = case["kf1"], case["kf2"]
    return LR.search_by_bow_kf(a["desc"], a["keys_un"]["angle"], a["has_point"], a["fv"], b["desc"],
                               b["keys_un"]["angle"], b["has_point"], b["fv"], case["nn_ratio"], case["check_ori"],
                               trace)


# ---------------------------------------------------------------- SearchBySim3
def sim3_keyframe(kps, rows, g, Tcw=EYE):
    kf = FC.make_keyframe(kps, g)
    return dict(Tcw=np.asarray(Tcw, np.float32).reshape(16), kun=kf["kun"], desc=kf["desc"], go=kf["go"], gi=kf["gi"],
                match_row=np.array(rows, np.int32).reshape(-1))


@functools.lru_cache(maxsize=None)
def sim3_cases():
    """(points, point_bad, cases, the hand-made sites' keypoint indices by name).  The real pair's points are rows
    0 .. n_real - 1; the hand-made ones follow."""
    g, kfs, real_points, T12 = real_pair()
    hand = []                                                        # hand-made point records
    n_real = len(real_points)
    cases = []

    def row(p, d=None):
        p = p.copy()
        if d is not None:
            p["desc"] = d
        hand.append(p)
        return n_real + len(hand) - 1

    def add(name, kf1, kf2, match12=None, s12=1.0, R12=np.eye(3), t12=(0, 0, 0), already2=None, th=7.5):
        m = np.full(len(kf1["kun"]), -1, np.int32) if match12 is None else np.asarray(match12, np.int32)
        cases.append(dict(name=name, kf1=kf1, kf2=kf2, s12=np.float32(s12), R12=np.asarray(R12, np.float32),
                          t12=np.asarray(t12, np.float32), match12=m, already2=already2, th=th))

    # ---- the real pair at the ground-truth Sim3 (s12 = 1), from an initial set of matches as ComputeSim3 has it:
    # the BoW matches whose bins survive, thinned as RANSAC's inliers would
    k1, k2 = [dict(k) for k in kfs]
    R12, t12 = T12[:3, :3], T12[:3, 3]
    m0, _ = LR.search_by_bow_kf(k1["desc"], k1["kun"]["angle"], k1["match_row"] >= 0, k1["fv"], k2["desc"],
                                k2["kun"]["angle"], k2["match_row"] >= 0, k2["fv"])
    rng = np.random.default_rng(8)
    m_in = np.where(rng.uniform(size=len(m0)) < 0.6, m0, -1).astype(np.int32)
    add("real_ground_truth", k1, k2, m_in, 1.0, R12, t12)
    add("real_no_initial_matches", k1, k2, None, 1.0, R12, t12)
    add("real_scale_1p01", k1, k2, m_in, 1.01, R12, t12)
    add("real_already2_override", k1, k2, m_in, 1.0, R12, t12,
        already2=(rng.uniform(size=len(k2["kun"])) < 0.3).astype(np.uint8))
    G = PTS_PER_GROUP
    for na, nb in ((0, G + 1), (1, G), (G - 1, 1), (G, 0), (G + 1, G - 1)):
        a, b = cut_keyframe(k1, na), cut_keyframe(k2, nb)
        add(f"real_cut_{na}_{nb}", a, b, np.where(m_in[:na] < nb, m_in[:na], -1), 1.0, R12, t12)

    # ---- hand-made: both poses the identity, S12 the identity or a pure scale, so p3Dc2 = p3Dw / s12.  Sites are
    # 40 px apart; each has a keypoint in both keyframes, and each keypoint's map point projects beside it.
    pt = lambda u, v, **kw: FC.point_at(g, u, v, **kw)  # noqa: E731
    Z = np.zeros(32, np.uint8)
    kp1, kp2, rows1, rows2 = [], [], [], []

    def site(u, v, d1k=Z, p1d=Z, d2k=Z, p2d=Z, p1=None, p2=None, oct1=0, oct2=0):
        """keypoint + map point in KF1 and in KF2 at (u, v); p1 / p2 replace the point records (None: no point)."""
        kp1.append((u, v, oct1, -1.0, d1k))
        kp2.append((u, v, oct2, -1.0, d2k))
        rows1.append(-1 if p1 is False else row(pt(u + 0.3, v + 0.2) if p1 is None else p1, p1d))
        rows2.append(-1 if p2 is False else row(pt(u + 0.2, v + 0.1) if p2 is None else p2, p2d))
        return len(kp1) - 1

    head_on = np.array([0, 0, 1], np.float32)
    raw = FC.raw_point
    x_max = FC.x_with_u(g, _f(640.0))
    x_in = FC.x_with_u(g, np.nextafter(_f(640.0), _f(0.0)))
    S = {}
    S["agree"] = site(100.0, 100.0)
    S["dist_100"] = site(140.0, 100.0, d2k=bits(100))                # 100 accepted
    S["dist_101"] = site(180.0, 100.0, d2k=bits(101))                # 101 refused: vnMatch1 stays -1
    S["back_101"] = site(220.0, 100.0, p2d=bits(101))                # refused on the way back: no agreement
    S["z_neg"] = site(260.0, 100.0, p1=raw([0.1, 0.0, -1.0], head_on, 0.1, 9.0))
    S["z_zero"] = site(300.0, 100.0, p1=raw([0.1, 0.0, 0.0], head_on, 0.1, 9.0))
    S["z_neg_zero"] = site(340.0, 100.0, p1=raw([-0.1, 0.1, -0.0], head_on, 0.1, 9.0))
    S["u_at_max"] = site(380.0, 100.0, p1=raw([x_max, 0.0, 2.0], head_on, 0.1, 9.0))
    S["u_inside"] = site(637.0, 240.0, p1=raw([x_in, 0.0, 2.0], head_on, 0.1, 9.0))

    def ranged(u, v, end):
        """A point beside (u, v) whose distance is at an end of its invariance range, or one float outside it:
        0.8f * min_dist the largest float <= dist, or the next one; 1.2f * max_dist the smallest >= dist, or the
        one before (level 0 either way)."""
        p = pt(u + 0.3, v + 0.2)
        d = LR.norm3([_f(c) for c in p["xw"]])
        f, key, up = (_f(0.8), "min_dist", True) if "near" in end else (_f(1.2), "max_dist", False)
        x = _f(d / f)
        while _f(f * x) <= d if up else _f(f * x) >= d:              # to the first float past the end
            x = np.nextafter(x, _f(np.inf) if up else _f(0.0))
        inside = np.nextafter(x, _f(0.0) if up else _f(np.inf))
        while not (_f(f * inside) <= d if up else _f(f * inside) >= d):
            inside = np.nextafter(inside, _f(0.0) if up else _f(np.inf))
        p[key] = inside if end.endswith("end") else x
        return p

    S["near_end"] = site(100.0, 140.0, p1=ranged(100.0, 140.0, "near_end"))
    S["too_near"] = site(140.0, 140.0, p1=ranged(140.0, 140.0, "too_near"))
    S["too_far"] = site(180.0, 140.0, p1=ranged(180.0, 140.0, "too_far"))
    S["far_end"] = site(220.0, 140.0, p1=ranged(220.0, 140.0, "far_end"))
    S["level_filter"] = site(260.0, 140.0, p1=pt(260.3, 140.2, level=3), oct2=0)   # octave 0 outside [2, 3]
    S["level_ok"] = site(300.0, 140.0, p1=pt(300.3, 140.2, level=3), oct2=2)
    S["empty_window"] = site(340.0, 140.0, p1=pt(500.0, 400.0))
    S["bad_point"] = site(380.0, 140.0)
    S["no_point_1"] = site(420.0, 140.0, p1=False)
    S["no_point_2"] = site(460.0, 140.0, p2=False)
    S["already"] = site(500.0, 140.0)                                # matched on entry: kept, and blocks idx2
    # a disagreement: site a's point goes to site b's keypoint in KF2, whose point comes back to b in KF1
    S["dis_a"] = site(100.0, 300.0, p1=pt(140.3, 300.2), p2=False)
    S["dis_b"] = site(140.0, 300.0, p1=False)
    bad = np.zeros(n_real + len(hand), np.uint8)
    bad[rows1[S["bad_point"]]] = 1
    m = np.full(len(kp1), -1, np.int32)
    m[S["already"]] = S["already"]
    ka, kb = sim3_keyframe(kp1, rows1, g), sim3_keyframe(kp2, rows2, g)
    add("hand_edges", ka, kb, m)
    add("hand_edges_scale_2", ka, kb, m, s12=2.0)                    # p3Dc2 = p3Dw / 2: other distances, other levels
    add("hand_edges_scale_1_ulp", ka, kb, m, s12=np.nextafter(_f(1.0), _f(2.0)))
    # the override: nothing of KF2 blocked although match12 names a keypoint, and another one blocked instead
    a2 = np.zeros(len(kp2), np.uint8)
    a2[S["agree"]] = 1
    add("hand_edges_already2_override", ka, kb, m, already2=a2)
    points = np.concatenate([real_points, np.array(hand, real_points.dtype)])
    return points, bad, cases, S


def sim3_reference(case, points, bad, trace=None):
    return LR.search_by_sim3(case["kf1"], case["kf2"], points, bad, case["s12"], case["R12"], case["t12"],
                             case["match12"], geo(), case["th"], case["already2"], trace)


# ---------------------------------------------------------------- SearchByProjection(pKF, Scw) and Fuse(pKF, Scw)
def scaled(T, s):
    """Scw of scale s over the pose T: s * [R | t] in float."""
    S = np.asarray(T, np.float32).reshape(4, 4).copy()
    S[:3, :] = (S[:3, :] * _f(s)).astype(np.float32)
    return S.reshape(16)


@functools.lru_cache(maxsize=None)
def scw_cases():
    """(keyframes, projection problems, fuse problems)."""
    g, rkfs, points, _ = real_pair()
    fkfs, fproblems = FC.build()
    kfs = [dict(k) for k in fkfs]                                    # fuse_cases' keyframes keep their indices
    by_name = {p["name"]: p for p in fproblems}
    proj, fuse = [], []

    def add_proj(name, Scw, P, kf, th=10.0, skip=None, taken=None):
        proj.append(dict(name=name, Scw=np.asarray(Scw, np.float32).reshape(16), P=P, kf=kf, th=th, skip=skip,
                         taken=taken))

    def add_fuse(name, Scw, P, kf, th=4.0, skip=None):
        fuse.append(dict(name=name, Scw=np.asarray(Scw, np.float32).reshape(16), P=P, kf=kf, th=th, skip=skip))

    # ---- the loop's shape: keyframe 1's map points into keyframe 2 (frame 16) by its pose, as Scw of scale 1, of
    # scale 1 up to a few ulp (LoopClosing.cc:337) and of scale 2
    kfs.append(dict(rkfs[1]))
    k16 = len(kfs) - 1
    P1 = points[rkfs[0]["match_row"][rkfs[0]["match_row"] >= 0]]
    T2 = rkfs[1]["Tcw"]
    rng = np.random.default_rng(13)
    skip = (rng.uniform(size=len(P1)) < 0.1).astype(np.uint8)
    taken = (rng.uniform(size=len(rkfs[1]["kun"])) < 0.3).astype(np.uint8)
    ulp = _f(1.0)
    for _ in range(3):
        ulp = np.nextafter(ulp, _f(2.0))
    add_proj("real", T2, P1, k16)
    add_proj("real_skip_taken", T2, P1, k16, skip=skip, taken=taken)
    add_proj("real_scale_ulp", scaled(T2, ulp), P1, k16, skip=skip, taken=taken)
    add_proj("real_scale_2", scaled(T2, 2.0), P1, k16, taken=taken)
    add_fuse("real", T2, P1, k16)
    add_fuse("real_skip", T2, P1, k16, skip=skip)
    add_fuse("real_scale_ulp", scaled(T2, ulp), P1, k16, skip=skip)
    add_fuse("real_scale_2", scaled(T2, 2.0), P1[:200], k16)
    add_fuse("real_th30", T2, P1[:200], k16, th=30.0)
    G = PTS_PER_GROUP
    for n in (0, 1, G - 1, G, G + 1):
        add_proj(f"real_n{n}", T2, P1[:n], k16, taken=taken)
        add_fuse(f"real_n{n}", T2, P1[:n], k16)
    no_kp = next(p for p in fproblems if p["name"] == "keyframe_without_keypoints")["kf"]
    add_proj("keyframe_without_keypoints", T2, P1[:70], no_kp)
    add_fuse("keyframe_without_keypoints", T2, P1[:70], no_kp)

    # ---- fuse_cases' hand-made problems under an Scw with scale: the status table, the candidates the other Fuse's
    # chi-square test refuses and this one takes, uright ignored, ties, clipped and wide windows
    st = by_name["statuses"]
    for s, tag in ((1.0, "1"), (2.0, "2"), (ulp, "ulp")):
        add_fuse(f"statuses_scale_{tag}", scaled(EYE, s), st["P"], st["kf"])
        add_proj(f"statuses_scale_{tag}", scaled(EYE, s), st["P"], st["kf"])
    for name in ("chi2_stereo_second_wins", "chi2_mono_second_wins", "uright_zero_is_stereo", "levels"):
        add_fuse(name, scaled(EYE, 2.0), by_name[name]["P"], by_name[name]["kf"])
    tz = by_name["ties_all_zero"]
    add_fuse("ties_all_zero", tz["Tcw"], tz["P"], tz["kf"], th=30.0)
    add_proj("ties_all_zero", tz["Tcw"], tz["P"], tz["kf"], th=30.0)   # equal descriptors: each takes the next one
    cl = by_name["clipped_th3"]
    for th in (4.0, 30.0):
        add_fuse(f"clipped_th{int(th)}", scaled(EYE, 2.0), cl["P"], cl["kf"], th=th)
        add_proj(f"clipped_th{int(th)}", EYE, cl["P"], cl["kf"], th=th)

    # ---- K + 1 and 2K contenders with equal descriptors on one window of as many keypoints: each takes the next
    # one in scan order, and past K the walk must re-scan
    for n in (PROJ_KEYS + 1, 2 * PROJ_KEYS):
        kfs.append(FC.make_keyframe([(300.0 + 0.5 * j, 200.0 + 0.25 * j, 0, -1.0, None) for j in range(n)], g))
        add_proj(f"contenders_{n}", EYE, FC.stack([FC.point_at(g, 301.0, 200.5) for _ in range(n)]), len(kfs) - 1)
        # ... and one contender too many: the last finds nothing
        add_proj(f"contenders_{n}_plus_1", EYE, FC.stack([FC.point_at(g, 301.0, 200.5) for _ in range(n + 1)]),
                 len(kfs) - 1)
    # ... a point whose K keys were all taken by others, its own distances to them above TH_LOW: out of keys, but
    # nothing further could be accepted, so no re-scan is due
    kfs.append(FC.make_keyframe([(300.0 + 0.5 * j, 200.0, 0, -1.0, bits(200) if j == PROJ_KEYS else None)
                                 for j in range(PROJ_KEYS + 1)], g))
    far = FC.point_at(g, 301.0, 200.5)
    far["desc"] = bits(60)
    add_proj("keys_taken_last_above_th", EYE, FC.stack([FC.point_at(g, 301.0, 200.5) for _ in range(PROJ_KEYS)] + [far]),
             len(kfs) - 1)

    # ---- initially taken keypoints and skip flags on a small window; distance 50 accepted, 51 refused
    kfs.append(FC.make_keyframe([(300.0, 200.0, 0, -1.0, bits(1)), (301.0, 200.0, 0, -1.0, bits(2)),
                                 (100.0, 100.0, 0, -1.0, bits(50)), (500.0, 100.0, 0, -1.0, bits(51))], g))
    k_small = len(kfs) - 1
    Ps = FC.stack([FC.point_at(g, 300.4, 200.2), FC.point_at(g, 300.6, 200.1), FC.point_at(g, 100.3, 100.2),
                   FC.point_at(g, 500.3, 100.2), FC.point_at(g, 300.5, 200.3)])
    add_proj("small", EYE, Ps, k_small)
    add_proj("small_taken", EYE, Ps, k_small, taken=np.array([1, 0, 0, 0], np.uint8))
    add_proj("small_skip", EYE, Ps, k_small, skip=np.array([1, 0, 0, 0, 0], np.uint8))
    add_proj("small_all_taken", EYE, Ps, k_small, taken=np.ones(4, np.uint8))
    add_fuse("small_50_51", EYE, Ps, k_small)
    return kfs, proj, fuse


def proj_reference(problem, kfs, trace=None):
    k = kfs[problem["kf"]]
    return LR.search_by_projection_sim3(problem["Scw"], problem["P"], k["kun"], k["desc"], k["go"], k["gi"], geo(),
                                        problem["th"], problem["skip"], problem["taken"], trace)


def fuse_reference(problem, kfs, traces=None):
    k = kfs[problem["kf"]]
    return LR.fuse_sim3_snapshot(problem["Scw"], problem["P"], k["kun"], k["desc"], k["go"], k["gi"], geo(),
                                 problem["th"], problem["skip"], traces)
