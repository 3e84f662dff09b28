"""The case table of tests/test_gpu_local_map.py: synthetic, tiny maps as spslam_local_map tables (one sequence each,
indices local to it), built by hand or from a seeded generator.  tests/test_local_map_host.py runs every case on the
restatement alone and asserts `want`: that the case reaches what it is there for, and stays within capacity."""
import numpy as np

import local_map_ref as R


def tables_from_dicts(points, kfs):
    """local_map_ref's map model (points 0 .. nr-1, keyframes 0 .. nk-1) as spslam_local_map tables."""
    nr, nk = len(points), len(kfs)
    obs_off, obs_kf = np.zeros(nr + 1, np.int32), []
    for r in range(nr):
        obs_kf.extend(sorted(points[r]["obs"]))
        obs_off[r + 1] = len(obs_kf)
    covis = np.full((nk, 10), -1, np.int32)
    child_off, child = np.zeros(nk + 1, np.int32), []
    match_off, match_row = np.zeros(nk + 1, np.int32), []
    parent = np.full(nk, -1, np.int32)
    for k in range(nk):
        c = kfs[k]["covis"][:10]
        covis[k, :len(c)] = c
        child.extend(sorted(kfs[k]["children"]))
        child_off[k + 1] = len(child)
        match_row.extend(-1 if p is None else p for p in kfs[k]["matches"])
        match_off[k + 1] = len(match_row)
        parent[k] = -1 if kfs[k]["parent"] is None else kfs[k]["parent"]
    return dict(obs_off=obs_off, obs_kf=np.asarray(obs_kf, np.int32),
                point_bad=np.array([points[r]["bad"] for r in range(nr)], np.uint8),
                kf_bad=np.array([kfs[k]["bad"] for k in range(nk)], np.uint8), covis=covis, child_off=child_off,
                child=np.asarray(child, np.int32), parent=parent, match_off=match_off,
                match_row=np.asarray(match_row, np.int32))


def hand(n_kf, matches, covis=None, parent=None, bad_kf=(), bad_pt=(), obs=None):
    """A map written out by hand.  matches: {k: [pid or None, ...]}; obs: {pid: [k, ...]}, default: the keyframes
    whose match lists hold the point; children follow from parent."""
    covis, parent, obs = covis or {}, parent or {}, obs or {}
    n_pts = 1 + max([p for m in matches.values() for p in m if p is not None] + list(obs) + [-1])
    points = {}
    for p in range(n_pts):
        o = obs.get(p, [k for k in sorted(matches) if p in matches[k]])
        points[p] = {"obs": list(o), "bad": p in bad_pt}
    kfs = {k: {"bad": k in bad_kf, "covis": list(covis.get(k, [])), "parent": parent.get(k),
               "children": [c for c in sorted(parent) if parent[c] == k], "matches": list(matches.get(k, []))}
           for k in range(n_kf)}
    return points, kfs


def random_map(seed, n_kf, own=(3, 6), share=0.4, empty=0.15, covis_n=4, parents=True, p_bad_pt=0.0):
    """Keyframe k creates own[0] .. own[1] points and also holds points of earlier keyframes (a fraction `share`
    of its filled slots) and empty slots (a fraction `empty` of all), shuffled.  Returns (points, kfs, creator)."""
    rng = np.random.default_rng(seed)
    matches, creator = {}, []
    for k in range(n_kf):
        n_own = int(rng.integers(own[0], own[1] + 1))
        lst = list(range(len(creator), len(creator) + n_own))
        n_sh = min(int(round(share / (1 - share) * n_own)), len(creator)) if k else 0
        lst += [int(p) for p in rng.choice(len(creator), n_sh, replace=False)] if n_sh else []
        creator += [k] * n_own
        lst += [None] * int(round(empty / (1 - empty) * len(lst)))
        matches[k] = [lst[i] for i in rng.permutation(len(lst))]
    covis = {k: [int(c) for c in rng.permutation([j for j in range(n_kf) if j != k])[:covis_n]] for k in range(n_kf)}
    parent = {k: int(rng.integers(0, k)) for k in range(1, n_kf)} if parents else {}
    bad_pt = set(np.flatnonzero(rng.uniform(size=len(creator)) < p_bad_pt).tolist())
    points, kfs = hand(n_kf, matches, covis, parent, bad_pt=bad_pt)
    return points, kfs, np.asarray(creator, np.int32)


def frame_rows(seed, kfs, n_kp, from_kfs=None, p_none=0.3):
    """n_kp keypoints: points drawn from the match lists of from_kfs (default: all keyframes), or -1."""
    rng = np.random.default_rng(seed)
    pool = sorted({p for k in (kfs if from_kfs is None else from_kfs) for p in kfs[k]["matches"] if p is not None})
    rows = rng.choice(pool, n_kp, replace=True).astype(np.int32)
    rows[rng.uniform(size=n_kp) < p_none] = -1
    if n_kp and (rows < 0).all():
        rows[0] = pool[0]
    return rows


def _case(name, points, kfs, rows, want, local_kfs=(), capacity=None, creator=None):
    T = tables_from_dicts(points, kfs)
    return dict(name=name, T=T, frame_rows=np.asarray(rows, np.int32), local_kfs=list(local_kfs),
                capacity=len(T["match_row"]) + 1 if capacity is None else capacity, want=want, creator=creator)


def _one_of_each(kfs, ks):
    """One point per keyframe of ks that only this keyframe observes (its first such match)."""
    held = {}
    for k in kfs:
        for p in kfs[k]["matches"]:
            if p is not None:
                held.setdefault(p, set()).add(k)
    return [next(p for p in kfs[k]["matches"] if p is not None and held[p] == {k}) for k in ks]


def build_cases():
    C = []
    # ---- keyframe counts
    P, K, _ = random_map(1, 1)
    C.append(_case("nkf1", P, K, frame_rows(1, K, 5), lambda r: r["local_kfs"] == [0] and r["kf_max"] == 0))
    P, K = hand(2, {0: [0, None, 1], 1: [2, 1, 3]}, covis={0: [1], 1: [0]}, parent={1: 0})
    C.append(_case("nkf2_neighbour", P, K, [0, -1, 0],
                   lambda r: r["trace"]["k1"] == 1 and r["local_kfs"] == [0, 1] and r["trace"]["n_dup"] == 1))
    # ---- keypoint counts around the workgroup size (256), 7 keyframes
    for n in (1, 63, 64, 65, 255, 256, 257, 700):
        P, K, cr = random_map(7, 7, own=(40, 60))
        C.append(_case(f"nkf7_kp{n}", P, K, frame_rows(100 + n, K, n),
                       lambda r: r["trace"]["k1"] >= 1 and r["n_total"] > 0 and r["trace"]["n_dup"] > 0, creator=cr))
    # ---- the > 80 limit
    P, K, _ = random_map(96, 96, share=0.0)
    C.append(_case("k1_over_80", P, K, _one_of_each(K, range(85)),
                   lambda r: r["trace"]["k1"] == 85 and r["trace"]["ended"] == "limit" and
                   r["trace"]["ended_at"] == 0 and len(r["local_kfs"]) == 85))
    P, K, _ = random_map(97, 96, share=0.0, parents=False)
    C.append(_case("k1_79_stops_midway", P, K, _one_of_each(K, range(79)),
                   lambda r: r["trace"]["k1"] == 79 and r["trace"]["ended"] == "limit" and
                   0 < r["trace"]["ended_at"] < 79 and len(r["local_kfs"]) == 81))
    # ---- a concatenated match list longer than one compaction chunk
    P, K, _ = random_map(12, 12, own=(150, 160), share=0.5)
    C.append(_case("long_concat", P, K, frame_rows(12, K, 300),
                   lambda r: r["trace"]["n_concat"] >= 3000 and r["trace"]["n_empty"] > 300 and
                   0.3 * r["trace"]["n_concat"] < r["trace"]["n_dup"] < 0.5 * r["trace"]["n_concat"]))
    # ---- covisible lists
    m3 = {0: [0, 1], 1: [2, None, 0], 2: [3]}
    m13 = {**m3, **{k: [10 + k] for k in range(3, 13)}}
    P, K = hand(13, m13, covis={0: [1, 2], 1: [0, 2], 2: [1, 0]})
    C.append(_case("covis_all_included", P, K, [0, 2, 3],
                   lambda r: r["local_kfs"] == [0, 1, 2] and r["trace"]["ended"] == "end"))
    P, K = hand(13, m13, covis={0: [3, 4], 1: [4], 2: [3]}, bad_kf={3, 4})
    C.append(_case("covis_all_bad", P, K, [0, 2, 3],
                   lambda r: r["local_kfs"] == [0, 1, 2] and r["trace"]["ended"] == "end"))
    P, K = hand(13, m13, covis={0: [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]}, bad_kf=set(range(3, 10)))
    C.append(_case("covis_first_free_at_10", P, K, [0, 2, 3], lambda r: r["local_kfs"] == [0, 1, 2, 10]))
    # ---- children and parents
    P, K = hand(6, {0: [0], 1: [1, 0], 2: [2], 5: [5]})
    C.append(_case("no_children_no_parent", P, K, [0, 1, 2],
                   lambda r: r["local_kfs"] == [0, 1, 2] and r["trace"]["ended"] == "end"))
    P, K = hand(6, {0: [0], 1: [1, 0], 2: [2], 5: [5]}, parent={1: 0, 2: 0, 5: 0})
    C.append(_case("child_first_free_last_parent_included", P, K, [0, 1, 2],
                   lambda r: r["local_kfs"] == [0, 1, 2, 5] and r["trace"]["ended"] == "end"))
    P, K = hand(6, {1: [0, 1], 2: [2], 3: [3, 0], 4: [4]}, covis={2: [4]}, parent={1: 3}, bad_kf={3})
    C.append(_case("bad_parent_appended_ends_loop", P, K, [1, 2],
                   lambda r: r["local_kfs"] == [1, 2, 3] and r["trace"]["ended"] == "parent" and
                   r["trace"]["ended_at"] == 0 and r["local_points"] == [0, 1, 2, 3]))
    # ---- bad points and bad keyframes
    P, K, _ = random_map(21, 7, own=(20, 30), p_bad_pt=0.2)
    rows = frame_rows(21, K, 90)
    C.append(_case("bad_points", P, K, rows,
                   lambda r, P=P, rows=rows: r["trace"]["n_bad"] > 0 and any(P[p]["bad"] for p in rows if p >= 0)))
    P, K, _ = random_map(22, 7, own=(20, 30))
    rows = frame_rows(22, K, 90)
    cnt = R.run_tables(tables_from_dicts(P, K), rows)["trace"]["counter"]
    top = max(sorted(cnt), key=lambda k: cnt[k])
    K[top]["bad"] = K[min(k for k in cnt if k != top)]["bad"] = True
    C.append(_case("bad_voters_with_the_top_one", P, K, rows,
                   lambda r, top=top: r["kf_max"] not in (-1, top) and top not in r["local_kfs"] and
                   r["trace"]["k1"] == len(r["trace"]["counter"]) - 2))
    P, K, _ = random_map(23, 7, share=0.0)
    K[2]["bad"] = K[4]["bad"] = True
    C.append(_case("all_voters_bad", P, K, _one_of_each(K, (2, 4)),
                   lambda r: r["local_kfs"] == [] and r["kf_max"] == -1 and r["n_total"] == 0 and
                   len(r["trace"]["counter"]) == 2, local_kfs=[0, 1]))
    # ---- an empty counter keeps the list, the points are gathered again
    P, K, _ = random_map(24, 7, p_bad_pt=0.2)
    bad = [p for p in P if P[p]["bad"]]
    C.append(_case("empty_counter_keeps_list", P, K, [-1, bad[0], -1, bad[-1]],
                   lambda r: r["local_kfs"] == [4, 1, 2] and r["kf_max"] == -1 and r["n_total"] > 0 and
                   r["trace"]["counter"] == {}, local_kfs=[4, 1, 2]))
    # ---- capacity: exactly n_local, one less (status 1, the prefix kept), one more
    P, K, _ = random_map(7, 7, own=(40, 60))
    rows = frame_rows(164, K, 64)
    n = R.run_tables(tables_from_dicts(P, K), rows)["n_total"]
    for d, st in ((0, 0), (-1, 1), (1, 0)):
        C.append(_case(f"capacity_n{d:+d}", P, K, rows,
                       lambda r, n=n, d=d, st=st: r["n_total"] == n and r["status"] == st and
                       len(r["local_points"]) == min(n, n + d), capacity=n + d))
    # ---- several observers per point: pKFmax differs from the vote that credits only the creator
    P, K = hand(2, {0: [0, 1, 2], 1: [3, 0, 1, 2, 4]})
    cr = np.array([0, 0, 0, 1, 1], np.int32)
    C.append(_case("observers_outvote_creator", P, K, [0, 1, 2, 3],
                   lambda r: r["kf_max"] == 1 and creator_vote([0, 1, 2, 3], np.array([0, 0, 0, 1, 1]), 2) == 0,
                   creator=cr))
    return C


def creator_vote(rows, creator, n_kf):
    """refkf_vote_kernel's vote: each point counted for the keyframe that created it, first maximum."""
    h = np.bincount(creator[[r for r in rows if r >= 0]], minlength=n_kf)
    return int(np.argmax(h)) if h.max() > 0 else -1


def reference(case):
    return R.run_tables(case["T"], case["frame_rows"], case["local_kfs"], case["capacity"])
