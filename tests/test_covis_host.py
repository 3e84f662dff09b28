"""CPU guards of the covisibility tests: every case of tests/covis_cases.py reaches the branch it is named for, the
referee's ordered list agrees with local_mapping.py covisible(), and the float64 products the culling's boundary
cases rely on are exact."""
import numpy as np

import covis_cases as CC
import covis_ref as CR


def test_update_cases_reach_their_branches():
    total = CR.collections.Counter()
    for name in CC.UPDATE_CASES:
        r = CC.replay_update(name)
        total.update(r["stats"])
        for branch in r["expect"]:
            assert r["stats"][branch] > 0, (name, branch)
    for branch in ("null_row", "bad_row", "own_observation", "empty", "below_th", "only_maximum", "unchanged_weight",
                   "first_connection"):
        assert total[branch] > 0, branch
    # the sizes and the positions of the keyframe
    for n in (2, 64, 65, 1024):
        r = CC.replay_update(f"n_kf_{n}")
        assert r["n_kfs"] == [n] and [int(s["problems"]["kf"][0]) for s in r["steps"]] == [0, n // 2, n - 1]
        assert all(s["want"]["status"][0] == CR.UPDATED for s in r["steps"])


def test_update_cases_hold_what_they_are_named_for():
    g = CC.replay_update("empty")
    assert g["steps"][1]["want"]["status"][0] == CR.EMPTY
    assert all(np.array_equal(g["steps"][1]["graph"][k], g["steps"][0]["graph"][k]) for k in g["graph0"])
    g = CC.replay_update("counts_14_15")["graphs"][0]
    assert g.ordered[2] == [4] and g.weights[2] == {1: 14, 4: 15} and g.ordered[1] == [] and g.ordered[4] == [2]
    g = CC.replay_update("equal_maxima")["graphs"][0]
    assert g.ordered[6] == [3] and g.ordered_w[6] == [7] and g.weights[6] == {1: 2, 3: 7, 5: 7}
    assert g.ordered[3] == [6] and g.ordered[5] == []
    g = CC.replay_update("equal_weights")["graphs"][0]
    assert g.ordered[1] == [7, 6, 2, 4] and g.ordered_w[1] == [31, 20, 20, 16]
    for n in (9, 10, 11, 64, 65, 128, 129):
        r = CC.replay_update(f"list_{n}")
        assert len(r["graphs"][0].ordered[0]) == n
        covis = r["steps"][-1]["graph"]["covis"][0]
        assert (covis >= 0).sum() == min(n, 10) and covis.tolist()[:min(n, 10)] == r["graphs"][0].ordered[0][:10]
        assert r["graphs"][0].parent[0] == -1 and r["graphs"][0].first_connection[0]   # index 0: never a parent
    g = CC.replay_update("null_and_bad_rows")["graphs"][0]
    assert g.weights[1] == {2: 15, 3: 14} and g.ordered[1] == [2]
    # the unchanged neighbour keeps a list that a re-sort would change; the changed one is re-sorted
    r = CC.replay_update("unchanged_neighbour")
    g = r["graphs"][0]
    assert g.ordered[3] == [1, 6] and g.weights[3] == {1: 17, 5: 9, 6: 15} and r["steps"][1]["want"]["n_resorted"][0] == 0
    before = [(w, j) for j, w in g.weights[3].items()]
    assert [j for _, j in sorted(before, reverse=True)] == [1, 6, 5]
    r = CC.replay_update("changed_neighbour")
    g = r["graphs"][0]
    assert g.ordered[3] == [1, 6, 5] and g.ordered_w[3] == [18, 15, 9] and r["steps"][1]["want"]["n_resorted"][0] == 1
    r = CC.replay_update("first_connection")
    assert [int(s["want"]["new_parent"][0]) for s in r["steps"]] == [-1, 3, -1]
    assert r["graphs"][0].parent[:3] == [-1, -1, 3] and r["graphs"][0].children[3] == {2}
    r = CC.replay_update("star_1024")
    assert r["steps"][0]["want"][0].tolist() == (CR.UPDATED, 1023, 1023, 1023)
    assert r["graphs"][0].ordered[5] == [k for k in range(1023, -1, -1) if k != 5]
    r = CC.replay_update("two_sequences")
    assert r["n_kfs"][0] != r["n_kfs"][1] and all(len(s["problems"]) == 2 for s in r["steps"])
    r = CC.replay_update("stream_of_calls")
    assert not r["sync"] and len(r["steps"]) == 11 and sum(int(s["want"]["n_resorted"][0]) for s in r["steps"]) > 11


def test_referee_agrees_with_local_mapping_covisible():
    """The ordered list after a keyframe's UpdateConnections on a fresh graph is covisible(j) of the product's
    local_mapping.py: its mp / obs dictionaries are filled from the same map."""
    import local_mapping
    checked = 0
    for name in ("n_kf_64", "n_kf_65", "equal_maxima", "equal_weights", "counts_14_15", "list_11", "two_sequences",
                 "stream_of_calls", "empty"):
        for m in CC.UPDATE_CASES[name]()["maps"]:
            lm = local_mapping.SeqMap.__new__(local_mapping.SeqMap)
            lm.kfs = [dict(mp={kp: r for kp, r in enumerate(rows) if r is not None and not m.bad[r]})
                      for rows in m.matches]
            lm.obs = {r: dict(o) for r, o in enumerate(m.obs)}
            for j in range(m.n_kf):
                g = CR.Graph(m.n_kf)
                CR.update_connections(m, g, j)
                assert g.ordered[j] == lm.covisible(j), (name, j)
                checked += bool(g.ordered[j])
    assert checked > 100


def test_culling_cases_reach_their_branches():
    r = CC.replay_culling("story")
    for branch in ("skipped_zero", "skipped_new_plane", "kept", "culled", "deferred", "depth_negative", "depth_far",
                   "few_observations", "coarser_observer", "too_few_observers", "erased_stereo", "erased_mono",
                   "point_went_bad"):
        assert r["stats"][branch] > 0, branch
    rec = {int(x["kf"]): (int(x["n_mps"]), int(x["n_redundant"]), int(x["status"])) for x in r["want_records"][0]}
    assert rec[0][2] == rec[6][2] == CR.SKIPPED and rec[7] == (0, 0, CR.KEPT) and rec[8] == (1, 1, CR.CULLED)
    assert rec[9][0] > 256 and rec[9][2] == CR.CULLED
    assert [rec[c] for c in (10, 11, 12, 13)] == [(10, 9, CR.KEPT), (10, 10, CR.CULLED), (20, 18, CR.KEPT),
                                                  (20, 19, CR.CULLED)]
    assert rec[14][0] == 3                                    # th_depth itself and 0 are counted
    assert rec[15] == (6, 3, CR.KEPT)
    assert rec[16][2] == CR.CULLED and rec[17] == (6, 0, CR.KEPT)      # B was redundant only through A
    assert rec[18][2] == CR.CULLED and rec[19] == (9, 9, CR.CULLED)    # a point of B went bad: nMPs 10 -> 9
    assert rec[20][2] == rec[22][2] == CR.CULLED
    assert rec[21] == (9, 9, CR.CULLED) and rec[23] == (10, 9, CR.KEPT)  # the erased observation weighs 2 or 1
    assert rec[24][2] == CR.DEFERRED and rec[25] == (6, 6, CR.CULLED)
    # without the earlier cullings B would have been judged otherwise
    m, cur, order = CC.culling_story()
    alone = dict((c, CR.keyframe_culling(CC.culling_story()[0], cur, [c], CC.TH_DEPTH)[0][0]) for c in (17, 19, 21))
    assert alone[17][3] == CR.CULLED and alone[19][1:] == (10, 9, CR.KEPT) and alone[21][1:] == (10, 9, CR.KEPT)
    assert CC.replay_culling("current_new_plane")["stats"]["current_new_plane"] == 1
    two = CC.replay_culling("two_sequences")
    assert two["want_summaries"]["status"].tolist() == [CR.RAN, CR.RAN, CR.NEW_PLANE]
    assert two["want_summaries"]["n_candidates"].tolist() == [4, 21, 0]


def test_point_culling_cases_reach_every_branch():
    tables, rows, cur, named = CC.point_cull_tables()
    want = CC.point_cull_want(tables, rows, cur)
    v = {name: int(want[q]) for name, q in named.items()}
    assert v == dict(drop=CR.POINT_DROP, drop_before_ratio=CR.POINT_DROP, bad_ratio=CR.POINT_BAD_RATIO,
                     ratio_before_obs=CR.POINT_BAD_RATIO, ratio_exactly_quarter=CR.POINT_KEEP,
                     bad_obs=CR.POINT_BAD_OBS, bad_obs_before_expired=CR.POINT_BAD_OBS,
                     four_observations=CR.POINT_KEEP, expired=CR.POINT_EXPIRED, young=CR.POINT_KEEP,
                     keep=CR.POINT_KEEP, never_visible=CR.POINT_KEEP, found_unseen=CR.POINT_KEEP)
    assert len(rows) > 256 and all((want == b).sum() > 5 for b in range(5))


def test_boundary_products_are_exact_in_float64():
    assert 0.9 * 10 == 9.0 and 0.9 * 20 == 18.0
    assert not 9.0 > 0.9 * 10.0 and not 18.0 > 0.9 * 20.0 and 10.0 > 0.9 * 10.0 and 19.0 > 0.9 * 20.0
