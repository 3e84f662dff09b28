"""CPU checks of the local-map step (Tracking::UpdateLocalMap, src/Tracking.cc:1427-1571): the scalar restatement
tests/local_map_ref.py pinned on cases whose expected lists are written out by hand; SeqMap.local_map_tables();
the layout of the two ABI structs; and a guard that the GPU case table (tests/local_map_cases.py) is not
degenerate, asserted from the restatement alone."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import local_map_cases as LC
import local_map_ref as R

ROOT = pathlib.Path(__file__).resolve().parents[1]


def kf(matches=(), covis=(), children=(), parent=None, bad=False):
    return {"bad": bad, "covis": list(covis), "children": list(children), "parent": parent,
            "matches": list(matches)}


def pts(obs, bad=()):
    return {p: {"obs": list(o), "bad": p in bad} for p, o in obs.items()}


# ---------------------------------------------------------------- the restatement, pinned by hand
def test_votes_first_maximum_and_point_order():
    points = pts({0: [0, 1], 1: [1], 2: [0], 3: [2], 4: [0, 2]})
    kfs = {0: kf([0, None, 2, 4]), 1: kf([1, 0]), 2: kf([4, 3, None])}
    # votes: point 0 -> kf 0, 1; point 1 -> kf 1; point 2 -> kf 0: kf 0 and kf 1 tie at 2, the first one wins
    r = R.update_local_map([0, None, 1, 2], points, kfs, [])
    assert r["local_kfs"] == [0, 1] and r["kf_max"] == 0
    assert r["local_points"] == [0, 2, 4, 1]  # kf 0's list, then kf 1's without the repeated point 0
    assert r["status"] == 0 and r["n_total"] == 4


def test_parent_break_ends_the_whole_loop():
    points = pts({0: [1], 1: [2], 2: [3], 3: [4]})
    # kf 1: covisible 4 is taken, child 5 is taken, its parent 3 is not in the list: appended, and the loop ends,
    # so kf 2 never gets to add its free covisible 6
    kfs = {0: kf(), 1: kf([0], covis=[4], children=[5], parent=3), 2: kf([1], covis=[6]), 3: kf([2], children=[1]),
           4: kf([3]), 5: kf([], parent=1), 6: kf([0])}
    r = R.update_local_map([0, 1], points, kfs, [9, 9])
    assert r["local_kfs"] == [1, 2, 4, 5, 3] and r["kf_max"] == 1
    assert r["trace"]["ended"] == "parent" and r["trace"]["ended_at"] == 0
    assert r["local_points"] == [0, 1, 3, 2]
    # the same map with the parent already a voter: the loop goes on and kf 2 adds 6
    points[2]["obs"] = [3]
    r = R.update_local_map([0, 1, 2], points, kfs, [])
    assert r["local_kfs"] == [1, 2, 3, 4, 5, 6] and r["trace"]["ended"] == "end"


def test_bad_parent_is_still_appended():
    points = pts({0: [0]})
    kfs = {0: kf([0], parent=1), 1: kf([], bad=True)}
    assert R.update_local_map([0], points, kfs, [])["local_kfs"] == [0, 1]


def test_stop_above_80():
    n = 90
    points = pts({p: [p] for p in range(n)})
    kfs = {k: kf([k], covis=[(k + 85) % n]) for k in range(n)}
    # 81 voters: the size check fails before the first entry, nothing is added
    r = R.update_local_map(list(range(81)), points, kfs, [])
    assert r["local_kfs"] == list(range(81)) and r["trace"]["ended"] == "limit" and r["trace"]["ended_at"] == 0
    # 79 voters: entry 0 adds kf 85, entry 1 adds kf 86 (81 entries), entry 2 is refused
    r = R.update_local_map(list(range(79)), points, kfs, [])
    assert r["local_kfs"] == list(range(79)) + [85, 86]
    assert r["trace"]["ended"] == "limit" and r["trace"]["ended_at"] == 2
    # 80 voters: 80 is not > 80, so entry 0 still adds one
    r = R.update_local_map(list(range(80)), points, kfs, [])
    assert r["local_kfs"] == list(range(80)) + [85] and r["trace"]["ended_at"] == 1


def test_bad_keyframe_cannot_be_kf_max():
    points = pts({0: [0, 1], 1: [0], 2: [1], 3: [2]})
    kfs = {0: kf([0, 1], bad=True), 1: kf([0, 2]), 2: kf([3])}
    r = R.update_local_map([0, 1, 2, 3], points, kfs, [])  # votes 2, 2, 1: kf 0 is bad
    assert r["local_kfs"] == [1, 2] and r["kf_max"] == 1 and r["local_points"] == [0, 2, 3]
    kfs[1]["bad"] = kfs[2]["bad"] = True                   # all voters bad: cleared, none
    r = R.update_local_map([0, 1, 2, 3], points, kfs, [2, 1])
    assert r["local_kfs"] == [] and r["kf_max"] == -1 and r["local_points"] == []


def test_empty_counter_keeps_the_old_list():
    points = pts({0: [0], 1: [1], 2: [1]}, bad={0})
    kfs = {0: kf([0]), 1: kf([1, 2, 0])}
    r = R.update_local_map([None, 0], points, kfs, [1, 0])  # the only frame point is bad: no vote at all
    assert r["local_kfs"] == [1, 0] and r["kf_max"] == -1 and r["local_points"] == [1, 2]
    assert r["trace"]["n_bad"] == 2


def test_covisibles_beyond_ten_are_not_looked_at():
    points = pts({0: [0]})
    kfs = {k: kf(bad=1 <= k <= 10) for k in range(12)}
    kfs[0] = kf([0], covis=list(range(1, 12)))
    assert R.update_local_map([0], points, kfs, [])["local_kfs"] == [0]


def test_capacity_rule():
    points = pts({p: [0] for p in range(5)})
    kfs = {0: kf([0, 1, None, 2, 1, 3, 4])}
    for cap, n, st in ((5, 5, 0), (4, 4, 1), (6, 5, 0), (0, 0, 1)):
        r = R.update_local_map([0], points, kfs, [], cap)
        assert r["local_points"] == [0, 1, 2, 3, 4][:n] and r["status"] == st and r["n_total"] == 5


def test_tables_round_trip():
    P, K, _ = LC.random_map(5, 9, p_bad_pt=0.1)
    K[3]["bad"] = True
    P2, K2 = R.dicts_from_tables(LC.tables_from_dicts(P, K))
    assert P2 == P and K2 == K


# ---------------------------------------------------------------- SeqMap.local_map_tables()
@pytest.fixture(scope="module")
def seqmap():
    import local_mapping
    import spslam_match
    n_kf, cap, own = 7, 64, 40
    kf_points = []
    for j in range(n_kf):
        Pj = np.zeros(own, spslam_match.LOCAL_POINT_DTYPE)
        Pj["id"] = j * cap + np.arange(own)
        kf_points.append(Pj)
    m = local_mapping.SeqMap(kf_points, cap, (500, 500, 320, 240, 40), np.ones(8), np.ones(8),
                             np.zeros(0, [("id", "<i4"), ("world", "<f4", 4)]))
    rng = np.random.default_rng(3)
    shared = {1: (0, 20), 2: (1, 16), 3: (2, 14), 4: (0, 3), 5: (4, 15), 6: (5, 2)}  # (earlier keyframe, how many)
    for j in range(n_kf):
        matched = {}
        if j in shared:
            i, n = shared[j]
            # the first n own points of keyframe i, seen at keypoints 40 .. 40 + n of keyframe j
            matched = {own + q: i * cap + q for q in range(n)}
        nkp = own + 24
        m.insert_keyframe(j, np.eye(4), rng.uniform(0, 600, (nkp, 2)), np.full(nkp, -1.0), np.zeros(nkp, np.int32),
                          matched, [])
    return m


def test_seqmap_tables(seqmap):
    m = seqmap
    T = m.local_map_tables()
    nk = len(m.kfs)
    assert nk >= 6 and len(T["parent"]) == nk and T["covis"].shape == (nk, 10)
    weights = sorted(sum(1 for p in m.kfs[j]["mp"].values() if i in m.obs[p]) for j in m.kfs for i in m.kfs if i < j)
    assert weights[0] < m.COVIS_TH <= weights[-1] and any(0 < w < m.COVIS_TH for w in weights)
    for r, pid in enumerate(m.table["id"].tolist()):
        assert T["obs_kf"][T["obs_off"][r]:T["obs_off"][r + 1]].tolist() == sorted(m.obs.get(pid, {}))
    assert not T["point_bad"].any() and not T["kf_bad"].any()
    for j in range(nk):
        c = m.covisible(j)
        assert T["covis"][j].tolist() == c[:10] + [-1] * (10 - len(c[:10]))
        assert T["parent"][j] == m.parent[j]
        assert T["child"][T["child_off"][j]:T["child_off"][j + 1]].tolist() == \
            sorted(c for c in m.parent if m.parent[c] == j)
        rows = T["match_row"][T["match_off"][j]:T["match_off"][j + 1]]
        assert len(rows) == len(m.kfs[j]["ur"])
        want = np.full(len(rows), -1)
        for kp, pid in m.kfs[j]["mp"].items():
            want[kp] = m.row_of[pid]
        assert np.array_equal(rows, want)
    # the first-connection rule: none for keyframe 0, else the best covisible when the keyframe was inserted
    assert m.parent == {0: -1, 1: 0, 2: 1, 3: 2, 4: 0, 5: 4, 6: 5}


def test_restatement_from_tables_equals_restatement_from_dicts(seqmap):
    m = seqmap
    T = m.local_map_tables()
    points = {pid: {"obs": sorted(m.obs.get(pid, {})), "bad": False} for pid in m.table["id"].tolist()}
    kfs = {j: {"bad": False, "covis": m.covisible(j)[:10], "parent": m.parent[j] if m.parent[j] >= 0 else None,
               "children": sorted(c for c in m.parent if m.parent[c] == j),
               "matches": [m.kfs[j]["mp"].get(kp) for kp in range(len(m.kfs[j]["ur"]))]} for j in m.kfs}
    rng = np.random.default_rng(8)
    for src in ((1,), (3,), (5, 6), (0, 1, 2, 3, 4, 5, 6)):
        ids = [m.kfs[j]["mp"][kp] for j in src for kp in sorted(m.kfs[j]["mp"])]
        fp = [ids[i] if rng.uniform() < 0.7 else None for i in rng.integers(0, len(ids), 50)]
        a = R.update_local_map(fp, points, kfs, [])
        b = R.run_tables(T, [-1 if p is None else m.row_of[p] for p in fp])
        assert a["local_kfs"] == b["local_kfs"] and a["kf_max"] == b["kf_max"]
        assert [m.row_of[p] for p in a["local_points"]] == b["local_points"]
        assert len(a["local_kfs"]) > a["trace"]["k1"] or len(src) == 7


# ---------------------------------------------------------------- struct layout
LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spslam_gpu.h"
#define S(T) printf(#T " %zu\n", sizeof(T));
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f));
int main(void) {
  S(spslam_local_map) S(spslam_local_map_out)
@FIELDS@
  return 0;
}
"""


def test_struct_layouts_match_bindings(tmp_path):
    import spslam_track
    structs = {"spslam_local_map": spslam_track.LocalMap, "spslam_local_map_out": spslam_track.LocalMapOut}
    lines = "\n".join(f"  O({name}, {f[0]})" for name, st in structs.items() for f in st._fields_)
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C.replace("@FIELDS@", lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = {k: int(v) for k, v in (line.split() for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    for name, st in structs.items():
        assert got[name] == ctypes.sizeof(st), name
        for f in st._fields_:
            assert got[f"{name}.{f[0]}"] == getattr(st, f[0]).offset, (name, f[0])


# ---------------------------------------------------------------- the GPU case table is not degenerate
CASES = LC.build_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_gpu_case_reaches_what_it_is_there_for(case):
    r = LC.reference(case)
    assert case["want"](r), (case["name"], r["local_kfs"], r["kf_max"], r["n_total"], r["trace"])
    if not case["name"].startswith("capacity_n-1"):
        assert r["status"] == 0 and r["n_total"] <= case["capacity"]


def test_gpu_case_table_covers_the_issue_list():
    names = {c["name"] for c in CASES}
    assert {f"nkf7_kp{n}" for n in (1, 63, 64, 65, 255, 256, 257, 700)} <= names
    assert {"nkf1", "nkf2_neighbour", "k1_over_80", "k1_79_stops_midway", "long_concat", "covis_all_included",
            "covis_all_bad", "covis_first_free_at_10", "no_children_no_parent",
            "child_first_free_last_parent_included", "bad_parent_appended_ends_loop", "bad_points",
            "bad_voters_with_the_top_one", "all_voters_bad", "empty_counter_keeps_list", "capacity_n+0",
            "capacity_n-1", "capacity_n+1", "observers_outvote_creator"} <= names
    c = next(c for c in CASES if c["name"] == "observers_outvote_creator")
    r = LC.reference(c)
    assert r["kf_max"] != LC.creator_vote(c["frame_rows"], c["creator"], len(c["T"]["parent"]))
