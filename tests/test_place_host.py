"""CPU guards of the place-recognition cases (tests/place_cases.py) and their referee (tests/place_ref.py): each case
reaches what its name claims, the referee's score agrees with the dense L1 formula, and the candidate lists of the
stateless cases agree with a second, set-based formulation."""
import numpy as np
import pytest

import place_cases as PC
import place_ref as PR
from matcher_ref import f32


def first_reloc(name):
    r = PC.replay(name)
    return r, r["steps"][0], r["stats"][0]


# ---------------------------------------------------------------- the referee's score
def dense_score(a, b):
    words = np.union1d(a[0], b[0])
    v, w = np.zeros(len(words)), np.zeros(len(words))
    v[np.searchsorted(words, a[0])], w[np.searchsorted(words, b[0])] = a[1], b[1]
    return 1.0 - 0.5 * np.abs(v - w).sum()


@pytest.mark.parametrize("name", ["n_kf_63", "vector_lengths", "vocabulary"])
def test_score_matches_dense_l1(name):
    """L1-normalised vectors: the score is 1 - 0.5 * ||v - w||_1 (to the float it is stored in)."""
    case = PC.CASES[name]()
    vs = [v for v in case["seqs"][0].vectors if len(v[0])][:12]
    for a in vs:
        for b in vs:
            st = {}
            got = PR.score(PR.Frame(0, *a), PR.Frame(0, *b), st)
            exact = -sum(st.get("terms", [])) / 2.0
            assert abs(exact - dense_score(a, b)) < 1e-12
            assert got == f32(exact)


def test_score_of_disjoint_vectors_is_minus_zero():
    s = PR.score(PR.Frame(0, *PC.vec([1, 2])), PR.Frame(0, *PC.vec([3])))
    assert s == 0 and np.signbit(s)


# ---------------------------------------------------------------- what each case reaches
def test_empty_cases_write_nothing():
    for name in ("empty_db", "no_shared_word"):
        r = PC.replay(name)
        for s in r["steps"]:
            assert s["want"]["status"].tolist() == [PR.EMPTY] and s["cands"][0].size == 0
            assert s["reloc_score"].tobytes() == r["packed"]["t"]["reloc_score"].tobytes()
            assert s["loop_score"].tobytes() == r["packed"]["t"]["loop_score"].tobytes()
    assert r["packed"]["t"]["reloc_score"].tobytes() == bytes([PC.SENT]) * 16


@pytest.mark.parametrize("name", ["first_seen_order", "equal_first_words", "retain_tie", "best_tie", "same_best"])
def test_order_cases(name):
    r, step, _ = first_reloc(name)
    want = r["case"]["want_order"]
    assert step["cands"][0].tolist() == want
    if name == "first_seen_order":
        assert want != sorted(want)


@pytest.mark.parametrize("max_common", [1, 4, 5, 10])
def test_word_threshold(max_common):
    r, step, _ = first_reloc(f"max_common_{max_common}")
    counts, mn = r["case"]["counts"], r["case"]["min_common"]
    rec = step["want"][0]
    assert (rec["max_common_words"], rec["min_common_words"]) == (max_common, mn)
    assert mn == {1: 0, 4: 3, 5: 4, 10: 8}[max_common]
    assert rec["n_scored"] == sum(c > mn for c in counts) and rec["n_sharing"] == len(counts)
    if mn >= 1:
        assert mn in counts and mn + 1 in counts      # exactly at the threshold, and one above
    # reloc_score is written for the scored keyframes only
    changed = step["reloc_score"] != 0
    assert changed.tolist() == [c > mn for c in counts]


def test_retain_tie_is_exact():
    _, step, st = first_reloc("retain_tie")
    assert st["retain_ties"] == [1] and 1 not in step["cands"][0]
    assert step["want"][0]["n_kept"] == 3 and step["want"][0]["n_candidates"] == 2


def test_best_tie_is_exact():
    _, step, st = first_reloc("best_tie")
    assert (0, 1) in st["best_ties"]
    assert step["reloc_score"][0] == step["reloc_score"][1]


def test_same_best_deduplicates():
    _, step, st = first_reloc("same_best")
    assert st["duplicates"] == [2, 2]


def test_stale_reads_happen():
    r = PC.replay("stale_three")
    second, third = r["stats"][1], r["stats"][2]
    assert second["stale_reads"] == [(0, 2, 0.75)]                  # the value query A left
    assert r["steps"][1]["cands"][0].tolist() == [2]                # a best keyframe this query did not score
    assert r["steps"][1]["reloc_score"][2] == r["steps"][0]["reloc_score"][2] == np.float32(0.75)
    assert third["stale_reads"] == [(1, 3, 0.0)]                    # the initial 0
    assert PC.replay("stale_two")["stats"][1]["stale_reads"] == [(0, 2, 0.75)]


def test_loop_story_reaches_its_branches():
    r = PC.replay("loop_story")
    step, st = r["steps"][0], r["stats"][0]
    assert st["connected_hits"] == {7, 8}
    assert (0, 8) in st["connected_neighbours"]                     # connected, inside a neighbour's covis row
    assert (0, 1) in st["below_min_feeds"]                          # scored below min_score, still feeds acc
    rec = step["want"][0]
    assert rec["n_scored"] == 4 and rec["n_kept"] == 3
    assert (step["loop_score"] != 0).tolist() == [True, True, False, True, False, True, False, False, False, False]
    below = PC.replay("loop_all_below")["steps"][0]
    assert below["want"][0]["status"] == PR.NONE_KEPT and below["want"][0]["n_scored"] == 4
    assert below["loop_score"].tobytes() == step["loop_score"].tobytes()      # the scores stay written
    bad, no_bad = PC.replay("loop_chained_bad"), PC.replay("loop_chained_no_bad")
    assert bad["steps"][0]["want_min"][0] == np.float32(0.27) and no_bad["steps"][0]["want_min"][0] == np.float32(0.2)
    assert bad["steps"][1]["chained"] and bad["steps"][1]["min_in"][0] == np.float32(0.27)


def test_erased_middle_keeps_index_order():
    r = PC.replay("erased_middle")
    assert [s["kind"] for s in r["steps"]] == ["reloc", "erase", "erase", "reloc", "add", "reloc"]
    assert r["steps"][3]["in_db"].tolist() == [1, 1, 0, 0, 1, 0]
    assert [s["cands"][0].tolist() for s in r["steps"] if s["kind"] == "reloc"] == [[1, 4], [1, 0, 4], [4]]


def test_sizes_and_lengths():
    for n in (1, 63, 64, 65, 1024):
        r = PC.replay(f"n_kf_{n}")
        assert r["case"]["seqs"][0].n_kf == n
        assert max(len(w) for w, _ in r["case"]["seqs"][0].vectors) <= 64
    r = PC.replay("vector_lengths")
    lens = r["packed"]["t"]["n_bow"].tolist()
    assert lens[:7] == list(PC.LENGTHS) and max(lens) == r["packed"]["cap"] == PC.LENGTHS_CAP
    assert r["steps"][3]["want_min"][0] == 0 and np.signbit(r["steps"][3]["want_min"][0])   # the empty vector: -0
    two = PC.replay("two_sequences")
    assert two["packed"]["kf_base"] == [0, 37] and len(two["steps"][0]["problems"]) == 2


def test_summation_order_case_is_order_sensitive():
    q, k = PC.order_sensitive_vectors()
    serial, rev, pairwise = PC.order_scores(list(q), list(k))
    assert serial != rev and serial != pairwise
    assert q.min() >= 1e-8 and q.max() <= 1 and k.min() >= 1e-8 and k.max() <= 1
    step = PC.replay("summation_order")["steps"][0]
    assert step["reloc_score"][0] == serial                         # the referee sums serially


# ---------------------------------------------------------------- a second formulation of the stateless cases
def set_based_reloc(case, frame):
    """Dense and stateless: sets of words, numpy sorts.  Valid where no neighbour is shared-but-unscored."""
    seq = case["seqs"][0]
    qw, qv = case["frames"][frame]
    pos = {int(w): i for i, w in enumerate(qw)}
    rows = []
    for k, (w, v) in enumerate(seq.vectors):
        common = sorted(set(pos) & set(int(x) for x in w)) if seq.in_db[k] else []
        if common:
            rows.append((min(pos[c] for c in common), k, len(common)))
    if not rows:
        return []
    rows.sort()
    mx = max(c for _, _, c in rows)
    mn = int(np.float32(mx) * np.float32(0.8))
    scored = [k for _, k, c in rows if c > mn]
    listed = {k for _, k, _ in rows}
    assert listed == set(scored) or not any(set(seq.covis.get(k, [])) & (listed - set(scored)) for k in scored)
    sc = {k: PR.score(PR.Frame(0, qw, qv), PR.Frame(0, *seq.vectors[k])) for k in scored}
    entries = []
    for k in scored:
        acc, best = sc[k], k
        for n in seq.covis.get(k, []):
            if n in sc:
                acc = np.float32(acc + sc[n])
                if sc[n] > sc[best]:
                    best = n
        entries.append((acc, best))
    top = max([a for a, _ in entries] + [np.float32(0)])
    kept = [b for a, b in entries if a > np.float32(0.75) * top]
    return list(dict.fromkeys(kept))


@pytest.mark.parametrize("name", PC.STATELESS)
def test_stateless_cases_against_set_formulation(name):
    r = PC.replay(name)
    assert r["steps"][0]["cands"][0].tolist() == set_based_reloc(r["case"], 0)
