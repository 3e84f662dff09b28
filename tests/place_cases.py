"""Named cases of the place-recognition entries (tests only): BowVectors written directly, run through the literal
referee of place_ref.py.  replay(name) gives the packed tables as the C ABI takes them and, per step of the case, the
problems, the wanted result records, candidates and score tables.  tests/test_place_host.py guards that each case
reaches what its name claims; tests/test_gpu_place.py holds the device to these bytes.

A case is dict(seqs=[Seq], frames=[(words, values)], steps=[...], cap, fcap).  A step is one call, or one flip of
in_db:
  ("reloc", [(seq, frame slot), ...])          ("min", [(seq, query keyframe), ...], use_bad)
  ("loop", [(seq, query keyframe), ...], min_scores or None: the values the previous "min" step left)
  ("add", seq, keyframe)                       ("erase", seq, keyframe)
"""
import functools
import time

import numpy as np

import place_ref as PR
from matcher_ref import f32

SENT = 0xEE
SENT_F = float(np.frombuffer(bytes([SENT] * 4), np.float32)[0])
BEST = 10
GAP = 3          # unwritten candidate slots between two problems' outputs

PROBLEM_DTYPE = np.dtype([("kf_base", "<i4"), ("n_kf", "<i4"), ("query", "<i4"), ("out_offset", "<i4")])
RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_sharing", "<i4"), ("max_common_words", "<i4"),
                         ("min_common_words", "<i4"), ("n_scored", "<i4"), ("n_kept", "<i4"),
                         ("n_candidates", "<i4"), ("best_acc_score", "<f4")])


def vec(words, values=None, seed=0):
    """A BowVector: sorted unique words; values given, or positive and L1-normalised."""
    if values is not None:
        assert all(a < b for a, b in zip(words, list(words)[1:])), "given values need ascending words"
    words = np.array(sorted(set(int(w) for w in words)), np.uint32)
    if values is None:
        r = np.random.default_rng(seed + 7 * len(words)).uniform(0.5, 1.5, len(words))
        values = r / r.sum() if len(words) else r
    values = np.array(values, np.float64)
    assert len(values) == len(words) and (values > 0).all() and (words <= 999999).all()
    return words, values


class Seq:
    """One sequence's fixture.  covis: {kf: neighbours} (rows -1 padded); connected: {kf: {other: weight}};
    ordered: {kf: list}; in_db: flags (default all set); bad: keyframes flagged in kf_bad."""

    def __init__(self, vectors, in_db=None, covis=None, connected=None, ordered=None, bad=(), score0=0.0):
        self.vectors = vectors
        self.n_kf = len(vectors)
        self.in_db = [True] * self.n_kf if in_db is None else [bool(x) for x in in_db]
        self.covis = covis or {}
        self.connected = connected or {}
        self.ordered = ordered or {}
        self.bad = set(bad)
        self.score0 = score0


# ---------------------------------------------------------------- builders
def _kf(shared, private_base, n_private=3, seed=0):
    """A keyframe vector: the given shared words and a few words nobody else has."""
    return vec(list(shared) + [private_base + i for i in range(n_private)], seed=seed)


def _empty_db():
    seqs = [Seq([_kf([10, 20], 1000), _kf([10], 2000), _kf([20], 3000)], in_db=[0, 0, 0])]
    return dict(seqs=seqs, frames=[vec([10, 20, 30])], steps=[("reloc", [(0, 0)])])


def _no_shared_word():
    vs = [_kf([10, 20], 1000), _kf([30], 2000), _kf([40, 50], 3000), vec([60, 70, 80])]
    seqs = [Seq(vs, in_db=[1, 1, 1, 0], covis={0: [1, 2], 1: [0]}, score0=SENT_F)]
    return dict(seqs=seqs, frames=[vec([5, 15, 25, 999999])], steps=[("reloc", [(0, 0)]), ("loop", [(0, 3)], [0.1])])


def _one_keyframe():
    seqs = [Seq([_kf([10, 20], 1000)])]
    return dict(seqs=seqs, frames=[vec([10, 20, 30])], steps=[("reloc", [(0, 0)]), ("min", [(0, 0)], True)])


def _same_score_kf(word, base):
    # one shared word of value 0.25 beside three private ones: every such keyframe scores the same
    return vec([word, base, base + 1, base + 2], [0.25, 0.25, 0.25, 0.25])


def _first_seen_order():
    q = vec([10, 20, 30, 40], [0.25] * 4)
    seqs = [Seq([_same_score_kf(40, 1000), _same_score_kf(30, 2000), _same_score_kf(10, 3000),
                 _same_score_kf(20, 4000)])]
    return dict(seqs=seqs, frames=[q], steps=[("reloc", [(0, 0)])], want_order=[2, 3, 1, 0])


def _equal_first_words():
    q = vec([10, 20, 30], [0.25, 0.25, 0.5])
    seqs = [Seq([_same_score_kf(10, 1000), _same_score_kf(20, 2000), _same_score_kf(10, 3000)])]
    return dict(seqs=seqs, frames=[q], steps=[("reloc", [(0, 0)])], want_order=[0, 2, 1])


def _threshold(max_common):
    """Keyframes with max, min_common_words, min + 1 and 1 common words (those that differ and are >= 1)."""
    mn = int(f32(max_common) * f32(0.8))
    counts = [max_common] + [c for c in (mn, mn + 1, 1) if 1 <= c < max_common]
    counts = sorted(set(counts), reverse=True)
    qwords = [100 + 10 * i for i in range(max_common)]
    vs = [_kf(qwords[:c], 1000 * (k + 1), seed=k) for k, c in enumerate(counts)]
    return dict(seqs=[Seq(vs)], frames=[vec(qwords + [5000, 5001])], steps=[("reloc", [(0, 0)])], counts=counts,
                min_common=mn)


def _retain_tie():
    # scores are sum min(vi, wi): 1.0 and 0.75, so acc of keyframe 1 == 0.75f * best exactly
    q = vec([10, 20], [1.0, 1.0])
    seqs = [Seq([vec([10, 1000], [1.0, 0.5]), vec([20, 2000], [0.75, 0.5]), vec([20, 3000], [0.8125, 0.5])])]
    return dict(seqs=seqs, frames=[q], steps=[("reloc", [(0, 0)])], want_order=[0, 2])


def _best_tie():
    # keyframe 0's neighbour 1 scores the same 0.5: it does not take over
    q = vec([10, 20], [1.0, 1.0])
    seqs = [Seq([vec([10, 1000], [0.5, 0.5]), vec([10, 2000], [0.5, 0.25])], covis={0: [1]})]
    return dict(seqs=seqs, frames=[q], steps=[("reloc", [(0, 0)])], want_order=[0])


def _same_best():
    # keyframes 0 and 1 both name their neighbour 2 (the higher score) and 2's own entry names itself: three kept
    # entries, one candidate, at the first one's place; keyframe 3's entry is not kept
    q = vec([10, 20, 30], [1.0, 1.0, 1.0])
    seqs = [Seq([vec([10, 1000], [0.25, 0.5]), vec([20, 2000], [0.25, 0.5]), vec([30, 3000], [0.875, 0.5]),
                 vec([10, 4000], [0.5, 0.5])], covis={0: [-1, 2], 1: [2], 3: []})]
    return dict(seqs=seqs, frames=[q], steps=[("reloc", [(0, 0)])], want_order=[2])


def _stale(three):
    """Query A scores keyframe 2 high.  Query B shares ten words with keyframe 0 and one with 2: 2 is in B's list,
    unscored, and adds what A left to 0's acc as 0's neighbour -- and, being greater, becomes a best keyframe that B
    did not score.  Query C (three): keyframe 3 likewise unscored beside 1, never scored before: it adds the
    initial 0."""
    wa = [100 + i for i in range(5)]
    wb = [200 + i for i in range(10)]
    wc = [300 + i for i in range(10)]
    vs = [vec(wb + [1000], [0.01] * 10 + [0.9]), vec(wc + [2000], [0.05] * 11), vec(wa + [wb[0], 3000], [0.15] * 7),
          vec([wc[0], 4000], [0.5, 0.5])]
    seqs = [Seq(vs, covis={0: [2], 1: [3, 0]})]
    frames = [vec(wa, [0.2] * 5), vec(wb, [0.1] * 10), vec(wc, [0.1] * 10)]
    steps = [("reloc", [(0, 0)]), ("reloc", [(0, 1)])] + ([("reloc", [(0, 2)])] if three else [])
    return dict(seqs=seqs, frames=frames, steps=steps)


def _loop_story(min_scores, chained=False, use_bad=True):
    """Query keyframe 9.  8 and 7 are connected and share most of its words; 0 .. 5 are in the database:
    0 scores high; 1 is scored below min_score and is 0's neighbour (it still feeds acc); 8 stands in 0's covis row
    too (connected: adds nothing); 2 shares too few words; 3 scores high and names 0 (higher) as best; 6 is not in
    the database and stands in 3's row."""
    w = [100 + i for i in range(10)]
    vs = [vec(w[:10] + [1000], [0.08] * 10 + [0.2]),      # 0: ten common words, score 0.8
          vec(w[:9] + [2000], [0.001] * 9 + [0.991]),     # 1: nine words, score 0.009
          vec(w[:3] + [3000], [0.1] * 3 + [0.7]),         # 2: three words: unscored
          vec(w[:10] + [4000], [0.05] * 10 + [0.5]),      # 3: score 0.5
          vec([5000, 5001]),                              # 4: nothing shared
          vec(w[:9] + [6000], [0.03] * 9 + [0.73]),       # 5: score 0.27
          vec(w[:10] + [7000], [0.09] * 10 + [0.1]),      # 6: not in the database
          vec(w[:10] + [8000], [0.02] * 10 + [0.8]),      # 7: connected, bad: score 0.2
          vec(w[:10] + [9000], [0.1] * 10 + [2e-3]),      # 8: connected
          vec(w, [0.1] * 10)]                             # 9: the query
    seqs = [Seq(vs, in_db=[1, 1, 1, 1, 1, 1, 0, 1, 1, 0], covis={0: [8, 1, -1, 2], 3: [6, 0], 5: [4]},
                connected={9: {8: 40, 7: 21}}, ordered={9: [8, 7, 5]}, bad=[7])]
    steps = ([("min", [(0, 9)], use_bad)] if chained else []) + [("loop", [(0, 9)], None if chained else min_scores)]
    return dict(seqs=seqs, frames=[], steps=steps)


def _erased_middle():
    """Keyframes 2 and 3 of six leave the database between two queries, then 5 (the newest) enters it: the list
    order stays index order.  Keyframe 4's neighbour 3 is then outside the database."""
    q = vec([10, 20], [0.5, 0.5])
    vs = [_same_score_kf(20, 1000), _same_score_kf(10, 2000), _same_score_kf(10, 3000), _same_score_kf(10, 4000),
          _same_score_kf(20, 5000), _same_score_kf(10, 6000)]
    seqs = [Seq(vs, in_db=[1, 1, 1, 1, 1, 0], covis={4: [3, -1, 5], 1: [2]})]
    steps = [("reloc", [(0, 0)]), ("erase", 0, 2), ("erase", 0, 3), ("reloc", [(0, 0)]), ("add", 0, 5),
             ("reloc", [(0, 0)])]
    return dict(seqs=seqs, frames=[q], steps=steps)


def random_seq(n_kf, seed, len_lo, len_hi, pool_size=400, window=60):
    """A sequence with locality: keyframe k draws its words from a window of the pool that moves with k, so
    neighbours share many words and far keyframes few.  Random covis rows (-1 padded, some out of the database),
    connections, ordered lists and bad flags."""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(1000000, pool_size, replace=False))
    vectors = []
    for k in range(n_kf):
        c = int(k / max(n_kf - 1, 1) * (pool_size - 1))
        lo, hi = max(0, c - window), min(pool_size, c + window)
        n = int(rng.integers(len_lo, len_hi + 1))
        idx = rng.choice(np.arange(lo, hi), min(n, hi - lo), replace=False)
        vectors.append(vec(pool[idx], seed=seed + k))
    in_db = rng.random(n_kf) < 0.85
    covis, connected, ordered = {}, {}, {}
    for k in range(n_kf):
        near = [j for j in range(max(0, k - 12), min(n_kf, k + 13)) if j != k]
        if near and rng.random() < 0.8:
            row = list(rng.choice(near, min(len(near), int(rng.integers(1, BEST + 1))), replace=False))
            if rng.random() < 0.3:
                row.insert(int(rng.integers(0, len(row) + 1)), -1)
            covis[k] = [int(x) for x in row[:BEST]]
        conn = {j: int(rng.integers(15, 90)) for j in near if abs(j - k) <= 3 and rng.random() < 0.8}
        connected[k] = conn
        ordered[k] = sorted(conn, key=lambda j: (-conn[j], -j))
    bad = [k for k in range(n_kf) if rng.random() < 0.1]
    return Seq(vectors, in_db=in_db, covis=covis, connected=connected, ordered=ordered, bad=bad), pool, rng


def query_near(seq, pool, rng, k, n_words):
    """A frame's vector that resembles keyframe k's: part of its words and some others of the pool."""
    kw = seq.vectors[k][0]
    take = rng.choice(kw, min(len(kw), max(1, (2 * n_words) // 3)), replace=False) if len(kw) else kw
    rest = rng.choice(pool, max(n_words - len(take), 0), replace=False)
    return vec(list(take) + list(rest), seed=int(rng.integers(1 << 20)))


def _sized(n_kf, seed, len_lo=20, len_hi=64):
    seq, pool, rng = random_seq(n_kf, seed, len_lo, len_hi)
    qa, qb = n_kf // 2, n_kf - 1
    seq.in_db[qa] = seq.in_db[qb] = False
    frames = [query_near(seq, pool, rng, n_kf // 3, 48), query_near(seq, pool, rng, (2 * n_kf) // 3, 30)]
    # adds are in keyframe order, as DetectLoop makes them: only the newest keyframe enters the database
    steps = [("reloc", [(0, 0)]), ("min", [(0, qa)], True), ("loop", [(0, qa)], None), ("reloc", [(0, 1)]),
             ("erase", 0, n_kf // 3), ("reloc", [(0, 0)]), ("min", [(0, qb)], False), ("loop", [(0, qb)], None),
             ("add", 0, qb), ("reloc", [(0, 1)])]
    if n_kf == 1:
        steps = [("reloc", [(0, 0)]), ("min", [(0, 0)], True), ("loop", [(0, 0)], None)]
    return dict(seqs=[seq], frames=frames, steps=steps)


LENGTHS = (0, 1, 63, 64, 65, 1000, 1100)
LENGTHS_CAP = 1100


def _vector_lengths():
    """Keyframe vectors of every length at which the 64-word chunks of the walk change, up to cap; queries shorter
    and longer than the keyframes' vectors, and one of cap words as a loop query."""
    rng = np.random.default_rng(77)
    pool = np.sort(rng.choice(1000000, 3000, replace=False))
    vs = [vec(rng.choice(pool, n, replace=False), seed=n) for n in LENGTHS] + \
         [vec(rng.choice(pool, n, replace=False), seed=n + 1) for n in (LENGTHS_CAP, 500)]
    n_kf = len(vs)
    covis = {k: [(k + 1) % n_kf, (k + 3) % n_kf] for k in range(n_kf)}
    seqs = [Seq(vs, in_db=[1] * (n_kf - 2) + [0, 1], covis=covis, ordered={n_kf - 2: list(range(n_kf - 2))},
                bad=[3])]
    frames = [vec(rng.choice(pool, 64, replace=False), seed=1), vec(rng.choice(pool, LENGTHS_CAP, replace=False), seed=2),
              vec(rng.choice(pool, 1, replace=False), seed=3)]
    steps = [("reloc", [(0, 0)]), ("reloc", [(0, 1)]), ("reloc", [(0, 2)]), ("min", [(0, n_kf - 2)], True),
             ("loop", [(0, n_kf - 2)], None)]
    return dict(seqs=seqs, frames=frames, steps=steps, cap=LENGTHS_CAP, fcap=LENGTHS_CAP)


def _two_sequences():
    a, pool_a, rng_a = random_seq(37, 5, 20, 50)
    b, pool_b, rng_b = random_seq(70, 6, 10, 64)
    a.in_db[36] = a.in_db[20] = b.in_db[40] = False
    frames = [query_near(b, pool_b, rng_b, 20, 40), query_near(a, pool_a, rng_a, 10, 40),
              query_near(a, pool_a, rng_a, 30, 25)]
    steps = [("reloc", [(0, 1), (1, 0)]), ("min", [(1, 40), (0, 36)], True), ("loop", [(1, 40), (0, 36)], None),
             ("reloc", [(1, 0), (0, 2)]), ("loop", [(0, 20)], [0.05])]
    return dict(seqs=[a, b], frames=frames, steps=steps)


# ---- summation order
def _terms(q, k):
    """The score's terms of two vectors over the same words, in word order."""
    return [abs(vi - wi) - abs(vi) - abs(wi) for vi, wi in zip(q, k)]


def _serial(t):
    s = 0.0
    for x in t:
        s += x
    return s


def _pairwise(t):
    t = list(t)
    while len(t) > 1:
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0]


def order_scores(q, k):
    """The float score under the serial sum, the reversed sum and a pairwise tree sum."""
    t = _terms(q, k)
    return tuple(f32(-s / 2.0) for s in (_serial(t), _serial(t[::-1]), _pairwise(t)))


@functools.lru_cache(None)
def order_sensitive_vectors(n=40):
    """A seeded search: unnormalised values log-uniform over 1e-8 .. 1, the last pair chosen so that the score lies
    on the midpoint of two floats to within the sum's rounding error, until the serial sum's float differs from the
    reversed sum's and from the pairwise sum's."""
    for seed in range(4000):
        rng = np.random.default_rng(seed)
        q = list(10.0 ** rng.uniform(-8, 0, n))
        k = list(10.0 ** rng.uniform(-8, 0, n))
        q[-1] = 1.0
        base = -_serial(_terms(q[:-1], k[:-1])) / 2.0
        lo = float(f32(base))
        if lo <= base:
            lo = float(np.nextafter(f32(lo), f32(np.inf)))
        mid = (lo + float(np.nextafter(f32(lo), f32(np.inf)))) / 2.0
        x = mid - base                                   # the last term is about -2 min(1, x)
        if not 1e-8 <= x <= 1.0:
            continue
        for nudge in range(-6, 7):
            k[-1] = x * (1.0 + nudge * 2.0 ** -30)
            s, r, pw = order_scores(q, k)
            if s != r and s != pw:
                return np.array(q), np.array(k)
    raise AssertionError("no order-sensitive vectors found")


def _summation_order():
    q, k = order_sensitive_vectors()
    words = [1000 * (i + 1) for i in range(len(q))]
    seqs = [Seq([vec(words, k), vec(words[:38] + [999999], list(k[:38]) + [0.5])], covis={0: [1]},
                ordered={1: [0]})]
    return dict(seqs=seqs, frames=[vec(words, q)], steps=[("reloc", [(0, 0)]), ("min", [(0, 1)], False)])


VOCAB_KFS = 12


@functools.lru_cache(None)
def _vocabulary_vectors():
    import bow_common
    voc = bow_common.PyVocab(bow_common.vocab_text())
    out = []
    for _, desc in bow_common.frames(VOCAB_KFS + 1, step=4):
        t = voc.transform(desc)
        out.append((t["words"], t["values"]))
    return out


def _vocabulary():
    """Twelve synthetic keyframes and one more frame of the same sequence through the in-repo vocabulary."""
    vs = _vocabulary_vectors()
    n = VOCAB_KFS
    covis = {k: [j for j in (k - 1, k + 1, k - 2, k + 2) if 0 <= j < n] for k in range(n)}
    connected = {n - 1: {n - 2: 60, n - 3: 30}}
    seqs = [Seq(list(vs[:n]), in_db=[1] * (n - 1) + [0], covis=covis, connected=connected,
                ordered={n - 1: [n - 2, n - 3]})]
    steps = [("reloc", [(0, 0)]), ("min", [(0, n - 1)], False), ("loop", [(0, n - 1)], None)]
    return dict(seqs=seqs, frames=[vs[n]], steps=steps, cap=1024, fcap=1024)


CASES = {
    "empty_db": _empty_db,
    "no_shared_word": _no_shared_word,
    "one_keyframe": _one_keyframe,
    "first_seen_order": _first_seen_order,
    "equal_first_words": _equal_first_words,
    "max_common_1": lambda: _threshold(1),
    "max_common_4": lambda: _threshold(4),
    "max_common_5": lambda: _threshold(5),
    "max_common_10": lambda: _threshold(10),
    "retain_tie": _retain_tie,
    "best_tie": _best_tie,
    "same_best": _same_best,
    "stale_two": lambda: _stale(False),
    "stale_three": lambda: _stale(True),
    "loop_story": lambda: _loop_story([0.25]),
    "loop_all_below": lambda: _loop_story([0.9]),
    "loop_chained_bad": lambda: _loop_story(None, chained=True, use_bad=True),
    "loop_chained_no_bad": lambda: _loop_story(None, chained=True, use_bad=False),
    "erased_middle": _erased_middle,
    "n_kf_1": lambda: _sized(1, 11),
    "n_kf_63": lambda: _sized(63, 12),
    "n_kf_64": lambda: _sized(64, 13),
    "n_kf_65": lambda: _sized(65, 14),
    "n_kf_1024": lambda: _sized(1024, 15),
    "vector_lengths": _vector_lengths,
    "two_sequences": _two_sequences,
    "summation_order": _summation_order,
    "vocabulary": _vocabulary,
}
# the cases whose every step is one problem of one sequence: the host forms take them
SINGLE = [n for n in CASES if n != "two_sequences"]
# relocalization cases whose queries read no state an earlier query left: a stateless formulation decides them
STATELESS = ["empty_db", "first_seen_order", "equal_first_words", "max_common_1", "max_common_4", "max_common_5",
             "max_common_10", "retain_tie", "best_tie", "same_best", "summation_order"]


# ---------------------------------------------------------------- replay
def pack(case):
    """The tables of the C ABI, the sequences one after the other."""
    seqs = case["seqs"]
    cap = case.get("cap") or max([len(w) for s in seqs for w, _ in s.vectors] + [1])
    fcap = case.get("fcap") or max([len(w) for w, _ in case["frames"]] + [1])
    n_total = sum(s.n_kf for s in seqs)
    stride = max(s.n_kf for s in seqs) + 2
    kf_base = np.cumsum([0] + [s.n_kf for s in seqs])[:-1].tolist()
    t = dict(bow_words=np.zeros((n_total, cap), np.uint32), bow_values=np.zeros((n_total, cap), np.float64),
             n_bow=np.zeros(n_total, np.int32), in_db=np.zeros(n_total, np.uint8),
             reloc_score=np.zeros(n_total, np.float32), loop_score=np.zeros(n_total, np.float32),
             covis=np.full((n_total, BEST), -1, np.int32), weights=np.zeros((n_total, stride), np.int32),
             ordered=np.full((n_total, stride), -7, np.int32), n_ordered=np.zeros(n_total, np.int32),
             kf_bad=np.zeros(n_total, np.uint8))
    for s, b in zip(seqs, kf_base):
        for k, (w, v) in enumerate(s.vectors):
            t["bow_words"][b + k, :len(w)] = w
            t["bow_values"][b + k, :len(w)] = v
            t["n_bow"][b + k] = len(w)
        t["in_db"][b:b + s.n_kf] = s.in_db
        t["reloc_score"][b:b + s.n_kf] = t["loop_score"][b:b + s.n_kf] = np.float32(s.score0)
        for k, row in s.covis.items():
            t["covis"][b + k, :len(row)] = row
        for k, conn in s.connected.items():
            for j, wgt in conn.items():
                t["weights"][b + k, j] = wgt
        for k, lst in s.ordered.items():
            t["ordered"][b + k, :len(lst)] = lst
            t["n_ordered"][b + k] = len(lst)
        t["kf_bad"][b + np.array(sorted(s.bad), int)] = 1
    f = dict(bow_words=np.zeros((max(len(case["frames"]), 1), fcap), np.uint32),
             bow_values=np.zeros((max(len(case["frames"]), 1), fcap), np.float64),
             n_bow=np.zeros(max(len(case["frames"]), 1), np.int32))
    for i, (w, v) in enumerate(case["frames"]):
        f["bow_words"][i, :len(w)] = w
        f["bow_values"][i, :len(w)] = v
        f["n_bow"][i] = len(w)
    return dict(t=t, f=f, cap=cap, fcap=fcap, stride=stride, kf_base=kf_base, n_total=n_total)


class Referee:
    """The reference's objects of one case: per sequence a KeyFrameDatabase and its KeyFrames."""

    def __init__(self, case):
        self.dbs, self.kfs = [], []
        for s in case["seqs"]:
            kfs = [PR.KeyFrame(k, w, v, s.score0) for k, (w, v) in enumerate(s.vectors)]
            for k, kf in enumerate(kfs):
                kf.connected = set(s.connected.get(k, {}))
                kf.best_covisibles = [kfs[j] for j in s.covis.get(k, []) if j >= 0]
                kf.ordered = [kfs[j] for j in s.ordered.get(k, [])]
                kf.bad = k in s.bad
            db = PR.KeyFrameDatabase()
            for k, kf in enumerate(kfs):                       # DetectLoop adds in mnId order
                if s.in_db[k]:
                    db.add(kf)
            self.dbs.append(db)
            self.kfs.append(kfs)


@functools.lru_cache(None)
def replay(name):
    """run() of a named case, computed once and shared: the tests leave it unchanged."""
    return run(CASES[name]())


def run(case):
    """The case through the referee.  Returns dict(case, packed, steps): per call step its kind, problems, the
    wanted records and candidates (per problem), min_in (the min scores given, None: chained), want_min, use_bad,
    the referee's time and the tables after it (reloc_score, loop_score, in_db); per flip step kind, index
    (absolute) and value."""
    packed = pack(case)
    ref = Referee(case)
    stats = {}
    reloc = packed["t"]["reloc_score"].copy()
    loop = packed["t"]["loop_score"].copy()
    in_db = packed["t"]["in_db"].copy()
    last_min, frame_id, steps = None, 0, []
    for step in case["steps"]:
        kind = step[0]
        if kind in ("add", "erase"):
            _, s, k = step
            (ref.dbs[s].add if kind == "add" else ref.dbs[s].erase)(ref.kfs[s][k])
            in_db[packed["kf_base"][s] + k] = kind == "add"
            steps.append(dict(kind=kind, index=packed["kf_base"][s] + k, value=int(kind == "add"),
                              in_db=in_db.copy()))
            continue
        probs = step[1]
        t0 = time.perf_counter()
        problems = np.zeros(len(probs), PROBLEM_DTYPE)
        records, cands, mins, off = [], [], [], 2
        min_in = None
        if kind == "loop":
            min_in = last_min if step[2] is None else np.array(step[2], np.float32)
            assert min_in is not None and len(min_in) == len(probs)
        for i, (s, q) in enumerate(probs):
            n_kf, b = case["seqs"][s].n_kf, packed["kf_base"][s]
            problems[i] = (b, n_kf, q, off)
            off += n_kf + GAP
            st = stats.setdefault(len(steps), {})
            if kind == "reloc":
                frame_id += 1
                out, rec = ref.dbs[s].detect_relocalization_candidates(
                    PR.Frame(frame_id, *case["frames"][q]), st)
            elif kind == "loop":
                out, rec = ref.dbs[s].detect_loop_candidates(ref.kfs[s][q], min_in[i], st)
            else:
                saved = [kf.bad for kf in ref.kfs[s]]
                if not step[2]:
                    for kf in ref.kfs[s]:
                        kf.bad = False
                mins.append(PR.loop_min_score(ref.kfs[s][q]))
                for kf, was in zip(ref.kfs[s], saved):
                    kf.bad = was
                continue
            records.append(rec)
            cands.append(np.array([kf.mnId for kf in out], np.int32))
            for k, kf in enumerate(ref.kfs[s]):
                reloc[b + k], loop[b + k] = kf.mRelocScore, kf.mLoopScore
        if kind == "min":
            last_min = np.array(mins, np.float32)
        steps.append(dict(kind=kind, problems=problems, n_out=off,
                          want=np.array(records, RESULT_DTYPE) if records else None, cands=cands, min_in=min_in,
                          chained=kind == "loop" and step[2] is None,
                          want_min=last_min.copy() if kind == "min" else None,
                          use_bad=kind == "min" and bool(step[2]), ref_ms=(time.perf_counter() - t0) * 1e3,
                          reloc_score=reloc.copy(), loop_score=loop.copy(),
                          in_db=in_db.copy()))
    return dict(case=case, packed=packed, steps=steps, stats=stats)
