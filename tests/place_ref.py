"""Literal Python restatement of the reference's place recognition (tests only): KeyFrameDatabase::add / erase /
DetectLoopCandidates / DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:40-67, :76-197, :199-309), the
reference score of LoopClosing::DetectLoop (src/LoopClosing.cc:126-140) and L1Scoring::score
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  Mutable state as the reference has it: an inverted file of
per-word lists, and per keyframe the query stamps, word counters and scores.  Deliberately not the dense,
keyframe-major formulation of place_kernels.hip.  float is numpy float32 (matcher_ref.f32), double is Python's.

One departure, the one include/spslam_gpu.h states: the stamps mnRelocQuery / mnLoopQuery start at -1 here, not 0,
so a query whose id is 0 is not mistaken for "already seen".  The scores start at 0 where the reference leaves them
uninitialised, or at the value a case gives."""
import bisect

from matcher_ref import f32

OK, EMPTY, NONE_KEPT = 0, 1, 2


class KeyFrame:
    def __init__(self, mn_id, words, values, score0=0.0):
        self.mnId = mn_id
        self.words = [int(w) for w in words]          # mBowVec: a std::map, ascending word id
        self.values = [float(v) for v in values]
        self.mnRelocQuery, self.mnRelocWords, self.mRelocScore = -1, 0, f32(score0)
        self.mnLoopQuery, self.mnLoopWords, self.mLoopScore = -1, 0, f32(score0)
        self.connected = set()                        # GetConnectedKeyFrames(): mnIds
        self.best_covisibles = []                     # GetBestCovisibilityKeyFrames(10): KeyFrames
        self.ordered = []                             # GetVectorCovisibleKeyFrames(): KeyFrames
        self.bad = False


class Frame:
    def __init__(self, mn_id, words, values):
        self.mnId = mn_id
        self.words = [int(w) for w in words]
        self.values = [float(v) for v in values]


def score(v1, v2, stats=None):
    """L1Scoring::score, with the lower_bound jumps; then the float the callers store it in."""
    i, j, n1, n2 = 0, 0, len(v1.words), len(v2.words)
    s = 0.0
    while i != n1 and j != n2:
        vi, wi = v1.values[i], v2.values[j]
        if v1.words[i] == v2.words[j]:
            s += abs(vi - wi) - abs(vi) - abs(wi)
            if stats is not None:
                stats.setdefault("terms", []).append(abs(vi - wi) - abs(vi) - abs(wi))
            i += 1
            j += 1
        elif v1.words[i] < v2.words[j]:
            i = bisect.bisect_left(v1.words, v2.words[j])
        else:
            j = bisect.bisect_left(v2.words, v1.words[i])
    s = -s / 2.0
    return f32(s)


class KeyFrameDatabase:
    def __init__(self):
        self.mvInvertedFile = {}

    def add(self, kf):
        for w in kf.words:
            self.mvInvertedFile.setdefault(w, []).append(kf)

    def erase(self, kf):
        for w in kf.words:
            lst = self.mvInvertedFile.get(w, [])
            for k, other in enumerate(lst):
                if other is kf:
                    del lst[k]
                    break

    def detect_relocalization_candidates(self, F, stats=None):
        """Returns (candidates, record) with record = (status, n_sharing, max_common_words, min_common_words,
        n_scored, n_kept, n_candidates, best_acc_score)."""
        sharing = []
        for w in F.words:
            for kfi in self.mvInvertedFile.get(w, []):
                if kfi.mnRelocQuery != F.mnId:
                    kfi.mnRelocWords = 0
                    kfi.mnRelocQuery = F.mnId
                    sharing.append(kfi)
                kfi.mnRelocWords += 1
        if not sharing:
            return [], (EMPTY, 0, 0, 0, 0, 0, 0, f32(0))
        max_common = 0
        for kfi in sharing:
            if kfi.mnRelocWords > max_common:
                max_common = kfi.mnRelocWords
        min_common = int(f32(max_common) * f32(0.8))
        score_and_match = []
        nscores = 0
        for kfi in sharing:
            if kfi.mnRelocWords > min_common:
                nscores += 1
                si = score(F, kfi)
                kfi.mRelocScore = si
                score_and_match.append((si, kfi))
        if not score_and_match:
            return [], (NONE_KEPT, len(sharing), max_common, min_common, nscores, 0, 0, f32(0))
        acc_and_match = []
        best_acc = f32(0)
        scored_now = {id(k) for _, k in score_and_match}
        for si, kfi in score_and_match:
            best_score, acc, best_kf = si, si, kfi
            for kf2 in kfi.best_covisibles:
                if kf2.mnRelocQuery != F.mnId:
                    continue
                if stats is not None and id(kf2) not in scored_now:
                    stats.setdefault("stale_reads", []).append((kfi.mnId, kf2.mnId, float(kf2.mRelocScore)))
                acc = f32(acc + kf2.mRelocScore)
                if kf2.mRelocScore > best_score:
                    best_kf = kf2
                    best_score = kf2.mRelocScore
                elif stats is not None and kf2.mRelocScore == best_score:
                    stats.setdefault("best_ties", []).append((kfi.mnId, kf2.mnId))
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_and_match, best_acc, len(sharing), max_common, min_common, nscores,
                            len(score_and_match), stats)

    def detect_loop_candidates(self, kf, min_score, stats=None):
        min_score = f32(min_score)
        sharing = []
        for w in kf.words:
            for kfi in self.mvInvertedFile.get(w, []):
                if kfi.mnLoopQuery != kf.mnId:
                    kfi.mnLoopWords = 0
                    if kfi.mnId not in kf.connected:
                        kfi.mnLoopQuery = kf.mnId
                        sharing.append(kfi)
                    elif stats is not None:
                        stats.setdefault("connected_hits", set()).add(kfi.mnId)
                kfi.mnLoopWords += 1
        if not sharing:
            return [], (EMPTY, 0, 0, 0, 0, 0, 0, f32(0))
        max_common = 0
        for kfi in sharing:
            if kfi.mnLoopWords > max_common:
                max_common = kfi.mnLoopWords
        min_common = int(f32(max_common) * f32(0.8))
        score_and_match = []
        nscores = 0
        for kfi in sharing:
            if kfi.mnLoopWords > min_common:
                nscores += 1
                si = score(kf, kfi)
                kfi.mLoopScore = si
                if si >= min_score:
                    score_and_match.append((si, kfi))
        if not score_and_match:
            return [], (NONE_KEPT, len(sharing), max_common, min_common, nscores, 0, 0, min_score)
        acc_and_match = []
        best_acc = min_score
        kept_now = {id(k) for _, k in score_and_match}
        for si, kfi in score_and_match:
            best_score, acc, best_kf = si, si, kfi
            for kf2 in kfi.best_covisibles:
                if kf2.mnLoopQuery == kf.mnId and kf2.mnLoopWords > min_common:
                    if stats is not None and id(kf2) not in kept_now:
                        stats.setdefault("below_min_feeds", []).append((kfi.mnId, kf2.mnId))
                    acc = f32(acc + kf2.mLoopScore)
                    if kf2.mLoopScore > best_score:
                        best_kf = kf2
                        best_score = kf2.mLoopScore
                elif stats is not None and kf2.mnId in kf.connected:
                    stats.setdefault("connected_neighbours", []).append((kfi.mnId, kf2.mnId))
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_and_match, best_acc, len(sharing), max_common, min_common, nscores,
                            len(score_and_match), stats)

    @staticmethod
    def _retain(acc_and_match, best_acc, n_sharing, max_common, min_common, nscores, n_kept, stats):
        """:175-196 and :289-308, the same text in both functions."""
        min_score_to_retain = f32(f32(0.75) * best_acc)
        already, out = set(), []
        for acc, kfi in acc_and_match:
            if stats is not None and acc == min_score_to_retain:
                stats.setdefault("retain_ties", []).append(kfi.mnId)
            if acc > min_score_to_retain:
                if id(kfi) not in already:
                    out.append(kfi)
                    already.add(id(kfi))
                elif stats is not None:
                    stats.setdefault("duplicates", []).append(kfi.mnId)
        return out, (OK, n_sharing, max_common, min_common, nscores, n_kept, len(out), best_acc)


def loop_min_score(kf):
    """LoopClosing.cc:126-140."""
    min_score = f32(1)
    for other in kf.ordered:
        if other.bad:
            continue
        s = score(kf, other)
        if s < min_score:
            min_score = s
    return min_score
