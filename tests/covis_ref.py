"""Scalar referees of the covisibility entries, written from the reference's text with real mutable state:
  KeyFrame::UpdateConnections / AddConnection / UpdateBestCovisibles   src/KeyFrame.cc:306-396, :128-162
  LocalMapping::KeyFrameCulling with KeyFrame::SetBadFlag's EraseObservation loop and MapPoint::EraseObservation /
  SetBadFlag                       src/LocalMapping.cc:644-711, src/KeyFrame.cc:470-488, src/MapPoint.cc:111-168
  LocalMapping::MapPointCulling    src/LocalMapping.cc:182-217
Keyframes are integers (the index in their sequence, 0 is mnId == 0) and ascending index stands for pointer order.
The culling referee erases observations, lowers nObs and removes bad points from the match lists as the reference
does; it has no notion of an "effective" observation count.  `stats` counts the branches taken."""
import collections

import numpy as np

UPDATED, EMPTY = 0, 1
KEPT, CULLED, DEFERRED, SKIPPED = range(4)
RAN, NEW_PLANE = 0, 1
POINT_KEEP, POINT_DROP, POINT_BAD_RATIO, POINT_BAD_OBS, POINT_EXPIRED = range(5)
TH = 15
TH_OBS = 3
BEST = 10


class Map:
    """One sequence's map as the reference holds it.  Per keyframe k: matches[k][i] = the point (row) of keypoint i
    or None (mvpMapPoints), uright / depth / octave per keypoint, new_plane, not_erase.  Per point r: obs[r] =
    {keyframe: keypoint} (mObservations), n_obs[r] (nObs), bad[r] (mbBad)."""

    def __init__(self, n_kf):
        self.n_kf = n_kf
        self.matches = [[] for _ in range(n_kf)]
        self.uright = [[] for _ in range(n_kf)]
        self.depth = [[] for _ in range(n_kf)]
        self.octave = [[] for _ in range(n_kf)]
        self.new_plane = [False] * n_kf
        self.not_erase = [False] * n_kf
        self.obs, self.n_obs, self.bad = [], [], []

    def add_keypoint(self, kf, row=None, octave=0, stereo=True, depth=1.0):
        """A keypoint of kf (uright >= 0 when stereo) holding `row` or nothing; returns its index."""
        self.matches[kf].append(row)
        self.uright[kf].append(10.0 if stereo else -1.0)
        self.depth[kf].append(depth)
        self.octave[kf].append(octave)
        return len(self.matches[kf]) - 1

    def add_point(self, observers, n_obs=None, bad=False):
        """A point seen by `observers`: keyframes, or {keyframe: dict(octave=, stereo=, depth=)}.  MapPoint::
        AddObservation's count (2 per stereo observation, else 1) unless n_obs is given.  bad: isBad() while the
        point still stands in the match lists (another thread's SetBadFlag under way)."""
        if not isinstance(observers, dict):
            observers = {k: {} for k in observers}
        row = len(self.obs)
        self.obs.append({})
        count = 0
        for k in sorted(observers):
            kw = observers[k]
            self.obs[row][k] = self.add_keypoint(k, row, **kw)
            count += 2 if kw.get("stereo", True) else 1
        self.n_obs.append(count if n_obs is None else n_obs)
        self.bad.append(bad)
        return row


class Graph:
    """The covisibility members of one sequence's keyframes."""

    def __init__(self, n_kf):
        self.weights = [dict() for _ in range(n_kf)]      # mConnectedKeyFrameWeights
        self.ordered = [[] for _ in range(n_kf)]          # mvpOrderedConnectedKeyFrames
        self.ordered_w = [[] for _ in range(n_kf)]        # mvOrderedWeights
        self.parent = [-1] * n_kf                         # mpParent
        self.children = [set() for _ in range(n_kf)]      # mspChildrens
        self.first_connection = [True] * n_kf             # mbFirstConnection


def _sorted_front(pairs):
    """sort(vPairs) then push_front of each: descending (weight, keyframe)."""
    pairs = sorted(pairs)
    kfs, ws = collections.deque(), collections.deque()
    for w, k in pairs:
        kfs.appendleft(k)
        ws.appendleft(w)
    return list(kfs), list(ws)


def update_best_covisibles(g, k):
    pairs = [(w, j) for j, w in sorted(g.weights[k].items())]
    g.ordered[k], g.ordered_w[k] = _sorted_front(pairs)


def add_connection(g, k, other, weight, stats=None):
    """KeyFrame k's AddConnection(other, weight); True when UpdateBestCovisibles ran."""
    if other not in g.weights[k]:
        g.weights[k][other] = weight
    elif g.weights[k][other] != weight:
        g.weights[k][other] = weight
    else:
        if stats is not None:
            stats["unchanged_weight"] += 1
        return False
    update_best_covisibles(g, k)
    return True


def update_connections(m, g, kf, th=TH, stats=None):
    """Returns (status, n_ordered, new_parent, n_resorted) and the keyframes whose ordered list was rewritten."""
    stats = collections.Counter() if stats is None else stats
    counter = {}
    for row in m.matches[kf]:
        if row is None:
            stats["null_row"] += 1
            continue
        if m.bad[row]:
            stats["bad_row"] += 1
            continue
        for j in sorted(m.obs[row]):
            if j == kf:
                stats["own_observation"] += 1
                continue
            counter[j] = counter.get(j, 0) + 1
    if not counter:
        stats["empty"] += 1
        return (EMPTY, 0, -1, 0), []
    nmax, kf_max = 0, None
    pairs, resorted = [], []
    for j in sorted(counter):
        if counter[j] > nmax:
            nmax, kf_max = counter[j], j
        if counter[j] >= th:
            pairs.append((counter[j], j))
            if add_connection(g, j, kf, counter[j], stats):
                resorted.append(j)
        else:
            stats["below_th"] += 1
    if not pairs:
        stats["only_maximum"] += 1
        pairs.append((nmax, kf_max))
        if add_connection(g, kf_max, kf, nmax, stats):
            resorted.append(kf_max)
    g.weights[kf] = dict(counter)
    g.ordered[kf], g.ordered_w[kf] = _sorted_front(pairs)
    new_parent = -1
    if g.first_connection[kf] and kf != 0:
        new_parent = g.parent[kf] = g.ordered[kf][0]
        g.children[new_parent].add(kf)
        g.first_connection[kf] = False
        stats["first_connection"] += 1
    return (UPDATED, len(pairs), new_parent, len(resorted)), [kf] + resorted


# ---------------------------------------------------------------- KeyFrameCulling
def set_point_bad(m, row):
    """MapPoint::SetBadFlag."""
    m.bad[row] = True
    obs, m.obs[row] = m.obs[row], {}
    for k, kp in obs.items():
        m.matches[k][kp] = None                           # EraseMapPointMatch


def erase_observation(m, row, kf, stats):
    """MapPoint::EraseObservation."""
    bad = False
    if kf in m.obs[row]:
        idx = m.obs[row][kf]
        if m.uright[kf][idx] >= 0:
            m.n_obs[row] -= 2
            stats["erased_stereo"] += 1
        else:
            m.n_obs[row] -= 1
            stats["erased_mono"] += 1
        del m.obs[row][kf]
        if m.n_obs[row] <= 2:
            bad = True
    if bad:
        stats["point_went_bad"] += 1
        set_point_bad(m, row)


def set_keyframe_bad(m, kf, stats):
    """KeyFrame::SetBadFlag as far as the culling loop can see it; False when mbNotErase defers it."""
    if kf == 0:
        return False
    if m.not_erase[kf]:
        return False                                      # mbToBeErased = true
    for row in list(m.matches[kf]):
        if row is not None:
            erase_observation(m, row, kf, stats)
    return True


def keyframe_culling(m, kf, ordered, th_depth, th_obs=TH_OBS, stats=None):
    """Mutates m.  Returns (records [(kf, n_mps, n_redundant, status)], problem status)."""
    stats = collections.Counter() if stats is None else stats
    if m.new_plane[kf]:
        stats["current_new_plane"] += 1
        return [], NEW_PLANE
    records = []
    for c in list(ordered):
        if c == 0 or m.new_plane[c]:
            stats["skipped_zero" if c == 0 else "skipped_new_plane"] += 1
            records.append((c, 0, 0, SKIPPED))
            continue
        n_red = n_mps = 0
        for i, row in enumerate(list(m.matches[c])):
            if row is None:
                continue
            if m.bad[row]:
                continue
            d = np.float32(m.depth[c][i])
            if d > np.float32(th_depth) or d < 0:
                stats["depth_far" if d > np.float32(th_depth) else "depth_negative"] += 1
                continue
            n_mps += 1
            if m.n_obs[row] > th_obs:
                level = m.octave[c][i]
                n = 0
                for j in sorted(m.obs[row]):
                    if j == c:
                        continue
                    if m.octave[j][m.obs[row][j]] <= level + 1:
                        n += 1
                        if n >= th_obs:
                            break
                    else:
                        stats["coarser_observer"] += 1
                if n >= th_obs:
                    n_red += 1
                else:
                    stats["too_few_observers"] += 1
            else:
                stats["few_observations"] += 1
        status = KEPT
        if float(n_red) > 0.9 * float(n_mps):
            status = CULLED if set_keyframe_bad(m, c, stats) else DEFERRED
        stats[("kept", "culled", "deferred")[status]] += 1
        records.append((c, n_mps, n_red, status))
    return records, RAN


# ---------------------------------------------------------------- MapPointCulling
def map_point_culling(found, visible, first_kf, bad, n_obs, rows, cur_kf_id, th_obs=TH_OBS):
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for r in rows:
            age = int(cur_kf_id) - int(first_kf[r])
            if bad[r]:
                out.append(POINT_DROP)
            elif np.float32(found[r]) / np.float32(visible[r]) < np.float32(0.25):
                out.append(POINT_BAD_RATIO)
            elif age >= 2 and n_obs[r] <= th_obs:
                out.append(POINT_BAD_OBS)
            elif age >= 3:
                out.append(POINT_EXPIRED)
            else:
                out.append(POINT_KEEP)
    return np.array(out, np.uint8)
