"""Scalar restatement of Tracking::UpdateLocalMap (src/Tracking.cc:1427-1571) over plain dicts and lists, written
from the reference: what spslam_track_update_local_map_batch_device is compared with, exactly.

Map model
  points: {pid: {"obs": [keyframe, ...] (MapPoint::GetObservations' keys), "bad": bool}}
  kfs:    {k: {"bad": bool, "covis": [keyframe, ...] (GetBestCovisibilityKeyFrames(10), best first),
               "children": [keyframe, ...] (GetChilds), "parent": keyframe or None (GetParent),
               "matches": [pid or None, ...] (GetMapPointMatches, keypoint order)}}
  frame_points: [pid or None, ...] (mCurrentFrame.mvpMapPoints)
  local_kfs: mvpLocalKeyFrames as the frame holds it on entry.

The project's standing substitution: keyframe id order where the reference iterates std::map<KeyFrame*> /
std::set<KeyFrame*> in pointer order (:1475, :1495, :1539).  Quirks kept: the return before clear() (:1485-1486),
no isBad() on the parent and its break leaving the outer loop (:1553-1562).  The neighbour loop walks the first K1
entries by index: the reference iterates the vector it push_back's into, which is only defined while the
reserve(3 * K1) (:1492) is not exceeded; the index walk is that defined reading.  mvpMapPoints[i] = NULL for a
bad point (:1480) is not part of the result.

capacity: the ABI's rule, not the reference's -- the point list is cut to its first `capacity` entries, status 1.
"""
import numpy as np


def update_local_keyframes(frame_points, points, kfs, local_kfs, trace=None):
    """:1463-1571.  Returns (mvpLocalKeyFrames, pKFmax or None).  trace (a dict, optional) receives what the run
    went through: counter, k1, and how the neighbour loop ended ("limit" at > 80, "parent", or "end")."""
    trace = {} if trace is None else trace
    counter = {}                                            # :1466 map<KeyFrame*,int> keyframeCounter
    for pid in frame_points:                                # :1467
        if pid is None:                                     # :1469
            continue
        if not points[pid]["bad"]:                          # :1472
            for k in sorted(points[pid]["obs"]):            # :1474-1476
                counter[k] = counter.get(k, 0) + 1
    trace.update(counter=dict(counter), k1=None, ended=None)
    if not counter:                                         # :1485-1486: before clear()
        return list(local_kfs), None
    mx, kf_max = 0, None                                    # :1488-1489
    out, member = [], set()                                 # :1491 clear(); mnTrackReferenceForFrame == mnId
    for k in sorted(counter):                               # :1495
        if kfs[k]["bad"]:                                   # :1499
            continue
        if counter[k] > mx:                                 # :1502
            mx, kf_max = counter[k], k
        out.append(k)                                       # :1508
        member.add(k)
    trace.update(k1=len(out), ended="end")
    for q in range(len(out)):                               # :1514, the first K1 entries
        if len(out) > 80:                                   # :1517
            trace.update(ended="limit", ended_at=q)
            break
        k = out[q]
        for nb in kfs[k]["covis"][:10]:                     # :1522-1536
            if not kfs[nb]["bad"] and nb not in member:
                out.append(nb)
                member.add(nb)
                break
        for ch in sorted(kfs[k]["children"]):               # :1538-1551
            if not kfs[ch]["bad"] and ch not in member:
                out.append(ch)
                member.add(ch)
                break
        p = kfs[k]["parent"]                                # :1553
        if p is not None and p not in member:               # :1554-1556: no isBad()
            out.append(p)
            member.add(p)
            trace.update(ended="parent", ended_at=q)
            break                                           # :1560: leaves the for over the keyframes
    return out, kf_max


def update_local_points(local_kfs, points, kfs, trace=None):
    """:1437-1460."""
    trace = {} if trace is None else trace
    trace.update(n_concat=sum(len(kfs[k]["matches"]) for k in local_kfs), n_dup=0, n_bad=0, n_empty=0)
    out, seen = [], set()                                   # mnTrackReferenceForFrame == mCurrentFrame.mnId
    for k in local_kfs:                                     # :1441
        for pid in kfs[k]["matches"]:                       # :1446
            if pid is None:                                 # :1449
                trace["n_empty"] += 1
                continue
            if pid in seen:                                 # :1451
                trace["n_dup"] += 1
                continue
            if not points[pid]["bad"]:                      # :1453
                out.append(pid)
                seen.add(pid)
            else:
                trace["n_bad"] += 1
    return out


def update_local_map(frame_points, points, kfs, local_kfs, capacity=None):
    """:1427-1435 (without SetReferenceMapPoints).  Returns dict(local_kfs, kf_max (-1 = none), local_points,
    n_total, status, trace)."""
    trace = {}
    lk, kf_max = update_local_keyframes(frame_points, points, kfs, local_kfs, trace)
    lp = update_local_points(lk, points, kfs, trace)
    n_total = len(lp)
    status = 0
    if capacity is not None and n_total > capacity:
        lp, status = lp[:capacity], 1
    return dict(local_kfs=lk, kf_max=-1 if kf_max is None else kf_max, local_points=lp, n_total=n_total,
                status=status, trace=trace)


def dicts_from_tables(T):
    """The map model above from the spslam_local_map tables of one sequence (point ids = rows)."""
    nr, nk = len(T["obs_off"]) - 1, len(T["parent"])
    pb, kb = T.get("point_bad"), T.get("kf_bad")
    points = {r: {"obs": [int(k) for k in T["obs_kf"][T["obs_off"][r]:T["obs_off"][r + 1]]],
                  "bad": bool(pb[r]) if pb is not None else False} for r in range(nr)}
    covis = np.asarray(T["covis"]).reshape(nk, 10)
    kfs = {}
    for k in range(nk):
        kfs[k] = {"bad": bool(kb[k]) if kb is not None else False,
                  "covis": [int(c) for c in covis[k] if c >= 0],
                  "children": [int(c) for c in T["child"][T["child_off"][k]:T["child_off"][k + 1]]],
                  "parent": int(T["parent"][k]) if T["parent"][k] >= 0 else None,
                  "matches": [int(r) if r >= 0 else None
                              for r in T["match_row"][T["match_off"][k]:T["match_off"][k + 1]]]}
    return points, kfs


def run_tables(T, frame_rows, local_kfs=(), capacity=None):
    points, kfs = dicts_from_tables(T)
    fp = [int(r) if r >= 0 else None for r in frame_rows]
    return update_local_map(fp, points, kfs, [int(k) for k in local_kfs], capacity)
