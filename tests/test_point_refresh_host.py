"""CPU checks of the map-point refresh's restatement (tests/point_refresh_ref.py) and cases
(tests/point_refresh_cases.py): the normal / depth half against oracle_local_map's update_normal_and_depth on the
same inputs, the descriptor half against a brute-force numpy sort, and what each case reaches."""
import numpy as np

import oracle_local_map as OL
import point_refresh_cases as PC
import point_refresh_ref as PR

BOTH = PR.DESCRIPTOR | PR.NORMAL_DEPTH


def _rows(packed, rows):
    """(row, observers, keypoints) of the listed rows."""
    t = packed["t"]
    for r in rows:
        o0, o1 = t["obs_off"][r], t["obs_off"][r + 1]
        yield int(r), t["obs_kf"][o0:o1].tolist(), t["obs_kp"][o0:o1].tolist()


def test_normal_and_depth_equal_the_oracle_bookkeeping():
    packed, rows, want = PC.build()
    t = packed["t"]
    got, status, _ = want[PR.NORMAL_DEPTH]
    m = object.__new__(OL.KeyframeMap)           # its update_normal_and_depth on the same tables
    m.table = packed["points"].copy()
    m.scale = PC.scale_factors()
    m.observations, m.ref_kf = {}, {}
    m.kfs = {k: {"octave": packed["keys_un"][t["kf_slot"][k]]["octave"].tolist()} for k in range(len(t["kf_slot"]))}
    centers = {k: OL.camera_center(t["kf_Tcw"][k]) for k in range(len(t["kf_slot"]))}
    n_done = 0
    for k, (r, kfs, kps) in enumerate(_rows(packed, rows)):
        if status[k] != PR.DONE:
            continue
        m.observations[r] = dict(zip(kfs, kps))
        m.ref_kf[r] = int(t["ref_kf"][r])
        m.update_normal_and_depth(r, r, centers)
        n_done += 1
    assert n_done > 40
    assert m.table.tobytes() == got.tobytes()
    assert not np.array_equal(got["normal"], packed["points"]["normal"])


def test_descriptor_equals_a_brute_force_sort():
    packed, rows, want = PC.build()
    t = packed["t"]
    got, status, _ = want[PR.DESCRIPTOR]
    expect = packed["points"].copy()
    for k, (r, kfs, kps) in enumerate(_rows(packed, rows)):
        if status[k] != PR.DONE:
            continue
        ds = np.array([packed["desc"][t["kf_slot"][kf], kp] for kf, kp in zip(kfs, kps) if not t["kf_bad"][kf]])
        if len(ds) == 0:
            continue
        D = np.unpackbits(ds[:, None, :] ^ ds[None, :, :], axis=2).sum(axis=2)
        med = np.sort(D, axis=1)[:, int(0.5 * (len(ds) - 1))]
        expect[r]["desc"] = ds[int(np.argmin(med))]      # argmin: the first smallest
    assert expect.tobytes() == got.tobytes()


def test_cases_reach_what_they_are_there_for():
    packed, rows, want = PC.build()
    t, names = packed["t"], packed["names"]
    got, status, traces = want[BOTH]
    at = {int(r): k for k, r in enumerate(rows)}
    n_obs = np.diff(t["obs_off"])
    assert sorted(rows.tolist()) == list(range(len(packed["points"]))) and rows.tolist() != sorted(rows.tolist())
    for i in (0, 1):
        for n in PC.COUNTS:
            r = names[f"{i}:n{n}"]
            assert n_obs[r] == n and status[at[r]] == PR.DONE
        assert n_obs[names[f"{i}:over_capacity"]] == PR.MAX_OBS + 1
        assert status[at[names[f"{i}:over_capacity"]]] == PR.CAPACITY
        for name in ("no_observers", "bad_point"):
            assert status[at[names[f"{i}:{name}"]]] == PR.UNTOUCHED
        for name in ("over_capacity", "no_observers", "bad_point"):
            r = names[f"{i}:{name}"]
            assert got[r].tobytes() == packed["points"][r].tobytes()
        # ties on the smallest median between rows with different descriptors; not row 0
        for name, first in (("tie_small", 1), ("dup_wide", 2)):
            med = traces[at[names[f"{i}:{name}"]]]["medians"]
            assert med.count(min(med)) >= 2 and med.index(min(med)) == first, (name, med)
        assert traces[at[names[f"{i}:first_bad"]]]["n_desc"] == 2
        assert traces[at[names[f"{i}:middle_bad"]]]["n_desc"] == 3
        for name in ("all_bad", "all_bad_wide"):
            r = names[f"{i}:{name}"]
            assert traces[at[r]]["n_desc"] == 0 and status[at[r]] == PR.DONE
            assert got[r]["desc"].tobytes() == packed["points"][r]["desc"].tobytes()
            assert got[r]["normal"].tobytes() != packed["points"][r]["normal"].tobytes()   # bad keyframes count here
        assert traces[at[names[f"{i}:ref_middle"]]]["ref_index"] == 2
        assert traces[at[names[f"{i}:ref_absent"]]]["ref_index"] is None
        assert traces[at[names[f"{i}:ref_last_wide"]]]["ref_index"] == 39
        assert traces[at[names[f"{i}:ref_absent_wide"]]]["ref_index"] is None
        assert traces[at[names[f"{i}:ref_second_chunk"]]]["ref_index"] == 77      # past the first 64 observers
    # each mask writes its own fields and nothing else
    d, nd = want[PR.DESCRIPTOR][0], want[PR.NORMAL_DEPTH][0]
    src = packed["points"]
    for f in ("xw", "id", "n_obs", "pad"):
        assert np.array_equal(got[f], src[f])
    for f in ("normal", "min_dist", "max_dist"):
        assert d[f].tobytes() == src[f].tobytes() and nd[f].tobytes() == got[f].tobytes()
    assert nd["desc"].tobytes() == src["desc"].tobytes() and d["desc"].tobytes() == got["desc"].tobytes()
    assert (d["desc"] != src["desc"]).any(axis=1).sum() > 30
