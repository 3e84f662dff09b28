"""CPU checks of the matcher case tables (tests/match_cases.py): every case through the oracle
(oracle/match_oracle.cpp) and through the Python transcriptions of the reference's loops (py_search, py_search_local
in tests/test_oracle_match.py), identical; the result known by construction where a case has one; and per case the
assertion that it reaches what it was built for, computed from the transcription's intermediate values or the
oracle's output, so that a change to the builders or to synth.py cannot quietly empty a case."""
import numpy as np
import pytest

import match_cases as MC
from matcher_ref import f32 as _f, fma
from test_oracle_match import py_search, py_search_local


def _current(case):
    return case["kun"], case["desc"], case["ur"], case["go"], case["gi"], case["geo"]


def transcribe(case):
    """The transcription's result in the oracle's form, and its traces (one per pass for frame to frame)."""
    G = MC.GEOMS[case["geom"]]
    fr, P = MC.effective(case)
    if case["kind"] == "proj":
        th, mono, ori, retry_below = case["params"]
        traces = [{}]
        m, nm = py_search(fr, P, *_current(case), th, mono=bool(mono), check_ori=bool(ori), trace=traces[0])
        if retry_below > 0 and nm < retry_below:
            traces.append({})
            m, nm = py_search(fr, P, *_current(case), 2 * th, mono=bool(mono), check_ori=bool(ori), trace=traces[1])
        return (m, nm, len(traces)), traces
    taken = case["taken"] if case["taken"] is not None else np.zeros(len(case["kun"]), np.uint8)
    trace = {}
    th, nn, vcl = case["params"][:3]
    out = py_search_local(fr, P, *_current(case), taken, th=th, nn=nn, vcl=vcl, scale_factor=G["scale_factor"],
                          n_levels=G["nlevels"], trace=trace)
    return out, trace


def expected_match(case):
    m = np.full(len(case["kun"]), -1, np.int32)
    for k, i in case["expect"]["match"].items():
        m[k] = i
    return m


def check_witnesses(case):
    """Oracle, transcription and (where given) construction agree; returns the oracle's output and the traces."""
    name = case["name"]
    out = MC.oracle(case)
    ref, traces = transcribe(case)
    assert out[1] == ref[1], (name, out[1], ref[1])
    assert np.array_equal(out[0], ref[0]), (name, np.nonzero(out[0] != ref[0])[0][:10])
    assert np.array_equal(np.asarray(out[2]), np.asarray(ref[2])), name   # passes / in_view
    if case["expect"] is not None:
        assert out[1] == case["expect"]["nm"], (name, out[1])
        assert np.array_equal(out[0], expected_match(case)), (name, out[0])
    if case["kind"] == "local" and case["taken"] is not None:
        assert not (out[0][case["taken"].astype(bool)] >= 0).any(), name
    return out, traces


def _cells(case):
    return np.diff(case["go"])


def check_proj_reach(case, out, traces):
    name, R = case["name"], case["reach"]
    m, nm, passes = out
    t = traces[0]
    pts = t["points"]
    if "fwd" in R:
        assert (t["fwd"], t["bwd"]) == (R["fwd"], R["bwd"]), (name, t["tlc_z"], t["mb"])
    if "nm_min" in R:
        assert nm >= R["nm_min"], (name, nm)
    if R.get("overwritten"):   # a keypoint held by a point without observations was taken again
        assert passes == 1 and not case["params"][2] and nm > int((m >= 0).sum()), (name, nm)
    if R.get("last_keypoint_matched"):
        assert m[-1] >= 0, name
    if R.get("rescan"):        # for both key counts a point finds every kept key held by a blocking point
        for n_keys in MC.K_KEYS:
            assert any(MC.rescans(p["keys"], n_keys, False) for p in pts.values()), (name, n_keys)
    if R.get("cells"):
        assert int((_cells(case) > 0).sum()) == R["cells"], name
    if R.get("cell_population"):
        assert int(_cells(case).max()) == R["cell_population"], name
    if R.get("clipped"):       # windows reach the first and the last column and row of the grid
        cells = np.array([p["cells"] for p in pts.values() if "cells" in p])
        assert (cells[:, 0] == 0).any() and (cells[:, 1] == 63).any(), (name, cells)
        assert (cells[:, 2] == 0).any() and (cells[:, 3] == 47).any(), (name, cells)
    if R.get("empty_window"):
        assert any("cells" in p and not p["keys"] for p in pts.values()), name
    if R.get("off_grid") is not None:
        assert len(case["kun"]) - len(case["gi"]) == R["off_grid"], (name, len(case["gi"]))
    for i, (axis, bound, _) in enumerate(R.get("exact", ())):
        assert "cells" in pts[i] and float(pts[i]["uv"[axis]]) == bound, (name, i, pts[i])
    for i, (axis, bound, above) in enumerate(R.get("outside", ())):
        val = float(pts[i]["uv"[axis]])
        assert pts[i].get("outside") and (val > bound if above else val < bound), (name, i, val)
        assert abs(val - bound) <= 2.0 ** -13, (name, i, val, bound)   # (the nearest pixel the products reach)
    if "best" in R:
        assert [pts[i]["best"] for i in range(len(R["best"]))] == R["best"], name
    if "ties" in R:
        assert sum(len(p["keys"]) > 1 and p["keys"][0][0] == p["keys"][1][0] for p in pts.values()) >= R["ties"], name
    if "stereo" in R:
        mono = case["ur"] <= 0
        searched = [bool(p["keys"]) for p in pts.values()]
        if R["stereo"] == "all_mono":
            assert mono.all() and all(searched), name
        elif R["stereo"] == "all_stereo":
            assert not mono.any() and all(searched), name
        else:                  # the right-coordinate test empties the windows of one half
            assert not mono.any() and any(searched) and not all(searched), name
    for k, side in R.get("stereo_error", ()):
        g = case["geo"]
        r = _f(_f(case["params"][0]) * g[11])
        x3 = case["P"][k]["xw"]
        invz = _f(1.0 / float(x3[2]))
        urp = fma(-g[4], invz, pts[k]["u"])
        err, err_next = abs(_f(urp - case["ur"][k])), abs(_f(urp - MC.up(case["ur"][k])))
        # exactly the radius, or the nearest right coordinate whose error exceeds it
        assert case["ur"][k] > 0 and (err == r if side == "at" else err > r >= err_next), (name, k, err, r)
    if "hist" in R:
        assert {b: n for b, n in enumerate(t["hist"]) if n} == R["hist"], (name, t["hist"])
    if "dropped" in R:
        assert [b for b, n in enumerate(t["hist"]) if n and b not in t["kept"]] == sorted(R["dropped"]), (name, t)
    if R.get("bins_dropped"):
        assert any(n and b not in t["kept"] for b, n in enumerate(t["hist"])), name
    if "pushed_twice" in R:
        k = R["pushed_twice"]
        assert sum(1 for p in case["P"] if np.array_equal(p["xw"], case["P"][k]["xw"])) == 2 and m[k] == -1, name
    if "passes" in R:
        assert passes == R["passes"], (name, passes, nm)


def check_local_reach(case, out, trace):
    name, R = case["name"], case["reach"]
    m, nm, iv = out
    G = MC.GEOMS[case["geom"]]
    if "in_view" in R:
        assert list(iv) == R["in_view"] and iv.any() and not iv.all(), (name, iv)
    if R.get("in_view_mixed"):
        assert iv.any() and not iv.all(), name
    for i, why in R.get("why", {}).items():
        assert trace[i]["why"] == why, (name, i, trace[i])
    if "reasons" in R:
        assert R["reasons"] <= {p["why"] for p in trace.values()}, (name, {p["why"] for p in trace.values()})
    if R.get("raw_below"):
        assert all(trace[i]["raw_level"] < 0 for i in trace), (name, trace)
    if R.get("raw_above"):
        assert all(trace[i]["raw_level"] >= G["nlevels"] for i in trace), (name, trace)
    if "level" in R:
        assert [trace[i]["level"] for i in sorted(trace)] == R["level"], name
    if "radius" in R:
        assert [float(trace[i]["radius"]) for i in sorted(trace)] == R["radius"], name
    if "nm_min" in R:
        assert nm >= R["nm_min"], (name, nm)
    if "nm_max" in R:          # (the ratio test stops the list)
        assert nm <= R["nm_max"], (name, nm)
    if R.get("rescan"):        # for both key counts a point finds fewer than two of its kept keys free
        for n_keys in MC.K_KEYS:
            assert any(MC.rescans(p.get("keys", []), n_keys, True) for p in trace.values()), (name, n_keys)
    if R.get("taken") == "all":
        assert case["taken"].all() and nm == 0, name
    if R.get("taken") == "seams":
        n = len(case["kun"])
        assert set(np.nonzero(case["taken"])[0]) == {k for k in MC.TAKEN_SEAMS + (n - 1,) if k < n}, name
    if R.get("seen"):          # the stamped points match when not stamped, and the referee's list drops them
        seen = case["seen"]
        plain = dict(case, seen=None)
        mp, _, ivp = MC.oracle(plain)
        assert 10 < seen.sum() < len(seen) and ivp[seen].all() and np.isin(np.nonzero(seen)[0], mp).all(), name
        assert not iv[seen].any() and not np.isin(np.nonzero(seen)[0], m).any(), name
        assert np.array_equal(iv[~seen], ivp[~seen]), name


@pytest.mark.parametrize("group", list(MC.PROJ_GROUPS))
def test_projection_cases(group):
    cases = MC.proj_group(group)
    assert cases
    for case in cases:
        out, traces = check_witnesses(case)
        check_proj_reach(case, out, traces)


@pytest.mark.parametrize("group", list(MC.LOCAL_GROUPS))
def test_local_point_cases(group):
    cases = MC.local_group(group)
    assert cases
    for case in cases:
        out, trace = check_witnesses(case)
        check_local_reach(case, out, trace)


def test_direction_cases_change_the_assignment():
    """The three octave ranges give three different assignments on the constructed and on the rendered frames."""
    by_name = {c["name"]: MC.oracle(c)[0] for c in MC.proj_group("direction")}
    for a, b, c in (("direction_tum_plus_mono0", "direction_tum_minus_mono0", "direction_tum_zero_mono0"),
                    ("rendered_forward", "rendered_backward", "rendered_forward_mono")):
        assert not np.array_equal(by_name[a], by_name[b]), (a, b)
        assert not np.array_equal(by_name[a], by_name[c]) and not np.array_equal(by_name[b], by_name[c]), (a, b, c)
    # one float either side of mb decides (a strict >), and mono switches both flags off
    assert np.array_equal(by_name["direction_tum_at_mb_mono0"], by_name["direction_tum_zero_mono0"])
    assert np.array_equal(by_name["direction_tum_above_mb_mono0"], by_name["direction_tum_plus_mono0"])
    assert np.array_equal(by_name["direction_tum_beyond_neg_mb_mono0"], by_name["direction_tum_minus_mono0"])
    assert np.array_equal(by_name["direction_tum_above_mb_mono1"], by_name["direction_tum_zero_mono0"])


def test_second_geometries_differ_from_the_first():
    tum = MC.proj_group("border")[0]["geo"]
    barrel = next(c for c in MC.proj_group("second_geometry") if c["geom"] == "barrel")["geo"]
    small = next(c for c in MC.proj_group("second_geometry") if c["geom"] == "small")["geo"]
    assert list(tum[5:11]) == [0.0, 640.0, 0.0, 480.0, _f(0.1), _f(0.1)]
    assert barrel[5] < 0 and barrel[7] < 0 and barrel[6] > 640 and barrel[8] > 480 and barrel[9] < _f(0.1)
    assert list(small[5:11]) == [0.0, 480.0, 0.0, 360.0, _f(64) / _f(480), _f(48) / _f(360)]
    assert list(small[11:16]) == [1.0, 1.5, 2.25, 3.375, 5.0625] and not small[16:].any()


def test_case_tables_are_deterministic():
    """A second build of the constructed tables equals the first byte for byte."""
    for build, group in ((MC.dense_cases, "dense"), (MC.seam_cases, "seams"), (MC.local_count_cases, "counts")):
        first = MC.proj_group(group) if build is not MC.local_count_cases else MC.local_group(group)
        for a, b in zip(first, build()):
            pts = "P" if a["kind"] == "proj" else "LP"
            assert a["name"] == b["name"] and a[pts].tobytes() == b[pts].tobytes()
            assert all(a[k].tobytes() == b[k].tobytes() for k in ("kun", "desc", "ur", "go", "gi", "geo")), a["name"]


def test_lds_limit_expression():
    """The largest cap whose taken bits and claim table fit the dynamic LDS the launches opt into: the figures the
    GPU test drives the launches with (ceil(cap / 32) * 4 + cap * 4 bytes against 160 KB and 150 KB)."""
    lds = lambda cap: (cap + 31) // 32 * 4 + cap * 4  # noqa: E731
    for limit_kb, cap in ((160, MC.LOCAL_CAP_LIMIT), (150, MC.PROJ_CAP_LIMIT)):
        assert lds(cap) <= limit_kb * 1024 < lds(cap + 1), (limit_kb, cap)
