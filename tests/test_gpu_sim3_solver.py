"""GPU parity: Sim3Solver on gfx950 (spslam_sim3_solver_batch_device and the host form spslam_sim3_solver) against
the scalar restatement tests/sim3_solver_ref.py.  Bar: every result record, inlier byte, pair record and filtered
match12 byte for byte, and every byte between and after the problems' output ranges as it was.  The cases are
tests/sim3_solver_cases.py; tests/test_sim3_solver_host.py guards that each of them reaches what it is there for."""
import numpy as np
import pytest

import sim3_solver_cases as C
import sim3_solver_ref as SR

pytestmark = pytest.mark.gpu

SENT = 0xCD
SENT32 = np.frombuffer(bytes([SENT] * 4), np.int32)[0]
GAP = 3  # sentinel entries between the problems' ranges


@pytest.fixture(scope="module")
def gpu():
    import spslam_frame
    import spslam_gpu
    import spslam_loop
    import synth
    K = synth.TUM3
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], (0,) * 5, K["bf"], 640, 480)
    yield ex, spslam_loop.LoopMatcher(ex)
    ex.close()


@pytest.fixture(scope="module")
def data():
    points, bad, cases = C.build()
    return points, bad, cases, C.references()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def params_of(c):
    return (c["min_inliers"], c["max_iterations"], bool(c["fix_scale"]))


def run_batch(gpu, points, bad, items, with_out=True, with_bad=True, follow=None):
    """One call over items = [(case, (iterations_done, best_inliers), n_iterations)], all of one parameter set.
    Keyframe k of the map sits in slot n_kf - 1 - k; match12, rand and inlier ranges are GAP apart.  Returns per item
    (result record, inlier bytes, pair record or None, filtered match12 or None); None where the output kept its
    sentinels.  follow(t, ...) may enqueue more work on the same stream before the results are read."""
    import torch
    import spslam_gpu as G
    import spslam_loop as L
    ex, lm = gpu
    mn, mx, fix = params_of(items[0][0])
    assert all(params_of(c) == (mn, mx, fix) for c, _, _ in items)
    kfs = [k for c, _, _ in items for k in (c["kf1"], c["kf2"])]
    n_kf, P = len(kfs), len(items)
    cap = max(max(len(k["kun"]) for k in kfs), 1)
    kun, counts = np.zeros((n_kf, cap), G.KEYPOINT_DTYPE), np.zeros(n_kf, np.int32)
    for s, k in enumerate(kfs[::-1]):
        kun[s, :len(k["kun"])], counts[s] = k["kun"], len(k["kun"])
    kf_slot = np.arange(n_kf - 1, -1, -1).astype(np.int32)
    Tcw = np.stack([k["Tcw"] for k in kfs]).astype(np.float32)
    off = np.zeros(n_kf + 1, np.int32)
    off[1:] = np.cumsum([len(k["kun"]) for k in kfs])
    rows = np.concatenate([k["match_row"] for k in kfs] + [np.zeros(1, np.int32)]).astype(np.int32)
    rec = np.zeros(P, L.SIM3_PROBLEM_DTYPE)
    total, rtotal, m_off = GAP, GAP, []
    for p, (c, state, n_it) in enumerate(items):
        rec[p]["kf1"], rec[p]["kf2"], rec[p]["match_offset"], rec[p]["inlier_offset"] = 2 * p, 2 * p + 1, total, total
        rec[p]["rand_offset"], rec[p]["iterations_done"], rec[p]["best_inliers"] = rtotal, state[0], state[1]
        rec[p]["n_iterations"] = n_it
        m_off.append(total)
        total += len(c["match12"]) + GAP
        rtotal += 3 * mx + GAP
    m_in, r_in = np.full(total, SENT32, np.int32), np.full(rtotal, SENT32, np.int32)
    for p, (c, _, _) in enumerate(items):
        m_in[m_off[p]:m_off[p] + len(c["match12"])] = c["match12"]
        r_in[rec[p]["rand_offset"]:rec[p]["rand_offset"] + 3 * mx] = c["rand"]
    table = lm.sim3_ransac_table(cap, C.PROBABILITY, mn, mx)
    t = [dev(a) for a in (Tcw, kf_slot, off, rows, bad, points, rec, kun, counts, m_in, r_in, table)]
    smap = L.Sim3Map(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                     t[4].data_ptr() if with_bad else 0, t[5].data_ptr())
    fill = lambda n: torch.full((n,), SENT, dtype=torch.uint8, device="cuda")  # noqa: E731
    d_res, d_inl = fill((P + 1) * L.SIM3_RESULT_DTYPE.itemsize), fill(total)
    d_pairs, d_mout = fill((P + 1) * 80), fill(total * 4)
    lm.sim3_solver_batch_device(P, t[6].data_ptr(), smap, t[7].data_ptr(), t[8].data_ptr(), cap, t[9].data_ptr(),
                                t[10].data_ptr(), t[11].data_ptr(), d_res.data_ptr(), d_inl.data_ptr(),
                                d_pairs.data_ptr() if with_out else 0, d_mout.data_ptr() if with_out else 0,
                                min_inliers=mn, max_iterations=mx, fix_scale=fix)
    extra = follow(t, smap, cap, d_pairs, d_mout, rec) if follow else None
    torch.cuda.synchronize()
    res, inl = host(d_res, L.SIM3_RESULT_DTYPE), d_inl.cpu().numpy()
    pairs, mout = host(d_pairs, L.SIM3_PAIR_DTYPE), host(d_mout, np.int32)
    if follow:
        return res, pairs, extra
    # the inputs are as they were; nothing between or after the ranges, and nothing for a problem that is not FOUND
    assert np.array_equal(host(t[9], np.int32), m_in) and np.array_equal(host(t[10], np.int32), r_in)
    inside = np.zeros(total, bool)
    for p, (c, _, _) in enumerate(items):
        inside[m_off[p]:m_off[p] + len(c["match12"])] = True
    assert (inl[~inside] == SENT).all() and (mout[~inside] == SENT32).all()
    assert (res[P:].view(np.uint8) == SENT).all() and (pairs[P:].view(np.uint8) == SENT).all()
    out = []
    for p, (c, _, _) in enumerate(items):
        sl = slice(m_off[p], m_off[p] + len(c["match12"]))
        found = with_out and int(res[p]["status"]) == SR.FOUND
        if not found:
            assert (pairs[p:p + 1].view(np.uint8) == SENT).all() and (mout[sl] == SENT32).all(), c["name"]
        out.append((res[p].copy(), inl[sl].copy(), pairs[p].copy() if found else None, mout[sl].copy() if found else None))
    return out, rec


def expected_pair(rec_p, p, want):
    import spslam_loop as L
    o = np.zeros((), L.SIM3_PAIR_DTYPE)
    o["kf1"], o["kf2"], o["match_offset"], o["result_offset"] = rec_p["kf1"], rec_p["kf2"], rec_p["match_offset"], p
    o["s12"], o["R12"], o["t12"] = want["s12"], want["R12"], want["t12"]
    return o


def check(got, rec, items, wants, with_out=True):
    for p, ((res, inl, pair, mout), (c, _, _), (want, want_inl, want_m)) in enumerate(zip(got, items, wants)):
        assert res.tobytes() == want.tobytes(), (c["name"], res, want)
        assert inl.tobytes() == want_inl.tobytes(), (c["name"], np.flatnonzero(inl != want_inl)[:8])
        if want_m is not None and with_out:
            assert mout.tobytes() == want_m.tobytes(), c["name"]
            assert pair.tobytes() == expected_pair(rec[p], p, want).tobytes(), c["name"]
        else:
            assert pair is None and mout is None, c["name"]
        if int(want["status"]) != SR.FOUND:
            assert not inl.any() and not res["T12"].any() and res["s12"] == 0, c["name"]


def state_before(c, calls, r):
    """The solver's state before call r of a case, from the referee's records."""
    if r == 0:
        return c["state"] if c["state"] is not None else (0, 0)
    return int(calls[r - 1][0]["iterations_done"]), int(calls[r - 1][0]["best_inliers"])


def grouped(cases, refs, r):
    groups = {}
    for c, (calls, _) in zip(cases, refs):
        if r < len(c["calls"]):
            groups.setdefault(params_of(c), []).append(((c, state_before(c, calls, r), c["calls"][r]), calls[r]))
    return groups


def test_every_case_and_call_matches_the_referee(gpu, data):
    """Call r of every case that has one, in one launch per parameter set: mixed statuses, N from 0 to cap, 1 to 300
    iterations, every first-success position, the draws' edges, the seam, the degenerate triples, both scale modes."""
    points, bad, cases, refs = data
    seen = set()
    for r in range(max(len(c["calls"]) for c in cases)):
        for key, group in grouped(cases, refs, r).items():
            items, wants = [g[0] for g in group], [g[1] for g in group]
            got, rec = run_batch(gpu, points, bad, items)
            check(got, rec, items, wants)
            seen |= {int(w[0]["status"]) for w in wants}
    assert seen == {SR.FOUND, SR.NOT_YET, SR.NO_MORE}


def test_batches_of_1_2_and_17_in_two_orders_and_without_optional_outputs(gpu, data):
    points, bad, cases, refs = data
    group = grouped(cases, refs, 0)[(6, 300, True)]
    assert len(group) >= 15
    group = (group + group[:2])[:17]                                   # a case may appear twice: disjoint ranges
    assert len({int(g[1][0]["status"]) for g in group}) == 3
    for sel in (group[3:4], group[:2], group, group[::-1]):
        items, wants = [g[0] for g in sel], [g[1] for g in sel]
        got, rec = run_batch(gpu, points, bad, items)
        check(got, rec, items, wants)
    items, wants = [g[0] for g in group], [g[1] for g in group]
    got, rec = run_batch(gpu, points, bad, items, with_out=False)      # no pair records, no filtered match12
    check(got, rec, items, wants, with_out=False)
    clean = [g for g in group if g[0][0]["name"] != "gather_bad_and_missing"]   # no bad point: the same without the table
    got, rec = run_batch(gpu, points, bad, [g[0] for g in clean], with_bad=False)
    check(got, rec, [g[0] for g in clean], [g[1] for g in clean])


def test_results_do_not_depend_on_the_scratch(gpu, data):
    ex, lm = gpu
    points, bad, cases, refs = data
    group = grouped(cases, refs, 0)[(3, 300, True)]
    items, wants = [g[0] for g in group], [g[1] for g in group]
    run_batch(gpu, points, bad, items)                                 # sizes the scratch
    for value in (0x00, 0xFF, None):                                   # None: what the launch before left
        if value is not None:
            lm.debug_fill_loop_scratch(value)
        got, rec = run_batch(gpu, points, bad, items)
        check(got, rec, items, wants)


def test_solver_continued_over_calls_of_5_equals_one_call(gpu, data):
    """The state read back from the device is carried into the next call."""
    points, bad, cases, refs = data
    by = {c["name"]: (c, calls) for c, (calls, _) in zip(cases, refs)}
    c, calls = by["calls_of_5"]
    state, last = (0, 0), None
    for r, n_it in enumerate(c["calls"]):
        got, rec = run_batch(gpu, points, bad, [(c, state, n_it)])
        check(got, rec, [(c, state, n_it)], [calls[r]])
        last = got[0]
        state = (int(last[0]["iterations_done"]), int(last[0]["best_inliers"]))
    one, calls1 = by["one_call_of_all"]
    got, _ = run_batch(gpu, points, bad, [(one, (0, 0), 300)])
    assert got[0][0].tobytes() == last[0].tobytes() and got[0][1].tobytes() == last[1].tobytes()
    assert got[0][3].tobytes() == last[3].tobytes()


def test_host_form_equals_the_batch_form(gpu, data):
    ex, lm = gpu
    points, bad, cases, refs = data
    for c, (calls, _) in zip(cases, refs):
        state = c["state"] if c["state"] is not None else (0, 0)
        for n_it, (want, want_inl, want_m) in zip(c["calls"], calls):
            res, inl, mout, state = lm.sim3_solver(c["kf1"], c["kf2"], points, bad, c["match12"], c["rand"], n_it, state,
                                                   C.PROBABILITY, c["min_inliers"], c["max_iterations"], c["fix_scale"])
            assert res.tobytes() == want.tobytes() and inl.tobytes() == want_inl.tobytes(), c["name"]
            assert state == (int(want["iterations_done"]), int(want["best_inliers"]))
            assert (mout is None) == (want_m is None) and (mout is None or mout.tobytes() == want_m.tobytes()), c["name"]


def test_pair_and_filtered_match12_feed_search_by_sim3_on_the_same_stream(gpu):
    """ComputeSim3's chain (LoopClosing.cc:303-325) without a host round trip: the solver's pair record and filtered
    match12 are SearchBySim3's inputs.  The result equals the two referees called in sequence."""
    import torch
    import loop_match_ref as LR
    ex, lm = gpu
    points, bad, kf1, kf2, match12, rand, geo = C.chain_case()
    s = SR.Sim3Solver(kf1, kf2, points, bad, match12, geo, True, rand)
    s.set_ransac_parameters(C.PROBABILITY, 20, 300)
    T12, no_more, inl, n = s.iterate(5)
    want = s.result(T12, no_more, n)
    want_m, want_found = LR.search_by_sim3(kf1, kf2, points, bad, s.mBestScale, s.mBestRotation, s.mBestTranslation,
                                           SR.filtered_match12(match12, inl), geo)
    case = dict(name="chain", kf1=kf1, kf2=kf2, match12=match12, rand=rand, min_inliers=20, max_iterations=300,
                fix_scale=True)
    keep = []

    def follow(t, smap, cap, d_pairs, d_mout, rec):
        # the full slots of the two keyframes, keyframe k in slot 1 - k as run_batch laid them out
        desc, go, gi = np.zeros((2, cap, 32), np.uint8), np.zeros((2, 64 * 48 + 1), np.int32), np.zeros((2, cap), np.int32)
        for slot, k in enumerate((kf2, kf1)):
            desc[slot, :len(k["desc"])], go[slot] = k["desc"], k["go"]
            gi[slot, :len(k["gi"])] = k["gi"]
        d = [dev(a) for a in (desc, go, gi)]
        d_found = torch.full((8,), SENT, dtype=torch.uint8, device="cuda")
        keep.extend(d + [d_found])
        lm.search_by_sim3_batch_device(1, d_pairs.data_ptr(), smap, t[7].data_ptr(), d[0].data_ptr(), d[1].data_ptr(),
                                       d[2].data_ptr(), t[8].data_ptr(), cap, 0, d_mout.data_ptr(), d_found.data_ptr())
        return d_mout, d_found, int(rec[0]["match_offset"])

    res, pairs, (d_mout, d_found, off) = run_batch(gpu, points, bad, [(case, (0, 0), 5)], follow=follow)
    assert res[0].tobytes() == want.tobytes()
    m = host(d_mout, np.int32)[off:off + len(match12)]
    assert m.tobytes() == want_m.tobytes() and int(host(d_found, np.int32)[0]) == want_found and want_found > 0


def test_validation_returns_errors_without_launching(gpu, data):
    import spslam_gpu
    import spslam_loop as L
    ex, lm = gpu
    points, bad, cases, refs = data
    for kw in (dict(min_inliers=2), dict(max_iterations=0), dict(max_iterations=L.SIM3_MAX_ITERATIONS + 1), dict(rand_max=0)):
        with pytest.raises(spslam_gpu.SpslamError, match="sim3_solver_batch_device"):
            lm.sim3_solver_batch_device(1, 1, L.Sim3Map(1, 1, 1, 1, 0, 1), 1, 1, 8, 1, 1, 1, 1, 1, **kw)
    with pytest.raises(spslam_gpu.SpslamError, match="sim3_solver_batch_device"):
        lm.sim3_solver_batch_device(1, 1, L.Sim3Map(1, 1, 1, 1, 0, 1), 1, 1, 8193, 1, 1, 1, 1, 1)
    with pytest.raises(spslam_gpu.SpslamError, match="sim3_solver_batch_device"):
        lm.sim3_solver_batch_device(1, 1, L.Sim3Map(), 1, 1, 8, 1, 1, 1, 1, 1)
    c = next(q for q in cases if q["name"] == "first_at_0")
    call = lambda **kw: lm.sim3_solver(kw.get("kf1", c["kf1"]), kw.get("kf2", c["kf2"]), points, bad,  # noqa: E731
                                       kw.get("match12", c["match12"]), kw.get("rand", c["rand"]),
                                       kw.get("n_iterations", 1), kw.get("state", (0, 0)), C.PROBABILITY,
                                       kw.get("min_inliers", 3), 300, True)
    assert int(call()[0]["status"]) == SR.FOUND
    rows = c["kf1"]["match_row"].copy()
    rows[0] = len(points)
    with pytest.raises(spslam_gpu.SpslamError, match="map point outside"):
        call(kf1=dict(c["kf1"], match_row=rows))
    rows = c["kf2"]["match_row"].copy()
    rows[-1] = -2
    with pytest.raises(spslam_gpu.SpslamError, match="map point outside"):
        call(kf2=dict(c["kf2"], match_row=rows))
    m = c["match12"].copy()
    m[0] = len(c["kf2"]["kun"])
    with pytest.raises(spslam_gpu.SpslamError, match="match12 entry outside"):
        call(match12=m)
    for side in ("kf1", "kf2"):
        for octave in (8, -1):
            kun = c[side]["kun"].copy()
            kun["octave"][1] = octave
            with pytest.raises(spslam_gpu.SpslamError, match="octave outside"):
                call(**{side: dict(c[side], kun=kun)})
    with pytest.raises(spslam_gpu.SpslamError, match="min_inliers below 3"):
        call(min_inliers=2)
    with pytest.raises(spslam_gpu.SpslamError, match="n_iterations is negative"):
        call(n_iterations=-1)
    with pytest.raises(spslam_gpu.SpslamError, match="state is negative"):
        call(state=(-1, 0))
    r = c["rand"].copy()
    r[-1] = -1
    with pytest.raises(spslam_gpu.SpslamError, match="draw outside"):
        call(rand=r)
    assert int(call()[0]["status"]) == SR.FOUND                        # the context still works
