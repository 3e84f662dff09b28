"""GPU parity: PnPsolver on gfx950 (spslam_pnp_solver_batch_device and the host form spslam_pnp_solver) against the
literal restatement tests/pnp_ref.cpp.  Bar: every result record, inlier byte, best-mask byte and frame point byte for
byte, and every byte between and after the problems' output ranges as it was.  The cases are tests/pnp_cases.py;
tests/test_pnp_host.py guards that each of them reaches what it is there for."""
import numpy as np
import pytest

import pnp_cases as C

pytestmark = pytest.mark.gpu

SENT = 0xCD
SENT32 = np.frombuffer(bytes([SENT] * 4), np.int32)[0]
GAP = 3  # sentinel entries between the problems' ranges


@pytest.fixture(scope="module")
def gpu():
    import spslam_frame
    import spslam_gpu
    import spslam_loop
    import spslam_reloc
    import synth
    K = synth.TUM3
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], (0,) * 5, K["bf"], 640, 480)
    yield ex, spslam_reloc, spslam_loop.LoopMatcher(ex)
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


def solver_for(gpu, params):
    ex, R, _ = gpu
    return R.PnPSolver(ex, C.PROBABILITY, params[0], params[1], C.MIN_SET, params[2], C.TH2, C.RAND_MAX)


def run_batch(gpu, points, bad, items, with_fp=True, with_bad=True, d_match=None, launch=None):
    """One call over items = [(case, previous result record or None, best mask before, n_iterations)], all of one
    parameter set.  The frame of item p sits in slot P - 1 - p; the keyframe of item p is keyframe p of the map;
    match, rand, inlier and mask ranges are GAP apart.  Returns per item (result record, inlier bytes, best mask
    after, frame points or None where the range kept its sentinels).  launch(call), if given, makes the device call
    (tools/pnp_timing.py repeats it between events); a new solver's call can be repeated: it does not read the mask."""
    import torch
    import spslam_gpu as G
    import spslam_loop as L
    ex, R, _ = gpu
    params = items[0][0]["params"]
    assert all(c["params"] == params for c, _, _, _ in items)
    P = len(items)
    cap = max(max(len(c["kun"]) for c, _, _, _ in items), 1)
    kun, counts = np.zeros((P, cap), G.KEYPOINT_DTYPE), np.zeros(P, np.int32)
    off = np.zeros(P + 1, np.int32)
    off[1:] = np.cumsum([len(c["kf_rows"]) for c, _, _, _ in items])
    rows = np.concatenate([c["kf_rows"] for c, _, _, _ in items] + [np.zeros(1, np.int32)]).astype(np.int32)
    rec = np.zeros(P, R.PNP_PROBLEM_DTYPE)
    total, rtotal, m_off = GAP, GAP, []
    for p, (c, prev, mask, n_it) in enumerate(items):
        slot = P - 1 - p
        kun[slot, :len(c["kun"])], counts[slot] = c["kun"], len(c["kun"])
        q = rec[p]
        q["kf"], q["frame_slot"] = p, slot
        q["match_offset"] = q["inlier_offset"] = q["best_mask_offset"] = total
        q["rand_offset"], q["n_iterations"], q["rand_iterations"] = rtotal, n_it, c["rand_iterations"]
        if prev is not None:
            q["iterations_done"], q["best_inliers"], q["best_Tcw"] = prev["iterations_done"], prev["best_inliers"], prev["best_Tcw"]
        m_off.append(total)
        total += len(c["kun"]) + GAP
        rtotal += 4 * c["rand_iterations"] + GAP
    m_in, r_in = np.full(total, SENT32, np.int32), np.full(rtotal, SENT32, np.int32)
    mask_in = np.full(total, SENT, np.uint8)
    for p, (c, _, mask, _) in enumerate(items):
        nf = len(c["kun"])
        m_in[m_off[p]:m_off[p] + nf] = c["match"]
        mask_in[m_off[p]:m_off[p] + nf] = mask[:nf]
        r_in[rec[p]["rand_offset"]:rec[p]["rand_offset"] + 4 * c["rand_iterations"]] = c["rand"]
    S = solver_for(gpu, params)
    max_its, min_n = S.ransac_table(cap)
    t = [dev(a) for a in (off, rows, bad, points, rec, kun, counts, m_in, r_in, max_its, min_n)]
    smap = L.Sim3Map(0, 0, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr() if with_bad else 0, t[3].data_ptr())
    fill = lambda n: torch.full((n,), SENT, dtype=torch.uint8, device="cuda")  # noqa: E731
    d_res, d_inl, d_fp = fill((P + 1) * R.PNP_RESULT_DTYPE.itemsize), fill(total), fill(total * 4)
    d_mask = dev(mask_in)
    call = lambda: S.batch_device(  # noqa: E731
        P, t[4].data_ptr(), smap, t[5].data_ptr(), t[6].data_ptr(), cap,
        (d_match if d_match is not None else t[7]).data_ptr(), t[8].data_ptr(), t[9].data_ptr(), t[10].data_ptr(),
        d_res.data_ptr(), d_inl.data_ptr(), d_mask.data_ptr(), d_fp.data_ptr() if with_fp else 0)
    launch(call) if launch else call()
    torch.cuda.synchronize()
    res, inl, mask_out, fp = host(d_res, R.PNP_RESULT_DTYPE), d_inl.cpu().numpy(), d_mask.cpu().numpy(), host(d_fp, np.int32)
    # the inputs are as they were; nothing between or after the ranges
    assert np.array_equal(host(t[7], np.int32), m_in) and np.array_equal(host(t[8], np.int32), r_in)
    inside = np.zeros(total, bool)
    for p, (c, _, _, _) in enumerate(items):
        inside[m_off[p]:m_off[p] + len(c["kun"])] = True
    assert (inl[~inside] == SENT).all() and (fp[~inside] == SENT32).all() and (mask_out[~inside] == SENT).all()
    assert (res[P:].view(np.uint8) == SENT).all()
    out = []
    for p, (c, _, _, _) in enumerate(items):
        sl = slice(m_off[p], m_off[p] + len(c["kun"]))
        pose = int(res[p]["status"]) in (C.REFINED, C.BEST_NO_MORE)
        if not (pose and with_fp):
            assert (fp[sl] == SENT32).all(), c["name"]                  # no pose: the frame points are untouched
        out.append((res[p].copy(), inl[sl].copy(), mask_out[sl].copy(), fp[sl].copy() if pose and with_fp else None))
    return out


def check(got, items, wants, with_fp=True):
    for (res, inl, mask, fp), (c, _, _, _), (w, r) in zip(got, items, wants):
        assert res.tobytes() == w["results"][r].tobytes(), (c["name"], r, res, w["results"][r])
        assert inl.tobytes() == w["inliers"][r].tobytes(), (c["name"], r)
        assert mask.tobytes() == w["best_mask"][r].tobytes(), (c["name"], r)
        pose = int(w["results"][r]["status"]) in (C.REFINED, C.BEST_NO_MORE)
        if pose and with_fp:
            assert fp.tobytes() == w["frame_points"][r].tobytes(), (c["name"], r)
        else:
            assert fp is None, (c["name"], r)
        if not pose:
            assert not inl.any() and not res["Tcw"].any() and int(res["n_inliers"]) == 0, c["name"]


def item(c, w, r):
    """Call r of a case with the state the referee had before it."""
    nf = max(len(c["kun"]), 1)
    prev = w["results"][r - 1] if r else None
    mask = w["best_mask"][r - 1] if r else np.zeros(nf, np.uint8)
    return (c, prev, mask, c["calls"][r])


def grouped(cases, refs, r):
    groups = {}
    for c, w in zip(cases, refs):
        if r < len(c["calls"]):
            groups.setdefault(c["params"], []).append((item(c, w, r), (w, r)))
    return groups


def test_every_case_and_call_matches_the_referee(gpu, data):
    """Call r of every case that has one, in one launch per parameter set: a mixed batch of every N from 0 to 300, every
    outcome, states carried in, every seam of the gather and of the hypothesis kernel."""
    points, bad, cases, refs = data
    seen = set()
    for r in range(max(len(c["calls"]) for c in cases)):
        for params, group in grouped(cases, refs, r).items():
            items, wants = [g[0] for g in group], [g[1] for g in group]
            check(run_batch(gpu, points, bad, items), items, wants)
            seen |= {int(w["results"][q]["status"]) for w, q in wants}
    assert seen == {C.REFINED, C.BEST_NO_MORE, C.NO_MORE, C.OUT_OF_DRAWS}


def test_one_problem_at_a_time_in_reverse_and_without_optional_arguments(gpu, data):
    points, bad, cases, refs = data
    group = grouped(cases, refs, 0)[C.TRACKING]
    pick = [g for g in group if g[0][0]["name"] in ("n0", "n10", "n15", "n64", "fail_then_refined", "all_wrong", "coincident")]
    assert len(pick) == 7
    for g in pick:
        check(run_batch(gpu, points, bad, [g[0]]), [g[0]], [g[1]])
    rev = group[::-1]
    check(run_batch(gpu, points, bad, [g[0] for g in rev]), [g[0] for g in rev], [g[1] for g in rev])
    check(run_batch(gpu, points, bad, [g[0] for g in pick], with_fp=False), [g[0] for g in pick], [g[1] for g in pick],
          with_fp=False)
    # no bad row among the matched points: the same without the table
    clean = [g for g in group if not bad[g[0][0]["kf_rows"][g[0][0]["kf_rows"] >= 0]].any()]
    assert len(clean) >= 3
    check(run_batch(gpu, points, bad, [g[0] for g in clean], with_bad=False), [g[0] for g in clean], [g[1] for g in clean])


def test_results_do_not_depend_on_the_scratch(gpu, data):
    """The scratch is the buffer the loop-closing entries use: whatever a call before left there, or a fill."""
    ex, R, lm = gpu
    points, bad, cases, refs = data
    group = grouped(cases, refs, 0)[C.LONG]
    items, wants = [g[0] for g in group], [g[1] for g in group]
    big = grouped(cases, refs, 0)[C.TRACKING]
    # another loop-closing call on the same context first: Sim3Solver reserves and writes the shared buffer
    import sim3_solver_cases as SC
    spoints, sbad, scases = SC.build()
    sc = next(q for q in scases if q["name"] == "n_cap_300")
    lm.sim3_solver(sc["kf1"], sc["kf2"], spoints, sbad, sc["match12"], sc["rand"], 2, (0, 0), SC.PROBABILITY,
                   sc["min_inliers"], sc["max_iterations"], sc["fix_scale"])
    check(run_batch(gpu, points, bad, items), items, wants)            # on what Sim3Solver left
    run_batch(gpu, points, bad, [g[0] for g in big])                    # a larger PnP call grows and dirties it
    for value in (None, 0x00, 0xFF):
        if value is not None:
            lm.debug_fill_loop_scratch(value)
        check(run_batch(gpu, points, bad, items), items, wants)


def test_state_read_back_from_one_call_feeds_the_next(gpu, data):
    """The device's own result record and best mask are the next call's input; the referee is one object called
    again."""
    points, bad, cases, refs = data
    by = {c["name"]: (c, w) for c, w in zip(cases, refs)}
    for name in ("reentry", "carried_mask_governs", "reentry_below_max", "n10", "all_wrong", "out_of_draws"):
        c, w = by[name]
        prev, mask = None, np.zeros(max(len(c["kun"]), 1), np.uint8)
        for r, n_it in enumerate(c["calls"]):
            it = (c, prev, mask, n_it)
            got = run_batch(gpu, points, bad, [it])
            check(got, [it], [(w, r)])
            prev, mask = got[0][0], got[0][2]


def test_host_form_keeps_the_state_between_calls(gpu, data):
    import torch
    ex, R, _ = gpu
    points, bad, cases, refs = data
    for c, w in zip(cases, refs):
        S = solver_for(gpu, c["params"])
        use_torch = c["name"] in ("n15", "reentry")
        conv = (lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy())
                if a.dtype.names else torch.from_numpy(np.ascontiguousarray(a))) if use_torch else (lambda a: a)
        for r, n_it in enumerate(c["calls"]):
            res, inl, fp = S.solve(conv(c["kun"]) if len(c["kun"]) else c["kun"], conv(c["match"]), conv(c["kf_rows"]),
                                   conv(points), conv(bad), conv(c["rand"]), n_it)
            inl, fp = (None if a is None else np.asarray(a) for a in (inl, fp))
            assert res.tobytes() == w["results"][r].tobytes(), (c["name"], r, res, w["results"][r])
            assert inl.tobytes() == w["inliers"][r].tobytes(), (c["name"], r)
            pose = int(res["status"]) in (C.REFINED, C.BEST_NO_MORE)
            assert (fp is not None) == pose and (fp is None or fp.tobytes() == w["frame_points"][r].tobytes()), (c["name"], r)
            assert S.best_mask.tobytes() == w["best_mask"][r].tobytes(), (c["name"], r)


def test_search_by_bow_feeds_the_solver_on_the_same_stream(gpu):
    """Relocalization's second and third calls without a host copy between: d_match as
    spslam_search_by_bow_batch_device leaves it is the solver's input.  The map is made so that the matches of a
    rendered pair are consistent with one pose, but for every seventh."""
    import torch
    import bow_common as BC
    import oracle_bow
    import spslam_bow
    import spslam_gpu as G
    import spslam_match
    ex, R, _ = gpu
    (kk, kd), (fk, fd) = BC.frames(2)
    ov = oracle_bow.Vocabulary(BC.vocab_text())
    fvs = [ov.transform(kd), ov.transform(fd)]
    rng = np.random.default_rng(3)
    has = (rng.random(len(kd)) < 0.9).astype(np.uint8)
    want_match, want_n = oracle_bow.search_by_bow(kd, kk["angle"], has, fvs[0], fd, fk["angle"], fvs[1], 0.75, True)
    assert want_n >= 15                                                 # Tracking.cc:1617
    # the keyframe's map: a point behind every matched frame keypoint under the pose T; every seventh is elsewhere
    T, cam = C.pose(), C.camera().astype(np.float64)
    Tinv = np.linalg.inv(T)
    pts = np.zeros(len(kd), spslam_match.LOCAL_POINT_DTYPE)
    kf_rows = np.where(has != 0, np.arange(len(kd)), -1).astype(np.int32)
    pts["xw"] = rng.uniform(-1, 1, (len(kd), 3))
    for n, i in enumerate(np.flatnonzero(want_match >= 0)):
        z = rng.uniform(1.0, 4.0)
        Xc = np.array([(fk["x"][i] - cam[2]) / cam[0] * z, (fk["y"][i] - cam[3]) / cam[1] * z, z])
        if n % 7 != 6:
            pts["xw"][want_match[i]] = Tinv[:3, :3] @ Xc + Tinv[:3, 3]
    bad = np.zeros(len(kd), np.uint8)
    case = dict(name="chain", kun=fk, match=want_match.astype(np.int32), kf_rows=kf_rows, rand=np.array(C.random_draws(9, 340), np.int32),
                rand_iterations=340, params=C.TRACKING, calls=(5,))
    w = C.reference(case, pts, bad)
    assert int(w["results"][0]["status"]) == C.REFINED and int(w["results"][0]["n_inliers"]) > 15
    # SearchByBoW on the device: keyframe slot 0, frame slot 0 of two sides of cap features
    cap = max(len(kd), len(fd))

    def side(keys, desc, fv, hp):
        d, k = np.zeros((cap, 32), np.uint8), np.zeros(cap, G.KEYPOINT_DTYPE)
        d[:len(desc)], k[:len(keys)] = desc, keys
        fn, fs, ff = np.zeros(cap, np.uint32), np.zeros(cap + 1, np.int32), np.zeros(cap, np.int32)
        fn[:len(fv["nodes"])], fs[:len(fv["start"])], ff[:len(fv["features"])] = fv["nodes"], fv["start"], fv["features"]
        h = np.zeros(cap, np.uint8)
        if hp is not None:
            h[:len(hp)] = hp
        t = [dev(a) for a in (d, k, h, np.array([len(desc)], np.int32), fn, fs, ff, np.array([len(fv["nodes"])], np.int32))]
        return t, spslam_bow.BowSide(*[a.data_ptr() for a in t], cap, 0)
    tk, sk = side(kk, kd, fvs[0], has)
    tf, sf = side(fk, fd, fvs[1], None)
    d_pairs = dev(np.array([0, 0], np.int32))
    # the matcher writes its cap ints GAP ints into the buffer, where run_batch puts the first problem's match_offset
    d_match = torch.full((cap + 2 * GAP,), -7, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    spslam_bow.search_by_bow_batch_device(ex, 1, d_pairs.data_ptr(), sk, sf, d_match.data_ptr() + 4 * GAP,
                                          d_n.data_ptr(), nn_ratio=0.75)
    it = (case, None, np.zeros(len(fk), np.uint8), 5)
    got = run_batch(gpu, pts, bad, [it], d_match=d_match)               # no synchronisation, no copy between the two
    check(got, [it], [(w, 0)])
    assert int(d_n.cpu()[0]) == want_n
    assert np.array_equal(d_match.cpu().numpy()[GAP:GAP + len(fd)], want_match)


def test_validation_returns_errors_without_launching(gpu, data):
    import spslam_gpu
    import spslam_loop as L
    ex, R, _ = gpu
    points, bad, cases, refs = data
    S = solver_for(gpu, C.TRACKING)
    smap = L.Sim3Map(0, 0, 1, 1, 0, 1)
    for kw in (dict(min_set=3), dict(min_set=5), dict(max_iterations=0), dict(max_iterations=R.PNP_MAX_ITERATIONS + 1),
               dict(rand_max=0), dict(min_inliers=0), dict(epsilon=0.0), dict(th2=0.0)):
        bad_S = solver_for(gpu, C.TRACKING)
        for k, v in kw.items():
            setattr(bad_S.params, k, v)
        with pytest.raises(spslam_gpu.SpslamError, match="pnp_solver_batch_device"):
            bad_S.batch_device(1, 1, smap, 1, 1, 8, 1, 1, 1, 1, 1, 1, 1)
    with pytest.raises(spslam_gpu.SpslamError, match="pnp_solver_batch_device"):
        S.batch_device(1, 1, smap, 1, 1, 8193, 1, 1, 1, 1, 1, 1, 1)
    with pytest.raises(spslam_gpu.SpslamError, match="pnp_solver_batch_device"):
        S.batch_device(1, 1, L.Sim3Map(), 1, 1, 8, 1, 1, 1, 1, 1, 1, 1)
    c, w = next((q, r) for q, r in zip(cases, refs) if q["name"] == "n15")
    xw_rows = np.ascontiguousarray(points)

    def raw(**kw):
        """spslam_pnp_solver itself on sentinel-filled outputs: (return code, the outputs are untouched, result)."""
        import ctypes
        par = R.PnPParams(10, 300, 4, C.RAND_MAX, 0.5, C.TH2)
        for k, v in kw.get("params", {}).items():
            setattr(par, k, v)
        kun = np.ascontiguousarray(kw.get("kun", c["kun"]))
        m = np.ascontiguousarray(kw.get("match", c["match"]), np.int32)
        rows = np.ascontiguousarray(kw.get("kf_rows", c["kf_rows"]), np.int32)
        rnd = np.ascontiguousarray(kw.get("rand", c["rand"]), np.int32)
        q = np.zeros((), R.PNP_PROBLEM_DTYPE)
        q["n_iterations"], q["rand_iterations"] = kw.get("n_iterations", 5), kw.get("rand_iterations", len(rnd) // 4)
        res = np.full(R.PNP_RESULT_DTYPE.itemsize, SENT, np.uint8)
        inl, mask, fp = (np.full(len(kun) * k, SENT, np.uint8) for k in (1, 1, 4))
        rc = ex.lib.spslam_pnp_solver(ex.ctx, kun.ctypes.data, len(kun), m.ctypes.data, rows.ctypes.data, len(rows),
                                      xw_rows.ctypes.data, bad.ctypes.data, len(points), rnd.ctypes.data, ctypes.byref(par),
                                      C.PROBABILITY, q.ctypes.data, res.ctypes.data, inl.ctypes.data, mask.ctypes.data,
                                      fp.ctypes.data)
        untouched = all((a == SENT).all() for a in (res, inl, mask, fp))
        return rc, untouched, res.view(R.PNP_RESULT_DTYPE)[0], ex.lib.spslam_last_error(ex.ctx).decode()
    rc, untouched, res, _ = raw()
    assert rc == 0 and not untouched and res["status"] == w["results"][0]["status"] and res["n"] == w["results"][0]["n"]
    m = c["match"].copy()
    m[c["kept"][0]] = len(c["kf_rows"])
    rc, untouched, _, msg = raw(match=m)
    assert rc == -1 and untouched and "match entry outside" in msg                  # an out-of-range match
    m[c["kept"][0]] = -2
    rc, untouched, _, msg = raw(match=m)
    assert rc == -1 and untouched and "match entry outside" in msg
    rows = c["kf_rows"].copy()
    rows[c["match"][c["kept"][1]]] = len(points)
    rc, untouched, _, msg = raw(kf_rows=rows)
    assert rc == -1 and untouched and "map point outside" in msg                    # an out-of-range row
    for octave in (8, -1):
        kun = c["kun"].copy()
        kun["octave"][2] = octave
        rc, untouched, _, msg = raw(kun=kun)
        assert rc == -1 and untouched and "octave outside" in msg                   # an octave beyond the levels
    for ms in (3, 5):
        rc, untouched, _, msg = raw(params=dict(min_set=ms))
        assert rc == -1 and untouched and "min_set is not 4" in msg                 # min_set != 4
    rc, untouched, _, msg = raw(rand_iterations=0)
    assert rc == -1 and untouched and "too few draws" in msg                        # too few draws
    rc, untouched, _, msg = raw(n_iterations=-1)
    assert rc == -1 and untouched and "n_iterations outside" in msg
    r = c["rand"].copy()
    r[5] = -1
    rc, untouched, _, msg = raw(rand=r)
    assert rc == -1 and untouched and "draw outside" in msg
    # draws that end inside the call's range are no error: the call reports OUT_OF_DRAWS
    wa = next(r for q, r in zip(cases, refs) if q["name"] == "out_of_draws")
    ca = next(q for q in cases if q["name"] == "out_of_draws")
    S = solver_for(gpu, C.TRACKING)
    res, inl, fp = S.solve(ca["kun"], ca["match"], ca["kf_rows"], points, bad, ca["rand"], 5)
    assert res.tobytes() == wa["results"][0].tobytes() and int(res["status"]) == C.OUT_OF_DRAWS and fp is None
    rc, untouched, res, _ = raw()                                                    # the context still works
    assert rc == 0 and res.tobytes() == w["results"][0].tobytes()
