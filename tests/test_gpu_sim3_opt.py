"""GPU parity: Optimizer::OptimizeSim3 and Scw on gfx950 (spslam_sim3_optimize_batch_device and the host form
spslam_sim3_optimize) against the sequential referee tests/sim3_opt_ref.cpp.  Bar: every result record and every
match12 entry byte for byte (NaN for NaN), and every byte between and after the problems' ranges as it was.  The
cases are tests/sim3_opt_cases.py; tests/test_sim3_opt_host.py guards that each of them reaches what it is there for."""
import numpy as np
import pytest

import sim3_opt_cases as C

pytestmark = pytest.mark.gpu

SENT = 0xCD
SENT32 = np.frombuffer(bytes([SENT] * 4), np.int32)[0]
GAP = 3  # sentinel entries between the problems' ranges


@pytest.fixture(scope="module")
def gpu():
    """One context per camera: {name: (extractor, LoopMatcher)}."""
    import spslam_frame
    import spslam_gpu
    import spslam_loop
    import synth
    out = {}
    for name, K in (("TUM3", synth.TUM3), ("ICL", synth.ICL)):
        ex = spslam_gpu.OrbExtractor(max_batch=1)
        spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], (0,) * 5, K["bf"], 640, 480)
        out[name] = (ex, spslam_loop.LoopMatcher(ex))
    yield out
    for ex, _ in out.values():
        ex.close()


@pytest.fixture(scope="module")
def data():
    points, bad, cases = C.all_cases()
    return points, bad, cases, C.references()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def same_record(a, b):
    """Byte for byte, or field for field with NaN for NaN."""
    if a.tobytes() == b.tobytes():
        return True
    return all(np.array_equal(a[f], b[f], equal_nan=a.dtype[f].base.kind == "f") for f in a.dtype.names)


def params_of(c):
    return (c["cam"], float(c["th2"]))


def run_batch(gpu, points, bad, cases, with_bad=True, launch=None):
    """One call over cases of one parameter set.  Keyframe k of the map sits in slot n_kf - 1 - k; the match12 ranges
    are GAP apart.  Returns per case (result record, match12 after).  launch(call, d_match12), if given, makes the
    call itself (tools/sim3_opt_timing.py repeats it between events)."""
    import torch
    import spslam_gpu as G
    import spslam_loop as L
    cam, th2 = params_of(cases[0])
    assert all(params_of(c) == (cam, th2) for c in cases)
    ex, lm = gpu[cam]
    kfs = [k for c in cases for k in (c["kf1"], c["kf2"])]
    n_kf, P = len(kfs), len(cases)
    cap = max(max(len(k["kun"]) for k in kfs), 1)
    kun, counts = np.zeros((n_kf, cap), G.KEYPOINT_DTYPE), np.zeros(n_kf, np.int32)
    for s, k in enumerate(kfs[::-1]):
        kun[s, :len(k["kun"])], counts[s] = k["kun"], len(k["kun"])
    kf_slot = np.arange(n_kf - 1, -1, -1).astype(np.int32)
    Tcw = np.stack([k["Tcw"] for k in kfs]).astype(np.float32)
    off = np.zeros(n_kf + 1, np.int32)
    off[1:] = np.cumsum([len(k["kun"]) for k in kfs])
    rows = np.concatenate([k["match_row"] for k in kfs] + [np.zeros(1, np.int32)]).astype(np.int32)
    rec = np.zeros(P, L.SIM3_PAIR_DTYPE)
    total, m_off = GAP, []
    for p, c in enumerate(cases):
        rec[p]["kf1"], rec[p]["kf2"], rec[p]["match_offset"], rec[p]["result_offset"] = 2 * p, 2 * p + 1, total, p
        rec[p]["s12"], rec[p]["R12"], rec[p]["t12"] = c["pair"][0], c["pair"][1:10], c["pair"][10:13]
        m_off.append(total)
        total += len(c["match12"]) + GAP
    m_in = np.full(total, SENT32, np.int32)
    for p, c in enumerate(cases):
        m_in[m_off[p]:m_off[p] + len(c["match12"])] = c["match12"]
    t = [dev(a) for a in (Tcw, kf_slot, off, rows, bad, points, rec, kun, counts, m_in)]
    smap = L.Sim3Map(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                     t[4].data_ptr() if with_bad else 0, t[5].data_ptr())
    d_res = torch.full(((P + 1) * L.SIM3_OPT_RESULT_DTYPE.itemsize,), SENT, dtype=torch.uint8, device="cuda")
    call = lambda: lm.sim3_optimize_batch_device(P, t[6].data_ptr(), smap, t[7].data_ptr(), t[8].data_ptr(), cap,  # noqa: E731
                                                 t[9].data_ptr(), d_res.data_ptr(), th2=th2,
                                                 min_inliers=cases[0]["min_inliers"])
    launch(call, t[9]) if launch else call()
    torch.cuda.synchronize()
    res, m = host(d_res, L.SIM3_OPT_RESULT_DTYPE), host(t[9], np.int32)
    inside = np.zeros(total, bool)
    for p, c in enumerate(cases):
        inside[m_off[p]:m_off[p] + len(c["match12"])] = True
    assert (m[~inside] == SENT32).all() and (res[P:].view(np.uint8) == SENT).all()   # between and after the ranges
    assert host(t[6], L.SIM3_PAIR_DTYPE).tobytes() == rec.tobytes()                  # the pair records are inputs
    return [(res[p].copy(), m[m_off[p]:m_off[p] + len(c["match12"])].copy()) for p, c in enumerate(cases)]


def check(got, cases, wants):
    for (res, m), c, w in zip(got, cases, wants):
        assert same_record(res, w["result"]), (c["name"], res, w["result"])
        assert m.tobytes() == w["match12"].tobytes(), (c["name"], np.flatnonzero(m != w["match12"])[:8])


def grouped(cases, refs):
    groups = {}
    for c, r in zip(cases, refs):
        groups.setdefault(params_of(c), []).append((c, r))
    return groups


def test_every_case_matches_the_referee_in_mixed_batches(gpu, data):
    """One launch per parameter set (camera, th2), all its cases mixed: 0 to 300 correspondences, both statuses,
    rejected trials, checks that read a rejected trial's errors, the th2 seams, the NaN chi2."""
    points, bad, cases, refs = data
    groups = grouped(cases, refs)
    assert len(groups[("TUM3", C.TH2)]) >= 25 and ("ICL", C.TH2) in groups and len(groups) >= 6
    statuses = set()
    for group in groups.values():
        sel, wants = [g[0] for g in group], [g[1] for g in group]
        check(run_batch(gpu, points, bad, sel), sel, wants)
        statuses |= {int(w["result"]["status"]) for w in wants}
    assert statuses == {C.OK, C.TOO_FEW}


def test_batches_of_one_two_and_reversed_and_without_the_bad_table(gpu, data):
    points, bad, cases, refs = data
    group = grouped(cases, refs)[("TUM3", C.TH2)]
    for sel in (group[5:6], group[:2], group[::-1]):
        check(run_batch(gpu, points, bad, [g[0] for g in sel]), [g[0] for g in sel], [g[1] for g in sel])
    clean = [g for g in group if g[0]["name"] != "gather_bad_and_missing"]   # no bad point: the same without the table
    check(run_batch(gpu, points, bad, [g[0] for g in clean], with_bad=False), [g[0] for g in clean], [g[1] for g in clean])


def test_results_do_not_depend_on_the_scratch(gpu, data):
    points, bad, cases, refs = data
    group = grouped(cases, refs)[("TUM3", C.TH2)]
    sel, wants = [g[0] for g in group], [g[1] for g in group]
    first = run_batch(gpu, points, bad, sel)                            # sizes the scratch
    check(first, sel, wants)
    for value in (0x00, 0xFF):
        gpu["TUM3"][1].debug_fill_loop_scratch(value)
        got = run_batch(gpu, points, bad, sel)
        check(got, sel, wants)
        assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(got, first))


def test_host_form_equals_the_referee(gpu, data):
    points, bad, cases, refs = data
    for c, w in zip(cases, refs):
        lm = gpu[c["cam"]][1]
        res, m = lm.sim3_optimize(c["kf1"], c["kf2"], points, bad, c["pair"][0], c["pair"][1:10], c["pair"][10:13],
                                  c["match12"], th2=float(c["th2"]), min_inliers=c["min_inliers"])
        check([(res, m)], [c], [w])


def test_solver_search_optimize_and_scw_search_chain_on_one_stream(gpu):
    """ComputeSim3 from the RANSAC to the Scw search (LoopClosing.cc:303-393) without a host read in between:
    spslam_sim3_solver_batch_device leaves the pair record and the filtered match12, spslam_search_by_sim3_batch_device
    extends match12, spslam_sim3_optimize_batch_device prunes it and leaves mScw, which a device-to-device copy puts
    into the spslam_fuse_problem record of spslam_search_by_projection_sim3_batch_device.  The result equals the
    four referees chained."""
    import torch
    import loop_match_ref as LR
    import sim3_solver_cases as SC
    import sim3_solver_ref as SR
    import spslam_loop as L
    import test_gpu_sim3_solver as TS
    g = gpu["TUM3"]
    ex, lm = g
    points, bad, kf1, kf2, match12, rand, geo = SC.chain_case()
    assert np.array_equal(np.asarray(geo[:4], np.float32), C.cameras()["TUM3"])
    # ---- the four referees
    s = SR.Sim3Solver(kf1, kf2, points, bad, match12, geo, True, rand)
    s.set_ransac_parameters(SC.PROBABILITY, 20, 300)
    T12, no_more, inl, n = s.iterate(5)
    want_solver = s.result(T12, no_more, n)
    assert T12 is not None
    m_sim3, found = LR.search_by_sim3(kf1, kf2, points, bad, s.mBestScale, s.mBestRotation, s.mBestTranslation,
                                      SR.filtered_match12(match12, inl), geo)
    pair = np.concatenate([[s.mBestScale], np.asarray(s.mBestRotation).reshape(9), np.asarray(s.mBestTranslation).reshape(3)])
    case = dict(name="chain", cam="TUM3", kf1=kf1, kf2=kf2, match12=m_sim3, pair=pair.astype(np.float32),
                th2=np.float32(C.TH2), min_inliers=C.MIN_INLIERS)
    want_opt = C.reference(case, points, bad)
    assert int(want_opt["result"]["n_corr"]) >= 20
    loop_points = points[kf2["match_row"][kf2["match_row"] >= 0]]       # mvpLoopMapPoints: the loop keyframe's points
    mScw = want_opt["result"]["mScw"].reshape(4, 4)
    want_proj, want_n = LR.search_by_projection_sim3(mScw, loop_points, kf1["kun"], kf1["desc"], kf1["go"], kf1["gi"], geo,
                                                     10.0)
    solver_case = dict(name="chain", kf1=kf1, kf2=kf2, match12=match12, rand=rand, min_inliers=20, max_iterations=300,
                       fix_scale=True)
    keep = []

    def follow(t, smap, cap, d_pairs, d_mout, rec):
        # the full slots of the two keyframes, keyframe k in slot 1 - k as run_batch laid them out
        desc, go, gi = np.zeros((2, cap, 32), np.uint8), np.zeros((2, 64 * 48 + 1), np.int32), np.zeros((2, cap), np.int32)
        for slot, k in enumerate((kf2, kf1)):
            desc[slot, :len(k["desc"])], go[slot] = k["desc"], k["go"]
            gi[slot, :len(k["gi"])] = k["gi"]
        frec = np.zeros(1, L.FUSE_PROBLEM_DTYPE)
        frec[0]["Tcw"] = SENT                                          # overwritten on the device
        frec[0]["kf_slot"], frec[0]["n_points"] = 1, len(loop_points)  # the current keyframe KF1 sits in slot 1
        d = [dev(a) for a in (desc, go, gi, frec, loop_points)]
        fill = lambda nbytes: torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda")  # noqa: E731
        d_found, d_res, d_match, d_n = fill(8), fill(2 * 232), fill(2 * cap * 4), fill(8)
        keep.extend(d + [d_found, d_res, d_match, d_n])
        slots = (t[7].data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), t[8].data_ptr())
        lm.search_by_sim3_batch_device(1, d_pairs.data_ptr(), smap, *slots, cap, 0, d_mout.data_ptr(), d_found.data_ptr())
        lm.sim3_optimize_batch_device(1, d_pairs.data_ptr(), smap, slots[0], slots[4], cap, d_mout.data_ptr(),
                                      d_res.data_ptr())
        d[3][:64].copy_(d_res[168:232])                                # mScw into spslam_fuse_problem.Tcw, on the device
        lm.search_by_projection_sim3_batch_device(1, d[3].data_ptr(), d[4].data_ptr(), len(loop_points), *slots, cap, 0, 0,
                                                  d_match.data_ptr(), d_n.data_ptr(), 10.0)
        return d_mout, d_res, d_match, d_n, int(rec[0]["match_offset"])

    res, pairs, (d_mout, d_res, d_match, d_n, off) = TS.run_batch(g, points, bad, [(solver_case, (0, 0), 5)],
                                                                   follow=follow)
    assert res[0].tobytes() == want_solver.tobytes()
    got_opt = host(d_res, L.SIM3_OPT_RESULT_DTYPE)
    assert same_record(got_opt[0], want_opt["result"]) and (got_opt[1:].view(np.uint8) == SENT).all()
    m = host(d_mout, np.int32)[off:off + len(match12)]
    assert m.tobytes() == want_opt["match12"].tobytes()
    n1 = len(kf1["kun"])
    got_proj = host(d_match, np.int32)[:n1]
    assert got_proj.tobytes() == want_proj.tobytes() and int(host(d_n, np.int32)[0]) == want_n
    assert int(want_opt["result"]["accepted"]) == 1 and want_n >= 0


def test_validation_returns_errors_without_launching(gpu, data):
    import spslam_gpu
    import spslam_loop as L
    ex, lm = gpu["TUM3"]
    points, bad, cases, refs = data
    ok = L.Sim3Map(1, 1, 1, 1, 0, 1)
    for kw in (dict(fix_scale=False), dict(th2=0.0), dict(th2=-1.0), dict(th2=float("nan"))):
        with pytest.raises(spslam_gpu.SpslamError, match="sim3_optimize_batch_device"):
            lm.sim3_optimize_batch_device(1, 1, ok, 1, 1, 8, 1, 1, **kw)
    for args in ((0, 1, ok, 1, 1, 8, 1, 1), (1, 1, ok, 1, 1, 8193, 1, 1), (1, 1, L.Sim3Map(), 1, 1, 8, 1, 1),
                 (1, 1, ok, 1, 1, 8, 0, 1), (1, 1, ok, 1, 1, 8, 1, 0)):
        with pytest.raises(spslam_gpu.SpslamError, match="sim3_optimize_batch_device"):
            lm.sim3_optimize_batch_device(*args)
    c, w = next((c, w) for c, w in zip(cases, refs) if c["name"] == "clean_40")
    call = lambda **kw: lm.sim3_optimize(kw.get("kf1", c["kf1"]), kw.get("kf2", c["kf2"]), points, bad, c["pair"][0],  # noqa: E731
                                         c["pair"][1:10], c["pair"][10:13], kw.get("match12", c["match12"]),
                                         th2=kw.get("th2", 10.0), fix_scale=kw.get("fix_scale", True))
    check([call()], [c], [w])
    with pytest.raises(spslam_gpu.SpslamError, match="fix_scale is not 1"):
        call(fix_scale=False)
    with pytest.raises(spslam_gpu.SpslamError, match="th2 is not positive"):
        call(th2=0.0)
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
    check([call()], [c], [w])                                          # the context still works
