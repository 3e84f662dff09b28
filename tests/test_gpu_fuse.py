"""GPU parity: the search of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:842-949) on gfx950 --
spslam_fuse_search_batch_device and its host-pointer form -- against the scalar restatement tests/fuse_ref.py.
Bar: every result record, nfused and every byte outside the out ranges identical.  The cases are
tests/fuse_cases.py; tests/test_fuse_host.py guards that each of them reaches what it is there for."""
import numpy as np
import pytest

import fuse_cases as FC
import fuse_ref as FR

pytestmark = pytest.mark.gpu

SENT = 0xCD
GAP = 3  # sentinel records between the problems' out ranges


@pytest.fixture(scope="module")
def gpu():
    import spslam_frame
    import spslam_gpu
    import spslam_match
    import synth
    K = synth.TUM3
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], (0,) * 5, K["bf"], 640, 480)
    yield ex, spslam_match
    ex.close()


@pytest.fixture(scope="module")
def cases():
    """(keyframes, problems by name, the restatement's (records, nfused) by name), computed once."""
    kfs, problems = FC.build()
    by_name = {p["name"]: p for p in problems}
    # real0's points into the other sequence's keyframe: a second and third problem on that point range
    by_name["real0_into_kf1"] = dict(by_name["real0"], name="real0_into_kf1", kf=1)
    by_name["real0_n65_into_kf1"] = dict(by_name["real0_n65"], name="real0_n65_into_kf1", kf=1)
    refs = {name: FC.reference(p, kfs, FC.geo()) for name, p in by_name.items()}
    return kfs, by_name, refs


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Slots:
    """The keyframes in the frame stage's batch layouts, on the device."""

    def __init__(self, kfs):
        import spslam_gpu as G
        S = len(kfs)
        self.cap = cap = max(max(len(k["kun"]) for k in kfs), 1)
        kun, desc = np.zeros((S, cap), G.KEYPOINT_DTYPE), np.zeros((S, cap, 32), np.uint8)
        ur, go = np.zeros((S, cap), np.float32), np.zeros((S, 64 * 48 + 1), np.int32)
        gi, counts = np.zeros((S, cap), np.int32), np.zeros(S, np.int32)
        for s, k in enumerate(kfs):
            n = len(k["kun"])
            kun[s, :n], desc[s, :n], ur[s, :n], go[s], counts[s] = k["kun"], k["desc"], k["ur"], k["go"], n
            gi[s, :len(k["gi"])] = k["gi"]
        self.d = [dev(a) for a in (kun, desc, ur, go, gi, counts)]


def run_batch(gpu, slots, problems, with_skip=True):
    """One launch over `problems` (all of one th).  Point ranges that are a prefix of an earlier problem's are
    shared with it.  Returns per problem (records, nfused) plus what the launch left outside the out ranges."""
    import torch
    ex, M = gpu
    th = {p["th"] for p in problems}
    assert len(th) == 1
    fs = M.FuseSearch(ex, (th.pop(), 0))
    rec = np.zeros(len(problems), M.FUSE_PROBLEM_DTYPE)
    packed, pts_off, out_off, total = [], [], [], GAP
    for n, p in enumerate(problems):
        raw = p["P"].tobytes()
        share = next((k for k, (o, q) in enumerate(packed) if len(q) >= len(p["P"]) and
                      q[:len(p["P"])].tobytes() == raw), None)
        if share is None:
            packed.append((sum(len(q) for _, q in packed), p["P"]))
            share = len(packed) - 1
        pts_off.append(packed[share][0])
        rec[n]["Tcw"], rec[n]["kf_slot"], rec[n]["point_offset"] = p["Tcw"], p["kf"], packed[share][0]
        rec[n]["n_points"], rec[n]["out_offset"] = len(p["P"]), total
        out_off.append(total)
        total += len(p["P"]) + GAP
    points = np.concatenate([q for _, q in packed] + [np.zeros(1, M.LOCAL_POINT_DTYPE)])
    skip = np.full(total, SENT, np.uint8)
    for p, o in zip(problems, out_off):
        skip[o:o + len(p["P"])] = 0 if p["skip"] is None else p["skip"]
    assert with_skip or all(p["skip"] is None for p in problems)
    d_rec, d_pts, d_skip = dev(rec), dev(points), dev(skip)
    d_res = torch.full((total * 8,), SENT, dtype=torch.uint8, device="cuda")
    d_nf = torch.full((len(problems),), -9, dtype=torch.int32, device="cuda")
    d = slots.d
    fs.batch_device(len(problems), d_rec.data_ptr(), d_pts.data_ptr(), max(max(len(p["P"]) for p in problems), 0),
                    d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                    d[5].data_ptr(), slots.cap, d_skip.data_ptr() if with_skip else 0, d_res.data_ptr(),
                    d_nf.data_ptr())
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(M.FUSE_RESULT_DTYPE)
    nf = d_nf.cpu().numpy()
    inside = np.zeros(total, bool)
    for p, o in zip(problems, out_off):
        inside[o:o + len(p["P"])] = True
    assert (res.view(np.uint8).reshape(total, 8)[~inside] == SENT).all()      # nothing outside the out ranges
    assert np.array_equal(d_skip.cpu().numpy(), skip)
    shared = len(problems) - len(packed)
    return [(res[o:o + len(p["P"])], int(nf[n])) for n, (p, o) in enumerate(zip(problems, out_off))], shared


def check(got, refs, problems):
    for (res, nf), p in zip(got, problems):
        want, want_nf = refs[p["name"]]
        assert res.tobytes() == want.astype(res.dtype).tobytes(), \
            (p["name"], [(i, res[i], want[i]) for i in np.flatnonzero(res != want.astype(res.dtype))[:5]])
        assert nf == want_nf, (p["name"], nf, want_nf)


TH3_BATCH = ["real0", "real1", "real0_n0", "real0_n1", "real0_n63", "real0_n64", "real0_n65", "real1_skip",
             "keyframe_without_keypoints", "statuses", "clipped_th3", "chi2_stereo_second_wins",
             "chi2_mono_second_wins", "uright_zero_is_stereo", "levels", "real0_into_kf1", "real0_n65_into_kf1"]


def test_batch_of_17_matches_the_restatement(gpu, cases):
    """17 problems in one launch: seven on keyframe slot 0, three on slot 1, and real0's point range shared by
    eight of them (whole or as a prefix)."""
    kfs, by_name, refs = cases
    problems = [by_name[n] for n in TH3_BATCH]
    assert len(problems) == 17
    assert sum(p["kf"] == 0 for p in problems) >= 3 and sum(p["kf"] == 1 for p in problems) >= 3
    got, shared = run_batch(gpu, Slots(kfs), problems)
    assert shared >= 3
    check(got, refs, problems)


def test_wide_windows_ties_and_single_problem_launches(gpu, cases):
    kfs, by_name, refs = cases
    slots = Slots(kfs)
    wide = [by_name[n] for n in ("real0_th30", "ties_all_zero", "clipped_th30")]
    check(run_batch(gpu, slots, wide)[0], refs, wide)
    for name in ("real0_th30", "statuses", "real0_n0"):                       # one problem per launch
        check(run_batch(gpu, slots, [by_name[name]])[0], refs, [by_name[name]])


def test_without_skip_flags(gpu, cases):
    kfs, by_name, refs = cases
    problems = [by_name[n] for n in TH3_BATCH if by_name[n]["skip"] is None]
    check(run_batch(gpu, Slots(kfs), problems, with_skip=False)[0], refs, problems)


def test_same_batch_twice_in_two_orders(gpu, cases):
    """Nothing is carried from launch to launch: the batch again in the same context, reversed, per problem the
    same records."""
    kfs, by_name, refs = cases
    slots = Slots(kfs)
    problems = [by_name[n] for n in TH3_BATCH]
    a, _ = run_batch(gpu, slots, problems)
    b, _ = run_batch(gpu, slots, problems[::-1])
    check(a, refs, problems)
    for (ra, na), (rb, nb) in zip(a, b[::-1]):
        assert ra.tobytes() == rb.tobytes() and na == nb


def test_host_form_equals_the_batch_form(gpu, cases):
    ex, M = gpu
    kfs, by_name, refs = cases
    for name in ("real1_skip", "real0_n65", "real0_n0", "keyframe_without_keypoints", "statuses", "clipped_th30",
                 "uright_zero_is_stereo"):
        p = by_name[name]
        k = kfs[p["kf"]]
        res, nf = M.FuseSearch(ex, (p["th"], 0))(p["Tcw"], p["P"], k["kun"], k["desc"], k["ur"], k["go"], k["gi"],
                                                 p["skip"])
        check([(res, nf)], refs, [p])


def test_second_camera_with_distortion_shifted_bounds():
    """A context configured with distortion: the Frame's bounds are not integers, the KeyFrame's are."""
    import spslam_frame
    import spslam_gpu
    import spslam_match
    import synth
    K = synth.TUM3
    g, kfs, problems = FC.build_distorted()
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    try:
        st = spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], FC.DISTORTED, K["bf"], 640, 480)
        assert st.bounds.tolist() == g[5:9].tolist() and st.grid_inv.tolist() == g[9:11].tolist()
        refs = {p["name"]: FC.reference(p, kfs, g) for p in problems}
        check(run_batch((ex, spslam_match), Slots(kfs), problems)[0], refs, problems)
        p, k = problems[0], kfs[0]
        res, nf = spslam_match.FuseSearch(ex)(p["Tcw"], p["P"], k["kun"], k["desc"], k["ur"], k["go"], k["gi"])
        check([(res, nf)], refs, [p])
    finally:
        ex.close()


def test_validation_returns_errors_without_launching(gpu, cases):
    import spslam_gpu
    ex, M = gpu
    fs = M.FuseSearch(ex)
    with pytest.raises(spslam_gpu.SpslamError, match="fuse_search"):
        fs.batch_device(0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 8, 0, 1, 1)
    with pytest.raises(spslam_gpu.SpslamError, match="fuse_search"):
        fs.batch_device(1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1)
    with pytest.raises(spslam_gpu.SpslamError, match="fuse_search"):
        fs.batch_device(1, 1, 0, 4, 1, 1, 1, 1, 1, 1, 8, 0, 1, 1)
