"""GPU parity: LocalMapping::CreateNewMapPoints on gfx950 -- spslam_search_for_triangulation_batch_device,
spslam_triangulate_batch_device, spslam_create_new_points_batch_device and the two host-pointer forms -- against the
scalar restatement tests/triangulation_ref.py.  Bar: match12, nmatches, every result record, n_new, the pair
statuses, the has-point masks and every byte outside the out ranges identical.  The cases are
tests/triangulation_cases.py; tests/test_triangulation_host.py guards that each reaches what it is there for."""
import numpy as np
import pytest

import triangulation_cases as TC
import triangulation_ref as TR

pytestmark = pytest.mark.gpu

SENT = 0xCD
GAP = 3  # sentinel records between the pairs' out ranges


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
def refs():
    """The restatement over every case, computed once: {name: (case, match12, nmatches, records, n_new)}."""
    cam = TC.cam()
    out = {}
    for c in TC.search_cases():
        m, n = TR.search_for_triangulation(c["kf1"], c["kf2"], c["F12"], c["only_stereo"], c["check_orientation"], cam)
        rec, nn = TR.triangulate_all(c["kf1"], c["kf2"], m, cam)
        out[c["name"]] = (c, m, n, rec, nn)
    for c in TC.triangulation_cases():
        rec, nn = TR.triangulate_all(c["kf1"], c["kf2"], c["match12"], cam)
        out[c["name"]] = (dict(c, F12=np.zeros(9, np.float32)), c["match12"], None, rec, nn)
    return out


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Slots:
    """Keyframes in the frame stage's / the bow stage's batch layouts, on the device."""

    def __init__(self, M, kfs, cap=None):
        import spslam_gpu as G
        S = len(kfs)
        self.cap = cap = max(max(len(k["kun"]) for k in kfs), 1) if cap is None else cap
        keys, kun = np.zeros((S, cap), G.KEYPOINT_DTYPE), np.zeros((S, cap), G.KEYPOINT_DTYPE)
        ur, depth = np.zeros((S, cap), np.float32), np.zeros((S, cap), np.float32)
        desc, has = np.zeros((S, cap, 32), np.uint8), np.zeros((S, cap), np.uint8)
        counts, n_fv = np.zeros(S, np.int32), np.zeros(S, np.int32)
        nodes, start, feats = np.zeros((S, cap), np.uint32), np.zeros((S, cap + 1), np.int32), \
            np.zeros((S, cap), np.int32)
        for s, k in enumerate(kfs):
            n, fv = len(k["kun"]), k["fv"]
            keys[s, :n], kun[s, :n], ur[s, :n], depth[s, :n] = k["keys"], k["kun"], k["ur"], k["depth"]
            desc[s, :n], has[s, :n], counts[s], n_fv[s] = k["desc"], k["has"], n, len(fv["nodes"])
            nodes[s, :len(fv["nodes"])], start[s, :len(fv["start"])] = fv["nodes"], fv["start"]
            feats[s, :len(fv["features"])] = fv["features"]
        self.has0 = has
        self.d = [dev(a) for a in (keys, kun, ur, depth, desc, has, counts, nodes, start, feats, n_fv)]
        self.side = M.TriSide(*[t.data_ptr() for t in self.d], cap, 0)

    def has(self):
        return self.d[5].cpu().numpy().reshape(self.has0.shape)


def pair_records(M, cases, slots_of, flags=None):
    """TRI_PAIR_DTYPE records and out offsets of `cases` (slots_of[n] = (kf1 slot, kf2 slot))."""
    rec = np.zeros(len(cases), M.TRI_PAIR_DTYPE)
    offs, total = [], GAP
    for n, c in enumerate(cases):
        T1 = np.asarray(c["kf1"]["Tcw"], np.float32).reshape(4, 4)[:3].reshape(12)
        T2 = np.asarray(c["kf2"]["Tcw"], np.float32).reshape(4, 4)[:3].reshape(12)
        rec[n]["kf1"], rec[n]["kf2"] = slots_of[n]
        rec[n]["Tcw1"], rec[n]["Tcw2"], rec[n]["Ow1"], rec[n]["Ow2"] = T1, T2, c["kf1"]["Ow"], c["kf2"]["Ow"]
        rec[n]["F12"], rec[n]["out_offset"] = np.asarray(c["F12"], np.float32).reshape(9), total
        rec[n]["flags"] = 0 if flags is None else flags[n]
        offs.append(total)
        total += len(c["kf1"]["kun"]) + GAP
    return rec, offs, total


def outside_is_untouched(buf, item, cases, offs, total):
    inside = np.zeros(total, bool)
    for c, o in zip(cases, offs):
        inside[o:o + len(c["kf1"]["kun"])] = True
    return (buf.view(np.uint8).reshape(total, item)[~inside] == SENT).all()


def run_search(gpu, cases, only_stereo, check_orientation, flags=None, cap=None):
    """One launch over `cases`, each on two slots of its own.  Returns [(match12, nmatches)]."""
    import torch
    ex, M = gpu
    slots = Slots(M, [k for c in cases for k in (c["kf1"], c["kf2"])], cap)
    rec, offs, total = pair_records(M, cases, [(2 * n, 2 * n + 1) for n in range(len(cases))], flags)
    d_rec = dev(rec)
    d_m = torch.full((total * 4,), SENT, dtype=torch.uint8, device="cuda")
    d_n = torch.full((len(cases),), -9, dtype=torch.int32, device="cuda")
    M.SearchForTriangulation(ex).batch_device(len(cases), d_rec.data_ptr(), slots.side, only_stereo,
                                              check_orientation, d_m.data_ptr(), d_n.data_ptr())
    torch.cuda.synchronize()
    m = d_m.cpu().numpy().view(np.int32)
    assert outside_is_untouched(m, 4, cases, offs, total)
    assert np.array_equal(slots.has(), slots.has0)                             # nothing is marked
    return [(m[o:o + len(c["kf1"]["kun"])].copy(), int(k)) for c, o, k in zip(cases, offs, d_n.cpu().numpy())]


def run_triangulate(gpu, cases, matches, cap=None, mark=0):
    import torch
    ex, M = gpu
    slots = Slots(M, [k for c in cases for k in (c["kf1"], c["kf2"])], cap)
    rec, offs, total = pair_records(M, cases, [(2 * n, 2 * n + 1) for n in range(len(cases))])
    m = np.full(total, -7, np.int32)
    for o, mm in zip(offs, matches):
        m[o:o + len(mm)] = mm
    d_rec, d_m = dev(rec), dev(m)
    d_res = torch.full((total * 20,), SENT, dtype=torch.uint8, device="cuda")
    d_new = torch.full((len(cases),), -9, dtype=torch.int32, device="cuda")
    M.Triangulate(ex).batch_device(len(cases), d_rec.data_ptr(), slots.side, d_m.data_ptr(), mark, d_res.data_ptr(),
                                   d_new.data_ptr())
    torch.cuda.synchronize()
    res = d_res.cpu().numpy()
    assert outside_is_untouched(res, 20, cases, offs, total)
    assert np.array_equal(d_m.cpu().numpy().view(np.int32), m)
    r = res.view(M.TRI_RESULT_DTYPE)
    return [(r[o:o + len(c["kf1"]["kun"])].copy(), int(k)) for c, o, k in zip(cases, offs, d_new.cpu().numpy())], slots


def same_records(got, want, name):
    """Byte for byte, except that a NaN coordinate matches a NaN coordinate whatever its sign and payload (the
    sweep-limit case: the device's and numpy's conversions make different NaNs)."""
    got, want = got.copy(), want.astype(got.dtype)
    for f in ("x", "y", "z"):
        nan = np.isnan(got[f])
        assert np.array_equal(nan, np.isnan(want[f])), (name, f)
        got[f][nan] = 0
        want[f][nan] = 0
    assert got.tobytes() == want.tobytes(), \
        (name, [(i, got[i], want[i]) for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()][:5])


SEARCH_PLAIN = ["lists", "ties_thresholds_has", "epipole_radius", "octaves", "c2z_zero", "zero_F12",
                "stereo_mix_only0", "all_key1_hold_points", "key1_empty", "key2_empty", "empty_feature_vectors",
                "disjoint_feature_vectors", "real0", "real2"]


def test_search_batch_matches_the_restatement(gpu, refs):
    """14 pairs in one launch, out ranges separated by sentinels, a cap (206) that is no multiple of 64; then the
    same launch again: identical bytes."""
    cases = [refs[n][0] for n in SEARCH_PLAIN]
    assert TC.real_search_cases()[0]["name"] == "real0" and len(cases[-1]["kf1"]["kun"]) % 64
    first = run_search(gpu, cases, 0, 0)
    for (m, n), name in zip(first, SEARCH_PLAIN):
        assert np.array_equal(m, refs[name][1]), (name, np.flatnonzero(m != refs[name][1])[:8])
        assert n == refs[name][2], (name, n, refs[name][2])
    again = run_search(gpu, cases, 0, 0)
    for (m, n), (m2, n2) in zip(first, again):
        assert m.tobytes() == m2.tobytes() and n == n2


def test_search_flags_and_the_skip_bit(gpu, refs):
    for names, only_stereo, ori in ((["stereo_mix_only1", "real2_only_stereo"], 1, 0),
                                    (["orientation_bins_removed", "orientation_second_below_tenth",
                                      "real0_orientation"], 0, 1)):
        got = run_search(gpu, [refs[n][0] for n in names], only_stereo, ori)
        for (m, n), name in zip(got, names):
            assert np.array_equal(m, refs[name][1]) and n == refs[name][2], name
    names = ["real0", "lists", "real2", "octaves", "ties_thresholds_has"]    # a batch of 5, the middle one skipped
    got = run_search(gpu, [refs[n][0] for n in names], 0, 0, flags=[0, 0, 1, 0, 0], cap=333)
    for k, ((m, n), name) in enumerate(zip(got, names)):
        if k == 2:
            assert (m == -1).all() and n == 0
        else:
            assert np.array_equal(m, refs[name][1]) and n == refs[name][2], name


def test_triangulation_batch_matches_the_restatement(gpu, refs):
    names = [c["name"] for c in TC.triangulation_cases()] + ["real0", "real2", "lists", "key1_empty"]
    cases = [refs[n][0] for n in names]
    got, slots = run_triangulate(gpu, cases, [refs[n][1] for n in names])
    for (rec, nn), name in zip(got, names):
        same_records(rec, refs[name][3], name)
        assert nn == refs[name][4], (name, nn, refs[name][4])
    assert np.array_equal(slots.has(), slots.has0)                             # mark = 0
    again, _ = run_triangulate(gpu, cases, [refs[n][1] for n in names])
    for (rec, nn), (rec2, nn2) in zip(got, again):
        assert rec.tobytes() == rec2.tobytes() and nn == nn2
    # mark = 1 on its own slots: exactly the accepted idx1 / idx2 bytes are set
    sub = ["real0", "mixed_70", "new_stereo2"]
    got, slots = run_triangulate(gpu, [refs[n][0] for n in sub], [refs[n][1] for n in sub], mark=1)
    want = slots.has0.copy()
    for k, name in enumerate(sub):
        rec = refs[name][3]
        same_records(got[k][0], rec, name)
        for i in np.flatnonzero(rec["status"] == TR.NEW):
            want[2 * k, i] = 1
            want[2 * k + 1, rec[i]["idx2"]] = 1
    assert np.array_equal(slots.has(), want) and (want != slots.has0).sum() >= 40


def test_host_forms_equal_the_batch_forms(gpu, refs):
    ex, M = gpu
    search, tri = M.SearchForTriangulation(ex), M.Triangulate(ex)
    for name in [c["name"] for c in TC.search_cases()]:             # every search case, with its own flags
        c, m, n, rec, nn = refs[name]
        pairs, got_n = search(c["kf1"], c["kf2"], c["F12"], c["only_stereo"], c["check_orientation"])
        want = np.array([(i, m[i]) for i in range(len(m)) if m[i] >= 0], np.int32).reshape(-1, 2)
        assert got_n == n and np.array_equal(pairs, want), name
        res, got_new = tri(c["kf1"], c["kf2"], pairs)
        same_records(res, rec[want[:, 0]] if len(want) else rec[:0], name)
        assert got_new == nn, name
    for c in TC.triangulation_cases():
        _, m, _, rec, nn = refs[c["name"]]
        want = np.array([(i, m[i]) for i in range(len(m)) if m[i] >= 0], np.int32).reshape(-1, 2)
        res, got_new = tri(c["kf1"], c["kf2"], want)
        same_records(res, rec[want[:, 0]], c["name"])
        assert got_new == nn, c["name"]


def test_three_chained_rounds_of_two_sequences(gpu):
    """Keyframe 0 of two sequences against its three neighbours (the second below the baseline): three calls on one
    stream without synchronisation in between, both sequences in each call."""
    import torch
    ex, M = gpu
    cam = TC.cam()
    models = [TC.chained_model(seq) for seq in TC.SEQS]
    order = [0, TC.STEP, 3, 2 * TC.STEP]
    kfs = [model["kfs"][fi] for model, _, _ in models for fi in order]
    slots = Slots(M, kfs, cap=211)
    rounds_rec, outs = [], []
    for r in range(3):
        cases, slots_of = [], []
        for s, (model, k1, nb) in enumerate(models):
            kf1, kf2 = model["kfs"][k1], model["kfs"][nb[r]]
            cases.append(dict(kf1=kf1, kf2=kf2, F12=TR.compute_f12(kf1, kf2, TC.Kmat())))
            slots_of.append((4 * s, 4 * s + 1 + r))
        rec, offs, total = pair_records(M, cases, slots_of)
        rounds_rec.append((cases, offs, total, dev(rec)))
    stream = torch.cuda.Stream()
    create = M.CreateNewPoints(ex)
    with torch.cuda.stream(stream):
        for cases, offs, total, d_rec in rounds_rec:
            o = dict(m=torch.full((total * 4,), SENT, dtype=torch.uint8, device="cuda"),
                     res=torch.full((total * 20,), SENT, dtype=torch.uint8, device="cuda"),
                     n=torch.full((2,), -9, dtype=torch.int32, device="cuda"),
                     new=torch.full((2,), -9, dtype=torch.int32, device="cuda"),
                     st=torch.full((2,), SENT, dtype=torch.uint8, device="cuda"))
            outs.append(o)
        stream.synchronize()                                                   # the fills; none between the rounds
        for (cases, offs, total, d_rec), o in zip(rounds_rec, outs):
            create.batch_device(2, d_rec.data_ptr(), slots.side, o["m"].data_ptr(), o["n"].data_ptr(),
                                o["res"].data_ptr(), o["new"].data_ptr(), o["st"].data_ptr(),
                                stream=stream.cuda_stream)
    stream.synchronize()
    total_new = 0
    for s, (model, k1, nb) in enumerate(models):
        want, nnew = TR.create_new_map_points(model, k1, nb, cam, TC.Kmat())
        assert [w[0] for w in want] == [TR.SEARCHED, TR.SHORT_BASELINE, TR.SEARCHED]
        for r, (st, m, rec) in enumerate(want):
            cases, offs, total, _ = rounds_rec[r]
            o = outs[r]
            n1 = len(cases[s]["kf1"]["kun"])
            got_m = o["m"].cpu().numpy().view(np.int32)[offs[s]:offs[s] + n1]
            got_rec = o["res"].cpu().numpy().view(M.TRI_RESULT_DTYPE)[offs[s]:offs[s] + n1]
            assert int(o["st"][s]) == st, (s, r)
            if st == TR.SEARCHED:
                assert np.array_equal(got_m, m), (s, r)
                same_records(got_rec, rec, (s, r))
                assert int(o["n"][s]) == int((m >= 0).sum()) and int(o["new"][s]) == int((rec["status"] == 0).sum())
            else:
                assert (got_m == -1).all() and (got_rec["status"] == TR.NO_MATCH).all()
                assert int(o["n"][s]) == 0 and int(o["new"][s]) == 0
            assert outside_is_untouched(o["m"].cpu().numpy(), 4, cases, offs, total)
            assert outside_is_untouched(o["res"].cpu().numpy(), 20, cases, offs, total)
        total_new += nnew
        has = slots.has()
        for q, fi in enumerate(order):                                         # the masks after the three rounds
            kf = model["kfs"][fi]
            want_has = np.array([i in kf["points"] for i in range(len(kf["kun"]))], np.uint8)
            assert np.array_equal(has[4 * s + q, :len(want_has)], want_has), (s, fi)
            assert (has[4 * s + q, len(want_has):] == 0).all()
    assert total_new >= 30


def test_validation_returns_errors_without_launching(gpu):
    import spslam_gpu
    ex, M = gpu
    c = TC.search_cases()[1]
    slots = Slots(M, [c["kf1"], c["kf2"]])
    s, t, cr = M.SearchForTriangulation(ex), M.Triangulate(ex), M.CreateNewPoints(ex)
    with pytest.raises(spslam_gpu.SpslamError, match="search_for_triangulation"):
        s.batch_device(0, 1, slots.side, 0, 0, 1, 1)
    big = M.TriSide(*[t_.data_ptr() for t_ in slots.d], 8193, 0)
    with pytest.raises(spslam_gpu.SpslamError, match="search_for_triangulation"):
        s.batch_device(1, 1, big, 0, 0, 1, 1)
    with pytest.raises(spslam_gpu.SpslamError, match="triangulate"):
        t.batch_device(1, 1, big, 1, 0, 1, 1)
    with pytest.raises(spslam_gpu.SpslamError, match="triangulate"):
        t.batch_device(1, 1, slots.side, 0, 0, 1, 1)
    with pytest.raises(spslam_gpu.SpslamError, match="create_new_points"):
        cr.batch_device(1, 1, slots.side, 1, 1, 1, 1, 0)
    no_has = M.TriSide(*[0 if k == 5 else t_.data_ptr() for k, t_ in enumerate(slots.d)], slots.cap, 0)
    with pytest.raises(spslam_gpu.SpslamError, match="create_new_points"):
        cr.batch_device(1, 1, no_has, 1, 1, 1, 1, 1)
