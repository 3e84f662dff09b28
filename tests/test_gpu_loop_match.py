"""GPU parity: LoopClosing's four ORBmatcher overloads on gfx950 -- SearchByBoW(KF, KF), SearchBySim3,
SearchByProjection(pKF, Scw) and the search of Fuse(pKF, Scw), each in its device-resident form and its host-pointer
form -- against the scalar restatements of tests/loop_match_ref.py.  Bar: every record, match array and count byte
for byte, and every byte between and after the problems' output ranges as it was.  The cases are
tests/loop_match_cases.py; tests/test_loop_match_host.py guards that each of them reaches what it is there for."""
import numpy as np
import pytest

import loop_match_cases as C

pytestmark = pytest.mark.gpu

SENT = 0xCD
SENT32 = np.frombuffer(bytes([SENT] * 4), np.int32)[0]
GAP = 3  # sentinel entries between the problems' output ranges


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
def bow():
    cases = C.bow_cases()
    return cases, [C.bow_reference(c) for c in cases]


@pytest.fixture(scope="module")
def sim3():
    points, bad, cases, _ = C.sim3_cases()
    return points, bad, cases, [C.sim3_reference(c, points, bad) for c in cases]


@pytest.fixture(scope="module")
def scw():
    kfs, proj, fuse = C.scw_cases()
    return kfs, proj, [C.proj_reference(p, kfs) for p in proj], fuse, [C.fuse_reference(p, kfs) for p in fuse]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


class Slots:
    """Keyframes in the frame stage's batch layouts, on the device (no uright: the loop matchers do not read it)."""

    def __init__(self, kfs):
        import spslam_gpu as G
        S = len(kfs)
        self.cap = cap = max(max(len(k["kun"]) for k in kfs), 1)
        kun, desc = np.zeros((S, cap), G.KEYPOINT_DTYPE), np.zeros((S, cap, 32), np.uint8)
        go, gi, counts = np.zeros((S, 64 * 48 + 1), np.int32), np.zeros((S, cap), np.int32), np.zeros(S, np.int32)
        for s, k in enumerate(kfs):
            n = len(k["kun"])
            kun[s, :n], desc[s, :n], go[s], counts[s] = k["kun"], k["desc"], k["go"], n
            gi[s, :len(k["gi"])] = k["gi"]
        self.counts = counts
        self.d = [dev(a) for a in (kun, desc, go, gi, counts)]

    def ptrs(self):
        return [t.data_ptr() for t in self.d]


# ---------------------------------------------------------------- SearchByBoW(KF, KF)
def bow_side(kfs):
    """The keyframes as slots of one spslam_bow_side; returns (BowSide, cap, the tensors that back it)."""
    import spslam_gpu as G
    import spslam_loop as L
    S = len(kfs)
    cap = max(max(len(k["desc"]) for k in kfs), 1)
    desc, keys = np.zeros((S, cap, 32), np.uint8), np.zeros((S, cap), G.KEYPOINT_DTYPE)
    has, counts = np.zeros((S, cap), np.uint8), np.zeros(S, np.int32)
    nodes, start = np.zeros((S, cap), np.uint32), np.zeros((S, cap + 1), np.int32)
    feats, n_fv = np.zeros((S, cap), np.int32), np.zeros(S, np.int32)
    for s, k in enumerate(kfs):
        n, f = len(k["desc"]), k["fv"]
        desc[s, :n], keys[s, :n], has[s, :n], counts[s] = k["desc"], k["keys_un"], k["has_point"], n
        n_fv[s] = len(f["nodes"])
        nodes[s, :n_fv[s]], start[s, :n_fv[s] + 1] = f["nodes"], f["start"]
        feats[s, :len(f["features"])] = f["features"]
    t = [dev(a) for a in (desc, keys, has, counts, nodes, start, feats, n_fv)]
    return L.BowSide(*[x.data_ptr() for x in t], cap, 0), cap, t


def run_bow(gpu, cases, nn_ratio, check_ori, swap=False):
    import torch
    ex, lm = gpu
    A, cap1, keep1 = bow_side([c["kf1"] for c in cases])
    B, cap2, keep2 = bow_side([c["kf2"] for c in cases])
    order = list(range(len(cases)))[::-1] if swap else list(range(len(cases)))
    pairs = np.array([(i, i) for i in order], np.int32)
    d_pairs = dev(pairs)
    P = len(pairs)
    d_match = torch.full(((P + 1) * cap1 * 4,), SENT, dtype=torch.uint8, device="cuda")
    d_n = torch.full(((P + 1) * 4,), SENT, dtype=torch.uint8, device="cuda")
    lm.search_by_bow_kf_batch_device(P, d_pairs.data_ptr(), A, B, d_match.data_ptr(), d_n.data_ptr(), nn_ratio,
                                     check_ori)
    torch.cuda.synchronize()
    m, n = host(d_match, np.int32).reshape(P + 1, cap1), host(d_n, np.int32)
    out = {}
    for p, i in enumerate(order):
        n1 = len(cases[i]["kf1"]["desc"])
        assert (m[p, n1:] == SENT32).all(), cases[i]["name"]            # nothing past the keyframe's keypoints
        out[i] = (m[p, :n1].copy(), int(n[p]))
    assert (m[P] == SENT32).all() and n[P] == SENT32                     # nothing after the last pair
    return [out[i] for i in range(len(cases))]


def test_bow_kf_batches_match_the_restatement(gpu, bow):
    """Every case, in one launch per (nn_ratio, orientation) setting: up to 19 pairs over slots of one capacity."""
    cases, refs = bow
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault((c["nn_ratio"], c["check_ori"]), []).append(i)
    assert len(groups) >= 3 and max(len(g) for g in groups.values()) > C.BOW_WAVES
    for (nn, ori), idx in groups.items():
        for swap in (False, True):
            got = run_bow(gpu, [cases[i] for i in idx], nn, ori, swap)
            for i, (m, n) in zip(idx, got):
                want_m, want_n = refs[i]
                assert m.tobytes() == want_m.tobytes(), (cases[i]["name"], np.flatnonzero(m != want_m)[:8])
                assert n == want_n, (cases[i]["name"], n, want_n)


def test_bow_kf_host_form(gpu, bow):
    ex, lm = gpu
    cases, refs = bow
    for c, (want_m, want_n) in zip(cases, refs):
        m, n = lm.search_by_bow_kf(c["kf1"], c["kf2"], c["nn_ratio"], c["check_ori"])
        assert m.tobytes() == want_m.tobytes() and n == want_n, c["name"]


# ---------------------------------------------------------------- SearchBySim3
def run_sim3(gpu, cases, points, bad, with_bad=True):
    """One call over `cases` (all with, or all without, the already2 override).  Keyframe k of the map sits in slot
    n_kf - 1 - k, the pairs' match12 ranges are GAP apart and their result offsets reversed."""
    import torch
    import spslam_loop as L
    ex, lm = gpu
    kfs = [k for c in cases for k in (c["kf1"], c["kf2"])]
    n_kf = len(kfs)
    slots = Slots(kfs[::-1])
    cap = slots.cap
    kf_slot = np.arange(n_kf - 1, -1, -1).astype(np.int32)
    Tcw = np.stack([k["Tcw"] for k in kfs]).astype(np.float32)
    off = np.zeros(n_kf + 1, np.int32)
    off[1:] = np.cumsum([len(k["kun"]) for k in kfs])
    rows = np.concatenate([k["match_row"] for k in kfs] + [np.zeros(1, np.int32)]).astype(np.int32)
    override = cases[0]["already2"] is not None
    assert all((c["already2"] is not None) == override for c in cases)
    P = len(cases)
    rec = np.zeros(P, L.SIM3_PAIR_DTYPE)
    total, m_off = GAP, []
    a2 = np.zeros((P, cap), np.uint8)
    for p, c in enumerate(cases):
        n1 = len(c["kf1"]["kun"])
        rec[p]["kf1"], rec[p]["kf2"], rec[p]["match_offset"], rec[p]["result_offset"] = 2 * p, 2 * p + 1, total, P - 1 - p
        rec[p]["s12"], rec[p]["R12"], rec[p]["t12"] = c["s12"], c["R12"].reshape(9), c["t12"]
        m_off.append(total)
        total += n1 + GAP
        if override:
            a2[p, :len(c["already2"])] = c["already2"]
    m_in = np.full(total, SENT32, np.int32)
    for c, o in zip(cases, m_off):
        m_in[o:o + len(c["match12"])] = c["match12"]
    t = [dev(a) for a in (Tcw, kf_slot, off, rows, bad, points, rec, a2)]
    smap = L.Sim3Map(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                     t[4].data_ptr() if with_bad else 0, t[5].data_ptr())
    d_m = dev(m_in)
    d_nf = torch.full(((P + 1) * 4,), SENT, dtype=torch.uint8, device="cuda")
    th = {c["th"] for c in cases}
    assert len(th) == 1
    lm.search_by_sim3_batch_device(P, t[6].data_ptr(), smap, *slots.ptrs(), cap, t[7].data_ptr() if override else 0,
                                   d_m.data_ptr(), d_nf.data_ptr(), th.pop())
    torch.cuda.synchronize()
    m, nf = host(d_m, np.int32), host(d_nf, np.int32)
    inside = np.zeros(total, bool)
    for c, o in zip(cases, m_off):
        inside[o:o + len(c["match12"])] = True
    assert (m[~inside] == SENT32).all() and nf[P] == SENT32               # nothing between or after the ranges
    return [(m[o:o + len(c["match12"])].copy(), int(nf[P - 1 - p])) for p, (c, o) in enumerate(zip(cases, m_off))]


def check_sim3(got, cases, refs):
    for (m, nf), c, (want_m, want_nf) in zip(got, cases, refs):
        assert m.tobytes() == want_m.tobytes(), (c["name"], np.flatnonzero(m != want_m)[:8])
        assert nf == want_nf, (c["name"], nf, want_nf)


def test_sim3_batches_match_the_restatement(gpu, sim3):
    points, bad, cases, refs = sim3
    for override in (False, True):
        idx = [i for i, c in enumerate(cases) if (c["already2"] is not None) == override]
        assert len(idx) >= 2
        got = run_sim3(gpu, [cases[i] for i in idx], points, bad)
        check_sim3(got, [cases[i] for i in idx], [refs[i] for i in idx])


def test_sim3_without_a_bad_table_and_single_pair_launches(gpu, sim3):
    points, bad, cases, refs = sim3
    by_name = {c["name"]: i for i, c in enumerate(cases)}
    # no point of the real pair is bad: the same results without the table
    idx = [by_name[n] for n in ("real_ground_truth", "real_cut_65_63")]
    check_sim3(run_sim3(gpu, [cases[i] for i in idx], points, bad, with_bad=False), [cases[i] for i in idx],
               [refs[i] for i in idx])
    for n in ("hand_edges", "real_cut_0_65", "real_cut_64_0"):
        i = by_name[n]
        check_sim3(run_sim3(gpu, [cases[i]], points, bad), [cases[i]], [refs[i]])


def test_sim3_host_form(gpu, sim3):
    ex, lm = gpu
    points, bad, cases, refs = sim3
    for c, (want_m, want_nf) in zip(cases, refs):
        if c["name"] in ("real_no_initial_matches", "real_scale_1p01"):
            continue
        m, nf = lm.search_by_sim3(c["kf1"], c["kf2"], points, bad, c["s12"], c["R12"], c["t12"], c["match12"],
                                  c["already2"], c["th"])
        assert m.tobytes() == want_m.tobytes() and nf == want_nf, c["name"]


# ---------------------------------------------------------------- Fuse(pKF, Scw) and SearchByProjection(pKF, Scw)
def pack(problems):
    """Problem records over one packed point table, out ranges GAP apart: (records, points, out offsets, total)."""
    import spslam_loop as L
    rec = np.zeros(len(problems), L.FUSE_PROBLEM_DTYPE)
    pts, out_off, total, at = [], [], GAP, 0
    for n, p in enumerate(problems):
        rec[n]["Tcw"], rec[n]["kf_slot"], rec[n]["point_offset"] = p["Scw"], p["kf"], at
        rec[n]["n_points"], rec[n]["out_offset"] = len(p["P"]), total
        pts.append(p["P"])
        at += len(p["P"])
        out_off.append(total)
        total += len(p["P"]) + GAP
    points = np.concatenate(pts + [np.zeros(1, L.LOCAL_POINT_DTYPE)])
    skip = np.full(total, SENT, np.uint8)
    for p, o in zip(problems, out_off):
        skip[o:o + len(p["P"])] = 0 if p["skip"] is None else p["skip"]
    return rec, points, skip, out_off, total


def run_fuse(gpu, slots, problems, with_skip=True):
    import torch
    import spslam_loop as L
    ex, lm = gpu
    rec, points, skip, out_off, total = pack(problems)
    d_rec, d_pts, d_skip = dev(rec), dev(points), dev(skip)
    d_res = torch.full((total * 8,), SENT, dtype=torch.uint8, device="cuda")
    d_nf = torch.full(((len(problems) + 1) * 4,), SENT, dtype=torch.uint8, device="cuda")
    th = {p["th"] for p in problems}
    assert len(th) == 1
    lm.fuse_sim3_search_batch_device(len(problems), d_rec.data_ptr(), d_pts.data_ptr(),
                                     max(len(p["P"]) for p in problems), *slots.ptrs(), slots.cap,
                                     d_skip.data_ptr() if with_skip else 0, d_res.data_ptr(), d_nf.data_ptr(), th.pop())
    torch.cuda.synchronize()
    res, nf = host(d_res, L.FUSE_RESULT_DTYPE), host(d_nf, np.int32)
    inside = np.zeros(total, bool)
    for p, o in zip(problems, out_off):
        inside[o:o + len(p["P"])] = True
    assert (res.view(np.uint8).reshape(total, 8)[~inside] == SENT).all() and nf[len(problems)] == SENT32
    assert np.array_equal(d_skip.cpu().numpy(), skip)
    return [(res[o:o + len(p["P"])], int(nf[n])) for n, (p, o) in enumerate(zip(problems, out_off))]


def check_fuse(got, problems, refs):
    for (res, nf), p, (want, want_nf) in zip(got, problems, refs):
        assert res.tobytes() == want.astype(res.dtype).tobytes(), \
            (p["name"], [(i, res[i], want[i]) for i in np.flatnonzero(res != want.astype(res.dtype))[:5]])
        assert nf == want_nf, (p["name"], nf, want_nf)


def by_th(problems):
    groups = {}
    for i, p in enumerate(problems):
        groups.setdefault(p["th"], []).append(i)
    return groups


def test_fuse_sim3_batches_match_the_restatement(gpu, scw):
    kfs, _, _, fuse, refs = scw
    slots = Slots(kfs)
    groups = by_th(fuse)
    assert sorted(groups) == [4.0, 30.0] and len(groups[4.0]) >= 15
    for th, idx in groups.items():
        check_fuse(run_fuse(gpu, slots, [fuse[i] for i in idx]), [fuse[i] for i in idx], [refs[i] for i in idx])
    idx = [i for i in groups[4.0] if fuse[i]["skip"] is None]          # the same without the flag array
    check_fuse(run_fuse(gpu, slots, [fuse[i] for i in idx], with_skip=False), [fuse[i] for i in idx],
               [refs[i] for i in idx])


def test_fuse_sim3_host_form(gpu, scw):
    ex, lm = gpu
    kfs, _, _, fuse, refs = scw
    for p, ref in zip(fuse, refs):
        if p["name"] in ("real", "real_skip", "real_n63", "real_n64"):
            continue
        k = kfs[p["kf"]]
        res, nf = lm.fuse_sim3_search(p["Scw"], p["P"], k["kun"], k["desc"], k["go"], k["gi"], p["skip"], p["th"])
        check_fuse([(res, nf)], [p], [ref])


def run_proj(gpu, slots, kfs, problems, with_flags=True):
    import torch
    ex, lm = gpu
    rec, points, skip, out_off, total = pack(problems)
    P, cap = len(problems), slots.cap
    taken = np.zeros((P, cap), np.uint8)
    for n, p in enumerate(problems):
        if p["taken"] is not None:
            taken[n, :len(p["taken"])] = p["taken"]
    d_rec, d_pts, d_skip, d_taken = dev(rec), dev(points), dev(skip), dev(taken)
    d_match = torch.full(((P + 1) * cap * 4,), SENT, dtype=torch.uint8, device="cuda")
    d_n = torch.full(((P + 1) * 4,), SENT, dtype=torch.uint8, device="cuda")
    th = {p["th"] for p in problems}
    assert len(th) == 1
    lm.search_by_projection_sim3_batch_device(P, d_rec.data_ptr(), d_pts.data_ptr(),
                                              max(len(p["P"]) for p in problems), *slots.ptrs(), cap,
                                              d_skip.data_ptr() if with_flags else 0,
                                              d_taken.data_ptr() if with_flags else 0, d_match.data_ptr(),
                                              d_n.data_ptr(), th.pop())
    torch.cuda.synchronize()
    m, n = host(d_match, np.int32).reshape(P + 1, cap), host(d_n, np.int32)
    out = []
    for q, p in enumerate(problems):
        n_kp = len(kfs[p["kf"]]["kun"])
        assert (m[q, n_kp:] == SENT32).all(), p["name"]                  # nothing past the keyframe's keypoints
        out.append((m[q, :n_kp].copy(), int(n[q])))
    assert (m[P] == SENT32).all() and n[P] == SENT32
    assert np.array_equal(d_skip.cpu().numpy(), skip) and np.array_equal(d_taken.cpu().numpy().reshape(P, cap), taken)
    return out


def check_proj(got, problems, refs):
    for (m, n), p, (want_m, want_n) in zip(got, problems, refs):
        assert m.tobytes() == want_m.tobytes(), (p["name"], np.flatnonzero(m != want_m)[:8], n, want_n)
        assert n == want_n, (p["name"], n, want_n)


def test_projection_sim3_batches_match_the_restatement(gpu, scw):
    kfs, proj, refs, _, _ = scw
    slots = Slots(kfs)
    groups = by_th(proj)
    assert sorted(groups) == [4.0, 10.0, 30.0] and len(groups[10.0]) >= 20
    for th, idx in groups.items():
        check_proj(run_proj(gpu, slots, kfs, [proj[i] for i in idx]), [proj[i] for i in idx], [refs[i] for i in idx])
    idx = [i for i in groups[10.0] if proj[i]["skip"] is None and proj[i]["taken"] is None]
    assert len(idx) >= 8                                               # the same without the two flag arrays
    check_proj(run_proj(gpu, slots, kfs, [proj[i] for i in idx], with_flags=False), [proj[i] for i in idx],
               [refs[i] for i in idx])


def test_projection_sim3_same_batch_twice_in_two_orders(gpu, scw):
    """Nothing is carried from launch to launch, the scratch windows included."""
    kfs, proj, refs, _, _ = scw
    slots = Slots(kfs)
    idx = by_th(proj)[10.0]
    a = run_proj(gpu, slots, kfs, [proj[i] for i in idx])
    b = run_proj(gpu, slots, kfs, [proj[i] for i in idx[::-1]])
    check_proj(a, [proj[i] for i in idx], [refs[i] for i in idx])
    for (ma, na), (mb, nb) in zip(a, b[::-1]):
        assert ma.tobytes() == mb.tobytes() and na == nb


def test_projection_sim3_host_form(gpu, scw):
    ex, lm = gpu
    kfs, proj, refs, _, _ = scw
    for p, ref in zip(proj, refs):
        if p["name"] in ("real", "real_scale_2", "real_n63", "real_n64"):
            continue
        k = kfs[p["kf"]]
        m, n = lm.search_by_projection_sim3(p["Scw"], p["P"], k["kun"], k["desc"], k["go"], k["gi"], p["skip"],
                                            p["taken"], p["th"])
        check_proj([(m, n)], [p], [ref])


# ---------------------------------------------------------------- argument checking
def test_validation_returns_errors_without_launching(gpu, bow, sim3, scw):
    import spslam_gpu
    import spslam_loop as L
    ex, lm = gpu
    with pytest.raises(spslam_gpu.SpslamError, match="fuse_sim3_search"):
        lm.fuse_sim3_search_batch_device(0, 1, 1, 1, 1, 1, 1, 1, 1, 8, 0, 1, 1)
    with pytest.raises(spslam_gpu.SpslamError, match="projection_sim3"):
        lm.search_by_projection_sim3_batch_device(1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1)
    with pytest.raises(spslam_gpu.SpslamError, match="search_by_sim3"):
        lm.search_by_sim3_batch_device(1, 1, L.Sim3Map(), 1, 1, 1, 1, 1, 8, 0, 1, 1)
    with pytest.raises(spslam_gpu.SpslamError, match="search_by_bow_kf"):
        lm.search_by_bow_kf_batch_device(1, 1, L.BowSide(), L.BowSide(), 1, 1)
    # the host forms check their indices: a feature, a grid entry, a map point and a match outside their tables
    c = bow[0][0]
    broken = dict(c["kf2"], fv=dict(c["kf2"]["fv"], features=c["kf2"]["fv"]["features"] + len(c["kf2"]["desc"])))
    with pytest.raises(spslam_gpu.SpslamError, match="outside the keypoints"):
        lm.search_by_bow_kf(c["kf1"], broken)
    kfs, proj = scw[0], scw[1]
    p = next(q for q in proj if q["name"] == "small")
    k = kfs[p["kf"]]
    gi = k["gi"].copy()
    gi[0] = len(k["kun"])
    with pytest.raises(spslam_gpu.SpslamError, match="grid entry outside"):
        lm.search_by_projection_sim3(p["Scw"], p["P"], k["kun"], k["desc"], k["go"], gi)
    with pytest.raises(spslam_gpu.SpslamError, match="grid entry outside"):
        lm.fuse_sim3_search(p["Scw"], p["P"], k["kun"], k["desc"], k["go"], gi)
    points, bad, cases, _ = sim3
    s = next(q for q in cases if q["name"] == "hand_edges")
    rows = s["kf1"]["match_row"].copy()
    rows[0] = len(points)
    with pytest.raises(spslam_gpu.SpslamError, match="map point outside"):
        lm.search_by_sim3(dict(s["kf1"], match_row=rows), s["kf2"], points, bad, s["s12"], s["R12"], s["t12"],
                          s["match12"])
    m = s["match12"].copy()
    m[0] = len(s["kf2"]["kun"])
    with pytest.raises(spslam_gpu.SpslamError, match="match12 entry outside"):
        lm.search_by_sim3(s["kf1"], s["kf2"], points, bad, s["s12"], s["R12"], s["t12"], m)
