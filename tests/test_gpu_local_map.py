"""GPU parity: Tracking::UpdateLocalMap (UpdateLocalKeyFrames + UpdateLocalPoints, src/Tracking.cc:1427-1571) on
gfx950 -- spslam_track_update_local_map_batch_device and its host-pointer form -- against the scalar restatement
tests/local_map_ref.py.  Bar: every output array identical (lists, counts, kf_max, status, the gathered records
byte for byte).  The cases are tests/local_map_cases.py; tests/test_local_map_host.py guards that each of them
reaches what it is there for."""
import ctypes

import numpy as np
import pytest

import local_map_cases as LC
import local_map_ref as R

pytestmark = pytest.mark.gpu

CASES = LC.build_cases()
SENT = -7


@pytest.fixture(scope="module")
def gpu():
    import spslam_frame
    import spslam_gpu
    import spslam_track
    import synth
    K = synth.TUM3
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], (0,) * 5, K["bf"], 640, 480)
    yield ex, spslam_track.TrackGraph(ex)
    ex.close()


def point_table(n, seed):
    """n spslam_local_point records of random bytes (the gather moves them, nothing reads them)."""
    import spslam_match
    raw = np.random.default_rng(seed).integers(0, 256, max(n, 1) * 80, dtype=np.uint8)
    return raw.view(spslam_match.LOCAL_POINT_DTYPE)[:n].copy()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


class Packed:
    """Several sequences' tables in one set of device tables (CSR offsets absolute, indices local)."""

    def __init__(self, seqs, tables):
        import spslam_track
        self.nk = len(seqs[0]["parent"])
        assert all(len(T["parent"]) == self.nk for T in seqs)
        self.n_rows = [len(T["obs_off"]) - 1 for T in seqs]
        self.row_base = np.concatenate([[0], np.cumsum(self.n_rows)]).astype(np.int32)
        self.kf_base = (np.arange(len(seqs) + 1) * self.nk).astype(np.int32)

        def csr(off, val):
            o, base = [], 0
            for T in seqs:
                o.append(T[off][:-1] + base)
                base += len(T[val])
            return np.concatenate(o + [[base]]).astype(np.int32), np.concatenate([T[val] for T in seqs] + [[0]])
        arrays = {}
        arrays["obs_off"], arrays["obs_kf"] = csr("obs_off", "obs_kf")
        arrays["child_off"], arrays["child"] = csr("child_off", "child")
        arrays["match_off"], arrays["match_row"] = csr("match_off", "match_row")
        for name in ("point_bad", "kf_bad", "covis", "parent"):
            arrays[name] = np.concatenate([np.asarray(T[name]).reshape(-1) for T in seqs] + [[0]])
        self.points = np.concatenate(tables)
        self.d = {name: dev(np.asarray(arrays[name], dt)) for name, dt in spslam_track.LOCAL_MAP_TABLES}
        self.d["points"] = dev(self.points if len(self.points) else point_table(1, 0))


def run_device(tg, pk, frames, capacity, records=True, scratch=None, state=None, mm=None, id_to_row=None,
               id_base=None, keep=None):
    """frames: [(sequence, frame_rows, local_kfs on entry)].  Outputs are sentinel-filled before the launch.
    Returns the outputs as numpy arrays (and the device buffers, for a second launch via keep=)."""
    import spslam_match
    import spslam_track
    import torch
    F = len(frames)
    cap = max(max(len(fr[1]) for fr in frames), 1)
    rows = np.full((F, cap), -1, np.int32)
    counts = np.zeros(F, np.int32)
    kfs_in = np.full((F, pk.nk), SENT, np.int32)
    n_in = np.zeros(F, np.int32)
    for f, (s, r, lk) in enumerate(frames):
        rows[f, :len(r)], counts[f] = r, len(r)
        kfs_in[f, :len(lk)], n_in[f] = lk, len(lk)
    stride = max(max(pk.n_rows), 1)
    lfr = np.zeros(F, spslam_match.LOCAL_FRAME_DTYPE)
    lfr["Tcw"], lfr["point_offset"], lfr["n_points"] = 3.5, SENT, SENT
    lfr["seen_offset"], lfr["stamp"] = 11, 12
    if keep is None:
        b = dict(rows=dev(rows), counts=dev(counts), kf_base=dev(pk.kf_base[[fr[0] for fr in frames]]),
                 row_base=dev(pk.row_base[[fr[0] for fr in frames]]), kfs=dev(kfs_in), n_kfs=dev(n_in),
                 kf_max=dev(np.full(F, SENT, np.int32)), lrows=dev(np.full((F, max(capacity, 1)), SENT, np.int32)),
                 n_local=dev(np.full(F, SENT, np.int32)), status=dev(np.full(F, SENT, np.int32)),
                 rec=dev(np.full(F * max(capacity, 1) * 80, 0xAB, np.uint8)), lfr=dev(lfr),
                 scratch=dev(np.zeros(F * stride, np.int32) if scratch is None else scratch),
                 state=dev(np.asarray(state, np.int8)) if state is not None else None,
                 id_to_row=dev(id_to_row) if id_to_row is not None else None,
                 id_base=dev(id_base) if id_base is not None else None)
    else:
        b = keep
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    m = spslam_track.LocalMap(frame_rows=None if mm is not None else p(b["rows"]), kp_counts=p(b["counts"]),
                              id_to_row=p(b["id_to_row"]), id_base=p(b["id_base"]), kf_base=p(b["kf_base"]),
                              row_base=p(b["row_base"]), cap=cap, n_kf=pk.nk, points=p(pk.d["points"]),
                              **{name: p(pk.d[name]) for name, _ in spslam_track.LOCAL_MAP_TABLES})
    o = spslam_track.LocalMapOut(state=p(b["state"]), local_kfs=p(b["kfs"]), n_local_kfs=p(b["n_kfs"]),
                                 kf_max=p(b["kf_max"]), local_rows=p(b["lrows"]), n_local=p(b["n_local"]),
                                 status=p(b["status"]), scratch=p(b["scratch"]), kf_cap=pk.nk, capacity=capacity,
                                 scratch_stride=stride, records=p(b["rec"]) if records else None,
                                 local_frames=p(b["lfr"]) if records else None)
    tg.update_local_map_device(F, mm, m, o)
    torch.cuda.synchronize()
    C = max(capacity, 1)
    return dict(kfs=host(b["kfs"], np.int32).reshape(F, pk.nk), n_kfs=host(b["n_kfs"], np.int32),
                kf_max=host(b["kf_max"], np.int32), lrows=host(b["lrows"], np.int32).reshape(F, C),
                n_local=host(b["n_local"], np.int32), status=host(b["status"], np.int32),
                rec=host(b["rec"], np.uint8).reshape(F, C * 80), lfr=host(b["lfr"], spslam_match.LOCAL_FRAME_DTYPE),
                buffers=b, lfr_in=lfr)


def check_frame(out, f, ref, points, capacity, records=True):
    """Frame f of a device run against the restatement: everything written, and nothing past it."""
    nk, n = len(ref["local_kfs"]), len(ref["local_points"])
    assert out["n_kfs"][f] == nk and out["kfs"][f, :nk].tolist() == ref["local_kfs"]
    assert out["kf_max"][f] == ref["kf_max"]
    assert out["n_local"][f] == n and out["status"][f] == ref["status"]
    assert out["lrows"][f, :n].tolist() == ref["local_points"]
    assert (out["lrows"][f, n:capacity] == SENT).all()
    if records:
        assert out["rec"][f, :n * 80].tobytes() == points[ref["local_points"]].tobytes()
        assert (out["rec"][f, n * 80:capacity * 80] == 0xAB).all()
        want = out["lfr_in"][f].copy()
        want["point_offset"], want["n_points"] = f * capacity, n
        assert out["lfr"][f].tobytes() == want.tobytes()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_single_frame_host_form(gpu, case):
    import spslam_match
    ex, tg = gpu
    ref = LC.reference(case)
    pts = point_table(len(case["T"]["obs_off"]) - 1, 5)
    lf = np.zeros((), spslam_match.LOCAL_FRAME_DTYPE)
    lf["Tcw"], lf["point_offset"], lf["seen_offset"], lf["stamp"] = 2.0, 99, 5, 6
    r = tg.update_local_map(case["T"], case["frame_rows"], case["local_kfs"], case["capacity"], points=pts,
                            local_frame=lf)
    assert r["local_kfs"].tolist() == ref["local_kfs"] and r["kf_max"] == ref["kf_max"]
    assert r["local_rows"].tolist() == ref["local_points"] and r["status"] == ref["status"]
    assert r["records"].tobytes() == pts[ref["local_points"]].tobytes()
    want = lf.copy()
    want["point_offset"], want["n_points"] = 0, len(ref["local_points"])
    assert r["local_frame"].tobytes() == want.tobytes()
    if case["creator"] is not None and case["name"] == "observers_outvote_creator":
        assert r["kf_max"] != LC.creator_vote(case["frame_rows"], case["creator"], len(case["T"]["parent"]))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_form_does_not_depend_on_the_scratch(gpu, case):
    ex, tg = gpu
    ref = LC.reference(case)
    nr = len(case["T"]["obs_off"]) - 1
    pts = point_table(nr, 6)
    pk = Packed([case["T"]], [pts])
    frames = [(0, case["frame_rows"], case["local_kfs"])]
    fills = [np.zeros(max(nr, 1), np.int32), np.full(max(nr, 1), -1, np.int32),
             np.random.default_rng(9).integers(-2 ** 31, 2 ** 31, max(nr, 1)).astype(np.int32)]
    for fill in fills:
        out = run_device(tg, pk, frames, case["capacity"], scratch=fill)
        check_frame(out, 0, ref, pts, case["capacity"])
    # again on the buffers the last run left: the list it wrote is the list it is given, the scratch is dirty
    ref2 = R.run_tables(case["T"], case["frame_rows"], ref["local_kfs"], case["capacity"])
    out2 = run_device(tg, pk, frames, case["capacity"], keep=out["buffers"])
    assert ref2["local_kfs"] == ref["local_kfs"] and ref2["local_points"] == ref["local_points"]
    check_frame(out2, 0, ref2, pts, case["capacity"])


def _three_sequences():
    seqs, tabs, dicts = [], [], []
    for s, (seed, own) in enumerate(((31, (20, 30)), (32, (5, 9)), (33, (40, 50)))):
        P, K, _ = LC.random_map(seed, 7, own=own, p_bad_pt=0.1)
        K[(s + 2) % 7]["bad"] = True
        T = LC.tables_from_dicts(P, K)
        seqs.append(T)
        tabs.append(point_table(len(P), 40 + s))
        dicts.append(K)
    frames = [(0, LC.frame_rows(51, dicts[0], 70), []), (1, LC.frame_rows(52, dicts[1], 9), [3]),
              (0, LC.frame_rows(53, dicts[0], 300, from_kfs=(1, 2)), [1, 2]), (2, np.full(4, -1, np.int32), [6, 0, 3]),
              (1, LC.frame_rows(55, dicts[1], 257, from_kfs=(5,)), [])]
    return seqs, tabs, frames


def test_batch_of_three_sequences_equals_single_frame_calls(gpu):
    ex, tg = gpu
    seqs, tabs, frames = _three_sequences()
    pk = Packed(seqs, tabs)
    capacity = max(len(T["match_row"]) for T in seqs)
    out = run_device(tg, pk, frames, capacity)
    for f, (s, rows, lk) in enumerate(frames):
        ref = R.run_tables(seqs[s], rows, lk, capacity)
        check_frame(out, f, ref, tabs[s], capacity)
        one = tg.update_local_map(seqs[s], rows, lk, capacity, points=tabs[s])
        n, nk = out["n_local"][f], out["n_kfs"][f]
        assert one["local_kfs"].tolist() == out["kfs"][f, :nk].tolist() and one["kf_max"] == out["kf_max"][f]
        assert one["local_rows"].tolist() == out["lrows"][f, :n].tolist() and one["status"] == out["status"][f]
        assert one["records"].tobytes() == out["rec"][f, :n * 80].tobytes()
    assert len({fr[0] for fr in frames}) == 3 and (out["n_local"] > 0).all()


def test_lost_frame_is_not_touched(gpu):
    ex, tg = gpu
    seqs, tabs, frames = _three_sequences()
    pk = Packed(seqs, tabs)
    capacity = max(len(T["match_row"]) for T in seqs)
    frames = frames[:3]
    out = run_device(tg, pk, frames, capacity, state=[0, 2, 1])
    for f in (0, 2):
        check_frame(out, f, R.run_tables(seqs[frames[f][0]], frames[f][1], frames[f][2], capacity),
                    tabs[frames[f][0]], capacity)
    assert out["n_kfs"][1] == 1 and out["kfs"][1].tolist() == [3] + [SENT] * 6
    assert out["kf_max"][1] == SENT and out["n_local"][1] == SENT and out["status"][1] == SENT
    assert (out["lrows"][1] == SENT).all() and (out["rec"][1] == 0xAB).all()
    assert out["lfr"][1].tobytes() == out["lfr_in"][1].tobytes()


def test_frame_points_from_the_track_batch(gpu):
    """frame_rows == NULL: the frame's points come from the first graph's batch (edge_of_kp, point_outlier,
    proj_match, proj_points[].id) through an id -> row table, and equal the same points passed explicitly."""
    import spslam_match
    import spslam_track
    ex, tg = gpu
    seqs, tabs, frames = _three_sequences()
    pk = Packed(seqs, tabs)
    capacity = max(len(T["match_row"]) for T in seqs)
    rng = np.random.default_rng(77)
    F, cap = len(frames), max(len(fr[1]) for fr in frames)
    # per sequence: ids are a scrambled function of the row
    ids = [rng.permutation(3 * n)[:n].astype(np.int32) for n in pk.n_rows]
    id_base_seq = np.concatenate([[0], np.cumsum([3 * n for n in pk.n_rows])]).astype(np.int32)
    id_to_row = np.full(id_base_seq[-1], -1, np.int32)
    for s, a in enumerate(ids):
        id_to_row[id_base_seq[s] + a] = np.arange(len(a))
    pf = np.zeros(F, spslam_match.PROJ_FRAME_DTYPE)
    pp, match, edge, outl, counts = [], np.full((F, cap), -1, np.int32), np.full((F, cap), -1, np.int32), \
        np.zeros((F, cap), np.uint8), np.zeros(F, np.int32)
    explicit = []
    for f, (s, rows, lk) in enumerate(frames):
        n = len(rows)
        counts[f] = n
        has = np.flatnonzero(rows >= 0)
        P = np.zeros(len(has), spslam_match.PROJ_POINT_DTYPE)
        order = rng.permutation(len(has))          # the frame's last-frame points, in another order
        P["id"][order] = ids[s][rows[has]]
        pf[f]["point_offset"], pf[f]["n_points"] = sum(len(q) for q in pp), len(P)
        pp.append(P)
        match[f, has] = order
        with_edge = has[rng.uniform(size=len(has)) < 0.8]
        edge[f, with_edge] = np.arange(len(with_edge))
        outl[f, :len(with_edge)] = rng.uniform(size=len(with_edge)) < 0.25
        ex_rows = np.full(n, -1, np.int32)
        live = with_edge[outl[f, :len(with_edge)] == 0]
        ex_rows[live] = rows[live]
        explicit.append((s, ex_rows, lk))
        assert 0 < len(live) < len(has) or len(has) == 0
    d = [dev(counts), dev(pf), dev(np.concatenate(pp)), dev(match), dev(edge), dev(outl)]
    mm = spslam_track.TrackBatch(kp_counts=d[0].data_ptr(), cap=cap, proj_frames=d[1].data_ptr(),
                                 proj_points=d[2].data_ptr(), proj_match=d[3].data_ptr(), edge_of_kp=d[4].data_ptr(),
                                 point_outlier=d[5].data_ptr())
    a = run_device(tg, pk, frames, capacity, mm=mm, id_to_row=id_to_row,
                   id_base=id_base_seq[[fr[0] for fr in frames]])
    b = run_device(tg, pk, explicit, capacity)
    for f, (s, rows, lk) in enumerate(explicit):
        check_frame(a, f, R.run_tables(seqs[s], rows, lk, capacity), tabs[s], capacity)
    for k in ("kfs", "n_kfs", "kf_max", "lrows", "n_local", "status", "rec"):
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def local_pairs():
    from test_oracle_match import local_problems, make_pairs
    pairs = make_pairs(((0, 10, 12), (1, 30, 31), (2, 50, 53), (3, 5, 9), (4, 70, 71), (5, 0, 2)), seed=17)
    return local_problems(pairs, seed=23)


def test_chain_into_search_local_points(gpu, local_pairs):
    """The problems' points split over 4 keyframes with overlaps: the new entry with the record gather, then
    spslam_search_local_points_batch_device on its output, equal the CPU matcher on the restatement's list."""
    import oracle_match as OM
    import spslam_gpu as G
    import spslam_match as M
    import torch
    ex, tg = gpu
    lm = M.LocalMatcher(ex)
    rng = np.random.default_rng(23)
    seqs, tabs, frames = [], [], []
    for q in local_pairs:
        n = len(q["LP"])
        matches = {}
        for k in range(4):  # keyframe k holds the points [k n / 6, (k + 3) n / 6), shuffled, with empty slots
            lst = list(range(k * n // 6, (k + 3) * n // 6)) + [None] * (n // 20)
            matches[k] = [lst[i] for i in rng.permutation(len(lst))]
        P, K = LC.hand(4, matches, covis={0: [1], 3: [2]}, parent={1: 0, 2: 1, 3: 2})
        seqs.append(LC.tables_from_dicts(P, K))
        tabs.append(q["LP"][:len(P)])
        frames.append((len(frames), rng.choice(n // 6, 40).astype(np.int32), []))  # votes for keyframe 0 only
    pk = Packed(seqs, tabs)
    capacity = max(len(t) for t in tabs)
    out = run_device(tg, pk, frames, capacity)
    F, cap = len(local_pairs), max(len(q["kun"]) for q in local_pairs)
    kun, desc = np.zeros((F, cap), G.KEYPOINT_DTYPE), np.zeros((F, cap, 32), np.uint8)
    ur, go = np.zeros((F, cap), np.float32), np.zeros((F, 64 * 48 + 1), np.int32)
    gi, tk, counts = np.zeros((F, cap), np.int32), np.zeros((F, cap), np.uint8), np.zeros(F, np.int32)
    lfr = out["lfr"].copy()
    for f, q in enumerate(local_pairs):
        n = len(q["kun"])
        kun[f, :n], desc[f, :n], ur[f, :n], go[f] = q["kun"], q["desc"], q["ur"], q["go"]
        gi[f, :len(q["gi"])] = q["gi"]
        tk[f, :n], counts[f] = q["taken"], n
        lfr[f]["Tcw"] = q["lfr"]["Tcw"]  # Tcw is the caller's: the entry leaves it as it is
    b = out["buffers"]
    b["lfr"].copy_(dev(lfr))
    d = [dev(kun), dev(desc), dev(ur), dev(go), dev(gi), dev(counts), dev(tk)]
    d_match = torch.full((F * cap,), -9, dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(F, dtype=torch.int32, device="cuda")
    lm.batch_device(F, b["lfr"].data_ptr(), b["rec"].data_ptr(), capacity, d[0].data_ptr(), d[1].data_ptr(),
                    d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), cap, d[6].data_ptr(),
                    d_match.data_ptr(), d_nm.data_ptr())
    torch.cuda.synchronize()
    mb, nb = d_match.cpu().numpy().reshape(F, cap), d_nm.cpu().numpy()
    for f, q in enumerate(local_pairs):
        ref = R.run_tables(seqs[f], frames[f][1], [], capacity)
        check_frame(out, f, ref, tabs[f], capacity)
        assert ref["trace"]["k1"] == 1 and ref["local_kfs"] == [0, 1] and ref["trace"]["n_dup"] > 100
        fr = q["lfr"].copy()
        fr["point_offset"], fr["n_points"] = 0, len(ref["local_points"])
        mo, nmo, _ = OM.search_local_points(fr, q["LP"][ref["local_points"]], q["kun"], q["desc"], q["ur"], q["go"],
                                            q["gi"], q["geo"], taken=q["taken"])
        assert nmo > 20 and nb[f] == nmo, (f, nb[f], nmo)
        assert np.array_equal(mb[f, :len(q["kun"])], mo), f


def test_validation_returns_errors_without_launching(gpu):
    import spslam_gpu
    import spslam_track
    ex, tg = gpu
    case = CASES[1]
    pk = Packed([case["T"]], [point_table(len(case["T"]["obs_off"]) - 1, 1)])
    frames = [(0, case["frame_rows"], [])]
    out = run_device(tg, pk, frames, 8)
    b = out["buffers"]
    before = {k: out[k].copy() for k in ("kfs", "n_kfs", "kf_max", "lrows", "n_local", "status", "rec")}

    def structs(**over):
        p = lambda t: t.data_ptr()  # noqa: E731
        m = dict(frame_rows=p(b["rows"]), kp_counts=p(b["counts"]), kf_base=p(b["kf_base"]), row_base=p(b["row_base"]),
                 cap=3, n_kf=pk.nk, points=p(pk.d["points"]),
                 **{name: p(pk.d[name]) for name, _ in spslam_track.LOCAL_MAP_TABLES})
        o = dict(local_kfs=p(b["kfs"]), n_local_kfs=p(b["n_kfs"]), kf_max=p(b["kf_max"]), local_rows=p(b["lrows"]),
                 n_local=p(b["n_local"]), status=p(b["status"]), scratch=p(b["scratch"]), kf_cap=pk.nk, capacity=8,
                 scratch_stride=4, records=p(b["rec"]), local_frames=p(b["lfr"]))
        for k, v in over.items():
            (m if k in m else o)[k] = v
        return spslam_track.LocalMap(**m), spslam_track.LocalMapOut(**o)

    bad = [dict(n_kf=0), dict(n_kf=1025), dict(capacity=-1), dict(kf_cap=-1), dict(scratch_stride=-1),
           dict(kf_cap=pk.nk - 1)]
    bad += [{k: None} for k in ("kf_base", "row_base", "obs_off", "obs_kf", "covis", "child_off", "child", "parent",
                                "match_off", "match_row", "local_kfs", "n_local_kfs", "kf_max", "local_rows",
                                "n_local", "status", "scratch", "points", "kp_counts", "frame_rows")]
    for over in bad:
        m, o = structs(**over)
        with pytest.raises(spslam_gpu.SpslamError, match="update_local_map"):
            tg.update_local_map_device(1, None, m, o)
    with pytest.raises(spslam_gpu.SpslamError, match="update_local_map"):
        tg.update_local_map_device(0, None, *structs())
    rc = ex.lib.spslam_track_update_local_map_batch_device(ex.ctx, 1, None, None, None, None)
    assert rc != 0 and b"update_local_map" in ex.lib.spslam_last_error(ex.ctx)
    with pytest.raises(spslam_gpu.SpslamError, match="n_kf"):
        tg.update_local_map(dict(case["T"], parent=np.zeros(0, np.int32)), [0], [])
    import torch
    torch.cuda.synchronize()
    for k, v in before.items():  # nothing ran on the buffers
        assert np.array_equal(host(b[k], v.dtype).reshape(v.shape), v), k
    assert ctypes.sizeof(spslam_track.LocalMap) % 8 == 0
