"""GPU parity: ORBmatcher::SearchByProjection (frame to frame, with
GetFeaturesInArea, DescriptorDistance, the rotation check and
TrackWithMotionModel's retry; src/ORBmatcher.cc:1328-1470, src/Frame.cc:427-480,
src/Tracking.cc:968-975) on gfx950 vs the CPU oracle.  Bar: identical
mvpMapPoints assignment and nmatches (index work: bit-exact)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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
def pairs():
    from test_oracle_match import make_pairs
    return make_pairs(((0, 10, 12), (1, 30, 31), (2, 50, 53), (3, 5, 9), (4, 70, 71), (5, 0, 2)), seed=17)


def test_single_pairs_match_oracle(gpu, pairs):
    import oracle_match as OM
    ex, M = gpu
    for params in ((15.0, 0, 1, 20), (15.0, 0, 0, 0), (7.0, 0, 1, 0), (15.0, 1, 1, 20), (4.0, 0, 1, 400)):
        m = M.Matcher(ex, params)
        for k, q in enumerate(pairs):
            mo, nmo, _ = OM.search_by_projection(q["fr"], q["P"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"],
                                                 q["geo"], params=params)
            mg, nmg = m(q["fr"], q["P"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"])
            assert nmg == nmo, (params, k, nmg, nmo)
            assert np.array_equal(mg, mo), (params, k, np.nonzero(mg != mo)[0][:10])


def test_edge_cases(gpu, pairs):
    import oracle_match as OM
    ex, M = gpu
    m = M.Matcher(ex)
    q = pairs[0]
    cases = [q["P"][:0], q["P"][:1], q["P"]]
    behind = q["P"].copy()
    behind["xw"] = -behind["xw"] * 50  # far behind / outside the image
    cases.append(behind)
    zero_obs = q["P"].copy()
    zero_obs["n_obs"] = 0  # nothing blocks: later points may take the same keypoint
    cases.append(zero_obs)
    for P in cases:
        fr = q["fr"].copy()
        fr["n_points"] = len(P)
        mo, nmo, _ = OM.search_by_projection(fr, P, q["kun"], q["desc"], q["ur"], q["go"], q["gi"], q["geo"])
        mg, nmg = m(fr, P, q["kun"], q["desc"], q["ur"], q["go"], q["gi"])
        assert nmg == nmo and np.array_equal(mg, mo), len(P)


def _pack(problems, fr_key, pts_key, frame_dtype):
    """The problems' arrays as the batch entry points read them (one row per frame, padded to the largest keypoint
    count): the device buffers [frames, points, kun, desc, uright, grid_off, grid_idx, counts, taken], cap,
    max_points and the total number of points."""
    import torch
    import spslam_gpu as G
    F, cap = len(problems), max(len(q["kun"]) for q in problems)
    frames = np.zeros(F, frame_dtype)
    kun = np.zeros((F, cap), G.KEYPOINT_DTYPE)
    desc = np.zeros((F, cap, 32), np.uint8)
    ur = np.zeros((F, cap), np.float32)
    go = np.zeros((F, 64 * 48 + 1), np.int32)
    gi = np.zeros((F, cap), np.int32)
    tk = np.zeros((F, cap), np.uint8)
    counts = np.zeros(F, np.int32)
    pts, off = [], 0
    for f, q in enumerate(problems):
        n = len(q["kun"])
        frames[f] = q[fr_key]
        frames[f]["point_offset"] = off
        off += len(q[pts_key])
        pts.append(q[pts_key])
        kun[f, :n], desc[f, :n], ur[f, :n], go[f] = q["kun"], q["desc"], q["ur"], q["go"]
        gi[f, :len(q["gi"])] = q["gi"]
        if "taken" in q:
            tk[f, :n] = q["taken"]
        counts[f] = n
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa
    d = [dev(a) for a in (frames, np.concatenate(pts), kun, desc, ur, go, gi, counts, tk)]
    return d, cap, max(len(p) for p in pts), off


def _match_batch(m, M, problems):
    """Matcher.batch_device over `problems`: match [F, cap] and nmatches [F]."""
    import torch
    d, cap, max_points, _ = _pack(problems, "fr", "P", M.PROJ_FRAME_DTYPE)
    F = len(problems)
    d_match = torch.full((F * cap,), -9, dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(F, dtype=torch.int32, device="cuda")
    m.batch_device(F, d[0].data_ptr(), d[1].data_ptr(), max_points, d[2].data_ptr(), d[3].data_ptr(),
                   d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), cap, d_match.data_ptr(),
                   d_nm.data_ptr())
    torch.cuda.synchronize()
    return d_match.cpu().numpy().reshape(F, cap), d_nm.cpu().numpy()


def test_batch_device_matches_single(gpu, pairs):
    ex, M = gpu
    m = M.Matcher(ex)
    mb, nb = _match_batch(m, M, pairs)
    for f, q in enumerate(pairs):
        ms, ns = m(q["fr"], q["P"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"])
        assert nb[f] == ns and np.array_equal(mb[f, :len(q["kun"])], ms), f


@pytest.fixture(scope="module")
def local_pairs(pairs):
    from test_oracle_match import local_problems
    return local_problems(pairs, seed=23)


def test_local_points_match_oracle(gpu, local_pairs):
    import oracle_match as OM
    ex, M = gpu
    for params in ((3.0, 0.8, 0.5, 0), (5.0, 0.8, 0.5, 0), (1.0, 0.6, 0.5, 0), (3.0, 0.95, 0.9, 0)):
        lm = M.LocalMatcher(ex, params)
        for k, q in enumerate(local_pairs):
            for taken in (q["taken"], None):
                mo, nmo, ivo = OM.search_local_points(q["lfr"], q["LP"], q["kun"], q["desc"], q["ur"], q["go"],
                                                      q["gi"], q["geo"], taken=taken, params=params[:3])
                mg, nmg, ivg = lm(q["lfr"], q["LP"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"], taken)
                assert np.array_equal(ivg, ivo), (params, k)
                assert nmg == nmo, (params, k, nmg, nmo)
                assert np.array_equal(mg, mo), (params, k, np.nonzero(mg != mo)[0][:10])


def _local_batch(lm, M, problems, with_taken=True):
    """LocalMatcher.batch_device over `problems`: match [F, cap], nmatches [F] and in_view per frame."""
    import torch
    d, cap, max_points, n_pts = _pack(problems, "lfr", "LP", M.LOCAL_FRAME_DTYPE)
    F = len(problems)
    d_match = torch.full((F * cap,), -9, dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(F, dtype=torch.int32, device="cuda")
    d_iv = torch.zeros(n_pts, dtype=torch.uint8, device="cuda")
    lm.batch_device(F, d[0].data_ptr(), d[1].data_ptr(), max_points, d[2].data_ptr(), d[3].data_ptr(),
                    d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), cap,
                    d[8].data_ptr() if with_taken else 0, d_match.data_ptr(), d_nm.data_ptr(), d_iv.data_ptr())
    torch.cuda.synchronize()
    iv = np.split(d_iv.cpu().numpy().astype(bool), np.cumsum([len(q["LP"]) for q in problems])[:-1])
    return d_match.cpu().numpy().reshape(F, cap), d_nm.cpu().numpy(), iv


def test_local_points_batch_matches_single(gpu, local_pairs):
    ex, M = gpu
    lm = M.LocalMatcher(ex)
    mb, nb, ivb = _local_batch(lm, M, local_pairs)
    for f, q in enumerate(local_pairs):
        ms, ns, ivs = lm(q["lfr"], q["LP"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"], q["taken"])
        assert nb[f] == ns and np.array_equal(mb[f, :len(q["kun"])], ms), f
        assert np.array_equal(ivb[f], ivs), f


# ---------------------------------------------------------------------------
# The window re-scan (the branch a point takes when earlier points took its kept keys) and the 3-key
# instantiations that batches of more than 16 frames select.

COPIES = 8
CROWDED_PROJ = ((30.0, 0, 0, 0), (15.0, 0, 0, 700), (30.0, 0, 1, 0))  # plain; two passes (retry at 2 th); rotation check
CROWDED_LOCAL = (8.0, 0.8, 0.5, 0)


@pytest.fixture(scope="module")
def crowded(local_pairs):
    """local_pairs[0] with its first 96 last-frame points and first 96 local points 8 times in a row each, and every
    descriptor zero.  With equal descriptors the keys order by CSR position, so every copy of a point takes the next
    free keypoint of the same window: the copies use up the kept keys by construction."""
    q = dict(local_pairs[0])
    q["desc"] = np.zeros_like(q["desc"])
    for fr_key, pts_key in (("fr", "P"), ("lfr", "LP")):
        P = q[pts_key][:96].copy()
        P["desc"] = 0
        q[pts_key] = np.repeat(P, COPIES)
        q[fr_key] = q[fr_key].copy()
        q[fr_key]["n_points"] = len(q[pts_key])
    return q


def _proj_oracle(q, params):
    import oracle_match as OM
    m, nm, _ = OM.search_by_projection(q["fr"], q["P"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"], q["geo"],
                                       params=params)
    return m, nm


def _local_oracle(q, with_taken):
    import oracle_match as OM
    return OM.search_local_points(q["lfr"], q["LP"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"], q["geo"],
                                  taken=q["taken"] if with_taken else None, params=CROWDED_LOCAL[:3])


def _copies_matched(m):
    """Matched copies per original point of the crowded problem (a keypoint holds one point, so they are matched to
    distinct keypoints)."""
    return np.bincount(m[m >= 0] // COPIES)


@pytest.fixture(scope="module")
def crowded_oracle(crowded):
    """The oracle's results on the crowded problem, after asserting on them that the inputs force the re-scan for
    K = 6 and K = 3.  Frame to frame: a point with K + 1 matched copies found all K kept keys taken at the K + 1-th.
    Local search (best and second best among the free keys): a point with K matched copies."""
    proj = {params: _proj_oracle(crowded, params) for params in CROWDED_PROJ}
    local = {with_taken: _local_oracle(crowded, with_taken) for with_taken in (False, True)}
    for K in (6, 3):
        for params in CROWDED_PROJ[:2]:  # (the rotation check takes matches away after the same walk as the first)
            assert (_copies_matched(proj[params][0]) >= K + 1).any(), (K, params)
        for with_taken in (False, True):
            assert (_copies_matched(local[with_taken][0]) >= K).any(), (K, with_taken)
    return proj, local


def test_crowded_single_rescans_match_oracle(gpu, crowded, crowded_oracle):
    """n_frames = 1: the 6-key instantiations on inputs that reach the window re-scan."""
    ex, M = gpu
    q = crowded
    proj, local = crowded_oracle
    for params in CROWDED_PROJ:
        mg, nmg = M.Matcher(ex, params)(q["fr"], q["P"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"])
        mo, nmo = proj[params]
        assert nmg == nmo, (params, nmg, nmo)
        assert np.array_equal(mg, mo), (params, np.nonzero(mg != mo)[0][:10])
    lm = M.LocalMatcher(ex, CROWDED_LOCAL)
    for with_taken in (False, True):
        mg, nmg, ivg = lm(q["lfr"], q["LP"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"],
                          q["taken"] if with_taken else None)
        mo, nmo, ivo = local[with_taken]
        assert np.array_equal(ivg, ivo), with_taken
        assert nmg == nmo, (with_taken, nmg, nmo)
        assert np.array_equal(mg, mo), (with_taken, np.nonzero(mg != mo)[0][:10])


def _batch17(crowded, problems):
    """17 frames, the smallest batch that selects the 3-key instantiations (n_frames > kSmallBatchKeys = 16): the
    crowded problem in slots 0 and 16, the six fixture problems cycled between them."""
    return [crowded] + [problems[i % len(problems)] for i in range(1, 16)] + [crowded]


def test_batch17_matches_oracle(gpu, pairs, crowded, crowded_oracle):
    """Every frame against the oracle (the single call runs the other K)."""
    ex, M = gpu
    batch = _batch17(crowded, pairs)
    for params in CROWDED_PROJ:
        want = {id(crowded): crowded_oracle[0][params], **{id(q): _proj_oracle(q, params) for q in pairs}}
        mb, nb = _match_batch(M.Matcher(ex, params), M, batch)
        for f, q in enumerate(batch):
            mo, nmo = want[id(q)]
            assert nb[f] == nmo, (params, f, nb[f], nmo)
            assert np.array_equal(mb[f, :len(q["kun"])], mo), (params, f)


def test_local_batch17_matches_oracle(gpu, local_pairs, crowded, crowded_oracle):
    ex, M = gpu
    batch = _batch17(crowded, local_pairs)
    lm = M.LocalMatcher(ex, CROWDED_LOCAL)
    for with_taken in (False, True):
        want = {id(crowded): crowded_oracle[1][with_taken],
                **{id(q): _local_oracle(q, with_taken) for q in local_pairs}}
        mb, nb, ivb = _local_batch(lm, M, batch, with_taken)
        for f, q in enumerate(batch):
            mo, nmo, ivo = want[id(q)]
            assert np.array_equal(ivb[f], ivo), (with_taken, f)
            assert nb[f] == nmo, (with_taken, f, nb[f], nmo)
            assert np.array_equal(mb[f, :len(q["kun"])], mo), (with_taken, f)
