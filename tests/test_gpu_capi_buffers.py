"""The C API's grow-on-demand and re-configure buffer paths (csrc/capi_ctx.h DevBuf / Stage): a context that has
grown a buffer, or been configured again, computes bit for bit what it computed before and what a fresh context
computes.  One context per stage; every comparison is byte identity.  Each context is destroyed at the end of its
test (close() raises nothing: the ownership of every device buffer is the context's)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = __import__("pathlib").Path(__file__).resolve().parents[1]


def _ctx(**kw):
    import spslam_gpu
    return spslam_gpu.OrbExtractor(max_batch=kw.pop("max_batch", 1), **kw)


def _bytes(x):
    """A result (array, scalar, or a tuple / dict / list of them) as one comparable tuple of byte strings."""
    if isinstance(x, dict):
        return tuple((k, _bytes(x[k])) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return tuple(_bytes(v) for v in x)
    return np.ascontiguousarray(x).tobytes()


def _grow_then_reuse(make, run, small, large):
    """small, large, small on one context: first == third, second == a fresh context's; both contexts close."""
    ex = make()
    try:
        first, second, third = run(ex, small), run(ex, large), run(ex, small)
    finally:
        ex.close()
    fresh = make()
    try:
        ref = run(fresh, large)
    finally:
        fresh.close()
    assert _bytes(first) == _bytes(third), "small input differs after the buffer grew"
    assert _bytes(second) == _bytes(ref), "large input differs from a fresh context's result"
    return first, second


@pytest.fixture(scope="module")
def pair():
    """One (last, current) frame pair with the oracle's ORB and frame-stage outputs."""
    from test_oracle_match import make_pairs
    return make_pairs(((0, 10, 12),), seed=17)[0]


def _first_keypoints(q, n):
    """The pair restricted to the current frame's first n keypoints (grid CSR rebuilt)."""
    go, gi = q["go"], q["gi"][:q["go"][-1]]
    cell = np.repeat(np.arange(len(go) - 1), np.diff(go))
    keep = gi < n
    off = np.concatenate([[0], np.cumsum(np.bincount(cell[keep], minlength=len(go) - 1))]).astype(np.int32)
    return dict(q, kun=q["kun"][:n], desc=q["desc"][:n], ur=q["ur"][:n], go=off, gi=gi[keep].astype(np.int32))


def _match_ctx():
    import spslam_frame
    import synth
    K = synth.TUM3
    ex = _ctx()
    spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], (0,) * 5, K["bf"], 640, 480)
    return ex


def test_pose_optimize_grow_then_reuse():
    import oracle_ctypes
    import spslam_gpu
    import synth
    sc = synth.Scene(0)
    orb = oracle_ctypes.OrbOracle()
    g, d, fid = sc.render(sc.pose(0), noise_seed=0)
    kps, _ = orb.extract(g)
    prob, pts, pls, _ = synth.pose_problem(sc, 0, kps, d, fid, orb.scale_tables()[3], np.random.default_rng(100))
    assert len(pts) >= 200

    def cut(n):
        p = prob.copy()
        p["n_points"] = n
        return p, pts[:n], pls

    def run(ex, P):
        return spslam_gpu.pose_optimize(ex, *P)

    small, large = _grow_then_reuse(_ctx, run, cut(8), cut(200))
    assert int(large[0]["n_inliers"]) > 100  # the 200-point problem is a real optimisation


def test_search_by_projection_grow_then_reuse(pair):
    import spslam_match
    n = len(pair["kun"])
    assert n > 900
    full, few, none = pair, _first_keypoints(pair, 40), _first_keypoints(pair, 0)

    def run(ex, qs):
        m = spslam_match.Matcher(ex)
        return [m(q["fr"], q["P"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"]) for q in qs]

    # the n = 0 call reserves one-keypoint slots
    ((m40, n40), (m0, n0)), ((mf, nf),) = _grow_then_reuse(_match_ctx, run, (few, none), (full,))
    assert len(m40) == 40 and len(m0) == 0 and n0 == 0 and len(mf) == n and nf > 0.5 * len(pair["P"])


def test_search_by_projection_batch_device_grows_on_caller_stream(pair):
    """1 frame, then 4 frames, on a non-default stream of one context: the window scratch grows between the two
    calls (after a wait for that stream) and every frame equals the single-frame result."""
    import torch
    import spslam_gpu as G
    import spslam_match as M
    few = _first_keypoints(pair, 40)
    ex = _match_ctx()
    try:
        m = M.Matcher(ex)
        cap = len(pair["kun"])
        single = {id(q): m(q["fr"], q["P"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"]) for q in (pair, few)}
        stream = torch.cuda.Stream()
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa
        for qs in ([pair], [pair, few, few, pair]):
            F = len(qs)
            frames = np.zeros(F, M.PROJ_FRAME_DTYPE)
            kun = np.zeros((F, cap), G.KEYPOINT_DTYPE)
            desc = np.zeros((F, cap, 32), np.uint8)
            ur = np.zeros((F, cap), np.float32)
            go = np.zeros((F, 64 * 48 + 1), np.int32)
            gi = np.zeros((F, cap), np.int32)
            counts = np.zeros(F, np.int32)
            for f, q in enumerate(qs):
                k = len(q["kun"])
                frames[f] = q["fr"]
                frames[f]["point_offset"] = f * len(q["P"])
                kun[f, :k], desc[f, :k], ur[f, :k], go[f], counts[f] = q["kun"], q["desc"], q["ur"], q["go"], k
                gi[f, :len(q["gi"])] = q["gi"]
            d = [dev(a) for a in (frames, np.concatenate([q["P"] for q in qs]), kun, desc, ur, go, gi, counts)]
            d_match = torch.full((F * cap,), -9, dtype=torch.int32, device="cuda")
            d_nm = torch.zeros(F, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                m.batch_device(F, d[0].data_ptr(), d[1].data_ptr(), len(pair["P"]), d[2].data_ptr(), d[3].data_ptr(),
                               d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), cap,
                               d_match.data_ptr(), d_nm.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            mb, nb = d_match.cpu().numpy().reshape(F, cap), d_nm.cpu().numpy()
            for f, q in enumerate(qs):
                ms, ns = single[id(q)]
                assert nb[f] == ns and mb[f, :len(ms)].tobytes() == ms.tobytes(), (F, f)
    finally:
        ex.close()


# ---------------------------------------------------------------------------
# The three window searches' host forms stage the current frame through one helper (csrc/capi_ctx.h CurrentFrame):
# its empty and one-entry ends, per host form, against that form's referee.

def _edge_cuts(q, frame_key, points_key, k):
    """q with no points; with no keypoints and an all-zero grid_off; with keypoint k alone (the points kept)."""
    fr0 = q[frame_key].copy()
    fr0["n_points"] = 0
    none = _first_keypoints(q, 0)
    cell = np.repeat(np.arange(len(q["go"]) - 1), np.diff(q["go"]))[list(q["gi"][:q["go"][-1]]).index(k)]
    one = dict(q, kun=q["kun"][k:k + 1], desc=q["desc"][k:k + 1], ur=q["ur"][k:k + 1],
               go=(np.arange(len(q["go"])) > cell).astype(np.int32), gi=np.zeros(1, np.int32))
    assert not none["go"].any() and len(none["gi"]) == 0
    return (("no points", dict(q, **{frame_key: fr0, points_key: q[points_key][:0]})), ("no keypoints", none),
            ("one keypoint", one))


@pytest.fixture(scope="module")
def local_pair(pair):
    from test_oracle_match import local_problems
    return local_problems([pair], seed=23)[0]


def _matched_keypoint(match):
    """A keypoint the whole problem matches: the one-keypoint cut keeps it, so that cut has something to find."""
    return int(np.flatnonzero(match >= 0)[0])


def _local_matched_keypoint(q):
    import oracle_match as OM
    return _matched_keypoint(OM.search_local_points(q["lfr"], q["LP"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"],
                                                    q["geo"], taken=None)[0])


def test_search_by_projection_host_form_at_its_empty_ends(pair):
    import oracle_match as OM
    import spslam_match
    ex = _match_ctx()
    try:
        m = spslam_match.Matcher(ex)
        q = pair
        k = _matched_keypoint(OM.search_by_projection(q["fr"], q["P"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"],
                                                      q["geo"])[0])
        for name, q in _edge_cuts(pair, "fr", "P", k):
            mo, nmo, _ = OM.search_by_projection(q["fr"], q["P"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"],
                                                 q["geo"])
            mg, nmg = m(q["fr"], q["P"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"])
            assert nmg == nmo and len(mg) == len(q["kun"]) and np.array_equal(mg, mo), name
    finally:
        ex.close()


def test_search_local_points_host_form_at_its_empty_ends(local_pair):
    import oracle_match as OM
    import spslam_match
    ex = _match_ctx()
    try:
        lm = spslam_match.LocalMatcher(ex)
        for name, q in _edge_cuts(local_pair, "lfr", "LP", _local_matched_keypoint(local_pair)):  # taken absent
            mo, nmo, ivo = OM.search_local_points(q["lfr"], q["LP"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"],
                                                  q["geo"], taken=None)
            mg, nmg, ivg = lm(q["lfr"], q["LP"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"], None)
            assert nmg == nmo and len(mg) == len(q["kun"]) and np.array_equal(mg, mo), name
            assert len(ivg) == len(q["LP"]) and np.array_equal(ivg, ivo), name
    finally:
        ex.close()


def test_fuse_search_host_form_at_its_empty_ends(local_pair):
    import fuse_ref as FR
    import spslam_match
    ex = _match_ctx()
    try:
        fs = spslam_match.FuseSearch(ex)
        for name, q in _edge_cuts(local_pair, "lfr", "LP", _local_matched_keypoint(local_pair)):  # skip absent
            want, want_nf = FR.snapshot_search(q["lfr"]["Tcw"], q["LP"], q["kun"], q["desc"], q["ur"], q["go"],
                                               q["gi"], q["geo"])
            res, nf = fs(q["lfr"]["Tcw"], q["LP"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"])
            assert len(res) == len(q["LP"]) and res.tobytes() == want.astype(res.dtype).tobytes(), name
            assert nf == want_nf, name
    finally:
        ex.close()


def test_bow_transform_grow_then_reuse():
    import bow_common as BC
    import spslam_bow
    text = BC.vocab_text()
    desc = np.random.default_rng(5).integers(0, 256, (500, 32), dtype=np.uint8)

    def make():
        ex = _ctx()
        ex.vocabulary = spslam_bow.Vocabulary(ex, text)
        return ex

    def run(ex, descs):
        return [ex.vocabulary.transform(dsc) for dsc in descs]

    # n = 0 reserves one-feature slots
    (one, none), (many,) = _grow_then_reuse(make, run, (desc[:1], desc[:0]), (desc,))
    assert len(one["words"]) <= 1 and len(none["words"]) == 0 and len(many["words"]) > 100


def _lba_window(ref, n_points):
    """The fixture's window cut down to its first n_points points and their observations, planes dropped."""
    pts = ref["points"][:n_points].copy()
    obs = np.concatenate([ref["point_obs"][p["obs_offset"]:p["obs_offset"] + p["n_obs"]] for p in pts])
    pts["obs_offset"] = np.concatenate([[0], np.cumsum(pts["n_obs"])[:-1]])
    prob = ref["prob"].copy()
    prob["n_points"], prob["n_point_obs"], prob["n_planes"], prob["n_plane_obs"] = len(pts), len(obs), 0, 0
    return prob, ref["kfs"], pts, obs, ref["planes"][:0], ref["plane_obs"][:0]


def test_lba_optimize_grow_then_reuse():
    """tests/golden/lba_seq1.npz holds one window (8 keyframes, 400 points): the small input is that window with
    its first 60 points only, the large one the whole window."""
    import spslam_lba
    ref = np.load(ROOT / "tests" / "golden" / "lba_seq1.npz")
    whole = tuple(ref[k] for k in ("prob", "kfs", "points", "point_obs", "planes", "plane_obs"))

    def run(ex, P):
        g = spslam_lba.LocalBA(ex)(*P)
        r = g.pop("result")  # the record also carries phase timings
        assert int(r["status"]) == 0
        return dict(g, iterations=r["iterations"], trials=r["trials"], stopped=r["stopped"],
                    outliers=(r["n_point_outliers"], r["n_plane_outliers"]))

    _, large = _grow_then_reuse(_ctx, run, _lba_window(ref, 60), whole)
    assert large["Tcw"].tobytes() == ref["Tcw"].tobytes() and large["points"].tobytes() == ref["pts_out"].tobytes()


def test_planes_associate_grow_then_reuse():
    import spslam_assoc
    import synth
    from test_gpu_assoc import _map
    m, b = _map(np.random.default_rng(2), synth.Scene(0, n_boxes=0))
    assert len(m) >= 3
    T = np.eye(4, dtype=np.float32)
    c = np.array([[0, 1, 0, 1.3], [1, 0, 0, 2.5], [0, 0, 1, 0.1]], np.float32)

    def run(ex, args):
        pa = spslam_assoc.PlaneAssociator(ex)
        return [pa(T, *a) for a in args]

    # n_map = 0 and n_planes = 0 (one-plane slots), then a few map planes
    (no_map, no_planes), (some,) = _grow_then_reuse(_ctx, run, ((c, m[:0], b[:0]), (c[:0], m, b)), ((c, m, b),))
    assert len(no_map["match"]) == len(c) and len(no_planes["match"]) == 0 and len(some["match"]) == len(c)


def test_planes_reconfigure():
    """333x77 / cloud_dis 4, then 640x480 / cloud_dis 3, then 333x77 again on one context: every buffer of the
    plane and supposed-plane stages is reallocated twice."""
    import oracle_planes
    import spslam_planes
    import synth
    K = synth.TUM3
    full = []
    for seq, fi in ((3, 20), (5, 7)):  # box scenes of the supposed-plane tests
        sc = synth.Scene(seq, n_boxes=8)
        full.append(oracle_planes.depth_to_float(sc.render(sc.pose(fi), noise_seed=fi)[1]))
    # the small frames are 333x77 windows of the same depth images
    depth = {640: full, 333: [np.ascontiguousarray(d[y:y + 77, 150:483]) for d in full for y in (120, 300)]}

    def run(ex, w, h, cloud_dis):
        pe = spslam_planes.PlaneExtractor(ex, K["fx"], K["fy"], K["cx"], K["cy"], w, h, cloud_dis=cloud_dis,
                                          min_size=30 if w < 640 else 500)
        out = []
        for d in depth[w]:
            planes = pe(d)
            # the organized cloud, normals and plane distances too: the reference finds no plane in the 20-row
            # cloud of a 333x77 frame (not even in a flat wall), so there the stage buffers are all there is to see
            out.append((planes, pe.generate_from_boundaries(d), [pe.debug(0, what) for what in (0, 1, 2)]))
        return out

    ex = _ctx()
    try:
        first, second, third = run(ex, 333, 77, 4), run(ex, 640, 480, 3), run(ex, 333, 77, 4)
    finally:
        ex.close()
    fresh = _ctx()
    try:
        ref = run(fresh, 640, 480, 3)
    finally:
        fresh.close()
    counts = [[(len(p["coef"]), len(s["coef"])) for p, s, _ in r] for r in (first, second)]
    assert _bytes(first) == _bytes(third)
    assert _bytes(second) == _bytes(ref)
    # the inputs are not degenerate: a measured cloud at the small size, planes and supposed planes at the large
    assert all(np.isfinite(dbg[0]).any() and dbg[0].shape == (84 * 20, 3) for _, _, dbg in first)
    assert sum(n for n, _ in counts[1]) >= 2 and sum(m for _, m in counts[1]) >= 1, counts
