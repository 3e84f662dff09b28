"""GPU parity of the two tracking matchers off the rendered pairs and at their seams: match_window_kernel /
match_assign_kernel (ORBmatcher::SearchByProjection frame to frame) and local_window_kernel / local_assign_kernel
(Tracking::SearchLocalPoints) on the case tables of tests/match_cases.py -- the forward / backward octave ranges, each
isInFrustum rejection and both PredictScale clamps, point and keypoint counts at the chunk, word and loader seams,
cells of up to 513 keypoints with forced re-scans, windows at the image border, the distance, stereo, ratio and
rotation-histogram seams, the retry pass, seen stamps, two further geometries (distortion; a second image size and
scale table) and the LDS limit of the walks.  tests/test_oracle_match_cases.py asserts on the CPU that every case
reaches what it was built for.  Every case runs through the single-frame host form (six keys per point) and as a slot
of a batch of at least 17 frames (three keys); both are held to the oracle.  Bar: match, nmatches and in_view
identical (index work: no tolerance)."""
import numpy as np
import pytest

import match_cases as MC

pytestmark = pytest.mark.gpu

SENTINEL, BYTE_SENTINEL = -9, 0xA5


@pytest.fixture(scope="module")
def gpu():
    """One context per geometry, with its frame stage configured."""
    import spslam_frame
    import spslam_gpu
    ctx = {}
    for geom, G in MC.GEOMS.items():
        ex = spslam_gpu.OrbExtractor(scale_factor=G["scale_factor"], nlevels=G["nlevels"], width=G["width"],
                                     height=G["height"], max_batch=1)
        fs = spslam_frame.FrameStage(ex, G["fx"], G["fy"], G["cx"], G["cy"], G["dist"], G["bf"], G["width"],
                                     G["height"])
        ctx[geom] = (ex, fs)
    yield ctx
    for ex, _ in ctx.values():
        ex.close()


_oracle_cache = {}


def oracle(case, max_points=None, with_taken=True):
    """The oracle on a case as a batch call with this max_points sees it (cached: the cases are shared)."""
    key = (case["name"], max_points, with_taken)
    if key not in _oracle_cache:
        n = len(case["P" if case["kind"] == "proj" else "LP"])
        cut = min(case.get("max_points", n), max_points if max_points is not None else n)
        _oracle_cache[key] = MC.oracle(dict(case, max_points=cut) if cut < n else case, with_taken=with_taken)
    return _oracle_cache[key]


def test_frame_stage_geometry(gpu):
    """The bounds and grid inverses the matchers read equal the oracle's bit for bit, for all three geometries."""
    groups = {"tum": MC.proj_group("border"), "barrel": MC.proj_group("second_geometry"),
              "small": MC.proj_group("second_geometry")}
    for geom, (_, fs) in gpu.items():
        geo = next(c for c in groups[geom] if c["geom"] == geom)["geo"]
        assert fs.bounds.tobytes() == geo[5:9].tobytes(), (geom, fs.bounds, geo[5:9])
        assert fs.grid_inv.tobytes() == geo[9:11].tobytes(), (geom, fs.grid_inv, geo[9:11])
    assert gpu["barrel"][1].bounds[0] < 0 and gpu["small"][1].grid_inv[0] == np.float32(64) / np.float32(480)


# ---------------------------------------------------------------------------------------------- the single-frame form
def _single(gpu, case):
    import spslam_match as M
    ex = gpu[case["geom"]][0]
    fr, P = MC.effective(case)
    cur = (case["kun"], case["desc"], case["ur"], case["go"], case["gi"])
    if case["kind"] == "proj":
        return M.Matcher(ex, case["params"])(fr, P, *cur)
    return M.LocalMatcher(ex, case["params"] + (0,))(fr, P, *cur, case["taken"])


def _assert_equal(got, want, what):
    assert got[1] == want[1], (what, got[1], want[1])
    assert np.array_equal(got[0], want[0]), (what, np.nonzero(got[0] != want[0])[0][:10])
    if len(got) > 2:
        assert np.array_equal(got[2], want[2]), (what, np.nonzero(got[2] != want[2])[0][:10])


@pytest.mark.parametrize("group", list(MC.PROJ_GROUPS))
def test_projection_single(gpu, group):
    for case in MC.proj_group(group):
        _assert_equal(_single(gpu, case), oracle(case)[:2], case["name"])


@pytest.mark.parametrize("group", [g for g in MC.LOCAL_GROUPS if g != "seen"])  # (the host form takes no stamps)
def test_local_points_single(gpu, group):
    for case in MC.local_group(group):
        _assert_equal(_single(gpu, case), oracle(case), case["name"])


# ------------------------------------------------------------------------------------------------ the batch-device form
def batch_cap(n_max):
    """A capacity above every count of the batch and no multiple of 32."""
    cap = n_max + 5
    return cap + 1 if cap % 32 == 0 else cap


def run_batch(gpu, cases, max_points=None, with_taken=True, cap=None, seen_table=None):
    """One batch-device call over `cases` (one geometry, one parameter set), every output pre-filled with a sentinel.
    Returns (rc error or None, match [F, cap], nmatches [F], in_view per frame or None, the call's max_points)."""
    import spslam_gpu as G
    import spslam_match as M
    import torch
    kind, geom, params = cases[0]["kind"], cases[0]["geom"], cases[0]["params"]
    assert all((c["kind"], c["geom"], c["params"]) == (kind, geom, params) for c in cases)
    ex = gpu[geom][0]
    fr_key, pts_key, fdt = ("fr", "P", M.PROJ_FRAME_DTYPE) if kind == "proj" else ("lfr", "LP", M.LOCAL_FRAME_DTYPE)
    F = len(cases)
    cap = cap or batch_cap(max(len(c["kun"]) for c in cases))
    frames = np.zeros(F, fdt)
    kun = np.zeros((F, cap), G.KEYPOINT_DTYPE)
    desc = np.zeros((F, cap, 32), np.uint8)
    ur = np.zeros((F, cap), np.float32)
    go = np.zeros((F, 64 * 48 + 1), np.int32)
    gi = np.zeros((F, cap), np.int32)
    tk = np.zeros((F, cap), np.uint8)
    counts = np.zeros(F, np.int32)
    pts, off = [], 0
    for f, c in enumerate(cases):
        n = len(c["kun"])
        frames[f] = c[fr_key]
        frames[f]["point_offset"] = off
        off += len(c[pts_key])
        pts.append(c[pts_key])
        kun[f, :n], desc[f, :n], ur[f, :n], go[f], counts[f] = c["kun"], c["desc"], c["ur"], c["go"], n
        gi[f, :len(c["gi"])] = c["gi"]
        if kind == "local" and c["taken"] is not None:
            tk[f, :n] = c["taken"]
    if max_points is None:
        max_points = max(len(p) for p in pts)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d = [dev(a) for a in (frames, np.concatenate(pts), kun, desc, ur, go, gi, counts, tk)]
    d_match = torch.full((F * cap,), SENTINEL, dtype=torch.int32, device="cuda")
    d_nm = torch.full((F,), SENTINEL, dtype=torch.int32, device="cuda")
    d_iv = torch.full((max(off, 1),), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
    d_seen = dev(seen_table) if seen_table is not None else None
    args = [F, d[0].data_ptr(), d[1].data_ptr(), max_points] + [d[i].data_ptr() for i in range(2, 8)] + [cap]
    err = None
    try:
        if kind == "proj":
            M.Matcher(ex, params).batch_device(*args, d_match.data_ptr(), d_nm.data_ptr())
        else:
            M.LocalMatcher(ex, params + (0,)).batch_device(
                *args, d[8].data_ptr() if with_taken else 0, d_match.data_ptr(), d_nm.data_ptr(), d_iv.data_ptr(),
                d_seen=d_seen.data_ptr() if d_seen is not None else 0)
    except G.SpslamError as e:
        err = e
    torch.cuda.synchronize()
    iv = None
    if kind == "local":
        iv = np.split(d_iv.cpu().numpy()[:off], np.cumsum([len(p) for p in pts])[:-1])
    return err, d_match.cpu().numpy().reshape(F, cap), d_nm.cpu().numpy(), iv, max_points


def assert_batch(cases, result, with_taken=True, label=""):
    """Every frame equals the oracle; every entry at or beyond counts[f] and every in_view byte at or beyond max_points
    is untouched, every one below is written."""
    err, match, nm, iv, max_points = result
    assert err is None, (label, err)
    for f, c in enumerate(cases):
        what = (label, f, c["name"])
        want = oracle(c, max_points, with_taken)
        n = len(c["kun"])
        assert (match[f, n:] == SENTINEL).all(), what
        assert (match[f, :n] >= -1).all(), what
        assert nm[f] == want[1], (what, nm[f], want[1])
        assert np.array_equal(match[f, :n], want[0]), (what, np.nonzero(match[f, :n] != want[0])[0][:10])
        if iv is not None:
            k = min(len(iv[f]), max_points)
            assert (iv[f][k:] == BYTE_SENTINEL).all() and (iv[f][:k] <= 1).all(), what
            assert np.array_equal(iv[f][:k].astype(bool), want[2]), what


def batches(cases, at_least=17):
    """The cases grouped by geometry and parameters, each group cycled up to `at_least` frames (the smallest batch
    that selects the three-key instantiations is 17)."""
    groups = {}
    for c in cases:
        if c.get("seen") is None and "max_points" not in c:
            groups.setdefault((c["geom"], c["params"]), []).append(c)
    return [[g[i % len(g)] for i in range(max(at_least, len(g)))] for _, g in sorted(groups.items())]


def test_projection_batches_of_17(gpu):
    for batch in batches(MC.proj_cases()):
        assert len(batch) >= 17
        assert_batch(batch, run_batch(gpu, batch), label=batch[0]["params"])


def test_local_points_batches_of_17(gpu):
    for with_taken in (True, False):   # (absent: the d_taken argument is NULL and every frame starts free)
        for batch in batches(MC.local_cases()):
            assert len(batch) >= 17
            assert_batch(batch, run_batch(gpu, batch, with_taken=with_taken), with_taken, label=batch[0]["params"])


def test_small_batches_with_different_counts(gpu):
    """Ten frames of 2 .. 513 keypoints in one call (six keys): rows beyond each count stay untouched."""
    proj = MC.proj_group("keypoint_counts")
    assert sorted(len(c["kun"]) for c in proj) == sorted(MC.KP_COUNTS)
    assert_batch(proj, run_batch(gpu, proj), label="proj")
    for variant in ("no_taken", "taken_seams", "taken_all"):
        local = [c for c in MC.local_group("counts") if c["name"].startswith("local_keypoints")
                 and c["name"].endswith(variant)]
        assert len(local) == len(MC.KP_COUNTS)
        assert_batch(local, run_batch(gpu, local), label=variant)


def test_max_points_cuts_the_lists(gpu):
    """max_points below n_points: the expectation is the oracle on the first max_points points of each frame."""
    for cases in ([c for c in MC.proj_group("point_counts") if "max_points" not in c],
                  [c for c in MC.local_group("counts") if c["name"].startswith("local_points")
                   and "max_points" not in c]):
        assert max(len(c["P" if c["kind"] == "proj" else "LP"]) for c in cases) == 129
        for batch in (cases, [cases[i % len(cases)] for i in range(18)]):
            assert_batch(batch, run_batch(gpu, batch, max_points=100), label=("max_points", len(batch)))


def test_seen_stamps(gpu):
    """Two frames read one stamp table through different offsets; the referee is the oracle on the lists with the
    stamped points mirrored behind the camera."""
    a, b = MC.local_group("seen")
    assert not np.array_equal(a["seen"], b["seen"]) and a["seen_table"] is b["seen_table"]
    plain = dict(a, name="seen_none", seen=None)   # a frame whose stamp no entry of the table holds
    plain["lfr"] = a["lfr"].copy()
    plain["lfr"]["stamp"] = 99
    for batch in ([a, b, plain], [(a, b, plain)[i % 3] for i in range(18)]):
        assert_batch(batch, run_batch(gpu, batch, seen_table=a["seen_table"]), label=("seen", len(batch)))


# ------------------------------------------------------------------------------------------------------- the LDS limit
def test_lds_limit(gpu):
    """The walks keep the taken bits and the claim table of `cap` keypoints in dynamic LDS.  At the largest cap that
    fits, a frame of 513 keypoints gives the oracle's result; one above it the call reports an error and leaves every
    output as it was."""
    proj = next(c for c in MC.proj_group("keypoint_counts") if len(c["kun"]) == 513)
    local = next(c for c in MC.local_group("counts") if c["name"] == "local_keypoints_513_taken_seams")
    for case, limit in ((proj, MC.PROJ_CAP_LIMIT), (local, MC.LOCAL_CAP_LIMIT)):
        assert_batch([case], run_batch(gpu, [case], cap=limit), label=("cap", limit))
        err, match, nm, iv, _ = run_batch(gpu, [case], cap=limit + 1)
        assert err is not None, (case["kind"], limit + 1)
        assert (match == SENTINEL).all() and (nm == SENTINEL).all(), case["kind"]
        assert iv is None or (iv[0] == BYTE_SENTINEL).all()
        # the context still serves the next call
        assert_batch([case], run_batch(gpu, [case]), label=("after the refusal", case["kind"]))
