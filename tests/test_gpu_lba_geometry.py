"""GPU parity: LocalBundleAdjustment on sparse windows and at its structure seams, bit for bit against the CPU oracle.

The cases are tests/lba_cases.py's (tests/test_oracle_lba_cases.py shows on the CPU which branch of structure() and of
the factor dispatch each takes): banded windows with and without a hub pose, two components, every scalar dense without
every pose coupled, at each free-pose seam of the factor dispatch on the narrow and on the wide instance, the AMD
workspace in LDS and in global memory; keyframe ids out of list order, fixed keyframes between free ones, keyframe id 0,
a free keyframe that sees nothing, no free pose at all, planes only, one point, one plane; second passes that lose a
coupling landmark's edge, a pose's every edge, or every edge; and the chunk seams of the scans (kT landmarks and edges,
lbg_pad32(E), 64 landmarks and kSchurBlk blocks per Schur chunk, two tiles of the id ranking).

Every case runs through the host form and again as a slot of two batch_device calls (one of windows of at most 64
keyframes, one that mixes them with larger windows so the small ones run on the wide instance) whose outputs are
pre-filled with a sentinel and whose rows are separated by guard rows.  The team split runs in process with 1 .. 8
workgroups and in a fresh child process with SPSLAM_LBG_ROWS_MAX_TEAM lowered (the library reads it once), so both
Schur layouts meet sparse block lists.  The fast order is held to its 1e-4 relative bar at 13 and 14 free poses."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import lba_cases as C

pytestmark = pytest.mark.gpu
FAST = [n for n in C.NAMES if n not in C.SLOW]
GUARD, SENTINEL = 3, 0xA5
TEAM_CASES = ("free11-band(2)", "free43-band(3)+hub", "wide66-free16-band(2)", "wide86-band(3)+hub")
TEAMS = (1, 2, 3, 5, 8)


@pytest.fixture(scope="module")
def lba():
    import spslam_gpu
    import spslam_lba
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    yield spslam_lba.LocalBA(ex)
    ex.close()


@pytest.fixture(scope="module")
def singles(lba):
    """Every case's host-form result, computed once on first use (the batches are compared with it)."""
    class Singles(dict):
        def __missing__(self, name):
            self[name] = lba(*C.case(name)["P"][:6])
            return self[name]
    return Singles()


def _identical(g, o, tag):
    import test_gpu_lba
    test_gpu_lba._assert_identical(g, o, tag)
    for k in ("n_point_outliers", "n_plane_outliers"):
        assert g["result"][k] == o["result"][k], (tag, k)


@pytest.mark.parametrize("name", FAST)
def test_case_matches_oracle(singles, name):
    _identical(singles[name], C.oracle(name), name)


def _batch(lba, names):
    """One batch_device call over the named cases.  Every problem's rows in every input and output array are
    preceded by GUARD rows that belong to no problem; the outputs are pre-filled with SENTINEL bytes."""
    import torch
    import spslam_lba as L
    dts = (L.LBA_KEYFRAME_DTYPE, L.LBA_POINT_DTYPE, L.LBA_POINT_OBS_DTYPE, L.LBA_PLANE_DTYPE, L.LBA_PLANE_OBS_DTYPE)
    hdr = np.zeros(len(names), L.LBA_PROBLEM_DTYPE)
    rows = [[] for _ in dts]
    cnt = [0] * 5
    where = []
    for i, name in enumerate(names):
        prob, kfs, pts, pobs, pls, plobs, _ = C.case(name)["P"]
        for j, dt in enumerate(dts):
            rows[j].append(np.zeros(GUARD, dt))
            cnt[j] += GUARD
        hdr[i] = prob
        hdr[i]["kf_offset"], hdr[i]["point_offset"], hdr[i]["plane_offset"] = cnt[0], cnt[1], cnt[3]
        pts, pls = pts.copy(), pls.copy()
        pts["obs_offset"] += cnt[2]
        pls["obs_offset"] += cnt[4]
        where.append(tuple(cnt))
        for j, a in enumerate((kfs, pts, pobs, pls, plobs)):
            rows[j].append(a)
            cnt[j] += len(a)
    for j, dt in enumerate(dts):
        rows[j].append(np.zeros(GUARD, dt))
        cnt[j] += GUARD
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()  # noqa: E731
    d_in = [dev(hdr)] + [dev(np.concatenate(r)) for r in rows]
    widths = (64, 12, 1, 16, 1)  # bytes per keyframe, point, point observation, plane, plane observation
    d_out = [torch.full((cnt[j] * w,), SENTINEL, dtype=torch.uint8, device="cuda") for j, w in enumerate(widths)]
    rsz = L.LBA_RESULT_DTYPE.itemsize
    d_res = torch.full(((len(names) + GUARD) * rsz,), SENTINEL, dtype=torch.uint8, device="cuda")
    lba.batch_device(len(names), hdr, *[x.data_ptr() for x in d_in], d_out[0].data_ptr(), d_out[1].data_ptr(),
                     d_out[3].data_ptr(), d_out[2].data_ptr(), d_out[4].data_ptr(), d_res.data_ptr())
    torch.cuda.synchronize()
    out = [x.cpu().numpy() for x in d_out]
    res = d_res.cpu().numpy()
    assert (res[len(names) * rsz:] == SENTINEL).all()
    res = res[:len(names) * rsz].view(L.LBA_RESULT_DTYPE)
    written = [np.zeros(len(o), bool) for o in out]
    got = {}
    for i, name in enumerate(names):
        P = C.case(name)["P"]
        sl = []
        for j, w in enumerate(widths):
            a, b = where[i][j] * w, (where[i][j] + len(P[1 + j])) * w
            written[j][a:b] = True
            sl.append(out[j][a:b])
        got[name] = dict(Tcw=sl[0].view(np.float32).reshape(-1, 16), points=sl[1].view(np.float32).reshape(-1, 3),
                         point_outlier=sl[2], planes=sl[3].view(np.float32).reshape(-1, 4), plane_outlier=sl[4],
                         result=res[i])
    for j, o in enumerate(out):  # the guard rows between and beyond the problems' rows
        assert (o[~written[j]] == SENTINEL).all(), ("guard rows overwritten in output", j)
    return got


def _same_as_single(got, singles):
    for name, g in got.items():
        s = singles[name]
        for k in ("Tcw", "points", "planes", "point_outlier", "plane_outlier"):
            assert np.array_equal(g[k], s[k]), (name, k)
        for k in ("status", "trials", "stopped", "n_point_outliers", "n_plane_outliers"):
            assert g["result"][k] == s["result"][k], (name, k)
        assert list(g["result"]["iterations"]) == list(s["result"]["iterations"]), name


def test_batch_of_narrow_windows(lba, singles):
    """Every window of at most 64 keyframes in one call: the narrow instance."""
    names = [n for n in FAST if C.case(n)["want"]["pw"] == 1]
    assert len(names) > 60
    _same_as_single(_batch(lba, names), singles)


def test_batch_mixed_with_wide_windows(lba, singles):
    """Every case in one call: the windows of more than 64 keyframes put the whole batch, the small windows
    included, on the wide instance (kLdsN 90, kSchurBlk 360, two-word pose masks)."""
    assert {C.case(n)["want"]["pw"] for n in FAST} == {1, 2}
    _same_as_single(_batch(lba, FAST), singles)


@pytest.mark.parametrize("team", TEAMS)
def test_team_split_on_sparse_windows(lba, team):
    lba.set_team(team)
    try:
        for name in TEAM_CASES:
            _identical(lba(*C.case(name)["P"][:6]), C.oracle(name), f"{name} team {team}")
    finally:
        lba.set_team(0)


_CHILD = """
import sys
sys.path[:0] = {path!r}
import lba_cases as C, spslam_gpu, spslam_lba, test_gpu_lba_geometry as T
ex = spslam_gpu.OrbExtractor(max_batch=1)
lba = spslam_lba.LocalBA(ex)
for team in T.TEAMS:
    lba.set_team(team)
    for name in T.TEAM_CASES:
        T._identical(lba(*C.case(name)["P"][:6]), C.oracle(name), f"{{name}} team {{team}}")
ex.close()
print("team children identical")
"""


@pytest.mark.parametrize("rows_max_team", [0, 1])
def test_team_split_other_schur_layout(rows_max_team):
    """SPSLAM_LBG_ROWS_MAX_TEAM lowered in a fresh process: members with fewer than 16 pattern blocks then take the
    lane-per-entry Schur layout at every team size, the others keep the row-group layout."""
    env = dict(os.environ, SPSLAM_LBG_ROWS_MAX_TEAM=str(rows_max_team))
    r = subprocess.run([sys.executable, "-c", _CHILD.format(path=[p for p in sys.path if p])], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0 and "team children identical" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("mask", [0b1, 0b1100])
def test_failed_solves_under_a_permutation(lba, mask):
    """Forced solve failures on an AMD-ordered system of 132 rows: the kept solution vector is read back through the
    permutation."""
    import oracle_ctypes
    import oracle_lba
    import spslam_gpu
    name = "free22-band(2)"
    P = C.case(name)["P"]
    try:
        spslam_gpu.debug_force_solve_failures(lba.ex, mask)
        g = lba(*P[:6])
    finally:
        spslam_gpu.debug_force_solve_failures(lba.ex, 0)
    with oracle_ctypes.solve_failures(mask):
        o = oracle_lba.lba_optimize(*P[:6])
    _identical(g, o, f"{name} mask {mask:#x}")
    assert not np.array_equal(o["Tcw"], C.oracle(name)["Tcw"])  # the failures are observable in the bits


@pytest.mark.parametrize("name", [n for n in FAST if C.case(n)["want"].get("fast")])
def test_fast_order_past_eight_free_poses(lba, name):
    """13 free poses (the matrix-core Schur complement's last size) and 14 (the pose-pair tasks), dense and banded:
    the decisions of the g2o order, values within 1e-4 relative."""
    import spslam_lba
    import test_gpu_lba
    P, o = C.case(name)["P"], C.oracle(name)
    lba.set_order(spslam_lba.FAST_ORDER)
    try:
        g = lba(*P[:6])
    finally:
        lba.set_order(spslam_lba.G2O_ORDER)
    assert list(g["result"]["iterations"]) == list(o["result"]["iterations"]), name
    assert np.array_equal(g["point_outlier"], o["point_outlier"]), name
    assert test_gpu_lba._close(g["Tcw"], o["Tcw"]) and test_gpu_lba._close(g["points"], o["points"]), name


def test_rank_counting_second_tile(lba):
    """34,817 points with ids out of list order: setup()'s rank counting takes a second LDS tile."""
    name = "rank-tiles-34817"
    P = C.case(name)["P"]
    t0 = time.perf_counter()
    o = C.oracle(name)
    t1 = time.perf_counter()
    g = lba(*P[:6])
    t2 = time.perf_counter()
    print(f"\n{name}: oracle {t1 - t0:.2f} s, device {t2 - t1:.2f} s")
    _identical(g, o, name)
