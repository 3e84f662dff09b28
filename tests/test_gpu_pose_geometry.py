"""GPU parity of PoseOptimization off the twelve problems of test_gpu_pose.py: the case tables of pose_common.py
(edge counts at every seam of the kernel's staging schedule, rings wrapped by point and by plane rows, the plane
cache on and off, contents the scene problems never had) against the CPU oracle, bit for bit -- Tcw, n_inliers,
lm_iterations, trials and both outlier flag arrays.  Also one mixed batch through the device entry with the bytes
between the problems watched, forced solve failures at the new shapes, and the seam cases under kSpec 1 and 2.
test_oracle_pose_cases.py checks on the CPU that every case still is what its row says.
"""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import pose_common as PC

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]
CHILD_TIMEOUT = 120   # seconds, one child process (eight problems and the context's start-up)


@pytest.fixture(scope="module")
def gpu():
    import spslam_gpu
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    yield ex
    ex.close()


@pytest.mark.parametrize("table,name", [(t, n) for t, tab in PC.TABLES.items() for n in tab])
def test_case_bit_exact_to_oracle(gpu, table, name):
    import spslam_gpu
    prob, pts, pls, _ = PC.problem(table, name)
    got = spslam_gpu.pose_optimize(gpu, prob, pts, pls, PC.config_of(PC.TABLES[table][name]))
    PC.assert_equal_to_oracle(got, PC.expected(table, name), f"{table}/{name} ({PC.TABLES[table][name]['why']})")


# ---------------------------------------------------------------------------
# One mixed batch through the device entry.

BATCH = (("early_return_2_points", None), ("point_seams", "p3"), ("plane_seams", "p300_l65"),
         ("point_seams", "p448"),           # no planes, between two problems that have them
         ("ring_wraps", "p2049_l130"), ("content", "all_outliers"))
GAP = 5   # observation slots (and outlier bytes) no problem owns, before, between and after the problems


def _batch_problems():
    out = []
    for table, name in BATCH:
        out.append(PC.pose_problem(2, 5, seed=3)[:3] if name is None else PC.problem(table, name)[:3])
    return out


def _run_batch(gpu, torch, probs, pts_all, pls_all, init_from=None):
    import spslam_gpu as G
    n = len(probs)
    dev = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()
    d_probs, d_pts, d_pls = dev(probs), dev(pts_all), dev(pls_all)
    d_res = torch.zeros(n * G.POSE_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_po = torch.full((len(pts_all),), PC.SENTINEL, dtype=torch.uint8, device="cuda")
    d_plo = torch.full((len(pls_all),), PC.SENTINEL, dtype=torch.uint8, device="cuda")
    d_init = dev(init_from) if init_from is not None else None
    G.pose_optimize_batch_device(gpu, n, d_probs.data_ptr(), d_pts.data_ptr(), d_pls.data_ptr(), d_res.data_ptr(),
                                 d_po.data_ptr(), d_plo.data_ptr(),
                                 init_from_ptr=d_init.data_ptr() if d_init is not None else 0,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_res.cpu().numpy().view(G.POSE_RESULT_DTYPE).copy(), d_po.cpu().numpy(), d_plo.cpu().numpy()


def test_mixed_batch_device_chained(gpu):
    """Problems of every kind in one launch, each against the oracle; then the same launch started from the first
    results.  The observation slots between the problems hold NaN and the outlier bytes there a sentinel: the
    kernel owns [offset, offset + n) of each array and nothing else (the tail's discard reads those bytes)."""
    torch = pytest.importorskip("torch")
    import oracle_ctypes
    import spslam_gpu as G
    problems = _batch_problems()
    probs = np.zeros(len(problems), G.POSE_PROBLEM_DTYPE)
    po_off, pl_off = GAP, GAP
    for i, (prob, pts, pls) in enumerate(problems):
        probs[i] = prob
        probs[i]["point_offset"], probs[i]["plane_offset"] = po_off, pl_off
        po_off += len(pts) + GAP
        pl_off += len(pls) + GAP
    pts_all = np.frombuffer(np.full(po_off * G.POINT_OBS_DTYPE.itemsize // 4, np.nan, np.float32).tobytes(),
                            G.POINT_OBS_DTYPE).copy()
    pls_all = np.frombuffer(np.full(pl_off * G.PLANE_OBS_DTYPE.itemsize // 4, np.nan, np.float32).tobytes(),
                            G.PLANE_OBS_DTYPE).copy()
    owned_po, owned_pl = np.zeros(po_off, bool), np.zeros(pl_off, bool)
    for p, (_, pts, pls) in zip(probs, problems):
        a, b = int(p["point_offset"]), int(p["plane_offset"])
        pts_all[a:a + len(pts)], pls_all[b:b + len(pls)] = pts, pls
        owned_po[a:a + len(pts)], owned_pl[b:b + len(pls)] = True, True
    assert (~owned_po).sum() == GAP * (len(problems) + 1) and (~owned_pl).sum() == GAP * (len(problems) + 1)

    def check(res, po, plo, wants, what):
        assert (po[~owned_po] == PC.SENTINEL).all(), f"{what}: point outlier bytes outside the problems written"
        assert (plo[~owned_pl] == PC.SENTINEL).all(), f"{what}: plane outlier bytes outside the problems written"
        for i, (prob, pts, pls) in enumerate(problems):
            a, b = int(probs[i]["point_offset"]), int(probs[i]["plane_offset"])
            got = (res[i], po[a:a + len(pts)], plo[b:b + len(pls)])
            assert set(np.unique(got[1])) | set(np.unique(got[2])) <= {0, 1}, f"{what}: problem {i} flag bytes"
            PC.assert_equal_to_oracle(got, wants[i], f"{what}: problem {i} {BATCH[i]}")

    def oracle_from(i, Tcw):
        prob, pts, pls = problems[i]
        p = prob.copy()
        p["Tcw"] = Tcw
        return oracle_ctypes.pose_optimize(p, pts, pls)

    res1, po1, plo1 = _run_batch(gpu, torch, probs, pts_all, pls_all)
    check(res1, po1, plo1, [PC.expected(t, n) if n else oracle_from(i, problems[i][0]["Tcw"])
                            for i, (t, n) in enumerate(BATCH)], "first launch")
    assert int(res1[0]["n_inliers"]) == 0 and int(res1[0]["trials"]) == 0   # fewer than 3 points: the early return
    assert np.array_equal(res1[0]["Tcw"], problems[0][0]["Tcw"])
    assert int(res1[-1]["n_inliers"]) == 0 and po1[owned_po][-200:].all()    # the all-outlier problem
    res2, po2, plo2 = _run_batch(gpu, torch, probs, pts_all, pls_all, init_from=res1)
    check(res2, po2, plo2, [oracle_from(i, res1[i]["Tcw"]) for i in range(len(problems))], "chained launch")


# ---------------------------------------------------------------------------
# Forced solve failures at the new shapes.

@pytest.mark.parametrize("mask", PC.FAILURE_MASKS, ids=lambda m: f"{m:#x}")
@pytest.mark.parametrize("table,name", PC.FAILURE_CASES)
def test_failed_solves_at_the_seams(gpu, table, name, mask):
    """g2o's failed-LDLT path (test_gpu_pose.py test_pose_failed_solve_keeps_previous_solution) with the plane
    cache off, past the kSpec 4 pass-B ring and with the cache on.  0b11111: five failures in a row, a second
    trial pass within one iteration; 0xFFFFFFFF: every one of the first 32 trials."""
    import spslam_gpu
    prob, pts, pls, _ = PC.problem(table, name)
    try:
        spslam_gpu.debug_force_solve_failures(gpu, mask)
        got = spslam_gpu.pose_optimize(gpu, prob, pts, pls)
    finally:
        spslam_gpu.debug_force_solve_failures(gpu, 0)
    PC.assert_equal_to_oracle(got, PC.expected(table, name, mask), f"{name} mask {mask:#x}")


# ---------------------------------------------------------------------------
# kSpec 1 and 2 at the seams (SPSLAM_POSE_SPEC is read once per process: one fresh child each).

@pytest.mark.parametrize("spec", ["1", "2"])
def test_seams_independent_of_trial_batching(spec, tmp_path):
    """Pass-B plane rounds of 224 (kSpec 1) and 112 (kSpec 2) edges and the 4096-row pass-B ring, against the
    oracle (not against the kSpec 4 run)."""
    dst = tmp_path / f"spec{spec}.npz"
    env = dict(os.environ, SPSLAM_POSE_SPEC=spec)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "pose_common.py"), str(dst)], env=env,
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, r.stderr[-2000:]
    data = np.load(dst, allow_pickle=False)
    for table, name in PC.SPEC_CASES:
        got = (data[f"{name}/res"], data[f"{name}/po"], data[f"{name}/plo"])
        PC.assert_equal_to_oracle(got, PC.expected(table, name), f"kSpec {spec} {name}")
