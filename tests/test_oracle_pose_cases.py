"""The case tables of test_gpu_pose_geometry.py (pose_common.py), with the oracle alone: every case still has the
counts its name states and still gives the oracle what it is there for -- convergence, rejected trials, flagged
plane edges on both sides of the plane cache, a problem that ends without an inlier, planes through the camera
centre -- so a change of the generator cannot quietly empty the GPU tests.  These are conditions on the seeds, not
measurements: a seed that fails one is replaced.
"""
import re

import numpy as np
import pytest

import pose_common as PC

TABLES = PC.TABLES
ALL_CASES = [(t, n) for t, tab in TABLES.items() for n in tab]


@pytest.mark.parametrize("table,name", ALL_CASES)
def test_case_counts_and_convergence(table, name):
    c = TABLES[table][name]
    prob, pts, pls, Tgt = PC.problem(table, name)
    assert (len(pts), len(pls)) == (c["n_points"], c["n_planes"])
    assert (int(prob["n_points"]), int(prob["n_planes"])) == (c["n_points"], c["n_planes"])
    m = re.fullmatch(r"p(\d+)(?:_l(\d+))?(?:_\d+deg)?", name)
    if m:   # the counts the name states
        assert (c["n_points"], c["n_planes"]) == (int(m.group(1)), int(m.group(2) or 0))
    assert c["why"]
    ro, poo, ploo = PC.expected(table, name)
    assert len(poo) == c["n_points"] and len(ploo) == c["n_planes"]
    assert int(ro["trials"]) >= int(ro["lm_iterations"]) >= 1 and int(ro["trial_passes"]) == 0
    if not c["degenerate"]:
        dr, dt = PC.pose_error(ro["Tcw"], Tgt)
        assert dr <= PC.GT_TOL and dt <= PC.GT_TOL, (dr, dt)
    if c["perturbed"]:
        assert int(ro["trials"]) > int(ro["lm_iterations"])


def test_tables_hold_the_seams():
    """The rows the tables are there for."""
    assert [c["n_points"] for c in PC.POINT_SEAM_CASES.values()] == \
        [3, 9, 10, 63, 64, 65, 447, 448, 449, 511, 512, 513, 896, 897, 1024]
    assert all(c["n_planes"] == 0 for c in PC.POINT_SEAM_CASES.values())
    counts = {(c["n_points"], c["n_planes"]) for c in PC.PLANE_SEAM_CASES.values()}
    assert counts == {(300, n) for n in (1, 8, 9, 55, 56, 57, 63, 64, 65, 112, 113, 129, 200)} | \
        {(3, 6), (3, 7), (5, 64), (3, 129)}
    assert {(c["n_points"], c["n_planes"]) for c in PC.RING_WRAP_CASES.values()} == \
        {(500, 30), (2040, 20), (2049, 130), (4097, 200)}
    for n, l in ((500, 30),):        # the pass-A ring wraps inside the plane rounds
        assert n < 512 < n + l
    for n, l in ((2040, 20),):       # the kSpec 4 pass-B ring wraps inside the plane rounds
        assert n < 2048 < n + l
    starts = {(c["n_points"], c["n_planes"], c["kw"]["rot_deg"], c["kw"]["trans"])
              for c in PC.CONTENT_CASES.values() if c["perturbed"]}
    assert starts >= {(n, l, r, t) for n, l in ((600, 20), (300, 100))
                      for r, t in ((5.0, 0.2), (15.0, 0.5), (40.0, 1.0), (90.0, 2.0))}
    for table, name in PC.SPEC_CASES + PC.FAILURE_CASES:
        assert name in TABLES[table]
    assert {TABLES[t][n]["n_planes"] <= 64 for t, n in PC.FAILURE_CASES} == {True, False}


def test_generator_content():
    """What the generator promises of every problem with enough edges to show it."""
    levels = set(np.float32(PC.level_inv_sigma2()))
    assert len(levels) == 8
    prob, pts, pls, Tgt = PC.problem("ring_wraps", "p2049_l130")
    assert set(pts["inv_sigma2"]) == levels
    assert np.array_equal(pls["kind"], np.sort(pls["kind"])) and np.bincount(pls["kind"]).tolist() == [44, 43, 43]
    for f in ("meas", "world"):     # both Converter::toPlane3D sign flips, on about a third of the rows each
        assert 0.25 < (pls[f][:, 3] < 0).mean() < 0.42, f
        assert np.allclose(np.linalg.norm(pls[f][:, :3].astype(np.float64), axis=1), 1.0, atol=1e-6)
    # the ground-truth camera sees every point in front of it, 0.5 - 5 m away (the displaced ones apart)
    Xc = pts["xw"].astype(np.float64) @ Tgt[:3, :3].T + Tgt[:3, 3]
    assert np.quantile(Xc[:, 2], 0.1) > 0.5 and Xc[:, 2].max() < 6.5
    # kind 2: a world plane perpendicular to the measured one, at the ground truth
    ver = pls[pls["kind"] == 2]
    cosines = np.einsum("ij,ij->i", ver["world"][:, :3].astype(np.float64) @ Tgt[:3, :3].T,
                        ver["meas"][:, :3].astype(np.float64))
    assert np.abs(cosines).max() < 0.03
    assert (pts["ur"] < 0).sum() == round(0.02 * 2049)
    cfg, tum = PC.second_config(), __import__("spslam_gpu").PlaneConfig.tum()
    assert all(getattr(cfg, f) != getattr(tum, f) for f, _ in cfg._fields_)


def test_mono_shares():
    for name, share in (("all_mono", 1.0), ("all_stereo", 0.0)):
        pts = PC.problem("content", name)[1]
        assert (pts["ur"] < 0).mean() == share, name


def test_all_outlier_case_ends_without_inliers():
    """No inlier at the end, and a last round without an active edge: the reference restarts every round from
    the input pose and an optimize() without edges leaves it there."""
    prob = PC.problem("content", "all_outliers")[0]
    ro, poo, _ = PC.expected("content", "all_outliers")
    assert int(ro["n_inliers"]) == 0 and poo.all()
    assert np.abs(ro["Tcw"] - prob["Tcw"]).max() < 1e-6
    # a round without an active edge runs no iteration and no trial (g2o's optimize() returns at once)
    assert 1 <= int(ro["lm_iterations"]) <= 30 and int(ro["trials"]) <= 300


def test_flagged_plane_edges_on_both_sides_of_the_cache():
    flagged = {}
    for name in PC.FLAGGED_PLANE_CASES:
        c = PC.CONTENT_CASES[name]
        flagged[name] = int(PC.expected("content", name)[2].sum())
        assert 0 < flagged[name] < c["n_planes"], flagged
        assert c["kw"]["rot_deg"] >= 90
    assert {PC.CONTENT_CASES[n]["n_planes"] <= 64 for n in flagged} == {True, False}
    # and points behind the start camera
    for name in flagged:
        prob, pts, _, _ = PC.problem("content", name)
        T0 = prob["Tcw"].reshape(4, 4).astype(np.float64)
        assert ((pts["xw"].astype(np.float64) @ T0[:3, :3].T + T0[:3, 3])[:, 2] < 0).any()


@pytest.mark.parametrize("name", PC.FALLBACK_CASES)
def test_fallback_cases_have_planes_through_the_camera_centre(name):
    """From the float32 inputs: the start's translation is exactly 0 and at least three edges of every kind have a
    world plane with distance 0 and no small normal component, so at the start pose the +1e-9 and -1e-9
    translation steps leave the plane distance -(+-1e-9 n_x) on opposite sides of zero."""
    prob, pts, pls, _ = PC.problem("content", name)
    T0 = prob["Tcw"].reshape(4, 4)
    assert T0.dtype == np.float32 and np.array_equal(T0[:3, 3], np.zeros(3, np.float32))
    assert not np.signbit(T0[:3, 3]).any()
    through = (pls["world"][:, 3] == 0) & ~np.signbit(pls["world"][:, 3])
    assert np.bincount(pls["kind"][through], minlength=3).min() >= 3
    n_cam = pls["world"][through][:, :3].astype(np.float64) @ T0[:3, :3].astype(np.float64).T
    assert np.abs(pls["world"][through][:, :3]).min() >= 0.29 and np.abs(n_cam).min() > 0.05
    d_plus, d_minus = 0.0 - 1e-9 * n_cam[:, 0], 0.0 + 1e-9 * n_cam[:, 0]
    assert ((d_plus < 0) != (d_minus < 0)).all()
    assert len(pts) >= 200


def test_fallback_variants():
    """The moved variant's result differs from its input and is the ground truth; the stuck one stays."""
    prob, _, _, Tgt = PC.problem("content", "fallback_moved")
    ro, _, ploo = PC.expected("content", "fallback_moved")
    assert not np.array_equal(ro["Tcw"], prob["Tcw"])
    assert PC.pose_error(prob["Tcw"], Tgt)[0] > PC.GT_TOL >= max(PC.pose_error(ro["Tcw"], Tgt))
    assert ploo[:3].all() and not ploo[3:].any()    # the kind 0 edges through the centre, and only they
    prob, _, _, Tgt = PC.problem("content", "fallback_stuck")
    ro = PC.expected("content", "fallback_stuck")[0]
    assert PC.pose_error(ro["Tcw"], Tgt)[0] > PC.GT_TOL


def test_forced_failures_change_the_oracle():
    """The masks of the forced-failure test do something at its shapes."""
    for table, name in PC.FAILURE_CASES:
        free = PC.expected(table, name)[0]
        for mask in PC.FAILURE_MASKS:
            forced = PC.expected(table, name, mask)[0]
            assert int(forced["trials"]) != int(free["trials"]) or not np.array_equal(forced["Tcw"], free["Tcw"])
