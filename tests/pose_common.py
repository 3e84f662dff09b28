"""Shared by the PoseOptimization geometry tests: a generator of problems with exact edge counts (no ORB, no
rendered frame), the case tables of test_gpu_pose_geometry.py / test_oracle_pose_cases.py, the comparison with the
CPU oracle and (run as a script) the child process that runs cases under the SPSLAM_POSE_SPEC it was started with.

Bar of every comparison (test_gpu_pose.py's): Tcw bit-equal, n_inliers, lm_iterations and trials equal, both
outlier flag arrays equal.

What the tables are sized against (sp-slam_amd/csrc/pose_kernels.hip): seven compute waves stage 448 point edges
per round; plane rounds take 7 * ps edges, ps = 8 (9 once an accepted trial left its plane errors behind) in pass A
and 32 / kSpec in pass B; the pass-A ring has 512 rows, the pass-B ring 2048 (kSpec 4) or 4096 (kSpec 1, 2); the
plane cache and the saved trial errors exist only while n_planes <= 64.
"""
import functools
import pathlib
import sys

import numpy as np

SENTINEL = 0xA5          # fill of the outlier bytes no problem owns
GT_TOL = 2e-2            # test_gpu_pose.py's distance to the ground truth
CAM = dict(fx=535.4, fy=539.2, cx=320.1, cy=247.6, bf=40.0)   # TUM3 (synth.TUM3), 640 x 480


def _rot(axis_angle):
    th = np.linalg.norm(axis_angle)
    if th < 1e-12:
        return np.eye(3)
    k = axis_angle / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _unit(rng, min_abs=0.0):
    """A random unit vector; min_abs > 0: none of its components is smaller than that."""
    while True:
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        if np.abs(v).min() >= min_abs:
            return v


def _perpendicular(rng, n, min_abs=0.0):
    while True:
        v = np.cross(n, _unit(rng))
        if np.linalg.norm(v) < 0.2:
            continue
        v /= np.linalg.norm(v)
        if np.abs(v).min() >= min_abs:
            return v


def _transform_plane(T, p):
    """operator*(Isometry3D, Plane3D): the plane n . X + d = 0 of the world, in the camera of Tcw = T."""
    n2 = T[:3, :3] @ p[:3]
    return np.array([*n2, p[3] - T[:3, 3] @ n2])


def _positive(p):
    return -p if p[3] < 0 else p


@functools.lru_cache(maxsize=None)
def level_inv_sigma2():
    """mvInvLevelSigma2 of the oracle's eight pyramid levels."""
    import oracle_ctypes
    return tuple(float(v) for v in oracle_ctypes.OrbOracle().scale_tables()[3])


def pose_problem(n_points, n_planes, seed, mono=0.02, outliers=0.08, rot_deg=2.0, trans=0.05, pix_noise=0.5,
                 origin_planes=0, origin_turn_deg=0.0):
    """(problem record, point obs, plane obs, Tcw_gt) like synth.pose_problem, with exactly n_points and n_planes.

    Points: uniform pixels, 0.5 - 5 m in front of the ground-truth camera, pixel noise; round(mono * n) of them
    without a right coordinate, round(outliers * n) displaced by 0.3 m; inv_sigma2 from the eight level values.
    Planes: random unit planes of kinds 0, 1, 2 in rotation (listed kind 0 first, then 1, then 2, as the header
    asks): the frame's plane is a world plane seen from the ground truth with 0.3 deg / 5 mm of noise; its map
    plane is that world plane (kind 0), a parallel one (kind 1) or one perpendicular to it (kind 2).  A third of
    the world rows and a third of the measured rows have d < 0, so both Converter::toPlane3D sign flips run.
    The start is the ground truth turned by rot_deg about a random axis and moved by trans along another.
    origin_planes = k > 0: the ground-truth camera sits at the world origin and the start has translation exactly
    0; the first k planes of every kind have a world plane through the origin (world[3] == 0) whose normal has no
    component below 0.3."""
    import spslam_gpu as G
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = (CAM[k] for k in ("fx", "fy", "cx", "cy", "bf"))
    Tcw = np.eye(4)
    if not origin_planes:
        Tcw[:3, :3] = _rot(_unit(rng) * np.deg2rad(rng.uniform(0, 25)))
        Tcw[:3, 3] = rng.uniform(-1.0, 1.0, 3)
    Twc = np.linalg.inv(Tcw)

    points = np.zeros(n_points, G.POINT_OBS_DTYPE)
    z = rng.uniform(0.5, 5.0, n_points)
    order = rng.permutation(n_points)
    is_mono = np.zeros(n_points, bool)
    is_mono[order[:int(round(mono * n_points))]] = True
    # a stereo point's right coordinate u - bf / z stays positive under the noise (ur < 0 would make it monocular)
    u_min = np.where(is_mono, 0.0, bf / z + 5 * pix_noise + 1)
    u, v = rng.uniform(u_min, 640), rng.uniform(0, 480, n_points)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Xw = Xc @ Twc[:3, :3].T + Twc[:3, 3]
    order = rng.permutation(n_points)
    is_out = np.zeros(n_points, bool)
    is_out[order[:int(round(outliers * n_points))]] = True
    Xw[is_out] += rng.normal(0, 0.3, (int(is_out.sum()), 3))
    points["u"] = u + rng.normal(0, pix_noise, n_points)
    points["v"] = v + rng.normal(0, pix_noise, n_points)
    points["ur"] = np.where(is_mono, -1.0, np.maximum(u - bf / z + rng.normal(0, pix_noise, n_points), 0.0))
    points["inv_sigma2"] = np.array(level_inv_sigma2())[rng.integers(0, 8, n_points)]
    points["xw"] = Xw
    points["kp_index"] = np.arange(n_points)

    planes = np.zeros(n_planes, G.PLANE_OBS_DTYPE)
    kinds = np.sort(np.arange(n_planes) % 3)
    seen = [0, 0, 0]
    for j, kind in enumerate(kinds):
        through_origin = seen[kind] < origin_planes
        seen[kind] += 1
        nf = _unit(rng, 0.3 if through_origin else 0.0)        # the frame's plane, in the world
        df = 0.0 if through_origin and kind == 0 else rng.uniform(0.5, 3.0)
        if kind == 0:
            world = np.array([*nf, df])
        elif kind == 1:
            world = np.array([*nf, 0.0 if through_origin else rng.uniform(0.5, 3.0)])
        else:
            world = np.array([*_perpendicular(rng, nf, 0.3 if through_origin else 0.0),
                              0.0 if through_origin else rng.uniform(0.5, 3.0)])
        cp = _transform_plane(Tcw, np.array([*nf, df]))
        meas = np.array([*(_rot(rng.normal(0, np.deg2rad(0.3), 3)) @ cp[:3]), cp[3] + rng.normal(0, 0.005)])
        if through_origin and kind == 0 and origin_turn_deg:
            meas[:3] = _rot(_perpendicular(rng, meas[:3]) * np.deg2rad(origin_turn_deg)) @ meas[:3]
        meas, world = _positive(meas), _positive(world)
        if j % 3 == 1:
            meas = -meas
        if j % 3 == 2 and not through_origin:
            world = -world
        planes[j]["meas"], planes[j]["world"] = meas, world + 0.0   # (+ 0.0: no negative zero distance)
        planes[j]["kind"], planes[j]["plane_index"], planes[j]["map_plane_id"] = kind, j, j

    T0 = Tcw.copy()
    T0[:3, :3] = _rot(_unit(rng) * np.deg2rad(rot_deg)) @ Tcw[:3, :3]
    T0[:3, 3] = Tcw[:3, 3] + (0.0 if origin_planes else trans) * _unit(rng)
    prob = np.zeros((), G.POSE_PROBLEM_DTYPE)
    prob["Tcw"] = T0.astype(np.float32).ravel()
    prob["fx"], prob["fy"], prob["cx"], prob["cy"], prob["bf"] = fx, fy, cx, cy, bf
    prob["n_points"], prob["n_planes"] = n_points, n_planes
    return prob, points, planes, Tcw


def second_config():
    """A PlaneConfig that differs from PlaneConfig.tum() in every field."""
    import spslam_gpu as G
    return G.PlaneConfig(2.0, 60.0, 1.0, 0.8, 120.0, 90.0)


# ---------------------------------------------------------------------------
# Case tables.  Every row: the counts, the seed, the generator's other arguments and what the row is there for.
# degenerate: the oracle is not expected to end at the ground truth.  perturbed: rejected trials are expected
# (trials > lm_iterations).  config: "second" = second_config().

def case(n_points, n_planes, why, seed=1, degenerate=False, perturbed=False, config=None, **kw):
    return dict(n_points=n_points, n_planes=n_planes, seed=seed, why=why, degenerate=degenerate,
                perturbed=perturbed, config=config, kw=kw)


POINT_SEAM_CASES = {
    "p3": case(3, 0, "the reference's minimum (nInitialCorrespondences >= 3); one round (< 10 edges)", mono=0,
               outliers=0, pix_noise=0.1),
    "p9": case(9, 0, "the last count with the single-round break", outliers=0),
    "p10": case(10, 0, "the first count that runs all four rounds", outliers=0),
    "p63": case(63, 0, "a partial wave"),
    "p64": case(64, 0, "a whole wave"),
    "p65": case(65, 0, "a whole wave and one edge of the next"),
    "p447": case(447, 0, "a partial 448-edge round"),
    "p448": case(448, 0, "a whole round"),
    "p449": case(449, 0, "a whole round and a second one of one edge"),
    "p511": case(511, 0, "one row short of the pass-A ring"),
    "p512": case(512, 0, "the last segment ends exactly at the ring end (chain_seg reads up to 23 rows past it)"),
    "p513": case(513, 0, "the pass-A ring wraps by one row"),
    "p896": case(896, 0, "two whole rounds"),
    "p897": case(897, 0, "two whole rounds and one edge"),
    "p1024": case(1024, 0, "two ring lengths"),
}

PLANE_SEAM_CASES = dict(
    {f"p300_l{n}": case(300, n, why) for n, why in (
        (1, "one plane edge"),
        (8, "ps = 8: wave 0's share of a pass-A round, one pass-B share at kSpec 4"),
        (9, "ps = 9 (plane errors left behind): wave 0's share; ps = 8: one edge into wave 1"),
        (55, "one short of a 56-edge plane round"),
        (56, "a whole 56-edge plane round (pass A with ps 8, pass B at kSpec 4)"),
        (57, "a 56-edge round and one edge"),
        (63, "a whole 63-edge plane round (pass A with ps 9)"),
        (64, "the largest count with the plane cache, perrB and perrT"),
        (65, "the smallest count without them: every evaluation reads and normalizes the planes"),
        (112, "a whole pass-B plane round at kSpec 2; two at kSpec 4"),
        (113, "the same and one edge"),
        (129, "past two plane chunks"),
        (200, "a pass-B plane round of 224 at kSpec 1 left partial; four rounds at kSpec 4"))},
    p3_l6=case(3, 6, "the single-round break with planes (9 edges)", mono=0, outliers=0, pix_noise=0.1),
    p3_l7=case(3, 7, "four rounds, mostly plane edges (10 edges)", mono=0, outliers=0, pix_noise=0.1),
    p5_l64=case(5, 64, "plane-dominated, cache on", mono=0, outliers=0),
    p3_l129=case(3, 129, "plane-dominated, cache off", mono=0, outliers=0, pix_noise=0.1),
)

RING_WRAP_CASES = {
    "p500_l30": case(500, 30, "the pass-A ring (512 rows) wraps inside the plane rounds"),
    "p2040_l20": case(2040, 20, "the kSpec 4 pass-B ring (2048 rows) wraps inside the plane rounds"),
    "p2049_l130": case(2049, 130, "the kSpec 4 pass-B ring wraps at the points; cache off"),
    "p4097_l200": case(4097, 200, "the kSpec 1 and 2 pass-B ring (4096 rows) wraps"),
}

CONTENT_CASES = dict(
    {
        "all_mono": case(600, 20, "every point edge monocular", mono=1.0),
        "all_stereo": case(600, 20, "every point edge stereo", mono=0.0),
        "all_outliers": case(200, 0, "every point displaced, 30 deg / 1 m start: the oracle ends with no inlier, "
                             "so the later rounds have no active edge", seed=7, degenerate=True, outliers=1.0,
                             rot_deg=30.0, trans=1.0),
        "second_config": case(600, 20, "a PlaneConfig that differs from tum() in every field", config="second"),
        "second_config_l100": case(300, 100, "the same with the plane cache off", config="second"),
    },
    **{f"p{n}_l{l}_{int(r)}deg": case(n, l, f"start {r} deg / {t} m off: rejected trials" + (
                                         "; most plane edges end flagged, points behind the camera" if r >= 90 else ""),
                                     seed=s, perturbed=True, degenerate=r >= 90, rot_deg=r, trans=t)
       # seeds chosen by the oracle: trials > lm_iterations everywhere; at 90 and 170 deg it ends far from the
       # ground truth with 19, 18 of 20 and 93, 97 of 100 plane edges flagged
       for n, l, r, t, s in ((600, 20, 5.0, 0.2, 1), (600, 20, 15.0, 0.5, 1), (600, 20, 40.0, 1.0, 1),
                             (600, 20, 90.0, 2.0, 7), (600, 20, 170.0, 2.0, 2),
                             (300, 100, 5.0, 0.2, 1), (300, 100, 15.0, 0.5, 1), (300, 100, 40.0, 1.0, 1),
                             (300, 100, 90.0, 2.0, 1), (300, 100, 170.0, 2.0, 5))},
    **{
        # the camera at the world origin and planes through it: at the first pass A of every round the +1e-9 and
        # -1e-9 translation steps put the plane distance on opposite sides of zero, so the shared evaluation of
        # the five other translation perturbations is refused and the full evaluation runs.  The kind 0 edges'
        # numeric Jacobians are then of the order 1e9 (the transformed normal changes sign between the two steps)
        # and hold the translation; kinds 1 and 2 do not depend on that sign.
        "fallback_identity": case(300, 12, "planes through the camera centre, start = ground truth", origin_planes=3,
                                  rot_deg=0.0),
        "fallback_stuck": case(300, 12, "the same from 3 deg off: the damping set by the kind 0 edges holds the "
                               "rotation too, every round", seed=3, degenerate=True, origin_planes=3, rot_deg=3.0),
        "fallback_moved": case(300, 12, "the same with the kind 0 measurements 40 deg off: flagged after the first "
                               "round, the later rounds (kinds 1 and 2 through the centre) reach the ground truth",
                               origin_planes=3, origin_turn_deg=40.0, rot_deg=3.0),
    })
FALLBACK_CASES = ("fallback_identity", "fallback_stuck", "fallback_moved")
FLAGGED_PLANE_CASES = ("p600_l20_90deg", "p600_l20_170deg", "p300_l100_90deg", "p300_l100_170deg")

TABLES = {"point_seams": POINT_SEAM_CASES, "plane_seams": PLANE_SEAM_CASES, "ring_wraps": RING_WRAP_CASES,
          "content": CONTENT_CASES}

# Cases the kSpec 1 and 2 children run: the pass-B plane round lengths 112 and 224, and both pass-B rings.
SPEC_CASES = tuple(("plane_seams", f"p300_l{n}") for n in (56, 57, 112, 113, 129, 200)) + \
    (("ring_wraps", "p2040_l20"), ("ring_wraps", "p4097_l200"))
# Forced solve failures: cache off, cache off past the kSpec 4 pass-B ring, cache on.
FAILURE_CASES = (("plane_seams", "p300_l65"), ("ring_wraps", "p2049_l130"), ("ring_wraps", "p500_l30"))
FAILURE_MASKS = (0b11111, 0xFFFFFFFF)


def config_of(c):
    return second_config() if c["config"] == "second" else None


@functools.lru_cache(maxsize=None)
def problem(table, name):
    """(problem, points, planes, Tcw_gt) of a case, made once per process and left unchanged."""
    c = TABLES[table][name]
    out = pose_problem(c["n_points"], c["n_planes"], c["seed"], **c["kw"])
    for a in out[:3]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(table, name, fail_mask=0):
    """The oracle's (result, point flags, plane flags) of a case, computed once per process."""
    import oracle_ctypes
    prob, pts, pls, _ = problem(table, name)
    with oracle_ctypes.solve_failures(fail_mask):
        return oracle_ctypes.pose_optimize(prob, pts, pls, config_of(TABLES[table][name]))


def pose_error(T, Tgt):
    """(largest rotation entry difference, translation distance over max(|t_gt|, 1)): test_gpu_pose.py's."""
    Ta, Tb = np.asarray(T, np.float64).reshape(4, 4), np.asarray(Tgt, np.float64).reshape(4, 4)
    return (np.abs(Ta[:3, :3] - Tb[:3, :3]).max(),
            np.linalg.norm(Ta[:3, 3] - Tb[:3, 3]) / max(np.linalg.norm(Tb[:3, 3]), 1.0))


RESULT_FIELDS = ("n_inliers", "lm_iterations", "trials")


def assert_equal_to_oracle(got, want, what):
    """got, want = (result record, point flags, plane flags): every compared field, the first differing named."""
    rg, pog, plog = got
    ro, poo, ploo = want
    assert np.array_equal(np.asarray(rg["Tcw"]).view(np.uint32), np.asarray(ro["Tcw"]).view(np.uint32)), \
        f"{what}: Tcw differs, {pose_error(rg['Tcw'], ro['Tcw'])}"
    for f in RESULT_FIELDS:
        assert int(rg[f]) == int(ro[f]), f"{what}: {f} {int(rg[f])} vs {int(ro[f])}"
    pog, poo, plog, ploo = (np.asarray(a, bool) for a in (pog, poo, plog, ploo))
    assert np.array_equal(pog, poo), f"{what}: point outliers differ at {np.nonzero(pog != poo)[0][:10]}"
    assert np.array_equal(plog, ploo), f"{what}: plane outliers differ at {np.nonzero(plog != ploo)[0][:10]}"


# ---------------------------------------------------------------------------
# Child process of the kSpec tests: python pose_common.py <out.npz>.  Runs SPEC_CASES under the SPSLAM_POSE_SPEC
# it was started with (read once per process) and saves every compared field.

def _child(dst):
    root = pathlib.Path(__file__).resolve().parent.parent
    for p in (root / "sp-slam_amd", root / "oracle"):
        sys.path.insert(0, str(p))
    import spslam_gpu
    out = {}
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    try:
        for table, name in SPEC_CASES:
            prob, pts, pls, _ = problem(table, name)
            r, po, plo = spslam_gpu.pose_optimize(ex, prob, pts, pls, config_of(TABLES[table][name]))
            out[f"{name}/res"], out[f"{name}/po"], out[f"{name}/plo"] = r, po, plo
    finally:
        ex.close()
    np.savez(dst, **out)


if __name__ == "__main__":
    _child(sys.argv[1])
