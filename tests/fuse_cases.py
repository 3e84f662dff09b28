"""The cases of the Fuse search tests (tests/test_fuse_host.py guards what each reaches, tests/test_gpu_fuse.py runs
them on the device): problems taken from synthetic sequences -- a keyframe's points into the frame four frames
later, Fuse's geometry -- and hand-made keyframes of a few keypoints that put single candidates on each side of
every test of ORBmatcher.cc:852-949.

A problem: dict(name, Tcw [16], P (spslam_local_point records), kf (index into the keyframe list), th, skip or None).
A keyframe: dict(kun, desc, ur, go, gi).  Hand-made problems use Tcw = identity, so Ow = 0, PO = xw, dist = |xw|.
The camera is synth.TUM3 without distortion: test_oracle_match.make_pairs offers no second camera, so the one with
distortion-shifted bounds (build_distorted) is hand-made too.
"""
import functools

import numpy as np

import fuse_ref as FR
from matcher_ref import f32 as _f

PTS_PER_GROUP = 64  # points per workgroup of fuse_search_kernel (256 threads, 4 lanes per point)
EYE = np.eye(4, dtype=np.float32).reshape(16)


@functools.lru_cache(maxsize=None)
def real_problems():
    """Two sequences' local-map problems (test_oracle_match.local_problems), made once per process."""
    from test_oracle_match import local_problems, make_pairs
    return local_problems(make_pairs(((0, 10, 12), (3, 5, 9)), seed=17), seed=23)


def keyframe_of(q):
    return dict(kun=q["kun"], desc=q["desc"], ur=q["ur"], go=q["go"], gi=q["gi"])


def make_keyframe(kps, geo):
    """kps: [(x, y, octave, uright, descriptor or None)].  The grid as Frame::AssignFeaturesToGrid / PosInGrid make
    it (Frame.cc:326-341, :480-492: round((x - mnMinX) * inv))."""
    import spslam_gpu
    n = len(kps)
    kun = np.zeros(n, spslam_gpu.KEYPOINT_DTYPE)
    desc = np.zeros((n, 32), np.uint8)
    ur = np.zeros(n, np.float32)
    cells = [[] for _ in range(64 * 48)]
    for i, (x, y, o, r, d) in enumerate(kps):
        kun[i]["x"], kun[i]["y"], kun[i]["octave"], ur[i] = x, y, o, r
        if d is not None:
            desc[i] = d
        px = int(np.round(_f(_f(_f(x) - _f(geo[5])) * _f(geo[9]))))
        py = int(np.round(_f(_f(_f(y) - _f(geo[7])) * _f(geo[10]))))
        if 0 <= px < 64 and 0 <= py < 48:
            cells[px * 48 + py].append(i)
    go = np.zeros(64 * 48 + 1, np.int32)
    go[1:] = np.cumsum([len(c) for c in cells])
    gi = np.array([i for c in cells for i in c], np.int32)
    return dict(kun=kun, desc=desc, ur=ur, go=go, gi=gi)


def bits(n_set):
    """A descriptor with the first n_set bits set: distance n_set to the zero descriptor."""
    b = np.zeros(256, np.uint8)
    b[:n_set] = 1
    return np.packbits(b)


def point_at(geo, u, v, z=2.0, level=0):
    """A point record projecting (Tcw = identity) to about (u, v) at depth z, seen head-on, whose PredictScale
    level is `level`: mfMaxDistance = dist * 1.2^level * 0.95."""
    import spslam_match
    p = np.zeros((), spslam_match.LOCAL_POINT_DTYPE)
    fx, fy, cx, cy = [float(c) for c in geo[:4]]
    xw = np.array([(u - cx) * z / fx, (v - cy) * z / fy, z], np.float32)
    dist = float(np.linalg.norm(xw.astype(np.float64)))
    p["xw"] = xw
    p["normal"] = xw / _f(dist)
    p["max_dist"] = dist * 1.2 ** level * 0.95
    p["min_dist"] = p["max_dist"] / _f(1.2 ** 7)
    return p


def x_with_u(geo, target, z=2.0):
    """The float X (Tcw = identity, Y = 0) whose projected u is exactly `target`: u is monotone in X and X's
    spacing is far below u's, so a bisection over the floats lands on it."""
    lo, hi = _f(-10.0), _f(10.0)
    while True:
        mid = _f((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            break
        if FR.projection(geo, mid, _f(0.0), _f(z))[1] < target:
            lo = mid
        else:
            hi = mid
    assert FR.projection(geo, hi, _f(0.0), _f(z))[1] == target, (hi, target)
    return hi


def raw_point(xw, normal, min_dist, max_dist):
    import spslam_match
    p = np.zeros((), spslam_match.LOCAL_POINT_DTYPE)
    p["xw"], p["normal"], p["min_dist"], p["max_dist"] = xw, normal, min_dist, max_dist
    return p


def stack(points):
    import spslam_match
    return np.array(points, spslam_match.LOCAL_POINT_DTYPE) if points else np.zeros(0, spslam_match.LOCAL_POINT_DTYPE)


@functools.lru_cache(maxsize=None)
def build():
    """(keyframes, problems)."""
    real = real_problems()
    geo = real[0]["geo"]
    kfs = [keyframe_of(q) for q in real]
    problems = []

    def add(name, Tcw, P, kf, th=3.0, skip=None):
        problems.append(dict(name=name, Tcw=np.asarray(Tcw, np.float32).reshape(16), P=P, kf=kf, th=th, skip=skip))

    # ---- the sequences' own problems, whole and cut around the points per workgroup
    for k, q in enumerate(real):
        add(f"real{k}", q["lfr"]["Tcw"], q["LP"], k)
    q = real[0]
    add("real0_th30", q["lfr"]["Tcw"], q["LP"][:200], 0, th=30.0)
    for n in (0, 1, PTS_PER_GROUP - 1, PTS_PER_GROUP, PTS_PER_GROUP + 1):
        add(f"real0_n{n}", q["lfr"]["Tcw"], q["LP"][:n], 0)
    rng = np.random.default_rng(3)
    add("real1_skip", real[1]["lfr"]["Tcw"], real[1]["LP"], 1,
        skip=(rng.uniform(size=len(real[1]["LP"])) < 0.4).astype(np.uint8))
    zero = dict(kfs[0], desc=np.zeros_like(kfs[0]["desc"]))
    kfs.append(zero)  # equal descriptors: the scan order decides
    Pz = q["LP"][:150].copy()
    Pz["desc"] = 0
    add("ties_all_zero", q["lfr"]["Tcw"], Pz, len(kfs) - 1, th=30.0)
    kfs.append(make_keyframe([], geo))
    add("keyframe_without_keypoints", q["lfr"]["Tcw"], q["LP"][:70], len(kfs) - 1)

    # ---- statuses, by construction (Tcw = identity)
    kfs.append(make_keyframe([(320.0, 240.0, 0, -1.0, None), (100.0, 100.0, 0, -1.0, None)], geo))
    k_st = len(kfs) - 1
    head_on = np.array([0, 0, 1], np.float32)
    x_max = x_with_u(geo, _f(640.0))
    x_in = x_with_u(geo, np.nextafter(_f(640.0), _f(0.0)))
    P = [raw_point([0.1, 0.0, -1.0], head_on, 0.1, 9.0),                  # 0 z < 0
         raw_point([0.1, 0.0, 0.0], head_on, 0.1, 9.0),                   # 1 z == 0: u = +inf
         raw_point([0.0, 0.0, 0.0], head_on, 0.1, 9.0),                   # 2 z == 0, X == 0: u = NaN
         raw_point([-0.1, 0.1, -0.0], head_on, 0.1, 9.0),                 # 3 z == -0.0f: not < 0, u = +-inf
         raw_point([x_max, 0.0, 2.0], [x_max, 0.0, 2.0], 0.1, 9.0),       # 4 u == max_x: outside (half open)
         raw_point([x_in, 0.0, 2.0], [x_in, 0.0, 2.0], 0.1, 9.0),         # 5 one float inside: goes on
         raw_point([0.0, 0.0, 2.0], head_on, 2.6, 9.0),                   # 6 too near: 2 < 0.8 * 2.6
         raw_point([0.0, 0.0, 2.0], head_on, 0.1, 1.6),                   # 7 too far: 2 > 1.2 * 1.6
         raw_point([0.0, 0.0, 2.0], [0, 0, 0.5], 0.1, 2.0),               # 8 PO.Pn == 0.5 * dist: not less, goes on
         raw_point([0.0, 0.0, 2.0], [0, 0, np.nextafter(_f(0.5), _f(0))], 0.1, 2.0),   # 9 one float less: view angle
         point_at(geo, 500.0, 400.0),                                     # 10 an empty window
         point_at(geo, 320.4, 240.3)]                                     # 11 searched
    add("statuses", EYE, stack(P), k_st)

    # ---- windows clipped at the grid's first and last columns and rows; a wide window of many cells
    corner = [(2.0, 2.0), (637.5, 2.5), (3.0, 477.0), (638.0, 478.0), (320.0, 1.0), (1.0, 240.0)]
    kp = []
    for n, (x, y) in enumerate(corner):
        kp += [(x, y, 0, -1.0, bits(8)), (x + 1.0, y + 0.5, 0, -1.0, bits(3)), (x - 1.5, y + 1.0, 1, -1.0, bits(5))]
    kfs.append(make_keyframe(kp, geo))
    for th in (3.0, 30.0):
        add(f"clipped_th{int(th)}", EYE, stack([point_at(geo, x + 0.3, y + 0.2, level=lv)
                                               for x, y in corner for lv in (0, 1)]), len(kfs) - 1, th=th)

    # ---- the chi-square tests, the stereo boundary, the levels
    u0, v0, z0 = 300.0, 200.0, 2.0
    pt = point_at(geo, u0, v0, z=z0)
    _, u, v, urp = FR.projection(geo, pt["xw"][0], pt["xw"][1], pt["xw"][2])
    u, v, urp = float(u), float(v), float(urp)
    # stereo: the nearest descriptor 2.5 / 2.0 px off (e2 = 10.25 > 7.8), the second one 0.5 px off
    kfs.append(make_keyframe([(u + 2.5, v + 2.0, 0, urp, bits(1)), (u + 0.5, v, 0, urp + 0.25, bits(20))], geo))
    add("chi2_stereo_second_wins", EYE, stack([pt]), len(kfs) - 1)
    # monocular (uright = -1): 2.0 / 1.5 px off (e2 = 6.25 > 5.99; it would pass 7.8)
    kfs.append(make_keyframe([(u + 2.0, v + 1.5, 0, -1.0, bits(1)), (u + 0.5, v, 0, -1.0, bits(20))], geo))
    add("chi2_mono_second_wins", EYE, stack([pt]), len(kfs) - 1)
    # uright == 0.0f exactly is a stereo keypoint here: er = ur, far above 7.8; with `> 0` it would be accepted
    kfs.append(make_keyframe([(u + 0.5, v, 0, 0.0, bits(2))], geo))
    add("uright_zero_is_stereo", EYE, stack([pt]), len(kfs) - 1)
    # octaves level - 2 .. level + 1 around a level-2 point: the best descriptors are outside [level - 1, level]
    p2 = point_at(geo, u0, v0, z=z0, level=2)
    kfs.append(make_keyframe([(u + 0.5, v, 3, -1.0, bits(1)), (u - 0.5, v, 0, -1.0, bits(2)),
                              (u, v + 0.5, 2, -1.0, bits(30)), (u, v - 0.5, 1, -1.0, bits(25))], geo))
    add("levels", EYE, stack([p2]), len(kfs) - 1)
    return kfs, problems


def reference(problem, kfs, geo, traces=None):
    k = kfs[problem["kf"]]
    return FR.snapshot_search(problem["Tcw"], problem["P"], k["kun"], k["desc"], k["ur"], k["go"], k["gi"], geo,
                              problem["th"], problem["skip"], traces)


def geo():
    return real_problems()[0]["geo"]


# ---------------------------------------------------------------- a second camera: distortion-shifted bounds
DISTORTED = (-0.1, 0.02, 0.0, 0.0, 0.0)  # k1, k2, p1, p2, k3: ComputeImageBounds gives non-integer bounds


@functools.lru_cache(maxsize=None)
def build_distorted():
    """(geo, keyframes, problems) for synth.TUM3 with DISTORTED.  The Frame's bounds are about [-18.84, 658.82] x
    [-14.58, 493.07]; the KeyFrame's are ints, [-18, 658] x [-14, 493] (KeyFrame.cc:41).  Points 0-3 project
    between the two readings on each side; points 4 and 5 are searched in the grid's first and last cells."""
    import oracle_frame
    import synth
    K = synth.TUM3
    b = oracle_frame.frame_rgbd(np.array([[100.0, 100.0]], np.float32), np.ones((480, 640), np.float32), K["fx"],
                                K["fy"], K["cx"], K["cy"], dist=DISTORTED, bf=K["bf"])["bounds"]
    g = np.array(geo(), np.float32)
    g[5:9] = b
    g[9], g[10] = _f(64) / _f(b[1] - b[0]), _f(48) / _f(b[3] - b[2])
    kf = make_keyframe([(-17.0, -13.0, 0, -1.0, bits(4)), (-16.0, -12.5, 0, -1.0, bits(2)),
                        (650.0, 485.0, 0, -1.0, bits(3)), (649.0, 484.5, 1, -1.0, bits(1))], g)
    P = stack([point_at(g, -18.5, 100.0), point_at(g, 658.5, 100.0), point_at(g, 100.0, -14.3),
               point_at(g, 100.0, 493.03), point_at(g, -17.4, -13.2), point_at(g, 650.3, 485.2)])
    return g, [kf], [dict(name="distorted_bounds", Tcw=EYE, P=P, kf=0, th=3.0, skip=None)]
