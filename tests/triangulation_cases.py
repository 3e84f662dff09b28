"""The cases of the CreateNewMapPoints tests (tests/test_triangulation_host.py guards what each reaches,
tests/test_gpu_triangulation.py runs them on the device).

Real keyframes: bow_common.frames() at nfeatures = 200 (frames 0, 3, 20, 40 of two synthetic sequences), the in-repo
vocab_k6_l6 vocabulary, the true poses of synth.Scene, depths from the rendered depth through the frame oracle.
Hand-built keyframes: a few keypoints each, the FeatureVector given directly (a node per group of features), made so
that single candidates sit on each side of every test of ORBmatcher.cc:657-823 and LocalMapping.cc:298-443.

A search case: dict(name, kf1, kf2, F12, only_stereo, check_orientation).
A triangulation case: dict(name, kf1, kf2, match12, want = the status it is there for).
The camera is synth.TUM3 without distortion; `keys` differs from `kun` only where a case says so.
"""
import functools

import numpy as np

import bow_common as BC
import triangulation_ref as TR
from matcher_ref import f32 as _f

GROUP = 8          # kTriGroup of triangulation_search_kernel: lanes per key-1 feature
STEP = 20          # frame step of the real pairs: the baseline (0.08 m) is above mb = bf/fx (0.075 m), and both the
                   # SVD and the UnprojectStereo source occur
SEQS = (0, 2)      # the sequences whose pairs give >= 20 matches at 200 features
LIST_LENGTHS = (0, 1, GROUP - 1, GROUP, GROUP + 1, 64, 65)


@functools.lru_cache(maxsize=None)
def cam():
    import synth
    K = synth.TUM3
    s, scale = _f(1.0), []
    for _ in range(8):                                              # ORBextractor.cc:415-423 (double scaleFactor)
        scale.append(s)
        s = _f(float(s) * float(_f(1.2)))
    return TR.camera(K["fx"], K["fy"], K["cx"], K["cy"], K["bf"], scale)


def Kmat():
    c = cam()
    return np.array([[c["fx"], 0, c["cx"]], [0, c["fy"], c["cy"]], [0, 0, 1]], np.float32)


def bits(n_set):
    """A descriptor with the first n_set bits set: distance n_set to the zero descriptor."""
    d = np.zeros(256, np.uint8)
    d[:n_set] = 1
    return np.packbits(d)


def pose(t=(0, 0, 0), R=None):
    T = np.eye(4, dtype=np.float32)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = t
    return T


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def project(T, X):
    """Pixel and depth of the world point X in the camera T (float64; the keypoints are test inputs)."""
    c = cam()
    p = np.asarray(T, np.float64)[:3, :3] @ np.asarray(X, np.float64) + np.asarray(T, np.float64)[:3, 3]
    return float(c["fx"]) * p[0] / p[2] + float(c["cx"]), float(c["fy"]) * p[1] / p[2] + float(c["cy"]), p[2]


def ray_point(T, x, y, depth):
    """The world point at `depth` on the ray of pixel (x, y) of camera T."""
    c = cam()
    pc = np.array([(x - float(c["cx"])) / float(c["fx"]) * depth, (y - float(c["cy"])) / float(c["fy"]) * depth, depth])
    T = np.asarray(T, np.float64)
    return T[:3, :3].T @ (pc - T[:3, 3])


class Hand:
    """A hand-built keyframe: add(...) rows, then build()."""

    def __init__(self, Tcw):
        self.T = np.asarray(Tcw, np.float32)
        self.rows = []

    def add(self, x, y, node, desc=None, octave=0, ur=-1.0, depth=-1.0, angle=0.0, has=0, key_xy=None):
        self.rows.append(dict(x=x, y=y, node=node, desc=bits(0) if desc is None else desc, octave=octave, ur=ur,
                              depth=depth, angle=angle, has=has, key_xy=(x, y) if key_xy is None else key_xy))
        return len(self.rows) - 1

    def add_stereo(self, x, y, node, depth, **kw):
        """A keypoint with a depth: mvuRight = x - mbf/depth (Frame.cc:760)."""
        return self.add(x, y, node, ur=float(_f(x) - cam()["bf"] / _f(depth)), depth=depth, **kw)

    def build(self):
        import spslam_gpu
        n = len(self.rows)
        kun = np.zeros(n, spslam_gpu.KEYPOINT_DTYPE)
        keys = np.zeros(n, spslam_gpu.KEYPOINT_DTYPE)
        desc = np.zeros((n, 32), np.uint8)
        ur, depth, has = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
        by_node = {}
        for i, r in enumerate(self.rows):
            kun[i]["x"], kun[i]["y"], kun[i]["octave"], kun[i]["angle"] = r["x"], r["y"], r["octave"], r["angle"]
            keys[i] = kun[i]
            keys[i]["x"], keys[i]["y"] = r["key_xy"]
            desc[i], ur[i], depth[i], has[i] = r["desc"], r["ur"], r["depth"], r["has"]
            if r["node"] is not None:
                by_node.setdefault(r["node"], []).append(i)
        nodes = sorted(by_node)
        fv = dict(nodes=np.array(nodes, np.uint32),
                  start=np.cumsum([0] + [len(by_node[k]) for k in nodes]).astype(np.int32),
                  features=np.array([i for k in nodes for i in by_node[k]], np.int32))
        return dict(keys=keys, kun=kun, ur=ur, depth=depth, desc=desc, has=has, fv=fv, Tcw=self.T,
                    Ow=TR.camera_centre(self.T))


# the two hand geometries: G has its epipole inside the second image, X (a pure x translation) has C2.z == 0
T_G = pose((0.1, 0.05, 0.5))
T_X = pose((-0.2, 0.0, 0.0))


def on_line(T2, x1, y1, depth):
    """The pixel in camera T2 of the point at `depth` on the ray of (x1, y1) of the identity camera: a point of
    that keypoint's epipolar line."""
    return project(T2, ray_point(pose(), x1, y1, depth))[:2]


def off_line(T2, x1, y1, depth, delta):
    """on_line moved by delta pixels along the line's normal."""
    (xa, ya), (xb, yb) = on_line(T2, x1, y1, depth), on_line(T2, x1, y1, depth * 1.5)
    n = np.array([-(yb - ya), xb - xa])
    n /= np.linalg.norm(n)
    return xa + delta * n[0], ya + delta * n[1]


def search_case(name, h1, h2, only_stereo=0, check_orientation=0, F12=None):
    kf1, kf2 = h1.build(), h2.build()
    F = TR.compute_f12(kf1, kf2, Kmat()) if F12 is None else np.asarray(F12, np.float32)
    return dict(name=name, kf1=kf1, kf2=kf2, F12=F, only_stereo=only_stereo, check_orientation=check_orientation)


def _lists_case():
    """Node key-2 lists of every length in LIST_LENGTHS: candidate j of a list has distance 10 + (7 j mod 13), so the
    minimum recurs (the later one wins) and sits in different lanes of the group."""
    h1, h2 = Hand(pose()), Hand(T_G)
    for k, L in enumerate(LIST_LENGTHS):
        x1, y1 = 100.0 + 60 * k, 120.0 + 30 * k
        h1.add_stereo(x1, y1, 100 + k, 2.0)
        for j in range(L):
            x2, y2 = on_line(T_G, x1, y1, 1.5 + 0.02 * j)
            h2.add_stereo(x2, y2, 100 + k, 2.0, desc=bits(10 + (7 * j) % 13))
    h2.add_stereo(10.0, 10.0, 99, 2.0)                              # so that key 2 is not empty when L = 0 only
    return search_case("lists", h1, h2)


def _ties_thresholds_has_case():
    h1, h2 = Hand(pose()), Hand(T_G)
    # 0: two candidates tie, both pass: the later wins.  1: the later fails the epipolar test: the earlier is kept
    for k, late_delta in enumerate((0.0, 6.0)):
        x1, y1 = 150.0 + 100 * k, 200.0
        h1.add_stereo(x1, y1, 10 + k, 2.0)
        h2.add_stereo(*on_line(T_G, x1, y1, 1.8), 10 + k, 2.0, desc=bits(12))
        h2.add_stereo(*off_line(T_G, x1, y1, 2.2, late_delta), 10 + k, 2.0, desc=bits(12))
    # 2, 3: distances of exactly 50 and 51
    for k, d in enumerate((50, 51)):
        x1, y1 = 200.0 + 50 * k, 300.0
        h1.add_stereo(x1, y1, 20 + k, 2.0)
        h2.add_stereo(*on_line(T_G, x1, y1, 2.0), 20 + k, 2.0, desc=bits(d))
    # 4: key 1 holds a point (skipped).  5: key 2's nearest candidate holds a point: the next one is taken
    h1.add_stereo(400.0, 100.0, 30, 2.0, has=1)
    h2.add_stereo(*on_line(T_G, 400.0, 100.0, 2.0), 30, 2.0)
    h1.add_stereo(450.0, 150.0, 31, 2.0)
    h2.add_stereo(*on_line(T_G, 450.0, 150.0, 2.0), 31, 2.0, desc=bits(3), has=1)
    h2.add_stereo(*on_line(T_G, 450.0, 150.0, 2.1), 31, 2.0, desc=bits(30))
    # 6, 7: two key-1 features on one pixel take the same idx2; key 2 sees the point at its true depth, so that both
    # matches are accepted and the second AddMapPoint overwrites the first
    for _ in range(2):
        h1.add_stereo(500.0, 350.0, 40, 2.0)
    x2, y2, z2 = project(T_G, ray_point(pose(), 500.0, 350.0, 2.0))
    h2.add_stereo(x2, y2, 40, z2, desc=bits(4))
    return search_case("ties_thresholds_has", h1, h2)


def epipole_G():
    kf1, kf2 = Hand(pose()).build(), Hand(T_G).build()
    return TR.epipole(kf1, kf2, cam())


def _epipole_case():
    """Mono-mono candidates 20, exactly 10 and 5 pixels from the epipole on one epipolar line (100*scale = 100 at
    octave 0): the nearest descriptor is inside and skipped, the one on the radius is not (`<`)."""
    ex, ey = epipole_G()
    h1, h2 = Hand(pose()), Hand(T_G)
    far = (float(ex) - 60.0, float(ey) - 80.0)
    x1, y1, _ = project(pose(), ray_point(T_G, far[0], far[1], 2.0))
    h1.add(x1, y1, 5)
    h2.add(float(_f(ex - _f(12.0))), float(_f(ey - _f(16.0))), 5, desc=bits(20))
    h2.add(float(_f(ex - _f(6.0))), float(_f(ey - _f(8.0))), 5, desc=bits(10))
    h2.add(float(_f(ex - _f(3.0))), float(_f(ey - _f(4.0))), 5, desc=bits(5))
    # the same three as a stereo key-1 feature sees them: no epipole test, the nearest descriptor wins
    h1.add_stereo(x1, y1, 5, 2.0)
    return search_case("epipole_radius", h1, h2)


def _octaves_case():
    """Per octave a candidate just inside and one just outside 3.84*sigma2 of the line; the outside one has the
    nearer descriptor."""
    c = cam()
    h1, h2 = Hand(pose()), Hand(T_G)
    for o in range(8):
        x1, y1 = 80.0 + 60 * o, 150.0 + 20 * o
        h1.add_stereo(x1, y1, 50 + o, 2.0)
        lim = np.sqrt(3.84 * float(c["sigma2"][o]))
        h2.add_stereo(*off_line(T_G, x1, y1, 2.0, 0.97 * lim), 50 + o, 2.0, desc=bits(20), octave=o)
        h2.add_stereo(*off_line(T_G, x1, y1, 2.0, 1.03 * lim), 50 + o, 2.0, desc=bits(5), octave=o)
    return search_case("octaves", h1, h2)


def _c2z_zero_case(zero_F=False):
    h1, h2 = Hand(pose()), Hand(T_X)
    for k in range(6):                                              # mono-mono: the epipole test runs on inf / NaN
        x1, y1 = 120.0 + 70 * k, 100.0 + 40 * k
        h1.add(x1, y1, 7)
        h2.add(*on_line(T_X, x1, y1, 2.0), 7, desc=bits(k))
    return search_case("zero_F12" if zero_F else "c2z_zero", h1, h2, F12=np.zeros(9) if zero_F else None)


def _stereo_mix_case(only_stereo):
    h1, h2 = Hand(pose()), Hand(T_G)
    for k in range(8):
        x1, y1 = 100.0 + 50 * k, 90.0 + 45 * k
        (h1.add_stereo(x1, y1, 3, 2.0) if k % 2 else h1.add(x1, y1, 3))
        x2, y2 = on_line(T_G, x1, y1, 2.0)
        (h2.add_stereo(x2, y2, 3, 2.0, desc=bits(k)) if k % 4 < 2 else h2.add(x2, y2, 3, desc=bits(k)))
    return search_case(f"stereo_mix_only{only_stereo}", h1, h2, only_stereo=only_stereo)


def _orientation_case(name, bins):
    """bins: {rotation bin: number of matches}; every match is its own node."""
    h1, h2 = Hand(pose()), Hand(T_G)
    k = 0
    for b, count in bins.items():
        for _ in range(count):
            x1, y1 = 60.0 + 11 * k, 60.0 + 7 * k
            h1.add_stereo(x1, y1, 200 + k, 2.0, angle=30.0 * b + 5.0)
            h2.add_stereo(*on_line(T_G, x1, y1, 2.0), 200 + k, 2.0, angle=5.0 if k % 2 else 4.0)
            k += 1
    return search_case(name, h1, h2, check_orientation=1)


def _degenerate_cases():
    out = []
    full = _lists_case()
    a = dict(full, name="all_key1_hold_points", kf1=dict(full["kf1"], has=np.ones(len(full["kf1"]["kun"]), np.uint8)))
    out.append(a)
    empty = Hand(pose()).build()
    out.append(dict(full, name="key1_empty", kf1=empty))
    out.append(dict(full, name="key2_empty", kf2=dict(empty, Tcw=full["kf2"]["Tcw"], Ow=full["kf2"]["Ow"])))
    h1, h2 = Hand(pose()), Hand(T_G)
    for k in range(3):
        h1.add_stereo(100.0 + k, 100.0, None, 2.0)                  # features, but no FeatureVector entry
        h2.add_stereo(100.0 + k, 100.0, None, 2.0)
    out.append(search_case("empty_feature_vectors", h1, h2))
    h1, h2 = Hand(pose()), Hand(T_G)
    for k in range(4):
        h1.add_stereo(100.0 + 40 * k, 100.0, 2 * k, 2.0)
        h2.add_stereo(*on_line(T_G, 100.0 + 40 * k, 100.0, 2.0), 2 * k + 1, 2.0)
    out.append(search_case("disjoint_feature_vectors", h1, h2))
    return out


# ---------------------------------------------------------------- real keyframes
@functools.lru_cache(maxsize=None)
def real_keyframes():
    """{(seq, frame): keyframe} for frames 0, 3, STEP, 2*STEP of the sequences SEQS."""
    import oracle_ctypes
    import oracle_frame
    import synth
    K = synth.TUM3
    voc = BC.PyVocab(BC.vocab_text())
    orb = oracle_ctypes.OrbOracle(nfeatures=200)
    out = {}
    for seq in SEQS:
        sc = synth.Scene(seq, n_boxes=3)
        for fi in (0, 3, STEP, 2 * STEP):
            Twc = sc.pose(fi)
            g, d16, _ = sc.render(Twc, noise_seed=fi)               # bow_common.frames()' frames
            kp, desc = orb.extract(g)
            depth = d16.astype(np.float32) * _f(_f(1.0) / _f(5000.0))
            fo = oracle_frame.frame_rgbd(np.stack([kp["x"], kp["y"]], 1), depth, K["fx"], K["fy"], K["cx"], K["cy"],
                                         bf=K["bf"])
            kun = kp.copy()
            kun["x"], kun["y"] = fo["un"][:, 0], fo["un"][:, 1]
            Tcw = np.linalg.inv(Twc).astype(np.float32)
            fv = voc.transform(desc)
            out[(seq, fi)] = dict(keys=kp, kun=kun, ur=fo["uright"], depth=fo["depth"], desc=desc,
                                  has=np.zeros(len(kp), np.uint8),
                                  fv=dict(nodes=fv["nodes"], start=fv["start"], features=fv["features"]), Tcw=Tcw,
                                  Ow=TR.camera_centre(Tcw), depth_map=depth)
    return out


def real_search_cases():
    kfs = real_keyframes()
    out = []
    for seq in SEQS:
        kf1, kf2 = kfs[(seq, 0)], kfs[(seq, STEP)]
        F = TR.compute_f12(kf1, kf2, Kmat())
        out.append(dict(name=f"real{seq}", kf1=kf1, kf2=kf2, F12=F, only_stereo=0, check_orientation=0))
    out.append(dict(out[0], name="real0_orientation", check_orientation=1))
    out.append(dict(out[1], name=f"real{SEQS[1]}_only_stereo", only_stereo=1))
    return out


@functools.lru_cache(maxsize=None)
def search_cases():
    out = [_lists_case(), _ties_thresholds_has_case(), _epipole_case(), _octaves_case(), _c2z_zero_case(),
           _c2z_zero_case(zero_F=True), _stereo_mix_case(0), _stereo_mix_case(1),
           _orientation_case("orientation_bins_removed", {0: 10, 3: 5, 7: 3, 11: 2}),
           _orientation_case("orientation_second_below_tenth", {0: 21, 5: 2, 9: 1})]
    return out + _degenerate_cases() + real_search_cases()


# ---------------------------------------------------------------- triangulation cases
def _tri(name, want, source, h1, h2, match12, patch=None):
    kf1, kf2 = h1.build(), h2.build()
    case = dict(name=name, want=want, source=source, kf1=kf1, kf2=kf2, match12=np.array(match12, np.int32))
    if patch:
        patch(case)
    return case


def _pair_of(X, T2, stereo1, stereo2, dy2=0.0, dx2=0.0, octave1=0, octave2=0, key_off=(0.0, 0.0)):
    """One keypoint per keyframe observing the world point X from the identity camera and from T2."""
    h1, h2 = Hand(pose()), Hand(T2)
    for h, T, st, dx, dy, o, ko in ((h1, pose(), stereo1, 0.0, 0.0, octave1, key_off),
                                    (h2, T2, stereo2, dx2, dy2, octave2, (0.0, 0.0))):
        x, y, z = project(T, X)
        x, y = x + dx, y + dy
        if st:
            h.add_stereo(x, y, 1, z, octave=o, key_xy=(x + ko[0], y + ko[1]))
        else:
            h.add(x, y, 1, octave=o)
    return h1, h2


def _zero_dist_patch(case):
    """Ow1 := the point KeyFrame 2 unprojects, so that dist1 == 0 while z1 > 0 (Ow is an input of its own)."""
    case["kf1"] = dict(case["kf1"], Ow=np.array(TR.unproject_stereo(case["kf2"], 0, cam()), np.float32))


def _right_error_patch(case):
    """The neighbour's right-image coordinate off by four pixels: only the three-term error sees it."""
    case["kf2"]["ur"][0] += _f(4.0)


@functools.lru_cache(maxsize=None)
def triangulation_cases():
    N, S = TR, TR
    X = np.array([0.3, -0.2, 2.0])
    wide, narrow = pose((-0.3, 0.0, 0.0)), pose((-0.02, 0.0, 0.0))
    sheared = pose((0.3, 0.1, 0.0), R=np.array([[1, 0, 0], [0, 1, 0], [0.5, 0, 1.0]]))
    out = [
        _tri("new_svd_mono_mono", N.NEW, S.FROM_SVD, *_pair_of(X, wide, False, False), [0]),
        _tri("new_svd_stereo_stereo", N.NEW, S.FROM_SVD, *_pair_of(X, wide, True, True), [0]),
        _tri("new_svd_mono_stereo", N.NEW, S.FROM_SVD, *_pair_of(X, wide, False, True), [0]),
        _tri("new_stereo1", N.NEW, S.FROM_STEREO_1, *_pair_of(X, narrow, True, False), [0]),
        _tri("new_stereo1_both_stereo", N.NEW, S.FROM_STEREO_1, *_pair_of(X, narrow, True, True), [0]),
        _tri("new_stereo2", N.NEW, S.FROM_STEREO_2, *_pair_of(X, narrow, False, True), [0]),
        _tri("new_stereo1_distorted_keys", N.NEW, S.FROM_STEREO_1,
             *_pair_of(X, narrow, True, False, key_off=(1.0, -1.0)), [0]),
        _tri("low_parallax", N.LOW_PARALLAX, S.FROM_SVD, *_pair_of(X, narrow, False, False), [0]),
        _tri("rays_apart_cos_negative", N.LOW_PARALLAX, S.FROM_SVD,
             *_pair_of(np.array([0.0, 0.0, 1.0]), pose((0.0, 0.0, 1.5), R=rot_y(np.pi * 0.75)), False, False), [0]),
        _tri("behind_1", N.BEHIND_1, S.FROM_SVD, *_pair_of(X, wide, False, False, dx2=160.0), [0]),
        _tri("behind_2", N.BEHIND_2, S.FROM_STEREO_1,
             *_pair_of(np.array([0.0, 0.0, 1.0]), pose((0.0, 0.0, -2.0)), True, False), [0]),
        _tri("reproj_1", N.REPROJ_1, S.FROM_SVD, *_pair_of(X, wide, False, False, dy2=10.0), [0]),
        _tri("reproj_2", N.REPROJ_2, S.FROM_STEREO_1, *_pair_of(X, narrow, True, False, dy2=10.0), [0]),
        _tri("reproj_2_stereo_right_error", N.REPROJ_2, S.FROM_STEREO_1, *_pair_of(X, narrow, True, True), [0],
             patch=_right_error_patch),
        _tri("zero_dist", N.ZERO_DIST, S.FROM_STEREO_2, *_pair_of(X, narrow, False, True), [0],
             patch=_zero_dist_patch),
        _tri("scale", N.SCALE, S.FROM_SVD, *_pair_of(X, wide, False, False, octave1=7, octave2=0), [0]),
    ]
    # x3D(3) == 0: kp1 and kp2 on the principal point, Tcw2 sheared (not a rigid motion) so that the rays still
    # differ: the z column of A is exactly zero, A has rank 3 and its null vector is (0, 0, 1, 0)
    c = cam()
    h1, h2 = Hand(pose()), Hand(sheared)
    h1.add(float(c["cx"]), float(c["cy"]), 1)
    h2.add(float(c["cx"]), float(c["cy"]), 1)
    out.append(_tri("w_zero_rank_deficient", N.W_ZERO, S.FROM_SVD, h1, h2, [0]))
    # an A that needs the sweep limit: translations near FLT_MAX make xn*Tcw(2,3) - Tcw(k,3) overflow to +inf in
    # row 0 and -inf in row 1; the rays depend on the rotation only, so the match passes the parallax test and
    # reaches the SVD; inf - inf makes a NaN dot product, |p| <= eps*sqrt(a*b) is false on every pair from then on,
    # and all 30 sweeps run.  The null vector is NaN, every later comparison is false, and the reference's code
    # accepts the match with a NaN point.  With one overflowing row only, the inf column is never rotated
    # (|inf| <= inf skips it), the Jacobi ends after 4 sweeps and x3D(3) is exactly 0.
    for name, t, want in (("sweep_limit_overflowing_translation", (-3.2e38, 3.2e38, 3.2e38), N.NEW),
                          ("w_zero_one_overflowing_row", (-3.2e38, 0.0, 3.2e38), N.W_ZERO)):
        h1, h2 = _pair_of(X, wide, False, False)
        h1.T = pose(t)
        out.append(_tri(name, want, S.FROM_SVD, h1, h2, [0]))
    # a keyframe of several matches and non-matches, cap-straddling in the GPU test
    h1, h2 = Hand(pose()), Hand(wide)
    m = []
    rng = np.random.default_rng(3)
    for k in range(70):
        P = np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.5, 0.5), rng.uniform(1.0, 4.0)])
        x1, y1, z1 = project(pose(), P)
        x2, y2, z2 = project(wide, P)
        x2, y2 = x2 + rng.normal(0, 0.7), y2 + rng.normal(0, 0.7)
        (h1.add_stereo(x1, y1, 1, z1, octave=k % 4) if k % 3 else h1.add(x1, y1, 1, octave=k % 4))
        (h2.add_stereo(x2, y2, 1, z2, octave=k % 4) if k % 2 else h2.add(x2, y2, 1, octave=k % 4))
        m.append(-1 if k % 7 == 6 else k)
    out.append(_tri("mixed_70", None, None, h1, h2, m))
    return out


# ---------------------------------------------------------------- chained rounds
def chained_model(seq):
    """Keyframe 0 of a sequence with the neighbours [STEP, 3 (below the baseline), 2*STEP]; a seventh of every
    keyframe's keypoints already hold a map point."""
    kfs = real_keyframes()
    rng = np.random.default_rng(40 + seq)
    model = dict(kfs={}, points={})
    for fi in (0, STEP, 3, 2 * STEP):
        kf = dict(kfs[(seq, fi)])
        kf["points"] = {}
        for i in np.flatnonzero(rng.uniform(size=len(kf["kun"])) < 0.15):
            pid = len(model["points"])
            model["points"][pid] = dict(x3D=None, obs={fi: int(i)})
            kf["points"][int(i)] = pid
        kf["has"] = np.array([i in kf["points"] for i in range(len(kf["kun"]))], np.uint8)
        model["kfs"][fi] = kf
    return model, 0, [STEP, 3, 2 * STEP]
