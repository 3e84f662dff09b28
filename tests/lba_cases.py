"""The cases of the LocalBundleAdjustment structure tests (tests/test_oracle_lba_cases.py shows on the CPU what each
reaches, tests/test_gpu_lba_geometry.py runs them on the device): local windows whose structure is given, not sampled.

Geometry: cameras on a gently curving line (6 cm apart, a slow yaw and drift), looking at a wall 4 m away and at the
floor below it; every point lies in front of every camera, so a point can be given to any set of observers
(LocalBundleAdjustment has no image-bounds check).  Observations are the exact projections of the ground truth plus
seeded pixel noise, stereo and mono mixed; free poses, points and planes start perturbed as synth.lba_problem perturbs
them.  A case names its keyframes (which are fixed, their ids) and, per point, the keyframes that observe it: the
coupling pattern of the free poses is realised exactly.

Patterns over the free poses (by their rank in list order): `full`, `band(r)` (observers within r of a point's first
observer), `band(r)+hub` (the last pose also sees one point of every other pose: the current keyframe of a real window),
`two` (two components, block diagonal), `alld` (a band so wide that every scalar passes Eigen's dense-row threshold
while the end poses stay uncoupled).

A case is dict(name, P, want): P is synth.lba_problem's tuple (problem, keyframes, points, point_obs, planes,
plane_obs, ground truth); want holds what the case was built to reach (free poses `np`, class `cls` in
{"dense", "alld", "amd"}, the instance `pw`, and the tags the CPU file asserts).  The kernel's size constants below
(sp-slam_amd/csrc/lba_g2o.hip, lbg_factor.h) name the branch a case reaches; none of them is a tolerance."""
import functools

import numpy as np

K_T = 512                       # kT: threads, the chunk of every block scan over landmarks or edges
K_LDS_N = {1: 96, 2: 90}        # kLdsN per instance: reduced systems factorised in LDS
K_PACK_N = 180                  # kPackN: dense systems factorised with L packed in LDS
K_DYN = 136 * 1024              # kDyn: dynamic LDS (the AMD workspace lives there while it fits)
K_SCHUR_LM = 64                 # kSchurLm: landmarks per Schur chunk
K_SCHUR_BLK = {1: 412, 2: 360}  # kSchurBlk per instance: Hpl blocks staged per Schur chunk
K_TILE = K_DYN // 4             # setup()'s LDS tile of ids in the rank counting
K_MAX_FREE = 64                 # windows of more keyframes than this run the wide instance (two-word pose masks)

# world planes (a, b, c, d), d >= 0 as the reference signs them, and the axis of each normal
PLANES = {"wall": (np.array([0.0, 0.0, -1.0, 4.0]), 2), "floor": (np.array([0.0, -1.0, 0.0, 1.2]), 1),
          "ceil": (np.array([0.0, 1.0, 0.0, 1.5]), 1), "side": (np.array([1.0, 0.0, 0.0, 3.0]), 0)}


def rig(n_kf):
    """Ground-truth Tcw of n_kf cameras along the line."""
    T = np.zeros((n_kf, 4, 4))
    for k in range(n_kf):
        c = np.array([0.06 * k, 0.03 * np.sin(0.21 * k), 2e-5 * k * k])
        a = 8e-4 * k
        Rwc = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        T[k, :3, :3] = Rwc.T
        T[k, :3, 3] = -Rwc.T @ c
        T[k, 3, 3] = 1.0
    return T


# ---------------------------------------------------------------- patterns (observer ranks per point)
def band(n_free, r, n_pts, lo=0, hi=None):
    hi = n_free if hi is None else hi
    s = hi - lo
    if s == 1:
        return [[lo] for _ in range(n_pts)]
    return [list(range(lo + i % (s - 1), min(lo + i % (s - 1) + r, hi - 1) + 1)) for i in range(n_pts)]


def hub(n_free):
    return [[p, n_free - 1] for p in range(n_free - 1)]


def pattern(kind, n_free, n_pts=None):
    n_pts = max(160, 2 * n_free) if n_pts is None else n_pts
    if kind == "full":
        return band(n_free, 2, n_pts) + [list(range(n_free)) for _ in range(12)]
    if kind.startswith("band"):
        r = int(kind[5:kind.index(")")])
        return band(n_free, r, n_pts) + (hub(n_free) if kind.endswith("+hub") else [])
    if kind == "two":
        m = n_free // 2
        return band(n_free, 3, n_pts // 2, 0, m) + band(n_free, 3, n_pts - n_pts // 2, m, n_free)
    if kind == "alld":
        return band(n_free, alld_reach(n_free), n_pts)
    raise ValueError(kind)


def dense_threshold(n):
    """Eigen's AMD: rows with more entries than this are dense (absorbed last, in index order)."""
    return min(n - 2, max(16, int(10 * np.sqrt(float(n)))))


def alld_reach(n_free):
    """The narrowest band whose end poses (reach + 1 coupled poses, themselves included) pass the dense threshold."""
    r = dense_threshold(6 * n_free) // 6
    assert 6 * (r + 1) > dense_threshold(6 * n_free) and r < n_free - 1
    return r


def expected_pattern(kind, n_free):
    """The coupling pattern (boolean, symmetric, diagonal set) the named pattern stands for."""
    i, j = np.indices((n_free, n_free))
    if kind == "full":
        return np.ones((n_free, n_free), bool)
    if kind == "two":
        m = n_free // 2
        return (np.abs(i - j) <= 3) & ((i < m) == (j < m))
    r = alld_reach(n_free) if kind == "alld" else int(kind[5:kind.index(")")])
    pat = np.abs(i - j) <= r
    if kind.endswith("+hub"):
        pat[n_free - 1, :] = pat[:, n_free - 1] = True
    return pat


# ---------------------------------------------------------------- the builder
def build(name, n_kf, fixed, observers, want, *, seed, ids=None, first_id=1, planes=(), pix_noise=1.0,
          outlier_frac=0.03, stereo_frac=0.7, gross=(), gross_disparity=(), all_gross=False, point_ids=None,
          on_floor=None):
    """observers: per point the keyframes (list indices) that see it, first observer first.  planes: (name, keyframes)
    pairs -- each keyframe gets the plane's observation edge, then vertical and parallel edges to the other planes of
    the case.  gross: (point, keyframe) observations moved far off; gross_disparity: stereo observations whose right
    coordinate lies right of the left one (no pose in front of which the point lies can explain it); all_gross: every
    observation a random pixel."""
    import spslam_lba as L
    import synth
    rng = np.random.default_rng(seed)
    K = synth.TUM3
    fx, fy, cx, cy, bf = K["fx"], K["fy"], K["cx"], K["cy"], K["bf"]
    gt = rig(n_kf)
    fixed = set(fixed)
    kfs = np.zeros(n_kf, L.LBA_KEYFRAME_DTYPE)
    for k in range(n_kf):
        T = gt[k].copy()
        if k not in fixed:
            T[:3, :3] = synth._rot(rng.normal(0, np.deg2rad(0.4), 3)) @ T[:3, :3]
            T[:3, 3] = T[:3, 3] + rng.normal(0, 0.02, 3)
        kfs[k]["Tcw"] = T.astype(np.float32).ravel()
        kfs[k]["fx"], kfs[k]["fy"], kfs[k]["cx"], kfs[k]["cy"], kfs[k]["bf"] = fx, fy, cx, cy, bf
        kfs[k]["id"] = first_id + k if ids is None else ids[k]
        kfs[k]["fixed"] = int(k in fixed)
    inv_s2 = np.array([1.0 / (1.2 ** (2 * o)) for o in range(8)])
    gross, gross_disparity = set(gross), set(gross_disparity)
    n_pts = len(observers)
    points = np.zeros(n_pts, L.LBA_POINT_DTYPE)
    n_obs = np.array([len(o) for o in observers], np.int64)
    offs = np.concatenate([[0], np.cumsum(n_obs)]).astype(np.int64)
    pobs = np.zeros(int(offs[-1]), L.LBA_POINT_OBS_DTYPE)
    for i, ob in enumerate(observers):
        ob = np.asarray(ob, np.int64)
        x0 = 0.06 * ob[0] if len(ob) else 0.0
        if (i % 2 == 0) if on_floor is None else not on_floor:
            X = np.array([x0 + rng.uniform(-1.2, 1.2), rng.uniform(-1.0, 1.0), 4.0])
        else:
            X = np.array([x0 + rng.uniform(-1.2, 1.2), 1.2, rng.uniform(2.5, 4.0)])
        points[i]["xw"] = (X + rng.normal(0, 0.02, 3)).astype(np.float32)
        points[i]["id"] = 2000 + 3 * i if point_ids is None else point_ids[i]
        points[i]["obs_offset"], points[i]["n_obs"] = offs[i], len(ob)
        if not len(ob):
            continue
        Xc = gt[ob, :3, :3] @ X + gt[ob, :3, 3]
        assert (Xc[:, 2] > 0.3).all(), (name, i)
        m = len(ob)
        u = fx * Xc[:, 0] / Xc[:, 2] + cx + rng.normal(0, pix_noise, m)
        v = fy * Xc[:, 1] / Xc[:, 2] + cy + rng.normal(0, pix_noise, m)
        out = rng.random(m) < outlier_frac
        if all_gross:
            out[:] = True
        ru, rv = rng.uniform(10, 630, m), rng.uniform(10, 470, m)
        u, v = np.where(out, ru, u), np.where(out, rv, v)
        for j, k in enumerate(ob):
            if (i, int(k)) in gross:
                ang = rng.uniform(0, 2 * np.pi)
                d = rng.uniform(60, 160)
                u[j], v[j] = u[j] + d * np.cos(ang), v[j] + d * np.sin(ang)
        z = Xc[:, 2]
        ur = np.where(rng.random(m) < stereo_frac, u - bf / (z + rng.normal(0, 0.002 * z * z)), -1.0)
        if all_gross:
            ur = np.where(ur >= 0, rng.uniform(10, 630, m), ur)
        for j, k in enumerate(ob):
            if (i, int(k)) in gross_disparity:
                ur[j] = u[j] + rng.uniform(30, 80)
        seg = pobs[offs[i]:offs[i + 1]]
        seg["kf"], seg["u"], seg["v"], seg["ur"] = ob, u, v, ur
        seg["inv_sigma2"] = inv_s2[rng.integers(8, size=m)]
    # planes: observation edges, then vertical, then parallel (Optimizer.cc:1501-1613), as synth.lba_problem
    pl_rows, plo = [], []
    names = [p[0] for p in planes]
    for j, (pname, ks) in enumerate(planes):
        wp, axis = PLANES[pname]
        off = len(plo)
        for kind in (0, 2, 1):
            for k in ks:
                m = pname
                if kind:
                    cand = [q for q in names if q != pname and ((PLANES[q][1] == axis) == (kind == 1))]
                    if not cand or (k + j + kind) % 2:
                        continue
                    m = cand[(k + j) % len(cand)]
                cp = synth.transform_plane(gt[k], PLANES[m][0])
                Rn = synth._rot(rng.normal(0, np.deg2rad(0.5), 3))
                plo.append((k, kind, np.array([*(Rn @ cp[:3]), cp[3] + rng.normal(0, 0.01)]).astype(np.float32)))
        Rn = synth._rot(rng.normal(0, np.deg2rad(0.5), 3))
        wn = np.array([*(Rn @ wp[:3]), wp[3] + rng.normal(0, 0.01)])
        pl_rows.append((wn.astype(np.float32), 900000 + 5 * j, off, len(plo) - off, 0))
    pls = np.array(pl_rows, L.LBA_PLANE_DTYPE) if pl_rows else np.zeros(0, L.LBA_PLANE_DTYPE)
    plobs = np.array(plo, L.LBA_PLANE_OBS_DTYPE) if plo else np.zeros(0, L.LBA_PLANE_OBS_DTYPE)
    prob = np.zeros((), L.LBA_PROBLEM_DTYPE)
    prob["n_kf"], prob["n_points"], prob["n_planes"] = n_kf, n_pts, len(pls)
    prob["n_point_obs"], prob["n_plane_obs"] = len(pobs), len(plobs)
    want = dict(want)
    want.setdefault("pw", 1 if n_kf <= K_MAX_FREE else 2)
    return dict(name=name, P=(prob, kfs, points, pobs, pls, plobs, dict(Tcw=gt)), want=want)


def window(name, n_free, kind, want=None, *, n_fixed=2, n_kf=None, seed=0, n_pts=None, with_planes=True, **kw):
    """n_free free keyframes first, then the fixed ones (n_kf pads the window with further fixed keyframes that see
    nothing); the named pattern over the free poses; every third point is also seen by a fixed keyframe; three planes
    seen by the first free poses within the band."""
    n_kf = n_free + n_fixed if n_kf is None else n_kf
    fixed = list(range(n_free, n_kf))
    obs = pattern(kind, n_free, n_pts)
    if n_fixed:
        obs = [o + [n_free + (i // 3) % n_fixed] if i % 3 == 0 else o for i, o in enumerate(obs)]
    planes = ()
    if with_planes:
        f0 = fixed[:1]
        planes = (("wall", [0, 1] + f0), ("floor", [1, 2] + f0), ("ceil", [0, 2] + f0))
    w = dict(np=n_free, pattern=kind)
    w.update(want or {})
    return build(name, n_kf, fixed, obs, w, seed=seed, planes=planes, **kw)


def pairs(n_free, counts):
    """Observer ranks of points with the given numbers of observations, cycling over the free poses so that every
    pair of poses is coupled."""
    out = []
    for i, c in enumerate(counts):
        a = i % n_free
        step = 1 + (i // n_free) % (n_free - 1)
        out.append([(a + q * step) % n_free for q in range(c)] if c <= 2 else
                   [(a + q) % n_free for q in range(c)])
    return out


def seam_points(name, n_points=None, n_edges=None, want=None, *, n_free=6, n_fixed=2, n_kf=None, seed=0, counts=None,
                **kw):
    """A points-only window of n_points landmarks (two observations each) or of exactly n_edges observations."""
    if counts is None:
        if n_points is not None:
            counts = [2] * n_points
        else:
            counts = [2] * (n_edges // 2 - 1) + [2 + n_edges % 2]
    n_kf = n_free + n_fixed if n_kf is None else n_kf
    obs = pairs(n_free, counts)
    w = dict(np=n_free)
    w.update(want or {})
    return build(name, n_kf, range(n_free, n_kf), obs, w, seed=seed, **kw)


# ---------------------------------------------------------------- the case list
def _specs():
    S = []
    add = lambda name, fn, *a, **kw: S.append((name, functools.partial(fn, name, *a, **kw)))  # noqa: E731
    seed = iter(range(7000, 9000))
    # free-pose seams of the factor dispatch (narrow instance)
    for nf in (10, 11, 16, 17, 21, 22, 30, 31, 32, 33, 42, 43, 64):
        for kind in ("full", "band(2)", "band(3)+hub"):
            cls = "dense" if kind == "full" else "amd"
            add(f"free{nf}-{kind}", window, nf, kind, dict(cls=cls), n_fixed=0 if nf == 64 else 2, seed=next(seed))
    for nf in (25, 62):
        add(f"free{nf}-alld", window, nf, "alld", dict(cls="alld"), seed=next(seed))
    # the wide instance
    for nf in (65, 85, 86, 128):
        for kind in ("band(3)+hub", "two"):
            add(f"wide{nf}-{kind}", window, nf, kind, dict(cls="amd", pw=2), seed=next(seed))
    for nf in (15, 16):
        for kind in ("full", "band(2)"):
            add(f"wide66-free{nf}-{kind}", window, nf, kind, dict(cls="dense" if kind == "full" else "amd", pw=2),
                n_kf=66, seed=next(seed))
    add("wide120-band(8)-amd-global", window, 120, "band(8)", dict(cls="amd", pw=2, amd_global=True), seed=next(seed))
    add("wide128-landmark-of-all", _landmark_of_all, 128, seed=next(seed))
    # structure
    add("ids-permuted", _ids_permuted, seed=next(seed))
    add("fixed-interleaved", _fixed_interleaved, seed=next(seed))
    add("id0-and-fixed-only-points", _id0, seed=next(seed))
    add("free-kf-unobserved", _unobserved, seed=next(seed))
    add("all-fixed", _all_fixed, seed=next(seed))
    add("planes-only", _planes_only, seed=next(seed))
    add("points-only", window, 8, "band(2)", dict(cls="amd"), with_planes=False, seed=next(seed))
    add("one-point", build, 3, [2], [[0, 1, 2]], dict(np=2, cls="dense"), stereo_frac=1.0, outlier_frac=0.0,
        seed=next(seed))
    add("one-plane", build, 3, [2], [], dict(np=2, cls="dense"), planes=(("wall", [0, 1, 2]),), seed=next(seed))
    add("bridge-outlier", _bridge, seed=next(seed))
    add("pose-all-outliers", _pose_outliers, seed=next(seed))
    add("all-outliers", _all_outliers, seed=next(seed))
    # chunk seams
    for n in (511, 512, 513, 1025):
        add(f"landmarks{n}", seam_points, n, None, dict(cls="dense", landmarks=n), seed=next(seed))
    for n in (31, 32, 33, 511, 512, 513):
        add(f"edges{n}", seam_points, None, n, dict(cls="dense", edges=n), n_free=3 if n < 100 else 6,
            seed=next(seed))
    for n in (64, 65, 128, 129):
        add(f"active{n}", seam_points, n, None, dict(cls="dense", landmarks=n), seed=next(seed))
    for pw in (1, 2):
        for extra in (0, 1):
            add(f"schur-blk-{'narrow' if pw == 1 else 'wide'}-{K_SCHUR_BLK[pw] + extra}", _schur_group, pw, extra,
                seed=next(seed))
    add("rank-tiles-34817", _rank_tiles, seed=next(seed))
    # the fast order past 8 free poses: no outlier, half the pixel noise
    for nf in (13, 14):
        for kind in ("full", "band(2)"):
            add(f"fast{nf}-{kind}", window, nf, kind, dict(cls="dense" if kind == "full" else "amd", fast=True),
                outlier_frac=0.0, pix_noise=0.5, seed=next(seed))
    return S


def _landmark_of_all(name, n_free, seed):
    obs = band(n_free, 2, 200) + [list(range(n_free))]
    obs = [o + [n_free + i % 2] if i % 3 == 0 else o for i, o in enumerate(obs)]
    return build(name, n_free + 2, [n_free, n_free + 1], obs, dict(np=n_free, cls="dense", pw=2, pattern="full"),
                 seed=seed)


def _ids_permuted(name, seed):
    """17 free poses whose ids are a permutation of list order (and the fixed ones' ids between them)."""
    n_free, n_kf = 17, 20
    ids = [int(x) for x in 3 + np.random.default_rng(seed).permutation(n_kf) * 2]
    return window(name, n_free, "band(3)+hub", dict(cls="amd", ids_permuted=True), n_fixed=3, ids=ids, seed=seed)


def _fixed_interleaved(name, seed):
    """Every third keyframe fixed, the list starting with a fixed one."""
    n_kf = 27
    fixed = list(range(0, n_kf, 3))
    free = [k for k in range(n_kf) if k not in fixed]
    obs = [[free[r] for r in o] for o in pattern("band(2)", len(free))]
    obs = [o + [fixed[(i // 2) % len(fixed)]] if i % 2 == 0 else o for i, o in enumerate(obs)]
    planes = (("wall", [0, 1, 2]), ("floor", [2, 3, 4]), ("side", [1, 2]))
    return build(name, n_kf, fixed, obs, dict(np=len(free), cls="amd", pattern="band(2)", interleaved=True),
                 planes=planes, seed=seed)


def _id0(name, seed):
    """The first keyframe has id 0 (held fixed by its id, not by its flag); some points are seen only by it and by
    fixed keyframes: they move, but take no part in the reduced system."""
    n_free = 12  # list entries 0 .. 11 not flagged fixed; entry 0 has id 0
    obs = [[1 + r for r in o] for o in pattern("band(2)", n_free - 1, 150)]
    obs = [o + [0] if i % 4 == 0 else o for i, o in enumerate(obs)]
    lonely = [[0, 12], [0, 13], [12, 13], [0, 12, 13], [0], [13]] * 3
    want = dict(np=n_free - 1, cls="amd", pattern="band(2)", lonely=len(lonely))
    return build(name, 14, [12, 13], obs + lonely, want, first_id=0, seed=seed)


def _unobserved(name, seed):
    """Free keyframe 5 of 13 sees nothing: it is no vertex of the optimisation and comes back unchanged."""
    free = [k for k in range(13) if k != 5]
    obs = [[free[r] for r in o] for o in pattern("band(2)", 12, 150)]
    obs = [o + [13] if i % 3 == 0 else o for i, o in enumerate(obs)]
    return build(name, 15, [13, 14], obs, dict(np=12, cls="amd", pattern="band(2)", unobserved=5), seed=seed)


def _all_fixed(name, seed):
    obs = [[i % 5, (i + 1 + i // 5 % 4) % 5] for i in range(150)]
    return build(name, 5, range(5), obs, dict(np=0, cls="none"), planes=(("wall", [0, 1, 2]), ("floor", [2, 3, 4])),
                 seed=seed)


def _planes_only(name, seed):
    ks = list(range(8))
    planes = (("wall", ks), ("floor", ks[1:]), ("ceil", ks[:6]), ("side", ks[2:]))
    return build(name, 8, [6, 7], [], dict(np=6, cls="dense", planes_only=True), planes=planes, seed=seed)


def _bridge(name, seed):
    """Two components of 9 free poses joined by one point (seen by poses 7, 8 and 9) whose observation in pose 9 is
    a gross outlier: the relabel removes that edge, the block (8, 9) stays in the Schur pattern of the second pass."""
    obs = pattern("two", 18, 240)
    obs = [o + [18 + i % 2] if i % 3 == 0 else o for i, o in enumerate(obs)]
    b = len(obs)
    obs.append([7, 8, 9])
    return build(name, 20, [18, 19], obs, dict(np=18, cls="amd", bridge=(b, 9)), gross=[(b, 9)], stereo_frac=1.0,
                 outlier_frac=0.0, seed=seed)


def _pose_outliers(name, seed):
    """Every observation of free pose 6 (of 12) is a gross outlier (a stereo match with a disparity of the wrong sign,
    which the pose cannot move to fit as it can fit a few of many shifted pixels): it has no active edge in the second
    pass."""
    obs = pattern("band(3)", 12, 180)
    obs = [o + [12 + i % 2] if i % 3 == 0 else o for i, o in enumerate(obs)]
    gross = [(i, 6) for i, o in enumerate(obs) if 6 in o]
    return build(name, 14, [12, 13], obs, dict(np=12, cls="amd", dead_pose=6), gross_disparity=gross,
                 stereo_frac=1.0,
                 outlier_frac=0.0, seed=seed)


def _all_outliers(name, seed):
    obs = [[0, 1, 2, 3, 4] for _ in range(40)]
    return build(name, 5, [3, 4], obs, dict(np=3, cls="dense", all_outliers=True), stereo_frac=1.0, all_gross=True,
                 seed=seed)


def _schur_group(name, pw, extra, seed):
    """The first 64-landmark group of the Schur phase holds kSchurBlk (+ extra) Hpl blocks; a second group follows."""
    n_free = 10
    lim = K_SCHUR_BLK[pw] + extra
    lo = lim // K_SCHUR_LM
    n_hi = lim - lo * K_SCHUR_LM
    counts = [lo + 1] * n_hi + [lo] * (K_SCHUR_LM - n_hi) + [3] * 30
    assert sum(counts[:64]) == lim
    n_kf = 12 if pw == 1 else 66
    return seam_points(name, None, None, dict(cls="dense", pw=pw, schur_blocks=lim), n_free=n_free, n_kf=n_kf,
                       counts=counts, outlier_frac=0.0, seed=seed)


def _rank_tiles(name, seed):
    """34,817 points with two stereo observations each over three keyframes, point and keyframe ids out of list
    order: one more point than an LDS tile of setup()'s rank counting holds."""
    n = K_TILE + 1
    rng = np.random.default_rng(seed)
    obs = [[i % 2, 2] if i % 3 else [0, 1] for i in range(n)]
    pid = [int(x) for x in 100 + rng.permutation(n)]
    return build(name, 3, [2], obs, dict(np=2, cls="dense", rank_tiles=2), ids=[9, 4, 6], point_ids=pid,
                 stereo_frac=1.0, outlier_frac=0.0, seed=seed)


SPECS = _specs()
NAMES = [n for n, _ in SPECS]
assert len(set(NAMES)) == len(NAMES)
SLOW = {"rank-tiles-34817"}  # built only by the tests that are about it


@functools.lru_cache(maxsize=None)
def case(name):
    return dict(SPECS)[name]()


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The oracle's result for a case (computed once, shared, never modified)."""
    import oracle_lba
    return oracle_lba.lba_optimize(*case(name)["P"][:6])
