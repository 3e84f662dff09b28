"""Case tables for the two tracking matchers (ORBmatcher::SearchByProjection frame to frame and
Tracking::SearchLocalPoints) off the rendered 640x480 pairs: derived cases (a rendered pair with changed records) and
constructed frames (keypoints placed by hand, descriptors with exact Hamming distances, a constant or stepped depth
image, the frame stage of the oracle building kun / uright / the grid / the bounds, points back-projected under the
identity pose).  No GPU import: tests/test_oracle_match_cases.py holds every case to the oracle and the Python
transcriptions and asserts that it reaches what it was built for; tests/test_gpu_match_geometry.py runs them on the
device.

A case is a dict: name, kind ("proj" / "local"), geom (a GEOMS key), the current frame (kun, desc, ur, go, gi, geo,
bounds), the record and list (fr, P / lfr, LP), params, for local cases taken (None: absent), and
  reach   what the case must reach, asserted on the transcription's intermediate values by the CPU test,
  expect  optionally the result known by construction: {keypoint: point} of the final assignment and nmatches.
Everything is deterministic (fixed seeds, no clock)."""
import functools

import numpy as np

import oracle_ctypes
import oracle_frame
import oracle_match as OM
from matcher_ref import f32 as _f, fma

GEOMS = {
    # Examples/RGB-D/TUM3.yaml as the rendered fixtures use it: no distortion, bounds 0 .. w, 10 x 10 px cells
    "tum": dict(fx=535.4, fy=539.2, cx=320.1, cy=247.6, bf=40.0, dist=(0.0,) * 5, width=640, height=480,
                scale_factor=1.2, nlevels=8),
    # barrel distortion: the undistorted corners lie outside the image, min_x / min_y negative, cells > 10 px
    "barrel": dict(fx=535.4, fy=539.2, cx=320.1, cy=247.6, bf=40.0, dist=(-0.28, 0.07, 0.0005, -0.0003, 0.0),
                   width=640, height=480, scale_factor=1.2, nlevels=8),
    # a second image size (7.5 x 7.5 px cells) with a second scale table (1.5, 5 levels)
    "small": dict(fx=401.55, fy=404.4, cx=240.075, cy=185.7, bf=30.0, dist=(0.0,) * 5, width=480, height=360,
                  scale_factor=1.5, nlevels=5),
}
K_KEYS = (6, 3)   # keys kept per point: batches of up to 16 frames, larger ones (match_launch.h)
# The largest cap the launches accept: the taken bits and the claim table, ceil(cap / 32) * 4 + cap * 4 bytes of
# dynamic LDS, against the 160 KB local_match_launch opts into and the 150 KB of match_launch (whose walk also holds
# the rotation histogram in static LDS).
LOCAL_CAP_LIMIT, PROJ_CAP_LIMIT = 39718, 37236
INF = np.float32(np.inf)


def up(x):
    return np.nextafter(np.float32(x), INF)


def down(x):
    return np.nextafter(np.float32(x), -INF)


@functools.lru_cache(None)
def scale_table(geom):
    """mvScaleFactors of the geometry's extractor, in the 8 slots of the oracle's geometry vector."""
    G = GEOMS[geom]
    t = oracle_ctypes.OrbOracle(1000, G["scale_factor"], G["nlevels"]).scale_tables()[0]
    out = np.zeros(8, np.float32)
    out[:len(t)] = t
    return out


def geometry(geom, bounds):
    """The oracle's geometry vector: fx fy cx cy bf, the bounds, the grid inverses, the scale table."""
    G, b = GEOMS[geom], np.asarray(bounds, np.float32)
    return np.concatenate([[G["fx"], G["fy"], G["cx"], G["cy"], G["bf"], b[0], b[1], b[2], b[3],
                            np.float32(64) / np.float32(b[1] - b[0]), np.float32(48) / np.float32(b[3] - b[2])],
                           scale_table(geom)]).astype(np.float32)


def bits(d):
    """A descriptor with exactly d bits set: Hamming distance d to the all-zero descriptor."""
    return np.packbits(np.arange(256) < int(d))


def frame(geom, kps, depth=2.0):
    """The current frame of keypoints (x, y, octave, angle, set descriptor bits) in distorted pixel coordinates over a
    depth image (a constant, or an [h, w] array), through the oracle's frame stage."""
    G = GEOMS[geom]
    k = np.asarray(kps, np.float64).reshape(-1, 5)
    img = np.broadcast_to(np.float32(depth), (G["height"], G["width"])) if np.isscalar(depth) else depth
    fo = oracle_frame.frame_rgbd(k[:, :2], np.ascontiguousarray(img, np.float32), G["fx"], G["fy"], G["cx"], G["cy"],
                                 dist=G["dist"], bf=G["bf"])
    kun = np.zeros(len(k), OM.KEYPOINT_DTYPE)
    kun["x"], kun["y"] = fo["un"][:, 0], fo["un"][:, 1]
    kun["octave"], kun["angle"] = k[:, 2].astype(np.int32), k[:, 3].astype(np.float32)
    kun["size"], kun["response"], kun["class_id"] = 31.0 * scale_table(geom)[kun["octave"]], 1.0, -1
    desc = np.stack([bits(b) for b in k[:, 4]]) if len(k) else np.zeros((0, 32), np.uint8)
    return dict(geom=geom, kun=kun, desc=desc, ur=fo["uright"].copy(), go=fo["grid_off"], gi=fo["grid_idx"],
                geo=geometry(geom, fo["bounds"]), bounds=fo["bounds"])


def stepped_depth(geom, near=1.0, far=3.0):
    """Depth `near` on the left half of the image, `far` on the right half."""
    G = GEOMS[geom]
    img = np.full((G["height"], G["width"]), near, np.float32)
    img[:, G["width"] // 2:] = far
    return img


def backproject(geom, u, v, z):
    G = GEOMS[geom]
    return np.array([(u - G["cx"]) * z / G["fx"], (v - G["cy"]) * z / G["fy"], z], np.float32)


IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


def proj_case(name, fr, pts, params=(15.0, 0, 0, 0), tlw_z=0.0, reach=None, expect=None, **extra):
    """pts: rows (u, v, z, octave, angle, n_obs, bits) projected under the identity pose, or (xw, octave, angle,
    n_obs, bits) with the camera coordinates given.  tlw_z: Tlw[11], which feeds nothing but the direction flags."""
    P = np.zeros(len(pts), OM.PROJ_POINT_DTYPE)
    for i, row in enumerate(pts):
        if len(row) == 7:
            row = (backproject(fr["geom"], *row[:3]),) + tuple(row[3:])
        P[i]["xw"], P[i]["octave"], P[i]["angle"], P[i]["n_obs"], P[i]["desc"] = row[0], row[1], row[2], row[3], \
            bits(row[4])
        P[i]["last_index"], P[i]["id"] = i, i
    rec = np.zeros((), OM.PROJ_FRAME_DTYPE)
    rec["Tcw"], rec["Tlw"], rec["n_points"] = IDENTITY, IDENTITY, len(P)
    rec["Tlw"][11] = tlw_z
    return dict(fr, name=name, kind="proj", fr=rec, P=P, params=tuple(params), reach=reach or {}, expect=expect,
                **extra)


def local_point(geom, u, v, z, level, bits_=0, tilt_deg=0.0, xw=None, dist_scale=1.0, pid=0):
    """A local map point seen at pixel (u, v), depth z, whose distance range predicts `level` (max_dist = dist *
    s^(level - 0.5)) and whose normal is tilted by tilt_deg off the viewing ray; dist_scale scales the range."""
    G = GEOMS[geom]
    p = np.zeros((), OM.LOCAL_POINT_DTYPE)
    x = backproject(geom, u, v, z) if xw is None else np.asarray(xw, np.float32)
    d = float(np.linalg.norm(x.astype(np.float64)))
    ray = x.astype(np.float64) / d if d > 0 else np.array([0.0, 0.0, 1.0])
    side = np.cross(ray, [0.0, 1.0, 0.0])
    side /= np.linalg.norm(side)
    t = np.deg2rad(tilt_deg)
    p["xw"], p["normal"] = x, np.cos(t) * ray + np.sin(t) * side
    s = float(G["scale_factor"])
    p["max_dist"] = max(d, 1e-3) * s ** (level - 0.5) * dist_scale
    p["min_dist"] = p["max_dist"] / np.float32(s ** (G["nlevels"] - 1))
    p["id"], p["n_obs"], p["desc"] = pid, 1, bits(bits_)
    return p


def local_case(name, fr, pts, params=(3.0, 0.8, 0.5), taken=None, reach=None, expect=None, **extra):
    LP = np.array(pts, OM.LOCAL_POINT_DTYPE) if len(pts) else np.zeros(0, OM.LOCAL_POINT_DTYPE)
    LP["id"] = np.arange(len(LP))
    rec = np.zeros((), OM.LOCAL_FRAME_DTYPE)
    rec["Tcw"], rec["n_points"] = IDENTITY, len(LP)
    return dict(fr, name=name, kind="local", lfr=rec, LP=LP, params=tuple(params),
                taken=None if taken is None else np.asarray(taken, np.uint8), reach=reach or {}, expect=expect,
                **extra)


def lattice(n, geom="tum", cols=13, margin=30):
    """n sites on a lattice inside the grid, far enough apart that the windows of two sites share no keypoint."""
    G = GEOMS[geom]
    rows = -(-n // cols)
    dx = (G["width"] - 2 * margin - 10) / max(cols - 1, 1)
    dy = (G["height"] - 2 * margin - 10) / max(rows - 1, 1)
    return [(margin + dx * (i % cols), margin + dy * (i // cols)) for i in range(n)]


def solve_axis(f, c, target, above):
    """A camera coordinate x at a depth z whose pixel coordinate fma(f * x, (float)(1 / z), c) is exactly `target`,
    and at the same depth the nearest coordinate whose pixel lies outside it (above or below).  Depths are tried in
    turn (the products f * x * (1 / z) reach only some of the floats near the target).  Returns (z, x_on, x_out)."""
    f, c, target = _f(f), _f(c), _f(target)
    for step_z in range(400):
        z = _f(1.0 + step_z / 64.0)
        invz = _f(1.0 / float(z))
        x = _f((float(target) - float(c)) / float(f) * float(z))
        xs = [x]
        for step in (up, down):
            y = x
            for _ in range(24):
                y = step(y)
                xs.append(y)
        vals = sorted((float(fma(_f(f * xi), invz, c)), float(xi)) for xi in xs)
        on = [xi for val, xi in vals if val == float(target)]
        out = [xi for val, xi in vals if (val > float(target) if above else val < float(target))]
        if on and out:
            return z, _f(on[0]), _f(out[0] if above else out[-1])
    raise AssertionError(f"no camera coordinate projects exactly onto {target}")


# ---------------------------------------------------------------------------------------------------- rendered pair
@functools.lru_cache(None)
def rendered():
    """The first rendered pair of tests/test_gpu_match.py with its local-map problem."""
    from test_oracle_match import local_problems, make_pairs
    return local_problems(make_pairs(((0, 10, 12),), seed=17), seed=23)[0]


def _derived(name, kind, reach=None, **changes):
    q = rendered()
    base = {k: q[k] for k in ("kun", "desc", "ur", "go", "gi", "geo")}
    base.update(geom="tum", bounds=q["geo"][5:9], name=name, kind=kind, reach=reach or {}, expect=None)
    if kind == "proj":
        base.update(fr=q["fr"].copy(), P=q["P"].copy(), params=(15.0, 0, 1, 0))
    else:
        base.update(lfr=q["lfr"].copy(), LP=q["LP"].copy(), params=(3.0, 0.8, 0.5), taken=q["taken"])
    base.update(changes)
    return base


def _shift_tlw(fr, dz):
    fr = fr.copy()
    fr["Tlw"][11] += np.float32(dz)
    return fr


# ------------------------------------------------------------------------------------------------- SearchByProjection
def _direction_frame(geom):
    """Three sites; around each, one keypoint per octave whose descriptor distance orders the octaves so that the
    forward range (>= the point's octave), the backward range (<= it) and the plain range (+-1) each pick another
    keypoint: the top octave is nearest, octave 0 next, the point's own octave third."""
    G = GEOMS[geom]
    nl, w = G["nlevels"], G["width"] / 640.0
    p_oct = nl // 2 - 1 if nl == 8 else nl // 2
    order = [nl - 1, 0, p_oct] + [o for o in range(nl) if o not in (nl - 1, 0, p_oct)]
    dist_of = {o: 5 + r for r, o in enumerate(order)}
    sites = [(100 * w, 100 * w), (300 * w, 200 * w), (500 * w, 350 * w)]
    kps = [(sx + (2 * o - nl + 1) * w, sy + (o % 3 - 1) * w, o, 0.0, dist_of[o]) for sx, sy in sites
           for o in range(nl)]
    return frame(geom, kps), sites, p_oct, nl


def direction_cases(geom):
    fr, sites, p_oct, nl = _direction_frame(geom)
    G = GEOMS[geom]
    mb = _f(_f(G["bf"]) / _f(G["fx"]))
    out = []
    for tag, z in (("zero", 0.0), ("plus", 0.15), ("minus", -0.15), ("at_mb", mb), ("above_mb", up(mb)),
                   ("below_mb", down(mb)), ("at_neg_mb", -mb), ("beyond_neg_mb", -up(mb)),
                   ("inside_neg_mb", -down(mb))):
        for mono in (0, 1):
            fwd, bwd = bool(_f(z) > mb) and not mono, bool(-_f(z) > mb) and not mono
            win = nl - 1 if fwd else 0 if bwd else p_oct
            mid = [fr["kun"][s * nl + nl // 2] for s in range(len(sites))]  # (sites in undistorted coordinates)
            pts = [(float(k["x"]), float(k["y"]), 2.0, p_oct, 0.0, 1, 0) for k in mid]
            out.append(proj_case(f"direction_{geom}_{tag}_mono{mono}", fr, pts, params=(15.0, mono, 0, 0), tlw_z=z,
                                 reach=dict(fwd=fwd, bwd=bwd),
                                 expect=dict(match={s * nl + win: s for s in range(len(sites))}, nm=len(sites))))
    return out


def _pair_frame(n_sites, geom="tum", depth=2.0, cols=13):
    """Two keypoints per site (distances 3 and 9), 2 px apart."""
    s = lattice(n_sites, geom, cols)
    return frame(geom, [(x + 2 * j, y, 0, 30.0 * (i % 12), 3 + 6 * j) for i, (x, y) in enumerate(s) for j in range(2)],
                 depth), s


def point_count_cases():
    """Point counts at kPtsPerBlock and at the 64-point chunks of the in-order walk: two points per site; the second
    takes the second keypoint where the first blocks it and overwrites the first where it does not."""
    out = []
    for n in (15, 16, 17, 63, 64, 65, 127, 128, 129):
        fr, s = _pair_frame(-(-n // 2))
        pts = [(s[i // 2][0], s[i // 2][1], 2.0, 0, 30.0 * ((i // 2) % 12), int(i % 3 != 0), 0) for i in range(n)]
        out.append(proj_case(f"points_{n}", fr, pts, reach=dict(nm_min=n // 2, overwritten=n >= 17)))
    # a batch call whose max_points cuts the list: the expectation is the oracle on the first max_points points
    out.append(dict(out[-1], name="points_129_max_points_100", max_points=100))
    return out


def _kp_frame(n_kp, depth=2.0):
    s = lattice(n_kp, cols=27, margin=20)
    return frame("tum", [(x, y, j % 2, 0.0, 1 + j % 40) for j, (x, y) in enumerate(s)], depth), s


KP_COUNTS = (2, 31, 32, 33, 63, 64, 65, 511, 512, 513)


def keypoint_count_cases():
    """Keypoint counts at the word seams of the taken bits and the 512-keypoint stride of their loader: two points per
    site on the last (up to) 40 keypoints, so the highest indices are the ones claimed and taken."""
    out = []
    for n_kp in KP_COUNTS:
        fr, s = _kp_frame(n_kp)
        sites = list(range(n_kp - 1, max(n_kp - 41, -1), -1))
        pts = [(s[k][0], s[k][1], 2.0, 0, 0.0, int((i + j) % 4 != 0), 0) for i, k in enumerate(sites)
               for j in range(2)]
        out.append(proj_case(f"keypoints_{n_kp}", fr, pts, reach=dict(last_keypoint_matched=True)))
    return out


TAKEN_SEAMS = (31, 32, 63, 64, 511, 512)   # and the last keypoint: the word seams of the taken-bit loader


def _taken_seams(n_kp):
    t = np.zeros(n_kp, np.uint8)
    t[[k for k in TAKEN_SEAMS + (n_kp - 1,) if k < n_kp]] = 1
    return t


def dense_frame(n_kp, layout, alternate_octaves=False):
    """n_kp keypoints inside an 8 x 8 px square: within the cell (30, 20) ("cell") or around the corner of the cells
    (30..31, 20..21) ("corner").  The keypoints on the loader's word seams have the smallest distances (0, 1, ...), so
    a search that misses one of their taken bits picks it at once; the others 7 + (j * 37) % 90, all accepted, with
    up to 6 equal ones for 513.  alternate_octaves: octaves 0 and 1 in turn along the keypoints sorted by distance,
    so that the local search's best and second best differ in octave (and pass the ratio test) wherever no taken
    keypoint breaks the turn.  Returns the frame, the window's centre and the keypoints in that order."""
    ox, oy = (296.0, 196.0) if layout == "cell" else (301.0, 201.0)
    seams = [k for k in TAKEN_SEAMS + (n_kp - 1,) if k < n_kp]
    dist = [seams.index(j) if j in seams else 7 + (j * 37) % 90 for j in range(n_kp)]
    fr = frame("tum", [(ox + 8 * ((j * 0.6180339887) % 1.0), oy + 8 * ((j * 0.7548776662) % 1.0), 0, 12.0 * (j % 30),
                        dist[j]) for j in range(n_kp)])
    # the order in which a search prefers them: by distance, equal ones by scan (CSR) position
    pos = np.empty(n_kp, np.int64)
    pos[fr["gi"]] = np.arange(n_kp)
    order = [j for _, _, j in sorted((dist[j], pos[j], j) for j in range(n_kp))]
    if alternate_octaves:
        fr["kun"]["octave"][order] = np.arange(n_kp) % 2
        fr["kun"]["size"] = 31.0 * scale_table("tum")[fr["kun"]["octave"]]
    return fr, (ox + 4.0, oy + 4.0), order


def dense_cases():
    """More points than kept keys compete for the keypoints of one window: blocking holders force the next key and
    then the re-scan, non-blocking ones are overwritten."""
    out = []
    rng = np.random.default_rng(41)
    for n_kp, n_pts in ((65, 40), (200, 129), (513, 129)):
        for layout in ("cell", "corner"):
            fr, (cx, cy), _ = dense_frame(n_kp, layout)
            n_obs = (rng.uniform(size=n_pts) < 0.7).astype(int)
            pts = [(cx, cy, 2.0, 0, 12.0 * (i % 7), int(n_obs[i]), 0) for i in range(n_pts)]
            reach = dict(rescan=True, overwritten=True, cells=1 if layout == "cell" else 4,
                         cell_population=n_kp if layout == "cell" else None)
            out.append(proj_case(f"dense_{n_kp}_{layout}", fr, pts, reach=reach))
            if n_kp == 200:
                out.append(proj_case(f"dense_{n_kp}_{layout}_ori", fr, pts, params=(15.0, 0, 1, 0),
                                     reach=dict(rescan=True, bins_dropped=True)))
    return out


def border_cases(geom):
    """Windows clipped at each side and at two corners, windows without keypoints, keypoints outside the grid, and
    projections exactly on each bound and the nearest projection outside it."""
    G = GEOMS[geom]
    w, h = G["width"], G["height"]
    s = w / 640.0
    # distorted pixel positions; the keypoints of the last two columns / rows of pixels round to cell 64 / 48 without
    # distortion and are absent from the grid
    sites = [(4 * s, h / 2), (w - 9 * s, h / 2), (w / 2, 4 * s), (w / 2, h - 9 * s), (4 * s, 4 * s),
             (w - 9 * s, h - 9 * s)]
    kps = [(x + dx, y + dy, 1, 0.0, 10 + i) for i, (x, y) in enumerate(sites) for dx, dy in ((0, 0), (2 * s, 1 * s))]
    kps += [(w - 1.5, h / 2, 1, 0.0, 1), (w / 2, h - 1.5, 1, 0.0, 1), (w - 1.5, h - 1.5, 1, 0.0, 1)]
    fr = frame(geom, kps)
    b = fr["bounds"]
    pts = []
    # the sites, through the undistorted positions of their first keypoints, and two windows over empty cells
    for i in range(len(sites)):
        pts.append((float(fr["kun"]["x"][2 * i]), float(fr["kun"]["y"][2 * i]), 2.0, 2, 0.0, 1, 0))
    pts += [(w * 0.3, h * 0.3, 2.0, 2, 0.0, 1, 0), (w * 0.7, h * 0.6, 2.0, 0, 0.0, 1, 0)]
    case = proj_case(f"border_{geom}", fr, pts,
                     reach=dict(clipped=True, empty_window=True, off_grid=3 if not any(G["dist"]) else None, nm_min=6))
    # on the bounds and just outside: an undistorted keypoint sits near the middle of each bound
    mid_u, mid_v = _f((b[0] + b[1]) / 2), _f((b[2] + b[3]) / 2)
    edge_kun = [(b[0] + 3, mid_v), (b[1] - 8 * s, mid_v), (mid_u, b[2] + 3), (mid_u, b[3] - 8 * s)]
    on_pts, out_pts, exact = [], [], []
    for axis, bound, above in ((0, b[0], False), (0, b[1], True), (1, b[2], False), (1, b[3], True)):
        f, c = (G["fx"], G["cx"]) if axis == 0 else (G["fy"], G["cy"])
        z, x_on, x_out = solve_axis(f, c, bound, above)
        other = _f((float(mid_v if axis == 0 else mid_u) - float(G["cy"] if axis == 0 else G["cx"])) /
                   float(G["fy"] if axis == 0 else G["fx"]) * z)
        for lst, x in ((on_pts, x_on), (out_pts, x_out)):
            xw = np.array([x, other, z] if axis == 0 else [other, x, z], np.float32)
            lst.append((xw, 2, 0.0, 1, 0))
        exact.append((axis, float(bound), above))
    edge = dict(geom=geom, **_placed_frame(geom, edge_kun, fr["bounds"], octave=1, bits_=7))
    on_case = proj_case(f"on_bounds_{geom}", edge, on_pts, reach=dict(exact=exact, nm_min=4),
                        expect=dict(match={k: k for k in range(4)}, nm=4))
    out_case = proj_case(f"off_bounds_{geom}", edge, out_pts, reach=dict(outside=exact),
                         expect=dict(match={}, nm=0))
    return [case, on_case, out_case]


def _placed_frame(geom, kun_xy, bounds, octave, bits_):
    """A frame whose undistorted keypoints are given directly (the grid by Frame::PosInGrid on them, in double on
    exactly the float expressions of AssignFeaturesToGrid), every keypoint mono."""
    n = len(kun_xy)
    kun = np.zeros(n, OM.KEYPOINT_DTYPE)
    kun["x"], kun["y"] = [p[0] for p in kun_xy], [p[1] for p in kun_xy]
    kun["octave"], kun["size"], kun["response"], kun["class_id"] = octave, 31.0, 1.0, -1
    geo = geometry(geom, bounds)
    cells = {}
    for k in range(n):
        px = int(np.floor(float(_f(_f(kun["x"][k] - geo[5]) * geo[9])) + 0.5))
        py = int(np.floor(float(_f(_f(kun["y"][k] - geo[7]) * geo[10])) + 0.5))
        if 0 <= px < 64 and 0 <= py < 48:
            cells.setdefault(px * 48 + py, []).append(k)
    go, gi = np.zeros(64 * 48 + 1, np.int32), []
    for c in range(64 * 48):
        go[c] = len(gi)
        gi += cells.get(c, [])
    go[-1] = len(gi)
    return dict(kun=kun, desc=np.stack([bits(bits_)] * n), ur=np.full(n, -1.0, np.float32), go=go,
                gi=np.array(gi, np.int32), geo=geo, bounds=np.asarray(bounds, np.float32))


def seam_cases():
    s = lattice(8, cols=4, margin=60)
    out = []
    # TH_HIGH: 100 is accepted, 101 is not
    fr = frame("tum", [(s[0][0], s[0][1], 0, 0.0, 100), (s[1][0], s[1][1], 0, 0.0, 101)])
    out.append(proj_case("th_high", fr, [(s[0][0], s[0][1], 2.0, 0, 0.0, 1, 0), (s[1][0], s[1][1], 2.0, 0, 0.0, 1, 0)],
                         reach=dict(best=[100, 101]), expect=dict(match={0: 0}, nm=1)))
    # equal distances: the first keypoint in the scan order (cells by column, then row; within a cell by index) wins.
    # Site A, one cell: keypoints 0 and 1.  Site B, two cells: keypoint 2 lies in the later cell (x + 6), keypoint 3 in
    # the earlier one, so the higher index wins.  Site C, two rows of one column: 4 is below (later) 5.
    ax, ay, bx, by, cx, cy = 102.0, 102.0, 303.0, 202.0, 401.0, 303.0
    fr = frame("tum", [(ax, ay, 0, 0.0, 9), (ax + 1, ay + 1, 0, 0.0, 9), (bx + 4, by, 0, 0.0, 9),
                       (bx - 2, by, 0, 0.0, 9), (cx, cy + 4, 0, 0.0, 9), (cx, cy - 2, 0, 0.0, 9)])
    out.append(proj_case("equal_distances", fr, [(ax, ay, 2.0, 0, 0.0, 1, 0), (bx, by, 2.0, 0, 0.0, 1, 0),
                                                  (cx, cy, 2.0, 0, 0.0, 1, 0)],
                         reach=dict(ties=3), expect=dict(match={0: 0, 3: 1, 5: 2}, nm=3)))
    # stereo: every keypoint mono (no depth), every keypoint stereo with the points at the keypoints' depth, and
    # a stepped depth image against points at one depth (the right-coordinate test drops the far half)
    for tag, depth in (("all_mono", 0.0), ("all_stereo", 2.0), ("stepped", stepped_depth("tum", 2.0, 0.5))):
        fr, st = _pair_frame(33, depth=depth)
        pts = [(st[i // 2][0], st[i // 2][1], 2.0, 0, 30.0 * ((i // 2) % 12), int(i % 3 != 0), 0) for i in range(65)]
        out.append(proj_case(f"stereo_{tag}", fr, pts, reach=dict(stereo=tag)))
    # the right-coordinate error exactly the radius (kept) and the next float above it (dropped)
    fr = frame("tum", [(s[2][0], s[2][1], 0, 0.0, 4), (s[3][0], s[3][1], 0, 0.0, 4)])
    pts = [(s[2][0], s[2][1], 2.0, 0, 0.0, 1, 0), (s[3][0], s[3][1], 2.0, 0, 0.0, 1, 0)]
    case = proj_case("stereo_error_at_radius", fr, pts, expect=dict(match={0: 0}, nm=1))
    g = case["geo"]
    r = _f(_f(15.0) * g[11])
    for k, above in ((0, False), (1, True)):
        x3 = case["P"][k]["xw"]
        invz = _f(1.0 / float(x3[2]))
        urp = fma(-g[4], invz, fma(_f(g[0] * x3[0]), invz, g[2]))
        ur = _f(urp - r)
        for _ in range(64):  # the float whose error is exactly r, then the nearest one whose error exceeds it
            err = abs(_f(urp - ur))
            if (err > r) if above else (err == r):
                break
            ur = down(ur) if err <= r else up(ur)
        case["ur"][k] = ur
    case["reach"] = dict(stereo_error=[(0, "at"), (1, "above")])
    out.append(case)
    return out


def _histogram_case(name, counts, extra_pts=(), expect_dropped=()):
    """One keypoint and one point per site; the angle difference of site i puts it into the bin given by `counts`
    (bin: number of sites)."""
    bins = [b for b, n in counts.items() for _ in range(n)]
    s = lattice(len(bins) + 2, cols=13)
    fr = frame("tum", [(x, y, 0, 40.0, 5) for x, y in s])
    pts = [(s[i][0], s[i][1], 2.0, 0, (40.0 + 30.0 * b) % 360.0, 1, 0) for i, b in enumerate(bins)]
    return proj_case(name, fr, pts, params=(15.0, 0, 1, 0),
                     reach=dict(hist=counts, dropped=list(expect_dropped)),
                     expect=dict(match={i: i for i, b in enumerate(bins) if b not in expect_dropped},
                                 nm=sum(n for b, n in counts.items() if b not in expect_dropped)))


def rotation_cases():
    out = [
        # second and third maxima tie, each exactly 0.1 x the first (kept: the test is <); the fourth is dropped
        _histogram_case("rotation_tie_at_tenth", {0: 20, 3: 2, 7: 2, 9: 1}, expect_dropped=(9,)),
        # the second maximum just under 0.1 x the first: it and the third go
        _histogram_case("rotation_second_under_tenth", {2: 21, 5: 2, 6: 1}, expect_dropped=(5, 6)),
        # the third just under, the second at it
        _histogram_case("rotation_third_under_tenth", {1: 30, 4: 3, 8: 2}, expect_dropped=(8,)),
        # three bins tie for second: the first two found stay
        _histogram_case("rotation_three_tie", {0: 10, 4: 3, 6: 3, 11: 3}, expect_dropped=(11,)),
    ]
    # angle differences on the bin boundaries: rot / 30 rounds half away from zero, so 15 is bin 1 and the float
    # below it bin 0; 0 and just under 360 (bin 12); a negative difference wraps by +360
    s = lattice(16, cols=4, margin=60)
    fr = frame("tum", [(x, y, 0, 100.0, 5) for x, y in s[:12]])
    angles = [100.0, 100.0, 100.0, 100.0, 115.0, 115.0, down(115.0), 145.0, down(100.0), 85.0, 60.0, 114.0]
    pts = [(s[i][0], s[i][1], 2.0, 0, float(angles[i]), 1, 0) for i in range(12)]
    out.append(proj_case("rotation_bin_boundaries", fr, pts, params=(15.0, 0, 1, 0),
                         reach=dict(hist={0: 6, 1: 2, 2: 1, 11: 1, 12: 2}, dropped=[2, 11])))
    # one keypoint pushed twice: a non-blocking point, then another, their pushes in a kept and in a dropped bin.
    # The reference clears the keypoint for the dropped push whichever it was, and counts one match less.  Bins 2 and
    # 3 (two pushes each) put bin 5's single push in fourth place.
    n0 = 6
    fr = frame("tum", [(x, y, 0, 40.0, 5) for x, y in s[:n0 + 1] + s[8:12]])
    for tag, first_bin, second_bin in (("kept_then_dropped", 0, 5), ("dropped_then_kept", 5, 0)):
        pts = [(s[i][0], s[i][1], 2.0, 0, 40.0, 1, 0) for i in range(n0)]
        pts += [(s[n0][0], s[n0][1], 2.0, 0, 40.0 + 30.0 * first_bin, 0, 0),
                (s[n0][0], s[n0][1], 2.0, 0, 40.0 + 30.0 * second_bin, 1, 0)]
        pts += [(s[8 + j][0], s[8 + j][1], 2.0, 0, 40.0 + 30.0 * (2 + j // 2), 1, 0) for j in range(4)]
        kept = {**{i: i for i in range(n0)}, **{n0 + 1 + j: n0 + 2 + j for j in range(4)}}
        out.append(proj_case(f"pushed_twice_{tag}", fr, pts, params=(15.0, 0, 1, 0),
                             reach=dict(hist={0: n0 + 1, 2: 2, 3: 2, 5: 1}, dropped=[5], pushed_twice=n0),
                             expect=dict(match=kept, nm=n0 + 1 + 4)))
    return out


def retry_cases():
    """TrackWithMotionModel's second search at 2 * th: retry_below just above and just below the first pass's count,
    on a forward case, a dense case and the rendered pair."""
    out = []
    q = rendered()
    shifted = _derived("", "proj", fr=_shift_tlw(q["fr"], 0.15))
    bases = [direction_cases("tum")[2], dense_cases()[2], shifted]
    for base in bases:
        th, mono, ori, _ = base["params"]
        _, n1, _ = OM.search_by_projection(base["fr"], base["P"], base["kun"], base["desc"], base["ur"], base["go"],
                                           base["gi"], base["geo"], params=(th, mono, ori, 0))
        tag = base["name"] or "rendered_forward"
        for rb, passes in ((n1, 1), (n1 + 1, 2)):
            out.append(dict(base, name=f"retry_{tag}_{'taken' if passes == 2 else 'not_taken'}",
                            params=(th, mono, ori, rb),
                            reach=dict({k: v for k, v in base["reach"].items() if k in ("fwd", "bwd")}, passes=passes),
                            expect=None))
    return out


def derived_proj_cases():
    q = rendered()
    return [_derived("rendered_forward", "proj", fr=_shift_tlw(q["fr"], 0.15), reach=dict(fwd=True, bwd=False)),
            _derived("rendered_backward", "proj", fr=_shift_tlw(q["fr"], -0.15), reach=dict(fwd=False, bwd=True)),
            _derived("rendered_forward_mono", "proj", fr=_shift_tlw(q["fr"], 0.15), params=(15.0, 1, 1, 0),
                     reach=dict(fwd=False, bwd=False))]


def second_geometry_proj_cases():
    out = []
    for geom in ("barrel", "small"):
        out += [c for c in direction_cases(geom) if "_zero_" in c["name"] or "_plus_" in c["name"]
                or "_minus_" in c["name"] or "_at_mb_" in c["name"]]
        out += border_cases(geom)
        fr, s = _pair_frame(33, geom)
        top = GEOMS[geom]["nlevels"] - 1
        pts = [(float(fr["kun"]["x"][2 * (i // 2)]), float(fr["kun"]["y"][2 * (i // 2)]), 2.0, (0, 1, top)[i % 3],
                30.0 * ((i // 2) % 12), int(i % 3 != 0), 0) for i in range(65)]
        out.append(proj_case(f"pairs_{geom}", fr, pts, reach=dict(nm_min=30)))
    return out


PROJ_GROUPS = {
    "direction": lambda: direction_cases("tum") + derived_proj_cases(),
    "point_counts": point_count_cases,
    "keypoint_counts": keypoint_count_cases,
    "dense": dense_cases,
    "border": lambda: border_cases("tum"),
    "seams": seam_cases,
    "rotation": rotation_cases,
    "retry": retry_cases,
    "second_geometry": second_geometry_proj_cases,
}


@functools.lru_cache(None)
def proj_group(name):
    return PROJ_GROUPS[name]()


def proj_cases():
    cases = [c for name in PROJ_GROUPS for c in proj_group(name)]
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


# ------------------------------------------------------------------------------------------------ SearchLocalPoints
FRUSTUM_REASONS = ("behind", "left", "right", "top", "bottom", "near", "far", "view_cos")


def frustum_cases(geom="tum"):
    """Each isInFrustum rejection on its own list, then all of them mixed with points in view."""
    G = GEOMS[geom]
    w = G["width"]
    s = lattice(20, geom, cols=5, margin=int(60 * w / 640))
    fr = frame(geom, [(x, y, i % 2, 0.0, 3) for i, (x, y) in enumerate(s)])
    b = fr["bounds"]
    s = [(float(k["x"]), float(k["y"])) for k in fr["kun"]]  # (the sites in undistorted coordinates)
    good = lambda i: local_point(geom, s[i][0], s[i][1], 2.0, 1)  # noqa: E731

    def rejected(why, i):
        x, y = s[i]
        if why == "behind":   # mirrored through the camera centre
            return local_point(geom, x, y, 2.0, 1, xw=-backproject(geom, x, y, 2.0))
        if why == "z_zero":   # Pc.z exactly 0 is not "behind": 1 / 0 projects it to infinity, outside the bounds
            return local_point(geom, x, y, 2.0, 1, xw=(0.3, 0.2, 0.0))
        if why in ("left", "right", "top", "bottom"):  # shifted sideways
            uv = dict(left=(b[0] - 40.0, y), right=(b[1] + 40.0, y), top=(x, b[2] - 40.0), bottom=(x, b[3] + 40.0))[why]
            return local_point(geom, uv[0], uv[1], 2.0, 1)
        if why == "near":     # the distance range scaled up: dist < 0.8 * min_dist
            return local_point(geom, x, y, 2.0, G["nlevels"] - 1, dist_scale=1.6)
        if why == "far":      # and scaled down: dist > 1.2 * max_dist
            return local_point(geom, x, y, 2.0, 0, dist_scale=0.7)
        return local_point(geom, x, y, 2.0, 1, tilt_deg=75.0 if why == "view_cos" else 180.0)  # normal turned away

    out = []
    kinds = ("behind", "z_zero", "left", "right", "top", "bottom", "near", "far", "view_cos", "flipped")
    for why in kinds:
        pts = [good(0), rejected(why, 1), good(2), rejected(why, 3)]
        test = dict(z_zero="right", flipped="view_cos").get(why, why)  # the isInFrustum test that rejects it
        out.append(local_case(f"frustum_{geom}_{why}", fr, pts,
                              reach=dict(in_view=[True, False, True, False], why={1: test, 3: test}),
                              expect=dict(match={0: 0, 2: 2}, nm=2)))
    pts = [good(i) if i % 2 == 0 else rejected(kinds[(i // 2) % len(kinds)], i) for i in range(20)]
    out.append(local_case(f"frustum_{geom}_mixed", fr, pts,
                          reach=dict(in_view=[i % 2 == 0 for i in range(20)], reasons=set(FRUSTUM_REASONS))))
    return out


def _level_search(geom, kind):
    """A point whose PredictScale level before the clamp is -1 (kind "low": the distance at the far end of its range)
    or above the top level (kind "high": at the near end); searched over floats so the isInFrustum range still holds."""
    from test_oracle_match import py_search_local
    G = GEOMS[geom]
    fr = frame(geom, [])
    u, v = G["width"] / 2.0, G["height"] / 2.0
    rec = np.zeros((), OM.LOCAL_FRAME_DTYPE)
    rec["Tcw"], rec["n_points"] = IDENTITY, 1
    # low: max_dist within a few floats of dist / 1.2, over depths until the roundings of 1.2f * max_dist and of
    # max_dist / dist fall that way; high: min_dist = 1.24 dist, so 0.8 min_dist lies just under dist
    for step in range(7 * 64 if kind == "low" else 1):
        p = local_point(geom, u, v, 2.0 + 0.013 * (step // 7), 0.5 if kind == "low" else G["nlevels"] - 1 + 0.5,
                        dist_scale=1.0 / 1.2 if kind == "low" else 1.24)
        for _ in range(abs(step % 7 - 3)):
            p["max_dist"] = (up if step % 7 > 3 else down)(p["max_dist"])
        t = {}
        py_search_local(rec, np.array([p]), fr["kun"], fr["desc"], fr["ur"], fr["go"], fr["gi"], fr["geo"], [],
                        scale_factor=G["scale_factor"], n_levels=G["nlevels"], trace=t)
        if t[0]["why"] is None and (t[0]["raw_level"] < 0 if kind == "low" else t[0]["raw_level"] >= G["nlevels"]):
            return p
    raise AssertionError(f"no point clamps {kind} for {geom}")


def scale_cases(geom):
    """PredictScale clamped at both ends, with keypoints of the clamped level's octaves and of the octaves an
    unclamped level would search."""
    G = GEOMS[geom]
    nl = G["nlevels"]
    u, v = G["width"] / 2.0, G["height"] / 2.0
    step = G["width"] / 640.0
    kps = [(u + (o - nl / 2) * step, v + (o % 2) * step, o, 0.0, 20 - o) for o in range(nl)]
    fr = frame(geom, kps)
    # high: level nl - 1 searches octaves nl - 2 .. nl - 1, the nearer descriptor being the top octave's
    out = [local_case(f"predict_scale_high_{geom}", fr, [_level_search(geom, "high")],
                      reach=dict(raw_above=True, level=[nl - 1]), expect=dict(match={nl - 1: 0}, nm=1))]
    # low: level -1 needs max_dist / dist <= 1 / scale_factor inside the range dist <= 1.2 max_dist, which only a
    # scale factor of 1.2 allows; level 0 searches octaves -1 .. 0, so keypoint 0
    if G["scale_factor"] == 1.2:
        out.append(local_case(f"predict_scale_low_{geom}", fr, [_level_search(geom, "low")],
                              reach=dict(raw_below=True, level=[0]), expect=dict(match={0: 0}, nm=1)))
    return out


def radius_and_ratio_cases():
    s = lattice(12, cols=4, margin=60)
    out = []
    # RadiusByViewingCos: the keypoint 11 px off is inside 4.0 * 3 * 1.2 = 14.4 and outside 2.5 * 3 * 1.2 = 9
    fr = frame("tum", [(s[0][0] + 11, s[0][1], 1, 0.0, 5), (s[1][0] + 11, s[1][1], 1, 0.0, 5)])
    pts = [local_point("tum", s[0][0], s[0][1], 2.0, 1, tilt_deg=3.0), local_point("tum", s[1][0], s[1][1], 2.0, 1,
                                                                                   tilt_deg=4.0)]
    out.append(local_case("radius_by_view_cos", fr, pts, reach=dict(radius=[7.5, 12.0]),
                          expect=dict(match={1: 1}, nm=1)))
    # the ratio test, per site two keypoints (best, second): same octave 80 / 100 kept (80 > 0.8f * 100 is false in
    # float), 81 / 100 dropped; different octaves kept whatever the ratio; a single candidate; best 100 and 101
    sites = [((80, 1), (100, 1), True), ((81, 1), (100, 1), False), ((90, 1), (91, 0), True), ((99, 1), None, True),
             ((100, 1), None, True), ((101, 1), None, False), ((100, 0), (100, 1), True), ((50, 1), (50, 1), False)]
    kps, pts, match = [], [], {}
    for i, (a, b, kept) in enumerate(sites):
        if kept:
            match[len(kps)] = i
        kps.append((s[i][0], s[i][1], a[1], 0.0, a[0]))
        if b:
            kps.append((s[i][0] + 2, s[i][1] + 1, b[1], 0.0, b[0]))
        pts.append(local_point("tum", s[i][0], s[i][1], 2.0, 1))
    out.append(local_case("ratio_test", frame("tum", kps), pts, reach=dict(nm_min=len(match)),
                          expect=dict(match=match, nm=len(match))))
    return out


def _taken_variants(name, fr, pts, reach, **extra):
    n = len(fr["kun"])
    return [local_case(f"{name}_no_taken", fr, pts, taken=None, reach=reach, **extra),
            local_case(f"{name}_taken_seams", fr, pts, taken=_taken_seams(n), reach=dict(reach, taken="seams"),
                       **extra),
            local_case(f"{name}_taken_all", fr, pts, taken=np.ones(n, np.uint8), reach=dict(taken="all"),
                       expect=dict(match={}, nm=0), **extra)]


def local_count_cases():
    out = []
    # point counts: two points per site, two keypoints per site (octaves 1 and 0 keep the pair past the ratio test)
    for n in (15, 16, 17, 63, 64, 65, 127, 128, 129):
        s = lattice(-(-n // 2))
        fr = frame("tum", [(x + 2 * j, y, 1 - j, 0.0, 3 + 6 * j) for x, y in s for j in range(2)])
        pts = [local_point("tum", s[i // 2][0], s[i // 2][1], 2.0, 1) for i in range(n)]
        out.append(local_case(f"local_points_{n}", fr, pts, reach=dict(nm_min=n - 1)))
    out.append(dict(out[-1], name="local_points_129_max_points_100", max_points=100, reach=dict(nm_min=99)))
    # keypoint counts, with the taken flags absent, on the loader's word seams and all set
    for n_kp in KP_COUNTS:
        fr, s = _kp_frame(n_kp)
        sites = list(range(n_kp - 1, max(n_kp - 41, -1), -1))
        pts = [local_point("tum", s[k][0], s[k][1], 2.0, 1) for k in sites]
        out += _taken_variants(f"local_keypoints_{n_kp}", fr, pts, dict(nm_min=1 if n_kp > 2 else 0))
    # dense cells: every point takes the next keypoint by distance and re-scans once the kept keys are used up; with
    # the 21st keypoint of that order taken as well, its neighbours share an octave and the ratio test stops the rest
    for n_kp, n_pts in ((65, 40), (200, 129), (513, 129)):
        for layout in ("cell", "corner"):
            fr, (cx, cy), order = dense_frame(n_kp, layout, alternate_octaves=True)
            pts = [local_point("tum", cx, cy, 2.0, 1) for _ in range(n_pts)]
            out += _taken_variants(f"local_dense_{n_kp}_{layout}", fr, pts, dict(rescan=True, nm_min=n_pts - 8))[:2]
            broken = _taken_seams(n_kp)
            broken[order[20]] = 1
            out.append(local_case(f"local_dense_{n_kp}_{layout}_taken_break", fr, pts, taken=broken,
                                  reach=dict(rescan=True, nm_min=8, nm_max=20)))
    return out


def seen_cases():
    """Points the frame already tracks (their seen stamp equals the frame's) are skipped before isInFrustum.  Two
    frames of one batch read one table through different seen_offsets.  The referee is the oracle on a copy of the
    list with the stamped points mirrored behind the camera: in_view 0, no window, the other indices unchanged."""
    q = rendered()
    n = len(q["LP"])
    ids = np.arange(n, dtype=np.int32)
    m, _, _ = OM.search_local_points(q["lfr"], q["LP"], q["kun"], q["desc"], q["ur"], q["go"], q["gi"], q["geo"],
                                     taken=q["taken"])
    matched = np.sort(m[m >= 0])     # the stamped points are chosen among those that match when not stamped
    stamp, off_b = 7, n + 8
    table = np.zeros(2 * n + 16, np.int32)
    table[matched[::3]] = stamp              # frame a: every third matched point
    table[matched[2::3]] = stamp + 1         # another frame's stamp: not seen
    table[off_b + matched[1::4]] = stamp     # frame b, through its own offset into the same table
    out = []
    for tag, off in (("a", 0), ("b", off_b)):
        LP = q["LP"].copy()
        LP["id"] = ids
        lfr = q["lfr"].copy()
        lfr["seen_offset"], lfr["stamp"] = off, stamp
        out.append(_derived(f"seen_{tag}", "local", lfr=lfr, LP=LP, seen=table[off + ids] == stamp, seen_table=table,
                            reach=dict(seen=True)))
    return out


def seen_referee_points(case):
    """The list the oracle referees a seen case on: the stamped points mirrored through the camera centre."""
    LP = case["LP"].copy()
    T = case["lfr"]["Tcw"].reshape(4, 4).astype(np.float64)
    Ow = -T[:3, :3].T @ T[:3, 3]
    LP["xw"][case["seen"]] = (2 * Ow - LP["xw"][case["seen"]].astype(np.float64)).astype(np.float32)
    return LP


def derived_local_cases():
    """The probe's construction on the rendered local problem: mirror through the camera centre, shift sideways,
    scale the distance range, flip the normal -- one rejection per point in turn, every sixth point left alone."""
    q = rendered()
    LP = q["LP"].copy()
    T = q["lfr"]["Tcw"].reshape(4, 4).astype(np.float64)
    R, Ow = T[:3, :3], -T[:3, :3].T @ T[:3, 3]
    i = np.arange(len(LP))
    LP["xw"][i % 6 == 1] = (2 * Ow - LP["xw"][i % 6 == 1]).astype(np.float32)
    LP["xw"][i % 6 == 2] += (R.T @ np.array([6.0, 0.0, 0.0])).astype(np.float32)
    LP["min_dist"][i % 6 == 3] *= 4.0
    LP["max_dist"][i % 6 == 3] *= 4.0
    LP["min_dist"][i % 6 == 4] *= 0.2
    LP["max_dist"][i % 6 == 4] *= 0.2
    LP["normal"][i % 6 == 5] *= -1.0
    return [_derived("rendered_frustum_mixed", "local", LP=LP,
                     reach=dict(in_view_mixed=True, reasons={"behind", "right", "near", "far", "view_cos"})),
            _derived("rendered_frustum_mixed_no_taken", "local", LP=LP, taken=None, reach=dict(in_view_mixed=True))]


def second_geometry_local_cases():
    out = []
    for geom in ("barrel", "small"):
        out += frustum_cases(geom)[-1:] + scale_cases(geom)
    return out


LOCAL_GROUPS = {
    "frustum": lambda: frustum_cases() + derived_local_cases(),
    "scale_radius_ratio": lambda: scale_cases("tum") + radius_and_ratio_cases(),
    "counts": local_count_cases,
    "second_geometry": second_geometry_local_cases,
    "seen": seen_cases,
}


@functools.lru_cache(None)
def local_group(name):
    return LOCAL_GROUPS[name]()


def local_cases():
    cases = [c for name in LOCAL_GROUPS for c in local_group(name)]
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


# ------------------------------------------------------------------------------------------------ oracle and reach
def effective(case):
    """The record and list the expectation is computed on: a batch call's max_points cuts the list."""
    fr_key, pts_key = ("fr", "P") if case["kind"] == "proj" else ("lfr", "LP")
    fr, P = case[fr_key], case[pts_key]
    if case.get("seen") is not None:
        P = seen_referee_points(case)
    if "max_points" in case:
        fr, P = fr.copy(), P[:case["max_points"]]
        fr["n_points"] = len(P)
    return fr, P


def oracle(case, with_taken=True):
    """The oracle's result on a case: (match, nmatches, passes) or (match, nmatches, in_view)."""
    G = GEOMS[case["geom"]]
    fr, P = effective(case)
    cur = (case["kun"], case["desc"], case["ur"], case["go"], case["gi"], case["geo"])
    if case["kind"] == "proj":
        return OM.search_by_projection(fr, P, *cur, params=case["params"])
    return OM.search_local_points(fr, P, *cur, taken=case["taken"] if with_taken else None, params=case["params"][:3],
                                  scale_factor=G["scale_factor"], n_levels=G["nlevels"])


def rescans(keys, n_keys, local):
    """Whether a point with these candidate keys (distance, scan position, held), sorted, finds its n_keys kept keys
    used up when it is walked: frame to frame all of them held; local search fewer than two of them free."""
    if len(keys) < n_keys:
        return False
    free = sum(1 for _, _, held in keys[:n_keys] if not held)
    return free < 2 if local else free == 0
