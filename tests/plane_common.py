"""Shared by the plane-extraction tests: the comparison with the CPU oracle, the case tables of
test_gpu_plane_geometry.py / test_oracle_plane_cases.py, their depth images, the batched device entry on
sentinel-filled torch buffers, and (run as a script) the child process of the opt-in launch shapes.

Bar of every comparison (test_gpu_planes.py's): organized cloud, chamfer distance map and normals bit-equal with
equal NaN positions; connected-component labels equal; plane count equal; coefficients bit-equal; inlier and
contour index lists equal.
"""
import functools
import pathlib
import sys

import numpy as np

COEF_TOL = 1e-4
SENTINEL = 0x5A5A5A5A   # int32 fill of the output buffers
ORB_SMALL = dict(width=128, height=96, nfeatures=100, nlevels=1)   # an OrbExtractor whose own buffers stay small


def intrinsics(name="tum3", scale=1.0):
    import synth
    K = {"tum3": synth.TUM3, "icl": synth.ICL}[name]
    return tuple(K[k] * scale for k in ("fx", "fy", "cx", "cy"))


def oracle(depth, scale=1.0, min_size=500, cloud_dis=3, angle_threshold=3.0, distance_threshold=0.05, K="tum3"):
    """(PlaneOracle, its result) of one depth image; width and height are the image's."""
    import oracle_planes
    po = oracle_planes.PlaneOracle()
    res = po.extract(depth, *intrinsics(K, scale), cloud_dis=cloud_dis, min_size=min_size, angle_th=angle_threshold,
                     dist_th=distance_threshold)
    return po, res


def assert_stages_equal(stages, po, what):
    """stages = (cloud, normals, distance map, labels) of the device against the oracle's."""
    cloud, ng, dist, labels = stages
    assert np.array_equal(cloud, po.cloud(), equal_nan=True), f"{what}: cloud"
    assert np.array_equal(dist, po.distance(), equal_nan=True), f"{what}: distance map"
    no = po.normals()
    assert np.array_equal(np.isnan(ng), np.isnan(no)), f"{what}: normal validity"
    m = ~np.isnan(no)
    assert np.array_equal(ng[m], no[m]), f"{what}: normals"
    assert np.array_equal(labels, po.labels(False)), f"{what}: CC labels"


def assert_planes_equal(rg, ro, what):
    assert len(rg["coef"]) == len(ro["coef"]), f"{what}: {len(rg['coef'])} vs {len(ro['coef'])} planes"
    for j in range(len(ro["coef"])):
        assert np.abs(rg["coef"][j] - ro["coef"][j]).max() <= COEF_TOL * max(1.0, abs(ro["coef"][j][3])), \
            f"{what} plane {j}: {rg['coef'][j]} vs {ro['coef'][j]}"
        assert np.array_equal(rg["coef"][j], ro["coef"][j]), f"{what} plane {j}: coef not bit-exact"
        assert np.array_equal(rg["inliers"][j], ro["inliers"][j]), f"{what} plane {j}: inliers"
        assert np.array_equal(rg["contour"][j], ro["contour"][j]), f"{what} plane {j}: contour"


def device_stages(pe, frame=0):
    return tuple(pe.debug(frame, what) for what in (0, 1, 2, 3))


def compare(pe, depth, k, scale=1.0, min_size=500, expected=None, **params):
    """Every stage and output of one frame against the oracle; returns (#planes, #models).
    expected = (po, ro) reuses an oracle run of the same depth and parameters."""
    po, ro = expected or oracle(depth, scale, min_size, **params)
    rg = pe(depth)
    assert_stages_equal(device_stages(pe), po, f"frame {k}")
    assert_planes_equal(rg, ro, f"frame {k}")
    return len(ro["coef"]), po.n_models


def refine_path(n_models):
    """Which refinement the kernel takes (plane_segment.hip phase K): fast narrow (<= 14 models, 16-bit
    descriptors), fast wide (<= 30, 32-bit descriptors) or the general 64-bit path."""
    return "narrow" if n_models <= 14 else "wide" if n_models <= 30 else "general"


def big_components(po, min_size):
    """Connected components larger than MinSize: labels(False) counted over the valid points."""
    lab = po.labels(False)
    valid = np.isfinite(po.cloud()[:, 2]) & (lab != 0xFFFFFFFF)
    return int((np.bincount(lab[valid].astype(np.int64)) > min_size).sum())


# ---------------------------------------------------------------------------
# Depth images.  Renders are cached: several cases crop the same frame.

@functools.lru_cache(maxsize=None)
def render(seq, frame, boxes, w=640, h=480):
    import oracle_planes
    import synth
    sc = synth.Scene(seq, n_boxes=boxes)
    d = oracle_planes.depth_to_float(sc.render(sc.pose(frame), w, h, noise_seed=frame)[1])
    d.setflags(write=False)
    return d


def crop(d, x, y, w, h):
    assert 0 <= x and x + w <= d.shape[1] and 0 <= y and y + h <= d.shape[0]
    return np.ascontiguousarray(d[y:y + h, x:x + w])


def wall(w, h, z=2.0):
    return np.full((h, w), z, np.float32)


def slope(w=640, h=480):
    """One smooth tilted surface, 1.5 m to 2.3 m."""
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return (1.5 + 0.8 * x / w + 0.2 * y / h).astype(np.float32)


def banded(fill, w=640, h=480):
    """slope() cut in two by a horizontal band of `fill` 30 rows high."""
    d = slope(w, h)
    d[h // 2 - 15:h // 2 + 15] = fill
    return d


def facets(nx, ny, w=640, h=480, seed=7):
    """nx x ny tilted facets: each its own plane, offset in depth from its neighbours by more than the
    depth-change threshold so that no component spans two facets."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    fx, fy = np.minimum((x * nx / w).astype(int), nx - 1), np.minimum((y * ny / h).astype(int), ny - 1)
    base = 1.2 + 0.45 * ((fx + 2 * fy) % 4) + 0.03 * rng.random((ny, nx))[fy, fx]
    sx, sy = rng.uniform(-0.5, 0.5, (2, ny, nx))
    u, v = x * nx / w - fx - 0.5, y * ny / h - fy - 0.5
    return (base + 0.15 * (sx[fy, fx] * u + sy[fy, fx] * v)).astype(np.float32)


def punched(d, nan=True, inf=True):
    """d with a NaN band six rows high across its left half and a +Inf block of 9 x 18 samples in its right half
    (every Cloud.Dis up to 5 samples both): the gradients beside them are the elements IntegralImage2D leaves out."""
    d = d.copy()
    h, w = d.shape
    if nan:
        d[h // 2:h // 2 + 6, :w // 2] = np.nan
    if inf:
        d[h // 5:h // 5 + 9, w // 2:w // 2 + 18] = np.inf
    return d


def far_to(value, seq=1, frame=5, boxes=3, limit=2.5):
    d = render(seq, frame, boxes).copy()
    far = d > limit
    assert far.any() and (~far).any()
    d[far] = value if value is not None else -d[far]
    return d


# ---------------------------------------------------------------------------
# Case tables.  depth: a callable without arguments.  expect: the launch the case is there for, as the fields of
# PlaneExtractor.launch_shape() it pins (lds = segmentation maps in LDS, k = row positions per lane, nw = waves of
# the wave kernels).  planes / models: what the oracle finds (asserted by test_oracle_plane_cases.py).

def case(depth, dis, min_size, lds, k, nw, planes, models, K="tum3", scale=1.0, angle_threshold=3.0,
         distance_threshold=0.05, path=None):
    return dict(depth=depth, cloud_dis=dis, min_size=min_size, lds=lds, k=k, nw=nw, planes=planes, models=models,
                K=K, scale=scale, angle_threshold=angle_threshold, distance_threshold=distance_threshold, path=path)


def oracle_params(c):
    return dict(scale=c["scale"], min_size=c["min_size"], cloud_dis=c["cloud_dis"], K=c["K"],
                angle_threshold=c["angle_threshold"], distance_threshold=c["distance_threshold"])


def cloud_size(c, d=None):
    d = c["depth"]() if d is None else d
    return -(-d.shape[1] // c["cloud_dis"]), -(-d.shape[0] // c["cloud_dis"])


def _r640(seq=0, frame=20, boxes=3):
    return lambda: render(seq, frame, boxes)


def _c640(x, y, w, h, seq=0, frame=20, boxes=3):
    return lambda: crop(render(seq, frame, boxes), x, y, w, h)


def _doubled(x, y, w, h):
    """A w x h window with every sample repeated 2 x 2: Cloud.Dis 2 reads each of the window's samples once."""
    return lambda: np.ascontiguousarray(np.kron(crop(render(0, 20, 3), x, y, w, h), np.ones((2, 2), np.float32)))


def _transposed(x, y, w, h):
    return lambda: np.ascontiguousarray(crop(render(0, 20, 3), x, y, w, h).T)


GEOMETRY_CASES = {
    # name: depth, Cloud.Dis, MinSize, LDS maps, K, NW, oracle planes, models                     # cloud W x H
    "wide_lds_300x100": case(_c640(20, 200, 600, 200), 2, 200, True, 8, 2, 3, 5),                # 300 x 100
    "large_narrow_200x200": case(_c640(120, 40, 400, 400), 2, 500, False, 4, 4, 2, 2),           # 200 x 200
    "large_narrow_256x160": case(_c640(192, 160, 256, 160), 1, 500, False, 4, 3, 2, 2),          # 256 x 160
    "w256": case(_c640(64, 120, 512, 240), 2, 300, True, 4, 2, 3, 4),                            # 256 x 120
    "w257": case(_c640(63, 120, 514, 240), 2, 300, True, 8, 2, 3, 4),                            # 257 x 120
    "w512": case(_doubled(64, 200, 512, 96), 2, 300, False, 8, 2, 2, 3, scale=2.0),              # 512 x 96
    "w63": case(_c640(300, 200, 63, 100), 1, 100, True, 4, 2, 1, 1),                             # 63 x 100
    "w64": case(_c640(300, 200, 64, 100), 1, 100, True, 4, 2, 1, 1),                             # 64 x 100
    "w65": case(_c640(300, 200, 65, 100), 1, 100, True, 4, 2, 1, 1),                             # 65 x 100
    "h64": case(_c640(220, 208, 200, 64), 1, 200, True, 4, 1, 1, 1),                             # 200 x 64
    "h65": case(_c640(220, 208, 200, 65), 1, 200, True, 4, 2, 1, 1),                             # 200 x 65
    "h128": case(_c640(245, 176, 150, 128), 1, 200, True, 4, 2, 1, 1),                           # 150 x 128
    "h129": case(_c640(245, 176, 150, 129), 1, 200, True, 4, 3, 1, 1),                           # 150 x 129
    "h330": case(_c640(245, 0, 150, 330), 1, 200, False, 4, 6, 2, 2),                            # 150 x 330
    "h65_indivisible": case(_c640(120, 143, 400, 193), 3, 200, True, 4, 2, 1, 1),                # 134 x 65
    "tall_100x512": case(_transposed(64, 200, 512, 100), 1, 300, False, 4, 8, 2, 3),             # 100 x 512
    "tall_96x480": case(_c640(272, 0, 96, 480), 1, 300, False, 4, 8, 2, 2),                      # 96 x 480
    "dis2": case(_r640(), 2, 500, False, 8, 4, 3, 3),                                            # 320 x 240
    "dis4": case(_r640(), 4, 300, True, 4, 2, 3, 3),                                             # 160 x 120
    "dis5": case(_r640(), 5, 200, True, 4, 2, 2, 2),                                             # 128 x 96
    "patch_24x24": case(lambda: wall(24, 24), 1, 10, True, 4, 1, 1, 1),                          # 24 x 24: 575 inliers
}

# The oracle finds no valid normal (the estimator's border is 10 points) and so no plane; every stage is compared.
DEGENERATE_CASES = {
    "cloud_1x1": case(lambda: wall(1, 1), 1, 10, True, 4, 1, 0, 0),
    "cloud_2x3": case(lambda: crop(render(0, 20, 3), 300, 200, 4, 6), 2, 10, True, 4, 1, 0, 0),
    "cloud_7x5": case(lambda: crop(render(0, 20, 3), 300, 200, 20, 13), 3, 10, True, 4, 1, 0, 0),
    "cloud_16x16": case(lambda: wall(16, 16), 1, 10, True, 4, 1, 0, 0),
}

# 640 x 480 / Cloud.Dis 3: cloud 214 x 160, maps in LDS, K 4, NW 3.  The last two numbers: oracle planes, models.
CONTENT_CASES = {
    "wall": case(lambda: wall(640, 480), 3, 500, True, 4, 3, 1, 1),            # 34239 inliers, empty contour
    "zero_band": case(lambda: banded(0.0), 3, 500, True, 4, 3, 1, 2),          # PlaneNotSeen drops the second half
    "nan_band": case(lambda: banded(np.nan), 3, 500, True, 4, 3, 1, 2),
    # gradients next to the Inf / NaN points are not finite: IntegralImage2D leaves them out of its sums
    "far_inf": case(lambda: far_to(np.inf), 3, 500, True, 4, 3, 1, 1),
    "far_negated": case(lambda: far_to(None), 3, 500, True, 4, 3, 3, 3),
    "depth_x4": case(lambda: render(0, 20, 3) * np.float32(4), 3, 500, True, 4, 3, 3, 3),
    "icl": case(_r640(), 3, 500, True, 4, 3, 3, 3, K="icl"),
    "all_nan": case(lambda: wall(640, 480, np.nan), 3, 500, True, 4, 3, 0, 0),   # no planes expected
    "facets_8x6": case(lambda: facets(8, 6), 3, 100, True, 4, 3, 13, 47, path="general"),
    "tight_thresholds": case(_r640(), 3, 500, True, 4, 3, 2, 2, angle_threshold=1.5, distance_threshold=0.02),
    "loose_thresholds": case(_r640(), 3, 500, True, 4, 3, 3, 3, angle_threshold=6.0, distance_threshold=0.1),
}

# Past a limit (kMaxPlanesPerFrame = 64 models, kMaxBig = 255 components over MinSize): flags, no parity.
LIMIT_CASES = {
    "models_10x8": case(lambda: facets(10, 8), 3, 60, True, 4, 3, 20, 80),         # 80 components over MinSize
    "components_21x16": case(lambda: facets(21, 16), 3, 10, True, 4, 3, 54, 214),  # 266 components over MinSize
}
LIMIT_COMPONENTS = {"models_10x8": 80, "components_21x16": 266}
MAX_MODELS, MAX_COMPONENTS = 64, 255   # kMaxPlanesPerFrame, kMaxBig

# NaN and +Inf samples at the three heights of the opt-in launch shapes: regression cases of the integral images'
# non-finite elements in every kernel that makes them (the default launch runs them too).
def _punched_case(name, planes, models):
    base = GEOMETRY_CASES[name]
    return dict(base, depth=lambda: punched(base["depth"]()), planes=planes, models=models)


NONFINITE_CASES = {
    "h129_nonfinite": _punched_case("h129", 1, 1),
    "dis2_nonfinite": _punched_case("dis2", 3, 3),
    "tall_96x480_nonfinite": _punched_case("tall_96x480", 2, 2),
}

# Batches past the 16-frame threshold of the one-workgroup wave kernel: cloud 134 x 65 (NW 2) and 214 x 160 (NW 3).
BATCH_CASES = {
    "b17_h65": dict(case=case(None, 3, 200, True, 4, 2, None, None), window=(120, 143, 400, 193), frames=17),
    "b17_h160": dict(case=case(None, 3, 500, True, 4, 3, None, None), window=(0, 0, 640, 480), frames=17),
    "b40_h65": dict(case=case(None, 3, 200, True, 4, 2, None, None), window=(120, 143, 400, 193), frames=40),
}


def batch_frames(b):
    """Frames from two renders through one window, mirrored left-right and top-bottom and scaled in depth by
    1, 1.05, 1.1, ...: no two alike.  Frames 3, 11, ... carry punched()'s NaN band and frames 5, 13, ... its +Inf
    block, so the one-workgroup wave kernel meets non-finite gradients."""
    base = [crop(render(0, 20, 3), *b["window"]), crop(render(1, 5, 3), *b["window"])]
    out = []
    for f in range(b["frames"]):
        d, k = base[f % 2], f // 2
        d = d[:, ::-1] if k & 1 else d
        d = d[::-1] if k & 2 else d
        d = np.ascontiguousarray(d * np.float32(1 + 0.05 * (k >> 2)))
        out.append(punched(d, nan=f % 8 == 3, inf=f % 8 == 5) if f % 8 in (3, 5) else d)
    return out


def batch_nonfinite(frames):
    """(indices of the frames with NaN samples, with +Inf samples)."""
    return ([f for f, d in enumerate(frames) if np.isnan(d).any()], [f for f, d in enumerate(frames) if np.isposinf(d).any()])


# Opt-in launch shapes: H <= 192, 192 < H <= 320 and H > 320 (plane_dist_integral_kernel's three instances), and for
# the wave kernels' one- and three-workgroup shapes NW 1 (h64: no ring above or below) and NW 6 (h330: 10 rows in the
# last wave).
VARIANT_CASES = (("geometry", "h129"), ("geometry", "dis2"), ("geometry", "tall_96x480"),
                 ("nonfinite", "h129_nonfinite"), ("nonfinite", "dis2_nonfinite"),
                 ("nonfinite", "tall_96x480_nonfinite"), ("geometry", "h64"), ("geometry", "h330"))
VARIANT_ROWS = {"h129": 192, "dis2": 320, "tall_96x480": 512, "h129_nonfinite": 192, "dis2_nonfinite": 320,
                "tall_96x480_nonfinite": 512, "h64": 192, "h330": 512}
VARIANTS = {"one_workgroup": {"SPSLAM_PLANE_WAVE": "1"}, "three_workgroups": {"SPSLAM_PLANE_WAVE": "3"},
            "barrier": {"SPSLAM_PLANE_WAVE_BARRIER": "1"}}


TABLES = {"geometry": GEOMETRY_CASES, "degenerate": DEGENERATE_CASES, "content": CONTENT_CASES,
          "limit": LIMIT_CASES, "nonfinite": NONFINITE_CASES}


@functools.lru_cache(maxsize=None)
def expected(table, name):
    """(depth, PlaneOracle, result) of a case, computed once per process and left unchanged."""
    c = TABLES[table][name]
    d = c["depth"]()
    po, ro = oracle(d, **oracle_params(c))
    return d, po, ro


# ---------------------------------------------------------------------------
# Extractors and the batched device entry.

def plane_extractor(ex, c, w, h):
    import spslam_planes
    pe = spslam_planes.PlaneExtractor(ex, *intrinsics(c["K"], c["scale"]), w, h, cloud_dis=c["cloud_dis"],
                                      min_size=c["min_size"], angle_threshold=c["angle_threshold"],
                                      distance_threshold=c["distance_threshold"])
    pe.keep_labels()
    return pe


def assert_launch(pe, c, n_frames=1, one_workgroup=False):
    """The launch the case is there for, from the functions the launch itself dispatches on."""
    sh = pe.launch_shape(n_frames)
    want = dict(seg_maps_in_lds=int(c["lds"]), seg_positions=c["k"], wave_count=c["nw"],
                one_workgroup=int(one_workgroup), barrier_rows=0)
    assert sh == want, (sh, want)
    return sh


def embed(frames, stride, frame_stride=None, base_offset=0, fillers=(np.nan, 3.0e38)):
    """Frames laid out `stride` floats per row and `frame_stride` per frame from element `base_offset` of a
    64-byte aligned buffer; the row padding and the gaps between frames hold NaN and a large finite value in
    turn, so a read of either shows.  Returns (torch tensor on the device, frame stride)."""
    import torch
    h, w = frames[0].shape
    fs = frame_stride or stride * h
    assert stride >= w and fs >= stride * (h - 1) + w
    buf = np.empty(base_offset + fs * len(frames) + 16, np.float32)
    buf[0::2], buf[1::2] = fillers
    for f, d in enumerate(frames):
        rows = np.lib.stride_tricks.as_strided(buf[base_offset + f * fs:], (h, w), (stride * 4, 4))
        rows[:] = d
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 64 == 0
    return t, fs


def run_batch(pe, d_buf, n, frame_stride, stride, base_offset=0):
    """spslam_planes_extract_batch_device on sentinel-filled outputs with one spare frame slot at the end.
    Returns (planes [n + 1][planes_cap], counts [n + 1], inliers [n + 1][inlier_cap], contours [n + 1][contour_cap])."""
    import torch
    import spslam_planes
    words = spslam_planes.PLANE_DTYPE.itemsize // 4
    bufs = [torch.full(((n + 1) * m,), SENTINEL, dtype=torch.int32, device="cuda")
            for m in (pe.planes_cap * words, 1, pe.inlier_cap, pe.contour_cap)]
    pe.extract_batch_device(d_buf.data_ptr() + 4 * base_offset, n, frame_stride, stride,
                            *[b.data_ptr() for b in bufs], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    P, C, I, Cn = [b.cpu().numpy() for b in bufs]
    return (P.view(spslam_planes.PLANE_DTYPE).reshape(n + 1, pe.planes_cap), C, I.reshape(n + 1, -1),
            Cn.reshape(n + 1, -1))


def frame_result(P, C, I, Cn, f):
    """Frame f of run_batch's outputs in the oracle's form; checks that the lists tile the buffers from 0 and
    that nothing past the planes, inliers and contours they name was written."""
    n = int(C[f])
    assert 0 <= n <= P.shape[1], n
    out = dict(coef=[], inliers=[], contour=[])
    ni = nc = 0
    for p in P[f, :n]:
        assert p["inlier_offset"] == ni and p["contour_offset"] == nc and p["n_inliers"] >= 0 and p["n_contour"] >= 0
        ni, nc = ni + int(p["n_inliers"]), nc + int(p["n_contour"])
        assert ni <= I.shape[1] and nc <= Cn.shape[1], (ni, nc)
        out["coef"].append(p["coef"].copy())
        out["inliers"].append(I[f, ni - p["n_inliers"]:ni].copy())
        out["contour"].append(Cn[f, nc - p["n_contour"]:nc].copy())
    assert (P[f, n:].view(np.int32) == SENTINEL).all(), f"frame {f}: plane records past counts[f] written"
    assert (I[f, ni:] == SENTINEL).all(), f"frame {f}: inlier indices past the planes' lists written"
    assert (Cn[f, nc:] == SENTINEL).all(), f"frame {f}: contour indices past the planes' lists written"
    return out


def assert_spare_untouched(P, C, I, Cn):
    for a in (P[-1].view(np.int32), C[-1:], I[-1], Cn[-1]):
        assert (a == SENTINEL).all(), "the slot after the last frame was written"


# ---------------------------------------------------------------------------
# Child process of the opt-in launch shapes: python plane_common.py <out.npz>.  Runs VARIANT_CASES under the
# environment it was started with and saves launch shape, stages and outputs of each.

def _child(dst):
    root = pathlib.Path(__file__).resolve().parent.parent
    for p in (root / "sp-slam_amd", root / "oracle"):
        sys.path.insert(0, str(p))
    import spslam_gpu
    out = {}
    ex = spslam_gpu.OrbExtractor(**ORB_SMALL)
    try:
        for table, name in VARIANT_CASES:
            c = TABLES[table][name]
            d = c["depth"]()
            pe = plane_extractor(ex, c, d.shape[1], d.shape[0])
            sh = pe.launch_shape(1)
            out[f"{name}/shape"] = np.array([sh[k] for k in ("seg_maps_in_lds", "seg_positions", "wave_count",
                                                             "one_workgroup", "barrier_rows")], np.int32)
            rg = pe(d)
            for s, a in enumerate(device_stages(pe)):
                out[f"{name}/s{s}"] = a
            out[f"{name}/n"] = np.array(len(rg["coef"]))
            for j in range(len(rg["coef"])):
                for k in ("coef", "inliers", "contour"):
                    out[f"{name}/{k}{j}"] = rg[k][j]
    finally:
        ex.close()
    np.savez(dst, **out)


if __name__ == "__main__":
    _child(sys.argv[1])
