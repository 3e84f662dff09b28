"""Shared pieces of the ORB extractor tests: the byte-identity comparisons against
oracle_ctypes.OrbOracle (final keypoints, descriptors, every per-level stage), the
geometry / parameter case table of tests/test_gpu_orb_geometry.py with its input
images, and the child-process entry of the launch-shape variants (run as a script).

The case table is data only; what each case is there for is asserted by the GPU
test from the extractor's own level_size() / tables() / max_kp, and
tests/test_oracle_orb_geometry.py keeps the table non-degenerate on the CPU."""
import functools
import math
import pathlib
import re
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
EDGE = 19          # EDGE_THRESHOLD, src/ORBextractor.cc:74
MIN_BORDER = EDGE - 3
TILE_W, TILE_H = 64, 32   # level_kernel output tile (orb_geom.h kLevelTileW / kLevelTileH)
SMALL_LEVEL_TILES = 128   # orb_kernels.hip kSmallLevelTiles


def assert_kps_equal(a, b, what):
    assert len(a) == len(b), f"{what}: count {len(a)} vs {len(b)}"
    for f in KP_FIELDS:
        bad = np.nonzero(a[f] != b[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at {bad[:10]} ({a[f][bad[:3]]} vs {b[f][bad[:3]]})"


def assert_extract_equal(kg, dg, ko, do, what):
    """Final keypoints (all seven fields) and descriptors, byte identity."""
    assert_kps_equal(kg, ko, what)
    assert dg.shape == do.shape, f"{what}: descriptor shape {dg.shape} vs {do.shape}"
    assert np.array_equal(dg, do), f"{what}: descriptors differ in {np.nonzero((dg != do).any(1))[0][:10]}"


def oracle_level(oracle, level):
    """(pyramid level, blurred level, FAST candidates, octree output) of an oracle that has seen an image."""
    return (oracle.level_image(level), oracle.level_blurred(level), oracle.level_candidates(level),
            oracle.level_keypoints(level))


def assert_level_stages_equal(got, ref, level, what=""):
    """One level's four stages as debug_stage returns them against oracle_level()'s, byte identity."""
    (pyr, blur, cand, oct_), (po, bo, co, ko) = got, ref
    assert pyr.shape == po.shape, f"{what}pyramid L{level}: {pyr.shape} vs {po.shape}"
    assert np.array_equal(pyr, po), f"{what}pyramid L{level}"
    assert np.array_equal(blur, bo), f"{what}blur L{level}"
    assert len(cand) == len(co), f"{what}candidates L{level}: {len(cand)} vs {len(co)}"
    for f in ("x", "y", "response"):
        assert np.array_equal(cand[f], co[f]), f"{what}candidates L{level} field {f}"
    assert len(oct_) == len(ko), f"{what}octree L{level}: {len(oct_)} vs {len(ko)}"
    for f in ("x", "y", "response", "octave", "size"):
        assert np.array_equal(oct_[f], ko[f]), f"{what}octree L{level} field {f}"


def assert_stages_equal(gpu, oracle, nlevels=8, frame=0, what=""):
    """Pyramid level, blurred level, FAST candidates and octree output of every level of `frame` of the
    extractor's last call against the oracle's (which has run pyramid() or extract() on the same image)."""
    for level in range(nlevels):
        assert_level_stages_equal([gpu.debug_stage(frame, level, s) for s in range(4)], oracle_level(oracle, level),
                                  level, what)


# ---------------------------------------------------------------------------
# Geometry restated from the extractor's own level sizes (never from the table below).

def n_ini(w, h):
    """Initial DistributeOctTree nodes of a w x h level: round(width / height) of the bordered area (:542)."""
    return int(math.floor((w - 2 * MIN_BORDER) / (h - 2 * MIN_BORDER) + 0.5))


def cell_grid(w, h):
    """(nCols, nRows, wCell, hCell) of a level's FAST cells (:769-787)."""
    width, height = float(w - 2 * MIN_BORDER), float(h - 2 * MIN_BORDER)
    ncols, nrows = int(width / 30), int(height / 30)
    return ncols, nrows, math.ceil(width / ncols), math.ceil(height / nrows)


def level_tiles(w, h):
    return -(-w // TILE_W) * -(-h // TILE_H)


def small_level_start(sizes):
    """First of the levels the launcher counts as small (orb_launch): the trailing levels with at most
    SMALL_LEVEL_TILES tiles together, at least two of them, never level 0; len(sizes) if there are none."""
    n = len(sizes)
    ls, tiles = n, 0
    while ls > 1 and tiles + level_tiles(*sizes[ls - 1]) <= SMALL_LEVEL_TILES:
        ls -= 1
        tiles += level_tiles(*sizes[ls])
    return n if n - ls < 2 else ls


def cell_cap():
    """kCellCap of the kernels' geometry header."""
    text = (ROOT / "sp-slam_amd" / "csrc" / "orb_geom.h").read_text()
    return int(re.search(r"constexpr int kCellCap = (\d+);", text).group(1))


# ---------------------------------------------------------------------------
# Images.  Each is built once per process and handed out read-only.

def _frozen(a):
    a = np.ascontiguousarray(a, np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def render(w, h):
    import synth
    sc = synth.Scene(0)
    return _frozen(sc.render(sc.pose(3), w, h, noise_seed=3)[0])


@functools.lru_cache(maxsize=None)
def noise(w, h, seed=5):
    return _frozen(np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def periodic(w, h):
    """A 37 x 41 random tile repeated: most keypoints share octave and response with another one."""
    tile = np.random.default_rng(11).integers(0, 256, (41, 37), dtype=np.uint8)
    return _frozen(np.tile(tile, (h // 41 + 1, w // 37 + 1))[:h, :w])


@functools.lru_cache(maxsize=None)
def checkerboard(w, h):
    """0 / 255 blocks of 11 x 9 pixels: blur and resize saturate; straight edges and X junctions only."""
    yy, xx = np.mgrid[0:h, 0:w]
    return _frozen(((xx // 11 + yy // 9) % 2) * 255)


@functools.lru_cache(maxsize=None)
def half_constant(w, h):
    g = render(w, h).copy()
    g[:, :600] = 90
    return _frozen(g)


DOTS = ((19, 19), (313, 19), (19, 226), (313, 226), (16, 16), (166, 123), (166, 18))


@functools.lru_cache(maxsize=None)
def dots(w, h):
    """3 x 3 bright dots on a constant frame, at and just inside the keypoint border."""
    g = np.full((h, w), 60, np.uint8)
    for x, y in DOTS:
        g[y - 1:y + 2, x - 1:x + 2] = 255
    return _frozen(g)


@functools.lru_cache(maxsize=None)
def constant(w, h):
    return _frozen(np.full((h, w), 128, np.uint8))


IMAGES = {"render": render, "noise": noise, "noise_seed8": functools.partial(noise, seed=8), "periodic": periodic,
          "checkerboard": checkerboard, "half_constant": half_constant, "dots": dots, "constant": constant}


# ---------------------------------------------------------------------------
# The case table.  `levels` = the levels the case claims yield keypoints (None: all of them).

def case(w, h, nfeatures, scale=1.2, nlevels=8, ini=20, mn=7, image="render", levels=None, min_kps=None):
    return dict(width=w, height=h, nfeatures=nfeatures, scale_factor=scale, nlevels=nlevels, ini_th_fast=ini,
                min_th_fast=mn, image=image, levels=tuple(range(nlevels)) if levels is None else tuple(levels),
                min_kps=nfeatures if min_kps is None else min_kps)


GEOMETRY_CASES = {                                    # section A of the test module
    "odd_641x481": case(641, 481, 1000),
    "small_333x246": case(333, 246, 500),
    "wide_754x480": case(754, 480, 1200),
    "tall_257x259": case(257, 259, 300, nlevels=5),
    "scale_1p5": case(640, 480, 1000, scale=1.5, nlevels=5),
    "scale_2p0": case(640, 480, 1000, scale=2.0, nlevels=3),
    "scale_1p05": case(640, 480, 1000, scale=1.05),
    "pano_1000x230": case(1000, 230, 700),
    "one_level": case(640, 480, 1000, nlevels=1),
    "min_127x96": case(127, 96, 100, nlevels=1),
    "min_64x64": case(64, 64, 50, nlevels=1),
}

CONTENT_CASES = {                                     # section C
    "periodic": case(641, 481, 1000, image="periodic"),
    "checkerboard": case(333, 246, 500, image="checkerboard", levels=range(1, 8), min_kps=300),
    "noise_th_1_1": case(333, 246, 500, ini=1, mn=1, image="noise"),
    "noise_th_100_100": case(333, 246, 500, ini=100, mn=100, image="noise", levels=(0, 1, 2), min_kps=100),
    "noise_th_7_20": case(333, 246, 500, ini=7, mn=20, image="noise"),
    "noise_th_254_200": case(333, 246, 500, ini=254, mn=200, image="noise_seed8", levels=(0,), min_kps=1),
    "half_constant_pano": case(1000, 230, 700, image="half_constant", min_kps=300),
    "border_dots": case(333, 246, 500, image="dots", levels=(), min_kps=1),
}

REJECTED = {                                          # spslam_create refuses these
    "level_below_one_cell": (dict(width=333, height=77, nlevels=8), "smaller than one FAST cell"),
    "aspect_ratio": (dict(width=2000, height=100, nlevels=1), "aspect ratio"),
    "octree_capacity": (dict(width=640, height=480, nfeatures=1100, nlevels=1), "node capacity"),
    "below_64": (dict(width=63, height=64), None),            # refused before the geometry is built
    # level 6 is 112 x 84: one 40 x 52 cell row, whose 20 * 26 possible NMS survivors exceed kCellCap = 512
    "cell_survivor_bound": (dict(width=333, height=250, nfeatures=500, nlevels=8), "kCellCap"),
}


def case_image(c):
    return IMAGES[c["image"]](c["width"], c["height"])


def extractor_args(c, **extra):
    return dict({k: c[k] for k in ("nfeatures", "scale_factor", "nlevels", "ini_th_fast", "min_th_fast", "width",
                                   "height")}, **extra)


def oracle_for(c):
    import oracle_ctypes
    return oracle_ctypes.OrbOracle(c["nfeatures"], c["scale_factor"], c["nlevels"], c["ini_th_fast"],
                                   c["min_th_fast"])


# ---------------------------------------------------------------------------
# Batched device entry on torch buffers, outputs pre-filled with a sentinel byte.

SENTINEL = 0xA5


def embed(frames, stride, base_offset=0, frame_stride=None, fill=None):
    """The frames (equal-sized 2-D u8 arrays) laid out in one byte buffer: frame f's row r starts at
    base_offset + f * frame_stride + r * stride.  Every byte that is no pixel holds `fill` (default: 0xEC and
    0x13 in turn, so one of the two bytes past any border pixel differs from it by more than 108): a read
    past a row's end changes the result.  Returns (buffer, frame_stride); the buffer ends stride bytes after the
    last row's start."""
    h, w = frames[0].shape
    assert stride >= w
    fs = stride * h if frame_stride is None else frame_stride
    assert fs >= stride * h
    n = len(frames)
    buf = np.empty(base_offset + (n - 1) * fs + stride * h, np.uint8)
    if fill is None:
        buf[:] = np.where(np.arange(buf.size) & 1, 0x13, 0xEC)
    else:
        buf[:] = fill
    for f, g in enumerate(frames):
        assert g.shape == (h, w)
        o = base_offset + f * fs
        view = np.lib.stride_tricks.as_strided(buf[o:], (h, w), (stride, 1))
        view[:] = g
    return buf, fs


def run_batch(ex, buf, n_frames, frame_stride, stride, base_offset=0, cap=None):
    """extract_batch_device on a copy of `buf` in device memory.  Returns (kps, desc, counts): the raw output
    buffers as host arrays, (n_frames * cap + 1) keypoint / descriptor slots and max_batch counts, every byte
    SENTINEL where the extractor wrote nothing."""
    import torch
    import spslam_gpu
    cap = ex.max_kp if cap is None else cap
    slots = n_frames * cap + 1
    dev = torch.from_numpy(np.array(buf)).cuda()
    kps = torch.full((slots * spslam_gpu.KEYPOINT_DTYPE.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda")
    desc = torch.full((slots * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    cnt = torch.full((ex.params.max_batch * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 256 == 0   # the allocation itself is aligned; base_offset decides the image's
    stream = torch.cuda.current_stream().cuda_stream
    ex.extract_batch_device(dev.data_ptr() + base_offset, n_frames, frame_stride, stride, kps.data_ptr(),
                            desc.data_ptr(), cnt.data_ptr(), cap, stream)
    torch.cuda.synchronize()
    return (kps.cpu().numpy().view(spslam_gpu.KEYPOINT_DTYPE), desc.cpu().numpy().reshape(slots, 32),
            cnt.cpu().numpy().view(np.int32))


def assert_batch_equal(kps, desc, counts, expected, cap, what):
    """Frame f's output equals expected[f] = (keypoints, descriptors) cut at cap; every output byte outside
    [f * cap, f * cap + counts[f]) and every count past the batch still holds the sentinel."""
    n = len(expected)
    written = np.zeros(len(kps), bool)
    for f, (ko, do) in enumerate(expected):
        m = min(len(ko), cap)
        assert counts[f] == m, f"{what} frame {f}: count {counts[f]} vs {m}"
        assert_extract_equal(kps[f * cap:f * cap + m], desc[f * cap:f * cap + m], ko[:m], do[:m], f"{what} frame {f}")
        written[f * cap:f * cap + m] = True
    assert np.all(counts.view(np.uint8)[4 * n:] == SENTINEL), f"{what}: a count past the batch was written"
    kb = kps.view(np.uint8).reshape(len(kps), -1)
    for label, a in (("keypoint", kb), ("descriptor", desc)):
        stray = np.nonzero((a != SENTINEL).any(1) & ~written)[0]
        assert stray.size == 0, f"{what}: {label} slots {stray[:10]} written"


# ---------------------------------------------------------------------------
# Child process of the launch-shape variants: python orb_common.py <in.npz> <out.npz>.  The switches are
# environment variables read once per process, so each variant is a fresh interpreter.  For every case of the
# input it extracts the case's frames in one batched call and stores the outputs and every stage.

def variant_frames(c):
    """The three frames a variant child extracts for a case: the case's image, noise, the image upside down."""
    g = case_image(c)
    return [g, noise(c["width"], c["height"]), _frozen(g[::-1])]


def _child(src, dst):
    for p in (ROOT / "sp-slam_amd",):
        sys.path.insert(0, str(p))
    import spslam_gpu
    data = np.load(src, allow_pickle=False)
    out = {}
    for name in [str(s) for s in data["names"]]:
        frames = data[f"{name}/frames"]
        n, h, w = frames.shape
        p = data[f"{name}/params"]
        ex = spslam_gpu.OrbExtractor(nfeatures=int(p[0]), scale_factor=float(p[1]), nlevels=int(p[2]),
                                     ini_th_fast=int(p[3]), min_th_fast=int(p[4]), width=w, height=h, max_batch=n)
        try:
            kps, desc, cnt = run_batch(ex, frames.reshape(-1), n, w * h, w)
            out[f"{name}/kps"], out[f"{name}/desc"], out[f"{name}/counts"] = kps, desc, cnt
            out[f"{name}/cap"] = np.array(ex.max_kp)
            for f in range(n):
                for level in range(int(p[2])):
                    for s in range(4):
                        out[f"{name}/f{f}/l{level}/s{s}"] = ex.debug_stage(f, level, s)
        finally:
            ex.close()
    np.savez(dst, **out)
    print("orb variant child: " + " ".join(f"{k}={out[k + '/counts'].tolist()}" for k in map(str, data["names"])))


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
