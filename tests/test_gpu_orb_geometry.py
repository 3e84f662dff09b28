"""GPU parity of the ORB extractor away from its two usual geometries: image sizes, strides, scale factors,
level counts, thresholds, batch layouts, output capacities, image contents and the opt-in launch shapes.

Bar as in test_gpu_orb.py: byte identity with oracle_ctypes.OrbOracle (same nfeatures, scale factor, levels,
thresholds) for every stage of every level, the final keypoints (all seven fields) and the descriptors.  The
cases and images live in orb_common.py; each case first asserts, from the extractor's own level_size() /
tables() / max_kp, the property it is there for, so an edit that makes a case degenerate fails loudly.
tests/test_oracle_orb_geometry.py keeps the same table non-degenerate with the oracle alone.
"""
import contextlib
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import orb_common as OC

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def extractor(c, **extra):
    import spslam_gpu
    ex = spslam_gpu.OrbExtractor(**OC.extractor_args(c, **extra))
    try:
        yield ex
    finally:
        ex.close()


def level_sizes(ex):
    return [ex.level_size(level) for level in range(ex.nlevels)]


def check_against_oracle(ex, c, img, what):
    """All stages of every level, the final keypoints and the descriptors of one image."""
    orc = OC.oracle_for(c)
    kg, dg = ex(img)
    ko, do = orc.extract(img)
    assert len(ko) >= c["min_kps"], f"{what}: the oracle finds {len(ko)} keypoints"
    OC.assert_stages_equal(ex, orc, c["nlevels"], what=f"{what} ")
    OC.assert_extract_equal(kg, dg, ko, do, what)
    return kg, ko


# ---------------------------------------------------------------------------
# A. Geometry and parameter sweep.  REACHES[name](sizes, features, ex) asserts what the case is there for.

def _odd_641x481(sizes, feat, ex):
    w0 = sizes[0][0]
    assert w0 % 4 != 0 and w0 % 2 == 1          # odd packed stride: byte loads at level 0, level 1's source unaligned
    assert w0 % 64 == 1                         # level 0's last tile is one column wide
    assert any(w % 64 in (2, 3) for w, _ in sizes[1:])   # a pyramid level with a 2-3 column last tile
    assert max(feat) + 16 <= 256                # the 256-node octree instance
    assert OC.small_level_start(sizes) == 4


def _small_333x246(sizes, feat, ex):
    assert len(sizes) == 8 and sizes[0][0] % 2 == 1
    ni = [OC.n_ini(*s) for s in sizes]
    assert ni[0] == 1 and ni[5:] == [2, 2, 2]
    assert OC.cell_grid(*sizes[-1])[1] == 1     # the last level has a single cell row
    assert OC.small_level_start(sizes) == 1     # every level but 0 is small to the launcher


def _wide_754x480(sizes, feat, ex):
    assert all(OC.n_ini(*s) == 2 for s in sizes)
    assert sizes[0][0] % 4 == 2                 # even stride, no multiple of 4
    assert max(feat) + 16 > 256                 # the 1024-node octree instance


def _tall_257x259(sizes, feat, ex):
    assert len(sizes) == 5 and sizes[0][1] > sizes[0][0] and sizes[0][0] % 64 == 1
    assert all(OC.n_ini(*s) == 1 for s in sizes)


def _scale_1p5(sizes, feat, ex):
    assert ex.tables()["scale"][1] == np.float32(1.5) and sizes[1] == (427, 320)
    assert list(feat[:2]) == [384, 256] and max(feat) + 16 > 256


def _scale_2p0(sizes, feat, ex):
    assert [w for w, _ in sizes] == [640, 320, 160] and [h for _, h in sizes] == [480, 240, 120]


def _scale_1p05(sizes, feat, ex):
    assert len(sizes) == 8 and OC.small_level_start(sizes) == 8   # no level is small to the launcher
    assert min(OC.level_tiles(*s) for s in sizes) > OC.SMALL_LEVEL_TILES // 2


def _pano_1000x230(sizes, feat, ex):
    ni = [OC.n_ini(*s) for s in sizes]
    assert ni[0] >= 5 and max(ni) == ni[-1] == 8 and sizes[-1] == (279, 64)


def _one_level(sizes, feat, ex):
    assert list(feat) == [1000] and ex.max_kp == 1016   # 1016 of the octree's 1024 node slots


def _min_127x96(sizes, feat, ex):
    assert sizes == [(127, 96)] and OC.cell_grid(127, 96)[:2] == (3, 2)


def _min_64x64(sizes, feat, ex):
    assert sizes == [(64, 64)] and OC.cell_grid(64, 64) == (1, 1, 32, 32)


REACHES = {"odd_641x481": _odd_641x481, "small_333x246": _small_333x246, "wide_754x480": _wide_754x480,
           "tall_257x259": _tall_257x259, "scale_1p5": _scale_1p5, "scale_2p0": _scale_2p0,
           "scale_1p05": _scale_1p05, "pano_1000x230": _pano_1000x230, "one_level": _one_level,
           "min_127x96": _min_127x96, "min_64x64": _min_64x64}
assert set(REACHES) == set(OC.GEOMETRY_CASES)


@pytest.mark.parametrize("name", list(OC.GEOMETRY_CASES))
def test_geometry_case_bit_exact(name):
    c = OC.GEOMETRY_CASES[name]
    with extractor(c) as ex:
        sizes, feat = level_sizes(ex), ex.tables()["features"]
        assert sizes[0] == (c["width"], c["height"]) and sum(feat) == c["nfeatures"]
        assert ex.max_kp == sum(max(int(n) + 16, 4 * OC.n_ini(*s) + 4) for n, s in zip(feat, sizes))
        REACHES[name](sizes, feat, ex)
        kg, _ = check_against_oracle(ex, c, OC.case_image(c), name)
        assert set(np.unique(kg["octave"])) >= set(c["levels"])


@pytest.mark.parametrize("name", list(OC.REJECTED))
def test_rejected_geometry(name, capfd):
    """spslam_create returns SPSLAM_ERR_ARG before anything is allocated or launched, and says why."""
    import spslam_gpu
    args, message = OC.REJECTED[name]
    with pytest.raises(spslam_gpu.SpslamError, match=r"\(-1\)"):
        spslam_gpu.OrbExtractor(**args)
    if message is not None:
        assert message in capfd.readouterr().err


# ---------------------------------------------------------------------------
# B. Input layout, batch and capacity, on the 641 x 481 case through the batched device entry.

ODD = OC.GEOMETRY_CASES["odd_641x481"]


@pytest.fixture(scope="module")
def odd_ctx():
    with extractor(ODD, max_batch=4) as ex:
        yield ex


@pytest.fixture(scope="module")
def odd_frames():
    """Three frames with more than 100 keypoints each, and their oracle results."""
    frames = OC.variant_frames(ODD)
    orc = OC.oracle_for(ODD)
    expected = [orc.extract(g) for g in frames]
    assert all(len(k) > 100 for k, _ in expected)
    return frames, expected


def test_padded_rows(odd_ctx, odd_frames):
    """Rows 700 bytes apart, the 59 bytes after each row filled with something else than its border."""
    frames, expected = odd_frames
    buf, fs = OC.embed(frames[:1], 700)
    kps, desc, cnt = OC.run_batch(odd_ctx, buf, 1, fs, 700)
    orc = OC.oracle_for(ODD)
    orc.pyramid(frames[0])
    OC.assert_stages_equal(odd_ctx, orc, ODD["nlevels"], what="stride 700 ")
    OC.assert_batch_equal(kps, desc, cnt, expected[:1], odd_ctx.max_kp, "stride 700")


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_misaligned_base(odd_ctx, odd_frames, offset):
    """stride 644 is a multiple of 4, so the base pointer alone decides the load paths."""
    frames, expected = odd_frames
    buf, fs = OC.embed(frames[:1], 644, base_offset=offset)
    kps, desc, cnt = OC.run_batch(odd_ctx, buf, 1, fs, 644, base_offset=offset)
    orc = OC.oracle_for(ODD)
    orc.pyramid(frames[0])
    OC.assert_stages_equal(odd_ctx, orc, ODD["nlevels"], what=f"base + {offset} ")
    OC.assert_batch_equal(kps, desc, cnt, expected[:1], odd_ctx.max_kp, f"base + {offset}")


def test_frame_stride_misaligns_later_frames(odd_ctx, odd_frames):
    """Frame 0 is dword aligned (packed load paths), frames 1 and 2 are not (byte paths); frame 1 is constant;
    three frames in a context for four."""
    frames, expected = odd_frames
    h, w = frames[0].shape
    stride = 644
    fs = stride * h + 1
    assert fs % 4 == 1 and (2 * fs) % 4 == 2
    batch = [frames[0], OC.constant(w, h), frames[2]]
    buf, _ = OC.embed(batch, stride, frame_stride=fs)
    kps, desc, cnt = OC.run_batch(odd_ctx, buf, 3, fs, stride)
    orc = OC.oracle_for(ODD)
    want = [expected[0], orc.extract(batch[1]), expected[2]]
    assert len(want[1][0]) == 0
    for f in range(3):
        orc.pyramid(batch[f])
        OC.assert_stages_equal(odd_ctx, orc, ODD["nlevels"], frame=f, what=f"frame {f} ")
    OC.assert_batch_equal(kps, desc, cnt, want, odd_ctx.max_kp, "frame stride")


@pytest.mark.parametrize("cap", [100, None])
def test_capacity_and_untouched_tail(odd_ctx, odd_frames, cap):
    """cap_per_frame = 100 cuts every frame at its first 100 keypoints; at 100 and at max_kp no byte outside
    [f * cap, f * cap + counts[f]) is written, the spare slot after the last frame included."""
    frames, expected = odd_frames
    h, w = frames[0].shape
    cap = odd_ctx.max_kp if cap is None else cap
    kps, desc, cnt = OC.run_batch(odd_ctx, np.stack(frames).reshape(-1), 3, w * h, w, cap=cap)
    if cap == 100:
        assert list(cnt[:3]) == [100, 100, 100]
    OC.assert_batch_equal(kps, desc, cnt, expected, cap, f"cap {cap}")


def test_host_entry_with_padded_rows(odd_ctx, odd_frames):
    """spslam_orb_extract with stride > w: the pitched host-to-device copy."""
    import spslam_gpu
    frames, expected = odd_frames
    h, w = frames[0].shape
    buf, _ = OC.embed(frames[:1], 700)
    cap = odd_ctx.max_kp
    kps = np.full((cap + 1) * spslam_gpu.KEYPOINT_DTYPE.itemsize, OC.SENTINEL, np.uint8).view(spslam_gpu.KEYPOINT_DTYPE)
    desc = np.full((cap + 1, 32), OC.SENTINEL, np.uint8)
    n = ctypes.c_int(-1)
    rc = odd_ctx.lib.spslam_orb_extract(odd_ctx.ctx, buf.ctypes.data, w, h, 700, kps.ctypes.data, desc.ctypes.data,
                                        cap, ctypes.byref(n))
    assert rc == 0, odd_ctx.lib.spslam_last_error(odd_ctx.ctx)
    OC.assert_batch_equal(kps, desc, np.array([n.value], np.int32), expected[:1], cap, "host stride 700")
    assert np.array_equal(odd_ctx.debug_stage(0, 0, 0), frames[0])   # the repacked image


# ---------------------------------------------------------------------------
# C. Image content.

def _cell_counts(cand, w, h):
    """Candidates per FAST cell of a w x h level, from debug_stage(.., 2)'s cell-window coordinates."""
    ncols, nrows, wcell, hcell = OC.cell_grid(w, h)
    cj, ci = (cand["x"].astype(int) - 3) // wcell, (cand["y"].astype(int) - 3) // hcell
    assert cj.min() >= 0 and cj.max() < ncols and ci.min() >= 0 and ci.max() < nrows
    return np.bincount(ci * ncols + cj, minlength=ncols * nrows)


@pytest.mark.parametrize("name", list(OC.CONTENT_CASES))
def test_content_case_bit_exact(name):
    c = OC.CONTENT_CASES[name]
    with extractor(c) as ex:
        kg, _ = check_against_oracle(ex, c, OC.case_image(c), name)
        assert set(np.unique(kg["octave"])) >= set(c["levels"])
        if name == "noise_th_1_1":
            sizes = level_sizes(ex)
            cand = ex.debug_stage(0, 0, 2)
            assert len(cand) > 5000
            per_cell = [_cell_counts(ex.debug_stage(0, level, 2), *sizes[level]).max() for level in range(8)]
            assert max(per_cell) <= OC.cell_cap(), per_cell
        if name == "half_constant_pano":
            assert OC.n_ini(*ex.level_size(0)) >= 5 and kg["x"].min() > 500   # the left initial nodes are empty


# ---------------------------------------------------------------------------
# D. Opt-in launch shapes: environment switches read once per process, so one fresh child per variant.

VARIANT_CASES = ("odd_641x481", "small_333x246")
VARIANTS = {"small_levels": {"SPSLAM_ORB_SMALL_LEVELS": "1"},
            "small_levels_2_groups": {"SPSLAM_ORB_SMALL_LEVELS": "1", "SPSLAM_ORB_SMALL_GROUPS": "2"},
            "split": {"SPSLAM_ORB_SPLIT": "1"}}


@pytest.fixture(scope="module")
def variant_inputs(tmp_path_factory):
    """The children's input file and the oracle's results: per case and frame the final output and the stages."""
    arrays = {"names": np.array(VARIANT_CASES)}
    expected = {}
    for name in VARIANT_CASES:
        c = OC.GEOMETRY_CASES[name]
        frames = OC.variant_frames(c)
        arrays[f"{name}/frames"] = np.stack(frames)
        arrays[f"{name}/params"] = np.array([c["nfeatures"], c["scale_factor"], c["nlevels"], c["ini_th_fast"],
                                             c["min_th_fast"]], np.float64)
        orc = OC.oracle_for(c)
        expected[name] = []
        for g in frames:
            k, d = orc.extract(g)
            expected[name].append((k, d, [OC.oracle_level(orc, level) for level in range(c["nlevels"])]))
    path = tmp_path_factory.mktemp("orb_variants") / "in.npz"
    np.savez(path, **arrays)
    return path, expected


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_launch_variant_bit_exact(variant, variant_inputs, tmp_path):
    src, expected = variant_inputs
    dst = tmp_path / "out.npz"
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPSLAM_ORB_")}
    env.update(VARIANTS[variant])
    r = subprocess.run([sys.executable, OC.__file__, str(src), str(dst)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(dst, allow_pickle=False)
    for name in VARIANT_CASES:
        c = OC.GEOMETRY_CASES[name]
        nl = c["nlevels"]
        sizes = [out[f"{name}/f0/l{level}/s0"].shape[::-1] for level in range(nl)]
        # the switches change this case's launches: it has small levels, and a level whose tile count leaves
        # tile groups of the fused kernel without a tile
        ls = OC.small_level_start(sizes)
        tiles = [OC.level_tiles(*s) for s in sizes[ls:]]
        assert ls < nl and any(t % 4 for t in tiles) and any(t % 2 for t in tiles), (ls, tiles)
        for f, (ko, do, stages) in enumerate(expected[name]):
            for level in range(nl):
                OC.assert_level_stages_equal([out[f"{name}/f{f}/l{level}/s{s}"] for s in range(4)], stages[level],
                                             level, f"{variant} {name} frame {f} ")
        OC.assert_batch_equal(out[f"{name}/kps"], out[f"{name}/desc"], out[f"{name}/counts"],
                              [(k, d) for k, d, _ in expected[name]], int(out[f"{name}/cap"]), f"{variant} {name}")
