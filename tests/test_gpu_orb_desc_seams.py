"""GPU parity of the ORB extractor where desc_kernel and fast_cells_kernel issue their loads in batches.

desc_kernel loads the whole 31 x 31 square round a keypoint before it applies the orientation circle, finds
the slot's level and output offset from one read of the frame's level counts, and writes a descriptor with one
store; fast_cells_kernel loads a cell's score window in groups of 18 * 64 = 1152 pixels.  Bar as in
test_gpu_orb_geometry.py: byte identity with oracle_ctypes.OrbOracle run on each frame alone.  Cases and
images come from orb_common.py; every case first asserts, from the oracle alone, the property it is there for.
"""
import contextlib

import numpy as np
import pytest

import orb_common as OC

pytestmark = pytest.mark.gpu

LOAD_GROUP = 18 * 64   # orb_kernels.hip kCellLoads * 64: score pixels of a cell window per load group


@contextlib.contextmanager
def extractor(c, **extra):
    import spslam_gpu
    ex = spslam_gpu.OrbExtractor(**OC.extractor_args(c, **extra))
    try:
        yield ex
    finally:
        ex.close()


# ---------------------------------------------------------------------------
# 1. Keypoints on the border of the keypoint area: the discarded loads outside the circle touch the square's
# corners, 4 pixels inside the image, and frame 1's buffer follows frame 0's directly.

BORDER_SEEDS = (0, 1)   # each of these noise frames alone has a keypoint on all four border lines, both cases


@pytest.mark.parametrize("name", ["min_64x64", "min_127x96"])
def test_border_keypoints_in_a_batch(name):
    c = OC.GEOMETRY_CASES[name]
    w, h = c["width"], c["height"]
    assert c["nlevels"] == 1               # level coordinates are image coordinates
    frames = [OC.noise(w, h, seed) for seed in BORDER_SEEDS]
    orc = OC.oracle_for(c)
    expected = [orc.extract(g) for g in frames]
    for ko, _ in expected:
        assert len(ko) >= c["min_kps"]
        # the admissible area is [EDGE, w - EDGE - 1] x [EDGE, h - EDGE - 1]: a FAST cell window starts at
        # MIN_BORDER and ends at w - MIN_BORDER, and scores stay 3 pixels inside it
        assert ko["x"].min() == OC.EDGE and ko["x"].max() == w - OC.EDGE - 1
        assert ko["y"].min() == OC.EDGE and ko["y"].max() == h - OC.EDGE - 1
    with extractor(c, max_batch=2) as ex:
        kps, desc, cnt = OC.run_batch(ex, np.stack(frames).reshape(-1), 2, w * h, w)
        for f in range(2):
            orc.pyramid(frames[f])
            OC.assert_stages_equal(ex, orc, 1, frame=f, what=f"{name} frame {f} ")
        OC.assert_batch_equal(kps, desc, cnt, expected, ex.max_kp, name)


# ---------------------------------------------------------------------------
# 2. Mixed counts in one batch: a full frame, a frame without a keypoint and a frame whose upper levels are
# empty, at the default capacity and at one below the noise frame's total.

SMALL = OC.GEOMETRY_CASES["small_333x246"]


def low_contrast(w, h):
    """Noise of amplitude 12 round 128: corners on the lower levels only (resizing flattens the upper ones)."""
    g = 128 + (OC.noise(w, h).astype(np.int32) - 128) * 12 // 128
    return np.ascontiguousarray(g, np.uint8)


@pytest.fixture(scope="module")
def mixed():
    w, h = SMALL["width"], SMALL["height"]
    frames = [OC.noise(w, h), OC.constant(w, h), low_contrast(w, h)]
    orc = OC.oracle_for(SMALL)
    expected = [orc.extract(g) for g in frames]
    per_level = [np.bincount(k["octave"], minlength=SMALL["nlevels"]) for k, _ in expected]
    assert per_level[0].min() > 0 and len(expected[0][0]) > 400
    assert per_level[1].sum() == 0
    assert per_level[2][:3].min() > 0 and per_level[2][4:].sum() == 0 and len(expected[2][0]) > 100
    return frames, expected


@pytest.mark.parametrize("cap", [100, None])
def test_mixed_counts_in_one_batch(mixed, cap):
    frames, expected = mixed
    h, w = frames[0].shape
    with extractor(SMALL, max_batch=4) as ex:
        cap = ex.max_kp if cap is None else cap
        kps, desc, cnt = OC.run_batch(ex, np.stack(frames).reshape(-1), 3, w * h, w, cap=cap)
        assert list(cnt[:3]) == [min(len(k), cap) for k, _ in expected]
        OC.assert_batch_equal(kps, desc, cnt, expected, cap, f"mixed cap {cap}")


# ---------------------------------------------------------------------------
# 3. A cell window larger than one load group: level 6 of the 333 x 246 pyramid is 112 x 82, two cells of
# 40 x 50 scored pixels (windows of 46 x 56, the widest of orb_common's accepted geometries): 2000 pixels, two
# load groups, the second one partly past the window's end.

def cell_counts(cand, w, h):
    """Candidates per FAST cell of a w x h level, from their cell-window coordinates (stage 2's layout)."""
    ncols, nrows, wcell, hcell = OC.cell_grid(w, h)
    cj, ci = (cand["x"].astype(int) - 3) // wcell, (cand["y"].astype(int) - 3) // hcell
    assert cj.min() >= 0 and cj.max() < ncols and ci.min() >= 0 and ci.max() < nrows
    return np.bincount(ci * ncols + cj, minlength=ncols * nrows)


def test_cell_window_of_two_load_groups():
    c = SMALL
    img = OC.noise(c["width"], c["height"])
    orc = OC.oracle_for(c)
    ko, do = orc.extract(img)
    with extractor(c) as ex:
        sizes = [ex.level_size(level) for level in range(c["nlevels"])]
        scored = [OC.cell_grid(*s)[2] * OC.cell_grid(*s)[3] for s in sizes]
        widest = int(np.argmax(scored))
        assert sizes[widest] == (112, 82) and OC.cell_grid(112, 82) == (2, 1, 40, 50)
        assert LOAD_GROUP < scored[widest] <= 2 * LOAD_GROUP
        kg, dg = ex(img)
        for level in range(c["nlevels"]):
            got, want = ex.debug_stage(0, level, 2), orc.level_candidates(level)
            assert np.array_equal(cell_counts(got, *sizes[level]), cell_counts(want, *sizes[level])), level
        assert cell_counts(orc.level_candidates(widest), *sizes[widest]).min() > 0
        OC.assert_stages_equal(ex, orc, c["nlevels"], what="two load groups ")
        OC.assert_extract_equal(kg, dg, ko, do, "two load groups")
