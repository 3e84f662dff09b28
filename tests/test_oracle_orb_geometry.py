"""CPU check of the case table of tests/test_gpu_orb_geometry.py (tests/orb_common.py).

Only the oracle runs here.  A case that no longer yields keypoints where it claims to (an edited image, size
or threshold) would turn its GPU parity test into a comparison of two empty lists; this keeps the table honest
on the machine without a GPU.
"""
import numpy as np
import pytest

import orb_common as OC

ALL_CASES = {**OC.GEOMETRY_CASES, **OC.CONTENT_CASES}


@pytest.fixture(scope="module")
def extracted():
    """name -> (keypoints, descriptors, oracle) of every case, computed once."""
    out = {}
    for name, c in ALL_CASES.items():
        orc = OC.oracle_for(c)
        k, d = orc.extract(OC.case_image(c))
        out[name] = (k, d, orc)
    return out


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_case_yields_keypoints_where_it_claims(extracted, name):
    c = ALL_CASES[name]
    kps, desc, orc = extracted[name]
    assert len(kps) >= c["min_kps"], f"{len(kps)} keypoints"
    assert desc.shape == (len(kps), 32)
    per_level = np.bincount(kps["octave"], minlength=c["nlevels"])
    for level in c["levels"]:
        assert per_level[level] > 0, f"no keypoint on level {level}: {per_level}"
        assert len(orc.level_candidates(level)) > 0


def test_content_cases_are_what_they_are_named_for(extracted):
    k, _, orc = extracted["periodic"]
    # the tile repeats: most keypoints have a twin with the same octave and response (the octree's tie-break)
    key = k["octave"].astype(np.int64) * 256 + k["response"].astype(np.int64)
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    assert (cnt[inv] > 1).sum() >= len(k) // 2
    _, _, orc = extracted["checkerboard"]
    assert len(orc.level_candidates(0)) == 0 and len(orc.level_candidates(1)) > 0   # an empty level, then full ones
    k, _, orc = extracted["noise_th_1_1"]
    assert len(orc.level_candidates(0)) > 5000
    k, _, orc = extracted["noise_th_100_100"]
    assert all(len(orc.level_candidates(level)) == 0 for level in range(3, 8))
    k, _, _ = extracted["noise_th_254_200"]
    assert 1 <= len(k) <= 3
    k, _, orc = extracted["border_dots"]
    assert 1 <= len(k) <= len(OC.DOTS) and len(orc.level_candidates(0)) == 0         # coarse levels only
    k, _, _ = extracted["half_constant_pano"]
    assert k["x"].min() >= 600 - 19 * 1.2 ** 7      # nothing in the constant part: its initial nodes are empty


def test_variant_frames_are_distinct():
    c = OC.GEOMETRY_CASES["small_333x246"]
    a, b, d = OC.variant_frames(c)
    assert a.shape == b.shape == d.shape and not np.array_equal(a, d) and not np.array_equal(a, b)
