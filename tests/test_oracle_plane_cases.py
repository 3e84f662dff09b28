"""The case tables of test_gpu_plane_geometry.py (plane_common.py), with the oracle alone: every case still gives
the oracle what it is there for -- planes to compare, the model count of its refinement path, components and
models past the kernel's limits, the split surface's two models and one plane -- so a change of synth.py cannot
quietly empty the GPU tests.  The counts are the ones written in the tables.
"""
import numpy as np
import pytest

import plane_common as PC

TABLES = PC.TABLES
NO_PLANES_EXPECTED = {"all_nan"} | set(PC.DEGENERATE_CASES)


@pytest.mark.parametrize("table,name", [(t, n) for t, tab in TABLES.items() for n in tab])
def test_case_counts(table, name):
    c = TABLES[table][name]
    d, po, ro = PC.expected(table, name)
    assert d.dtype == np.float32 and d.shape[0] <= 960 and d.shape[1] <= 1280
    assert (len(ro["coef"]), po.n_models) == (c["planes"], c["models"])
    if name in NO_PLANES_EXPECTED:
        assert c["planes"] == 0
    else:
        assert len(ro["coef"]) >= 1
    if table == "degenerate":
        assert np.isnan(po.normals()).all()
    if c["path"]:
        assert PC.refine_path(po.n_models) == c["path"]


def test_cloud_sizes():
    """The cloud sizes the geometry cases name."""
    sizes = {n: PC.cloud_size(c) for n, c in PC.GEOMETRY_CASES.items()}
    assert sizes == {"wide_lds_300x100": (300, 100), "large_narrow_200x200": (200, 200),
                     "large_narrow_256x160": (256, 160), "w256": (256, 120), "w257": (257, 120), "w512": (512, 96),
                     "w63": (63, 100), "w64": (64, 100), "w65": (65, 100), "h64": (200, 64), "h65": (200, 65),
                     "h128": (150, 128), "h129": (150, 129), "h330": (150, 330), "h65_indivisible": (134, 65),
                     "tall_100x512": (100, 512), "tall_96x480": (96, 480), "dis2": (320, 240), "dis4": (160, 120),
                     "dis5": (128, 96), "patch_24x24": (24, 24)}
    d = PC.GEOMETRY_CASES["h65_indivisible"]["depth"]()
    assert d.shape[1] % 3 and d.shape[0] % 3
    assert [PC.cloud_size(c) for c in PC.DEGENERATE_CASES.values()] == [(1, 1), (2, 3), (7, 5), (16, 16)]
    assert all(PC.cloud_size(c) == (214, 160) for t in (PC.CONTENT_CASES, PC.LIMIT_CASES) for c in t.values())


def test_table_covers_every_launch():
    """What the cases pin (and the GPU tests assert through the launch-shape hook) covers all four segmentation
    instances, K = 4 and 8 on each side of W = 256, and NW = 1, 2, 3, 4, 6 and 8 (NW = 5: test_planes_c5_size)."""
    cases = list(PC.GEOMETRY_CASES.values())
    assert {(c["lds"], c["k"]) for c in cases} == {(True, 4), (True, 8), (False, 4), (False, 8)}
    assert {c["nw"] for c in cases} == {1, 2, 3, 4, 6, 8}
    for c in cases:
        w, h = PC.cloud_size(c)
        assert c["k"] == (4 if w <= 256 else 8) and c["nw"] == -(-h // 64)
    assert {c["nw"] for b in PC.BATCH_CASES.values() for c in [b["case"]]} == {2, 3}


def test_content_cases_are_what_they_say():
    d, po, ro = PC.expected("content", "wall")
    n = po.W * po.H
    assert [len(i) for i in ro["inliers"]] == [n - 1] and [len(i) for i in ro["contour"]] == [0]
    _, po, ro = PC.expected("geometry", "patch_24x24")
    assert [len(i) for i in ro["inliers"]] == [575]
    for name in ("zero_band", "nan_band"):   # PlaneNotSeen drops one of the two models
        _, po, ro = PC.expected("content", name)
        assert (po.n_models, len(ro["coef"])) == (2, 1)
    for name, bad in (("far_inf", np.isposinf), ("far_negated", lambda a: a < 0)):
        d = PC.expected("content", name)[0]
        assert 0.2 < bad(d).mean() < 0.95
    assert np.isnan(PC.expected("content", "all_nan")[0]).all()
    _, po, _ = PC.expected("content", "facets_8x6")
    assert PC.refine_path(po.n_models) == "general" and po.n_models <= PC.MAX_MODELS
    assert PC.big_components(po, 100) <= PC.MAX_COMPONENTS


def test_limit_cases_cross_their_limits():
    _, po, _ = PC.expected("limit", "models_10x8")
    big = PC.big_components(po, PC.LIMIT_CASES["models_10x8"]["min_size"])
    assert po.n_models > PC.MAX_MODELS and big == PC.LIMIT_COMPONENTS["models_10x8"] <= PC.MAX_COMPONENTS
    _, po, _ = PC.expected("limit", "components_21x16")
    big = PC.big_components(po, PC.LIMIT_CASES["components_21x16"]["min_size"])
    assert big == PC.LIMIT_COMPONENTS["components_21x16"] > PC.MAX_COMPONENTS


@pytest.mark.parametrize("name", list(PC.BATCH_CASES))
def test_batch_frames_differ(name):
    b = PC.BATCH_CASES[name]
    frames = PC.batch_frames(b)
    assert len(frames) == b["frames"] > 16 and len({f.tobytes() for f in frames}) == len(frames)
    c = b["case"]
    assert PC.cloud_size(c, frames[0]) == {"b17_h65": (134, 65), "b17_h160": (214, 160), "b40_h65": (134, 65)}[name]
    results = [PC.oracle(d, **PC.oracle_params(c)) for d in frames]
    counts = [len(ro["coef"]) for _, ro in results]
    assert min(counts) >= 1 and len(set(counts)) > 1, counts
    # frames with NaN and with +Inf samples, which reach the cloud and still leave normals below and right of them
    nan, inf = PC.batch_nonfinite(frames)
    assert len(nan) >= 2 and len(inf) >= 2 and not set(nan) & set(inf)
    for f in nan + inf:
        z = results[f][0].cloud()[:, 2].reshape(results[f][0].H, -1)
        bad = ~np.isfinite(z)
        rows, cols = np.nonzero(bad)
        assert bad.sum() >= 10
        ok = ~np.isnan(results[f][0].normals()[:, 0]).reshape(z.shape)
        assert ok[rows.max() + 1:, cols.max() + 1:].sum() > 100


def test_variant_cases_cover_the_barrier_kernel():
    """Finite and non-finite depth at each of plane_dist_integral_kernel's three row bounds."""
    rows = {n: PC.cloud_size(PC.TABLES[t][n])[1] for t, n in PC.VARIANT_CASES}
    bound = {n: (192 if h <= 192 else 320 if h <= 320 else 512) for n, h in rows.items()}
    assert PC.VARIANT_ROWS == bound
    for table in ("geometry", "nonfinite"):
        assert {bound[n] for t, n in PC.VARIANT_CASES if t == table} == {192, 320, 512}
    assert sorted(bound[n] for t, n in PC.VARIANT_CASES if t == "nonfinite") == [192, 320, 512]


def test_variant_cases_cover_the_wave_kernels():
    """The forced one- and three-workgroup launches run the wave kernels without a ring (NW 1), with rings on both
    sides of a wave (NW 3 and more), at NW 6, and with a last wave that is not full (h330: 10 of 64 rows)."""
    nw = {n: PC.TABLES[t][n]["nw"] for t, n in PC.VARIANT_CASES}
    assert (nw["h64"], nw["h330"]) == (1, 6) and {1, 3, 4, 6, 8} <= set(nw.values())
    assert PC.cloud_size(PC.GEOMETRY_CASES["h64"])[1] == 64 and PC.cloud_size(PC.GEOMETRY_CASES["h330"])[1] % 64 == 10


@pytest.mark.parametrize("name", list(PC.NONFINITE_CASES))
def test_nonfinite_cases_reach_the_cloud(name):
    """NaN and +Inf points in the cloud, valid normals below and right of them (what a kernel adding the
    non-finite gradients into its integral images loses)."""
    _, po, _ = PC.expected("nonfinite", name)
    z = po.cloud()[:, 2].reshape(po.H, po.W)
    assert np.isnan(z).sum() >= 10 and np.isposinf(z).sum() >= 10
    rows, cols = np.nonzero(~np.isfinite(z))
    ok = ~np.isnan(po.normals()[:, 0]).reshape(po.H, po.W)
    assert ok[rows.max() + 1:, cols.max() + 1:].sum() > 100
