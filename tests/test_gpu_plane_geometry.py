"""GPU parity of plane extraction away from its two usual geometries (cloud 214 x 160 and 427 x 320): cloud sizes
on both sides of every launch threshold, Cloud.Dis values, input layouts, batches past the 16-frame switch to the
one-workgroup wave kernel, depth contents, the opt-in launch shapes, and the per-frame limits.

Bar as in test_gpu_planes.py, with no tolerance: cloud, distance map and normals bit-equal (NaN positions equal),
connected-component labels, plane count, coefficients (bit-equal), inlier and contour lists equal to
oracle_planes.PlaneOracle run with the same parameters.  Cases, depth images and measured oracle counts live in
plane_common.py; each case first asserts through PlaneExtractor.launch_shape() -- the launch code's own dispatch
functions -- the kernels it is there for.  tests/test_oracle_plane_cases.py keeps the table non-degenerate with
the oracle alone.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import plane_common as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex():
    import spslam_gpu
    e = spslam_gpu.OrbExtractor(max_batch=4, **PC.ORB_SMALL)
    yield e
    e.close()


def check_case(ex, table, name):
    c = PC.TABLES[table][name]
    d, po, ro = PC.expected(table, name)
    pe = PC.plane_extractor(ex, c, d.shape[1], d.shape[0])
    assert (pe.W, pe.H) == (po.W, po.H)
    PC.assert_launch(pe, c)
    n, _ = PC.compare(pe, d, name, expected=(po, ro))
    assert n == c["planes"] and pe.status() == 0
    return pe, ro


# ---------------------------------------------------------------------------
# A. Geometries.

@pytest.mark.parametrize("name", list(PC.GEOMETRY_CASES))
def test_geometry_case_matches_oracle(ex, name):
    check_case(ex, "geometry", name)


@pytest.mark.parametrize("name", list(PC.DEGENERATE_CASES))
def test_degenerate_cloud_is_supported(ex, name):
    """Clouds too small for a normal (include/spslam_gpu.h: no lower bound): every stage equals the oracle's,
    no plane comes out."""
    pe, ro = check_case(ex, "degenerate", name)
    assert len(ro["coef"]) == 0 and np.isnan(pe.debug(0, 1)).all()


def test_configure_refuses_what_the_launch_refuses(ex):
    """W = 513 passed spslam_planes_configure's own checks (W <= 546) and failed at extraction with a bare HIP
    error; now configure refuses it, and W = 512 with the same height goes through."""
    import spslam_gpu
    import spslam_planes
    K = PC.intrinsics()
    with pytest.raises(spslam_gpu.SpslamError, match="rc=-1.*512 columns"):
        spslam_planes.PlaneExtractor(ex, *K, 513, 96, cloud_dis=1)
    with pytest.raises(spslam_gpu.SpslamError, match="rc=-1.*512 rows"):
        spslam_planes.PlaneExtractor(ex, *K, 96, 513, cloud_dis=1)
    pe = spslam_planes.PlaneExtractor(ex, *K, 512, 96, cloud_dis=1)
    assert pe.launch_shape(1)["seg_positions"] == 8
    assert len(pe(PC.wall(512, 96))["coef"]) == 1
    # a refused configuration leaves the one before it in place, whole
    with pytest.raises(spslam_gpu.SpslamError, match="rc=-1"):
        spslam_planes.PlaneExtractor(ex, *K, 1026, 96, cloud_dis=2)
    assert pe.launch_shape(1)["seg_positions"] == 8 and len(pe(PC.wall(512, 96))["coef"]) == 1


# ---------------------------------------------------------------------------
# B. Layouts, on cloud 134 x 65 (depth 400 x 193, Cloud.Dis 3: neither divides).

LAYOUT = PC.BATCH_CASES["b17_h65"]


@pytest.fixture(scope="module")
def layout():
    """Three different frames, their oracle results, and an extractor of its own for up to four frames."""
    import spslam_gpu
    c = LAYOUT["case"]
    frames = PC.batch_frames(LAYOUT)[:3]
    expected = [PC.oracle(d, **PC.oracle_params(c)) for d in frames]
    assert all(len(ro["coef"]) >= 1 for _, ro in expected)
    h, w = frames[0].shape
    e = spslam_gpu.OrbExtractor(max_batch=4, **PC.ORB_SMALL)
    try:
        pe = PC.plane_extractor(e, c, w, h)
        PC.assert_launch(pe, c, 3)
        yield pe, frames, expected
    finally:
        e.close()


def check_batch(pe, out, expected, what):
    P, C, I, Cn = out
    for f, (po, ro) in enumerate(expected):
        PC.assert_stages_equal(PC.device_stages(pe, f), po, f"{what} frame {f}")
        PC.assert_planes_equal(PC.frame_result(P, C, I, Cn, f), ro, f"{what} frame {f}")
        assert pe.status(f) == 0
    PC.assert_spare_untouched(P, C, I, Cn)


def test_host_entry_with_padded_rows(layout):
    """spslam_planes_extract with stride_floats = w + 13 (the pitched copy), outputs pre-filled."""
    import spslam_planes
    pe, frames, expected = layout
    h, w = frames[0].shape
    buf = np.full((h, w + 13), 3.0e38, np.float32)
    buf[:, w::2] = np.nan
    buf[:, :w] = frames[0]
    planes = np.full((pe.planes_cap + 1) * 8, PC.SENTINEL, np.int32)
    inl = np.full(pe.inlier_cap + 1, PC.SENTINEL, np.int32)
    con = np.full(pe.contour_cap + 1, PC.SENTINEL, np.int32)
    n = ctypes.c_int(-1)
    rc = pe.ex.lib.spslam_planes_extract(pe.ex.ctx, buf.ctypes.data, w, h, w + 13, planes.ctypes.data, pe.planes_cap,
                                         ctypes.byref(n), inl.ctypes.data, con.ctypes.data)
    assert rc == 0, pe.ex.lib.spslam_last_error(pe.ex.ctx)
    P = planes.view(spslam_planes.PLANE_DTYPE)[None]
    rg = PC.frame_result(P, np.array([n.value]), inl[None], con[None], 0)
    PC.assert_stages_equal(PC.device_stages(pe), expected[0][0], "host stride w + 13")
    PC.assert_planes_equal(rg, expected[0][1], "host stride w + 13")


def test_batch_padded_rows_and_frame_gap(layout):
    """Rows w + 13 floats apart, frames 37 floats further apart than their rows need; NaN and 3e38 in between."""
    pe, frames, expected = layout
    h, w = frames[0].shape
    stride = w + 13
    d_buf, fs = PC.embed(frames, stride, frame_stride=stride * h + 37)
    check_batch(pe, PC.run_batch(pe, d_buf, 3, fs, stride), expected, "padded")


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_misaligned_base(layout, offset):
    """The depth base pointer 4, 8 and 12 bytes past a 16-byte boundary."""
    pe, frames, expected = layout
    h, w = frames[0].shape
    d_buf, fs = PC.embed(frames[:2], w, base_offset=offset)
    check_batch(pe, PC.run_batch(pe, d_buf, 2, fs, w, base_offset=offset), expected[:2], f"base + {offset}")


def test_second_cloud_set(layout):
    """Cloud set 1 gives what set 0 gives, and set 0's cloud stays as it was."""
    pe, frames, expected = layout
    h, w = frames[0].shape
    d_buf, fs = PC.embed(frames[:1], w)
    check_batch(pe, PC.run_batch(pe, d_buf, 1, fs, w), expected[:1], "set 0")
    try:
        pe.select_cloud_set(1)
        d_buf, fs = PC.embed(frames[1:2], w)
        check_batch(pe, PC.run_batch(pe, d_buf, 1, fs, w), expected[1:2], "set 1")
    finally:
        pe.select_cloud_set(0)
    assert np.array_equal(pe.debug(0, 0), expected[0][0].cloud(), equal_nan=True)


@pytest.mark.parametrize("name", list(PC.BATCH_CASES))
def test_batch_past_16_frames(name):
    """More than 16 frames in one call: plane_wave_kernel, one workgroup per frame (what bench.py times at
    B = 256).  Every frame against the oracle in full."""
    import spslam_gpu
    b = PC.BATCH_CASES[name]
    c, n = b["case"], b["frames"]
    frames = PC.batch_frames(b)
    assert all(PC.batch_nonfinite(frames))   # frames with NaN samples and frames with +Inf samples among them
    h, w = frames[0].shape
    e = spslam_gpu.OrbExtractor(max_batch=n, **PC.ORB_SMALL)
    try:
        pe = PC.plane_extractor(e, c, w, h)
        PC.assert_launch(pe, c, 16, one_workgroup=False)
        PC.assert_launch(pe, c, n, one_workgroup=True)
        d_buf, fs = PC.embed(frames, w)
        out = PC.run_batch(pe, d_buf, n, fs, w)
        expected = [PC.oracle(d, **PC.oracle_params(c)) for d in frames]
        check_batch(pe, out, expected, name)
    finally:
        e.close()


# ---------------------------------------------------------------------------
# C. Contents, at 640 x 480 / Cloud.Dis 3.

@pytest.mark.parametrize("name", list(PC.CONTENT_CASES))
def test_content_case_matches_oracle(ex, name):
    pe, ro = check_case(ex, "content", name)
    if name == "wall":   # the inlier list fills inlier_cap to within one
        assert [len(i) for i in ro["inliers"]] == [pe.inlier_cap - 1]


@pytest.mark.parametrize("name", list(PC.NONFINITE_CASES))
def test_nonfinite_case_matches_oracle(ex, name):
    """A NaN band and a +Inf block at NW 3, 4 and 8 in the default launch (section D runs them in the others)."""
    check_case(ex, "nonfinite", name)


# ---------------------------------------------------------------------------
# Limits: 255 components over MinSize, 64 models, 64 kept planes per frame.

def _host_extract(pe, d):
    """spslam_planes_extract on sentinel-filled outputs: (return code, message, planes, n, inliers, contours)."""
    import spslam_planes
    planes = np.full((pe.planes_cap + 1) * 8, PC.SENTINEL, np.int32)
    inl = np.full(pe.inlier_cap + 1, PC.SENTINEL, np.int32)
    con = np.full(pe.contour_cap + 1, PC.SENTINEL, np.int32)
    n = ctypes.c_int(-1)
    rc = pe.ex.lib.spslam_planes_extract(pe.ex.ctx, d.ctypes.data, d.shape[1], d.shape[0], d.shape[1],
                                         planes.ctypes.data, pe.planes_cap, ctypes.byref(n), inl.ctypes.data,
                                         con.ctypes.data)
    return (rc, pe.ex.lib.spslam_last_error(pe.ex.ctx).decode(), planes.view(spslam_planes.PLANE_DTYPE)[None],
            np.array([n.value]), inl[None], con[None])


@pytest.mark.parametrize("name,flag,message", [("models_10x8", "OVER_MODELS", "more than 64 plane models"),
                                               ("components_21x16", "OVER_COMPONENTS", "more than 255 components")])
def test_crossed_limit_is_reported(ex, name, flag, message):
    """Past a limit nothing is asserted about the planes themselves: only that the frame says so, that the output
    is well formed (counts, offsets and lengths within the capacities, nothing written past them), and that the
    next frame within the limits reports none."""
    import spslam_planes
    c = PC.LIMIT_CASES[name]
    d = PC.expected("limit", name)[0]
    pe = PC.plane_extractor(ex, c, 640, 480)
    bit = getattr(spslam_planes, flag)
    rc, msg, P, C, I, Cn = _host_extract(pe, d)
    assert rc == -2 and message in msg, (rc, msg)          # SPSLAM_ERR_CAPACITY
    assert pe.status() & bit
    assert 0 <= C[0] <= pe.planes_cap == 64
    PC.frame_result(P, C, I, Cn, 0)
    # the asynchronous entry returns as before; the flags of both frames are there after the synchronisation
    d_buf, fs = PC.embed([PC.wall(640, 480), d], 640)
    P, C, I, Cn = PC.run_batch(pe, d_buf, 2, fs, 640)
    assert pe.status(0) == 0 and pe.status(1) & bit
    for f in range(2):
        PC.frame_result(P, C, I, Cn, f)
    PC.assert_spare_untouched(P, C, I, Cn)
    assert C[0] == 1 and C[1] <= 64
    # the flag is the last extraction's: a frame within the limits clears it
    rc, msg, P, C, I, Cn = _host_extract(pe, PC.wall(640, 480))
    assert rc == 0 and C[0] == 1 and pe.status() == 0, (rc, msg)


# ---------------------------------------------------------------------------
# D. Opt-in launch shapes: environment switches read once per process, so one fresh child per variant.

@pytest.fixture(scope="module")
def variant_expected():
    return {name: PC.expected(table, name) for table, name in PC.VARIANT_CASES}


@pytest.mark.parametrize("variant", list(PC.VARIANTS))
def test_launch_variant_matches_oracle(variant, variant_expected, tmp_path):
    dst = tmp_path / "out.npz"
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPSLAM_PLANE_")}
    env.update(PC.VARIANTS[variant])
    r = subprocess.run([sys.executable, PC.__file__, str(dst)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(dst, allow_pickle=False)
    for table, name in PC.VARIANT_CASES:
        c = PC.TABLES[table][name]
        _, po, ro = variant_expected[name]
        lds, k, nw, one, rows = (int(v) for v in out[f"{name}/shape"])
        assert (lds, k, nw) == (int(c["lds"]), c["k"], c["nw"])
        assert (one, rows) == {"one_workgroup": (1, 0), "three_workgroups": (0, 0),
                               "barrier": (0, PC.VARIANT_ROWS[name])}[variant], (name, one, rows)
        what = f"{variant} {name}"
        PC.assert_stages_equal([out[f"{name}/s{s}"] for s in range(4)], po, what)
        n = int(out[f"{name}/n"])
        rg = {key: [out[f"{name}/{key}{j}"] for j in range(n)] for key in ("coef", "inliers", "contour")}
        PC.assert_planes_equal(rg, ro, what)
