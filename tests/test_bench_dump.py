"""bench.py --dump-outputs on the CPU: dump_outputs() over a stand-in for HotPath.results() writes float32 /
float64 .npy files field by field, zeroes the per-keypoint entries past each frame's count, is identical from
call to call and stays below its size limit by sampling only the large arrays."""
import types

import numpy as np

import bench
import spslam_gpu as G

B, CAP = 4, 50


def _results():
    rng = np.random.default_rng(1)
    kps = np.zeros((B, CAP), G.KEYPOINT_DTYPE)
    kps["x"] = rng.random((B, CAP), np.float32) + 1
    kps["octave"] = 3
    pose = np.zeros(B, G.POSE_RESULT_DTYPE)
    pose["Tcw"] = rng.random((B, 16), np.float32)
    pose["n_inliers"] = [5, 6, 7, 8]
    return dict(kps=kps, kp_counts=np.array([3, CAP, 0, 7], np.int32), pose1=pose,
                match=np.full((B, CAP), 7, np.int32), assoc=np.ones((2, 3, B, 5), np.int32),
                contour_points=np.arange(B, dtype=np.float64))


def _load(d):
    return {p.name: np.load(p) for p in sorted(d.iterdir())}


def test_dump_fields_dtypes_and_masking(tmp_path):
    hp = types.SimpleNamespace(kp_cap=CAP, n_lba=0)
    res = _results()
    bench.dump_outputs(hp, res, tmp_path / "a")
    got = _load(tmp_path / "a")
    assert {"kps.x.npy", "kps.octave.npy", "kp_counts.npy", "pose1.Tcw.npy", "pose1.n_inliers.npy", "match.npy",
            "assoc.npy", "contour_points.npy"} <= set(got)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["kps.x.npy"].dtype == np.float32 and got["kps.octave.npy"].dtype == np.float64
    live = np.arange(CAP)[None, :] < res["kp_counts"][:, None]
    assert np.array_equal(got["kps.x.npy"], np.where(live, res["kps"]["x"], 0))
    assert np.array_equal(got["match.npy"], np.where(live, 7.0, 0.0))
    assert np.array_equal(got["pose1.Tcw.npy"], res["pose1"]["Tcw"])
    assert np.array_equal(got["pose1.n_inliers.npy"], [5, 6, 7, 8])
    assert res["match"].min() == 7  # the caller's arrays are left alone


def test_dump_is_repeatable_and_bounded(tmp_path, monkeypatch):
    hp = types.SimpleNamespace(kp_cap=CAP, n_lba=0)
    n = len(_load_names(hp, tmp_path))
    limit = 4096 * n + 6000  # room for every small array (1.4 KB together) and a part of each (B, CAP) one
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    bench.dump_outputs(hp, _results(), tmp_path / "a")
    bench.dump_outputs(hp, _results(), tmp_path / "b")
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= limit
    assert a["kp_counts.npy"].shape == (B,) and a["pose1.Tcw.npy"].shape == (B, 16)  # small arrays whole
    assert a["match.npy"].ndim == 1 and 0 < a["match.npy"].size < B * CAP  # large ones sampled


def _load_names(hp, tmp_path):
    bench.dump_outputs(hp, _results(), tmp_path / "names")
    return list((tmp_path / "names").iterdir())
