"""CPU checks of the LocalMapping records of include/spslam_gpu.h (the Fuse search and the map-point refresh):
struct sizes and field offsets match the Python bindings, the new entry points are exported, and the status and
mask constants agree."""
import ctypes
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spslam_gpu.h"
#define S(T) printf(#T " %zu\n", sizeof(T));
#define O(T, f) printf(#T "." #f " %zu\n", offsetof(T, f));
#define C(N) printf(#N " %d\n", (int)N);
int main(void) {
  S(spslam_fuse_problem) O(spslam_fuse_problem, Tcw) O(spslam_fuse_problem, kf_slot)
  O(spslam_fuse_problem, point_offset) O(spslam_fuse_problem, n_points) O(spslam_fuse_problem, out_offset)
  S(spslam_fuse_result) O(spslam_fuse_result, best_idx) O(spslam_fuse_result, best_dist)
  O(spslam_fuse_result, level) O(spslam_fuse_result, status)
  S(spslam_fuse_params) O(spslam_fuse_params, th)
  S(spslam_point_refresh_map) O(spslam_point_refresh_map, kf_Tcw) O(spslam_point_refresh_map, kf_slot)
  O(spslam_point_refresh_map, kf_bad) O(spslam_point_refresh_map, obs_off) O(spslam_point_refresh_map, obs_kf)
  O(spslam_point_refresh_map, obs_kp) O(spslam_point_refresh_map, ref_kf) O(spslam_point_refresh_map, point_bad)
  O(spslam_point_refresh_map, points)
  C(SPSLAM_FUSE_SEARCHED) C(SPSLAM_FUSE_SKIPPED) C(SPSLAM_FUSE_BEHIND) C(SPSLAM_FUSE_OUTSIDE_IMAGE)
  C(SPSLAM_FUSE_OUT_OF_RANGE) C(SPSLAM_FUSE_VIEW_ANGLE) C(SPSLAM_FUSE_NO_CANDIDATES)
  C(SPSLAM_POINT_MAX_OBS) C(SPSLAM_REFRESH_DESCRIPTOR) C(SPSLAM_REFRESH_NORMAL_DEPTH) C(SPSLAM_REFRESH_DONE)
  C(SPSLAM_REFRESH_UNTOUCHED) C(SPSLAM_REFRESH_CAPACITY) C(SPSLAM_ERR_CAPACITY)
  return 0;
}
"""


def test_local_mapping_struct_layouts_match_bindings(tmp_path):
    import spslam_match as M
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = {k: int(v) for k, v in (line.split() for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    for name, dt in (("spslam_fuse_problem", M.FUSE_PROBLEM_DTYPE), ("spslam_fuse_result", M.FUSE_RESULT_DTYPE)):
        assert got[name] == dt.itemsize, name
        fields = [k.split(".", 1)[1] for k in got if k.startswith(name + ".")]
        assert sorted(fields) == sorted(dt.names)
        for f in fields:
            assert dt.fields[f][1] == got[f"{name}.{f}"], (name, f)
    assert got["spslam_fuse_problem"] == 80 and got["spslam_fuse_result"] == 8
    for name, st in (("spslam_fuse_params", M.FuseParams), ("spslam_point_refresh_map", M.PointRefreshMap)):
        assert got[name] == ctypes.sizeof(st), name
        for key, off in got.items():
            if key.startswith(name + "."):
                assert getattr(st, key.split(".", 1)[1]).offset == off, key
    assert [f for f, _ in M.PointRefreshMap._fields_] == [n for n, _ in M.REFRESH_MAP_TABLES] + ["points"]
    assert [got[f"SPSLAM_FUSE_{s}"] for s in ("SEARCHED", "SKIPPED", "BEHIND", "OUTSIDE_IMAGE", "OUT_OF_RANGE",
                                               "VIEW_ANGLE", "NO_CANDIDATES")] == \
        [M.FUSE_SEARCHED, M.FUSE_SKIPPED, M.FUSE_BEHIND, M.FUSE_OUTSIDE_IMAGE, M.FUSE_OUT_OF_RANGE, M.FUSE_VIEW_ANGLE,
         M.FUSE_NO_CANDIDATES]
    assert got["SPSLAM_POINT_MAX_OBS"] == M.POINT_MAX_OBS >= 128
    assert (got["SPSLAM_REFRESH_DESCRIPTOR"], got["SPSLAM_REFRESH_NORMAL_DEPTH"]) == \
        (M.REFRESH_DESCRIPTOR, M.REFRESH_NORMAL_DEPTH)
    assert (got["SPSLAM_REFRESH_DONE"], got["SPSLAM_REFRESH_UNTOUCHED"], got["SPSLAM_REFRESH_CAPACITY"]) == \
        (M.REFRESH_DONE, M.REFRESH_UNTOUCHED, M.REFRESH_CAPACITY)
    assert got["SPSLAM_ERR_CAPACITY"] == M.ERR_CAPACITY


def test_local_mapping_entry_points_are_exported():
    import spslam_gpu
    import spslam_match  # noqa: F401  (registers its entry points)
    lib = spslam_gpu.load_library()
    for name in ("spslam_fuse_search", "spslam_fuse_search_batch_device", "spslam_map_points_refresh",
                 "spslam_map_points_refresh_batch_device"):
        assert name in spslam_gpu.EXPORTED and hasattr(lib, name), name


def test_restatements_use_the_abi_constants():
    import fuse_ref as FR
    import point_refresh_ref as PR
    import spslam_match as M
    assert FR.RESULT_DTYPE == M.FUSE_RESULT_DTYPE and FR.TH_LOW == M.TH_LOW
    assert (FR.SEARCHED, FR.SKIPPED, FR.BEHIND, FR.OUTSIDE_IMAGE, FR.OUT_OF_RANGE, FR.VIEW_ANGLE, FR.NO_CANDIDATES) == \
        (M.FUSE_SEARCHED, M.FUSE_SKIPPED, M.FUSE_BEHIND, M.FUSE_OUTSIDE_IMAGE, M.FUSE_OUT_OF_RANGE, M.FUSE_VIEW_ANGLE,
         M.FUSE_NO_CANDIDATES)
    assert (PR.DESCRIPTOR, PR.NORMAL_DEPTH, PR.DONE, PR.UNTOUCHED, PR.CAPACITY, PR.MAX_OBS) == \
        (M.REFRESH_DESCRIPTOR, M.REFRESH_NORMAL_DEPTH, M.REFRESH_DONE, M.REFRESH_UNTOUCHED, M.REFRESH_CAPACITY,
         M.POINT_MAX_OBS)
