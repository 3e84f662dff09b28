"""CPU checks of the CreateNewMapPoints records of include/spslam_gpu.h: struct sizes and field offsets match the
Python bindings, the entry points are exported, the constants agree with the bindings and the restatement, and bad
arguments come back as SPSLAM_ERR_ARG before anything touches a device."""
import ctypes
import pathlib
import subprocess

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]

ENTRIES = ("spslam_search_for_triangulation", "spslam_search_for_triangulation_batch_device", "spslam_triangulate",
           "spslam_triangulate_batch_device", "spslam_create_new_points_batch_device")
SIDE_FIELDS = ("keys", "keys_un", "uright", "depth", "desc", "has_point", "counts", "fv_nodes", "fv_start",
               "fv_features", "n_fv", "cap", "pad")
PAIR_FIELDS = ("kf1", "kf2", "Tcw1", "Tcw2", "Ow1", "Ow2", "F12", "out_offset", "flags")
RESULT_FIELDS = ("x", "y", "z", "idx2", "status", "source", "pad")
KEYFRAME_FIELDS = ("keys", "keys_un", "uright", "depth", "desc", "has_point", "fv_nodes", "fv_start", "fv_features",
                   "n", "n_fv", "Tcw", "Ow", "pad")
STATUS = ("NEW", "NO_MATCH", "LOW_PARALLAX", "W_ZERO", "BEHIND_1", "BEHIND_2", "REPROJ_1", "REPROJ_2", "ZERO_DIST",
          "SCALE")
CONSTANTS = tuple(f"SPSLAM_TRI_{s}" for s in STATUS) + (
    "SPSLAM_TRI_FROM_SVD", "SPSLAM_TRI_FROM_STEREO_1", "SPSLAM_TRI_FROM_STEREO_2", "SPSLAM_TRI_PAIR_SEARCHED",
    "SPSLAM_TRI_PAIR_SKIPPED", "SPSLAM_TRI_PAIR_SHORT_BASELINE", "SPSLAM_TRI_PAIR_SKIP", "SPSLAM_ERR_ARG")


def _layout_source():
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "spslam_gpu.h"', "int main(void) {"]
    for name, fields in (("spslam_tri_side", SIDE_FIELDS), ("spslam_tri_pair", PAIR_FIELDS),
                         ("spslam_tri_result", RESULT_FIELDS), ("spslam_tri_keyframe", KEYFRAME_FIELDS)):
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += [f'  printf("{c} %d\\n", (int){c});' for c in CONSTANTS]
    return "\n".join(lines + ["  return 0;", "}"])


def test_create_points_struct_layouts_match_bindings(tmp_path):
    import spslam_match as M
    src = tmp_path / "layout.c"
    src.write_text(_layout_source())
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = {k: int(v) for k, v in (line.split() for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    for name, dt in (("spslam_tri_pair", M.TRI_PAIR_DTYPE), ("spslam_tri_result", M.TRI_RESULT_DTYPE)):
        assert got[name] == dt.itemsize, name
        fields = [k.split(".", 1)[1] for k in got if k.startswith(name + ".")]
        assert sorted(fields) == sorted(dt.names)
        for f in fields:
            assert dt.fields[f][1] == got[f"{name}.{f}"], (name, f)
    assert got["spslam_tri_pair"] == 172 and got["spslam_tri_result"] == 20
    for name, st in (("spslam_tri_side", M.TriSide), ("spslam_tri_keyframe", M.TriKeyframe)):
        assert got[name] == ctypes.sizeof(st), name
        fields = [k.split(".", 1)[1] for k in got if k.startswith(name + ".")]
        assert fields == [f for f, _ in st._fields_], name
        for f in fields:
            assert getattr(st, f).offset == got[f"{name}.{f}"], (name, f)
    assert [f for f, _ in M.TriSide._fields_][:len(M.TRI_SIDE_ARRAYS)] == list(M.TRI_SIDE_ARRAYS)
    assert [got[f"SPSLAM_TRI_{s}"] for s in STATUS] == \
        [M.TRI_NEW, M.TRI_NO_MATCH, M.TRI_LOW_PARALLAX, M.TRI_W_ZERO, M.TRI_BEHIND_1, M.TRI_BEHIND_2, M.TRI_REPROJ_1,
         M.TRI_REPROJ_2, M.TRI_ZERO_DIST, M.TRI_SCALE] == list(range(10))
    assert (got["SPSLAM_TRI_FROM_SVD"], got["SPSLAM_TRI_FROM_STEREO_1"], got["SPSLAM_TRI_FROM_STEREO_2"]) == \
        (M.TRI_FROM_SVD, M.TRI_FROM_STEREO_1, M.TRI_FROM_STEREO_2)
    assert (got["SPSLAM_TRI_PAIR_SEARCHED"], got["SPSLAM_TRI_PAIR_SKIPPED"], got["SPSLAM_TRI_PAIR_SHORT_BASELINE"]) == \
        (M.TRI_PAIR_SEARCHED, M.TRI_PAIR_SKIPPED, M.TRI_PAIR_SHORT_BASELINE)
    assert got["SPSLAM_TRI_PAIR_SKIP"] == M.TRI_PAIR_SKIP


def test_create_points_entry_points_are_exported():
    import spslam_gpu
    import spslam_match  # noqa: F401  (registers its entry points)
    lib = spslam_gpu.load_library()
    for name in ENTRIES:
        assert name in spslam_gpu.EXPORTED and hasattr(lib, name), name


def test_restatement_uses_the_abi_constants():
    import spslam_match as M
    import triangulation_cases as TC
    import triangulation_ref as TR
    assert TR.RESULT_DTYPE == M.TRI_RESULT_DTYPE and TR.TH_LOW == M.TH_LOW
    assert (TR.NEW, TR.NO_MATCH, TR.LOW_PARALLAX, TR.W_ZERO, TR.BEHIND_1, TR.BEHIND_2, TR.REPROJ_1, TR.REPROJ_2,
            TR.ZERO_DIST, TR.SCALE) == tuple(range(10))
    assert (TR.FROM_SVD, TR.FROM_STEREO_1, TR.FROM_STEREO_2) == (M.TRI_FROM_SVD, M.TRI_FROM_STEREO_1,
                                                                 M.TRI_FROM_STEREO_2)
    assert (TR.SEARCHED, TR.SKIPPED, TR.SHORT_BASELINE) == (M.TRI_PAIR_SEARCHED, M.TRI_PAIR_SKIPPED,
                                                            M.TRI_PAIR_SHORT_BASELINE)
    src = (ROOT / "sp-slam_amd" / "csrc" / "bow_launch.h").read_text()
    assert f"#define SPSLAM_TRI_GROUP {TC.GROUP}\n" in src


def test_bad_arguments_return_err_arg_without_a_device():
    """A NULL context is refused by every entry before any HIP call, so this runs where there is no GPU."""
    import spslam_gpu
    import spslam_match as M
    lib = spslam_gpu.load_library()
    M._bind_tri(lib)
    side = M.TriSide()
    kf = M.TriKeyframe()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    err = -1
    assert lib.spslam_search_for_triangulation_batch_device(None, 1, p, ctypes.byref(side), 0, 0, p, p, None) == err
    assert lib.spslam_triangulate_batch_device(None, 1, p, ctypes.byref(side), p, 0, p, p, None) == err
    assert lib.spslam_create_new_points_batch_device(None, 1, p, ctypes.byref(side), p, p, p, p, p, None) == err
    assert lib.spslam_search_for_triangulation(None, ctypes.byref(kf), ctypes.byref(kf), p, p, 0, 0) == err
    assert lib.spslam_triangulate(None, ctypes.byref(kf), ctypes.byref(kf), p, 0, p, p) == err
