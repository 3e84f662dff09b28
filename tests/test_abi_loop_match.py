"""CPU checks of the loop-closing records of include/spslam_gpu.h: struct sizes and field offsets match the Python
bindings, the entry points are exported, and the constants agree with the bindings, the cases and the referee."""
import ctypes
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]

RECORDS = {"spslam_sim3_pair": "SIM3_PAIR_DTYPE", "spslam_fuse_problem": "FUSE_PROBLEM_DTYPE",
           "spslam_fuse_result": "FUSE_RESULT_DTYPE"}
STRUCTS = {"spslam_sim3_map": "Sim3Map", "spslam_sim3_params": "Sim3Params", "spslam_bow_keyframe": "BowKeyframe",
           "spslam_sim3_keyframe": "Sim3Keyframe", "spslam_bow_side": "BowSide"}
FIELDS = {
    "spslam_sim3_pair": "kf1 kf2 match_offset result_offset s12 R12 t12 pad",
    "spslam_fuse_problem": "Tcw kf_slot point_offset n_points out_offset",
    "spslam_fuse_result": "best_idx best_dist level status",
    "spslam_sim3_map": "kf_Tcw kf_slot match_off match_row point_bad points",
    "spslam_sim3_params": "th pad",
    "spslam_bow_keyframe": "desc keys_un has_point fv_nodes fv_start fv_features n n_fv",
    "spslam_sim3_keyframe": "Tcw keys_un desc grid_off grid_idx match_row n pad",
    "spslam_bow_side": "desc keys has_point counts fv_nodes fv_start fv_features n_fv cap pad",
}
CONSTANTS = ("SPSLAM_PROJ_SIM3_KEYS SPSLAM_FUSE_SEARCHED SPSLAM_FUSE_SKIPPED SPSLAM_FUSE_BEHIND "
             "SPSLAM_FUSE_OUTSIDE_IMAGE SPSLAM_FUSE_OUT_OF_RANGE SPSLAM_FUSE_VIEW_ANGLE SPSLAM_FUSE_NO_CANDIDATES "
             "SPSLAM_GRID_COLS SPSLAM_GRID_ROWS").split()
ENTRIES = ("spslam_search_by_bow_kf", "spslam_search_by_bow_kf_batch_device", "spslam_search_by_sim3",
           "spslam_search_by_sim3_batch_device", "spslam_search_by_projection_sim3",
           "spslam_search_by_projection_sim3_batch_device", "spslam_fuse_sim3_search",
           "spslam_fuse_sim3_search_batch_device")


def layout_source():
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "spslam_gpu.h"', "int main(void) {"]
    for name, fields in FIELDS.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields.split()]
    lines += [f'  printf("{c} %d\\n", (int){c});' for c in CONSTANTS]
    return "\n".join(lines + ["  return 0;", "}", ""])


def test_loop_struct_layouts_match_bindings(tmp_path):
    import spslam_loop as L
    src = tmp_path / "layout.c"
    src.write_text(layout_source())
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = {k: int(v) for k, v in (line.split() for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    for name, binding in RECORDS.items():
        dt = getattr(L, binding)
        assert got[name] == dt.itemsize, name
        assert FIELDS[name].split() == list(dt.names), name
        for f in dt.names:
            assert dt.fields[f][1] == got[f"{name}.{f}"], (name, f)
    assert [got[n] for n in RECORDS] == [80, 80, 8]
    for name, binding in STRUCTS.items():
        st = getattr(L, binding)
        assert got[name] == ctypes.sizeof(st), name
        assert [f for f, _ in st._fields_] == FIELDS[name].split(), name
        for f in FIELDS[name].split():
            assert getattr(st, f).offset == got[f"{name}.{f}"], (name, f)
    assert [f for f, _ in L.Sim3Map._fields_] == [n for n, _ in L.SIM3_MAP_TABLES]
    assert got["SPSLAM_PROJ_SIM3_KEYS"] == L.PROJ_SIM3_KEYS
    assert (got["SPSLAM_GRID_COLS"], got["SPSLAM_GRID_ROWS"]) == (64, 48)


def test_loop_entry_points_are_exported():
    import spslam_gpu
    import spslam_loop  # noqa: F401  (registers its entry points)
    lib = spslam_gpu.load_library()
    for name in ENTRIES:
        assert name in spslam_gpu.EXPORTED and hasattr(lib, name), name


def test_cases_and_referee_use_the_abi_constants():
    import loop_match_cases as C
    import loop_match_ref as LR
    import spslam_loop as L
    import spslam_match as M
    assert (C.PTS_PER_GROUP, C.PROJ_KEYS, C.BOW_WAVES) == (L.POINTS_PER_GROUP, L.PROJ_SIM3_KEYS, L.BOW_WAVES)
    assert LR.RESULT_DTYPE == L.FUSE_RESULT_DTYPE
    assert (LR.SEARCHED, LR.SKIPPED, LR.BEHIND, LR.OUTSIDE_IMAGE, LR.OUT_OF_RANGE, LR.VIEW_ANGLE,
            LR.NO_CANDIDATES) == (M.FUSE_SEARCHED, M.FUSE_SKIPPED, M.FUSE_BEHIND, M.FUSE_OUTSIDE_IMAGE,
                                  M.FUSE_OUT_OF_RANGE, M.FUSE_VIEW_ANGLE, M.FUSE_NO_CANDIDATES)
    # the kernels' own constants, read from their source: 256 threads at 4 lanes per point, K keys, 4 waves
    kern = (ROOT / "sp-slam_amd" / "csrc" / "match_kernels.hip").read_text()
    launch = (ROOT / "sp-slam_amd" / "csrc" / "match_launch.h").read_text()
    assert "constexpr int kLGrp = 4, kLPtsPerBlock = kThreads / kLGrp;" in kern
    assert "constexpr int kFusePtsPerBlock = kThreads / kLGrp;" in kern and "kThreads = 256" in kern
    assert "constexpr int kSim3Keys = SPSLAM_PROJ_SIM3_KEYS;" in launch
    assert C.PTS_PER_GROUP == 256 // 4 and C.BOW_WAVES == 256 // 64
