"""CPU checks of the place-recognition records of include/spslam_gpu.h: struct sizes and field offsets match the
Python bindings, the entry points are exported, and the constants agree with the bindings, the cases and the
referee."""
import ctypes
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]

RECORDS = {"spslam_place_problem": "PLACE_PROBLEM_DTYPE", "spslam_place_result": "PLACE_RESULT_DTYPE"}
STRUCTS = {"spslam_place_db": "PlaceDb", "spslam_place_frames": "PlaceFrames"}
FIELDS = {
    "spslam_place_problem": "kf_base n_kf query out_offset",
    "spslam_place_result": "status n_sharing max_common_words min_common_words n_scored n_kept n_candidates "
                           "best_acc_score",
    "spslam_place_db": "bow_words bow_values n_bow in_db reloc_score loop_score cap pad",
    "spslam_place_frames": "bow_words bow_values n_bow cap pad",
}
CONSTANTS = ("SPSLAM_PLACE_MAX_WORDS SPSLAM_PLACE_OK SPSLAM_PLACE_EMPTY SPSLAM_PLACE_NONE_KEPT SPSLAM_COVIS_MAX_KF "
             "SPSLAM_COVIS_BEST").split()
ENTRIES = ("spslam_place_reloc_candidates", "spslam_place_reloc_candidates_batch_device",
           "spslam_place_loop_candidates", "spslam_place_loop_candidates_batch_device", "spslam_place_min_score",
           "spslam_place_min_score_batch_device")


def layout_source():
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "spslam_gpu.h"', "int main(void) {"]
    for name, fields in FIELDS.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields.split()]
    lines += [f'  printf("{c} %d\\n", (int){c});' for c in CONSTANTS]
    return "\n".join(lines + ["  return 0;", "}", ""])


def test_place_struct_layouts_match_bindings(tmp_path):
    import spslam_place as P
    src = tmp_path / "layout.c"
    src.write_text(layout_source())
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = {k: int(v) for k, v in (line.split() for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    for name, binding in RECORDS.items():
        dt = getattr(P, binding)
        assert got[name] == dt.itemsize, name
        assert FIELDS[name].split() == list(dt.names), name
        for f in dt.names:
            assert dt.fields[f][1] == got[f"{name}.{f}"], (name, f)
    assert [got[n] for n in RECORDS] == [16, 32]
    for name, binding in STRUCTS.items():
        st = getattr(P, binding)
        assert got[name] == ctypes.sizeof(st), name
        assert [f for f, _ in st._fields_] == FIELDS[name].split(), name
        for f in FIELDS[name].split():
            assert getattr(st, f).offset == got[f"{name}.{f}"], (name, f)
    assert [f for f, _ in P.PlaceDb._fields_][:-2] == [n for n, _ in P.PLACE_DB_TABLES]
    assert [f for f, _ in P.PlaceFrames._fields_][:-2] == [n for n, _ in P.PLACE_FRAME_TABLES]
    assert got["SPSLAM_PLACE_MAX_WORDS"] == P.PLACE_MAX_WORDS == 8192
    assert [got[f"SPSLAM_PLACE_{s}"] for s in ("OK", "EMPTY", "NONE_KEPT")] == \
        [P.PLACE_OK, P.PLACE_EMPTY, P.PLACE_NONE_KEPT] == [0, 1, 2]
    assert (got["SPSLAM_COVIS_MAX_KF"], got["SPSLAM_COVIS_BEST"]) == (P.COVIS_MAX_KF, P.COVIS_BEST)


def test_place_entry_points_are_exported():
    import spslam_gpu
    import spslam_place  # noqa: F401  (registers its entry points)
    lib = spslam_gpu.load_library()
    for name in ENTRIES:
        assert name in spslam_gpu.EXPORTED and hasattr(lib, name), name


def test_cases_and_referee_use_the_abi_constants():
    import place_cases as PC
    import place_ref as PR
    import spslam_place as P
    assert (PR.OK, PR.EMPTY, PR.NONE_KEPT) == (P.PLACE_OK, P.PLACE_EMPTY, P.PLACE_NONE_KEPT)
    assert PC.PROBLEM_DTYPE == P.PLACE_PROBLEM_DTYPE and PC.RESULT_DTYPE == P.PLACE_RESULT_DTYPE
    assert PC.BEST == P.COVIS_BEST and PC.LENGTHS_CAP <= P.PLACE_MAX_WORDS
