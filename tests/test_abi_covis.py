"""CPU checks of the covisibility records of include/spslam_gpu.h (UpdateConnections and the two cullings): struct
sizes and field offsets match the Python bindings, the entry points are exported, and the constants agree with the
bindings and with the referees."""
import ctypes
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]

RECORDS = {"spslam_covis_problem": "COVIS_PROBLEM_DTYPE", "spslam_covis_result": "COVIS_RESULT_DTYPE",
           "spslam_cull_problem": "CULL_PROBLEM_DTYPE", "spslam_cull_record": "CULL_RECORD_DTYPE",
           "spslam_cull_summary": "CULL_SUMMARY_DTYPE"}
STRUCTS = {"spslam_covis_map": "CovisMap", "spslam_covis_graph": "CovisGraph", "spslam_cull_params": "CullParams",
           "spslam_point_cull_map": "PointCullMap"}
FIELDS = {
    "spslam_covis_problem": "kf_base row_base kf n_kf", "spslam_covis_result": "status n_ordered new_parent n_resorted",
    "spslam_cull_problem": "kf_base row_base kf n_kf out_offset pad", "spslam_cull_record": "kf n_mps n_redundant status",
    "spslam_cull_summary": "n_candidates status",
    "spslam_covis_map": "match_off match_row obs_off obs_kf obs_kp kf_slot point_bad points",
    "spslam_covis_graph": "weights ordered ordered_w n_ordered covis parent first_connection stride pad",
    "spslam_cull_params": "th_depth th_obs", "spslam_point_cull_map": "found visible first_kf point_bad points",
}
CONSTANTS = ("SPSLAM_COVIS_MAX_KF SPSLAM_COVIS_BEST SPSLAM_COVIS_UPDATED SPSLAM_COVIS_EMPTY SPSLAM_CULL_KEPT "
             "SPSLAM_CULL_CULLED SPSLAM_CULL_DEFERRED SPSLAM_CULL_SKIPPED SPSLAM_CULL_RAN SPSLAM_CULL_NEW_PLANE "
             "SPSLAM_POINT_CULL_KEEP SPSLAM_POINT_CULL_DROP SPSLAM_POINT_CULL_BAD_RATIO SPSLAM_POINT_CULL_BAD_OBS "
             "SPSLAM_POINT_CULL_EXPIRED").split()
ENTRIES = ("spslam_covis_update_connections", "spslam_covis_update_connections_batch_device",
           "spslam_keyframe_culling", "spslam_keyframe_culling_batch_device", "spslam_map_point_culling",
           "spslam_map_point_culling_batch_device")


def layout_source():
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "spslam_gpu.h"', "int main(void) {"]
    for name, fields in FIELDS.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields.split()]
    lines += [f'  printf("{c} %d\\n", (int){c});' for c in CONSTANTS]
    return "\n".join(lines + ["  return 0;", "}", ""])


def test_covis_struct_layouts_match_bindings(tmp_path):
    import spslam_match as M
    src = tmp_path / "layout.c"
    src.write_text(layout_source())
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = {k: int(v) for k, v in (line.split() for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    for name, binding in RECORDS.items():
        dt = getattr(M, binding)
        assert got[name] == dt.itemsize, name
        assert sorted(FIELDS[name].split()) == sorted(dt.names), name
        for f in dt.names:
            assert dt.fields[f][1] == got[f"{name}.{f}"], (name, f)
    assert [got[n] for n in RECORDS] == [16, 16, 32, 16, 8]
    for name, binding in STRUCTS.items():
        st = getattr(M, binding)
        assert got[name] == ctypes.sizeof(st), name
        assert [f for f, _ in st._fields_] == FIELDS[name].split(), name
        for f in FIELDS[name].split():
            assert getattr(st, f).offset == got[f"{name}.{f}"], (name, f)
    assert [f for f, _ in M.CovisMap._fields_] == [n for n, _ in M.COVIS_MAP_TABLES]
    assert [f for f, _ in M.CovisGraph._fields_][:-2] == [n for n, _ in M.COVIS_GRAPH_TABLES]
    assert [f for f, _ in M.PointCullMap._fields_] == [n for n, _ in M.POINT_CULL_TABLES]
    assert (got["SPSLAM_COVIS_MAX_KF"], got["SPSLAM_COVIS_BEST"]) == (M.COVIS_MAX_KF, M.COVIS_BEST) == (1024, 10)
    assert (got["SPSLAM_COVIS_UPDATED"], got["SPSLAM_COVIS_EMPTY"]) == (M.COVIS_UPDATED, M.COVIS_EMPTY)
    assert [got[f"SPSLAM_CULL_{s}"] for s in ("KEPT", "CULLED", "DEFERRED", "SKIPPED")] == \
        [M.CULL_KEPT, M.CULL_CULLED, M.CULL_DEFERRED, M.CULL_SKIPPED]
    assert (got["SPSLAM_CULL_RAN"], got["SPSLAM_CULL_NEW_PLANE"]) == (M.CULL_RAN, M.CULL_NEW_PLANE)
    assert [got[f"SPSLAM_POINT_CULL_{s}"] for s in ("KEEP", "DROP", "BAD_RATIO", "BAD_OBS", "EXPIRED")] == \
        [M.POINT_CULL_KEEP, M.POINT_CULL_DROP, M.POINT_CULL_BAD_RATIO, M.POINT_CULL_BAD_OBS, M.POINT_CULL_EXPIRED]


def test_covis_entry_points_are_exported():
    import spslam_gpu
    import spslam_match  # noqa: F401  (registers its entry points)
    lib = spslam_gpu.load_library()
    for name in ENTRIES:
        assert name in spslam_gpu.EXPORTED and hasattr(lib, name), name


def test_referees_use_the_abi_constants():
    import covis_ref as CR
    import spslam_match as M
    assert (CR.UPDATED, CR.EMPTY, CR.TH, CR.TH_OBS, CR.BEST) == \
        (M.COVIS_UPDATED, M.COVIS_EMPTY, M.COVIS_TH, M.CULL_TH_OBS, M.COVIS_BEST)
    assert (CR.KEPT, CR.CULLED, CR.DEFERRED, CR.SKIPPED, CR.RAN, CR.NEW_PLANE) == \
        (M.CULL_KEPT, M.CULL_CULLED, M.CULL_DEFERRED, M.CULL_SKIPPED, M.CULL_RAN, M.CULL_NEW_PLANE)
    assert (CR.POINT_KEEP, CR.POINT_DROP, CR.POINT_BAD_RATIO, CR.POINT_BAD_OBS, CR.POINT_EXPIRED) == \
        (M.POINT_CULL_KEEP, M.POINT_CULL_DROP, M.POINT_CULL_BAD_RATIO, M.POINT_CULL_BAD_OBS, M.POINT_CULL_EXPIRED)
