"""CPU checks of the Sim3Solver records of include/spslam_gpu.h: struct sizes and field offsets match the Python
bindings, the entry points are exported, bad arguments come back as SPSLAM_ERR_ARG before anything touches a device,
and the host form's index checks (sp-slam_amd/csrc/loop_check.h) refuse each bad index."""
import ctypes
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]

RECORDS = {"spslam_sim3_problem": "SIM3_PROBLEM_DTYPE", "spslam_sim3_result": "SIM3_RESULT_DTYPE"}
FIELDS = {
    "spslam_sim3_problem": "kf1 kf2 match_offset rand_offset inlier_offset iterations_done best_inliers n_iterations",
    "spslam_sim3_result": "status n iterations_done best_inliers n_inliers s12 R12 t12 T12",
    "spslam_sim3_solver_params": "min_inliers max_iterations rand_max fix_scale",
}
CONSTANTS = "SPSLAM_SIM3_FOUND SPSLAM_SIM3_NOT_YET SPSLAM_SIM3_NO_MORE SPSLAM_SIM3_MAX_ITERATIONS SPSLAM_ERR_ARG".split()
ENTRIES = ("spslam_sim3_ransac_table", "spslam_sim3_solver", "spslam_sim3_solver_batch_device",
           "spslam_debug_fill_loop_scratch")


def test_sim3_solver_struct_layouts_match_bindings(tmp_path):
    import sim3_solver_ref as SR
    import spslam_loop as L
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "spslam_gpu.h"', "int main(void) {"]
    for name, fields in FIELDS.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields.split()]
    lines += [f'  printf("{c} %d\\n", (int){c});' for c in CONSTANTS]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = {k: int(v) for k, v in (line.split() for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    for name, binding in RECORDS.items():
        dt = getattr(L, binding)
        assert got[name] == dt.itemsize and FIELDS[name].split() == list(dt.names), name
        for f in dt.names:
            assert dt.fields[f][1] == got[f"{name}.{f}"], (name, f)
    assert [got[n] for n in RECORDS] == [32, 136]
    st = L.Sim3SolverParams
    assert got["spslam_sim3_solver_params"] == ctypes.sizeof(st) == 16
    for f in FIELDS["spslam_sim3_solver_params"].split():
        assert getattr(st, f).offset == got[f"spslam_sim3_solver_params.{f}"], f
    assert (got["SPSLAM_SIM3_FOUND"], got["SPSLAM_SIM3_NOT_YET"], got["SPSLAM_SIM3_NO_MORE"]) == \
        (L.SIM3_FOUND, L.SIM3_NOT_YET, L.SIM3_NO_MORE) == (SR.FOUND, SR.NOT_YET, SR.NO_MORE)
    assert got["SPSLAM_SIM3_MAX_ITERATIONS"] == L.SIM3_MAX_ITERATIONS
    assert SR.RESULT_DTYPE == L.SIM3_RESULT_DTYPE
    # the scratch records the header states: 56 bytes per correspondence, 64 per hypothesis
    math = (ROOT / "sp-slam_amd" / "csrc" / "sim3_math.h").read_text()
    assert "sizeof(Corr) == 56" in math and "sizeof(Hyp) == 64" in math


def test_sim3_solver_entry_points_are_exported():
    import spslam_gpu
    import spslam_loop  # noqa: F401  (registers its entry points)
    lib = spslam_gpu.load_library()
    for name in ENTRIES:
        assert name in spslam_gpu.EXPORTED and hasattr(lib, name), name


def test_bad_arguments_return_err_arg_without_a_device():
    import spslam_gpu
    import spslam_loop as L
    lib = spslam_gpu.load_library()
    L._bind(lib)
    p, err = ctypes.c_void_p(8), -1
    par = L.Sim3SolverParams(20, 300, L.RAND_MAX, 1)
    smap = L.Sim3Map()
    kf = L.Sim3Keyframe()
    assert lib.spslam_sim3_solver_batch_device(None, 1, p, ctypes.byref(smap), p, p, 8, p, p, p, ctypes.byref(par), p, p,
                                               None, None, None) == err
    one = ctypes.c_int(0)
    assert lib.spslam_sim3_solver(None, ctypes.byref(kf), ctypes.byref(kf), p, None, 1, p, p, ctypes.byref(par), 0.99, 5,
                                  ctypes.byref(one), ctypes.byref(one), p, p, None) == err
    assert lib.spslam_sim3_ransac_table(0.99, 20, 300, -1, p) == err
    assert lib.spslam_sim3_ransac_table(0.99, 20, 0, 8, p) == err
    assert lib.spslam_debug_fill_loop_scratch(None, 0) == err


def test_host_form_checks_refuse_each_bad_index(tmp_path):
    """The checks spslam_sim3_solver runs before it stages anything, in the stand-alone program that also serves a
    host sanitizer: match_row and match12 ranges, octaves against the levels, min_inliers >= 3, n_iterations >= 0,
    the state and the draws."""
    src = (ROOT / "tools" / "loop_check_main.cpp").read_text()
    for what in ("loop_check_solver_keyframe", "loop_check_solver_call", "an octave == n_levels", "min_inliers 2",
                 "n_iterations -1", "a draw above rand_max", "a match == n2", "a row == n_rows"):
        assert what in src, what
    capi = (ROOT / "sp-slam_amd" / "csrc" / "capi_loop_closing.cpp").read_text()
    body = capi[capi.index("int spslam_sim3_solver(spslam_ctx* c"):capi.index("int spslam_debug_fill_loop_scratch")]
    staged = body.index("Stage st(c)")
    for check in ("loop_check_solver_keyframe(", "loop_check_match12(", "loop_check_solver_call("):
        assert 0 <= body.index(check) < staged, check                  # every check runs before the staging
    exe = tmp_path / "loop_check"
    subprocess.run(["g++", "-std=c++17", "-O1", str(ROOT / "tools" / "loop_check_main.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks hold" in out.stdout, out.stdout
