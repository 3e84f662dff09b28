"""CPU checks of the OptimizeSim3 records of include/spslam_gpu.h: struct sizes and field offsets match the Python
bindings, the entry points are exported, bad arguments come back as SPSLAM_ERR_ARG before anything touches a device,
and the host form's checks (sp-slam_amd/csrc/loop_check.h) refuse fix_scale = 0, th2 <= 0 and each bad index."""
import ctypes
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]

FIELDS = {
    "spslam_sim3_opt_result": "n_in n_corr n_bad status accepted iterations1 trials1 iterations2 trials2 pad S12 Scw mScw",
    "spslam_sim3_opt_params": "th2 fix_scale min_inliers pad",
}
OFFSETS = dict(n_in=0, n_corr=4, n_bad=8, status=12, accepted=16, iterations1=20, trials1=24, iterations2=28, trials2=32,
               pad=36, S12=40, Scw=104, mScw=168)                       # as the header states them
CONSTANTS = "SPSLAM_SIM3_OPT_OK SPSLAM_SIM3_OPT_TOO_FEW SPSLAM_ERR_ARG".split()
ENTRIES = ("spslam_sim3_optimize", "spslam_sim3_optimize_batch_device", "spslam_debug_fill_loop_scratch")


def test_sim3_opt_struct_layouts_match_bindings(tmp_path):
    import sim3_opt_cases as C
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
    dt = L.SIM3_OPT_RESULT_DTYPE
    assert got["spslam_sim3_opt_result"] == dt.itemsize == 232
    assert FIELDS["spslam_sim3_opt_result"].split() == list(dt.names)
    for f in dt.names:
        assert dt.fields[f][1] == got[f"spslam_sim3_opt_result.{f}"] == OFFSETS[f], f
    assert C.RESULT_DTYPE == dt                                        # the referee's record is the same
    st = L.Sim3OptParams
    assert got["spslam_sim3_opt_params"] == ctypes.sizeof(st) == 16
    for f in FIELDS["spslam_sim3_opt_params"].split():
        assert getattr(st, f).offset == got[f"spslam_sim3_opt_params.{f}"], f
    assert (got["SPSLAM_SIM3_OPT_OK"], got["SPSLAM_SIM3_OPT_TOO_FEW"]) == (L.SIM3_OPT_OK, L.SIM3_OPT_TOO_FEW) == (C.OK, C.TOO_FEW)
    # the scratch record the header states: 104 bytes per keypoint slot; the seams the cases name
    math = (ROOT / "sp-slam_amd" / "csrc" / "sim3_opt_math.h").read_text()
    assert "sizeof(Corr) == 104" in math and L.SIM3_OPT_CORR_BYTES == 104
    header = (ROOT / "include" / "spslam_gpu.h").read_text()
    assert "16 + 104 * cap" in header
    kernel = (ROOT / "sp-slam_amd" / "csrc" / "sim3_opt_kernels.hip").read_text()
    assert "kThreads = 256" in kernel and "kChunk = kThreads / 2" in kernel
    assert (C.GATHER, C.CHUNK, C.WAVE) == (256, 128, 32)


def test_sim3_opt_entry_points_are_exported():
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
    smap, kf = L.Sim3Map(), L.Sim3Keyframe()
    for par in (L.Sim3OptParams(10.0, 1, 20, 0), L.Sim3OptParams(10.0, 0, 20, 0), L.Sim3OptParams(0.0, 1, 20, 0),
                L.Sim3OptParams(-1.0, 1, 20, 0)):
        assert lib.spslam_sim3_optimize_batch_device(None, 1, p, ctypes.byref(smap), p, p, 8, ctypes.byref(par), p, p,
                                                     None) == err
        assert lib.spslam_sim3_optimize(None, ctypes.byref(kf), ctypes.byref(kf), p, None, 1, p, ctypes.byref(par), p,
                                        p) == err


def test_refusals_come_before_anything_is_staged_or_launched(tmp_path):
    """fix_scale = 0, th2 <= 0 and each bad index: the checks the host form runs before it stages anything, in the
    stand-alone program that also serves a host sanitizer; the batch form refuses the parameters before it touches the
    device."""
    src = (ROOT / "tools" / "loop_check_main.cpp").read_text()
    for what in ("loop_check_opt_call", "fix_scale 0", "th2 0", "th2 -10", "th2 NaN", "an octave == n_levels",
                 "a match == n2", "a row == n_rows"):
        assert what in src, what
    capi = (ROOT / "sp-slam_amd" / "csrc" / "capi_loop_closing.cpp").read_text()
    body = capi[capi.index("int spslam_sim3_optimize(spslam_ctx* c"):capi.index("int spslam_debug_fill_loop_scratch")]
    staged = body.index("Stage st(c)")
    for check in ("loop_check_solver_keyframe(", "loop_check_match12(", "loop_check_opt_call("):
        assert 0 <= body.index(check) < staged, check                  # every check runs before the staging
    batch = capi[capi.index("int spslam_sim3_optimize_batch_device(spslam_ctx* c"):capi.index("int spslam_sim3_optimize(spslam_ctx* c")]
    device = batch.index("hipSetDevice")
    assert 0 <= batch.index("params->fix_scale != 1") < device and 0 <= batch.index("!(params->th2 > 0.f)") < device
    exe = tmp_path / "loop_check"
    subprocess.run(["g++", "-std=c++17", "-O1", str(ROOT / "tools" / "loop_check_main.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks hold" in out.stdout, out.stdout
