"""CPU checks of the PnPsolver records of include/spslam_gpu.h: struct sizes and field offsets match the Python
bindings and the referee's records, the status constants agree, the entry points are exported, bad arguments come back
as SPSLAM_ERR_ARG before anything touches a device, and spslam_pnp_ransac_table is the reference's expression."""
import ctypes
import math
import pathlib
import subprocess

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]

RECORDS = {"spslam_pnp_problem": "PNP_PROBLEM_DTYPE", "spslam_pnp_result": "PNP_RESULT_DTYPE"}
FIELDS = {
    "spslam_pnp_problem": "kf frame_slot match_offset rand_offset inlier_offset best_mask_offset iterations_done "
                          "best_inliers n_iterations rand_iterations pad best_Tcw",
    "spslam_pnp_result": "status n iterations_done best_inliers n_inliers iteration min_inliers max_its best_Tcw Tcw",
    "spslam_pnp_params": "min_inliers max_iterations min_set rand_max epsilon th2",
}
CONSTANTS = ("SPSLAM_PNP_REFINED SPSLAM_PNP_BEST_NO_MORE SPSLAM_PNP_NO_MORE SPSLAM_PNP_OUT_OF_DRAWS "
             "SPSLAM_PNP_MAX_ITERATIONS SPSLAM_ERR_ARG").split()
ENTRIES = ("spslam_pnp_ransac_table", "spslam_pnp_solver", "spslam_pnp_solver_batch_device")


def test_pnp_struct_layouts_match_bindings(tmp_path):
    import pnp_cases as C
    import spslam_reloc as R
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
        dt = getattr(R, binding)
        assert got[name] == dt.itemsize and FIELDS[name].split() == list(dt.names), name
        for f in dt.names:
            assert dt.fields[f][1] == got[f"{name}.{f}"], (name, f)
    assert [got[n] for n in RECORDS] == [112, 160]
    st = R.PnPParams
    assert got["spslam_pnp_params"] == ctypes.sizeof(st) == 24
    for f in FIELDS["spslam_pnp_params"].split():
        assert getattr(st, f).offset == got[f"spslam_pnp_params.{f}"], f
    assert (got["SPSLAM_PNP_REFINED"], got["SPSLAM_PNP_BEST_NO_MORE"], got["SPSLAM_PNP_NO_MORE"], got["SPSLAM_PNP_OUT_OF_DRAWS"]) == \
        (R.PNP_REFINED, R.PNP_BEST_NO_MORE, R.PNP_NO_MORE, R.PNP_OUT_OF_DRAWS) == \
        (C.REFINED, C.BEST_NO_MORE, C.NO_MORE, C.OUT_OF_DRAWS)
    assert got["SPSLAM_PNP_MAX_ITERATIONS"] == R.PNP_MAX_ITERATIONS
    # the referee's and the cases' records are the library's
    assert C.RESULT_DTYPE == R.PNP_RESULT_DTYPE and C.PROBLEM_DTYPE == R.PNP_PROBLEM_DTYPE
    ref = C.compiled("pnp_ref")
    assert (ref.pnp_ref_sizes(0), ref.pnp_ref_sizes(1)) == (R.PNP_RESULT_DTYPE.itemsize, C.TRACE_DTYPE.itemsize)
    # the scratch records the header states: 32 bytes per keypoint slot, 104 per iteration
    text = (ROOT / "sp-slam_amd" / "csrc" / "pnp_math.h").read_text()
    assert "sizeof(Corr) == 32" in text and "sizeof(Hyp) == 104" in text
    assert (R.PNP_CORR_BYTES, R.PNP_HYP_BYTES) == (32, 104)
    assert "16 + 32 * cap + 104 * max_iterations" in (ROOT / "include" / "spslam_gpu.h").read_text()


def test_pnp_entry_points_are_exported():
    import spslam_gpu
    import spslam_reloc  # noqa: F401  (registers its entry points)
    lib = spslam_gpu.load_library()
    for name in ENTRIES:
        assert name in spslam_gpu.EXPORTED and hasattr(lib, name), name


def test_bad_arguments_return_err_arg_without_a_device():
    import spslam_gpu
    import spslam_loop as L
    import spslam_reloc as R
    lib = spslam_gpu.load_library()
    R._bind(lib)
    p, err = ctypes.c_void_p(8), -1
    par = R.PnPParams(10, 300, 4, L.RAND_MAX, 0.5, 5.991)
    smap = L.Sim3Map()
    assert lib.spslam_pnp_solver_batch_device(None, 1, p, ctypes.byref(smap), p, p, 8, p, p, p, p, ctypes.byref(par), p, p,
                                              p, None, None) == err
    assert lib.spslam_pnp_solver(None, p, 1, p, p, 1, p, None, 1, p, ctypes.byref(par), 0.99, p, p, p, p, None) == err
    assert lib.spslam_pnp_ransac_table(0.99, 10, 300, 4, 0.5, -1, p, p) == err
    assert lib.spslam_pnp_ransac_table(0.99, 10, 0, 4, 0.5, 8, p, p) == err
    assert lib.spslam_pnp_ransac_table(0.99, 10, 300, 4, 0.5, 8, None, p) == err


def test_ransac_table_is_the_reference_expression_under_trackings_parameters():
    """SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) for N = 0 .. 400, evaluated here step by step: the int times
    the float, the float quotient, pow and log in double, ceil, the clamps; 0 where iterate returns at once."""
    import spslam_gpu
    import spslam_reloc as R
    lib = spslam_gpu.load_library()
    R._bind(lib)
    cap = 400
    max_its, min_n = np.zeros(cap + 1, np.int32), np.zeros(cap + 1, np.int32)
    assert lib.spslam_pnp_ransac_table(0.99, 10, 300, 4, 0.5, cap, max_its.ctypes.data, min_n.ctypes.data) == 0
    for n in range(cap + 1):
        m = max(int(np.float32(n) * np.float32(0.5)), 10, 4)
        assert min_n[n] == m, n
        if n < m:
            assert max_its[n] == 0, n
            continue
        its = 1
        if m != n:
            eps = max(np.float32(0.5), np.float32(m) / np.float32(n))
            its = math.ceil(math.log(1 - 0.99) / math.log(1 - math.pow(float(eps), 3)))
        assert max_its[n] == max(1, min(its, 300)), n
    assert (max_its[9], max_its[10], max_its[15], max_its[20], max_its[400]) == (0, 1, 14, 35, 35)
    assert (min_n[0], min_n[21], min_n[400]) == (10, 10, 200)
    # the cases' own evaluation agrees for both of their parameter sets
    import pnp_cases as C
    for params in (C.TRACKING, C.LONG):
        a, b = np.zeros(cap + 1, np.int32), np.zeros(cap + 1, np.int32)
        lib.spslam_pnp_ransac_table(C.PROBABILITY, params[0], params[1], C.MIN_SET, params[2], cap, a.ctypes.data,
                                    b.ctypes.data)
        wa, wb = C.ransac_tables(params, cap)
        assert np.array_equal(a, wa) and np.array_equal(b, wb), params
    # a quotient no int holds counts as max_iterations
    big_a, big_b = np.zeros(4001, np.int32), np.zeros(4001, np.int32)
    assert lib.spslam_pnp_ransac_table(1 - 1e-12, 4, 300, 4, 1e-4, 4000, big_a.ctypes.data, big_b.ctypes.data) == 0
    assert big_a[4000] == 300
