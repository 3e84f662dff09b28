"""Times spslam_sim3_optimize_batch_device with HIP events: warm, one event pair per call, the median over the repeats;
every timed configuration is compared with the referee (tests/sim3_opt_ref.cpp) in the same run.
  python tools/sim3_opt_timing.py [--repeats 50] [--dry]
Shape: 8 sequences, one pair each per call, with about 60 and about 150 kept correspondences, a tenth of them planted
outliers, started 0.04 rad and 5 cm off the truth.  The call rewrites match12 in place, so the input is put back (a
device-to-device copy outside the events) before every repeat.  --dry builds the inputs and runs the referee only."""
import argparse
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT / "sp-slam_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

import sim3_opt_cases as C  # noqa: E402

N_SEQ = 8


def inputs(n):
    B = C.Builder()
    for q in range(N_SEQ):
        m = n + q
        B.case(f"n{m}", m - m // 10, m // 10, seed=500 + m, start=C.OFF, extra=40)
    return np.array(B.rows, B.dtype), np.array(B.bad, np.uint8), B.cases


def referee(points, bad, cases):
    C.reference(cases[0], points, bad)                                 # compiles the referee
    out, ms = [], []
    for c in cases:
        t = time.perf_counter()
        out.append(C.reference(c, points, bad))
        ms.append((time.perf_counter() - t) * 1e3)
    return out, ms


def device(points, bad, cases, want, repeats):
    import torch
    import spslam_frame
    import spslam_gpu
    import spslam_loop
    import synth
    import test_gpu_sim3_opt as T
    K = synth.TUM3
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], (0,) * 5, K["bf"], 640, 480)
    gpu = {"TUM3": (ex, spslam_loop.LoopMatcher(ex))}
    T.check(T.run_batch(gpu, points, bad, cases), cases, want)          # the parity run (and the warm-up)
    times = []

    def launch(call, d_match12):
        keep = d_match12.clone()
        for q in range(5 + repeats):
            d_match12.copy_(keep)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if q >= 5:
                times.append(e0.elapsed_time(e1))

    T.check(T.run_batch(gpu, points, bad, cases, launch=launch), cases, want)
    ex.close()
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    for n in (60, 150):
        points, bad, cases = inputs(n)
        want, ms = referee(points, bad, cases)
        r = [w["result"] for w in want]
        print(f"n_corr {[int(x['n_corr']) for x in r]}, n_bad {[int(x['n_bad']) for x in r]}, n_in {[int(x['n_in']) for x in r]}, "
              f"LM iterations {[int(x['iterations1']) + int(x['iterations2']) for x in r]}, "
              f"trials {[int(x['trials1']) + int(x['trials2']) for x in r]}")
        print(f"  referee (C++, sequential), one pair: {' / '.join(f'{m:.2f}' for m in ms)} ms; the call's {N_SEQ} pairs: "
              f"{sum(ms):.2f} ms")
        if not a.dry:
            med, lo, hi = device(points, bad, cases, want, a.repeats)
            print(f"  device, {N_SEQ} pairs in one call (gather + both optimize calls + checks + Scw, one launch): "
                  f"median {med * 1e3:.0f} us (min {lo * 1e3:.0f}, max {hi * 1e3:.0f}) over {a.repeats} calls")


if __name__ == "__main__":
    main()
