"""Times spslam_pnp_solver_batch_device with HIP events: warm, one event pair per call, the median over the repeats;
every timed configuration is compared with the referee (tests/pnp_ref.cpp) first.
  python tools/pnp_timing.py [--repeats 30] [--dry]
Shape: 1, 16 and 256 problems per call of N about 60 and about 300 kept correspondences at Tracking's parameters
(0.99, 10, 300, 4, 0.5, 5.991: mRansacMaxIts 35), one iterate(5) of a new solver each: 60 % true correspondences with
half a sigma of pixel noise, 40 % wrong.  The device evaluates every hypothesis of the call's range and one Refine per
candidate mask; the referee, single-threaded, stops where its loop returns, which is what a caller of the reference
pays.  --dry builds the inputs and runs the referee only (no device)."""
import argparse
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT / "sp-slam_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

import pnp_cases as C  # noqa: E402

DISTINCT = 8


def inputs(n):
    """DISTINCT problems of about n kept correspondences among n + 40 frame keypoints."""
    B = C.Builder()
    for q in range(DISTINCT):
        m = n + q
        B.add(f"n{m}", C.mixed(m - 2 * m // 5, 2 * m // 5, 500 + q), 500 + n + q, n_frame=m + 40, n_kf=m + 60, noise=0.5,
              calls=(5,))
    return np.array(B.rows, B.dtype), np.array(B.bad, np.uint8), B.cases


def referee(points, bad, cases):
    C.compiled("pnp_ref")
    out, ms = [], []
    for c in cases:
        t = time.perf_counter()
        w = C.reference(c, points, bad)
        ms.append((time.perf_counter() - t) * 1e3)
        out.append(w)
    return out, ms


def device(points, bad, cases, want, counts, repeats):
    import torch
    import spslam_frame
    import spslam_gpu
    import spslam_loop
    import spslam_reloc
    import synth
    import test_gpu_pnp as T
    K = synth.TUM3
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], (0,) * 5, K["bf"], 640, 480)
    times = []

    def timed(call):
        """The same launch repeated, each bracketed by events.  A new solver's call does not read the best mask
        (best_inliers is 0), so every repeat computes the same."""
        for q in range(5 + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if q >= 5:
                times.append(e0.elapsed_time(e1))

    out = []
    for P in counts:
        reps = (P + len(cases) - 1) // len(cases)
        items = [T.item(c, w, 0) for _ in range(reps) for c, w in zip(cases, want)][:P]
        wants = [(w, 0) for _ in range(reps) for w in want][:P]
        gpu = (ex, spslam_reloc, spslam_loop.LoopMatcher(ex))
        T.check(T.run_batch(gpu, points, bad, items), items, wants)          # the parity run (and the warm-up)
        times.clear()
        T.check(T.run_batch(gpu, points, bad, items, launch=timed), items, wants)
        out.append((P, statistics.median(times), min(times), max(times)))
    ex.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    for n in (60, 300):
        points, bad, cases = inputs(n)
        want, ms = referee(points, bad, cases)
        want, ms = referee(points, bad, cases)                               # the second pass: warm caches
        res = [w["results"][0] for w in want]
        print(f"N {[int(r['n']) for r in res]}, mRansacMaxIts {[int(r['max_its']) for r in res]}, "
              f"statuses {[int(r['status']) for r in res]}, iterations the referee ran "
              f"{[int(r['iterations_done']) for r in res]}, Refine calls {[int(w['trace']['refine_ran'].sum()) for w in want]}")
        per = statistics.mean(ms)
        print(f"  referee, one thread, one problem: {' / '.join(f'{m:.2f}' for m in ms)} ms (mean {per:.2f} ms; "
              f"16 problems {16 * per:.1f} ms, 256 problems {256 * per:.0f} ms)")
        if not a.dry:
            for P, med, lo, hi in device(points, bad, cases, want, (1, 16, 256), a.repeats):
                print(f"  device, {P} problems in one call (gather + hypotheses + refine and select): median "
                      f"{med * 1e3:.0f} us (min {lo * 1e3:.0f}, max {hi * 1e3:.0f}) over {a.repeats} calls; "
                      f"referee / device {P * per / med:.1f}")


if __name__ == "__main__":
    main()
