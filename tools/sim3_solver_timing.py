"""Times spslam_sim3_solver_batch_device with HIP events: warm, one event pair per call, the median over the repeats;
every timed configuration is compared with the Python referee (tests/sim3_solver_ref.py) afterwards.
  python tools/sim3_solver_timing.py [--repeats 50] [--dry]
Shape: 8 sequences x 3 candidates = 24 problems per call, every problem 300 hypotheses in the one call (the solver's
mnBestInliers is set above any count, so no hypothesis ends the call early and the referee runs all 300 too), with N
around 30 (min_inliers 3, so that mRansacMaxIts is 300) and around 150 (ComputeSim3's 0.99, 20, 300).  --dry builds
the inputs and runs the referee only (no device)."""
import argparse
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT / "sp-slam_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

import sim3_solver_cases as C  # noqa: E402

N_SEQ, N_CAND, NEVER = 8, 3, 1 << 20


def inputs(n, min_inliers):
    """Three candidates of about n correspondences among 200 keypoints; a third of them outliers."""
    B = C.Builder()
    for cand in range(N_CAND):
        m = n + cand
        X1, X2 = C.scene(m - m // 3, m // 3, 100 + cand, noise=0.002)
        B.add(f"n{m}", *B.pair(200, 190, X1, X2, 100 + cand), C.random_draws(100 + cand, 900), min_inliers=min_inliers,
              calls=(300,), state=(0, NEVER))
    return np.array(B.rows, B.dtype), np.array(B.bad, np.uint8), B.cases


def referee(points, bad, cases):
    out, ms = [], []
    for c in cases:
        s = C.new_solver(c, points, bad)
        t = time.perf_counter()
        T12, no_more, inl, n = s.iterate(300)
        ms.append((time.perf_counter() - t) * 1e3)
        assert T12 is None and s.mnIterations == 300 and s.mRansacMaxIts == 300
        out.append((s.result(T12, no_more, n), inl, s.N, max(s.trace["counts"])))
    return out, ms


def device(points, bad, cases, want, repeats):
    import torch
    import spslam_frame
    import spslam_gpu
    import spslam_loop
    import synth
    import test_gpu_sim3_solver as T
    K = synth.TUM3
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], (0,) * 5, K["bf"], 640, 480)
    gpu = (ex, spslam_loop.LoopMatcher(ex))
    items = [(c, c["state"], 300) for _ in range(N_SEQ) for c in cases]
    got, _ = T.run_batch(gpu, points, bad, items)                     # the parity run (and the warm-up)
    for (res, inl, _, _), (w, w_inl, _, _) in zip(got, want * N_SEQ):
        assert res.tobytes() == w.tobytes() and inl.tobytes() == w_inl.tobytes(), "differs from the referee"
    times = []

    class Timed:
        """LoopMatcher whose solver call is bracketed by events, the same launch repeated."""
        def __getattr__(self, name):
            return getattr(gpu[1], name)

        def sim3_solver_batch_device(self, *a, **kw):
            for q in range(5 + repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gpu[1].sim3_solver_batch_device(*a, **kw)
                e1.record()
                e1.synchronize()
                if q >= 5:
                    times.append(e0.elapsed_time(e1))

    T.run_batch((ex, Timed()), points, bad, items)
    ex.close()
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    for n, mn in ((30, 3), (150, 20)):
        points, bad, cases = inputs(n, mn)
        want, ms = referee(points, bad, cases)
        ns = [w[2] for w in want]
        print(f"N {ns} (min_inliers {mn}), 300 hypotheses per problem; the most inliers of a hypothesis: "
              f"{[w[3] for w in want]}")
        print(f"  referee, sequential, one problem of 300 iterations: {' / '.join(f'{m:.0f}' for m in ms)} ms "
              f"(x {N_SEQ} sequences: {sum(ms) * N_SEQ / 1e3:.1f} s per call's worth)")
        if not a.dry:
            med, lo, hi = device(points, bad, cases, want, a.repeats)
            print(f"  device, {N_SEQ * N_CAND} problems x 300 hypotheses in one call (gather + hypotheses + selection): "
                  f"median {med * 1e3:.0f} us (min {lo * 1e3:.0f}, max {hi * 1e3:.0f}) over {a.repeats} calls")


if __name__ == "__main__":
    main()
