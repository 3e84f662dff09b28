"""Times the place-recognition entries (relocalization candidates, the loop query's reference score, loop candidates)
with HIP events: warm, one event pair per launch, the median over the repeats, beside the Python referee
(tests/place_ref.py) on the same inputs; every timed configuration is compared to the referee afterwards.
  python tools/place_timing.py [--repeats 50] [--dry]
Shapes: C3's (8 sequences of 35 keyframes with about 1000 words each, one query per sequence and call) and one
sequence of 1024 keyframes whose vectors fill cap = 1024.  --dry builds the inputs and runs the referee only (no
device)."""
import argparse
import pathlib
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT / "sp-slam_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import place_cases as PC  # noqa: E402


def c3_case(n_seq=8, n_kf=35):
    seqs, frames, reloc, loop = [], [], [], []
    for s in range(n_seq):
        seq, pool, rng = PC.random_seq(n_kf, 300 + s, 950, 1000, pool_size=20000, window=1500)
        seq.in_db = [True] * (n_kf - 1) + [False]
        seqs.append(seq)
        frames.append(PC.query_near(seq, pool, rng, n_kf // 2, 1000))
        reloc.append((s, s))
        loop.append((s, n_kf - 1))
    return dict(seqs=seqs, frames=frames, cap=1024, fcap=1024,
                steps=[("reloc", reloc), ("min", loop, True), ("loop", loop, None)])


def large_case(n_kf=1024, cap=1024):
    seq, pool, rng = PC.random_seq(n_kf, 400, cap, cap, pool_size=60000, window=2000)
    seq.in_db = [True] * (n_kf - 1) + [False]
    frame = PC.query_near(seq, pool, rng, n_kf // 2, cap)
    return dict(seqs=[seq], frames=[frame], cap=cap, fcap=cap,
                steps=[("reloc", [(0, 0)]), ("min", [(0, n_kf - 1)], True), ("loop", [(0, n_kf - 1)], None)])


def median_ms(launch, reset, repeats, warm=5):
    import torch
    times = []
    for q in range(warm + repeats):
        reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        if q >= warm:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def time_case(ex, label, r, repeats, rows):
    import torch
    import spslam_match as M
    import spslam_place as P

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()

    packed = r["packed"]
    t, f = packed["t"], packed["f"]
    d = {name: dev(np.asarray(t[name], dt)) for name, dt in P.PLACE_DB_TABLES}
    d.update({"f_" + name: dev(np.asarray(f[name], dt)) for name, dt in P.PLACE_FRAME_TABLES})
    d.update({name: dev(t[name]) for name in ("covis", "weights", "ordered", "n_ordered", "kf_bad")})
    db = P.PlaceDb(cap=packed["cap"], **{name: d[name].data_ptr() for name, _ in P.PLACE_DB_TABLES})
    frames = P.PlaceFrames(cap=packed["fcap"], **{name: d["f_" + name].data_ptr() for name, _ in P.PLACE_FRAME_TABLES})
    graph = M.CovisGraph(stride=packed["stride"],
                         **{name: d[name].data_ptr() for name in ("covis", "weights", "ordered", "n_ordered")})
    pr = P.PlaceRecognition(ex)
    pristine = {k: d[k].clone() for k in ("reloc_score", "loop_score")}
    d_min = None
    for s in r["steps"]:
        n = len(s["problems"])
        d_problems = dev(s["problems"])
        d_results = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
        d_cands = torch.zeros(4 * s["n_out"], dtype=torch.uint8, device="cuda")
        if s["kind"] == "min":
            d_min = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
        d_min_here = d_min

        def reset():
            for k in pristine:
                d[k].copy_(pristine[k])

        def launch():
            if s["kind"] == "reloc":
                pr.reloc_candidates_batch_device(n, d_problems.data_ptr(), db, frames, graph, d_results.data_ptr(),
                                                 d_cands.data_ptr())
            elif s["kind"] == "min":
                pr.min_score_batch_device(n, d_problems.data_ptr(), db, graph, d["kf_bad"].data_ptr(),
                                          d_min_here.data_ptr())
            else:
                pr.loop_candidates_batch_device(n, d_problems.data_ptr(), db, graph, d_min_here.data_ptr(),
                                                d_results.data_ptr(), d_cands.data_ptr())
        timing = median_ms(launch, reset, repeats)
        torch.cuda.synchronize()
        # the last launch ran on the pristine scores, as the referee's step did
        if s["kind"] == "min":
            assert d_min.cpu().numpy().tobytes() == s["want_min"].tobytes(), f"{label}: min score differs"
        else:
            got = d_results.cpu().numpy().view(P.PLACE_RESULT_DTYPE)
            assert got.tobytes() == s["want"].tobytes(), f"{label}: {s['kind']} records differ from the referee"
            cand = d_cands.cpu().numpy().view(np.int32)
            for prob, want in zip(s["problems"], s["cands"]):
                o = int(prob["out_offset"])
                assert cand[o:o + len(want)].tolist() == want.tolist(), f"{label}: {s['kind']} candidates differ"
            table = "reloc_score" if s["kind"] == "reloc" else "loop_score"
            assert d[table].cpu().numpy().tobytes() == s[table].tobytes(), f"{label}: {table} differs"
        detail = "" if s["kind"] == "min" else \
            f" (scored {s['want']['n_scored'].tolist()}, candidates {s['want']['n_candidates'].tolist()})"
        rows.append((f"{label}: {s['kind']}{detail}", s["ref_ms"], timing))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    runs = [("C3 shape, 8 sequences x 35 keyframes x ~1000 words", PC.run(c3_case())),
            ("1024 keyframes x 1024 words, one sequence", PC.run(large_case()))]
    if a.dry:
        for label, r in runs:
            print(label, [(s["kind"], round(s["ref_ms"], 1)) for s in r["steps"]])
        return
    import spslam_gpu
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    rows = []
    for label, r in runs:
        time_case(ex, label, r, a.repeats, rows)
    ex.close()
    print("| call | device median ms (min .. max) | Python referee ms |")
    print("|---|---|---|")
    for name, ref, (med, lo, hi) in rows:
        print(f"| {name} | {med:.4f} ({lo:.4f} .. {hi:.4f}) | {ref:.1f} |")


if __name__ == "__main__":
    main()
