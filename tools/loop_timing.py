"""Times the four loop-closing entries (SearchByBoW KF-KF, SearchBySim3, SearchByProjection with Scw, the search of Fuse
with Scw) with HIP events: warm, one event pair per call, the median over the repeats; every timed configuration is
compared with the Python referee (tests/loop_match_ref.py) afterwards.
  python tools/loop_timing.py [--repeats 50] [--dry]
Shape: 8 sequences per call, each the pair of 1004-keypoint keyframes of tests/loop_match_cases.real_pair (frames 12
and 16 of synthetic sequence 0) in slots of its own, and for the projection and the fuse a loop-point list of about
4000: keyframe 1's 831 map points five times over, the copies moved by a centimetre or so.  --dry builds the inputs
and runs the referee only (no device)."""
import argparse
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT / "sp-slam_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

import loop_match_cases as C  # noqa: E402
import loop_match_ref as LR  # noqa: E402

N_SEQ = 8


def inputs():
    g, kfs, points, T12 = C.real_pair()
    rng = np.random.default_rng(77)
    P1 = points[kfs[0]["match_row"][kfs[0]["match_row"] >= 0]]
    loop = np.concatenate([P1] * 5)
    loop["xw"][len(P1):] += rng.normal(scale=0.01, size=(len(loop) - len(P1), 3)).astype(np.float32)
    m0, _ = LR.search_by_bow_kf(kfs[0]["desc"], kfs[0]["kun"]["angle"], kfs[0]["match_row"] >= 0, kfs[0]["fv"],
                                kfs[1]["desc"], kfs[1]["kun"]["angle"], kfs[1]["match_row"] >= 0, kfs[1]["fv"])
    m_in = np.where(rng.uniform(size=len(m0)) < 0.6, m0, -1).astype(np.int32)
    return g, kfs, points, T12, loop, m_in


def referee(g, kfs, points, T12, loop, m_in):
    out, ms = {}, {}
    k1, k2 = kfs

    def timed(name, fn):
        t = time.perf_counter()
        out[name] = fn()
        ms[name] = (time.perf_counter() - t) * 1e3

    timed("bow", lambda: C.bow_reference(dict(kf1=C.real_bow_keyframe(k1), kf2=C.real_bow_keyframe(k2), nn_ratio=0.75,
                                              check_ori=True)))
    timed("sim3", lambda: LR.search_by_sim3(k1, k2, points, None, 1.0, T12[:3, :3], T12[:3, 3], m_in, g, 7.5))
    timed("proj", lambda: LR.search_by_projection_sim3(k2["Tcw"], loop, k2["kun"], k2["desc"], k2["go"], k2["gi"], g, 10.0))
    timed("fuse", lambda: LR.fuse_sim3_snapshot(k2["Tcw"], loop, k2["kun"], k2["desc"], k2["go"], k2["gi"], g, 4.0))
    return out, ms


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


def device(g, kfs, points, T12, loop, m_in, want, repeats):
    import torch
    import spslam_frame
    import spslam_gpu
    import spslam_loop as L
    import synth
    import test_gpu_loop_match as T

    K = synth.TUM3
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], (0,) * 5, K["bf"], 640, 480)
    lm = L.LoopMatcher(ex)
    k1, k2 = kfs
    rows = []
    i32 = lambda t: t.cpu().numpy().view(np.int32)  # noqa: E731
    nothing = lambda: None  # noqa: E731

    # ---- SearchByBoW: 8 pairs (slot s of side 1, slot s of side 2)
    A, cap1, keep_a = T.bow_side([C.real_bow_keyframe(k1)] * N_SEQ)
    B, cap2, keep_b = T.bow_side([C.real_bow_keyframe(k2)] * N_SEQ)
    d_pairs = T.dev(np.array([(s, s) for s in range(N_SEQ)], np.int32))
    d_m = torch.zeros(N_SEQ * cap1 * 4, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(N_SEQ * 4, dtype=torch.uint8, device="cuda")
    t = median_ms(lambda: lm.search_by_bow_kf_batch_device(N_SEQ, d_pairs.data_ptr(), A, B, d_m.data_ptr(),
                                                           d_n.data_ptr()), nothing, repeats)
    m, n = i32(d_m).reshape(N_SEQ, cap1), i32(d_n)
    for s in range(N_SEQ):
        assert m[s, :len(want["bow"][0])].tobytes() == want["bow"][0].tobytes() and n[s] == want["bow"][1], "bow differs"
    rows.append((f"SearchByBoW KF-KF, 8 pairs of 1004 keypoints ({want['bow'][1]} matches each)", "bow", t))

    # ---- the keyframe slots of the three projection searches: sequence s has keyframes 2s (frame 12), 2s + 1 (frame 16)
    slots = T.Slots([k for _ in range(N_SEQ) for k in (k1, k2)])
    cap = slots.cap
    n_kf = 2 * N_SEQ
    Tcw = np.stack([k["Tcw"] for _ in range(N_SEQ) for k in (k1, k2)]).astype(np.float32)
    off = (np.arange(n_kf + 1) * cap).astype(np.int32)
    mrows = np.full((n_kf, cap), -1, np.int32)
    for k in range(n_kf):
        src = (k1, k2)[k % 2]["match_row"]
        mrows[k, :len(src)] = src
    rec = np.zeros(N_SEQ, L.SIM3_PAIR_DTYPE)
    n1 = len(k1["kun"])
    for s in range(N_SEQ):
        rec[s]["kf1"], rec[s]["kf2"], rec[s]["match_offset"], rec[s]["result_offset"] = 2 * s, 2 * s + 1, s * cap, s
        rec[s]["s12"], rec[s]["R12"], rec[s]["t12"] = 1.0, T12[:3, :3].astype(np.float32).reshape(9), T12[:3, 3]
    m12 = np.full((N_SEQ, cap), -1, np.int32)
    m12[:, :n1] = m_in
    keep = [T.dev(a) for a in (Tcw, np.arange(n_kf, dtype=np.int32), off, mrows, points, rec)]
    smap = L.Sim3Map(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), 0,
                     keep[4].data_ptr())
    d_m12_0 = T.dev(m12)
    d_m12 = d_m12_0.clone()
    d_nf = torch.zeros(N_SEQ * 4, dtype=torch.uint8, device="cuda")
    t = median_ms(lambda: lm.search_by_sim3_batch_device(N_SEQ, keep[5].data_ptr(), smap, *slots.ptrs(), cap, 0,
                                                         d_m12.data_ptr(), d_nf.data_ptr()),
                  lambda: d_m12.copy_(d_m12_0), repeats)
    m, nf = i32(d_m12).reshape(N_SEQ, cap), i32(d_nf)
    for s in range(N_SEQ):
        assert m[s, :n1].tobytes() == want["sim3"][0].tobytes() and nf[s] == want["sim3"][1], "sim3 differs"
    rows.append((f"SearchBySim3, 8 pairs of 1004 keypoints at the true Sim3 ({int((m_in >= 0).sum())} matches in, "
                 f"{want['sim3'][1]} found each)", "sim3", t))

    # ---- SearchByProjection(pKF, Scw) and Fuse(pKF, Scw): the loop-point list into frame 16 of every sequence
    problems = [dict(Scw=k2["Tcw"], P=loop, kf=2 * s + 1, th=0.0, skip=None, taken=None) for s in range(N_SEQ)]
    prec, ppts, skip, out_off, total = T.pack(problems)
    prec["point_offset"] = 0                                          # one list, shared by the 8 problems
    d_prec, d_pts = T.dev(prec), T.dev(loop)
    d_match = torch.zeros(N_SEQ * cap * 4, dtype=torch.uint8, device="cuda")
    d_nm = torch.zeros(N_SEQ * 4, dtype=torch.uint8, device="cuda")
    t = median_ms(lambda: lm.search_by_projection_sim3_batch_device(N_SEQ, d_prec.data_ptr(), d_pts.data_ptr(),
                                                                    len(loop), *slots.ptrs(), cap, 0, 0,
                                                                    d_match.data_ptr(), d_nm.data_ptr()), nothing,
                  repeats)
    m, nm = i32(d_match).reshape(N_SEQ, cap), i32(d_nm)
    for s in range(N_SEQ):
        assert m[s, :len(k2["kun"])].tobytes() == want["proj"][0].tobytes() and nm[s] == want["proj"][1], "proj differs"
    rows.append((f"SearchByProjection with Scw, 8 problems of {len(loop)} points into 1004 keypoints, th 10 "
                 f"({want['proj'][1]} matches each)", "proj", t))

    d_res = torch.zeros(total * 8, dtype=torch.uint8, device="cuda")
    d_nfu = torch.zeros(N_SEQ * 4, dtype=torch.uint8, device="cuda")
    t = median_ms(lambda: lm.fuse_sim3_search_batch_device(N_SEQ, d_prec.data_ptr(), d_pts.data_ptr(), len(loop),
                                                           *slots.ptrs(), cap, 0, d_res.data_ptr(), d_nfu.data_ptr()),
                  nothing, repeats)
    res, nfu = d_res.cpu().numpy().view(L.FUSE_RESULT_DTYPE), i32(d_nfu)
    for s, o in enumerate(out_off):
        assert res[o:o + len(loop)].tobytes() == want["fuse"][0].astype(res.dtype).tobytes(), "fuse differs"
        assert nfu[s] == want["fuse"][1]
    rows.append((f"Fuse with Scw, the search, 8 problems of {len(loop)} points, th 4 ({want['fuse'][1]} fused each)",
                 "fuse", t))
    ex.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    data = inputs()
    want, ref_ms = referee(*data)
    if a.dry:
        print({k: round(v, 1) for k, v in ref_ms.items()}, len(data[4]), "loop points")
        return
    rows = device(*data, want, a.repeats)
    print("| call | device median ms (min .. max) | Python referee ms, one problem |")
    print("|---|---|---|")
    for name, key, (med, lo, hi) in rows:
        print(f"| {name} | {med:.4f} ({lo:.4f} .. {hi:.4f}) | {ref_ms[key]:.0f} |")


if __name__ == "__main__":
    main()
