"""First timings of the CreateNewMapPoints entries at C3's shape: keyframes of 1000 features, the ORBvoc-shaped
vocabulary (k = 10, L = 6), 10 neighbour rounds per keyframe, `--seqs` sequences in flight (one pair per sequence
and round).  HIP events around `--iters` repetitions of the 10 chained rounds after `--warmup`; the has-point masks
are restored between repetitions by a device copy (timed separately and subtracted).  Next to them
spslam_search_by_bow_batch_device (bow_search_kernel) on the same keyframe pairs.

  python tools/create_points_bench.py [--seqs 64] [--rounds 10] [--iters 20] [--warmup 3] [--out f.json]

Keyframes: frame 0 of two synthetic scenes and a distinct neighbour frame per round (20, 22, ...) through the CPU ORB
and frame oracles (reused across the sequences: the times depend on the shapes), FeatureVectors from the device transform, a share of
`--held` of the keypoints already holding a map point.  A measurement variant of the lane-group size is built with
`make variant VARIANT=g4 VAR_FLAGS=-DSPSLAM_TRI_GROUP=4` and loaded through SPSLAM_GPU_LIB.
"""
import argparse
import json
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in ("sp-slam_amd", "oracle", "tests"):
    sys.path.insert(0, str(ROOT / p))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def keyframes(vocab, n_scenes, frames, held, rng):
    import oracle_ctypes
    import oracle_frame
    import synth
    import triangulation_ref as TR
    K = synth.TUM3
    orb = oracle_ctypes.OrbOracle(nfeatures=1000)
    out = []
    for seq in range(n_scenes):
        sc = synth.Scene(seq, n_boxes=3)
        row = []
        for f in frames:
            Twc = sc.pose(f)
            g, d16, _ = sc.render(Twc, noise_seed=f)
            kp, desc = orb.extract(g)
            depth = d16.astype(np.float32) * np.float32(np.float32(1.0) / np.float32(5000.0))
            fo = oracle_frame.frame_rgbd(np.stack([kp["x"], kp["y"]], 1), depth, K["fx"], K["fy"], K["cx"], K["cy"],
                                         bf=K["bf"])
            kun = kp.copy()
            kun["x"], kun["y"] = fo["un"][:, 0], fo["un"][:, 1]
            Tcw = np.linalg.inv(Twc).astype(np.float32)
            fv = vocab.transform(desc)
            row.append(dict(keys=kp, kun=kun, ur=fo["uright"], depth=fo["depth"], desc=desc,
                            has=(rng.uniform(size=len(kp)) < held).astype(np.uint8), fv=fv, Tcw=Tcw,
                            Ow=TR.camera_centre(Tcw)))
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--held", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import spslam_bow as SB
    import spslam_frame
    import spslam_gpu as G
    import spslam_match as M
    import synth
    import triangulation_ref as TR
    K = synth.TUM3
    ex = G.OrbExtractor(max_batch=1)
    spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], (0,) * 5, K["bf"], 640, 480)
    vocab = SB.Vocabulary(ex, synth.shape_vocabulary_text())
    rng = np.random.default_rng(1)
    # per scene the keyframe (frame 0) and a distinct neighbour frame for every round (frames 20, 22, ...)
    real = keyframes(vocab, 2, [0] + [20 + 2 * r for r in range(a.rounds)], a.held, rng)
    S, R = a.seqs, a.rounds
    kfs, Kmat = [], np.array([[K["fx"], 0, K["cx"]], [0, K["fy"], K["cy"]], [0, 0, 1]], np.float32)
    for s in range(S):                                              # slot s*(R+1): the keyframe, then R neighbours
        row = real[s % len(real)]
        kfs += [row[0]] + [row[1 + r] for r in range(R)]
    cap = max(len(k["kun"]) for k in kfs)
    n_slots = len(kfs)
    keys, kun = np.zeros((n_slots, cap), G.KEYPOINT_DTYPE), np.zeros((n_slots, cap), G.KEYPOINT_DTYPE)
    ur, depth = np.zeros((n_slots, cap), np.float32), np.zeros((n_slots, cap), np.float32)
    desc, has = np.zeros((n_slots, cap, 32), np.uint8), np.zeros((n_slots, cap), np.uint8)
    counts, n_fv = np.zeros(n_slots, np.int32), np.zeros(n_slots, np.int32)
    nodes, start = np.zeros((n_slots, cap), np.uint32), np.zeros((n_slots, cap + 1), np.int32)
    feats = np.zeros((n_slots, cap), np.int32)
    for q, k in enumerate(kfs):
        n, fv = len(k["kun"]), k["fv"]
        keys[q, :n], kun[q, :n], ur[q, :n], depth[q, :n] = k["keys"], k["kun"], k["ur"], k["depth"]
        desc[q, :n], has[q, :n], counts[q], n_fv[q] = k["desc"], k["has"], n, len(fv["nodes"])
        nodes[q, :len(fv["nodes"])], start[q, :len(fv["start"])] = fv["nodes"], fv["start"]
        feats[q, :len(fv["features"])] = fv["features"]
    d = [dev(x) for x in (keys, kun, ur, depth, desc, has, counts, nodes, start, feats, n_fv)]
    d_has0 = d[5].clone()
    side = M.TriSide(*[t.data_ptr() for t in d], cap, 0)
    f12 = {}
    d_pairs, d_bow_pairs = [], []
    for r in range(R):
        rec = np.zeros(S, M.TRI_PAIR_DTYPE)
        for s in range(S):
            q1, q2 = s * (R + 1), s * (R + 1) + 1 + r
            k1, k2 = kfs[q1], kfs[q2]
            key = (s % len(real), r)
            if key not in f12:
                f12[key] = TR.compute_f12(k1, k2, Kmat)
            rec[s]["kf1"], rec[s]["kf2"] = q1, q2
            rec[s]["Tcw1"], rec[s]["Tcw2"] = k1["Tcw"][:3].reshape(12), k2["Tcw"][:3].reshape(12)
            rec[s]["Ow1"], rec[s]["Ow2"], rec[s]["F12"], rec[s]["out_offset"] = k1["Ow"], k2["Ow"], f12[key], s * cap
        d_pairs.append(dev(rec))
        d_bow_pairs.append(dev(np.stack([rec["kf1"], rec["kf2"]], 1).astype(np.int32)))
    d_m = torch.zeros(S * cap, dtype=torch.int32, device="cuda")
    d_res = torch.zeros(S * cap * 20, dtype=torch.uint8, device="cuda")
    d_n, d_new = torch.zeros(S, dtype=torch.int32, device="cuda"), torch.zeros(S, dtype=torch.int32, device="cuda")
    d_st = torch.zeros(S, dtype=torch.uint8, device="cuda")
    create, search, tri = M.CreateNewPoints(ex), M.SearchForTriangulation(ex), M.Triangulate(ex)

    def restore():
        d[5].copy_(d_has0)

    def all_rounds():
        restore()
        for r in range(R):
            create.batch_device(S, d_pairs[r].data_ptr(), side, d_m.data_ptr(), d_n.data_ptr(), d_res.data_ptr(),
                                d_new.data_ptr(), d_st.data_ptr())

    def search_only():
        for r in range(R):
            search.batch_device(S, d_pairs[r].data_ptr(), side, 0, 0, d_m.data_ptr(), d_n.data_ptr())

    def tri_only():                                                 # on the last search's matches, nothing marked
        for r in range(R):
            tri.batch_device(S, d_pairs[R - 1].data_ptr(), side, d_m.data_ptr(), 0, d_res.data_ptr(),
                             d_new.data_ptr())

    bow_side = SB.BowSide(d[4].data_ptr(), d[1].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(),
                          d[8].data_ptr(), d[9].data_ptr(), d[10].data_ptr(), cap, 0)

    def bow_only():
        for r in range(R):
            SB.search_by_bow_batch_device(ex, S, d_bow_pairs[r].data_ptr(), bow_side, bow_side, d_m.data_ptr(),
                                          d_n.data_ptr(), nn_ratio=0.6, check_orientation=False)

    t_restore = timed(restore, a.iters, a.warmup)
    t_all = timed(all_rounds, a.iters, a.warmup) - t_restore
    restore()                                                       # untimed: what each round finds
    matched, created = [], []
    for r in range(R):
        create.batch_device(S, d_pairs[r].data_ptr(), side, d_m.data_ptr(), d_n.data_ptr(), d_res.data_ptr(),
                            d_new.data_ptr(), d_st.data_ptr())
        torch.cuda.synchronize()
        matched.append(int(d_n.sum()) / S)
        created.append(int(d_new.sum()) / S)
    restore()
    t_search = timed(search_only, a.iters, a.warmup)                # every round on the unmarked masks
    t_tri = timed(tri_only, a.iters, a.warmup)
    t_bow = timed(bow_only, a.iters, a.warmup)
    out = {"lib": os.path.basename(os.environ.get("SPSLAM_GPU_LIB", "libspslam_gpu.so")), "seqs": S, "rounds": R, "cap": cap,
           "features": int(counts.mean()), "fv_nodes": int(n_fv.mean()), "held": a.held,
           "create_new_points_ms_per_round": t_all / R, "search_for_triangulation_ms_per_round": t_search / R,
           "triangulate_ms_per_round": t_tri / R, "search_by_bow_ms_per_round": t_bow / R,
           "matches_per_pair_by_round": matched, "new_points_per_pair_by_round": created,
           "restore_ms": t_restore}
    print(json.dumps(out))
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    ex.close()


if __name__ == "__main__":
    main()
