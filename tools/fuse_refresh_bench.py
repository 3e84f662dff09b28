"""Times of the Fuse search and the map-point refresh at C3's shape (64 sequences in flight, keyframes of about
1000 points, 10 target keyframes per SearchInNeighbors, point tables of 4000 rows), next to their nearest
relatives: spslam_search_local_points_batch_device on the same points and keyframes, and the host
SeqMap.update_normals_and_depths on the same points.  HIP events around `--iters` launches after `--warmup`.

  python tools/fuse_refresh_bench.py [--seqs 64] [--targets 10] [--rows 4000] [--iters 20] [--warmup 3] [--out f.json]

Per-kernel times (the local search is two kernels): run it under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import pathlib
import sys
import time

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


def fuse_part(ex, a):
    import fuse_cases as FC
    import spslam_gpu as G
    import spslam_match as M
    import torch
    real = FC.real_problems()
    S, T = a.seqs, a.targets
    F = S * T
    cap = max(len(q["kun"]) for q in real)
    kun, desc = np.zeros((F, cap), G.KEYPOINT_DTYPE), np.zeros((F, cap, 32), np.uint8)
    ur, go = np.zeros((F, cap), np.float32), np.zeros((F, 64 * 48 + 1), np.int32)
    gi, counts = np.zeros((F, cap), np.int32), np.zeros(F, np.int32)
    prob, lfr = np.zeros(F, M.FUSE_PROBLEM_DTYPE), np.zeros(F, M.LOCAL_FRAME_DTYPE)
    pts, off = [], 0
    for s in range(S):
        q = real[s % len(real)]
        n = len(q["kun"])
        for t in range(T):
            f = s * T + t
            kun[f, :n], desc[f, :n], ur[f, :n], go[f], counts[f] = q["kun"], q["desc"], q["ur"], q["go"], n
            gi[f, :len(q["gi"])] = q["gi"]
            prob[f]["Tcw"], prob[f]["kf_slot"], prob[f]["point_offset"] = q["lfr"]["Tcw"], f, off
            prob[f]["n_points"], prob[f]["out_offset"] = len(q["LP"]), f * 2048
            lfr[f]["Tcw"], lfr[f]["point_offset"], lfr[f]["n_points"] = q["lfr"]["Tcw"], off, len(q["LP"])
        pts.append(q["LP"])
        off += len(q["LP"])
    max_points = max(len(p) for p in pts)
    assert max_points <= 2048
    d = [dev(x) for x in (prob, np.concatenate(pts), kun, desc, ur, go, gi, counts, lfr)]
    d_res = torch.zeros(F * 2048 * 8, dtype=torch.uint8, device="cuda")
    d_nf = torch.zeros(F, dtype=torch.int32, device="cuda")
    d_match = torch.zeros(F * cap, dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(F, dtype=torch.int32, device="cuda")
    fs, lm = M.FuseSearch(ex), M.LocalMatcher(ex)
    p = [t.data_ptr() for t in d]

    def fuse():
        fs.batch_device(F, p[0], p[1], max_points, p[2], p[3], p[4], p[5], p[6], p[7], cap, 0, d_res.data_ptr(),
                        d_nf.data_ptr())

    def local():
        lm.batch_device(F, p[8], p[1], max_points, p[2], p[3], p[4], p[5], p[6], p[7], cap, 0, d_match.data_ptr(),
                        d_nm.data_ptr())

    out = dict(problems=F, points_per_problem=[len(x) for x in pts[:2]], keypoints=[int(c) for c in counts[:2]])
    out["fuse_search_ms"] = [timed(fuse, a.iters, a.warmup) for _ in range(3)]
    out["search_local_points_ms"] = [timed(local, a.iters, a.warmup) for _ in range(3)]
    out["fuse_search_ms"] += [timed(fuse, a.iters, a.warmup)]      # once more after the other: the spread
    out["nfused_first_problems"] = d_nf.cpu().numpy()[:4].tolist()
    out["local_matches_first_problems"] = d_nm.cpu().numpy()[:4].tolist()
    return out


def refresh_part(ex, a):
    import local_mapping
    import spslam_assoc
    import spslam_gpu as G
    import spslam_match as M
    import torch
    rng = np.random.default_rng(1)
    S, R, nk, cap = a.seqs, a.rows, 16, 1000
    scale = ex.tables()["scale"].astype(np.float32)
    # one sequence's map, then the same map S times with absolute indices
    cnt = rng.integers(2, 11, R)
    Tcw = np.zeros((nk, 4, 4), np.float32)
    for k in range(nk):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        Tcw[k, :3, :3], Tcw[k, :3, 3], Tcw[k, 3, 3] = q, rng.normal(size=3) * 2, 1
    octave = rng.integers(0, 8, (nk, cap)).astype(np.int32)
    obs_kf = [np.sort(rng.choice(nk, c, replace=False)) for c in cnt]
    obs_kp = [rng.integers(0, cap, c) for c in cnt]
    ref = np.array([k[0] for k in obs_kf], np.int32)
    table = np.zeros(R, M.LOCAL_POINT_DTYPE)
    table["xw"], table["id"] = rng.normal(size=(R, 3)) * 3, np.arange(R)
    sm = local_mapping.SeqMap([table], cap, (1, 1, 0, 0, 40), scale, np.ones(8, np.float32),
                              np.zeros(0, spslam_assoc.MAP_PLANE_DTYPE))
    for k in range(nk):
        sm.kfs[k] = dict(Tcw=Tcw[k], octave=octave[k])
    for r in range(R):
        sm.obs[r] = dict(zip(obs_kf[r].tolist(), obs_kp[r].tolist()))
        sm.ref[r] = int(ref[r])
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        sm.update_normals_and_depths(list(range(R)), np.arange(R))
        host.append((time.perf_counter() - t0) * 1e3)
    keys = np.zeros((S * nk, cap), G.KEYPOINT_DTYPE)
    keys["octave"] = np.tile(octave, (S, 1))
    desc = rng.integers(0, 256, (S * nk, cap, 32), dtype=np.uint8)
    okf, okp = np.concatenate(obs_kf), np.concatenate(obs_kp)
    off1 = np.concatenate([[0], np.cumsum(cnt)])
    t = dict(kf_Tcw=np.tile(Tcw.reshape(nk, 16), (S, 1)), kf_slot=np.arange(S * nk),
             kf_bad=np.zeros(S * nk), obs_off=np.concatenate([off1[:-1] + s * off1[-1] for s in range(S)] +
                                                              [[S * off1[-1]]]),
             obs_kf=np.concatenate([okf + s * nk for s in range(S)]), obs_kp=np.tile(okp, S),
             ref_kf=np.concatenate([ref + s * nk for s in range(S)]), point_bad=np.zeros(S * R))
    d = {name: dev(np.asarray(t[name], dt)) for name, dt in M.REFRESH_MAP_TABLES}
    d_points = dev(np.tile(table, S))
    d_rows, d_keys, d_desc = dev(np.arange(S * R, dtype=np.int32)), dev(keys), dev(desc)
    d_status = torch.zeros(S * R, dtype=torch.uint8, device="cuda")
    m = M.PointRefreshMap(points=d_points.data_ptr(), **{n: d[n].data_ptr() for n, _ in M.REFRESH_MAP_TABLES})
    pr = M.PointRefresh(ex)

    def run(what):
        return lambda: pr.batch_device(m, d_rows.data_ptr(), S * R, what, d_keys.data_ptr(), d_desc.data_ptr(), cap,
                                       d_status.data_ptr())

    out = dict(rows=S * R, observers_mean=float(cnt.mean()))
    out["refresh_both_ms"] = [timed(run(3), a.iters, a.warmup) for _ in range(3)]
    out["refresh_normal_depth_ms"] = [timed(run(2), a.iters, a.warmup) for _ in range(3)]
    out["refresh_descriptor_ms"] = [timed(run(1), a.iters, a.warmup) for _ in range(3)]
    out["host_update_normals_and_depths_ms_one_sequence"] = host
    got = d_points.cpu().numpy().view(M.LOCAL_POINT_DTYPE)[:R]
    out["normal_depth_equal_to_host"] = bool(all(got[f].tobytes() == sm.table[f].tobytes()
                                                 for f in ("normal", "min_dist", "max_dist")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--targets", type=int, default=10)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import spslam_frame
    import spslam_gpu
    import synth
    K = synth.TUM3
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    try:
        spslam_frame.FrameStage(ex, K["fx"], K["fy"], K["cx"], K["cy"], (0,) * 5, K["bf"], 640, 480)
        res = dict(shape=vars(a), fuse=fuse_part(ex, a), refresh=refresh_part(ex, a))
    finally:
        ex.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
