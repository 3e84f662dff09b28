"""Times the covisibility entries (UpdateConnections, KeyFrameCulling, MapPointCulling) with HIP events: warm, one
event pair per launch, the median over the repeats, beside the Python referee (tests/covis_ref.py) on the same inputs.
  python tools/covis_timing.py [--repeats 50] [--dry]
Shapes: C3's (25 local + 10 fixed keyframes, 4000 points, 1000 keypoints per keyframe, 8 sequences per call) and one
worst-shaped UpdateConnections (1024 keyframes, all connected, every weight changed, so that every neighbour's
1023-entry list is re-sorted).  --dry builds the inputs and runs the referee only (no device)."""
import argparse
import copy
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT / "sp-slam_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import covis_cases as CC  # noqa: E402
import covis_ref as CR  # noqa: E402
import spslam_match as M  # noqa: E402

N_SEQ, N_KF, N_POINTS, N_KP = 8, 35, 4000, 1000


def c3_map(seed):
    """35 keyframes of 1000 keypoints over 4000 points: a point is seen from a window of consecutive keyframes
    (35000 observations, 8.75 per point), at levels 0 .. 3, stereo, depth inside the threshold."""
    rng = np.random.default_rng(seed)
    m = CR.Map(N_KF)
    per_point = N_KF * N_KP // N_POINTS
    for _ in range(N_POINTS):
        w = int(rng.integers(per_point - 2, per_point + 3))
        lo = int(rng.integers(0, N_KF - w + 1))
        ks = [k for k in range(lo, lo + w) if len(m.matches[k]) < N_KP]
        m.add_point({k: dict(octave=int(rng.integers(0, 4)), stereo=True, depth=1.0) for k in ks})
    for k in range(N_KF):
        while len(m.matches[k]) < N_KP:
            m.add_keypoint(k)
    return m


def without_keyframe(m, kf):
    """The map before `kf` was inserted: none of its observations."""
    m = copy.deepcopy(m)
    for i, row in enumerate(m.matches[kf]):
        if row is not None:
            del m.obs[row][kf]
            m.matches[kf][i] = None
    return m


def connected_1024():
    """16 points that all 1024 keyframes see, on a graph that holds weight 15 everywhere: UpdateConnections of
    keyframe 5 changes every neighbour's weight."""
    n = 1024
    m = CR.Map(n)
    for _ in range(16):
        m.add_point(range(n))
    arrays = CC.fresh_graph([n], n)
    g = CR.Graph(n)
    idx = np.arange(n)
    for k in range(n):
        others = idx[idx != k][::-1]
        arrays["weights"][k] = 15
        arrays["weights"][k, k] = 0
        arrays["ordered"][k, :n - 1] = others
        arrays["ordered_w"][k, :n - 1] = 15
        arrays["n_ordered"][k] = n - 1
        arrays["covis"][k] = others[:10]
        g.weights[k] = {int(j): 15 for j in others[::-1]}
        g.ordered[k], g.ordered_w[k] = others.tolist(), [15] * (n - 1)
    arrays["first_connection"][:] = 0
    g.first_connection = [False] * n
    return m, arrays, g


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    rows = []

    # ---- C3 shape: the graph as UpdateConnections of keyframes 0 .. 33 left it before the last keyframe was
    # inserted, then the last keyframe's call (every neighbour gains a weight and is re-sorted)
    maps = [c3_map(100 + s) for s in range(N_SEQ)]
    packed = CC.pack(maps, N_KP)
    stride = N_KF
    arrays = CC.fresh_graph([N_KF] * N_SEQ, stride)
    graphs = [CR.Graph(N_KF) for _ in maps]
    for s in range(N_SEQ):
        earlier = without_keyframe(maps[s], N_KF - 1)
        for kf in range(N_KF - 1):
            res, rewritten = CR.update_connections(earlier, graphs[s], kf)
            CC.mirror(arrays, packed["kf_base"][s], N_KF, graphs[s], kf, rewritten)
    before = copy.deepcopy(arrays)
    kf = N_KF - 1
    t0 = time.perf_counter()
    want = []
    for s in range(N_SEQ):
        res, rewritten = CR.update_connections(maps[s], graphs[s], kf)
        want.append(res)
        CC.mirror(arrays, packed["kf_base"][s], N_KF, graphs[s], kf, rewritten)
    ref_update_ms = (time.perf_counter() - t0) * 1e3
    problems = np.zeros(N_SEQ, M.COVIS_PROBLEM_DTYPE)
    cull_problems = np.zeros(N_SEQ, M.CULL_PROBLEM_DTYPE)
    for s in range(N_SEQ):
        problems[s] = (packed["kf_base"][s], packed["row_base"][s], kf, N_KF)
        for key, v in zip(("kf_base", "row_base", "kf", "n_kf", "out_offset"),
                          (packed["kf_base"][s], packed["row_base"][s], kf, N_KF, s * N_KF)):
            cull_problems[key][s] = v
    cull_maps = copy.deepcopy(maps)
    t0 = time.perf_counter()
    cull_want = [CR.keyframe_culling(cull_maps[s], kf, graphs[s].ordered[kf], CC.TH_DEPTH) for s in range(N_SEQ)]
    ref_cull_ms = (time.perf_counter() - t0) * 1e3
    n_cand = sum(len(r) for r, _ in cull_want)
    n_culled = sum(sum(x[3] == CR.CULLED for x in r) for r, _ in cull_want)
    rng = np.random.default_rng(7)
    n_rows = len(packed["t"]["point_bad"])
    pt = dict(found=rng.integers(0, 40, n_rows).astype(np.int32), visible=rng.integers(1, 60, n_rows).astype(np.int32),
              first_kf=rng.integers(28, 35, n_rows).astype(np.int32), point_bad=packed["t"]["point_bad"],
              points=packed["t"]["points"])
    rows_list = np.arange(n_rows, dtype=np.int32)
    ids = np.full(n_rows, kf, np.int32)
    t0 = time.perf_counter()
    point_want = CR.map_point_culling(pt["found"], pt["visible"], pt["first_kf"], pt["point_bad"],
                                      pt["points"]["n_obs"], rows_list, kf)
    ref_point_ms = (time.perf_counter() - t0) * 1e3

    # ---- worst shape
    wm, warrays, wg = connected_1024()
    wpacked = CC.pack([wm])
    wbefore = copy.deepcopy(warrays)
    t0 = time.perf_counter()
    wres, wrewritten = CR.update_connections(wm, wg, 5)
    ref_worst_ms = (time.perf_counter() - t0) * 1e3
    CC.mirror(warrays, 0, 1024, wg, 5, wrewritten)
    print(f"inputs: C3 update results {want[0]} .., culling {n_cand} candidates, {n_culled} culled; worst {wres}")
    if a.dry:
        print(f"referee ms: update {ref_update_ms:.2f} culling {ref_cull_ms:.2f} points {ref_point_ms:.2f} "
              f"worst {ref_worst_ms:.1f}")
        return

    import torch
    import spslam_gpu
    ex =spslam_gpu.OrbExtractor(max_batch=1)

    def dev(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()

    def dev_map(t):
        d = {name: dev(np.asarray(t[name], dt)) for name, dt in M.COVIS_MAP_TABLES}
        return d, M.CovisMap(**{name: d[name].data_ptr() for name in d})

    def dev_graph(arr, st):
        d = {name: dev(arr[name]) for name, _ in M.COVIS_GRAPH_TABLES}
        return d, M.CovisGraph(stride=st, **{name: d[name].data_ptr() for name in d})

    def same(d_graph, arr):
        return all(d_graph[name].cpu().numpy().tobytes() == np.ascontiguousarray(arr[name]).tobytes()
                   for name, _ in M.COVIS_GRAPH_TABLES)

    uc = M.CovisUpdateConnections(ex)
    d_map, cm = dev_map(packed["t"])
    d_graph, G = dev_graph(before, stride)
    pristine = {k: v.clone() for k, v in d_graph.items()}
    d_problems, d_results = dev(problems), torch.zeros(16 * N_SEQ, dtype=torch.uint8, device="cuda")

    def reset():
        for k in d_graph:
            d_graph[k].copy_(pristine[k])

    def launch():
        uc.batch_device(N_SEQ, d_problems.data_ptr(), cm, G, d_results.data_ptr())
    rows.append(("UpdateConnections, C3 shape, 8 sequences, graph before the call", ref_update_ms,
                 median_ms(launch, reset, a.repeats)))
    assert same(d_graph, arrays), "UpdateConnections differs from the referee"
    rows.append(("UpdateConnections, C3 shape, repeated on its own result (no weight changes)", None,
                 median_ms(launch, lambda: None, a.repeats)))
    assert same(d_graph, arrays)

    kc = M.KeyFrameCulling(ex, CC.TH_DEPTH)
    frames = [dev(packed[k]) for k in ("keys_un", "uright", "depth", "new_plane", "not_erase")]
    d_cull, d_rec = dev(cull_problems), torch.zeros(16 * N_SEQ * N_KF, dtype=torch.uint8, device="cuda")
    d_sum = torch.zeros(8 * N_SEQ, dtype=torch.uint8, device="cuda")

    def launch_cull():
        kc.batch_device(N_SEQ, d_cull.data_ptr(), cm, G, frames[0].data_ptr(), frames[1].data_ptr(),
                        frames[2].data_ptr(), N_KP, frames[3].data_ptr(), frames[4].data_ptr(), d_rec.data_ptr(),
                        d_sum.data_ptr())
    rows.append((f"KeyFrameCulling, C3 shape, 8 sequences ({n_cand} candidates, {n_culled} culled)", ref_cull_ms,
                 median_ms(launch_cull, lambda: None, a.repeats)))
    rec = d_rec.cpu().numpy().view(M.CULL_RECORD_DTYPE).reshape(N_SEQ, N_KF)
    for s, (r, _) in enumerate(cull_want):
        assert rec[s, :len(r)].tolist() == [tuple(x) for x in r], "KeyFrameCulling differs from the referee"

    mc = M.MapPointCulling(ex)
    d_pt = {name: dev(np.asarray(pt[name], dt)) for name, dt in M.POINT_CULL_TABLES}
    pm = M.PointCullMap(**{name: d_pt[name].data_ptr() for name in d_pt})
    d_rows, d_ids, d_v = dev(rows_list), dev(ids), torch.zeros(n_rows, dtype=torch.uint8, device="cuda")

    def launch_points():
        mc.batch_device(pm, d_rows.data_ptr(), d_ids.data_ptr(), n_rows, d_v.data_ptr())
    rows.append((f"MapPointCulling, {n_rows} list entries (8 x 4000)", ref_point_ms,
                 median_ms(launch_points, lambda: None, a.repeats)))
    assert d_v.cpu().numpy().tolist() == point_want.tolist(), "MapPointCulling differs from the referee"

    d_wmap, wcm = dev_map(wpacked["t"])
    d_wgraph, WG = dev_graph(wbefore, 1024)
    wpristine = {k: v.clone() for k, v in d_wgraph.items()}
    d_wp = dev(np.array([(0, 0, 5, 1024)], M.COVIS_PROBLEM_DTYPE))

    def wreset():
        for k in d_wgraph:
            d_wgraph[k].copy_(wpristine[k])

    def wlaunch():
        uc.batch_device(1, d_wp.data_ptr(), wcm, WG, d_results.data_ptr())
    rows.append(("UpdateConnections, 1024 keyframes all connected, 1023 lists of 1023 re-sorted, one sequence",
                 ref_worst_ms, median_ms(wlaunch, wreset, max(a.repeats // 5, 5), warm=2)))
    assert same(d_wgraph, warrays), "the worst-shaped UpdateConnections differs from the referee"
    ex.close()

    print("| call | device median ms (min .. max) | Python referee ms |")
    print("|---|---|---|")
    for name, ref, (med, lo, hi) in rows:
        print(f"| {name} | {med:.4f} ({lo:.4f} .. {hi:.4f}) | {'-' if ref is None else f'{ref:.1f}'} |")


if __name__ == "__main__":
    main()
