"""GPU parity of the covisibility entries on gfx950 -- spslam_covis_update_connections, spslam_keyframe_culling and
spslam_map_point_culling, device and host forms -- against the mutable-state referees of tests/covis_ref.py on the
cases of tests/covis_cases.py (tests/test_covis_host.py guards what each case reaches).  Bar: every output byte and
every graph byte equal; the buffers are pre-filled with a sentinel, so bytes that must not be written are seen to be
kept."""
import numpy as np
import pytest

import covis_cases as CC
import covis_ref as CR

pytestmark = pytest.mark.gpu

SENT = CC.SENT


@pytest.fixture(scope="module")
def gpu():
    import spslam_gpu
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    yield ex
    ex.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def sentinel(n_bytes):
    import torch
    return torch.full((n_bytes,), SENT, dtype=torch.uint8, device="cuda")


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def device_map(tables):
    import spslam_match as M
    d = {name: dev(np.asarray(tables[name], dt)) for name, dt in M.COVIS_MAP_TABLES}
    return d, M.CovisMap(**{name: d[name].data_ptr() if d[name].numel() else None for name in d})


def device_graph(arrays, stride):
    import spslam_match as M
    d = {name: dev(arrays[name]) for name, _ in M.COVIS_GRAPH_TABLES}
    return d, M.CovisGraph(stride=stride, **{name: d[name].data_ptr() for name in d})


def graph_mismatch(d_graph, want):
    import spslam_match as M
    return [name for name, dt in M.COVIS_GRAPH_TABLES
            if host(d_graph[name], dt).tobytes() != np.ascontiguousarray(want[name]).tobytes()]


# ---------------------------------------------------------------- UpdateConnections
@pytest.mark.parametrize("name", list(CC.UPDATE_CASES))
def test_update_connections_device(gpu, name):
    """The case's calls in order on one stream and one persistent graph.  sync: results and graph compared after
    every call; otherwise the calls are launched back to back and compared at the end."""
    import spslam_match as M
    import torch
    r = CC.replay_update(name)
    uc = M.CovisUpdateConnections(gpu)
    d_graph, G = device_graph(r["graph0"], r["stride"])
    d_problems = [dev(s["problems"]) for s in r["steps"]]
    d_results = [sentinel(16 * (len(s["problems"]) + 1)) for s in r["steps"]]
    keep = []
    for q, s in enumerate(r["steps"]):
        if s["packed"] is not None:
            d_map, cm = device_map(s["packed"]["t"])
            keep.append(d_map)
        uc.batch_device(len(s["problems"]), d_problems[q].data_ptr(), cm, G, d_results[q].data_ptr())
        if r["sync"]:
            torch.cuda.synchronize()
            assert graph_mismatch(d_graph, s["graph"]) == [], (name, q)
    torch.cuda.synchronize()
    for q, s in enumerate(r["steps"]):
        got = host(d_results[q], M.COVIS_RESULT_DTYPE)
        assert got[:-1].tolist() == s["want"].tolist(), (name, q)
        assert got[-1:].tobytes() == bytes([SENT]) * 16
    assert graph_mismatch(d_graph, r["steps"][-1]["graph"]) == []


@pytest.mark.parametrize("name", [n for n in CC.UPDATE_CASES if n not in ("two_sequences", "n_kf_1024")])
def test_update_connections_host_form(gpu, name):
    import spslam_match as M
    r = CC.replay_update(name)
    uc = M.CovisUpdateConnections(gpu)
    graph = r["graph0"]
    for s in r["steps"]:
        packed = s["packed"] or packed
        graph, res = uc(packed["t"], graph, r["stride"], int(s["problems"]["kf"][0]))
        assert res.tolist() == s["want"][0].tolist()
        assert [k for k in graph if graph[k].tobytes() != s["graph"][k].tobytes()] == []


# ---------------------------------------------------------------- KeyFrameCulling
def culling_graph(r):
    """The graph as the culling reads it: each current keyframe's candidate list in its row."""
    n_total = sum(r["packed"]["n_kf"])
    stride = max(len(order) for _, order in r["ordered"]) + 2
    arrays = CC.fresh_graph([n_total], stride)
    for (cur, order), b in zip(r["ordered"], r["packed"]["kf_base"]):
        arrays["ordered"][b + cur, :len(order)] = order
        arrays["n_ordered"][b + cur] = len(order)
    return arrays, stride


def run_culling_device(gpu, r, not_erase=True):
    import spslam_match as M
    import torch
    p = r["packed"]
    kc = M.KeyFrameCulling(gpu, CC.TH_DEPTH)
    d_map, cm = device_map(p["t"])
    arrays, stride = culling_graph(r)
    d_graph, G = device_graph(arrays, stride)
    frames = [dev(p[k]) for k in ("keys_un", "uright", "depth", "new_plane", "not_erase")]
    d_problems = dev(r["problems"])
    d_records, d_summaries = sentinel(16 * r["n_out"]), sentinel(8 * (len(r["problems"]) + 1))
    before = {k: v.clone() for k, v in {**d_map, **d_graph}.items()}
    kc.batch_device(len(r["problems"]), d_problems.data_ptr(), cm, G, frames[0].data_ptr(), frames[1].data_ptr(),
                    frames[2].data_ptr(), p["cap"], frames[3].data_ptr(), frames[4].data_ptr() if not_erase else 0,
                    d_records.data_ptr(), d_summaries.data_ptr())
    torch.cuda.synchronize()
    for k, v in before.items():                           # nothing of the map or the graph is written
        assert torch.equal(v, {**d_map, **d_graph}[k]), k
    return host(d_records, M.CULL_RECORD_DTYPE), host(d_summaries, M.CULL_SUMMARY_DTYPE)


def check_culling(r, records, summaries, want_records, want_summaries):
    import spslam_match as M
    assert summaries[:-1].tolist() == want_summaries.tolist()
    assert summaries[-1:].tobytes() == bytes([SENT]) * 8
    written = np.zeros(len(records), bool)
    for prob, want in zip(r["problems"], want_records):
        o = int(prob["out_offset"])
        assert records[o:o + len(want)].tolist() == want.tolist(), int(prob["kf"])
        written[o:o + len(want)] = True
    assert records[~written].tobytes() == bytes([SENT]) * (16 * int((~written).sum()))


@pytest.mark.parametrize("name", list(CC.CULL_CASES))
def test_keyframe_culling_device(gpu, name):
    r = CC.replay_culling(name)
    records, summaries = run_culling_device(gpu, r)
    check_culling(r, records, summaries, r["want_records"], r["want_summaries"])


def test_keyframe_culling_without_not_erase(gpu):
    """not_erase NULL: the deferred candidate is culled, and the next one is judged without it."""
    r = CC.replay_culling("story")
    m, cur, order = CC.culling_story()
    m.not_erase = [False] * m.n_kf
    rec, status = CR.keyframe_culling(m, cur, order, CC.TH_DEPTH)
    want = np.array(rec, np.int32).view(r["want_records"][0].dtype).reshape(-1)
    assert want.tolist() != r["want_records"][0].tolist()
    records, summaries = run_culling_device(gpu, r, not_erase=False)
    check_culling(r, records, summaries, [want], r["want_summaries"])


@pytest.mark.parametrize("name", ["story", "second", "current_new_plane"])
def test_keyframe_culling_host_form(gpu, name):
    import spslam_match as M
    r = CC.replay_culling(name)
    p = r["packed"]
    cur, order = r["ordered"][0]
    kc = M.KeyFrameCulling(gpu, CC.TH_DEPTH)
    rec, summary = kc(p["t"], cur, order, p["keys_un"], p["uright"], p["depth"], p["cap"], p["new_plane"],
                      p["not_erase"])
    assert summary.tolist() == r["want_summaries"][0].tolist()
    assert rec.tolist() == r["want_records"][0].tolist()


# ---------------------------------------------------------------- MapPointCulling
def test_map_point_culling_device_and_host(gpu):
    """Two lists of one call with different current keyframes (more than one workgroup), the bytes past n kept;
    the host form; an empty list."""
    import spslam_match as M
    import torch
    tables, rows, cur, _ = CC.point_cull_tables()
    h = len(rows) // 2
    ids = np.where(np.arange(len(rows)) < h, cur, cur + 1).astype(np.int32)
    want = np.concatenate([CC.point_cull_want(tables, rows[:h], cur), CC.point_cull_want(tables, rows[h:], cur + 1)])
    assert (want[h:] != CC.point_cull_want(tables, rows[h:], cur)).any()
    mc = M.MapPointCulling(gpu)
    d = {name: dev(np.asarray(tables[name], dt)) for name, dt in M.POINT_CULL_TABLES}
    pm = M.PointCullMap(**{name: d[name].data_ptr() for name in d})
    d_rows, d_ids, d_verdict = dev(rows), dev(ids), sentinel(len(rows) + 8)
    mc.batch_device(pm, d_rows.data_ptr(), d_ids.data_ptr(), len(rows), d_verdict.data_ptr())
    torch.cuda.synchronize()
    got = d_verdict.cpu().numpy()
    assert got[:len(rows)].tolist() == want.tolist() and (got[len(rows):] == SENT).all()
    d_verdict = sentinel(8)
    mc.batch_device(pm, d_rows.data_ptr(), d_ids.data_ptr(), 0, d_verdict.data_ptr())
    mc.batch_device(pm, 0, 0, 0, 0)
    torch.cuda.synchronize()
    assert (d_verdict.cpu().numpy() == SENT).all()
    assert mc(tables, rows, cur).tolist() == CC.point_cull_want(tables, rows, cur).tolist()
    without = dict(tables, point_bad=None)
    clean = dict(tables, point_bad=np.zeros_like(tables["point_bad"]))
    assert mc(without, rows, cur).tolist() == CC.point_cull_want(clean, rows, cur).tolist()
    assert len(mc(tables, rows[:0], cur)) == 0


def test_validation_returns_errors_without_launching(gpu):
    import spslam_gpu
    import spslam_match as M
    r = CC.replay_update("counts_14_15")
    t, graph = r["steps"][0]["packed"]["t"], r["graph0"]
    with pytest.raises(spslam_gpu.SpslamError, match="covis_update_connections"):
        M.CovisUpdateConnections(gpu, th=0)(t, graph, r["stride"], 2)
    with pytest.raises(spslam_gpu.SpslamError, match="kf outside"):
        M.CovisUpdateConnections(gpu)(t, graph, r["stride"], 6)
    with pytest.raises(spslam_gpu.SpslamError, match="stride"):
        M.CovisUpdateConnections(gpu)(t, graph, 5, 2)
    outside = dict(t, match_row=np.where(t["match_row"] == 3, len(t["point_bad"]), t["match_row"]))
    with pytest.raises(spslam_gpu.SpslamError, match="outside the point table"):
        M.CovisUpdateConnections(gpu)(outside, graph, r["stride"], 2)
    with pytest.raises(spslam_gpu.SpslamError, match="update_connections_batch_device"):
        M.CovisUpdateConnections(gpu).batch_device(1, 1, M.CovisMap(), M.CovisGraph(), 1)
    c = CC.replay_culling("second")
    p = c["packed"]
    kc = M.KeyFrameCulling(gpu, CC.TH_DEPTH)
    with pytest.raises(spslam_gpu.SpslamError, match="candidate outside"):
        kc(p["t"], 8, [4, 9], p["keys_un"], p["uright"], p["depth"], p["cap"], p["new_plane"])
    with pytest.raises(spslam_gpu.SpslamError, match="longer than cap"):
        kc(p["t"], 8, [4], p["keys_un"][:, :4], p["uright"][:, :4], p["depth"][:, :4], 4, p["new_plane"])
    with pytest.raises(spslam_gpu.SpslamError, match="keyframe_culling_batch_device"):
        kc.batch_device(1, 1, M.CovisMap(), M.CovisGraph(), 1, 1, 1, 8, 1, 0, 1, 1)
    tables, rows, cur, _ = CC.point_cull_tables()
    with pytest.raises(spslam_gpu.SpslamError, match="outside the point table"):
        M.MapPointCulling(gpu)(tables, np.append(rows, len(tables["found"])), cur)
