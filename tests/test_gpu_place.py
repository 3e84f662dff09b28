"""GPU parity of the place-recognition entries on gfx950 -- spslam_place_reloc_candidates, spslam_place_loop_candidates
and spslam_place_min_score, device and host forms -- against the literal referee of tests/place_ref.py on the cases of
tests/place_cases.py (tests/test_place_host.py guards what each case reaches).  Bar: every byte equal -- result
records, candidates, reloc_score, loop_score and d_min_score; the buffers are pre-filled with a sentinel, so bytes
that must not be written are seen to be kept."""
import numpy as np
import pytest

import place_cases as PC

pytestmark = pytest.mark.gpu

SENT = PC.SENT


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


def device_tables(packed):
    import spslam_match as M
    import spslam_place as P
    t, f = packed["t"], packed["f"]
    d = {name: dev(np.asarray(t[name], dt)) for name, dt in P.PLACE_DB_TABLES}
    d.update({"f_" + name: dev(np.asarray(f[name], dt)) for name, dt in P.PLACE_FRAME_TABLES})
    d.update({name: dev(t[name]) for name in ("covis", "weights", "ordered", "n_ordered", "kf_bad")})
    db = P.PlaceDb(cap=packed["cap"], **{name: d[name].data_ptr() for name, _ in P.PLACE_DB_TABLES})
    frames = P.PlaceFrames(cap=packed["fcap"], **{name: d["f_" + name].data_ptr() for name, _ in P.PLACE_FRAME_TABLES})
    graph = M.CovisGraph(stride=packed["stride"], **{name: d[name].data_ptr()
                                                     for name in ("covis", "weights", "ordered", "n_ordered")})
    return d, db, frames, graph


def check_candidates(step, got, where):
    """The problem's candidates at its out_offset; every other slot keeps the sentinel."""
    written = np.zeros(len(got), bool)
    for prob, want in zip(step["problems"], step["cands"]):
        o = int(prob["out_offset"])
        assert got[o:o + len(want)].tolist() == want.tolist(), where
        written[o:o + len(want)] = True
    assert got[~written].tobytes() == bytes([SENT]) * (4 * int((~written).sum())), where


@pytest.mark.parametrize("name", list(PC.CASES))
def test_place_device(gpu, name):
    """The case's calls back to back on one stream over persistent tables: no synchronisation between them, the
    score tables copied on the stream after each call and everything compared at the end."""
    import spslam_place as P
    import torch
    r = PC.replay(name)
    packed = r["packed"]
    pr = P.PlaceRecognition(gpu)
    d, db, frames, graph = device_tables(packed)
    before = {k: d[k].clone() for k in d if k not in ("reloc_score", "loop_score", "in_db")}
    d_min = sentinel(4 * 4)                                  # at most two problems a call; the rest is watched
    out = []
    for s in r["steps"]:
        if s["kind"] in ("add", "erase"):
            d["in_db"][s["index"]] = s["value"]              # add() / erase() are the caller's
            out.append(None)
            continue
        n = len(s["problems"])
        d_problems = dev(s["problems"])
        d_results, d_cands = sentinel(32 * (n + 1)), sentinel(4 * (s["n_out"] + 2))
        if s["kind"] == "reloc":
            pr.reloc_candidates_batch_device(n, d_problems.data_ptr(), db, frames, graph, d_results.data_ptr(),
                                             d_cands.data_ptr())
        elif s["kind"] == "min":
            d_min.fill_(SENT)
            pr.min_score_batch_device(n, d_problems.data_ptr(), db, graph,
                                      d["kf_bad"].data_ptr() if s["use_bad"] else 0, d_min.data_ptr())
        else:
            if not s["chained"]:
                d_min = dev(np.concatenate([s["min_in"], np.frombuffer(bytes([SENT]) * (4 * (4 - n)), np.float32)]))
            pr.loop_candidates_batch_device(n, d_problems.data_ptr(), db, graph, d_min.data_ptr(),
                                            d_results.data_ptr(), d_cands.data_ptr())
        out.append((d_problems, d_results, d_cands, d_min.clone(), d["reloc_score"].clone(), d["loop_score"].clone()))
    torch.cuda.synchronize()
    for q, (s, o) in enumerate(zip(r["steps"], out)):
        if o is None:
            continue
        _, d_results, d_cands, d_min_after, reloc, loop = o
        n = len(s["problems"])
        assert host(reloc, np.float32).tobytes() == s["reloc_score"].tobytes(), (name, q)
        assert host(loop, np.float32).tobytes() == s["loop_score"].tobytes(), (name, q)
        if s["kind"] == "min":
            got = host(d_min_after, np.float32)
            assert got[:n].tobytes() == s["want_min"].tobytes(), (name, q, got[:n], s["want_min"])
            assert got[n:].tobytes() == bytes([SENT]) * (4 * (4 - n)), (name, q)
            assert (d_results == SENT).all() and (d_cands == SENT).all()
            continue
        got = host(d_results, P.PLACE_RESULT_DTYPE)
        assert got[:n].tobytes() == s["want"].tobytes(), (name, q, got[:n], s["want"])
        assert got[n:].tobytes() == bytes([SENT]) * 32, (name, q)
        check_candidates(s, host(d_cands, np.int32), (name, q))
    for k, v in before.items():                              # nothing but the score tables is written
        assert torch.equal(v, d[k]), k


def seq_tables(packed):
    t = packed["t"]
    return {name: t[name] for name in ("bow_words", "bow_values", "n_bow", "in_db", "reloc_score", "loop_score")}


@pytest.mark.parametrize("name", PC.SINGLE)
def test_place_host_forms(gpu, name):
    """The host forms on the single-problem cases, the state carried by the caller from call to call."""
    import spslam_place as P
    r = PC.replay(name)
    packed = r["packed"]
    t, f = packed["t"], packed["f"]
    pr = P.PlaceRecognition(gpu)
    db = seq_tables(packed)
    n_kf, cap, stride = packed["n_total"], packed["cap"], packed["stride"]
    last_min = None
    for q, s in enumerate(r["steps"]):
        if s["kind"] in ("add", "erase"):
            db["in_db"] = s["in_db"]
            continue
        query = int(s["problems"]["query"][0])
        if s["kind"] == "reloc":
            m = int(f["n_bow"][query])
            res, cand, score = pr.reloc_candidates(db, cap, n_kf, f["bow_words"][query, :m], f["bow_values"][query, :m],
                                                   t["covis"])
            db["reloc_score"] = score
        elif s["kind"] == "min":
            last_min = pr.min_score(db, cap, n_kf, query, t["ordered"], t["n_ordered"], stride,
                                    t["kf_bad"] if s["use_bad"] else None)
            assert np.float32(last_min).tobytes() == s["want_min"][0].tobytes(), (name, q)
            continue
        else:
            ms = last_min if s["chained"] else s["min_in"][0]
            res, cand, score = pr.loop_candidates(db, cap, n_kf, query, t["covis"], t["weights"], stride, ms)
            db["loop_score"] = score
        assert res.tobytes() == s["want"][0].tobytes(), (name, q, res, s["want"][0])
        assert cand.tolist() == s["cands"][0].tolist(), (name, q)
        assert db["reloc_score"].tobytes() == s["reloc_score"].tobytes(), (name, q)
        assert db["loop_score"].tobytes() == s["loop_score"].tobytes(), (name, q)


def test_host_forms_refuse_bad_indices(gpu):
    import spslam_gpu
    import spslam_match as M
    import spslam_place as P
    r = PC.replay("loop_story")
    packed = r["packed"]
    t = packed["t"]
    pr = P.PlaceRecognition(gpu)
    db, n_kf, cap, stride = seq_tables(packed), packed["n_total"], packed["cap"], packed["stride"]
    qw, qv = PC.vec([100, 101])
    err = spslam_gpu.SpslamError

    def covis_with(value):
        c = t["covis"].copy()
        c[3, 1] = value
        return c

    for value in (n_kf, -2):
        with pytest.raises(err, match="covis neighbour outside"):
            pr.reloc_candidates(db, cap, n_kf, qw, qv, covis_with(value))
        with pytest.raises(err, match="covis neighbour outside"):
            pr.loop_candidates(db, cap, n_kf, 9, covis_with(value), t["weights"], stride, 0.1)
    for query in (-1, n_kf):
        with pytest.raises(err, match="query outside"):
            pr.loop_candidates(db, cap, n_kf, query, t["covis"], t["weights"], stride, 0.1)
        with pytest.raises(err, match="query outside"):
            pr.min_score(db, cap, n_kf, query, t["ordered"], t["n_ordered"], stride)
    with pytest.raises(err, match="query keyframe is in the database"):
        pr.loop_candidates(db, cap, n_kf, 0, t["covis"], t["weights"], stride, 0.1)
    with pytest.raises(err, match="stride"):
        pr.loop_candidates(db, cap, n_kf, 9, t["covis"], t["weights"], n_kf - 1, 0.1)
    ordered = t["ordered"].copy()
    ordered[9, 1] = n_kf
    with pytest.raises(err, match="ordered keyframe outside"):
        pr.min_score(db, cap, n_kf, 9, ordered, t["n_ordered"], stride)
    n_ordered = t["n_ordered"].copy()
    n_ordered[9] = stride + 1
    with pytest.raises(err, match="longer than its row"):
        pr.min_score(db, cap, n_kf, 9, t["ordered"], n_ordered, stride)
    with pytest.raises(err, match="longer than cap"):
        pr.reloc_candidates(dict(db, n_bow=np.where(np.arange(n_kf) == 2, cap + 1, db["n_bow"])), cap, n_kf, qw, qv,
                            t["covis"])
    with pytest.raises(err, match="longer than cap"):
        pr.reloc_candidates(dict(db, n_bow=np.where(np.arange(n_kf) == 2, -1, db["n_bow"])), cap, n_kf, qw, qv,
                            t["covis"])
    words = db["bow_words"].copy()
    words[1, 0], words[1, 1] = words[1, 1], words[1, 0]
    with pytest.raises(err, match="do not ascend"):
        pr.reloc_candidates(dict(db, bow_words=words), cap, n_kf, qw, qv, t["covis"])
    with pytest.raises(err, match="do not ascend"):
        pr.reloc_candidates(db, cap, n_kf, qw[::-1], qv, t["covis"])
    for bad_n in (0, M.COVIS_MAX_KF + 1):
        with pytest.raises(err, match="n_kf outside"):
            pr.reloc_candidates(db, cap, bad_n, qw, qv, np.full((max(bad_n, 1), 10), -1, np.int32))
    with pytest.raises(err, match="cap outside"):
        pr.reloc_candidates(db, P.PLACE_MAX_WORDS + 1, n_kf, qw, qv, t["covis"])
    with pytest.raises(err, match="reloc_candidates_batch_device"):
        pr.reloc_candidates_batch_device(1, 1, P.PlaceDb(), P.PlaceFrames(), M.CovisGraph(), 1, 1)
    with pytest.raises(err, match="loop_candidates_batch_device"):
        pr.loop_candidates_batch_device(1, 1, P.PlaceDb(), M.CovisGraph(), 1, 1, 1)
    with pytest.raises(err, match="min_score_batch_device"):
        pr.min_score_batch_device(1, 1, P.PlaceDb(), M.CovisGraph(), 0, 1)
