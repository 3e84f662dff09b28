"""The maps of the covisibility tests, small and seeded, with their packing into the tables of include/spslam_gpu.h
and the replay of each case through the referees of covis_ref.py.  tests/test_covis_host.py guards that every case
reaches the branch it is named for; tests/test_gpu_covis.py runs the device on the same replays."""
import copy
import functools

import numpy as np

import covis_ref as CR
import spslam_gpu
import spslam_match as M

SENT = 0xEE
SENT32 = int(np.array([0xEEEEEEEE], np.uint32).view(np.int32)[0])
TH_DEPTH = 3.0


# ---------------------------------------------------------------- packing
def pack(maps, cap=0):
    """Several sequences' maps as the flat tables of spslam_covis_map (absolute CSR offsets, indices local to the
    sequence) with the per-sequence bases; cap > 0 adds the frame arrays (slot = the keyframes in reverse, so that
    kf_slot is followed) and the per-keyframe flags."""
    kf_base, row_base = [], []
    match_off, match_row, obs_off, obs_kf, obs_kp, bad, n_obs = [0], [], [0], [], [], [], []
    for m in maps:
        kf_base.append(len(match_off) - 1)
        row_base.append(len(obs_off) - 1)
        for k in range(m.n_kf):
            match_row += [-1 if r is None else r for r in m.matches[k]]
            match_off.append(len(match_row))
        for r in range(len(m.obs)):
            for k in sorted(m.obs[r]):
                obs_kf.append(k)
                obs_kp.append(m.obs[r][k])
            obs_off.append(len(obs_kf))
            bad.append(m.bad[r])
            n_obs.append(m.n_obs[r])
    points = np.zeros(len(bad), M.LOCAL_POINT_DTYPE)
    points["n_obs"] = n_obs
    points["id"] = np.arange(len(bad))
    n_total = len(match_off) - 1
    t = dict(match_off=np.array(match_off, np.int32), match_row=np.array(match_row, np.int32),
             obs_off=np.array(obs_off, np.int32), obs_kf=np.array(obs_kf, np.int32),
             obs_kp=np.array(obs_kp, np.int32), kf_slot=np.arange(n_total, dtype=np.int32)[::-1].copy(),
             point_bad=np.array(bad, np.uint8), points=points)
    out = dict(t=t, kf_base=kf_base, row_base=row_base, n_kf=[m.n_kf for m in maps], cap=cap)
    if cap:
        keys = np.zeros((n_total, cap), spslam_gpu.KEYPOINT_DTYPE)
        keys["octave"] = 7                                # unused slots: never a qualifying level
        uright = np.full((n_total, cap), 5.0, np.float32)
        depth = np.full((n_total, cap), -2.0, np.float32)
        new_plane, not_erase = np.zeros(n_total, np.uint8), np.zeros(n_total, np.uint8)
        for m, b in zip(maps, kf_base):
            for k in range(m.n_kf):
                n, s = len(m.matches[k]), t["kf_slot"][b + k]
                assert n <= cap
                keys["octave"][s, :n] = m.octave[k]
                uright[s, :n] = m.uright[k]
                depth[s, :n] = m.depth[k]
                new_plane[b + k], not_erase[b + k] = m.new_plane[k], m.not_erase[k]
        out.update(keys_un=keys, uright=uright, depth=depth, new_plane=new_plane, not_erase=not_erase)
    return out


def fresh_graph(n_kfs, stride):
    """The device graph of fresh sequences (n_kfs: keyframes per sequence): no weights, empty lists, covis -1, no
    parent, mbFirstConnection set.  The list entries and the weight columns past a sequence's n_kf hold a sentinel
    that no call may touch."""
    n = sum(n_kfs)
    g = dict(weights=np.zeros((n, stride), np.int32), ordered=np.full((n, stride), SENT32, np.int32),
             ordered_w=np.full((n, stride), SENT32, np.int32), n_ordered=np.zeros(n, np.int32),
             covis=np.full((n, M.COVIS_BEST), -1, np.int32), parent=np.full(n, -1, np.int32),
             first_connection=np.ones(n, np.uint8))
    b = 0
    for nk in n_kfs:
        g["weights"][b:b + nk, nk:] = SENT32
        b += nk
    return g


def mirror(arrays, kfb, n_kf, g, kf, rewritten):
    """Writes what one UpdateConnections of `kf` changed in the referee's graph g into the arrays, as the ABI
    states it: the keyframe's whole weights row, one weights entry per re-sorted neighbour, and for every
    rewritten list its entries, their count and the covis row; entries past the count are kept."""
    row = np.zeros(n_kf, np.int32)
    for j, w in g.weights[kf].items():
        row[j] = w
    arrays["weights"][kfb + kf, :n_kf] = row
    for x in rewritten:
        if x != kf:
            arrays["weights"][kfb + x, kf] = g.weights[x][kf]
        n = len(g.ordered[x])
        arrays["ordered"][kfb + x, :n] = g.ordered[x]
        arrays["ordered_w"][kfb + x, :n] = g.ordered_w[x]
        arrays["n_ordered"][kfb + x] = n
        arrays["covis"][kfb + x] = (g.ordered[x] + [-1] * M.COVIS_BEST)[:M.COVIS_BEST]
    arrays["parent"][kfb + kf] = g.parent[kf]
    arrays["first_connection"][kfb + kf] = g.first_connection[kf]


# ---------------------------------------------------------------- UpdateConnections cases
def share(m, a, b, count):
    """count points seen by exactly a and b."""
    for _ in range(count):
        m.add_point([a, b])


def windowed(n_kf, per_kf, window, seed):
    """A seeded map in which every point is seen by 2 .. 4 keyframes of a window of consecutive ones."""
    rng = np.random.default_rng(seed)
    m = CR.Map(n_kf)
    for _ in range(n_kf * per_kf // 3):
        lo = int(rng.integers(0, max(n_kf - window, 0) + 1))
        ks = rng.choice(np.arange(lo, min(lo + window, n_kf)), size=min(int(rng.integers(2, 5)), n_kf, window),
                        replace=False)
        m.add_point(sorted(int(k) for k in ks))
    return m


def _sizes(n_kf, seed):
    m = CR.Map(2) if n_kf == 2 else windowed(n_kf, 60 if n_kf <= 65 else 48, 5, seed)
    if n_kf == 2:
        share(m, 0, 1, 20)
    return dict(maps=[m], calls=[dict(problems=[(0, k)]) for k in (0, n_kf // 2, n_kf - 1)])


def _empty():
    m = CR.Map(4)
    share(m, 0, 1, 16)
    for _ in range(5):
        m.add_point([2])                                  # seen by itself only
    m.add_keypoint(2)
    return dict(maps=[m], calls=[dict(problems=[(0, 0)]), dict(problems=[(0, 2)])], expect=["empty"])


def _fourteen_fifteen():
    m = CR.Map(6)
    share(m, 2, 1, 14)
    share(m, 2, 4, 15)
    return dict(maps=[m], calls=[dict(problems=[(0, 2)])], expect=["below_th"])


def _equal_maxima():
    m = CR.Map(8)
    share(m, 6, 3, 7)
    share(m, 6, 5, 7)
    share(m, 6, 1, 2)
    return dict(maps=[m], calls=[dict(problems=[(0, 6)])], expect=["only_maximum"])


def _equal_weights():
    m = CR.Map(8)
    share(m, 1, 2, 20)
    share(m, 1, 6, 20)
    share(m, 1, 4, 16)
    share(m, 1, 7, 31)
    return dict(maps=[m], calls=[dict(problems=[(0, 1)])])


def _list_length(n):
    """n ordered entries with many equal weights: 9 .. 11 around the covis table's 10, 64 / 65 and 128 / 129 around
    the sizes at which the device's sort network doubles."""
    m = CR.Map(max(n + 3, 14))
    for q in range(n):
        share(m, 0, 1 + q, 15 + (q * 5) % 7)
    return dict(maps=[m], calls=[dict(problems=[(0, 0)])])


def _null_and_bad_rows():
    """Fifteen good shared points among bad ones and empty keypoints: counting a bad one would reach th for
    keyframe 3 too."""
    m = CR.Map(5)
    for q in range(15):
        m.add_keypoint(1)
        m.add_point([1, 2])
        m.add_point([1, 3], bad=q % 2 == 0)
    for _ in range(7):
        m.add_point([1, 3])
    return dict(maps=[m], calls=[dict(problems=[(0, 1)])], expect=["null_row", "bad_row", "own_observation"])


def _resort_pair(changed):
    """Keyframe 3 updates first: its row holds keyframe 5 (9 shared, below th) that its list leaves out.  Then
    keyframe 1 updates with its weight in 3's row unchanged (3's list must stay as it is: a re-sort would bring 5
    in), or, with one more shared point, changed (5 enters 3's list)."""
    m = CR.Map(7)
    share(m, 3, 1, 17)
    share(m, 3, 5, 9)
    share(m, 3, 6, 15)

    def one_more(maps):
        maps[0].add_point([1, 3])
    second = dict(problems=[(0, 1)], mutate=one_more) if changed else dict(problems=[(0, 1)])
    return dict(maps=[m], calls=[dict(problems=[(0, 3)]), second],
                expect=[] if changed else ["unchanged_weight"])


def _first_connection():
    m = CR.Map(4)
    share(m, 0, 2, 16)
    share(m, 2, 3, 18)
    return dict(maps=[m], calls=[dict(problems=[(0, 0)]), dict(problems=[(0, 2)]), dict(problems=[(0, 2)])],
                expect=["first_connection"])


def _star():
    """Fifteen points that every one of 1024 keyframes sees: keyframe 5 connects to all other 1023."""
    m = CR.Map(1024)
    for _ in range(15):
        m.add_point(range(1024))
    return dict(maps=[m], calls=[dict(problems=[(0, 5)])])


def _two_sequences():
    return dict(maps=[windowed(9, 60, 4, 11), windowed(33, 60, 5, 12)],
                calls=[dict(problems=[(0, 4), (1, 20)]), dict(problems=[(1, 21), (0, 8)])])


def _stream_of_calls():
    n = 12
    return dict(maps=[windowed(n, 70, 5, 21)], calls=[dict(problems=[(0, k)]) for k in range(1, n)], sync=False)


UPDATE_CASES = {
    "n_kf_2": lambda: _sizes(2, 1), "n_kf_64": lambda: _sizes(64, 2), "n_kf_65": lambda: _sizes(65, 3),
    "n_kf_1024": lambda: _sizes(1024, 4), "empty": _empty, "counts_14_15": _fourteen_fifteen,
    "equal_maxima": _equal_maxima, "equal_weights": _equal_weights, "list_9": lambda: _list_length(9),
    "list_10": lambda: _list_length(10), "list_11": lambda: _list_length(11), "list_64": lambda: _list_length(64),
    "list_65": lambda: _list_length(65), "list_128": lambda: _list_length(128), "list_129": lambda: _list_length(129),
    "null_and_bad_rows": _null_and_bad_rows, "unchanged_neighbour": lambda: _resort_pair(False),
    "changed_neighbour": lambda: _resort_pair(True), "first_connection": _first_connection, "star_1024": _star,
    "two_sequences": _two_sequences, "stream_of_calls": _stream_of_calls,
}


@functools.lru_cache(maxsize=None)
def replay_update(name):
    """The case run through the referee.  Returns dict(stride, n_kfs, graph0, steps, stats, sync, graphs); a step
    is dict(packed: the tables the call reads (None: those of the step before), problems: COVIS_PROBLEM_DTYPE
    records, want: COVIS_RESULT_DTYPE records, graph: the graph arrays after the call)."""
    case = UPDATE_CASES[name]()
    maps = case["maps"]
    n_kfs = [m.n_kf for m in maps]
    stride = max(n_kfs) + 3
    arrays = fresh_graph(n_kfs, stride)
    graph0 = copy.deepcopy(arrays)
    graphs = [CR.Graph(nk) for nk in n_kfs]
    stats = CR.collections.Counter()
    steps, packed = [], None
    for q, call in enumerate(case["calls"]):
        if "mutate" in call:
            call["mutate"](maps)
        fresh = pack(maps) if q == 0 or "mutate" in call else None
        packed = fresh or packed
        problems = np.zeros(len(call["problems"]), M.COVIS_PROBLEM_DTYPE)
        want = np.zeros(len(call["problems"]), M.COVIS_RESULT_DTYPE)
        assert len({s for s, _ in call["problems"]}) == len(call["problems"])   # one problem per sequence
        for p, (s, kf) in enumerate(call["problems"]):
            problems[p] = (packed["kf_base"][s], packed["row_base"][s], kf, n_kfs[s])
            res, rewritten = CR.update_connections(maps[s], graphs[s], kf, stats=stats)
            want[p] = res
            if res[0] == CR.UPDATED:
                mirror(arrays, packed["kf_base"][s], n_kfs[s], graphs[s], kf, rewritten)
        steps.append(dict(packed=fresh, problems=problems, want=want, graph=copy.deepcopy(arrays)))
    return dict(stride=stride, n_kfs=n_kfs, graph0=graph0, steps=steps, stats=stats, sync=case.get("sync", True),
                graphs=graphs, expect=case.get("expect", []), maps=maps)


# ---------------------------------------------------------------- KeyFrameCulling cases
def _obs(octave=0, stereo=True, depth=1.0):
    return dict(octave=octave, stereo=stereo, depth=depth)


def redundant(m, c, helpers, count, level=2, **own):
    """count keypoints of c that three helper keyframes see at a level that qualifies."""
    for _ in range(count):
        m.add_point({c: _obs(level, **own), **{h: _obs(level) for h in helpers[:3]}})


def plain(m, c, helper, count):
    """count keypoints of c with one other observer: counted, never redundant."""
    for _ in range(count):
        m.add_point({c: _obs(2), helper: _obs(2)})


def culling_story():
    """One sequence that holds every single-sequence case; the current keyframe is 1, the helpers 2 .. 5 are no
    candidates (so they are never culled).  Returns (map, current, candidate list)."""
    m = CR.Map(40)
    H = [2, 3, 4, 5]
    order = []
    m.new_plane[6] = True
    redundant(m, 6, H, 4)
    order += [0, 6]                                       # index 0, a candidate with mbNewPlane
    order.append(7)                                       # no keypoints at all: nMPs == 0
    m.add_point({8: _obs(2), **{h: _obs(2) for h in H[:3]}})
    order.append(8)                                       # one keypoint
    redundant(m, 9, H, 260)
    plain(m, 9, 2, 10)
    order.append(9)                                       # more than 256 keypoints
    for c, n, r in ((10, 10, 9), (11, 10, 10), (12, 20, 18), (13, 20, 19)):
        redundant(m, c, H, r)
        plain(m, c, 2, n - r)
        order.append(c)
    # depth: < 0 and just above th_depth are not counted, == th_depth is
    above = float(np.nextafter(np.float32(TH_DEPTH), np.float32(10)))
    for d in (-0.5, TH_DEPTH, above, TH_DEPTH, above, -1.0, 0.0):
        redundant(m, 14, H, 1, depth=d)
    order.append(14)
    # Observations() 3 and 4, the observers' level at +1 and +2, two and three that qualify
    m.add_point({15: _obs(2, stereo=False), 2: _obs(2, False), 3: _obs(2, False), 4: _obs(2, False)}, n_obs=3)
    m.add_point({15: _obs(2, stereo=False), 2: _obs(2, False), 3: _obs(2, False), 4: _obs(2, False)})
    m.add_point({15: _obs(2), 2: _obs(3), 3: _obs(3), 4: _obs(3)})
    m.add_point({15: _obs(2), 2: _obs(3), 3: _obs(4), 4: _obs(3)})
    m.add_point({15: _obs(2), 2: _obs(4), 3: _obs(3), 4: _obs(3), 5: _obs(0)})
    m.add_point({15: _obs(2), 2: _obs(1), 3: _obs(2)})
    m.add_keypoint(15)
    m.add_point({15: _obs(2), 2: _obs(2), 3: _obs(2), 4: _obs(2)}, bad=True)
    order.append(15)
    # A (16) is culled; B (17) was redundant only through A
    redundant(m, 16, H, 6)
    for _ in range(6):
        m.add_point({17: _obs(2), 16: _obs(2), 2: _obs(2), 3: _obs(2)})
    order += [16, 17]
    # A (18) is culled and takes a point of B (19) to nObs <= 2: nMPs 10 -> 9 with 9 redundant
    redundant(m, 18, H, 12)
    redundant(m, 19, H, 9)
    m.add_point({19: _obs(2, stereo=False), 18: _obs(2, stereo=True)})
    order += [18, 19]
    # the same twice with Observations() == 4 in both: only the culled observation's weight, 2 or 1, decides
    for a, b, a_stereo in ((20, 21, True), (22, 23, False)):
        redundant(m, a, H, 12)
        redundant(m, b, H, 9)
        m.add_point({b: _obs(2, stereo=not a_stereo), a: _obs(2, stereo=a_stereo), 2: _obs(2, stereo=False)})
        order += [a, b]
    # a candidate with mbNotErase: deferred, and still an observer for the next one
    m.not_erase[24] = True
    redundant(m, 24, H, 6)
    for _ in range(6):
        m.add_point({25: _obs(2), 24: _obs(2), 2: _obs(2), 3: _obs(2)})
    order += [24, 25]
    return m, 1, order


def culling_second():
    """A second, smaller sequence: keyframe 3 is culled, 2 depends on it."""
    m = CR.Map(9)
    H = [5, 6, 7]
    redundant(m, 3, H, 12, level=1)
    for _ in range(5):
        m.add_point({2: _obs(1), 3: _obs(1), 5: _obs(2), 6: _obs(0)})
    redundant(m, 4, H, 3)
    plain(m, 4, 8, 1)
    return m, 8, [4, 3, 2, 0]


def culling_new_plane():
    m, cur, order = culling_second()
    m.new_plane[cur] = True
    return m, cur, order


CULL_CASES = {"story": [culling_story], "second": [culling_second], "current_new_plane": [culling_new_plane],
              "two_sequences": [culling_second, culling_story, culling_new_plane]}
CULL_CAP = 512


@functools.lru_cache(maxsize=None)
def replay_culling(name):
    """Returns dict(packed, problems, ordered (per sequence), want_records, want_summaries, stats): the tables are
    packed before the referee mutates the maps."""
    built = [f() for f in CULL_CASES[name]]
    maps = [b[0] for b in built]
    packed = pack(maps, CULL_CAP)
    stats = CR.collections.Counter()
    problems = np.zeros(len(built), M.CULL_PROBLEM_DTYPE)
    summaries = np.zeros(len(built), M.CULL_SUMMARY_DTYPE)
    records, ordered, off = [], [], 0
    for p, (m, cur, order) in enumerate(built):
        for key, v in zip(("kf_base", "row_base", "kf", "n_kf", "out_offset"),
                          (packed["kf_base"][p], packed["row_base"][p], cur, m.n_kf, off + 2 * p)):
            problems[key][p] = v
        rec, status = CR.keyframe_culling(m, cur, order, TH_DEPTH, stats=stats)
        summaries[p] = (len(rec), status)
        records.append(np.array(rec, np.int32).reshape(-1, 4).view(M.CULL_RECORD_DTYPE).reshape(-1))
        ordered.append((cur, order))
        off += len(order)
    return dict(packed=packed, problems=problems, ordered=ordered, want_records=records, want_summaries=summaries,
                stats=stats, n_out=off + 2 * len(built))


# ---------------------------------------------------------------- MapPointCulling cases
def point_cull_tables():
    """Rows for every branch and for the order between them, then seeded ones; current keyframe id 10."""
    cur = 10
    named = [  # found, visible, first_kf, bad, n_obs -> the verdict's name
        ("drop", 0, 10, 0, 1, 1), ("drop_before_ratio", 1, 100, 9, 1, 9),
        ("bad_ratio", 24, 100, 10, 0, 9), ("ratio_before_obs", 1, 5, 7, 0, 2), ("ratio_exactly_quarter", 1, 4, 10, 0, 9),
        ("bad_obs", 9, 10, 8, 0, 3), ("bad_obs_before_expired", 9, 10, 2, 0, 2), ("four_observations", 9, 10, 8, 0, 4),
        ("expired", 9, 10, 7, 0, 9), ("young", 9, 10, 9, 0, 1), ("keep", 5, 5, 10, 0, 8),
        ("never_visible", 0, 0, 10, 0, 9), ("found_unseen", 3, 0, 10, 0, 9),
    ]
    rng = np.random.default_rng(5)
    n = 700
    t = dict(found=rng.integers(0, 40, n), visible=rng.integers(1, 60, n), first_kf=rng.integers(5, 11, n),
             point_bad=(rng.random(n) < 0.15), n_obs=rng.integers(0, 8, n))
    for q, (_, f, v, k, b, o) in enumerate(named):
        for key, val in zip(("found", "visible", "first_kf", "point_bad", "n_obs"), (f, v, k, b, o)):
            t[key][q] = val
    points = np.zeros(n, M.LOCAL_POINT_DTYPE)
    points["n_obs"] = t["n_obs"]
    tables = dict(found=t["found"].astype(np.int32), visible=t["visible"].astype(np.int32),
                  first_kf=t["first_kf"].astype(np.int32), point_bad=t["point_bad"].astype(np.uint8), points=points)
    rows = np.concatenate([np.arange(len(named)), rng.permutation(n)[:600]]).astype(np.int32)
    return tables, rows, cur, {name: q for q, (name, *_) in enumerate(named)}


def point_cull_want(tables, rows, cur):
    return CR.map_point_culling(tables["found"], tables["visible"], tables["first_kf"], tables["point_bad"],
                                tables["points"]["n_obs"], rows, cur)
