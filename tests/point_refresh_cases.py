"""The cases of the map-point refresh tests (tests/test_point_refresh_host.py guards what each reaches,
tests/test_gpu_point_refresh.py runs them on the device): two small maps whose rows are made one by one -- observer
counts around the kernel's lane-group size (8), its wave size (64) and its capacity, planted descriptors that tie,
bad keyframes among the observers, reference keyframes that are not the first observer or not an observer.

A map: dict(t = the tables of spslam_point_refresh_map as numpy arrays, points = the table, keys_un [n_slots, cap],
desc [n_slots, cap, 32], names = {row name: row}).  pack() joins maps with absolute offsets and indices.
"""
import functools

import numpy as np

import point_refresh_ref as PR

GROUP = 8            # lanes per row of map_points_refresh_kernel
N_KF = PR.MAX_OBS + 2
BAD_KFS = (3, 50, 51, 90)
COUNTS = (1, 2, 3, 4, 5, GROUP - 1, GROUP, GROUP + 1, 63, 64, 65, PR.MAX_OBS)


def _near(rng, d, n_bits):
    b = np.unpackbits(d)
    b[rng.choice(256, n_bits, replace=False)] ^= 1
    return np.packbits(b)


def row_specs(rng):
    """[(name, observers (ascending keyframes) or a count, dict of options)]."""
    A, C = (rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(2))
    B = _near(rng, A, 10)
    specs = [(f"n{n}", n, {}) for n in COUNTS]
    specs += [
        ("over_capacity", PR.MAX_OBS + 1, {}),
        ("no_observers", 0, {}),
        ("bad_point", 4, dict(bad=True)),
        # C, A, B with A and B ten bits apart: rows 1 and 2 tie on the smallest median; row 1 gives the descriptor
        ("tie_small", [5, 6, 7], dict(descs=[C, A, B])),
        ("first_bad", [3, 10, 20], {}), ("middle_bad", [1, 3, 9, 12], {}), ("all_bad", [3, 50], {}),
        ("all_bad_wide", [3, 50, 51, 90], {}),
        ("ref_middle", [2, 8, 30, 40], dict(ref=30)), ("ref_absent", [2, 8, 30, 40], dict(ref=41)),
        ("ref_last_wide", list(range(10, 90, 2)), dict(ref=88)), ("ref_absent_wide", list(range(10, 90, 2)), dict(ref=11)),
        ("ref_second_chunk", list(range(0, 100)), dict(ref=77)),
        # 12 observers, the whole wave's path: rows 2 .. 11 tie (A five times, B five times), row 2 gives A
        ("dup_wide", list(range(20, 32)), dict(descs=[C] * 2 + [A] * 5 + [B] * 5)),
    ]
    return specs


def make_map(seed):
    import spslam_gpu
    import spslam_match
    rng = np.random.default_rng(seed)
    specs = row_specs(rng)
    n_rows, cap = len(specs), len(specs)
    slot = rng.permutation(N_KF).astype(np.int32)
    keys_un = np.zeros((N_KF, cap), spslam_gpu.KEYPOINT_DTYPE)
    keys_un["octave"] = rng.integers(0, 8, (N_KF, cap))
    desc = rng.integers(0, 256, (N_KF, cap, 32), dtype=np.uint8)
    Tcw = np.zeros((N_KF, 4, 4), np.float32)
    for k in range(N_KF):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        Tcw[k, :3, :3], Tcw[k, :3, 3], Tcw[k, 3, 3] = q, rng.normal(size=3) * 2, 1
    kf_bad = np.zeros(N_KF, np.uint8)
    kf_bad[list(BAD_KFS)] = 1
    points = rng.integers(0, 256, n_rows * 80, dtype=np.uint8).view(spslam_match.LOCAL_POINT_DTYPE).copy()
    points["xw"] = rng.normal(size=(n_rows, 3)) * 3
    obs_off, obs_kf, obs_kp, ref_kf = [0], [], [], []
    point_bad = np.zeros(n_rows, np.uint8)
    next_kp = np.zeros(N_KF, int)
    names = {}
    for r, (name, who, opt) in enumerate(specs):
        names[name] = r
        kfs = sorted(rng.choice(N_KF, who, replace=False).tolist()) if isinstance(who, int) else list(who)
        for n, k in enumerate(kfs):
            kp = int(next_kp[k])
            next_kp[k] += 1
            obs_kf.append(k)
            obs_kp.append(kp)
            if "descs" in opt:
                desc[slot[k], kp] = opt["descs"][n]
        obs_off.append(len(obs_kf))
        point_bad[r] = opt.get("bad", False)
        # mpRefKF: an observer that is not the first where there is a choice
        ref_kf.append(opt.get("ref", kfs[len(kfs) // 2] if kfs else 0))
    t = dict(kf_Tcw=Tcw.reshape(N_KF, 16), kf_slot=slot, kf_bad=kf_bad, obs_off=np.array(obs_off, np.int32),
             obs_kf=np.array(obs_kf, np.int32), obs_kp=np.array(obs_kp, np.int32),
             ref_kf=np.array(ref_kf, np.int32), point_bad=point_bad)
    return dict(t=t, points=points, keys_un=keys_un, desc=desc, names=names)


def pack(maps):
    """Several maps as one: offsets, keyframe indices and slots made absolute."""
    t = {}
    kf_base = np.cumsum([0] + [len(m["t"]["kf_slot"]) for m in maps])
    obs_base = np.cumsum([0] + [len(m["t"]["obs_kf"]) for m in maps])
    row_base = np.cumsum([0] + [len(m["points"]) for m in maps])
    t["kf_Tcw"] = np.concatenate([m["t"]["kf_Tcw"] for m in maps])
    t["kf_slot"] = np.concatenate([m["t"]["kf_slot"] + kf_base[i] for i, m in enumerate(maps)]).astype(np.int32)
    t["kf_bad"] = np.concatenate([m["t"]["kf_bad"] for m in maps])
    t["obs_off"] = np.concatenate([m["t"]["obs_off"][:-1] + obs_base[i] for i, m in enumerate(maps)] +
                                  [[obs_base[-1]]]).astype(np.int32)
    t["obs_kf"] = np.concatenate([m["t"]["obs_kf"] + kf_base[i] for i, m in enumerate(maps)]).astype(np.int32)
    t["obs_kp"] = np.concatenate([m["t"]["obs_kp"] for m in maps])
    t["ref_kf"] = np.concatenate([m["t"]["ref_kf"] + kf_base[i] for i, m in enumerate(maps)]).astype(np.int32)
    t["point_bad"] = np.concatenate([m["t"]["point_bad"] for m in maps])
    cap = maps[0]["keys_un"].shape[1]
    assert all(m["keys_un"].shape[1] == cap for m in maps)
    names = {f"{i}:{k}": v + row_base[i] for i, m in enumerate(maps) for k, v in m["names"].items()}
    return dict(t=t, points=np.concatenate([m["points"] for m in maps]),
                keys_un=np.concatenate([m["keys_un"] for m in maps]), desc=np.concatenate([m["desc"] for m in maps]),
                names=names, row_base=row_base)


def scale_factors():
    """ORBextractor.cc:417-423: mvScaleFactor[i] = mvScaleFactor[i-1] * scaleFactor, in float."""
    s = [np.float32(1.0)]
    for _ in range(7):
        s.append(np.float32(s[-1] * np.float32(1.2)))
    return s


@functools.lru_cache(maxsize=None)
def build():
    """The packed pair of maps, a scrambled row list over both (every row once), and the restatement's table and
    status for each mask."""
    packed = pack([make_map(41), make_map(42)])
    rows = np.random.default_rng(7).permutation(len(packed["points"])).astype(np.int32)
    want = {}
    for what in (PR.DESCRIPTOR, PR.NORMAL_DEPTH, PR.DESCRIPTOR | PR.NORMAL_DEPTH):
        traces = []
        want[what] = PR.refresh(packed["t"], packed["points"], rows, what, packed["keys_un"], packed["desc"],
                                scale_factors(), traces) + (traces,)
    return packed, rows, want
