"""GPU parity: MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth (src/MapPoint.cc:242-307, :330-371)
on gfx950 -- spslam_map_points_refresh_batch_device and its host-pointer form -- against the scalar restatement
tests/point_refresh_ref.py.  Bar: the whole table byte for byte and every status.  The cases are
tests/point_refresh_cases.py; tests/test_point_refresh_host.py guards that each reaches what it is there for."""
import numpy as np
import pytest

import point_refresh_cases as PC
import point_refresh_ref as PR

pytestmark = pytest.mark.gpu

BOTH = PR.DESCRIPTOR | PR.NORMAL_DEPTH
SENT = 0xEE


@pytest.fixture(scope="module")
def gpu():
    import spslam_gpu
    import spslam_match
    ex = spslam_gpu.OrbExtractor(max_batch=1)
    assert [np.float32(s) for s in ex.tables()["scale"]] == PC.scale_factors()
    yield ex, spslam_match.PointRefresh(ex)
    ex.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def run_device(gpu, packed, rows, what, n=None, table=None, with_flags=True):
    """One launch on fresh device copies (or on the device table `table`): the table and the status bytes after."""
    import spslam_match as M
    import torch
    ex, pr = gpu
    t = packed["t"]
    d = {name: dev(np.asarray(t[name], dt)) for name, dt in M.REFRESH_MAP_TABLES}
    d_points = dev(packed["points"]) if table is None else table
    d_rows, d_keys, d_desc = dev(rows), dev(packed["keys_un"]), dev(packed["desc"])
    d_status = torch.full((len(rows) + 4,), SENT, dtype=torch.uint8, device="cuda")
    m = M.PointRefreshMap(points=d_points.data_ptr(), **{
        name: d[name].data_ptr() if with_flags or name not in ("kf_bad", "point_bad") else None
        for name, _ in M.REFRESH_MAP_TABLES})
    n = len(rows) if n is None else n
    pr.batch_device(m, d_rows.data_ptr(), n, what, d_keys.data_ptr(), d_desc.data_ptr(), packed["keys_un"].shape[1],
                    d_status.data_ptr())
    torch.cuda.synchronize()
    status = d_status.cpu().numpy()
    assert (status[n:] == SENT).all()
    return d_points.cpu().numpy().view(M.LOCAL_POINT_DTYPE), status[:n], d_points


@pytest.mark.parametrize("what", [PR.DESCRIPTOR, PR.NORMAL_DEPTH, BOTH], ids=["descriptor", "normal_depth", "both"])
def test_packed_maps_match_the_restatement(gpu, what):
    packed, rows, want = PC.build()
    table, status, _ = run_device(gpu, packed, rows, what)
    want_table, want_status, _ = want[what]
    assert status.tolist() == want_status.tolist()
    bad = np.flatnonzero([table[r].tobytes() != want_table[r].tobytes() for r in range(len(table))])
    names = {v: k for k, v in packed["names"].items()}
    assert table.tobytes() == want_table.tobytes(), [(names[r], table[r], want_table[r]) for r in bad[:4]]


def test_listed_rows_only_and_in_two_launches(gpu):
    """Half of the list: the other rows keep every byte; the second half on the same device table completes it."""
    packed, rows, want = PC.build()
    h = len(rows) // 2
    table, status, d_table = run_device(gpu, packed, rows[:h], BOTH)
    want_table, want_status, _ = want[BOTH]
    listed = np.zeros(len(table), bool)
    listed[rows[:h]] = True
    assert table[~listed].tobytes() == packed["points"][~listed].tobytes()
    assert table[listed].tobytes() == want_table[listed].tobytes() and status.tolist() == want_status[:h].tolist()
    table, status, _ = run_device(gpu, packed, rows[h:], BOTH, table=d_table)
    assert table.tobytes() == want_table.tobytes() and status.tolist() == want_status[h:].tolist()
    # n smaller than the list: the entries past n are not read
    table, status, _ = run_device(gpu, packed, rows, BOTH, n=5)
    listed[:] = False
    listed[rows[:5]] = True
    assert table[~listed].tobytes() == packed["points"][~listed].tobytes() and len(status) == 5


def test_without_bad_flags(gpu):
    """kf_bad and point_bad NULL: nothing is bad."""
    packed, rows, _ = PC.build()
    clean = dict(packed, t=dict(packed["t"], kf_bad=None, point_bad=None))
    want_table, want_status = PR.refresh(clean["t"], packed["points"], rows, BOTH, packed["keys_un"], packed["desc"],
                                         PC.scale_factors())
    table, status, _ = run_device(gpu, packed, rows, BOTH, with_flags=False)
    assert table.tobytes() == want_table.tobytes() and status.tolist() == want_status.tolist()
    assert (want_status == PR.UNTOUCHED).sum() == 2      # the rows without observers only


def test_host_form_equals_the_device_form(gpu):
    import spslam_match as M
    ex, pr = gpu
    packed, rows, want = PC.build()
    cap = packed["keys_un"].shape[1]
    for what in (PR.NORMAL_DEPTH, BOTH):
        table, status, rc = pr(packed["t"], packed["points"], rows, what, packed["keys_un"], packed["desc"], cap)
        assert rc == M.ERR_CAPACITY and b"observers" in ex.lib.spslam_last_error(ex.ctx)
        assert table.tobytes() == want[what][0].tobytes() and status.tolist() == want[what][1].tolist()
    keep = rows[want[BOTH][1] != PR.CAPACITY]
    table, status, rc = pr(packed["t"], packed["points"], keep, BOTH, packed["keys_un"], packed["desc"], cap)
    assert rc == 0 and table.tobytes() == want[BOTH][0].tobytes() and PR.CAPACITY not in status.tolist()
    table, status, rc = pr(packed["t"], packed["points"], rows[:0], BOTH, packed["keys_un"], packed["desc"], cap)
    assert rc == 0 and table.tobytes() == packed["points"].tobytes() and len(status) == 0


def test_validation_returns_errors_without_launching(gpu):
    import spslam_gpu
    import spslam_match as M
    ex, pr = gpu
    packed, rows, _ = PC.build()
    cap = packed["keys_un"].shape[1]
    full = M.PointRefreshMap(**{name: 1 for name, _ in M.REFRESH_MAP_TABLES}, points=1)
    for args in ((full, 1, 1, 0, 1, 1, cap, 1), (full, 1, 1, 4, 1, 1, cap, 1), (full, 0, 1, BOTH, 1, 1, cap, 1),
                 (full, 1, -1, BOTH, 1, 1, cap, 1), (full, 1, 1, BOTH, 1, 1, 0, 1), (full, 1, 1, BOTH, 1, 0, cap, 1),
                 (M.PointRefreshMap(), 1, 1, BOTH, 1, 1, cap, 1)):
        with pytest.raises(spslam_gpu.SpslamError, match="map_points_refresh"):
            pr.batch_device(*args)
    outside = rows.copy()
    outside[3] = len(packed["points"])
    with pytest.raises(spslam_gpu.SpslamError, match="outside its table"):
        pr(packed["t"], packed["points"], outside, BOTH, packed["keys_un"], packed["desc"], cap)
