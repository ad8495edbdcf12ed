"""clc_static_poses / clc_assemble_stations(_device) (K14, GetStaticPose src/utilities.cpp:86-155) on the GPU against the restatement
tests/stations_ref.py and the frozen output of the reference's own function: the walk's stations, member counts, run counts and
stamps exactly; the averages within derived bounds; scan -> station indices and offsets exactly, the stored points bit for bit;
host form == device form == a second run; the key-frame mode untouched; CalibrateOfflineStations against the oracle on the restated
records."""
import json
import os

import numpy as np
import pytest

import board_segment_ref as BS
import offline_ref as R
import stations_ref as SR
import camlasercalibratool_amd as clc
from camlasercalibratool_amd import calib, simdata as sd, simoffline as so

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = np.array([50.0, -40.0, 30.0])


@pytest.fixture(scope="module")
def sv():
    s = clc.Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def base_scans():
    """64 scans of 1 081 rays, most with a board."""
    return sd.sim_laser_scans(7, 64)


@pytest.fixture(scope="module")
def front(sv, base_scans):
    """The device's own points, segments and statuses of base_scans (computed once)."""
    return device_front(sv, base_scans)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def device_front(sv, scans):
    """TranScanToPoints + board segments on the device -> (points [M, 3], seg [S, 2], status [S])."""
    import torch
    off = np.ascontiguousarray(scans["offsets"], dtype=np.int64)
    S, n = len(off) - 1, int(off[-1])
    d_r, d_off, d_am, d_ai, d_rm = _dev(scans["ranges"]), _dev(off), _dev(scans["angle_min"]), _dev(scans["angle_increment"]), _dev(scans["range_min"])
    d_pts = torch.zeros((max(n, 1), 3), dtype=torch.float64, device=d_off.device)
    d_seg = torch.empty((S, 2), dtype=torch.int64, device=d_off.device)
    d_st = torch.empty((S,), dtype=torch.int32, device=d_off.device)
    torch.cuda.synchronize()
    sv.scan_to_points_device(d_r.data_ptr(), d_off.data_ptr(), S, n, d_am.data_ptr(), d_ai.data_ptr(), d_rm.data_ptr(), d_pts.data_ptr())
    sv.board_segments_device(d_pts.data_ptr(), d_off.data_ptr(), S, d_seg.data_ptr(), d_st.data_ptr())
    return d_pts.cpu().numpy()[:n], d_seg.cpu().numpy(), d_st.cpu().numpy()


def _opt(dist_max=None, min_members=None, close_last_run=None):
    o = clc.default_station_options()
    if dist_max is not None:
        o.center_dist_max = dist_max
    if min_members is not None:
        o.min_members = min_members
    if close_last_run is not None:
        o.close_last_run = close_last_run
    return o


# ---- the walk -----------------------------------------------------------------------------------------------------------------------
def dwell_walk(seed, n, sigma=0.0002):
    """Seeded dwell-and-move translations [n, 3]: dwells of 3 .. 90 poses (sigma of jitter about a centre, some with a slow drift),
    1 .. 3 moving poses in between.  The first draw whose membership distances all stay 1e-6 m clear of 2 mm is taken."""
    for attempt in range(64):
        rng = np.random.default_rng([seed, n, attempt])
        t = []
        while len(t) < n:
            c = rng.uniform(-2.0, 2.0, 3)
            d = rng.normal(0, 0.00002, 3) * (rng.random() < 0.3)
            for i in range(int(rng.integers(3, 91))):
                t.append(c + d * i + rng.normal(0, sigma, 3))
            for _ in range(int(rng.integers(1, 4))):
                t.append(rng.uniform(-2.0, 2.0, 3))
        t = np.array(t[:n]).reshape(n, 3)
        if SR.walk(t, min_members=0)["margin"] >= 1e-6:
            return t
    raise AssertionError("no draw with a margin")


def check_walk(sv, t, dist_max=SR.DIST_MAX, min_members=SR.MIN_MEMBERS, close_last_run=False, stamps=True):
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    ref = SR.walk(t, dist_max, min_members, close_last_run)
    assert ref["margin"] >= 1e-6 or dist_max == 0.0, ref["margin"]  # (dist < 0 is false whatever the rounding)
    o = _opt(dist_max, min_members, int(close_last_run))
    got = sv.debug_station_walk(t, o)
    assert (got["n_stations"], got["n_runs"]) == (len(ref["first"]), ref["n_runs"])
    for k in ("first", "last", "members"):
        assert np.array_equal(got[k], ref[k]), (k, got[k][:8], ref[k][:8])
    if stamps:
        n = t.shape[0]
        ps = 100.0 + np.arange(n) / 30.0
        q = np.tile([1.0, 0, 0, 0], (n, 1))
        a = sv.static_poses(ps, q, t, o)
        assert a["n_stations"] == len(ref["first"]) and np.array_equal(a["first"], ref["first"]) and np.array_equal(a["last"], ref["last"])
        assert np.array_equal(a["start_time"], ps[ref["first"]]) and np.array_equal(a["end_time"], ps[ref["last"]])
    return ref


@pytest.mark.parametrize("n", [0, 1, 2, 31, 63, 64, 65, 129, 1000])
def test_walk_equals_restatement(sv, n):
    t = dwell_walk(5, n)
    ref = check_walk(sv, t)
    check_walk(sv, t, min_members=0, stamps=False)
    check_walk(sv, t, close_last_run=True, stamps=False)
    if n == 1000:
        assert len(ref["first"]) >= 5 and ref["n_runs"] > len(ref["first"])


def _stations(lengths, breakers=1, tail=()):
    """Dwells of the given numbers of identical poses (each at its own place), `breakers` far poses behind each, then `tail`."""
    t = []
    for k, m in enumerate(lengths):
        t += [[float(k), 0.5 * k, -float(k)]] * m
        t += [list(FAR + 3.0 * (k + 1) * (i + 1)) for i in range(breakers)]
    return np.array(t + [list(p) for p in tail], dtype=np.float64).reshape(-1, 3)


def test_walk_member_counts_at_the_threshold(sv):
    ref = check_walk(sv, _stations([29, 30, 31]))  # 29 distinct poses: 30 members, no station
    assert ref["members"].tolist() == [31, 32] and ref["first"].tolist() == [30, 61] and ref["n_runs"] == 3
    ref = check_walk(sv, _stations([29, 30, 31]), min_members=29)
    assert ref["members"].tolist() == [30, 31, 32]


def test_walk_lane_and_chunk_edges(sv):
    # a breaker on lane 63 of the run's first chunk: the run is [0, 62], the next starts at pose 64
    ref = check_walk(sv, _stations([63, 40]))
    assert ref["first"].tolist() == [0, 64] and ref["last"].tolist() == [62, 103] and ref["members"].tolist() == [64, 41]
    # a breaker on lane 62: the next run starts on pose 63
    ref = check_walk(sv, _stations([62, 40]))
    assert ref["first"].tolist() == [0, 63]
    # breakers on lane 0 of a second and a third chunk; a run over many chunks with the sum carried from chunk to chunk
    check_walk(sv, _stations([64, 128, 33]))
    rng = np.random.default_rng(3)
    t = np.concatenate([np.array([0.3, -0.2, 1.1]) + rng.normal(0, 0.0002, (700, 3)), FAR[None], np.zeros((40, 3)), FAR[None]])
    ref = check_walk(sv, t)
    assert ref["members"].tolist() == [701, 41]


def test_walk_breakers_and_ends(sv):
    ref = check_walk(sv, _stations([35, 35], breakers=2))  # two in a row: the second is a run of its own, closed by (and eating) the next pose
    assert ref["first"].tolist() == [0, 38] and ref["members"].tolist() == [36, 35] and ref["n_runs"] == 3
    ref = check_walk(sv, _stations([35, 35], breakers=2), min_members=1)
    assert ref["members"].tolist() == [36, 2, 35]
    t = _stations([35])  # a breaker as the last pose
    assert check_walk(sv, t)["first"].tolist() == [0]
    assert check_walk(sv, t, close_last_run=True)["n_runs"] == 1
    t = _stations([35], tail=[[9.0, 9.0, 9.0]] * 40)  # an open run at the end: dropped, or kept
    assert check_walk(sv, t)["first"].tolist() == [0]
    ref = check_walk(sv, t, close_last_run=True)
    assert ref["first"].tolist() == [0, 36] and ref["last"].tolist() == [34, 75] and ref["members"].tolist() == [36, 41] and ref["n_runs"] == 2
    t = np.zeros((100, 3))  # nothing but one open run
    assert check_walk(sv, t)["n_runs"] == 0
    assert check_walk(sv, t, close_last_run=True)["members"].tolist() == [101]


def test_walk_constant_drift(sv):
    t = np.zeros((400, 3))
    t[:, 0] = 0.000053 * np.arange(400)  # the running centre follows: runs of 74 poses where a fixed centre gives 37
    ref = check_walk(sv, t)
    assert ref["members"][0] == 75 and len(ref["first"]) == 5


def test_walk_nan_translations(sv):
    t = _stations([40, 40, 80])
    t[41, 1] = np.nan   # at a run's start: a run of one member, the next run starts behind it
    t[120] = np.nan     # inside a run: closes it, the next run starts behind it
    ref = check_walk(sv, t)
    assert ref["first"].tolist() == [0, 42, 82, 121] and ref["last"].tolist() == [39, 80, 119, 161]
    ref = check_walk(sv, t, min_members=0)
    assert ref["members"][1] == 1 and ref["first"][1] == ref["last"][1] == 41
    t = np.full((70, 3), np.nan)
    assert check_walk(sv, t)["n_runs"] == 70


def test_walk_options(sv):
    t = dwell_walk(9, 600)
    for dist_max, min_members in ((0.0005, 30), (0.0011, 5), (0.01, 0), (0.0, 0), (0.002, 200)):
        check_walk(sv, t, dist_max, min_members)
    ref = check_walk(sv, _stations([5, 7]), dist_max=0.0, min_members=0, stamps=False)  # every pose a run of one member
    assert ref["members"].tolist() == [1] * 14
    for bad in (_opt(dist_max=-1.0), _opt(dist_max=np.nan), _opt(dist_max=np.inf), _opt(min_members=-1)):
        with pytest.raises(clc.ClcError) as e:
            sv.static_poses(None, np.zeros((3, 4)), np.zeros((3, 3)), bad)
        assert e.value.code == -1


# ---- the average --------------------------------------------------------------------------------------------------------------------
def posed_walk(seed, n, flip=False):
    """dwell_walk with orientations: one per dwell (re-drawn at every pose that moved) plus 2 mrad of noise."""
    t = dwell_walk(seed, n)
    rng = np.random.default_rng([seed, 77])
    ang, q = rng.uniform(-1.0, 1.0, 3), np.empty((n, 4))
    for i in range(n):
        if i and np.linalg.norm(t[i] - t[i - 1]) > 0.01:
            ang = rng.uniform(-1.0, 1.0, 3)
        a = ang + rng.normal(0, 0.002, 3)
        q[i] = sd.rot_to_quat_wxyz(sd.rot_zyx(a[0], a[1], a[2])[0]).reshape(4)
    if flip:
        q[1::2] *= -1.0
    return 100.0 + np.arange(n) / 30.0, q, t


def check_average(got, ps, q, t, ref_w, ref_a=None):
    a = ref_a or SR.average(ps, q, t, ref_w)
    assert got["n_stations"] == len(ref_w["first"]) and np.array_equal(got["status"], a["status"])
    assert np.array_equal(got["start_time"], a["start_time"]) and np.array_equal(got["end_time"], a["end_time"])
    for k in range(len(ref_w["first"])):
        if a["status"][k] != SR.STATION_OK:
            assert got["q"][k].tolist() == [1.0, 0.0, 0.0, 0.0] and got["t"][k].tolist() == [0.0, 0.0, 0.0]
            continue
        idx = SR.member_list(ref_w["first"][k], ref_w["members"][k])
        bound_t = 4 * len(idx) * EPS * np.abs(t[idx]).max()  # a reordered n-term sum
        assert np.abs(got["t"][k] - a["t"][k]).max() <= bound_t, (k, np.abs(got["t"][k] - a["t"][k]).max(), bound_t)
        assert a["gap"][k] >= 0.5
        dq = min(np.abs(got["q"][k] - a["q"][k]).max(), np.abs(got["q"][k] + a["q"][k]).max())
        assert dq <= 1e-12, (k, dq)
        assert got["q"][k][0] >= 0 and abs(np.linalg.norm(got["q"][k]) - 1.0) <= 8 * EPS  # 4 eps relative = 8 * 2^-53
    return a


def test_average_equals_restatement_and_sign_flips_change_nothing(sv):
    ps, q, t = posed_walk(5, 1000)
    w = SR.walk(t)
    assert w["margin"] >= 1e-6 and len(w["first"]) >= 5
    got = sv.static_poses(ps, q, t)
    a = check_average(got, ps, q, t, w)
    again = sv.static_poses(ps, q, t)
    assert all(np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes() for k in got)  # a second call: the same bits
    _, qf, _ = posed_walk(5, 1000, flip=True)
    flipped = sv.static_poses(ps, qf, t)
    check_average(flipped, ps, q, t, w, a)  # against the restatement of the UNFLIPPED poses
    no_stamp = sv.static_poses(None, q, t)
    assert not no_stamp["start_time"].any() and not no_stamp["end_time"].any() and no_stamp["q"].tobytes() == got["q"].tobytes()


def test_average_of_a_long_station(sv):
    rng = np.random.default_rng(11)
    n = 5000
    t = np.concatenate([np.array([1.5, -0.7, 2.2]) + rng.normal(0, 0.0002, (n, 3)), FAR[None]])
    a0 = np.array([0.4, -0.3, 0.8])
    ang = a0 + rng.normal(0, 0.002, (n + 1, 3))
    q = sd.rot_to_quat_wxyz(sd.rot_zyx(ang[:, 0], ang[:, 1], ang[:, 2])).reshape(n + 1, 4)
    ps = np.arange(n + 1) * 0.01
    w = SR.walk(t)
    assert w["margin"] >= 1e-6 and w["members"].tolist() == [n + 1]
    check_average(sv.static_poses(ps, q, t), ps, q, t, w)


def test_average_nonfinite_station(sv):
    ps, q, t = posed_walk(6, 300)
    w = SR.walk(t)
    assert len(w["first"]) >= 2
    q = q.copy()
    q[w["first"][1] + 3, 2] = np.nan
    got = sv.static_poses(ps, q, t)
    a = check_average(got, ps, q, t, w)
    assert a["status"][1] == SR.STATION_NONFINITE and got["status"][1] == clc._capi.STATION_NONFINITE and got["status"][0] == clc._capi.STATION_OK


def test_frozen_reference_output(sv):
    with open(os.path.join(ROOT, "tests", "golden", "static_poses_ref.json")) as f:
        G = json.load(f)
    ps, q, t = np.array(G["pose_stamp"]), np.array(G["q_wc"]), np.array(G["t_wc"])
    ref = {k: np.array(v) for k, v in G["ref"].items()}
    walk = sv.debug_station_walk(t)
    assert np.array_equal(walk["members"], ref["members"])
    got = sv.static_poses(ps, q, t)
    assert np.array_equal(got["first"], ref["first"]) and np.array_equal(got["last"], ref["last"])
    assert np.array_equal(got["start_time"], ref["start_time"]) and np.array_equal(got["end_time"], ref["end_time"])
    for k in range(len(ref["first"])):
        idx = SR.member_list(ref["first"][k], ref["members"][k])
        assert np.abs(got["t"][k] - ref["t"][k]).max() <= 4 * len(idx) * EPS * np.abs(t[idx]).max()
        assert min(np.abs(got["q"][k] - ref["q"][k]).max(), np.abs(got["q"][k] + ref["q"][k]).max()) <= 1e-12
        assert got["q"][k][0] > 0


def test_cap_stations_contract(sv):
    ps, q, t = posed_walk(5, 1000)
    full = sv.static_poses(ps, q, t)
    n = full["n_stations"]
    assert n >= 5
    assert sv.static_poses(ps, q, t, cap_stations=0)["n_stations"] == n  # the count query
    L, h, o = sv._L, sv._h, clc.default_station_options()
    import ctypes as C
    cnt = C.c_int64(-1)
    assert L.clc_static_poses(h, None, len(ps), ps.ctypes.data, q.ctypes.data, t.ctypes.data, 0, None, None, None, None, None, None, None, C.byref(cnt)) == 0
    assert cnt.value == n
    first = np.full(n, -7, np.int64); tq = np.full((n, 4), -7.0); st = np.full(n, -7, np.int32)
    assert L.clc_static_poses(h, C.byref(o), len(ps), ps.ctypes.data, q.ctypes.data, t.ctypes.data, 2, first.ctypes.data, None, None, None,
                              tq.ctypes.data, None, st.ctypes.data, C.byref(cnt)) == 0
    assert cnt.value == n and np.array_equal(first[:2], full["first"][:2]) and (first[2:] == -7).all()  # a short cap: `cap` rows and no more
    assert tq[:2].tobytes() == full["q"][:2].tobytes() and (tq[2:] == -7.0).all() and (st[2:] == -7).all() and (st[:2] == 1).all()
    assert L.clc_static_poses(h, None, 0, None, None, None, 0, None, None, None, None, None, None, None, C.byref(cnt)) == 0 and cnt.value == 0
    assert L.clc_static_poses(h, None, 5, None, None, None, 0, None, None, None, None, None, None, None, C.byref(cnt)) == -1
    assert L.clc_static_poses(None, None, 0, None, None, None, 0, None, None, None, None, None, None, None, None) == -1


# ---- assembly -----------------------------------------------------------------------------------------------------------------------
def station_poses(n_st, length=35, seed=2):
    """n_st stations of `length` poses (0.2 mm of jitter, an orientation each) with one breaker behind each; stamps 0, 1, 2, ..."""
    rng = np.random.default_rng(seed)
    t, q = [], []
    for k in range(n_st):
        c, ang = rng.uniform(-1, 1, 3), rng.uniform(-0.8, 0.8, 3)
        for _ in range(length):
            a = ang + rng.normal(0, 0.002, 3)
            t.append(c + rng.normal(0, 0.0002, 3)); q.append(sd.rot_to_quat_wxyz(sd.rot_zyx(a[0], a[1], a[2])[0]).reshape(4))
        t.append(FAR + k); q.append(np.array([1.0, 0, 0, 0]))
    t, q = np.array(t), np.array(q)
    return np.arange(len(t), dtype=np.float64), q, t


def check_against(sv, front, ps, q, t, scans, scan_stamp, opt=None):
    o = opt or clc.default_station_options()
    info, ss = sv.assemble_stations(ps, q, t, scans, scan_stamp, o)
    P, seg, status = front
    w = SR.walk(t, o.center_dist_max, o.min_members, bool(o.close_last_run))
    assert w["margin"] >= 1e-6
    a = SR.average(ps, q, t, w)
    ss_ref = SR.associate(a["start_time"], a["end_time"], a["status"], status, scan_stamp)
    assert np.array_equal(ss, ss_ref), np.nonzero(ss != ss_ref)[0][:8]
    off = scans["offsets"]
    kept = np.nonzero(ss_ref >= 0)[0]
    rows = [P[off[s] + seg[s, 0]: off[s] + seg[s, 1] + 1] for s in kept]
    pts_off = np.zeros(len(kept) + 1, dtype=np.int64)
    pts_off[1:] = np.cumsum([len(r) for r in rows])
    got = sv.stored_observations()
    assert np.array_equal(got.pts_off, pts_off)
    assert got.pts.tobytes() == (np.concatenate(rows) if rows else np.zeros((0, 3))).tobytes()  # a copy
    assert np.array_equal(np.diff(got.ptl_off), np.where(np.diff(pts_off) >= 2, 2, 0))
    assert [getattr(info, f[0]) for f in info._fields_] == \
        [w["n_runs"], len(w["first"]), int((a["status"] == SR.STATION_NONFINITE).sum()), int((status == 1).sum()), int((status == -1).sum()),
         int((ss_ref == SR.NO_POSE).sum()), len(kept), int(pts_off[-1]), int(got.ptl_off[-1])]
    assert info.n_observations == info.n_segments - info.n_unmatched
    if len(kept):
        avg = sv.static_poses(ps, q, t, o)  # the device's own averaged poses: the gather's arithmetic alone
        tp = [R.tag_pose(avg["q"][ss_ref[s]], avg["t"][ss_ref[s]]) for s in kept]
        assert np.abs(got.tag_q - np.array([x for x, _ in tp])).max() <= 1e-14 and np.abs(got.tag_t - np.array([y for _, y in tp])).max() <= 1e-14
    return info, ss, got, a


def _bytes(S):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (S.tag_q, S.tag_t, S.pts_off, S.pts, S.ptl_off, S.ptl))


def test_assembly_stamp_cases(sv, base_scans, front):
    ps, q, t = station_poses(4)  # stations [0, 34], [36, 70], [72, 106], [108, 142]
    S = 64
    ss = np.full(S, 1000.0)
    ss[0:8] = [0.0, 34.0, np.nextafter(0.0, -1.0), np.nextafter(34.0, 100.0), 36.0, 70.0, np.nextafter(36.0, 0.0), np.nextafter(70.0, 100.0)]
    ss[8:40] = np.linspace(72.5, 106.5, 32)   # station 2; station 3 takes no scan
    ss[40:48] = [35.0, 71.0, 107.0, np.nan, -5.0, 143.0, 17.25, 53.5]
    info, got_ss, got, a = check_against(sv, front, ps, q, t, base_scans, ss)
    st = front[2]
    want = {0: 0, 1: 0, 2: SR.NO_POSE, 3: SR.NO_POSE, 4: 1, 5: 1, 6: SR.NO_POSE, 7: SR.NO_POSE, 43: SR.NO_POSE, 46: 0, 47: 1}
    for s, v in want.items():
        if st[s] == 1:
            assert got_ss[s] == v, (s, got_ss[s], v)
    assert (st[:8] == 1).sum() >= 4  # (the ends are really looked at)
    assert info.n_stations == 4 and info.n_observations > 0 and 3 not in got_ss.tolist() and 2 in got_ss.tolist()


def test_assembly_no_station_and_no_scans(sv, base_scans, front):
    n = 50
    q = np.tile([1.0, 0, 0, 0], (n, 1)); t = np.zeros((n, 3)); t[:, 0] = np.arange(n)  # a metre apart: no station
    gen = sv.store_generation
    info, ss, got, _ = check_against(sv, front, np.arange(n, dtype=np.float64), q, t, base_scans, np.full(64, 3.0))
    assert info.n_stations == 0 and info.n_runs == 25 and info.n_observations == 0 and info.n_unmatched == info.n_segments > 0
    assert got.n_poses == 0 and got.pts.shape == (0, 3) and sv.store_generation == gen + 1
    info, ss = sv.assemble_stations(np.zeros(0), np.zeros((0, 4)), np.zeros((0, 3)), base_scans, np.full(64, 3.0))  # no poses at all
    assert info.n_runs == 0 and info.n_stations == 0 and info.n_observations == 0 and (ss < 0).all()
    none = {"ranges": np.zeros(0, np.float32), "offsets": np.zeros(1, np.int64), "angle_min": np.zeros(0, np.float32),
            "angle_increment": np.zeros(0, np.float32), "range_min": np.zeros(0, np.float32)}
    ps, q, t = station_poses(3)
    info, ss = sv.assemble_stations(ps, q, t, none, np.zeros(0))  # no scans at all
    assert info.n_stations == 3 and info.n_runs == 3 and info.n_observations == 0 and ss.shape == (0,)


def test_assembly_unsorted_stations_and_a_nonfinite_one(sv, base_scans, front):
    ps, q, t = station_poses(4)
    ps = (3 - np.arange(len(ps)) // 36) * 100.0 + np.arange(len(ps)) % 36  # start times 300, 200, 100, 0: the linear walk
    ss = np.concatenate([np.linspace(299.0, 336.0, 16), np.linspace(-1.0, 36.0, 16), np.linspace(100.0, 234.0, 32)])
    info, got_ss, got, a = check_against(sv, front, ps, q, t, base_scans, ss)
    assert a["start_time"].tolist() == [300.0, 200.0, 100.0, 0.0] and set(got_ss[got_ss >= 0].tolist()) == {0, 1, 2, 3}
    # overlapping intervals (equal stamps): the first station in station order
    ps2 = np.arange(len(ps)) % 36 + 0.0
    info, got_ss, _, _ = check_against(sv, front, ps2, q, t, base_scans, np.linspace(-1.0, 36.0, 64))
    assert set(got_ss[got_ss >= 0].tolist()) == {0}
    # a NaN quaternion inside station 1: CLC_STATION_NONFINITE, its scans get CLC_SCAN_NO_POSE (sorted stamps: the binary search)
    ps, q, t = station_poses(4)
    q = q.copy(); q[50, 0] = np.nan
    ss = np.linspace(0.5, 141.5, 64)
    info, got_ss, _, a = check_against(sv, front, ps, q, t, base_scans, ss)
    assert info.n_nonfinite == 1 and a["status"].tolist() == [1, -1, 1, 1] and 1 not in got_ss.tolist()
    inside = (ss >= 36.0) & (ss <= 70.0) & (front[2] == 1)
    assert inside.any() and (got_ss[inside] == SR.NO_POSE).all()


def test_assembly_host_form_device_form_second_run_and_keyframe_mode_untouched(sv, base_scans, front):
    import torch
    ps, q, t = station_poses(4)
    ss = np.linspace(-2.0, 145.0, 64)
    kq = np.tile([1.0, 0, 0, 0], (6, 1)); kt = np.zeros((6, 3)); kt[:, 0] = np.arange(6); kps = np.arange(6) * 25.0
    kss = kps[np.arange(64) % 6] + 0.004
    ki, ksp = sv.assemble_observations(kps, kq, kt, base_scans, kss)  # the key-frame mode before ...
    before = _bytes(sv.stored_observations())
    assert ki.n_observations > 0
    info, got_ss, got, _ = check_against(sv, front, ps, q, t, base_scans, ss)
    assert info.n_observations >= 20
    sc = base_scans
    S, n = 64, int(sc["offsets"][-1])
    d = [_dev(a) for a in (ps, q, t, sc["ranges"], sc["offsets"], sc["angle_min"], sc["angle_increment"], sc["range_min"], ss)]
    d_ss = torch.full((S,), 7, dtype=torch.int32, device=d[0].device)
    torch.cuda.synchronize()
    for _ in range(2):  # the device form, twice: the same bits as the host form
        i2 = sv.assemble_stations_device(len(ps), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), S, n,
                                         d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr(), d_ss.data_ptr())
        assert [getattr(i2, f[0]) for f in i2._fields_] == [getattr(info, f[0]) for f in info._fields_]
        assert np.array_equal(d_ss.cpu().numpy(), got_ss)
        assert _bytes(sv.stored_observations()) == _bytes(got)
    i3 = sv.assemble_stations_device(len(ps), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), S, n,
                                     d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr(), 0)  # scan_station nullable
    assert i3.n_observations == info.n_observations
    ki2, ksp2 = sv.assemble_observations(kps, kq, kt, base_scans, kss)  # ... and after: the same bits
    assert np.array_equal(ksp, ksp2) and _bytes(sv.stored_observations()) == before
    assert [getattr(ki2, f[0]) for f in ki2._fields_] == [getattr(ki, f[0]) for f in ki._fields_]


def test_assembly_bad_arguments(sv, base_scans):
    ps, q, t = station_poses(1)
    bad = dict(base_scans); bad["offsets"] = base_scans["offsets"].copy(); bad["offsets"][2] = 5
    with pytest.raises(clc.ClcError) as e:
        sv.assemble_stations(ps, q, t, bad, np.ones(64))
    assert e.value.code == -1
    for o in (_opt(dist_max=-0.001), _opt(dist_max=np.nan), _opt(min_members=-2)):
        with pytest.raises(clc.ClcError) as e:
            sv.assemble_stations(ps, q, t, base_scans, np.ones(64), o)
        assert e.value.code == -1
    o = _opt(); o.line.max_num_iterations = -1
    with pytest.raises(clc.ClcError):
        sv.assemble_stations(ps, q, t, base_scans, np.ones(64), o)
    L = sv._L
    assert L.clc_assemble_stations(sv._h, None, 2, None, None, None, None, None, 0, None, None, None, None, None, None) == -1
    assert L.clc_assemble_stations_device(None, None, 0, None, None, None, None, None, 0, 0, None, None, None, None, None, None) == -1


# ---- the flow -----------------------------------------------------------------------------------------------------------------------
def test_calibrate_offline_stations_matches_the_oracle_on_the_restated_records(sv, oracle_mod):
    rec = so.station_recording(1)
    ps, q, t, scans, ss = rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"]
    # the restated records: CPU scan points and segments, the restatement's stations, the oracle's line fits
    w = SR.walk(t)
    a = SR.average(ps, q, t, w)
    assert np.array_equal(w["first"], rec["station_first"]) and len(w["first"]) >= 10
    off = scans["offsets"]
    P = R.scan_points(scans, oracle_mod)
    seg, status = BS.board_segments(P, off)
    ss_ref = SR.associate(a["start_time"], a["end_time"], a["status"], status, ss)
    tq, tt, pts, ptl = [], [], [], []
    for s in np.nonzero(ss_ref >= 0)[0]:
        pp = P[off[s] + seg[s, 0]: off[s] + seg[s, 1] + 1]
        qi, ti = R.tag_pose(a["q"][ss_ref[s]], a["t"][ss_ref[s]])
        tq.append(qi); tt.append(ti); pts.append(pp); ptl.append(R.end_points(pp, oracle_mod.line_fit(pp[:, :2], (0.0, 0.0)).pose))
    n = len(pts)
    pts_off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64)
    ptl_off = np.concatenate([[0], np.cumsum([len(p) for p in ptl])]).astype(np.int64)
    obs = sd.ObservationSet(np.array(tq), np.array(tt), pts_off, np.ascontiguousarray(np.concatenate(pts)), ptl_off,
                            np.ascontiguousarray(np.concatenate(ptl)))
    Tlc0, _, _ = oracle_mod.closed_form(oracle_mod.flatten(obs, True, False))
    ref = oracle_mod.solve(oracle_mod.flatten(obs, False, False), sd.pose7_from_T(np.linalg.inv(Tlc0)))

    out = clc.CalibrateOfflineStations(ps, q, t, scans, ss, solver=sv, verbose=False)
    assert out is not None and np.array_equal(out["scan_station"], ss_ref) and out["info"].n_observations == n
    assert out["info"].n_stations == len(w["first"]) and out["info"].n_runs == w["n_runs"]
    dT = np.abs(out["Tcl"] - sd.T_from_pose7(ref.pose)).max()
    dc = abs(out["report"].result.summary.final_cost - ref.summary.final_cost)
    print(f"|dTcl| = {dT:.2e}, |dcost| = {dc:.2e}, iterations {out['report'].result.summary.num_iterations} / {ref.summary.num_iterations}")
    assert dT <= 1e-6 and dc <= 1e-8 and out["report"].result.summary.num_iterations == ref.summary.num_iterations
    assert np.abs(out["Tlc_initial"] - Tlc0).max() <= 1e-6
    # the reference's gates
    assert clc.CalibrateOfflineStations(ps[:9], q[:9], t[:9], scans, ss, solver=sv, verbose=False) is None
    assert clc.CalibrateOfflineStations(ps, q, t, scans, ss + 500.0, solver=sv, verbose=False) is None

    # the stations as resampling blocks
    out = clc.CalibrateOfflineStations(ps, q, t, scans, ss, solver=sv, verbose=False)
    blocks, ids = out["station_block_offsets"], out["station_block_ids"]
    kept = ss_ref[ss_ref >= 0]
    assert blocks is not None and blocks[0] == 0 and blocks[-1] == n and len(blocks) == len(ids) + 1 >= 10
    assert all((kept[blocks[b]:blocks[b + 1]] == ids[b]).all() for b in range(len(ids)))
    # (clc_solve_subsets wants a problem one workgroup holds: the points_on_line records, two per observation)
    stored = sv.stored_observations()
    T0 = np.linalg.inv(out["Tlc_initial"])
    Tp = T0.copy()
    plain = clc.CamLaserCalibration(stored, Tp, True, False, solver=sv, verbose=False)  # the plain solve of the same records
    T = T0.copy()
    rs = clc.CamLaserCalibrationResample(stored, T, True, False, mode="jackknife", solver=sv, block_offsets=blocks)
    B = len(ids)
    assert rs["weights"].shape == (B, B) and rs["poses"].shape == (B, 7) and rs["influence"].shape == (B,) and np.isfinite(rs["poses"]).all()
    assert np.abs(T - Tp).max() <= 1e-6 and abs(rs["summary"].final_cost - plain.result.summary.final_cost) <= 1e-8
    rec_off = calib._group_blocks(calib.pose_block_offsets(stored, True, False), blocks)
    assert rec_off[-1] == 2 * n and len(rec_off) == B + 1
    ones, sms = sv.solve_subsets(rec_off, np.ones((1, B), dtype=np.uint8), sd.pose7_from_T(T0))  # the all-ones row: the plain solve
    assert np.abs(sd.T_from_pose7(ones[0]) - Tp).max() <= 1e-6
    assert abs(sms[0].final_cost - plain.result.summary.final_cost) <= 1e-8 and sms[0].num_iterations == plain.result.summary.num_iterations
    shuffled = out["scan_station"].copy(); shuffled[:] = shuffled[::-1]
    assert calib.station_block_offsets(shuffled) == (None, None)
