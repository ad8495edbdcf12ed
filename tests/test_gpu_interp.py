"""clc_interpolate_poses / clc_assemble_interpolated(_device) / clc_clock_offset_sweep (K15) on the GPU against the restatement
tests/interp_ref.py: brackets exactly, u within 4 eps, quaternions within 1e-12, translations within 4 eps max|t|; scan -> bracket
indices, counts and offsets exactly, the stored points bit for bit; host form == device form == a second run; key-frame and station
mode untouched; the sweep's records against oracle.flatten of the restated decimated sets within 1e-12; every problem of the sweep,
the chosen offset and CalibrateOfflineInterpolated against the oracle on the restated records."""
import math

import numpy as np
import pytest

import board_segment_ref as BS
import interp_ref as IR
import offline_ref as R
import camlasercalibratool_amd as clc
from camlasercalibratool_amd import simdata as sd, simoffline as so

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def sv():
    s = clc.Solver(0)
    yield s
    s.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def device_front(sv, scans):
    """TranScanToPoints + board segments on the device -> (points [M, 3], seg [S, 2], status [S])."""
    import torch
    off = np.ascontiguousarray(scans["offsets"], dtype=np.int64)
    S, n = len(off) - 1, int(off[-1])
    if S == 0:
        return np.zeros((0, 3)), np.zeros((0, 2), np.int64), np.zeros(0, np.int32)
    d_r, d_off, d_am, d_ai, d_rm = _dev(scans["ranges"]), _dev(off), _dev(scans["angle_min"]), _dev(scans["angle_increment"]), _dev(scans["range_min"])
    d_pts = torch.zeros((max(n, 1), 3), dtype=torch.float64, device=d_off.device)
    d_seg = torch.empty((S, 2), dtype=torch.int64, device=d_off.device)
    d_st = torch.empty((S,), dtype=torch.int32, device=d_off.device)
    torch.cuda.synchronize()
    sv.scan_to_points_device(d_r.data_ptr(), d_off.data_ptr(), S, n, d_am.data_ptr(), d_ai.data_ptr(), d_rm.data_ptr(), d_pts.data_ptr())
    sv.board_segments_device(d_pts.data_ptr(), d_off.data_ptr(), S, d_seg.data_ptr(), d_st.data_ptr())
    return d_pts.cpu().numpy()[:n], d_seg.cpu().numpy(), d_st.cpu().numpy()


_FRONTS = {}


def scans_and_front(sv, S, seed=7):
    """S scans of 1 081 rays and the device's own points, segments and statuses of them (computed once per size)."""
    if (S, seed) not in _FRONTS:
        scans = sd.sim_laser_scans(seed, S) if S > 0 else {"ranges": np.zeros(0, np.float32), "offsets": np.zeros(1, np.int64),
                                                          "angle_min": np.zeros(0, np.float32), "angle_increment": np.zeros(0, np.float32),
                                                          "range_min": np.zeros(0, np.float32)}
        _FRONTS[(S, seed)] = (scans, device_front(sv, scans))
    return _FRONTS[(S, seed)]


def _opt(time_offset=None, max_gap=None):
    o = clc.default_interp_options()
    if time_offset is not None:
        o.time_offset = time_offset
    if max_gap is not None:
        o.max_gap = max_gap
    return o


def random_poses(seed, n, rate=30.0):
    """n stamped poses on a smooth random path: stamps 100 + i / rate, orientations a few degrees apart."""
    rng = np.random.default_rng([seed, n])
    ang = np.cumsum(rng.normal(0, 0.03, (n, 3)), axis=0) + rng.uniform(-0.5, 0.5, 3)
    q = sd.rot_to_quat_wxyz(sd.rot_zyx(ang[:, 0], ang[:, 1], ang[:, 2])).reshape(n, 4) if n else np.zeros((0, 4))
    t = np.cumsum(rng.normal(0, 0.01, (n, 3)), axis=0) + rng.uniform(-1, 1, 3) if n else np.zeros((0, 3))
    return 100.0 + np.arange(n) / rate, q, t


def check_interp(sv, ps, q, t, x, time_offset=0.0, max_gap=IR.MAX_GAP):
    """clc_interpolate_poses against the restatement, at the issue's gates -> (device result, restatement)."""
    got = sv.interpolate_poses(ps, q, t, x, _opt(time_offset, max_gap))
    ref = IR.interpolate(ps, q, t, x, time_offset, max_gap)
    assert np.array_equal(got["bracket"], ref["bracket"]), np.nonzero(got["bracket"] != ref["bracket"])[0][:8]
    assert got["u"].shape == ref["u"].shape and (np.abs(got["u"] - ref["u"]).max() if len(x) else 0.0) <= 4 * EPS
    ok = ref["bracket"] >= 0
    if ok.any():
        dq = np.abs(got["q"][ok] - ref["q"][ok]).max()
        tmax = np.abs(np.asarray(t)[np.isfinite(np.asarray(t))]).max()
        dt = np.abs(got["t"][ok] - ref["t"][ok]).max()
        assert dq <= 1e-12 and dt <= 4 * EPS * tmax, (dq, dt)
        assert np.abs(np.linalg.norm(got["q"][ok], axis=1) - 1.0).max() <= 8 * EPS
    if (~ok).any():  # no pose: u = 0, q = (1, 0, 0, 0), t = 0
        assert not got["u"][~ok].any() and not got["t"][~ok].any() and (got["q"][~ok] == [1.0, 0.0, 0.0, 0.0]).all()
    return got, ref


# ---- clc_interpolate_poses ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 64, 65, 130])
def test_interpolate_poses_equals_restatement(sv, n):
    ps, q, t = random_poses(3, n)
    rng = np.random.default_rng([9, n])
    lo, hi = (ps[0], ps[-1]) if n else (100.0, 101.0)
    x = np.concatenate([[lo - 0.01, hi + 0.01, lo - 1e-9, np.nextafter(hi, 1e9), np.nan], ps[:: max(n // 9, 1)], ps[-1:],   # outside, ON stamps
                        rng.uniform(lo - 0.05, hi + 0.05, 150)])
    got, ref = check_interp(sv, ps, q, t, x)
    if n >= 2:
        assert got["bracket"][0] == got["bracket"][1] == got["bracket"][4] == IR.NO_POSE
        assert ref["bracket"].max() == n - 2 and (n < 64 or (ref["bracket"] >= 0).sum() >= 100)
        on = 5 + len(ps[:: max(n // 9, 1)])
        assert got["bracket"][5] == 0 and got["u"][5] == 0.0          # on the first stamp: the first pair, u = 0
        assert got["bracket"][on] == n - 2 and got["u"][on] == 1.0    # on the last stamp: the last pair, u = 1
        if n >= 3:  # on an inner stamp: the pair that ENDS there (the first in file order), u = 1
            k = max(n // 9, 1)
            assert got["bracket"][6] == k - 1 and got["u"][6] == 1.0
        assert np.abs(got["q"][5] - q[0]).max() <= 1e-15 and np.array_equal(got["t"][5], t[0])
    else:
        assert (got["bracket"] == IR.NO_POSE).all()
    check_interp(sv, ps, q, t, x, time_offset=0.0123)
    check_interp(sv, ps, q, t, x, time_offset=-0.007, max_gap=1.0)
    check_interp(sv, ps, q, t, x, max_gap=0.03)  # every gap of 1/30 s is too long
    assert n < 2 or (sv.interpolate_poses(ps, q, t, x, _opt(max_gap=0.03))["bracket"] == IR.NO_POSE).all()
    again = sv.interpolate_poses(ps, q, t, x)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)  # a second call: the same bits


def test_interpolate_gaps_repeated_stamps_and_nans(sv):
    ps, q, t = random_poses(4, 80)
    ps = ps.copy()
    MG = 0.15                         # (the three equal stamps leave a gap of 0.1 s behind them: max_gap well clear of it)
    ps[30:] += 0.5                    # a gap of 0.533 s > max_gap between poses 29 and 30
    ps[51] = ps[50]; ps[52] = ps[50]  # three equal stamps: pairs 50 and 51 have a zero-length gap
    x = np.array([ps[29] + 0.2, ps[29], ps[30], ps[50], ps[50] - 0.01, ps[50] + 0.01, np.nextafter(ps[50], 0.0), np.nextafter(ps[50], 1e9),
                  ps[49], ps[53], np.nan, np.inf, -np.inf])
    got, ref = check_interp(sv, ps, q, t, x, max_gap=MG)
    assert got["bracket"].tolist() == [IR.NO_POSE, 28, 30, 49, 49, 52, 49, 52, 48, 52, IR.NO_POSE, IR.NO_POSE, IR.NO_POSE]
    assert got["u"][3] == 1.0 and got["u"][2] == 0.0
    got, _ = check_interp(sv, ps, q, t, x, max_gap=1.0)  # the long gap is interpolated across now
    assert got["bracket"][0] == 29
    dense = np.linspace(ps[0] - 0.1, ps[-1] + 0.1, 700)
    check_interp(sv, ps, q, t, dense, max_gap=MG)
    check_interp(sv, ps, q, t, np.concatenate([ps, ps + 1e-12, ps - 1e-12]), max_gap=MG)
    # a NaN pose inside a bracket: sorted stamps (the bisection), the two pairs that hold it give no pose
    qn = q.copy(); qn[10, 2] = np.nan
    tn = t.copy(); tn[20, 0] = np.nan
    qz = qn.copy(); qz[40] = 0.0     # a zero quaternion
    x = np.array([ps[9] + 0.01, ps[10] + 0.01, ps[11] + 0.01, ps[19] + 0.01, ps[20] + 0.01, ps[21] + 0.01, ps[39] + 0.01, ps[40] + 0.01, ps[41] + 0.01])
    got, _ = check_interp(sv, ps, qz, tn, x, max_gap=MG)
    assert got["bracket"].tolist() == [IR.NO_POSE, IR.NO_POSE, 11, IR.NO_POSE, IR.NO_POSE, 21, IR.NO_POSE, IR.NO_POSE, 41]
    # a NaN stamp: the list counts as unsorted (the linear walk); the pairs that hold it bracket nothing
    pn = ps.copy(); pn[60] = np.nan
    got, _ = check_interp(sv, pn, q, t, np.concatenate([dense, [ps[59] + 0.01, ps[60] + 0.01, ps[61] + 0.01]]), max_gap=MG)
    assert got["bracket"][-3:].tolist() == [IR.NO_POSE, IR.NO_POSE, 61]
    pi = ps.copy(); pi[-1] = np.inf  # an infinite last stamp: still sorted, its pair is no candidate
    got, _ = check_interp(sv, pi, q, t, np.array([ps[-2] + 0.01, ps[-3] + 0.01, np.inf]), max_gap=MG)
    assert got["bracket"].tolist() == [IR.NO_POSE, len(ps) - 3, IR.NO_POSE]


def test_interpolate_unsorted_stamps_take_the_linear_walk(sv):
    ps, q, t = random_poses(5, 130)
    blocks = [np.arange(65, 130), np.arange(0, 65)]      # the second half of the recording first
    order = np.concatenate(blocks)
    pu, qu, tu = ps[order], q[order], t[order]
    x = np.concatenate([np.linspace(ps[0] - 0.05, ps[-1] + 0.05, 400), ps[::7]])
    got, ref = check_interp(sv, pu, qu, tu, x, max_gap=0.05)
    assert (got["bracket"] >= 0).sum() >= 350 and 64 not in got["bracket"].tolist()  # (the pair across the jump back brackets nothing)
    # the same poses sorted give the same interpolated poses
    srt = sv.interpolate_poses(ps, q, t, x, _opt(max_gap=0.05))
    both = (got["bracket"] >= 0) & (srt["bracket"] >= 0)
    assert both.sum() >= 350 and np.abs(got["q"][both] - srt["q"][both]).max() <= 1e-15 and np.abs(got["t"][both] - srt["t"][both]).max() <= 1e-15
    # overlapping spans: a stamp two pairs bracket goes to the first in file order
    po = np.array([0.0, 1.0, 2.0, 0.5, 1.5, 2.5]); qo = np.tile([1.0, 0, 0, 0], (6, 1)); to = np.arange(18.0).reshape(6, 3)
    got, _ = check_interp(sv, po, qo, to, np.array([0.75, 1.25, 2.25, 0.5, 2.5, 2.6]), max_gap=2.0)
    assert got["bracket"].tolist() == [0, 1, 4, 0, 4, IR.NO_POSE]
    # stamps that decrease everywhere: no pair has a positive gap
    got, _ = check_interp(sv, ps[::-1].copy(), q, t, x)
    assert (got["bracket"] == IR.NO_POSE).all()


def test_interpolate_quaternion_signs_and_the_nlerp_switch(sv):
    ps, q, t = random_poses(6, 65)
    x = np.linspace(ps[0], ps[-1], 333)
    base, _ = check_interp(sv, ps, q, t, x)
    qf = q.copy(); qf[1::2] *= -1.0       # every other stored quaternion with the other sign: dot < 0 in every pair
    flip, _ = check_interp(sv, ps, qf, t, x)
    d = np.minimum(np.abs(flip["q"] - base["q"]).max(axis=1), np.abs(flip["q"] + base["q"]).max(axis=1))
    assert d.max() <= 4 * EPS and np.array_equal(flip["t"], base["t"]) and np.array_equal(flip["bracket"], base["bracket"])
    qs = q * np.linspace(0.5, 2.0, 65)[:, None]  # stored quaternions need not be unit
    scaled, _ = check_interp(sv, ps, qs, t, x)
    assert np.abs(scaled["q"] - base["q"]).max() <= 8 * EPS
    # nearly equal neighbours: half angles on both sides of acos(1 - 1e-10) = 1.414e-5 rad, and equal ones
    n = 40
    rng = np.random.default_rng(8)
    half = np.concatenate([[0.0], math.sqrt(2e-10) * (1.0 + np.linspace(-0.5, 0.5, n - 1))])
    qq = np.empty((n + 1, 4)); qq[0] = q[0]
    for i in range(n):
        axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
        w1, (x1, y1, z1) = math.cos(half[i]), math.sin(half[i]) * axis
        w0, x0, y0, z0 = qq[i]
        qq[i + 1] = [w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1, w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1,
                     w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1]
        qq[i + 1] /= np.linalg.norm(qq[i + 1])
    dots = np.abs((qq[:-1] * qq[1:]).sum(axis=1))
    assert (dots > IR.NLERP_ABOVE).sum() >= 10 and (dots <= IR.NLERP_ABOVE).sum() >= 10  # both branches are taken
    pp = 100.0 + np.arange(n + 1) / 30.0
    tt = rng.uniform(-1, 1, (n + 1, 3))
    got, _ = check_interp(sv, pp, qq, tt, np.linspace(pp[0], pp[-1], 500))
    assert (got["bracket"] >= 0).all()


def test_interpolate_bad_arguments(sv):
    ps, q, t = random_poses(3, 5)
    for bad in (_opt(max_gap=0.0), _opt(max_gap=-1.0), _opt(max_gap=np.nan), _opt(max_gap=np.inf), _opt(time_offset=np.nan), _opt(time_offset=np.inf)):
        with pytest.raises(clc.ClcError) as e:
            sv.interpolate_poses(ps, q, t, ps, bad)
        assert e.value.code == -1
    L = sv._L
    assert L.clc_interpolate_poses(sv._h, None, 3, None, None, None, 0, None, None, None, None, None) == -1
    assert L.clc_interpolate_poses(sv._h, None, 0, None, None, None, 2, None, None, None, None, None) == -1
    assert L.clc_interpolate_poses(None, None, 0, None, None, None, 0, None, None, None, None, None) == -1
    assert L.clc_interpolate_poses(sv._h, None, 0, None, None, None, 0, None, None, None, None, None) == 0
    x = np.array([ps[1] + 0.01])
    br = np.zeros(1, np.int32)  # every output nullable
    assert L.clc_interpolate_poses(sv._h, None, 5, ps.ctypes.data, q.ctypes.data, t.ctypes.data, 1, x.ctypes.data, br.ctypes.data, None, None, None) == 0
    assert br[0] == 1
    assert L.clc_interpolate_poses(sv._h, None, 5, ps.ctypes.data, q.ctypes.data, t.ctypes.data, 1, x.ctypes.data, None, None, None, None) == 0


# ---- assembly -----------------------------------------------------------------------------------------------------------------------
def _bytes(S):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (S.tag_q, S.tag_t, S.pts_off, S.pts, S.ptl_off, S.ptl))


def _fields(info):
    return [getattr(info, f[0]) for f in info._fields_]


def check_assembly(sv, ps, q, t, scans, front, scan_stamp, opt=None):
    o = opt or clc.default_interp_options()
    info, sb, su = sv.assemble_interpolated(ps, q, t, scans, scan_stamp, o)
    P, seg, status = front
    ip = IR.interpolate(ps, q, t, scan_stamp, o.time_offset, o.max_gap)
    sb_ref = IR.associate(ip, status)
    assert np.array_equal(sb, sb_ref), np.nonzero(sb != sb_ref)[0][:8]
    kept = np.nonzero(sb_ref >= 0)[0]
    assert (np.abs(su[kept] - ip["u"][kept]).max() if len(kept) else 0.0) <= 4 * EPS and not su[sb_ref < 0].any()
    off = scans["offsets"]
    rows = [P[off[s] + seg[s, 0]: off[s] + seg[s, 1] + 1] for s in kept]
    pts_off = np.zeros(len(kept) + 1, dtype=np.int64)
    pts_off[1:] = np.cumsum([len(r) for r in rows])
    got = sv.stored_observations()
    assert np.array_equal(got.pts_off, pts_off)
    assert got.pts.tobytes() == (np.concatenate(rows) if rows else np.zeros((0, 3))).tobytes()  # a copy
    assert np.array_equal(np.diff(got.ptl_off), np.where(np.diff(pts_off) >= 2, 2, 0))
    assert _fields(info) == [IR.n_pairs(ps, o.max_gap), int((status == 1).sum()), int((status == -1).sum()), int((sb_ref == IR.NO_POSE).sum()),
                             len(kept), int(pts_off[-1]), int(got.ptl_off[-1])]
    assert info.n_observations == info.n_segments - info.n_unmatched
    if len(kept):
        # the interpolated poses: the device's own against the restatement at clc_interpolate_poses' gates, then the gather's
        # arithmetic (:145-146) alone on the device's own values
        dev, _ = check_interp(sv, ps, q, t, np.asarray(scan_stamp)[kept], o.time_offset, o.max_gap)
        tp = [R.tag_pose(dev["q"][k], dev["t"][k]) for k in range(len(kept))]
        assert np.abs(got.tag_q - np.array([a for a, _ in tp])).max() <= 1e-14 and np.abs(got.tag_t - np.array([b for _, b in tp])).max() <= 1e-14
    return info, sb, su, got


@pytest.mark.parametrize("S", [0, 1, 63, 64, 65, 1025])
def test_assembly_equals_restatement(sv, S):
    scans, front = scans_and_front(sv, S)
    ps, q, t = random_poses(11, 130)
    rng = np.random.default_rng([12, S])
    ss = rng.uniform(ps[0] - 0.2, ps[-1] + 0.2, S)  # some before the first and behind the last pose
    if S >= 63:
        ss[:6] = [ps[0], ps[-1], ps[17], np.nan, ps[0] - 1e-9, np.nextafter(ps[-1], 1e9)]
    gen = sv.store_generation
    info, sb, su, got = check_assembly(sv, ps, q, t, scans, front, ss)
    assert sv.store_generation == gen + 1
    if S >= 63:
        assert info.n_observations >= S // 3 and info.n_keyframes == 129
        st = front[2]
        for s, v in {0: 0, 1: 128, 2: 16, 3: IR.NO_POSE, 4: IR.NO_POSE, 5: IR.NO_POSE}.items():
            if st[s] == 1:
                assert sb[s] == v, (s, sb[s], v)
    if S == 0:
        assert info.n_observations == 0 and got.n_poses == 0 and sb.shape == (0,)
    check_assembly(sv, ps, q, t, scans, front, ss, _opt(time_offset=0.011))
    if S == 65:
        i2, sb2, _, got2 = check_assembly(sv, ps, q, t, scans, front, ss, _opt(max_gap=0.03))  # no pair can bracket
        assert i2.n_keyframes == 0 and i2.n_observations == 0 and i2.n_unmatched == i2.n_segments > 0 and got2.n_poses == 0
        i3, sb3, _ = sv.assemble_interpolated(np.zeros(0), np.zeros((0, 4)), np.zeros((0, 3)), scans, ss)  # no poses at all
        assert i3.n_keyframes == 0 and i3.n_observations == 0 and (sb3 < 0).all()
        order = np.concatenate([np.arange(65, 130), np.arange(0, 65)])  # unsorted poses: the linear walk
        check_assembly(sv, ps[order], q[order], t[order], scans, front, ss, _opt(max_gap=0.05))


def test_assembly_host_form_device_form_second_run_and_other_modes_untouched(sv):
    import torch
    scans, front = scans_and_front(sv, 64)
    ps, q, t = random_poses(11, 130)
    ss = np.linspace(ps[0] - 0.1, ps[-1] + 0.1, 64)
    kq = np.tile([1.0, 0, 0, 0], (6, 1)); kt = np.zeros((6, 3)); kt[:, 0] = np.arange(6); kps = np.arange(6) * 25.0
    kss = kps[np.arange(64) % 6] + 0.004
    ki, ksp = sv.assemble_observations(kps, kq, kt, scans, kss)  # the key-frame mode before ...
    before_k = _bytes(sv.stored_observations())
    rng = np.random.default_rng(2)
    sps = np.arange(108, dtype=np.float64); sq = np.tile([1.0, 0, 0, 0], (108, 1))
    stt = np.concatenate([np.concatenate([rng.uniform(-1, 1, 3) + rng.normal(0, 0.0002, (35, 3)), [[50.0 + k, -40.0, 30.0]]]) for k in range(3)])
    sss = np.linspace(-2.0, 110.0, 64)
    si, ssp = sv.assemble_stations(sps, sq, stt, scans, sss)     # ... the station mode before ...
    before_s = _bytes(sv.stored_observations())
    assert ki.n_observations > 0 and si.n_observations > 0 and si.n_stations == 3

    info, sb, su, got = check_assembly(sv, ps, q, t, scans, front, ss)
    assert info.n_observations >= 20
    S, n = 64, int(scans["offsets"][-1])
    d = [_dev(a) for a in (ps, q, t, scans["ranges"], scans["offsets"], scans["angle_min"], scans["angle_increment"], scans["range_min"], ss)]
    d_sb = torch.full((S,), 7, dtype=torch.int32, device=d[0].device)
    d_su = torch.full((S,), 7.0, dtype=torch.float64, device=d[0].device)
    torch.cuda.synchronize()
    for _ in range(2):  # the device form, twice: the same bits as the host form
        i2 = sv.assemble_interpolated_device(len(ps), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), S, n,
                                             d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr(), d_sb.data_ptr(), d_su.data_ptr())
        assert _fields(i2) == _fields(info)
        assert np.array_equal(d_sb.cpu().numpy(), sb) and d_su.cpu().numpy().tobytes() == su.tobytes()
        assert _bytes(sv.stored_observations()) == _bytes(got)
    i3 = sv.assemble_interpolated_device(len(ps), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), S, n,
                                         d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr())  # bracket and u nullable
    assert i3.n_observations == info.n_observations and _bytes(sv.stored_observations()) == _bytes(got)
    info4, sb4, su4 = sv.assemble_interpolated(ps, q, t, scans, ss)  # the host form again
    assert _fields(info4) == _fields(info) and np.array_equal(sb4, sb) and su4.tobytes() == su.tobytes() and _bytes(sv.stored_observations()) == _bytes(got)

    ki2, ksp2 = sv.assemble_observations(kps, kq, kt, scans, kss)  # ... and after: the same bits
    assert np.array_equal(ksp, ksp2) and _bytes(sv.stored_observations()) == before_k and _fields(ki2) == _fields(ki)
    si2, ssp2 = sv.assemble_stations(sps, sq, stt, scans, sss)
    assert np.array_equal(ssp, ssp2) and _bytes(sv.stored_observations()) == before_s and _fields(si2) == _fields(si)


def test_assembly_bad_arguments(sv):
    scans, _ = scans_and_front(sv, 64)
    ps, q, t = random_poses(11, 20)
    bad = dict(scans); bad["offsets"] = scans["offsets"].copy(); bad["offsets"][2] = 5
    with pytest.raises(clc.ClcError) as e:
        sv.assemble_interpolated(ps, q, t, bad, np.ones(64))
    assert e.value.code == -1
    for o in (_opt(max_gap=0.0), _opt(max_gap=-0.1), _opt(max_gap=np.nan), _opt(max_gap=np.inf), _opt(time_offset=np.nan), _opt(time_offset=-np.inf)):
        with pytest.raises(clc.ClcError) as e:
            sv.assemble_interpolated(ps, q, t, scans, np.ones(64), o)
        assert e.value.code == -1
    o = _opt(); o.line.max_num_iterations = -1
    with pytest.raises(clc.ClcError):
        sv.assemble_interpolated(ps, q, t, scans, np.ones(64), o)
    o = _opt(); o.line0[0] = np.nan
    with pytest.raises(clc.ClcError) as e:
        sv.assemble_interpolated(ps, q, t, scans, np.ones(64), o)
    assert e.value.code == -3
    L = sv._L
    assert L.clc_assemble_interpolated(sv._h, None, 2, None, None, None, None, None, 0, None, None, None, None, None, None, None) == -1
    assert L.clc_assemble_interpolated_device(None, None, 0, None, None, None, None, None, 0, 0, None, None, None, None, None, None, None) == -1


# ---- the sweep's records ------------------------------------------------------------------------------------------------------------
def _sweep_opt(offset_min, offset_max, n_offsets, points_per_scan, max_gap=None):
    o = clc.default_time_offset_options()
    o.offset_min, o.offset_max, o.n_offsets, o.points_per_scan = offset_min, offset_max, n_offsets, points_per_scan
    if max_gap is not None:
        o.interp.max_gap = max_gap
    o.solve.max_num_iterations = 2  # (the records are what is looked at)
    return o


X0 = np.array([0.05, -0.02, 0.1, 0.0, 0.0, 0.0, 1.0])


def check_sweep_records(sv, oracle_mod, ps, q, t, scans, front, ss, o):
    P, seg, status = front
    cands = IR.candidates(o.offset_min, o.offset_max, o.n_offsets)
    used, sets = IR.sweep_sets(ps, q, t, ss, status, P, scans["offsets"], seg, cands, o.points_per_scan, o.interp.max_gap)
    out = sv.time_offset_sweep(ps, q, t, scans, ss, X0, o)
    assert np.array_equal(out["offsets"], cands)
    want = [oracle_mod.flatten(S, False, False) for S in sets]
    assert out["n_scans_used"] == len(used) and out["records_per_problem"] == (want[0].shape[0] if len(used) else 0)
    if len(used) == 0:
        assert out["best_index"] == -1 and math.isnan(out["best_offset"]) and np.isnan(out["final_cost"]).all()
        return out, used
    rec = sv.debug_sweep_records()
    R_ = want[0].shape[0]
    assert rec.shape == (o.n_offsets * R_, 8) and sv.num_problems == o.n_offsets
    for j in range(o.n_offsets):
        got = rec[j * R_:(j + 1) * R_]
        assert np.abs(got - want[j]).max() <= 1e-12, (j, np.abs(got - want[j]).max())
        assert got[:, 4:7].tobytes() == want[j][:, 4:7].tobytes()  # the points: copies
    return out, used


@pytest.mark.parametrize("n_offsets", [3, 5])
@pytest.mark.parametrize("S", [5, 70])
def test_sweep_records_equal_the_flattened_restated_sets(sv, oracle_mod, S, n_offsets):
    """points_per_scan 0, 1, 2, 16: every segment K7 returns has more than 50 points (s_end - s_start > 50, src/selectScanPoints.cpp), so
    none is shorter than 16 and these four all decimate or take all; 100 and 1000 are added for segments SHORTER than points_per_scan
    (the lengths here run from 65 to 278)."""
    scans, front = scans_and_front(sv, S)
    lens = (front[1][:, 1] - front[1][:, 0] + 1)[front[2] == 1]
    assert lens.min() < 100 < lens.max()
    ps, q, t = random_poses(13, 130)
    ss = np.linspace(ps[0] + 0.1, ps[-1] - 0.1, S) + 0.0003
    gen = sv.store_generation
    for m in (0, 1, 2, 16, 100, 1000):
        out, used = check_sweep_records(sv, oracle_mod, ps, q, t, scans, front, ss, _sweep_opt(-0.02, 0.02, n_offsets, m))
        assert len(used) == int((front[2] == 1).sum()) >= 3
        want = sum(min(int(L), m) if m else int(L) for L in lens)
        assert out["records_per_problem"] == want
    assert sv.store_generation == gen  # the observation store is not touched


def test_sweep_membership(sv, oracle_mod):
    scans, front = scans_and_front(sv, 70)
    found = np.nonzero(front[2] == 1)[0]
    ps, q, t = random_poses(13, 130)
    ss = np.linspace(ps[0] + 0.1, ps[-1] - 0.1, 70) + 0.0003
    a, b, c = found[0], found[1], found[-1]
    ss[a] = ps[0] + 0.015     # loses its bracket at the first offset (-20 ms) only: in front of the first pose there
    ss[b] = ps[-1] - 0.015    # ... at the last offset (+20 ms) only: behind the last pose
    ss[c] = ps[40] - 0.005    # ... at the last offset only: pair (40, 41) there, and pose 41 holds a NaN
    qn = q.copy(); qn[41, 1] = np.nan
    o = _sweep_opt(-0.02, 0.02, 3, 16)
    cands = IR.candidates(-0.02, 0.02, 3)
    for s, dropped_at in ((a, 0), (b, 2), (c, 2)):
        per = [IR.interpolate(ps, qn, t, ss[s:s + 1], d)["bracket"][0] >= 0 for d in cands]
        assert per.count(False) == 1 and not per[dropped_at]  # at one offset only ...
    out, used = check_sweep_records(sv, oracle_mod, ps, qn, t, scans, front, ss, o)
    assert a not in used and b not in used and c not in used and found[2] in used and len(used) >= 10  # ... dropped everywhere
    # every scan dropped: behind the last pose, or no pair short enough; no scans at all
    out, used = check_sweep_records(sv, oracle_mod, ps, q, t, scans, front, np.full(70, ps[-1] + 0.01), o)
    assert out["n_scans_used"] == 0 and out["best_index"] == -1 and out["at_edge"] == 0
    out, used = check_sweep_records(sv, oracle_mod, ps, q, t, scans, front, ss, _sweep_opt(-0.02, 0.02, 3, 16, max_gap=0.03))
    assert out["n_scans_used"] == 0
    none, nfront = scans_and_front(sv, 0)
    out, used = check_sweep_records(sv, oracle_mod, ps, q, t, none, nfront, np.zeros(0), o)
    assert out["n_scans_used"] == 0 and out["best_index"] == -1


def test_sweep_bad_arguments(sv):
    scans, _ = scans_and_front(sv, 5)
    ps, q, t = random_poses(13, 20)
    ss = np.linspace(ps[2], ps[-3], 5)
    bads = []
    for kw in (dict(n_offsets=2), dict(n_offsets=1025), dict(offset_min=0.01, offset_max=0.01), dict(offset_min=0.02, offset_max=-0.02),
               dict(offset_min=np.nan), dict(offset_max=np.inf), dict(points_per_scan=-1)):
        o = clc.default_time_offset_options()
        for k, v in kw.items():
            setattr(o, k, v)
        bads.append(o)
    o = clc.default_time_offset_options(); o.interp.max_gap = 0.0
    bads.append(o)
    for o in bads:
        with pytest.raises(clc.ClcError) as e:
            sv.time_offset_sweep(ps, q, t, scans, ss, X0, o)
        assert e.value.code == -1
    L = sv._L
    assert L.clc_clock_offset_sweep(sv._h, None, 0, None, None, None, None, None, 0, None, None, None, None, None, None, None, None, None, None) == -1
    assert L.clc_clock_offset_sweep_device(None, None, 0, None, None, None, None, None, 0, 0, None, None, None, None, None, None, None, None,
                                          None, None) == -1


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
OFF9 = [-0.02 + 0.005 * j for j in range(9)]
TRUE_OFFSET = 0.007
REF_OFFSET_ERR = 3.017e-5   # |best_offset - 7 ms| of the restatement + oracle on the CPU, seed 1 (measured; see the docstring below)
REF_TLC_ERR = 2.383e-3      # max |T_lc - truth| of the restatement + oracle on the CPU at its best_offset, seed 1


@pytest.fixture(scope="module")
def moving(oracle_mod):
    rec = so.moving_recording(1, n_stations=6, move_frames=10, still_frames=4, clock_offset=TRUE_OFFSET, offsets=OFF9 + [0.0])
    P = R.scan_points(rec["scans"], oracle_mod)
    seg, status = BS.board_segments(P, rec["scans"]["offsets"])
    return rec, P, seg, status


def restated_flow(oracle_mod, moving, offset):
    """Assembly at `offset` with all points -> (scan_bracket, ObservationSet, Tlc0 of the closed form, the oracle's solve from inv(Tlc0))."""
    rec, P, seg, status = moving
    ip = IR.interpolate(rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scan_stamp"], offset)
    sb = IR.associate(ip, status)
    obs = IR.observations(ip, sb, P, rec["scans"]["offsets"], seg, oracle_mod.line_fit)
    Tlc0, _, _ = oracle_mod.closed_form(oracle_mod.flatten(obs, True, False))
    return sb, obs, Tlc0, oracle_mod.solve(oracle_mod.flatten(obs, False, False), sd.pose7_from_T(np.linalg.inv(Tlc0)))


def test_end_to_end_sweep_and_flow_match_the_oracle_and_recover_the_clock_offset(sv, oracle_mod, moving):
    """moving_recording(1): 6 stations, 10 moving + 4 still frames, the laser's clock 7 ms behind; 9 candidates over -20 .. +20 ms.
    Measured on the CPU (restatement + oracle, this seed): the restated sweep's best_offset is 7.030 ms, 3.017e-5 s from the truth, and
    the restated flow at that offset ends max |T_lc - truth| = 2.383e-3 (8.9e-3 with the offset left at 0).  The GPU result is gated at
    those values + 1e-6 s / + the parity gates."""
    rec, P, seg, status = moving
    ps, q, t, scans, ss = rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"]
    _, _, Tlc_start, _ = restated_flow(oracle_mod, moving, 0.0)
    x0 = sd.pose7_from_T(np.linalg.inv(Tlc_start))
    cands = IR.candidates(-0.02, 0.02, 9)
    used, sets = IR.sweep_sets(ps, q, t, ss, status, P, scans["offsets"], seg, cands, 16)
    refs = [oracle_mod.solve(oracle_mod.flatten(S, False, False), x0) for S in sets]
    o = clc.default_time_offset_options()
    o.n_offsets = 9
    out = sv.time_offset_sweep(ps, q, t, scans, ss, x0, o)
    assert out["n_scans_used"] == len(used) >= 60 and out["records_per_problem"] == 16 * len(used)
    for j, ref in enumerate(refs):
        dT = np.abs(sd.T_from_pose7(out["poses"][j]) - sd.T_from_pose7(ref.pose)).max()
        dc = abs(out["final_cost"][j] - ref.summary.final_cost)
        print(f"offset {cands[j] * 1e3:+.0f} ms: cost {out['final_cost'][j]:.4e} |dTcl| = {dT:.2e} |dcost| = {dc:.2e} iterations "
              f"{out['summaries'][j].num_iterations} / {ref.summary.num_iterations}")
        assert dT <= 1e-6 and dc <= 1e-8 and out["summaries"][j].num_iterations == ref.summary.num_iterations
        assert out["summaries"][j].final_cost == out["final_cost"][j]
    bi, bo, ae = IR.best(cands, [r.summary.final_cost for r in refs], [r.summary.termination for r in refs])
    print(f"best offset {out['best_offset']:.6e} s (oracle {bo:.6e}), index {out['best_index']}")
    assert out["best_index"] == bi == 5 and out["at_edge"] == ae == 0 and abs(out["best_offset"] - bo) <= 1e-6
    assert abs(bo - TRUE_OFFSET) <= REF_OFFSET_ERR * 1.001  # the measured value is the restatement's
    assert abs(out["best_offset"] - TRUE_OFFSET) <= REF_OFFSET_ERR + 1e-6

    # the whole flow: the closed-form start at offset 0, the sweep, the assembly at its best offset, closed form, solve
    so.check_motion_margins(rec, [bo])  # (no bracket of the assembly at the chosen offset hinges on its last digits)
    sb_ref, obs_ref, Tlc0_ref, ref = restated_flow(oracle_mod, moving, bo)
    flow = clc.CalibrateOfflineInterpolated(ps, q, t, scans, ss, time_offset="estimate", sweep_options=o, solver=sv, verbose=False)
    assert flow is not None and abs(flow["time_offset"] - bo) <= 1e-6 and flow["sweep"]["best_index"] == bi
    assert np.array_equal(flow["sweep"]["offsets"], cands) and np.abs(flow["sweep"]["final_cost"] - out["final_cost"]).max() <= 1e-8
    assert np.array_equal(flow["scan_bracket"], sb_ref) and flow["info"].n_observations == obs_ref.n_poses >= 60
    dT = np.abs(flow["Tcl"] - sd.T_from_pose7(ref.pose)).max()
    dc = abs(flow["report"].result.summary.final_cost - ref.summary.final_cost)
    print(f"flow: |dTcl| = {dT:.2e}, |dcost| = {dc:.2e}, iterations {flow['report'].result.summary.num_iterations} / {ref.summary.num_iterations}")
    assert dT <= 1e-6 and dc <= 1e-8 and flow["report"].result.summary.num_iterations == ref.summary.num_iterations
    assert np.abs(flow["Tlc_initial"] - Tlc0_ref).max() <= 1e-6
    GT = np.eye(4); GT[:3, :3] = sd.GT_RLC; GT[:3, 3] = sd.GT_TLC
    ref_err = np.abs(np.linalg.inv(sd.T_from_pose7(ref.pose)) - GT).max()
    err = np.abs(flow["Tlc"] - GT).max()
    print(f"max |T_lc - truth|: {err:.4e} (restatement + oracle: {ref_err:.4e})")
    assert ref_err <= REF_TLC_ERR * 1.001 and err <= REF_TLC_ERR + 1e-6

    # a given offset; the gates of the reference's flow
    fixed = clc.CalibrateOfflineInterpolated(ps, q, t, scans, ss, time_offset=0.005, solver=sv, verbose=False)
    sb5, obs5, _, ref5 = restated_flow(oracle_mod, moving, 0.005)
    assert fixed["sweep"] is None and fixed["time_offset"] == 0.005 and np.array_equal(fixed["scan_bracket"], sb5)
    assert np.abs(fixed["Tcl"] - sd.T_from_pose7(ref5.pose)).max() <= 1e-6
    assert abs(fixed["report"].result.summary.final_cost - ref5.summary.final_cost) <= 1e-8
    assert clc.CalibrateOfflineInterpolated(ps[:9], q[:9], t[:9], scans, ss, solver=sv, verbose=False) is None
    assert clc.CalibrateOfflineInterpolated(ps, q, t, scans, ss + 500.0, solver=sv, verbose=False) is None
    with pytest.raises(ValueError):
        clc.CalibrateOfflineInterpolated(ps, q, t, scans, ss, time_offset="guess", solver=sv, verbose=False)
