"""clc_keyframes / clc_assemble_observations(_device) / clc_stored_observations (K13, main/calibr_offline.cpp:62-155) on the GPU
against the restatement tests/offline_ref.py: key-frame flags and scan -> pose indices exactly, offsets exactly, the stored points
bit for bit the rows that clc_scan_to_points_device + clc_board_segments_device select, host form == device form == a second run,
tag poses and end points within derived bounds, and CalibrateOffline against the oracle on the restated records."""
import numpy as np
import pytest

import offline_ref as R
import camlasercalibratool_amd as clc
from camlasercalibratool_amd import simdata as sd, simoffline as so

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sv():
    s = clc.Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def rec():
    return so.recording(1)


@pytest.fixture(scope="module")
def base_scans():
    """64 scans of 1 081 rays, most with a board: the material of the association and compaction cases."""
    return sd.sim_laser_scans(7, 64)


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


def expected(sv, pose_stamp, q, t, scans, scan_stamp, opt=None):
    """The restatement's decisions on the device's own points and segments -> (keep, scan_pose, pts_off, pts, tag_q, tag_t)."""
    o = opt or clc.default_assemble_options()
    P, seg, status = device_front(sv, scans)
    keep = R.keyframes(q, t, o.keyframe_dist_min, o.keyframe_theta_min)
    scan_pose = R.associate(pose_stamp, keep, status, scan_stamp, o.max_dt)
    off = scans["offsets"]
    kept = np.nonzero(scan_pose >= 0)[0]
    rows = [P[off[s] + seg[s, 0]: off[s] + seg[s, 1] + 1] for s in kept]
    pts_off = np.zeros(len(kept) + 1, dtype=np.int64)
    pts_off[1:] = np.cumsum([len(r) for r in rows])
    tp = [R.tag_pose(q[scan_pose[s]], t[scan_pose[s]]) for s in kept]
    return (keep, scan_pose, pts_off, np.concatenate(rows) if rows else np.zeros((0, 3)), np.array([a for a, _ in tp]).reshape(-1, 4),
            np.array([b for _, b in tp]).reshape(-1, 3), status)


def check_against(sv, pose_stamp, q, t, scans, scan_stamp, opt=None):
    info, scan_pose = sv.assemble_observations(pose_stamp, q, t, scans, scan_stamp, opt)
    keep, sp_ref, pts_off, pts, tq, tt, status = expected(sv, pose_stamp, q, t, scans, scan_stamp, opt)
    assert np.array_equal(scan_pose, sp_ref), np.nonzero(scan_pose != sp_ref)[0][:8]
    got = sv.stored_observations()
    assert np.array_equal(got.pts_off, pts_off)
    assert got.pts.tobytes() == pts.tobytes()  # a copy
    assert np.array_equal(np.diff(got.ptl_off), np.where(np.diff(pts_off) >= 2, 2, 0))
    assert (info.n_keyframes, info.n_segments, info.n_ref_throws, info.n_unmatched, info.n_observations, info.n_points, info.n_line_points) == \
        (int(keep.sum()), int((status == 1).sum()), int((status == -1).sum()), int((sp_ref == R.NO_POSE).sum()), len(pts_off) - 1, int(pts_off[-1]),
         int(got.ptl_off[-1]))
    if len(tq):
        assert np.abs(got.tag_q - tq).max() <= 1e-14 and np.abs(got.tag_t - tt).max() <= 1e-14
    return info, scan_pose, got


# ---- key frames ---------------------------------------------------------------------------------------------------------------------
def _walk(seed, n, step):
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.normal(0, step, (n, 3)), axis=0)
    ang = np.cumsum(rng.normal(0, 0.03, (n, 3)), axis=0)
    q = sd.rot_to_quat_wxyz(sd.rot_zyx(ang[:, 0], ang[:, 1], ang[:, 2])).reshape(n, 4)
    return q, t


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 1000])
def test_keyframes_equal_restatement(sv, n):
    for step in (0.03, 0.5):  # some kept, (nearly) all kept
        q, t = _walk(n, n, step)
        ref = R.keyframes(q, t)
        assert np.array_equal(sv.keyframes(q, t), ref)
    assert ref.sum() >= 0.9 * n  # (a step of 0.5 m: nearly every pose moved)


def test_keyframes_patterns(sv):
    q = np.tile([1.0, 0, 0, 0], (200, 1))
    t = np.zeros((200, 3))
    k = sv.keyframes(q, t)  # none kept after pose 0
    assert k.tolist() == [True] + [False] * 199 == R.keyframes(q, t).tolist()
    t[:, 0] = np.arange(200)  # every pose kept
    assert sv.keyframes(q, t).all()
    # a kept pose on lane 63 of the first chunk (candidates 1 .. 64), the next kept on lane 0 of the following chunk
    t = np.zeros((200, 3)); t[64:, 0] = 1.0; t[65:, 0] = 2.0
    k = sv.keyframes(q, t)
    assert np.nonzero(k)[0].tolist() == [0, 64, 65] == np.nonzero(R.keyframes(q, t))[0].tolist()
    assert sv.keyframes(np.zeros((0, 4)), np.zeros((0, 3))).shape == (0,)
    o = clc.default_assemble_options(); o.keyframe_dist_min = 2.5
    t = np.zeros((10, 3)); t[:, 0] = np.arange(10)
    assert np.array_equal(sv.keyframes(q[:10], t, o), R.keyframes(q[:10], t, 2.5))


def test_keyframes_keep_the_references_odd_ends(sv):
    q0 = np.array([0.5, 0.5, 0.5, 0.5]); z = np.zeros(3); tn = np.array([np.nan, 0, 0])
    for q, t in [(np.array([q0, -q0]), np.array([z, z])),          # antipodal: kept
                 (np.array([q0, 2.0 * q0]), np.array([z, z])),     # |w| > 1: NaN angle, dropped
                 (np.array([q0, q0]), np.array([z, tn])),          # NaN distance: dropped
                 (np.array([q0, -q0]), np.array([z, tn]))]:        # ... the angle still decides
        assert np.array_equal(sv.keyframes(q, t), R.keyframes(q, t))
    assert sv.keyframes(np.array([q0, -q0]), np.array([z, z])).tolist() == [True, True]
    assert sv.keyframes(np.array([q0, 2.0 * q0]), np.array([z, z])).tolist() == [True, False]


# ---- association ------------------------------------------------------------------------------------------------------------------------
def _far_poses(n):
    """n poses a metre apart: every one a key frame."""
    q = np.tile([1.0, 0, 0, 0], (n, 1))
    t = np.zeros((n, 3)); t[:, 0] = np.arange(n)
    return q, t


def _take(scans, idx):
    idx = np.asarray(idx)
    n = 1081
    r = scans["ranges"].reshape(-1, n)[idx]
    return {"ranges": np.ascontiguousarray(r).ravel(), "offsets": np.arange(len(idx) + 1, dtype=np.int64) * n,
            "angle_min": scans["angle_min"][idx], "angle_increment": scans["angle_increment"][idx], "range_min": scans["range_min"][idx]}


def test_association_cases(sv, base_scans):
    scans = _take(base_scans, np.arange(12))
    o = clc.default_assemble_options(); o.max_dt = 0.5
    # one key frame
    q, t = _far_poses(1)
    ss = np.array([1.0, 1.4, 1.6, 0.5, 0.49, 1.0, 2.0, np.nan, 1.25, 0.75, 1.5, 1.0])
    info, sp, _ = check_against(sv, np.array([1.0]), q, t, scans, ss, o)
    assert info.n_observations > 0 and info.n_unmatched > 0
    # exact ties on dyadic stamps, duplicates: the first in key-frame order
    q, t = _far_poses(6)
    ps = np.array([1.0, 1.0, 1.25, 1.25, 1.5, 1.5])
    ss = np.array([1.125, 1.0, 1.25, 1.375, 1.5, 3.0, 1.126, 1.124, 0.4, 2.0, 1.25, 1.1])
    info, sp, _ = check_against(sv, ps, q, t, scans, ss, o)
    assert set(sp[sp >= 0].tolist()) <= {0, 2, 4}
    # unsorted pose stamps: the linear walk
    ps = np.array([5.0, 1.0, 3.0, 1.01, 0.5, 1.0])
    check_against(sv, ps, q, t, scans, np.linspace(0.4, 5.2, 12), o)
    o2 = clc.default_assemble_options()
    check_against(sv, ps, q, t, scans, np.full(12, 1.004), o2)
    # a key frame with a NaN stamp is never chosen
    ps = np.array([1.0, np.nan, 1.2, 1.3, 1.4, 1.5])
    info, sp, _ = check_against(sv, ps, q, t, scans, np.array([1.0, 1.1, 1.2, 1.3, 1.4, 1.5, 1.09, 1.11, 1.21, 1.29, 1.6, 1.39]), o2)
    assert 1 not in sp.tolist() and info.n_observations > 0
    # key frames only: pose 1 is dropped by the filter and cannot be matched, though its stamp is the scan's
    t2 = t.copy(); t2[1] = t2[0]
    ps = np.array([1.0, 1.1, 1.2, 1.3, 1.4, 1.5])
    info, sp, _ = check_against(sv, ps, q, t2, scans, np.full(12, 1.1), o2)
    assert info.n_keyframes == 5 and info.n_observations == 0 and info.n_unmatched == info.n_segments


def test_every_pose_outside_the_gate(sv, base_scans):
    scans = _take(base_scans, np.arange(12))
    q, t = _far_poses(4)
    gen = sv.store_generation
    info, sp, got = check_against(sv, np.arange(4.0), q, t, scans, np.full(12, 100.0))
    assert info.n_observations == 0 and info.n_points == 0 and info.n_segments > 0 and info.n_unmatched == info.n_segments
    assert got.n_poses == 0 and got.pts.shape == (0, 3) and sv.store_generation == gen + 1
    info, sp = sv.assemble_observations(np.zeros(0), np.zeros((0, 4)), np.zeros((0, 3)), scans, np.full(12, 100.0))  # no poses at all
    assert info.n_keyframes == 0 and info.n_observations == 0 and (sp < 0).all()
    none = {"ranges": np.zeros(0, np.float32), "offsets": np.zeros(1, np.int64), "angle_min": np.zeros(0, np.float32),
            "angle_increment": np.zeros(0, np.float32), "range_min": np.zeros(0, np.float32)}
    info, sp = sv.assemble_observations(np.arange(4.0), q, t, none, np.zeros(0))  # no scans at all
    assert info.n_keyframes == 4 and info.n_observations == 0 and sp.shape == (0,)


# ---- compaction and gather --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_scans", [1, 63, 64, 65, 1025, 3000])
def test_compaction_shapes_and_patterns(sv, base_scans, n_scans):
    idx = (np.arange(n_scans) * 7) % 64
    scans = _take(base_scans, idx)
    q, t = _far_poses(3)
    ps = np.array([10.0, 20.0, 30.0])
    near = 20.0 + 0.001 * ((np.arange(n_scans) % 9) - 4)
    far = np.full(n_scans, 50.0)
    only_last = far.copy(); only_last[-1] = 30.005
    for ss in (far, near, np.where(np.arange(n_scans) % 2 == 0, near, far), only_last):
        info, sp, got = check_against(sv, ps, q, t, scans, ss)
    assert info.n_observations == (1 if sp[-1] >= 0 else 0)


def test_ragged_scans_with_an_empty_one(sv):
    parts = [sd.sim_laser_scans(11, 5, n_rays=300), sd.sim_laser_scans(12, 5, n_rays=700), sd.sim_laser_scans(13, 5, n_rays=1081)]
    order = [(0, 0), (1, 0), (2, 0), (2, 1), None, (2, 2), (1, 1), (0, 1), (2, 3), (1, 2), (2, 4)]  # None: the empty scan
    r, lens, am, ai, rm = [], [], [], [], []
    for e in order:
        if e is None:
            lens.append(0); am.append(0.0); ai.append(0.0); rm.append(0.05)
            continue
        b, k = parts[e[0]], e[1]
        r.append(b["ranges"][b["offsets"][k]:b["offsets"][k + 1]]); lens.append(len(r[-1]))
        am.append(b["angle_min"][k]); ai.append(b["angle_increment"][k]); rm.append(b["range_min"][k])
    scans = {"ranges": np.concatenate(r), "offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
             "angle_min": np.array(am, np.float32), "angle_increment": np.array(ai, np.float32), "range_min": np.array(rm, np.float32)}
    q, t = _far_poses(2)
    info, sp, got = check_against(sv, np.array([1.0, 2.0]), q, t, scans, np.full(len(order), 1.001))
    assert sp[4] == R.REF_THROWS and info.n_ref_throws >= 1 and info.n_observations >= 1
    # the neighbours are what they are without the empty scan
    keep = [i for i in range(len(order)) if i != 4]
    sub = {"ranges": scans["ranges"], "offsets": np.concatenate([[0], np.cumsum(np.array(lens)[keep])]).astype(np.int64),
           "angle_min": scans["angle_min"][keep], "angle_increment": scans["angle_increment"][keep], "range_min": scans["range_min"][keep]}
    info2, sp2 = sv.assemble_observations(np.array([1.0, 2.0]), q, t, sub, np.full(len(keep), 1.001))
    got2 = sv.stored_observations()
    assert np.array_equal(sp2, sp[keep]) and got2.pts.tobytes() == got.pts.tobytes() and got2.ptl.tobytes() == got.ptl.tobytes()


# ---- read-back values on the recording ----------------------------------------------------------------------------------------------------
def _bytes(S):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (S.tag_q, S.tag_t, S.pts_off, S.pts, S.ptl_off, S.ptl))


def test_recording_host_form_device_form_and_second_run(sv, rec):
    import torch
    info, sp, got = check_against(sv, rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"])
    assert info.n_observations >= 30
    sc = rec["scans"]
    S, n = len(sc["offsets"]) - 1, int(sc["offsets"][-1])
    d = [_dev(a) for a in (rec["pose_stamp"], rec["q_wc"], rec["t_wc"], sc["ranges"], sc["offsets"], sc["angle_min"], sc["angle_increment"],
                           sc["range_min"], rec["scan_stamp"])]
    d_sp = torch.full((S,), 7, dtype=torch.int32, device=d[0].device)
    torch.cuda.synchronize()
    for _ in range(2):  # the device form, twice: the same bits as the host form
        i2 = sv.assemble_observations_device(len(rec["pose_stamp"]), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                             d[4].data_ptr(), S, n, d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr(), d_sp.data_ptr())
        assert [getattr(i2, f[0]) for f in i2._fields_] == [getattr(info, f[0]) for f in info._fields_]
        assert np.array_equal(d_sp.cpu().numpy(), sp)
        assert _bytes(sv.stored_observations()) == _bytes(got)
    i3 = sv.assemble_observations_device(len(rec["pose_stamp"]), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                         d[4].data_ptr(), S, n, d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr(), 0)  # scan_pose nullable
    assert i3.n_observations == info.n_observations


def test_lines_and_end_points(sv, rec):
    """The assembly's fitted lines (read through the hooks build's clc_debug_assemble_lines) are bit for bit those of
    clc_line_fit_batched_device on the same xy, and each end point is the numpy arithmetic on them within
    8 * 2^-53 * (|x m| + 1) / |m'| — a contracted against an uncontracted x m + 1, divided by the other coefficient."""
    import torch
    info, sp = sv.assemble_observations(rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"])
    got = sv.stored_observations()
    P = got.n_poses
    d_xy, d_off = _dev(got.pts[:, :2]), _dev(got.pts_off)

    def device_fit(line0, options=None):
        d_lines = torch.from_numpy(np.tile(np.asarray(line0, dtype=np.float64), (P, 1))).to(d_xy.device)
        torch.cuda.synchronize()
        sv.line_fit_batched_device(d_xy.data_ptr(), d_off.data_ptr(), P, d_lines.data_ptr(), options=options)
        return d_lines.cpu().numpy()

    lines = device_fit((0.0, 0.0))
    assert sv.debug_assemble_lines().tobytes() == lines.tobytes()
    worst = 0.0
    for k in range(P):
        pp = got.pts[got.pts_off[k]:got.pts_off[k + 1]]
        e = R.end_points(pp, lines[k])
        g = got.ptl[got.ptl_off[k]:got.ptl_off[k + 1]]
        assert g.shape == e.shape == (2, 3) and np.all(g[:, 2] == 0)
        m0, m1 = lines[k]
        horiz = abs(pp[-1, 0] - pp[0, 0]) > abs(pp[-1, 1] - pp[0, 1])
        for i, p in enumerate((pp[0], pp[-1])):
            if horiz:
                bound = 8 * 2.0 ** -53 * (abs(p[0] * m0) + 1) / abs(m1)
                assert g[i, 0] == p[0] and abs(g[i, 1] - e[i, 1]) <= bound, (k, i, g[i], e[i], bound)
                worst = max(worst, abs(g[i, 1] - e[i, 1]) / bound)
            else:
                bound = 8 * 2.0 ** -53 * (abs(p[1] * m1) + 1) / abs(m0)
                assert g[i, 1] == p[1] and abs(g[i, 0] - e[i, 0]) <= bound, (k, i, g[i], e[i], bound)
                worst = max(worst, abs(g[i, 0] - e[i, 0]) / bound)
    print(f"end points: worst error / bound = {worst:.3f}")
    # a start line and line-fit options from the assembly's options reach the fit: with no iterations allowed the fit returns its start,
    # which no fit from (0, 0) does; with the default iterations the lines are again those of the device call from that start
    o = clc.default_assemble_options(); o.line0[0], o.line0[1] = -0.7, 0.1
    o.line.max_num_iterations = 0
    sv.assemble_observations(rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"], o)
    l0 = sv.debug_assemble_lines()
    assert l0.tobytes() == np.tile([-0.7, 0.1], (P, 1)).tobytes() == device_fit((-0.7, 0.1), o.line).tobytes()
    assert not np.any(l0 == lines)
    g0 = sv.stored_observations()
    assert g0.pts.tobytes() == got.pts.tobytes() and g0.ptl.tobytes() != got.ptl.tobytes()
    o.line.max_num_iterations = 10
    sv.assemble_observations(rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"], o)
    assert sv.debug_assemble_lines().tobytes() == device_fit((-0.7, 0.1), o.line).tobytes()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def test_calibrate_offline_matches_the_oracle_on_the_restated_records(sv, rec, oracle_mod):
    keep, sp_ref, obs, info_ref = R.assemble(rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"], oracle_mod)
    Tlc0, _, _ = oracle_mod.closed_form(oracle_mod.flatten(obs, True, False))
    ref = oracle_mod.solve(oracle_mod.flatten(obs, False, False), sd.pose7_from_T(np.linalg.inv(Tlc0)))
    out = clc.CalibrateOffline(rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"], solver=sv, verbose=False)
    assert out is not None and np.array_equal(out["scan_pose"], sp_ref) and out["info"].n_observations == info_ref["n_observations"]
    dT = np.abs(out["Tcl"] - sd.T_from_pose7(ref.pose)).max()
    dc = abs(out["report"].result.summary.final_cost - ref.summary.final_cost)
    print(f"|dTcl| = {dT:.2e}, |dcost| = {dc:.2e}, iterations {out['report'].result.summary.num_iterations} / {ref.summary.num_iterations}")
    assert dT <= 1e-6 and dc <= 1e-8 and out["report"].result.summary.num_iterations == ref.summary.num_iterations
    assert np.abs(out["Tlc_initial"] - Tlc0).max() <= 1e-6
    assert np.abs(out["Tlc"][:3, :3] - sd.GT_RLC).max() <= 2e-3 and np.abs(out["Tlc"][:3, 3] - sd.GT_TLC).max() <= 2e-3
    # the reference's gates
    assert clc.CalibrateOffline(rec["pose_stamp"][:9], rec["q_wc"][:9], rec["t_wc"][:9], rec["scans"], rec["scan_stamp"], solver=sv, verbose=False) is None
    assert clc.CalibrateOffline(rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"] + 50.0, solver=sv, verbose=False) is None


def test_adopting_session_refuses_replaced_scans(sv, rec):
    out = clc.CalibrateOffline(rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"], solver=sv, verbose=False)
    ses = out["session"]
    T = np.eye(4)
    ses.CamLaserCalClosedSolution(T, verbose=False)  # still the session's scans
    assert np.abs(T - out["Tlc_initial"]).max() <= 1e-9
    sv.store_observations(sd.GenerateSimData(3, n_poses=8))  # another caller replaces them
    with pytest.raises(clc.ClcError):
        ses.CamLaserCalClosedSolution(T, verbose=False)
    with pytest.raises(clc.ClcError):
        ses.CamLaserCalibration(np.eye(4), False, verbose=False)


def test_bad_arguments(sv, base_scans):
    scans = _take(base_scans, np.arange(3))
    q, t = _far_poses(2)
    bad = dict(scans); bad["offsets"] = np.array([0, 1081, 900, 3243], dtype=np.int64)
    with pytest.raises(clc.ClcError) as e:
        sv.assemble_observations(np.array([1.0, 2.0]), q, t, bad, np.ones(3))
    assert e.value.code == -1
    o = clc.default_assemble_options(); o.line.max_num_iterations = -1
    with pytest.raises(clc.ClcError):
        sv.assemble_observations(np.array([1.0, 2.0]), q, t, scans, np.ones(3), o)
    L = sv._L
    assert L.clc_assemble_observations(sv._h, None, 2, None, None, None, None, None, 0, None, None, None, None, None, None) == -1
    assert L.clc_keyframes(None, None, 0, None, None, None, None) == -1
    with clc.Solver(0) as fresh:
        with pytest.raises(clc.ClcError) as e:
            fresh.stored_observations()
        assert e.value.code == -5
