"""The offline flow's assembly (K13, clc_assemble_observations) without a GPU: the C-ABI surface, the restatement of
main/calibr_offline.cpp:62-155 (tests/offline_ref.py) on hand-written cases, and the seeded recording of simoffline.py — margins,
yield, and that the oracle's closed form + solve on the restated observations recovers the ground truth."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import offline_ref as R
from camlasercalibratool_amd import _build, _capi, simdata as sd, simoffline as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["clc_assemble_options_default", "clc_keyframes", "clc_assemble_observations", "clc_assemble_observations_device", "clc_stored_observations"]


def _header():
    return open(os.path.join(ROOT, "include", "clc.h")).read()


def test_symbols_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(clc_[a-z0-9_]+)\s*\(", hdr))
    L = _capi.load(_build.PRODUCT_LIB_PATH)
    for name in NEW:
        assert name in declared and name in _capi.EXPORTED and hasattr(L, name), name
    assert L.clc_version() == 210
    import camlasercalibratool_amd as clc
    for m in ("keyframes", "assemble_observations", "assemble_observations_device", "stored_observations"):
        assert callable(getattr(clc.Solver, m))
    assert callable(clc.CalibrateOffline)


def test_struct_layouts_match_header():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct clc_assemble_options \{(.*?)\} clc_assemble_options;", hdr, flags=re.S).group(1)
    names = [m.group(2) for m in re.finditer(r"(double|clc_options)\s+(\w+)(?:\[\d+\])?;", body)]
    assert names == [f[0] for f in _capi.AssembleOptions._fields_]
    assert C.sizeof(_capi.AssembleOptions) == 5 * 8 + C.sizeof(_capi.Options)
    body = re.search(r"typedef struct clc_assemble_info \{(.*?)\} clc_assemble_info;", hdr, flags=re.S).group(1)
    assert [m.group(1) for m in re.finditer(r"int64_t\s+(\w+);", body)] == [f[0] for f in _capi.AssembleInfo._fields_]
    assert C.sizeof(_capi.AssembleInfo) == 7 * 8
    codes = dict(re.findall(r"#define (CLC_SCAN_\w+) \((-\d+)\)", hdr))
    assert codes == {"CLC_SCAN_NO_SEGMENT": "-1", "CLC_SCAN_REF_THROWS": "-2", "CLC_SCAN_NO_POSE": "-3"}
    assert (_capi.SCAN_NO_SEGMENT, _capi.SCAN_REF_THROWS, _capi.SCAN_NO_POSE) == (R.NO_SEGMENT, R.REF_THROWS, R.NO_POSE) == (-1, -2, -3)


def test_defaults_are_the_references():
    o = _capi.default_assemble_options()  # host-side: needs no GPU
    assert o.keyframe_dist_min == 0.20 == R.DIST_MIN and o.keyframe_theta_min == 3.1415926 * 10 / 180. == R.THETA_MIN
    assert o.max_dt == 0.02 == R.MAX_DT and list(o.line0) == [0.0, 0.0]
    assert o.line.max_num_iterations == 10 and o.line.loss_scale_factor == 0.05


def test_measured_constants_stay_valid():
    """The new kernels live in a side header: the identity of the measured kernels' sources is the recorded one."""
    with open(os.path.join(ROOT, "profiles", "valu_counts.json")) as f:
        assert _build.csrc_sha16() == json.load(f)["csrc_sha16"]
    assert "clc_assemble.hpp" in _build.SIDE_HEADERS and "clc_assemble.hpp" not in _build.HEADERS


# ---- the restatement on hand-written cases ---------------------------------------------------------------------------------------
def test_keyframes_plain_walk():
    q = np.tile([1.0, 0, 0, 0], (6, 1))
    t = np.array([[0, 0, 0], [0.1, 0, 0], [0.19, 0, 0], [0.21, 0, 0], [0.3, 0, 0], [0.42, 0, 0]], dtype=float)
    assert R.keyframes(q, t).tolist() == [True, False, False, True, False, True]  # always against the LAST KEPT pose
    h = np.deg2rad(11.0) / 2
    q2 = np.array([[1.0, 0, 0, 0], [np.cos(h), 0, 0, np.sin(h)]])
    assert R.keyframes(q2, np.zeros((2, 3))).tolist() == [True, True]
    h = np.deg2rad(9.0) / 2
    q2[1] = [np.cos(h), 0, np.sin(h), 0]
    assert R.keyframes(q2, np.zeros((2, 3))).tolist() == [True, False]
    assert R.keyframes(np.zeros((0, 4)), np.zeros((0, 3))).tolist() == []


def test_keyframes_keep_the_references_odd_ends():
    q0 = np.array([0.5, 0.5, 0.5, 0.5])
    z = np.zeros(3)
    # antipodal quaternion: the same rotation, w = -1, theta = 2 pi > theta_min -> kept
    assert R.keyframes(np.array([q0, -q0]), np.array([z, z])).tolist() == [True, True]
    # |w| > 1 (newer not normalised): acos gives NaN, the angle test is false -> dropped
    assert R.keyframes(np.array([q0, 2.0 * q0]), np.array([z, z])).tolist() == [True, False]
    # ... also when the quotient exceeds 1 by rounding only
    qa = np.array([0.1, 0.7, 0.3, 0.64])
    assert R.keyframes(np.array([qa, qa * (1 + 2.0 ** -52)]), np.array([z, z])).tolist() == [True, False]
    # a NaN distance makes the distance test false; the angle still decides
    tn = np.array([np.nan, 0, 0])
    assert R.keyframes(np.array([q0, q0]), np.array([z, tn])).tolist() == [True, False]
    assert R.keyframes(np.array([q0, -q0]), np.array([z, tn])).tolist() == [True, True]


def test_closest_pose_ties_order_gate_and_nan():
    # exact tie (dyadic stamps): the first in key-frame order wins (strict <)
    assert R.closest_pose([1.0, 1.25], 1.125, max_dt=0.5) == 0
    assert R.closest_pose([1.25, 1.0], 1.125, max_dt=0.5) == 0
    assert R.closest_pose([1.0, 1.0, 1.0], 1.0) == 0
    # unsorted stamps: the walk looks at all of them
    assert R.closest_pose([5.0, 1.0, 3.0, 1.01, 0.5], 1.004) == 1
    # the gate is strict: |dt| == max_dt is rejected, the next float below is accepted
    assert R.closest_pose([1.0], 1.25, max_dt=0.25) == -1
    assert R.closest_pose([1.0], np.nextafter(1.25, 0), max_dt=0.25) == 0
    assert R.closest_pose([100.0], 100.019) == 0 and R.closest_pose([100.0], 100.021) == -1
    # a NaN stamp is never chosen; no key frames, or all beyond 10000 s: none
    assert R.closest_pose([np.nan, 2.0], 2.001) == 1 and R.closest_pose([np.nan], 2.0) == -1
    assert R.closest_pose([], 2.0) == -1 and R.closest_pose([0.0], 20000.0, max_dt=1e9) == -1


def test_associate_reports_original_indices_and_reasons():
    keep = np.array([True, False, True, True])
    stamp = np.array([10.0, 10.1, 10.2, 10.3])
    status = np.array([1, 1, 0, -1, 1], dtype=np.int32)
    sp = R.associate(stamp, keep, status, np.array([10.201, 10.1, 10.2, 10.2, 10.31]))
    assert sp.tolist() == [2, R.NO_POSE, R.NO_SEGMENT, R.REF_THROWS, 3]  # pose 1 is no key frame: scan 1 finds nothing within 20 ms


def test_tag_pose_and_end_points():
    rng = np.random.default_rng(0)
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    t = rng.uniform(-3, 3, 3)
    qi, ti = R.tag_pose(q, t)
    Rwc = sd.quat_wxyz_to_rot(q)
    assert np.allclose(sd.quat_wxyz_to_rot(qi), Rwc.T, atol=1e-15) and np.allclose(ti, -Rwc.T @ t, atol=1e-14)
    P = np.array([[1.0, -0.3, 0], [1.0, 0.0, 0], [1.02, 0.4, 0]])  # near-vertical in x: the ordinate branch
    e = R.end_points(P, (-1.0, 0.05))
    assert np.allclose(e[:, 1], [-0.3, 0.4]) and np.allclose(-1.0 * e[:, 0] + 0.05 * e[:, 1] + 1, 0, atol=1e-15) and np.all(e[:, 2] == 0)
    e = R.end_points(P[:, [1, 0, 2]], (0.05, -1.0))  # the abscissa branch
    assert np.allclose(e[:, 0], [-0.3, 0.4]) and np.allclose(0.05 * e[:, 0] - e[:, 1] + 1, 0, atol=1e-15)
    assert R.end_points(P[:1], (1.0, 1.0)).shape == (0, 3)


# ---- the recording ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated(oracle_mod):
    rec = so.recording(1)
    return rec, R.assemble(rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"], oracle_mod)


def test_recording_margins_hold_for_the_restatement(restated):
    rec, (keep, scan_pose, obs, info) = restated
    m = []
    assert np.array_equal(R.keyframes(rec["q_wc"], rec["t_wc"], margins=m), keep)
    assert min(m) >= 1e-6
    assert np.array_equal(so.keyframe_walk(rec["q_wc"], rec["t_wc"])[0], keep)
    ks = rec["pose_stamp"][keep]
    dt = np.sort(np.abs(ks[None, :] - rec["scan_stamp"][:, None]), axis=1)
    assert np.abs(dt - 0.02).min() >= 1e-6 and (dt[:, 1] - dt[:, 0]).min() >= 1e-6
    assert so.check_margins(rec)["keyframe"] >= 1e-6
    assert rec["scans"]["offsets"][1] == 1081 and np.all(np.diff(rec["pose_stamp"]) > 0)


def test_recording_has_something_of_everything(restated):
    rec, (keep, scan_pose, obs, info) = restated
    assert info["n_observations"] >= 30 and info["n_observations"] == obs.n_poses == (scan_pose >= 0).sum()
    assert 10 < info["n_keyframes"] < len(keep) // 2            # the still runs are dropped
    assert info["n_unmatched"] > 0 and (scan_pose == R.NO_SEGMENT).sum() > 0 and info["n_ref_throws"] == 0
    assert np.all(keep[scan_pose[scan_pose >= 0]])
    assert np.array_equal(scan_pose[scan_pose >= 0], rec["scan_frame"][scan_pose >= 0])  # the frame every scan is tied to
    assert np.all(np.diff(obs.ptl_off) == 2) and np.diff(obs.pts_off).min() > 50
    assert np.all(obs.pts[:, 2] == 0) and np.all(obs.ptl[:, 2] == 0)


def test_restated_observations_recover_the_ground_truth(restated, oracle_mod):
    """Closed form on points_on_line, Tcl = inv(Tlc), CamLaserCalibration(obs, Tcl, false) — all with the oracle.  Ranges carry
    N(0, 1 mm) noise and are rounded to float32; ~1.4e4 points on 77 poses.  The bound is 2 mm / 2e-3: two sigma of ONE ray, which an
    estimate from thousands of rays cannot exceed unless the records are inconsistent (a wrong pose matched to a scan is centimetres off).
    Achieved on seed 1: rotation entries 2.6e-4, translation 3.4e-4 m; the closed form alone 3.7e-4 / 1.0e-3 m."""
    rec, (keep, scan_pose, obs, info) = restated
    Tlc0, unobservable, _ = oracle_mod.closed_form(oracle_mod.flatten(obs, True, False))
    assert not unobservable
    res = oracle_mod.solve(oracle_mod.flatten(obs, False, False), sd.pose7_from_T(np.linalg.inv(Tlc0)))
    Tlc = np.linalg.inv(sd.T_from_pose7(res.pose))
    eR, et = np.abs(Tlc[:3, :3] - sd.GT_RLC).max(), np.abs(Tlc[:3, 3] - sd.GT_TLC).max()
    print(f"closed form: {np.abs(Tlc0[:3, :3] - sd.GT_RLC).max():.2e} {np.abs(Tlc0[:3, 3] - sd.GT_TLC).max():.2e}; solve: {eR:.2e} {et:.2e}")
    assert res.summary.termination in (1, 2, 3) and eR <= 2e-3 and et <= 2e-3
