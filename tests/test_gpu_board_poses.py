"""K10 on the MI355X: the camera models and clc_board_poses against the host build of the same code (tests/shim/campose_shim.cpp) and
scipy; the host and _device forms bit for bit; and the whole camera-to-T_cl flow: corners -> clc_board_poses -> observations ->
solve, against the oracle solve on the same estimated poses and against the truth."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import campose_ref as ref  # noqa: E402
import test_campose_host as H  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import camera as cam_mod, simdata as sd  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sv():
    with clc.Solver(0) as s:
        yield s


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpg") / "libcampose_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                           os.path.join(HERE, "shim", "campose_shim.cpp"), "-o", out])
    L = C.CDLL(out)
    L.shim_kb_theta.restype = C.c_double
    return L


@pytest.mark.parametrize("name", ["pinhole", "radtan", "kb", "kb_k5zero", "kb_noroot"])
def test_device_lift_project_match_host(sv, shim, name):
    cam = H.CAMERAS[name]
    px = H.grid(2.0)
    a = sv.camera_lift(cam, px)
    b = H.shim_lift(shim, cam, px)
    P = np.concatenate([b, np.ones((len(b), 1))], 1)
    rng = np.random.default_rng(1)
    q = np.concatenate([[1.0], 0.1 * rng.normal(size=3)]); q /= np.linalg.norm(q)
    pose7 = np.array([0.05, -0.02, 0.1, q[1], q[2], q[3], q[0]])
    pa, pb = sv.camera_project(cam, P, pose7), H.shim_project(shim, cam, P, pose7)
    if cam.model == 1:
        assert np.array_equal(a, b) and np.array_equal(pa, pb)
    else:
        assert np.all(np.abs(a - b) <= 1e-14 * np.maximum(1.0, np.abs(b)))
        # spaceToPlane's acos / atan2 differ from the host's in the last bit, and acos(z / |P|) amplifies that ~1 / theta near the axis
        assert np.abs(pa - pb).max() <= 1e-10


def mixed_batch(cam, n_images, seed):
    """>= n_images images: Kalibr subsets, single tags, chessboards, a 1 000+ corner board, empty, 3-corner, collinear, NaN."""
    rng = np.random.default_rng(seed)
    seq = []
    for k in range(n_images):
        kind = k % 16
        if kind == 5:
            seq.append((np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)))
        elif kind == 9:
            px, b, _, _ = H.synth_image(rng, cam, "tag", 0.3)
            seq.append((px[:3], b[:3]))
        elif kind == 11:
            lb = np.stack([np.linspace(0, 0.3, 8), np.zeros(8)], 1).astype(np.float32)
            R, t = H.random_pose(rng)
            X = np.concatenate([lb, np.zeros((8, 1))], 1)
            seq.append((ref.project(cam.model, cam.proj, cam.dist, X @ R.T + t).astype(np.float32), lb))
        elif kind == 13:
            px, b, _, _ = H.synth_image(rng, cam, "kalibr", 0.3)
            px = px.copy(); px[0, 1] = np.nan
            seq.append((px, b))
        elif kind == 15 and k % 256 == 15:
            b = cam_mod.chessboard_points(34, 32, 0.01).astype(np.float32)  # 1 088 corners
            R, t = H.random_pose(rng)
            X = np.concatenate([b, np.zeros((len(b), 1))], 1)
            px = ref.project(cam.model, cam.proj, cam.dist, X @ R.T + t) + rng.normal(size=(len(b), 2)) * 0.3
            seq.append((px.astype(np.float32), b))
        else:
            px, b, _, _ = H.synth_image(rng, cam, ("kalibr", "tag", "chess")[k % 3], 0.3)
            seq.append((px, b))
    corners = np.concatenate([s[0] for s in seq]); board = np.concatenate([s[1] for s in seq])
    off = np.concatenate([[0], np.cumsum([len(s[0]) for s in seq])]).astype(np.int64)
    return corners, board, off


@pytest.mark.parametrize("name", ["radtan", "kb"])
def test_board_poses_match_host_scipy_and_device_form(sv, shim, name):
    import torch
    cam = H.CAMERAS[name]
    corners, board, off = mixed_batch(cam, 4096, {"radtan": 7, "kb": 8}[name])  # 4 096 mixed images per model
    q, t, rms, st, sm = sv.board_poses(cam, corners, board, off, want_summaries=True)
    qh, th, rh, sh, smh = H.shim_board_poses(shim, cam, corners, board, off)
    assert np.array_equal(st, sh)
    assert set(np.unique(st)) == {1, 0, -1, -2}
    ok = st == 1
    # the controller (clc_lm.hpp) is built with FMA contraction on the device and without it on the host: the two LM paths end a
    # little apart (about half the images within 1e-12); where the cost is flat along a direction (a single far tag) they may stop
    # up to ~1e-8 apart, at the same cost
    dq, dt = np.abs(q - qh).max(1), np.abs(t - th).max(1)
    close = (dq <= 1e-12) & (dt <= 1e-12)
    for k in np.flatnonzero(ok & ~close):
        assert dq[k] <= 1e-7 and dt[k] <= 1e-7, (k, dq[k], dt[k])
        assert abs(sm[k].final_cost - smh[k].final_cost) <= 1e-10 * smh[k].final_cost, (k, sm[k].final_cost, smh[k].final_cost)
    assert np.all(np.abs(rms[ok] - rh[ok]) <= 1e-10 * rh[ok] + 1e-15)
    assert np.all(q[ok][:, 0] >= 0)
    lifted = ref.lift(cam.model, cam.proj, cam.dist, corners).astype(np.float32).astype(np.float64)
    for k in np.flatnonzero(ok)[::64]:
        s = slice(off[k], off[k + 1])
        R = ref.quat_wxyz_to_R(q[k])
        R2, t2, sol = ref.pnp_lsq(lifted[s], board[s], R, t[k])
        dR, dt = np.abs(R2 - R).max(), np.abs(t2 - t[k]).max()
        if not (dR <= 1e-9 and dt <= 1e-9):  # ill-conditioned image: as in test_campose_host
            assert dR <= 1e-7 and dt <= 1e-7 and sm[k].final_cost <= 0.5 * np.sum(sol.fun ** 2) * (1 + 1e-12), (k, dR, dt)
    dev = torch.device("cuda:0")
    n = len(off) - 1
    dc, db, do = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (corners, board, off))
    dq = torch.empty((n, 4), dtype=torch.float64, device=dev); dtt = torch.empty((n, 3), dtype=torch.float64, device=dev)
    dr = torch.empty(n, dtype=torch.float64, device=dev); ds = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    sv.board_poses_device(cam, dc.data_ptr(), db.data_ptr(), do.data_ptr(), n, dq.data_ptr(), dtt.data_ptr(), dr.data_ptr(), ds.data_ptr())
    assert np.array_equal(ds.cpu().numpy(), st)
    assert np.array_equal(dq.cpu().numpy(), q) and np.array_equal(dtt.cpu().numpy(), t)
    assert np.array_equal(dr.cpu().numpy(), rms, equal_nan=True)


def test_corners_to_tcl_end_to_end(sv):
    """The flow of the reference's offline tool: corners -> clc_board_poses -> clc_store_observations (tag poses = the estimated
    T_ca) -> clc_select_observations -> closed form -> solve, against the oracle solve of the same estimated poses from the same start,
    and against the truth."""
    import oracle
    cam = H.CAMERAS["radtan"]
    rng = np.random.default_rng(31)
    P = 40
    Rs, ts, corners, boards = [], [], [], []
    b = cam_mod.kalibr_board_points(np.arange(36), 6, 6, 0.055, 0.3)
    X = np.concatenate([b.astype(np.float64), np.zeros((len(b), 1))], 1)
    for _ in range(P):
        R, t = H.random_pose(rng)
        px = ref.project(cam.model, cam.proj, cam.dist, X @ R.T + t) + rng.normal(size=(len(b), 2)) * 0.3
        Rs.append(R); ts.append(t); corners.append(px.astype(np.float32)); boards.append(b)
    q, t, st, rms = clc.CalcCamPoses(cam, corners, boards, solver=sv)
    assert np.all(st == 1)
    obs = sd.points_from_tag_poses(np.array(Rs), np.array(ts), noise_sigma=0.002, rng=rng)
    est = sd.ObservationSet(q.copy(), t.copy(), obs.pts_off, obs.pts, obs.ptl_off, obs.ptl)
    sv.store_observations(est)
    sv.select_observations(use_linefitting_data=True)  # the closed form's records (points_on_line)
    Tlc, unobservable, _ = sv.closed_form()
    assert not unobservable
    x0 = sd.pose7_from_T(np.linalg.inv(Tlc))
    sv.select_observations(use_linefitting_data=False)
    res = sv.solve(x0)
    rec = clc.flatten_observations(est, use_linefitting_data=False)
    ref_res = oracle.solve(rec, x0, linear_solver="qr")
    dT = np.abs(sd.T_from_pose7(res.pose) - sd.T_from_pose7(ref_res.pose)).max()
    assert dT <= 1e-6 and abs(res.summary.final_cost - ref_res.summary.final_cost) <= 1e-8, dT
    Tcl = sd.T_from_pose7(res.pose)
    Rcl_true = sd.GT_RLC.T
    tcl_true = -Rcl_true @ sd.GT_TLC
    assert np.abs(Tcl[:3, :3] - Rcl_true).max() <= 2e-2 and np.abs(Tcl[:3, 3] - tcl_true).max() <= 3e-2, Tcl
