"""K10 (csrc/clc_campose.hpp) on the host: the camera models and the per-image planar PnP compiled with g++ (tests/shim/campose_shim.cpp)
against the numpy restatements of tests/campose_ref.py and scipy's least squares; the board helpers and the YAML reader of
camlasercalibratool_amd/camera.py; and the resources of the new kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import campose_ref as ref  # noqa: E402
from camlasercalibratool_amd import camera as cam_mod  # noqa: E402

PIN = dict(model=1, proj=(367.049931000148, 366.94446918887405, 368.7202381120387, 241.13814795878562))
CAMERAS = {
    "pinhole": cam_mod.Camera.pinhole(*PIN["proj"]),
    "radtan": cam_mod.Camera.pinhole(*PIN["proj"], k1=-0.012, k2=0.0015, p1=2e-4, p2=-1.5e-4),
    "radtan_strong": cam_mod.Camera.pinhole(*PIN["proj"], k1=-0.28, k2=0.07, p1=1e-3, p2=-5e-4),
    "kb": cam_mod.Camera.kannala_brandt(*PIN["proj"], -0.02276964, -0.00056958, -0.0026224, 0.00017455),
    "kb_k5zero": cam_mod.Camera.kannala_brandt(*PIN["proj"], -0.02276964, -0.00056958, -0.0026224, 0.0),
    "kb_k2only": cam_mod.Camera.kannala_brandt(*PIN["proj"], 0.05, 0.0, 0.0, 0.0),
    "kb_linear": cam_mod.Camera.kannala_brandt(*PIN["proj"], 0.0, 0.0, 0.0, 0.0),
    "kb_noroot": cam_mod.Camera.kannala_brandt(*PIN["proj"], -0.5, 0.0, 0.0, 0.0),
}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cp") / "libcampose_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                           os.path.join(HERE, "shim", "campose_shim.cpp"), "-o", out])
    L = C.CDLL(out)
    L.shim_kb_theta.restype = C.c_double
    L.shim_kb_theta.argtypes = [C.c_void_p, C.c_double]
    return L


def _d(a):
    return a.ctypes.data_as(C.c_void_p)


def shim_lift(L, cam, px):
    px = np.ascontiguousarray(px, dtype=np.float32).reshape(-1, 2)
    out = np.empty((len(px), 2))
    c = cam.to_c()
    L.shim_camera_lift(C.byref(c), _d(px), C.c_longlong(len(px)), _d(out))
    return out


def shim_project(L, cam, P, pose7=None):
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3)
    out = np.empty((len(P), 2))
    c = cam.to_c()
    pp = None if pose7 is None else _d(np.ascontiguousarray(pose7, dtype=np.float64))
    L.shim_camera_project(C.byref(c), pp, _d(P), C.c_longlong(len(P)), _d(out))
    return out


def shim_board_poses(L, cam, corners, board, offsets):
    from camlasercalibratool_amd._capi import Options, Summary
    corners = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 2)
    board = np.ascontiguousarray(board, dtype=np.float32).reshape(-1, 2)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    q = np.empty((n, 4)); t = np.empty((n, 3)); rms = np.empty(n); st = np.empty(n, dtype=np.int32)
    sm = (Summary * max(n, 1))()
    o = Options()
    L.shim_pose_options_default(C.byref(o))
    c = cam.to_c()
    L.shim_board_poses(C.byref(c), C.byref(o), _d(corners), _d(board), _d(offsets), C.c_longlong(n), _d(q), _d(t), _d(rms), _d(st), sm)
    return q, t, rms, st, sm


def grid(step=8.0):
    u, v = np.meshgrid(np.arange(0.0, 752.0 + 1e-9, step), np.arange(0.0, 480.0 + 1e-9, step))
    g = np.stack([u.ravel(), v.ravel()], 1)
    centre = np.array([[PIN["proj"][2], PIN["proj"][3]]], dtype=np.float32).astype(np.float64)
    return np.concatenate([g, centre, [[0, 0], [752, 0], [0, 480], [752, 480]]]).astype(np.float32)


def test_camera_struct_layout(shim):
    assert shim.shim_camera_size() == 72 == C.sizeof(cam_mod.ClcCamera)
    assert cam_mod.ClcCamera.proj.offset == 8 and cam_mod.ClcCamera.dist.offset == 40


def dr(k, th):
    """d/dtheta of the lift's polynomial (the degree rule of fold_values)."""
    npow = 9 - 2 * sum(1 for v in k if v == 0.0)
    d = np.ones_like(th)
    for i, v in ((3, k[0]), (5, k[1]), (7, k[2]), (9, k[3])):
        if npow >= i:
            d = d + i * v * th ** (i - 1)
    return d


def fold_values(k):
    """The local maxima of r(theta) = theta + k2 theta^3 + ... on theta > 0 (the degree rule of the lift): the |p_u| at which two
    roots of the lift's polynomial meet."""
    npow = 9 - 2 * sum(1 for v in k if v == 0.0)
    c = np.zeros(10)
    c[1] = 1.0
    for i, v in ((3, k[0]), (5, k[1]), (7, k[2]), (9, k[3])):
        if npow >= i:
            c[i] = v
    d = np.polyder(np.poly1d(c[::-1]))
    d2 = np.polyder(d)
    r = np.poly1d(c[::-1])
    out = []
    for z in (d.r if d.order > 0 else []):
        if abs(z.imag) < 1e-12 and z.real > 0 and d2(z.real) < 0:
            out.append(float(r(z.real)))
    return sorted(out)


@pytest.mark.parametrize("name", ["pinhole", "radtan", "radtan_strong"])
def test_pinhole_lift_matches_restatement(shim, name):
    cam = CAMERAS[name]
    px = grid(4.0)
    a = shim_lift(shim, cam, px)
    b = ref.lift(1, cam.proj, cam.dist, px)
    assert np.all(np.abs(a - b) <= 1e-14 * np.maximum(1.0, np.abs(b)))


@pytest.mark.parametrize("name", ["kb", "kb_k5zero", "kb_k2only", "kb_linear", "kb_noroot"])
def test_kb_lift_picks_the_reference_root(shim, name):
    cam = CAMERAS[name]
    c = cam.to_c()
    # theta on a dense |p_u| grid (the centre, the image corners at |p_u| ~ 1.2, far beyond) against np.roots
    ps = np.concatenate([[0.0, 1e-12, 5e-11], np.linspace(1e-6, 1.3, 700), np.linspace(1.3, 4.0, 200)])
    th = np.array([shim.shim_kb_theta(C.byref(c), p) for p in ps])
    th_ref = np.array([ref.kb_theta_roots(cam.dist, p) for p in ps])
    assert np.all(np.abs(th - th_ref) <= 1e-12), np.abs(th - th_ref).max()
    # where r(theta) folds (a local maximum of f + p), the two roots beside the maximum come as close as we like: samples clustered
    # on both sides of every local maximum value
    folds = fold_values(cam.dist)
    if name in ("kb", "kb_noroot"):
        assert folds, name
    for fm in folds:
        eps = np.logspace(-9, -2, 200)
        pf = np.concatenate([fm * (1 - eps), fm * (1 + eps)])
        thf = np.array([shim.shim_kb_theta(C.byref(c), v) for v in pf])
        thf_ref = np.array([ref.kb_theta_roots(cam.dist, v) for v in pf])
        # next to a fold f' is small: either root is only determined to ~eps p / |f'(theta)| (~1e-12 at 1e-9 below the fold),
        # while the two roots lie ~sqrt(2 (fm - p) / |f''|) >= 4e-5 apart — a different choice could not pass
        tol = np.maximum(1e-12, 1e-15 * pf / np.abs(dr(cam.dist, thf_ref)))
        assert np.all(np.abs(thf - thf_ref) <= tol), (fm, np.abs(thf - thf_ref).max(), pf[np.argmax(np.abs(thf - thf_ref) / tol)])
        assert tol.max() <= 1e-10
    if name == "kb_noroot":  # f = theta - 0.5 theta^3 peaks at 0.544: beyond, theta = |p_u|
        big = ps > 0.6
        assert np.array_equal(th[big], ps[big])
    px = grid(4.0)
    a = shim_lift(shim, cam, px)
    b = ref.lift(2, cam.proj, cam.dist, px)
    assert np.all(np.abs(a - b) <= 1e-12 * np.maximum(1.0, np.abs(b)))


@pytest.mark.parametrize("name", ["pinhole", "radtan", "kb", "kb_k5zero", "kb_k2only"])
def test_project_lift_round_trip(shim, name):
    cam = CAMERAS[name]
    px = grid(4.0)
    xy = shim_lift(shim, cam, px)
    P = np.concatenate([xy, np.ones((len(xy), 1))], 1)
    back = shim_project(shim, cam, P)
    err = np.abs(back - px.astype(np.float64)).max(1)
    if cam.model == 2:
        # spaceToPlane takes theta = acos(z / |P|): within a pixel of the principal point that loses ~1e-16 / theta rad, the
        # reference's own limit, not the lift's (at 1e-5 px from it: 1e-6 px)
        near = np.hypot(px[:, 0] - cam.proj[2], px[:, 1] - cam.proj[3]) < 1.0
        assert err[near].max() <= 1e-5
        err = err[~near]
    assert err.max() <= 1e-9
    assert np.array_equal(back, ref.project(cam.model, cam.proj, cam.dist, P)) or \
        np.abs(back - ref.project(cam.model, cam.proj, cam.dist, P)).max() <= 1e-9


def test_project_with_pose(shim):
    cam = CAMERAS["radtan"]
    rng = np.random.default_rng(3)
    P = rng.uniform([-1, -1, 2], [1, 1, 5], size=(50, 3))
    q = np.concatenate([[1.0], 0.1 * rng.normal(size=3)]); q /= np.linalg.norm(q)  # keeps the points in front
    pose7 = np.array([0.1, -0.2, 0.3, q[1], q[2], q[3], q[0]])
    R = ref.quat_wxyz_to_R(q)
    a = shim_project(shim, cam, P, pose7)
    b = ref.project(1, cam.proj, cam.dist, P @ R.T + pose7[:3])
    assert np.abs(a - b).max() <= 1e-9


def random_pose(rng):
    """A camera pose that keeps a ~0.5 m board in front: R_cw, t_cw."""
    R = ref.rotvec_to_R(rng.normal(size=3) * 0.3)
    t = np.array([-0.2, -0.2, 0.0]) + rng.uniform([-0.2, -0.2, 0.8], [0.2, 0.2, 1.6])
    return R, t


def synth_image(rng, cam, kind, noise):
    if kind == "kalibr":
        ids = np.sort(rng.choice(36, size=int(rng.integers(1, 37)), replace=False))
        board = cam_mod.kalibr_board_points(ids, 6, 6, 0.055, 0.3)
    elif kind == "tag":
        board = cam_mod.apriltag_points(0.165)
    else:
        board = cam_mod.chessboard_points(7, 9, 0.03)
    board = board.astype(np.float32)
    R, t = random_pose(rng)
    X = np.concatenate([board.astype(np.float64), np.zeros((len(board), 1))], 1)
    px = ref.project(cam.model, cam.proj, cam.dist, X @ R.T + t) + rng.normal(size=(len(board), 2)) * noise
    return px.astype(np.float32), board, R, t


@pytest.mark.parametrize("name", ["pinhole", "radtan", "kb"])
def test_pnp_matches_scipy_least_squares(shim, name):
    cam = CAMERAS[name]
    rng = np.random.default_rng({"pinhole": 11, "radtan": 12, "kb": 13}[name])
    imgs = [synth_image(rng, cam, k, 0.3) for k in ["kalibr"] * 8 + ["tag"] * 3 + ["chess"] * 2]
    corners = np.concatenate([i[0] for i in imgs]); board = np.concatenate([i[1] for i in imgs])
    off = np.concatenate([[0], np.cumsum([len(i[0]) for i in imgs])])
    q, t, rms, st, sm = shim_board_poses(shim, cam, corners, board, off)
    assert np.all(st == 1), st
    lifted = ref.lift(cam.model, cam.proj, cam.dist, corners).astype(np.float32).astype(np.float64)
    for k in range(len(imgs)):
        s = slice(off[k], off[k + 1])
        R = ref.quat_wxyz_to_R(q[k])
        R2, t2, sol = ref.pnp_lsq(lifted[s], board[s], R, t[k])
        dR, dt = np.abs(R2 - R).max(), np.abs(t2 - t[k]).max()
        if not (dR <= 1e-9 and dt <= 1e-9):
            # an ill-conditioned image (one small tag far away): the cost is flat to rounding along a direction, and the two
            # minimisers may stop a few 1e-9 apart; ours must then be at least as low as scipy's
            assert dR <= 1e-7 and dt <= 1e-7, (k, dR, dt)
            assert sm[k].final_cost <= 0.5 * np.sum(sol.fun ** 2) * (1 + 1e-12), (k, sm[k].final_cost, 0.5 * np.sum(sol.fun ** 2))
        # the same minimiser from the true pose (scipy above starts from our answer: that alone checks only local optimality)
        # (scipy's own stopping from that farther start leaves it up to ~2e-7 off; another local minimum would be far away and no
        # lower than ours)
        R3, t3, sol3 = ref.pnp_lsq(lifted[s], board[s], imgs[k][2], imgs[k][3])
        assert np.abs(R3 - R2).max() <= 1e-5 and np.abs(t3 - t2).max() <= 1e-5, (k, np.abs(R3 - R2).max(), np.abs(t3 - t2).max())
        assert sm[k].final_cost <= 0.5 * np.sum(sol3.fun ** 2) * (1 + 1e-12)
        assert q[k][0] >= 0
        assert abs(rms[k] - np.sqrt(np.sum(sol.fun ** 2) / (off[k + 1] - off[k]))) <= 1e-9
        assert sm[k].termination in (1, 2, 3)


@pytest.mark.parametrize("name", ["pinhole", "kb"])
def test_pnp_noise_free_reaches_rounding_floor(shim, name):
    cam = CAMERAS[name]
    rng = np.random.default_rng(21)
    for kind in ("kalibr", "tag", "chess"):
        px, board, R, t = synth_image(rng, cam, kind, 0.0)
        q, tt, rms, st, _ = shim_board_poses(shim, cam, px, board, np.array([0, len(px)]))
        assert st[0] == 1
        # float32 pixels and float32 lifted points: ~1e-7 relative; the pose follows to the same order
        assert np.abs(ref.quat_wxyz_to_R(q[0]) - R).max() <= 2e-5 and np.abs(tt[0] - t).max() <= 2e-5 * np.linalg.norm(t)
        assert rms[0] <= 1e-6


def test_status_cases_leave_neighbours_untouched(shim):
    cam = CAMERAS["radtan"]
    rng = np.random.default_rng(5)
    good = [synth_image(rng, cam, "kalibr", 0.3) for _ in range(4)]
    three = (good[0][0][:3], good[0][1][:3])
    line_board = np.stack([np.linspace(0, 0.3, 8), np.zeros(8)], 1).astype(np.float32)
    R, t = random_pose(rng)
    Xl = np.concatenate([line_board, np.zeros((8, 1))], 1)
    line_px = ref.project(1, cam.proj, cam.dist, Xl @ R.T + t).astype(np.float32)
    nan_px = good[1][0].copy(); nan_px[2, 0] = np.nan
    seq = [(good[0][0], good[0][1]), three, (good[1][0], good[1][1]), (line_px, line_board), (good[2][0], good[2][1]),
           (nan_px, good[1][1]), (good[3][0], good[3][1]), (np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))]
    corners = np.concatenate([s[0] for s in seq]); board = np.concatenate([s[1] for s in seq])
    off = np.concatenate([[0], np.cumsum([len(s[0]) for s in seq])])
    q, t, rms, st, _ = shim_board_poses(shim, cam, corners, board, off)
    assert list(st) == [1, 0, 1, -1, 1, -2, 1, 0]
    assert np.isnan(rms[1]) and np.array_equal(q[1], [1, 0, 0, 0]) and np.array_equal(t[1], [0, 0, 0])
    goods = [0, 2, 4, 6]
    alone = [shim_board_poses(shim, cam, seq[k][0], seq[k][1], np.array([0, len(seq[k][0])])) for k in goods]
    for k, a in zip(goods, alone):
        assert np.array_equal(q[k], a[0][0]) and np.array_equal(t[k], a[1][0]) and rms[k] == a[2][0]


def test_board_helpers_restate_the_reference():
    tag, sp = 0.055, 0.3
    P = cam_mod.kalibr_board_points([0, 7, 35], 6, 6, tag, sp)
    s = tag * (1 + sp)  # tag_spacing_sz, calcCamPose.cpp:115-141
    exp = []
    for i in (0, 7, 35):
        r, c = i // 6, i % 6
        exp += [(s * c, s * r), (s * c + tag, s * r), (s * c + tag, s * r + tag), (s * c, s * r + tag)]
    assert np.array_equal(P, np.array(exp, dtype=np.float32))
    assert np.array_equal(cam_mod.apriltag_points(0.165), np.array([[0, 0], [0.165, 0], [0.165, 0.165], [0, 0.165]], dtype=np.float32))
    C2 = cam_mod.chessboard_points(2, 3, 0.1)
    assert np.array_equal(C2, np.array([[0, 0], [0.1, 0], [0.2, 0], [0, 0.1], [0.1, 0.1], [0.2, 0.1]], dtype=np.float32))


def test_camera_from_yaml():
    g = os.path.join(HERE, "golden")
    p = cam_mod.Camera.from_yaml(os.path.join(g, "camera_pinhole.yaml"))
    assert p.model == 1 and p.proj == (367.049931000148, 366.94446918887405, 368.7202381120387, 241.13814795878562)
    assert p.dist == (0.0, 0.0, 0.0, 0.0)
    k = cam_mod.Camera.from_yaml(os.path.join(g, "camera_kannala_brandt.yaml"))
    assert k.model == 2 and k.dist == (-0.02276964, -0.00056958, -0.0026224, 0.00017455) and k.proj[2] == 368.7202381120387
    r = cam_mod.Camera.from_yaml(os.path.join(g, "camera_radtan.yaml"))
    assert r.model == 1 and r.dist == (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)


def test_board_pose_kernels_no_spills_no_scratch(tmp_path):
    from camlasercalibratool_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + ["-save-temps", "-c", os.path.join(CSRC, "abi_campose.hip"), "-o", str(tmp_path / "cp.o")],
                       capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    s_files = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "gfx950" in f]
    assert s_files
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_resources.py"), str(tmp_path / s_files[0]), "cp::"],
                         capture_output=True, text=True).stdout.splitlines()
    rows = [l.split() for l in out[1:] if l.strip()]
    names = " ".join(out)
    for frag in ("board_pose_kernel", "campose_lift_kernel", "campose_project_kernel"):
        assert frag in names, names
    for r in rows:
        assert int(r[3]) == 0, r  # no scratch
    # spill counts from the code-object metadata: one entry per kernel, "- .agpr_count" first
    text = open(tmp_path / s_files[0]).read()
    meta = text[text.index("amdhsa.kernels:"):]
    seen = 0
    for entry in meta.split("\n  - ")[1:]:
        m = re.search(r"\.name:\s+(\S+)", entry)
        if not m or "2cp" not in m.group(1):
            continue
        name = m.group(1)
        seen += 1
        sgpr = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", entry).group(1))
        vgpr = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", entry).group(1))
        assert vgpr == 0, (name, vgpr)
        # allowance: board_pose_kernel holds the 9x9 Jacobi rows, the evaluation and the inlined controller step at 256 VGPRs; the
        # compiler parks ~26 wave-uniform SGPRs in VGPR lanes (v_writelane / v_readlane, no memory traffic).  Every other kernel: none.
        assert sgpr <= (32 if "board_pose_kernel" in name else 0), (name, sgpr)
    assert seen >= 4, seen
