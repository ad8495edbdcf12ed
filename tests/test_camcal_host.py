"""K19 (csrc/clc_camcal.hpp, clc_arrow.hpp) on the host: the projection's derivatives, the evaluation blocks, the Schur step, the controller, the
outputs and the closed-form focal start compiled with g++ (tests/shim/camcal_shim.cpp) against the numpy / scipy restatement
tests/camcal_ref.py on the seeded sets of tests/camcal_cases.py: the symbols declared, exported and bound; Jacobians against central
differences through Plus; the minimiser, cost, RMS and H_cam; the hold masks; the closed-form start and the whole flow from it; images
that take no part and failing problems; the refusals of the C ABI (they need no device); a stand-alone AddressSanitizer / UBSan
program over the edge shapes; the YAML round trip of Camera."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import camcal_cases as cases  # noqa: E402
import camcal_ref as ref  # noqa: E402
import test_campose_host as H  # noqa: E402
from camlasercalibratool_amd import _build, _capi  # noqa: E402
from camlasercalibratool_amd.camera import Camera, ClcCamera, KANNALA_BRANDT, PINHOLE  # noqa: E402

CAMS = ["radtan", "kb"]
GXX = ["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off"]
d = H._d
NEW_SYMBOLS = ["clc_camcal_options_default", "clc_camera_guess", "clc_camera_guess_device", "clc_camera_calibrate",
               "clc_camera_calibrate_device"]

# Bounds: one decade over the worst gaps measured on the seeded sets (both cameras; 6, 12 and 20 images; default masks) — the figures
# are in test_seeded_sets_match_restatement's docstring.  A parameter's bound is stated in units of its own 1 sigma from H_cam and must
# stay below 1e-3 of it, so that it cannot hide another minimum; the cost bound lies inside the project's 1e-8 relative gate.
SIGMA_GATE, COST_GATE = 1e-3, 1e-8
PARAM_BOUND_SIGMA = 1.1e-5  # largest |k - k_ref| / sigma_k over the free intrinsics (1.08e-6)
COST_BOUND = 1.4e-13        # relative gap of the final cost (1.39e-14)
RMS_BOUND = 7.1e-14         # relative gap of the RMS in pixels (7.0e-15)
HCAM_BOUND = 3.3e-8         # relative (Frobenius) gap of H_cam to the dense Schur complement at the restatement's minimiser (3.24e-9)
HCAM_SAME_POINT = 1.5e-13   # the same at the answer's own point: what the blocks and the reduction themselves leave (1.42e-14)
POSE_BOUND = 1.9e-8         # largest gap of any R entry or t component, all intrinsics held: per-image pixel-space PnP (1.86e-9)
GUESS_BOUND = 4e-14         # relative gap of the closed-form focal length to the restatement's SVD-based DLT (3.95e-15)
GUESS_FLOW_SIGMA = 1.8e-6   # |dk| / sigma_k of the flow from the guess to the solve from the truth and to the restatement (1.71e-7)
GUESS_FLOW_COST = 9.5e-14   # the two flows' costs, relative (9.4e-15)
assert PARAM_BOUND_SIGMA < SIGMA_GATE and GUESS_FLOW_SIGMA < SIGMA_GATE and COST_BOUND <= COST_GATE and GUESS_FLOW_COST <= COST_GATE


def build_shim(path):
    subprocess.check_call(GXX + ["-shared", os.path.join(HERE, "shim", "camcal_shim.cpp"), "-o", path])
    L = C.CDLL(path)
    L.shim_camera_guess.restype = C.c_double
    L.shim_kb_theta.restype = C.c_double
    L.shim_kb_theta.argtypes = [C.c_void_p, C.c_double]
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(str(tmp_path_factory.mktemp("cc") / "libcamcal_shim.so"))


def k_of(cam):
    return np.r_[cam.proj, cam.dist].astype(np.float64)


def with_k(cam, k):
    return Camera(cam.model, tuple(float(v) for v in k[:4]), tuple(float(v) for v in k[4:]), cam.width, cam.height)


def shim_options(L, model, **kw):
    co = _capi.CamcalOptions()
    L.shim_camcal_options_default(C.byref(co), C.c_int(model))
    for k, v in kw.items():
        setattr(co, k, v)
    return co


def start_poses(L, cam, a):
    """K10 (the shim's) on every image -> q [n, 4], t [n, 3], status [n]."""
    q, t, _, st, _ = H.shim_board_poses(L, cam, a["corners"], a["board"], a["coff"])
    return q, t, st


def shim_calibrate(L, cams, a, q0, t0, keep=None, co=None, max_iterations=None, prob_off=True):
    """shim_camera_calibrate on the arrays of camcal_cases.arrays -> dict, the keys of Solver.camera_calibrate (+ k [np, 8])."""
    n, npb = len(a["coff"]) - 1, len(a["prob_off"]) - 1
    q, t = np.array(q0, dtype=np.float64, order="C"), np.array(t0, dtype=np.float64, order="C")
    o = _capi.Options()
    L.shim_pose_options_default(C.byref(o))
    if max_iterations is not None:
        o.max_num_iterations = max_iterations
    co = co or shim_options(L, cams[0].model)
    cc = (ClcCamera * max(npb, 1))(*[c.to_c() for c in cams])
    sm = (_capi.Summary * max(npb, 1))()
    Hc = np.empty((npb, 8, 8)); rms = np.empty(npb); st = np.full(n, -99, dtype=np.int32)
    k = None if keep is None else np.ascontiguousarray(np.asarray(keep).astype(np.uint8))
    L.shim_camera_calibrate(C.byref(o), C.byref(co), d(a["corners"]), d(a["board"]), d(a["coff"]), None if k is None else d(k),
                            C.c_longlong(n), d(a["prob_off"]) if prob_off else None, C.c_longlong(npb), cc, d(q), d(t), sm, d(Hc), d(rms),
                            d(st))
    ks = np.array([list(c.proj) + list(c.dist) for c in cc][:npb]).reshape(npb, 8)
    return dict(k=ks, cameras=[with_k(cams[i], ks[i]) for i in range(npb)], q=q, t=t, summaries=sm, H_cam=Hc, rms_px=rms, status=st,
                hold_mask=int(co.hold_mask))


def restatement_problem(cam, a, k, sigma=0.3, keep=None):
    """Problem k of the arrays as camcal_ref takes it (the participating images only) -> (prob, image indices)."""
    idx = [i for i in range(a["prob_off"][k], a["prob_off"][k + 1])
           if a["coff"][i + 1] - a["coff"][i] >= 4 and (keep is None or keep[i])]
    prob = dict(model=cam.model, px=[a["corners"][a["coff"][i]:a["coff"][i + 1]].astype(np.float64) for i in idx],
                board=[a["board"][a["coff"][i]:a["coff"][i + 1]].astype(np.float64) for i in idx], sigma=sigma)
    return prob, idx


def restatement_solve(prob, k0, q0, t0, idx, mask, hold_board=False, also_from=None):
    """The restatement from the same start and, where given, from the answer (scipy stops in shallow valleys: the lower of the two is
    its answer) -> (k, Rs, ts, cost)."""
    Rs0 = [ref.quat_wxyz_to_R(q0[i]) for i in idx]
    ts0 = [np.array(t0[i], dtype=np.float64) for i in idx]
    cand = [ref.solve(prob, k0, Rs0, ts0, hold_mask=mask, hold_board=hold_board)]
    if also_from is not None:
        cand.append(ref.solve(prob, also_from[0], also_from[1], also_from[2], hold_mask=mask, hold_board=hold_board))
    return min(cand, key=lambda c: c[3])


def pose_gap(Rs, ts, q, t, idx):
    return max(max(np.abs(Rs[j] - ref.quat_wxyz_to_R(q[i])).max(), np.abs(ts[j] - t[i]).max()) for j, i in enumerate(idx))


def compare_problem(cam, a, k, s, q0, t0, keep=None, hold_board=False):
    """One problem of a call against the restatement started at the same point -> dict of gaps."""
    mask = s["hold_mask"]
    prob, idx = restatement_problem(cam, a, k, keep=keep)
    mine = (s["k"][k], [ref.quat_wxyz_to_R(s["q"][i]) for i in idx], [s["t"][i].copy() for i in idx])
    kr, Rs, ts, cr = restatement_solve(prob, k_of(cam), q0, t0, idx, mask, hold_board, also_from=mine)
    Hd, _ = ref.normal_matrix(prob, kr, Rs, ts)
    Hr = ref.schur(Hd, mask, hold_board)
    sg = ref.sigmas(Hr, mask)
    free = [j for j in range(8) if not (mask >> j) & 1]
    Hm, _ = ref.normal_matrix(prob, *mine)
    Hs = ref.schur(Hm, mask, hold_board)
    n_corners = sum(len(p) for p in prob["px"])
    return dict(param_sigma=float(np.max(np.abs(mine[0] - kr)[free] / sg[free])) if free else 0.0,
                held_equal=all(mine[0][j] == k_of(cam)[j] for j in range(8) if j not in free),
                cost=abs(s["summaries"][k].final_cost - cr) / cr, cost_mine=s["summaries"][k].final_cost, cost_ref=cr,
                rms=abs(s["rms_px"][k] - 0.3 * np.sqrt(2 * cr / n_corners)) / (0.3 * np.sqrt(2 * cr / n_corners)),
                hcam=np.linalg.norm(s["H_cam"][k] - Hr) / np.linalg.norm(Hr), hcam_same=np.linalg.norm(s["H_cam"][k] - Hs) / np.linalg.norm(Hs),
                pose=pose_gap(Rs, ts, s["q"], s["t"], idx), sigma=sg, k_ref=kr)


# ---- declared, exported, bound -------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clc.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(clc_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", _build.PRODUCT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if len(l.split()) >= 3 and l.split()[-2] == "T"}
    L = _capi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.EXPORTED, name
        assert name in exported, name
        assert getattr(L, name).argtypes is not None, name
    assert "abi_camcal.hip" in _build.UNITS and "clc_camcal.hpp" in _build.SIDE_HEADERS and "clc_camcal.hpp" not in _build.HEADERS
    assert L.clc_version() == 210


def test_struct_layout_and_defaults(shim):
    assert C.sizeof(_capi.CamcalOptions) == 16 == shim.shim_camcal_options_size()
    for model, mask in ((PINHOLE, 0), (KANNALA_BRANDT, 0xC0)):
        for o in (_capi.default_camcal_options(model), shim_options(shim, model)):
            assert (o.sigma_px, o.hold_mask, o.hold_board_poses) == (0.3, mask, 0)
    assert (_capi.CAMCAL_OK, _capi.CAMCAL_TOO_FEW, _capi.CAMCAL_NOT_KEPT, _capi.CAMCAL_NONFINITE) == (1, 0, -1, -2)


# ---- Jacobians -----------------------------------------------------------------------------------------------------------------
def corner_terms(L, cam, pose7, X, Y, u, v, inv_s):
    r, J, JK = np.empty(2), np.empty((2, 6)), np.empty((2, 8))
    c = cam.to_c()
    front = L.shim_camcal_corner(C.byref(c), d(pose7), C.c_double(X), C.c_double(Y), C.c_double(u), C.c_double(v), C.c_double(inv_s), d(r),
                                 d(J), d(JK))
    return r, J, JK, front


@pytest.mark.parametrize("name", CAMS)
def test_jacobians_match_central_differences(shim, name):
    """corner_terms' J (over [dt, dtheta] through the project's Plus) and JK (over the 8 intrinsics) against central differences of its
    own residual, which is cam_project's; the step per column is 1e-6 of the column's scale, the bound 1e-7 of the Jacobian's
    largest entry (central differences of step h leave h^2 times the third derivative: ~1e-9 relative here)."""
    cam = cases.CAMERAS[name]
    inv_s = 1 / 0.3
    worst = 0.0
    for px, b, R, t in cases.images(name, 7, 3):
        pose7 = np.r_[t, ref.R_to_quat_wxyz(R)[[1, 2, 3, 0]]]
        for j in (0, 17, 70, 143):
            X, Y, u, v = float(b[j, 0]), float(b[j, 1]), float(px[j, 0]), float(px[j, 1])
            r, J, JK, front = corner_terms(shim, cam, pose7, X, Y, u, v, inv_s)
            assert front == 1
            # the residual is cam_project's
            want = (H.shim_project(shim, cam, np.array([[X, Y, 0.0]]), pose7)[0] - [u, v]) * inv_s
            assert np.array_equal(r, want)
            num = np.empty((2, 6))
            for c in range(6):
                e = np.zeros(6); e[c] = 1e-6
                out = []
                for sgn in (1, -1):
                    Rp, tp = ref.plus(R, t, sgn * e)
                    p7 = np.r_[tp, ref.R_to_quat_wxyz(Rp)[[1, 2, 3, 0]]]
                    out.append(corner_terms(shim, cam, p7, X, Y, u, v, inv_s)[0])
                num[:, c] = (out[0] - out[1]) / 2e-6
            numk = np.empty((2, 8))
            k = k_of(cam)
            for c in range(8):
                h = 1e-6 * max(1.0, abs(k[c])) if c < 4 else 1e-6
                out = []
                for sgn in (1, -1):
                    kk = k.copy(); kk[c] += sgn * h
                    out.append(corner_terms(shim, with_k(cam, kk), pose7, X, Y, u, v, inv_s)[0])
                numk[:, c] = (out[0] - out[1]) / (2 * h)
            g = max(np.abs(J - num).max() / np.abs(J).max(), np.abs(JK - numk).max() / np.abs(JK).max())
            worst = max(worst, g)
    print(name, "largest relative gap of a Jacobian entry to central differences:", worst)
    assert worst < 1e-7


@pytest.mark.parametrize("name", CAMS)
def test_evaluation_record_matches_dense_normal_matrix(shim, name):
    """One image's record (A, B, g, C, g_c, cost) against J^T J, J^T r of the restatement's analytic Jacobian: 1e-12 relative, the
    rounding of 288 products summed in another order."""
    cam = cases.CAMERAS[name]
    px, b, R, t = cases.images(name, 8, 1)[0]
    pose7 = np.r_[t, ref.R_to_quat_wxyz(R)[[1, 2, 3, 0]]]
    E = np.empty(120)
    c = cam.to_c()
    shim.shim_camcal_eval_image(C.byref(c), C.c_double(0.3), d(px), d(b), C.c_longlong(len(px)), d(pose7), d(E))
    prob = dict(model=cam.model, px=[px.astype(np.float64)], board=[b], sigma=0.3)
    Hd, g = ref.normal_matrix(prob, k_of(cam), [ref.quat_wxyz_to_R(ref.R_to_quat_wxyz(R))], [t])
    iu6, iu8 = np.triu_indices(6), np.triu_indices(8)
    rel = lambda x, y: np.abs(x - y).max() / np.abs(y).max()
    gaps = [rel(E[0:21], Hd[8:, 8:][iu6]), rel(E[21:69].reshape(6, 8), Hd[8:, :8]), rel(E[69:75], g[8:]), rel(E[75:111], Hd[:8, :8][iu8]),
            rel(E[111:119], g[:8]), abs(E[119] - ref.cost(prob, k_of(cam), [R], [t])) / E[119]]
    print(name, gaps)
    assert max(gaps) < 1e-12


# ---- against the restatement ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded_runs(shim):
    """Per camera: [(images, arrays, q0, t0, result from K10's poses under the true camera)] for the seeded sets."""
    out = {}
    for name in CAMS:
        cam = cases.CAMERAS[name]
        runs = []
        for imgs in cases.seeded(name):
            a = cases.arrays([imgs])
            q0, t0, st = start_poses(shim, cam, a)
            assert np.all(st == 1)
            runs.append((imgs, a, q0, t0, shim_calibrate(shim, [cam], a, q0, t0)))
        out[name] = runs
    return out


@pytest.mark.parametrize("name", CAMS)
def test_seeded_sets_match_restatement(seeded_runs, name):
    """The minimiser, cost, RMS and H_cam of the host build against scipy's, default masks, 6 / 12 / 20 images.  Measured (worst of the
    three sets): radtan |dk| / sigma 1.08e-6, cost 2.5e-15, RMS 1.3e-15, H_cam 3.0e-9 (8.9e-15 at the same point); kb 7.7e-7, 1.39e-14,
    7.0e-15, 3.24e-9 (1.42e-14).  The 20-image sets set the parameter gap (scipy's own stopping); the 6- and 12-image sets agree to 2e-9
    of a sigma or better."""
    cam = cases.CAMERAS[name]
    for imgs, a, q0, t0, s in seeded_runs[name]:
        sm = s["summaries"][0]
        assert sm.termination in (1, 2, 3) and np.all(s["status"] == 1)
        g = compare_problem(cam, a, 0, s, q0, t0)
        print(name, len(imgs), "images:", {k: v for k, v in g.items() if k not in ("sigma", "k_ref")}, "iterations", sm.num_iterations)
        print("   sigma", g["sigma"], "\n   k - truth", s["k"][0] - k_of(cam))
        assert g["param_sigma"] < PARAM_BOUND_SIGMA and g["held_equal"]
        assert g["cost"] < COST_BOUND and g["rms"] < RMS_BOUND
        assert g["hcam"] < HCAM_BOUND and g["hcam_same"] < HCAM_SAME_POINT
        assert np.array_equal(s["H_cam"][0], s["H_cam"][0].T)
        # the fit is well posed: the truth lies within a few sigma of the minimiser
        free = [j for j in range(8) if not (s["hold_mask"] >> j) & 1]
        assert np.all(np.abs(s["k"][0] - k_of(cam))[free] < 5 * g["sigma"][free])


# ---- hold masks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CAMS)
def test_all_intrinsics_held_is_the_pixel_space_pnp(shim, seeded_runs, name):
    cam = cases.CAMERAS[name]
    imgs, a, q0, t0, _ = seeded_runs[name][0]
    s = shim_calibrate(shim, [cam], a, q0, t0, co=shim_options(shim, cam.model, hold_mask=0xFF))
    assert np.array_equal(s["k"][0], k_of(cam)) and np.all(s["H_cam"][0] == 0.0)
    prob, idx = restatement_problem(cam, a, 0)
    worst = 0.0
    for j, i in enumerate(idx):  # the poses decouple: one small solve per image
        one = dict(model=cam.model, px=[prob["px"][j]], board=[prob["board"][j]], sigma=0.3)
        _, Rs, ts, _ = ref.solve(one, k_of(cam), [ref.quat_wxyz_to_R(q0[i])], [t0[i].copy()], hold_mask=0xFF)
        worst = max(worst, pose_gap(Rs, ts, s["q"], s["t"], [i]))
    print(name, "pose gap to the per-image pixel-space PnP:", worst)
    assert worst < POSE_BOUND


@pytest.mark.parametrize("name", CAMS)
def test_held_board_poses_keep_their_bits(shim, seeded_runs, name):
    cam = cases.CAMERAS[name]
    imgs, a, q0, t0, _ = seeded_runs[name][1]
    start = with_k(cam, k_of(cam) + [3.0, -2.0, 1.5, -1.0, 0, 0, 0, 0])
    s = shim_calibrate(shim, [start], a, q0, t0, co=shim_options(shim, cam.model, hold_board_poses=1))
    assert np.array_equal(s["q"], q0) and np.array_equal(s["t"], t0) and s["summaries"][0].termination in (1, 2, 3)
    g = compare_problem(start, a, 0, s, q0, t0, hold_board=True)
    print(name, {k: v for k, v in g.items() if k not in ("sigma", "k_ref")})
    assert g["param_sigma"] < PARAM_BOUND_SIGMA and g["cost"] < COST_BOUND and g["hcam"] < HCAM_BOUND


@pytest.mark.parametrize("name", CAMS)
def test_each_single_held_bit_keeps_that_parameter(shim, seeded_runs, name):
    cam = cases.CAMERAS[name]
    imgs, a, q0, t0, base = seeded_runs[name][0]
    default = shim_options(shim, cam.model).hold_mask
    start = with_k(cam, k_of(cam) * (1 + 1e-3 * np.array([1, -1, 1, -1, 1, -1, 0, 0])))
    for j in range(8):
        mask = default | (1 << j)
        s = shim_calibrate(shim, [start], a, q0, t0, co=shim_options(shim, cam.model, hold_mask=mask))
        assert s["summaries"][0].termination in (1, 2, 3), j
        held = [i for i in range(8) if (mask >> i) & 1]
        assert all(s["k"][0][i] == k_of(start)[i] for i in held), j
        assert np.all(s["H_cam"][0][held, :] == 0.0) and np.all(s["H_cam"][0][:, held] == 0.0)
        moved = [i for i in range(8) if i not in held and k_of(start)[i] != k_of(cam)[i]]
        assert all(s["k"][0][i] != k_of(start)[i] for i in moved), j


@pytest.mark.parametrize("mask", [0xFE, 0xFC, 0xF8, 0xF0])
@pytest.mark.parametrize("name", CAMS)
def test_one_to_four_free_intrinsics_match_restatement(shim, seeded_runs, name, mask):
    """1, 2, 3 and 4 free intrinsics (fx; fx fy; fx fy cx; fx fy cx cy; the rest held at the start's values): the reduced solves of those sizes,
    which the masks above (0, 5, 6, 7 and 8 free) do not reach, against the restatement at the bounds of the held-board-poses test
    above (parameters, cost, H_cam).  H_cam at the answer's own point is printed, not held to HCAM_SAME_POINT: that bound was measured
    where the large distortion entries carry the norm; over fx, fy, cx, cy alone, whose information the poses absorb almost wholly
    (C and the sum of the B^T A^-1 B cancel), the gap is 3.1e-13 (kb, 3 and 4 free)."""
    cam = cases.CAMERAS[name]
    imgs, a, q0, t0, _ = seeded_runs[name][1]
    start = with_k(cam, k_of(cam) + [3.0, -2.0, 1.5, -1.0, 0, 0, 0, 0])
    s = shim_calibrate(shim, [start], a, q0, t0, co=shim_options(shim, cam.model, hold_mask=mask))
    assert s["summaries"][0].termination in (1, 2, 3)
    g = compare_problem(start, a, 0, s, q0, t0)
    print(name, "free", 8 - bin(mask).count("1"), {k: v for k, v in g.items() if k not in ("sigma", "k_ref")})
    assert g["held_equal"] and all(s["k"][0][j] != k_of(start)[j] for j in range(8) if not (mask >> j) & 1)
    assert g["param_sigma"] < PARAM_BOUND_SIGMA and g["cost"] < COST_BOUND and g["hcam"] < HCAM_BOUND


def test_kb_nothing_held_only_lowers_the_cost(shim, seeded_runs):
    """k4 and k5 are not observable in this field of view: with nothing held only the cost is asserted (<= the default mask's)."""
    cam = cases.CAMERAS["kb"]
    for imgs, a, q0, t0, base in seeded_runs["kb"]:
        s = shim_calibrate(shim, [cam], a, q0, t0, co=shim_options(shim, cam.model, hold_mask=0))
        print(len(imgs), "images: cost", s["summaries"][0].final_cost, "<=", base["summaries"][0].final_cost, "k", s["k"][0][4:])
        assert s["summaries"][0].termination in (1, 2, 3)
        assert s["summaries"][0].final_cost <= base["summaries"][0].final_cost * (1 + 1e-12)


# ---- the closed-form start -----------------------------------------------------------------------------------------------------
def shim_guess(L, cam, a):
    n = len(a["coff"]) - 1
    Hh, st, nu = np.empty((n, 9)), np.empty(n, dtype=np.int32), C.c_int(0)
    f = L.shim_camera_guess(C.c_int(cam.width), C.c_int(cam.height), d(a["corners"]), d(a["board"]), d(a["coff"]), C.c_longlong(n), d(Hh),
                            d(st), C.byref(nu))
    return f, Hh, st, nu.value


@pytest.mark.parametrize("name", CAMS)
def test_guess_matches_restatement_formula(shim, seeded_runs, name):
    """The DLT by Jacobi eigenvectors of the normal matrix against the restatement's SVD of the design matrix, both Hartley-normalized:
    measured 3.95e-15 relative on the focal length at worst (tests/test_campose_host.py compares K10's DLT only through the pose it
    starts; the figure here is this test's own measurement)."""
    cam = cases.CAMERAS[name]
    for imgs, a, _, _, _ in seeded_runs[name]:
        f, Hh, st, used = shim_guess(shim, cam, a)
        fr, ur = ref.guess(cam.width, cam.height, [i[0] for i in imgs], [i[1] for i in imgs])
        print(name, len(imgs), "images: f", f, "restatement", fr, "true", cam.proj[:2])
        assert used == ur == len(imgs) and np.all(st == 1)
        assert abs(f - fr) / fr < GUESS_BOUND
        assert np.allclose(np.linalg.norm(Hh, axis=1), 1.0, rtol=1e-14, atol=0)
        assert abs(f - cam.proj[0]) < cam.proj[0] / 3  # a start, not an estimate


def test_guess_degenerate_inputs(shim):
    cam = cases.CAMERAS["radtan"]
    imgs = cases.images("radtan", 9, 3)
    line = (imgs[1][0][:8], np.stack([np.linspace(0, 0.4, 8), np.zeros(8)], 1).astype(np.float32), None, None)  # collinear board points
    a = cases.arrays([[imgs[0], line, (imgs[2][0][:3], imgs[2][1][:3], None, None)]])
    f, Hh, st, used = shim_guess(shim, cam, a)
    assert st.tolist() == [1, -1, 0] and used == 1 and np.isnan(f) and np.all(np.isnan(Hh[1:]))


@pytest.mark.parametrize("name", CAMS)
def test_flow_from_the_guess_reaches_the_same_minimiser(shim, seeded_runs, name):
    """CalibrateCamera's flow in the shim — the guess, K10's poses under it, the solve — against the solve from the true camera (for
    kb with the held k4, k5 at the guess's zeros in both, the same problem).  Measured: radtan 8.7e-9 of a sigma to the
    solve from the truth, 7.9e-9 to the restatement from the guess, cost 9.4e-15; kb (the seed as it is: the restatement converges
    from the guess too) 1.4e-9, 1.71e-7, 6.7e-15."""
    cam = cases.CAMERAS[name]
    imgs, a, _, _, _ = seeded_runs[name][1]
    mask = shim_options(shim, cam.model).hold_mask
    truth = with_k(cam, [0.0 if (mask >> j) & 1 else v for j, v in enumerate(k_of(cam))])
    q0, t0, st = start_poses(shim, truth, a)
    s_true = shim_calibrate(shim, [truth], a, q0, t0)
    f, _, _, _ = shim_guess(shim, cam, a)
    g = Camera(cam.model, (f, f, cam.width / 2.0, cam.height / 2.0), (0.0, 0.0, 0.0, 0.0), cam.width, cam.height)
    q1, t1, st1 = start_poses(shim, g, a)
    s = shim_calibrate(shim, [g], a, q1, t1, keep=st1 == 1)
    assert np.all(st1 == 1) and s["summaries"][0].termination in (1, 2, 3)
    prob, idx = restatement_problem(cam, a, 0)
    kr, Rs, ts, cr = restatement_solve(prob, k_of(g), q1, t1, idx, mask)
    Hd, _ = ref.normal_matrix(prob, kr, Rs, ts)
    sg = ref.sigmas(ref.schur(Hd, mask), mask)
    free = [j for j in range(8) if not (mask >> j) & 1]
    gap = np.max(np.abs(s["k"][0] - s_true["k"][0])[free] / sg[free])
    gap_ref = np.max(np.abs(s["k"][0] - kr)[free] / sg[free])
    cgap = abs(s["summaries"][0].final_cost - s_true["summaries"][0].final_cost) / s_true["summaries"][0].final_cost
    print(name, "from the guess f =", f, ": |dk| / sigma to the solve from the truth", gap, "to the restatement from the guess", gap_ref,
          "cost", cgap, "iterations", s["summaries"][0].num_iterations)
    assert gap < GUESS_FLOW_SIGMA and gap_ref < GUESS_FLOW_SIGMA and cgap < GUESS_FLOW_COST


# ---- images that take no part, failures ----------------------------------------------------------------------------------------
def test_images_that_take_no_part(shim):
    cam = cases.CAMERAS["radtan"]
    imgs = cases.images("radtan", 31, 9)
    three = (imgs[1][0][:3], imgs[1][1][:3], None, None)
    nan = (imgs[3][0].copy(), imgs[3][1], None, None)
    nan[0][5, 1] = np.nan
    p0 = [imgs[0], three, imgs[2], nan, imgs[4], imgs[5], imgs[6], imgs[7]]
    p1 = [three, imgs[8]]  # nothing takes part: 3 corners, keep = 0
    a = cases.arrays([p0, p1])
    keep = np.ones(10, dtype=bool); keep[5] = False; keep[9] = False
    q0, t0, st = start_poses(shim, cam, a)
    q0[3] = [1, 0, 0, 0]; t0[3] = [0, 0, 1]
    s = shim_calibrate(shim, [cam, cam], a, q0, t0, keep=keep)
    assert s["status"].tolist() == [1, 0, 1, -2, 1, -1, 1, 1, 0, -1]
    for i in (1, 3, 5, 8, 9):
        assert np.array_equal(s["q"][i], q0[i]) and np.array_equal(s["t"][i], t0[i])
    assert s["summaries"][0].termination in (1, 2, 3) and s["summaries"][1].termination == 6
    assert np.array_equal(s["k"][1], k_of(cam)) and np.all(np.isnan(s["H_cam"][1])) and np.isnan(s["rms_px"][1])
    # the same as the good images alone, and as one problem without problem offsets
    good = [0, 2, 4, 6, 7]
    ag = cases.arrays([[p0[i] for i in good]])
    for po in (True, False):
        sg = shim_calibrate(shim, [cam], ag, q0[good], t0[good], prob_off=po)
        assert np.array_equal(sg["q"], s["q"][good]) and np.array_equal(sg["t"], s["t"][good]) and np.array_equal(sg["k"][0], s["k"][0])
        assert np.array_equal(sg["H_cam"][0], s["H_cam"][0]) and sg["rms_px"][0] == s["rms_px"][0]
    # a non-finite camera or an unknown model: CLC_FAILURE, every bit kept
    for bad in (with_k(cam, np.r_[np.nan, k_of(cam)[1:]]), Camera(7, cam.proj, cam.dist)):
        sb = shim_calibrate(shim, [bad], ag, q0[good], t0[good])
        assert sb["summaries"][0].termination == 6 and np.array_equal(sb["q"], q0[good]) and np.array_equal(sb["t"], t0[good])
        assert np.array_equal(sb["k"][0], k_of(bad), equal_nan=True)
    # a start behind the camera is an invalid evaluation: CLC_FAILURE
    tb = t0[good].copy(); tb[:, 2] *= -1
    sb = shim_calibrate(shim, [cam], ag, q0[good], tb)
    assert sb["summaries"][0].termination == 6 and np.array_equal(sb["t"], tb) and np.array_equal(sb["k"][0], k_of(cam))


def calibrate_call(L, co, h=None, opt=None, **kw):
    z = np.zeros(2, dtype=np.int64)
    cam = (ClcCamera * 1)(H.CAMERAS["pinhole"].to_c())
    args = dict(coff=d(z), q=d(np.zeros(4)), t=d(np.zeros(3)), cams=cam, sm=(_capi.Summary * 1)(), st=d(np.zeros(1, np.int32)), prob=None,
                n_images=1, n_problems=1)
    args.update(kw)
    return L.clc_camera_calibrate(h, opt, C.byref(co) if co is not None else None, None, None, args["coff"], None,
                                  C.c_size_t(args["n_images"]), args["prob"], C.c_size_t(args["n_problems"]), args["cams"], args["q"],
                                  args["t"], args["sm"], None, None, args["st"])


def test_refusals_need_no_device():
    """NULL required pointers, a sigma that is not finite and positive, a mask of all 8 bits with hold_board_poses, mask bits beyond
    the 8, offsets that decrease, an unknown model: CLC_ERR_INVALID_ARG before any device work (the handle is NULL throughout)."""
    L = _capi.lib()
    who = "clc_camera_calibrate: "
    base = _capi.default_camcal_options(PINHOLE)
    for v in (float("nan"), float("inf"), 0.0, -0.3):
        assert calibrate_call(L, _capi.CamcalOptions(v, 0, 0)) == -1 and L.clc_last_error().decode() == who + "sigma_px must be finite and > 0"
    assert calibrate_call(L, _capi.CamcalOptions(0.3, 0xFF, 1)) == -1 and L.clc_last_error().decode() == who + "everything is held"
    assert calibrate_call(L, _capi.CamcalOptions(0.3, 0x100, 0)) == -1 and "beyond the 8" in L.clc_last_error().decode()
    bad = np.array([3, 1], dtype=np.int64)
    for kw in (dict(coff=d(bad)), dict(prob=d(bad))):
        assert calibrate_call(L, base, **kw) == -1 and L.clc_last_error().decode() == who + "offsets not monotone"
    for key in ("coff", "q", "t", "cams", "sm", "st"):
        assert calibrate_call(L, base, **{key: None}) == -1 and L.clc_last_error().decode() == who + "bad argument"
    unknown = (ClcCamera * 1)(Camera(3, (1.0, 1.0, 0.0, 0.0), (0.0,) * 4).to_c())
    assert calibrate_call(L, base, cams=unknown) == -1 and L.clc_last_error().decode() == who + "unknown camera model"
    assert calibrate_call(L, base, n_problems=2) == -1  # several problems need problem_offsets
    # good arguments (copt NULL: the defaults): the call gets as far as the missing handle
    for co in (base, None, _capi.CamcalOptions(0.3, 0xFF, 0)):
        assert calibrate_call(L, co) == -1 and L.clc_last_error().decode() == who + "bad argument"
    # the device form and the guess
    V = C.c_void_p
    one = V(8)  # never dereferenced: the handle is NULL
    dev = lambda co: L.clc_camera_calibrate_device(None, None, C.byref(co), one, one, one, None, C.c_size_t(1), None, C.c_size_t(1), one, one,
                                                   one, one, None, None, one)
    assert dev(_capi.CamcalOptions(0.0, 0, 0)) == -1 and "sigma_px" in L.clc_last_error().decode()
    assert dev(_capi.CamcalOptions(0.3, 0xFF, 1)) == -1 and "everything is held" in L.clc_last_error().decode()
    assert dev(base) == -1 and L.clc_last_error().decode() == "clc_camera_calibrate_device: bad argument"
    cam, used, z = ClcCamera(), C.c_int32(0), np.zeros(3, dtype=np.int64)
    guess = lambda fn, model, w, h, cam_out: fn(None, C.c_int32(model), C.c_int32(w), C.c_int32(h), one, one, d(z), C.c_size_t(2), cam_out,
                                                C.byref(used))
    for fn, nm in ((L.clc_camera_guess, "clc_camera_guess: "), (L.clc_camera_guess_device, "clc_camera_guess_device: ")):
        assert guess(fn, 3, 752, 480, C.byref(cam)) == -1 and L.clc_last_error().decode() == nm + "unknown camera model"
        assert guess(fn, PINHOLE, 0, 480, C.byref(cam)) == -1 and L.clc_last_error().decode() == nm + "width and height must be > 0"
        assert guess(fn, PINHOLE, 752, 480, None) == -1 and L.clc_last_error().decode() == nm + "bad argument"
        assert guess(fn, PINHOLE, 752, 480, C.byref(cam)) == -1 and L.clc_last_error().decode() == nm + "bad argument"  # the handle


def test_sanitized_standalone_program(tmp_path):
    """tests/shim/camcal_sanitize_main.cpp: the per-problem host function and the closed-form start on the edge shapes, every array of
    its exact size, built with -fsanitize=address,undefined and run as an ordinary process."""
    exe = str(tmp_path / "camcal_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "shim", "camcal_sanitize_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "shapes ok" in p.stdout, p.stdout


# ---- YAML ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("golden", ["camera_radtan.yaml", "camera_kannala_brandt.yaml", "camera_pinhole.yaml"])
def test_camera_yaml_round_trip(tmp_path, golden):
    cam = Camera.from_yaml(os.path.join(HERE, "golden", golden))
    # values that need all 17 digits
    odd = Camera(cam.model, tuple(v * (1 + 2.0 ** -50) + 1e-13 for v in cam.proj), tuple(v / 3.0 for v in cam.dist), cam.width, cam.height)
    for c in (cam, odd):
        path = str(tmp_path / "out.yaml")
        c.to_yaml(path)
        assert Camera.from_yaml(path) == c
        assert open(path).readline().strip() == "%YAML:1.0"
    with pytest.raises(ValueError):
        Camera(9, cam.proj, cam.dist).to_yaml(str(tmp_path / "bad.yaml"))
