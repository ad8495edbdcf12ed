"""K19 on the MI355X: clc_camera_calibrate and clc_camera_guess against the host build of the same code (tests/shim/camcal_shim.cpp)
and the restatement (tests/camcal_ref.py) on one batch per camera model sized to go wrong at the wave, lane and thread edges (images
per problem W-1, W, W+1 and T+1; corners per image 3, 4, 63, 64, 65, 144; keep with holes; a problem with every image dropped), the
1- and 2-image problems with the distortion held (cost only); two runs and a problem alone against the batch, bit for bit; batches of
1, 2 and 257 problems; the device-array form behind offsets above 0; the closed-form start in both forms; calib.CalibrateCamera end
to end; the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import camcal_cases as cases  # noqa: E402
import camcal_ref as ref  # noqa: E402
import test_camcal_host as CH  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi, calib  # noqa: E402
from camlasercalibratool_amd.camera import ClcCamera  # noqa: E402

pytestmark = pytest.mark.gpu
CAMS = CH.CAMS
# Measured on the MI355X on these batches, worst of both cameras (the figures: the docstrings of the tests that assert them), asserted
# one decade above; a parameter's bound is in units of its own 1 sigma from H_cam and stays below 1e-3 of it, the cost bounds inside
# the project's 1e-8 relative gate.
GPU_PARAM_SIGMA = 5.5e-6        # device against the restatement's minimiser, |dk| / sigma_k (5.44e-7)
GPU_COST_BOUND = 6.9e-13        # relative, final cost against the restatement (6.82e-14)
GPU_RMS_BOUND = 3.5e-13         # relative, RMS in pixels against the restatement (3.41e-14)
GPU_HCAM_BOUND = 7.9e-8         # relative (Frobenius), H_cam against the dense Schur complement at the restatement's minimiser (7.82e-9)
GPU_HOST_PARAM_SIGMA = 4.6e-5   # device against the host build, |dk| / sigma_k (4.6e-6: the two stop at different iterations)
GPU_HOST_COST_BOUND = 3.1e-12   # device against the host build, relative final cost (3.69e-14 here, 3.04e-13 over the 257 problems)
GPU_HOST_HCAM_BOUND = 9.3e-7    # device against the host build, H_cam relative in the Frobenius norm (9.3e-8: it moves with the point)
GPU_HOST_POSE_BOUND = 2e-7      # device against the host build, any quaternion or t component (1.93e-8)
GPU_FEW_COST_BOUND = 3.4e-12    # 1 and 2 images, distortion held: relative final cost against host build and restatement (3.35e-13)
GPU_GUESS_BOUND = CH.GUESS_BOUND  # the closed-form focal length against the host build: the DLT's measured agreement of the host test
                                  # (the device returned the host build's bits on all four sets)
assert max(GPU_PARAM_SIGMA, GPU_HOST_PARAM_SIGMA) <= CH.SIGMA_GATE and max(GPU_COST_BOUND, GPU_HOST_COST_BOUND, GPU_FEW_COST_BOUND) <= CH.COST_GATE
# The pose options with 200 iterations instead of 50: the shapes in which the intrinsics are barely observable (1 - 3 images, T + 1
# images of four tags) descend along nearly flat valleys; the well-posed problems stop after 7-17 either way.
ITERATIONS = 200
RESTATED_IMAGES = 16  # the restatement is dense: problems of up to 8 + 6 * 16 parameters are compared with it
DIST_HELD = 0xF0


@pytest.fixture(scope="module")
def sv():
    with clc.Solver(0) as s:
        yield s


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return CH.build_shim(str(tmp_path_factory.mktemp("ccg") / "libcamcal_shim.so"))


def pose_options():
    o = _capi.default_pose_options()
    o.max_num_iterations = ITERATIONS
    return o


def prepare(shim, name, problems, keep_fn=None, mask=None):
    """One call's inputs and the host build's result: the start camera of cases.start_camera, the start poses by the shim's K10."""
    cam = cases.CAMERAS[name]
    start = cases.start_camera(cam)
    a = cases.arrays(problems)
    n = len(a["coff"]) - 1
    keep = np.ones(n, bool)
    if keep_fn:
        keep_fn(a, keep)
    q0, t0, st = CH.start_poses(shim, start, a)
    bad = st != 1
    q0[bad] = [1, 0, 0, 0]; t0[bad] = [0, 0, 1]
    co = CH.shim_options(shim, cam.model)
    if mask is not None:
        co.hold_mask |= mask
    cams = [start] * len(problems)
    return dict(cam=cam, start=start, cams=cams, problems=problems, a=a, keep=keep, q0=q0, t0=t0, co=co,
                s=CH.shim_calibrate(shim, cams, a, q0, t0, keep=keep, co=co, max_iterations=ITERATIONS))


@pytest.fixture(scope="module")
def batch(shim):
    out = {}
    for name in CAMS:
        problems, notes = cases.edge_problems(name)

        def keep_fn(a, keep):
            keep[a["prob_off"][notes["holes"]] + np.array([1, 4])] = False
            keep[a["prob_off"][notes["dropped"]]:a["prob_off"][notes["dropped"] + 1]] = False

        out[name] = prepare(shim, name, problems, keep_fn)
        out[name]["notes"] = notes
    return out


def device(sv, e, sel=None):
    """The host-array form on the batch (sel: a subset of its problems, in order)."""
    a = e["a"]
    if sel is None:
        r = sv.camera_calibrate(e["cams"], a["corners"], a["board"], a["coff"], e["q0"], e["t0"], problem_offsets=a["prob_off"],
                                keep=e["keep"], camcal=e["co"], options=pose_options())
    else:
        img = np.concatenate([np.arange(a["prob_off"][k], a["prob_off"][k + 1]) for k in sel])
        ci = np.concatenate([np.arange(a["coff"][i], a["coff"][i + 1]) for i in img])
        co = np.concatenate([[0], np.cumsum([a["coff"][i + 1] - a["coff"][i] for i in img])]).astype(np.int64)
        pr = np.concatenate([[0], np.cumsum([a["prob_off"][k + 1] - a["prob_off"][k] for k in sel])]).astype(np.int64)
        r = sv.camera_calibrate([e["cams"][k] for k in sel], a["corners"][ci], a["board"][ci], co, e["q0"][img], e["t0"][img],
                                problem_offsets=pr, keep=e["keep"][img], camcal=e["co"], options=pose_options())
        r["images"] = img
    r["k"] = np.array([CH.k_of(c) for c in r["cameras"]])
    r["hold_mask"] = int(e["co"].hold_mask)
    return r


def same_bits(x, y, images=None, problems=None):
    """x (a run on a subset, or a whole run) against the whole run y."""
    ii = slice(None) if images is None else images
    pp = slice(None) if problems is None else problems
    for key in ("q", "t", "status"):
        assert np.array_equal(x[key], y[key][ii]), key
    for key in ("k", "H_cam", "rms_px"):
        assert np.array_equal(x[key], y[key][pp], equal_nan=True), key
    ys = [y["summaries"][k] for k in (range(len(y["k"])) if problems is None else problems)]
    for k, smy in enumerate(ys):
        smx = x["summaries"][k]
        assert (smx.termination, smx.num_iterations, smx.num_evaluations, smx.final_cost, smx.initial_cost) == \
               (smy.termination, smy.num_iterations, smy.num_evaluations, smy.final_cost, smy.initial_cost), k


def host_gaps(e, g, k, free):
    """Problem k of the device run g against the host build's e["s"] -> (|dk| / sigma, cost, H_cam, pose)."""
    s, a = e["s"], e["a"]
    sl = slice(a["prob_off"][k], a["prob_off"][k + 1])
    sg = ref.sigmas(g["H_cam"][k], g["hold_mask"])
    pg = np.max(np.abs(g["k"][k] - s["k"][k])[free] / sg[free]) if free else 0.0
    cg = abs(g["summaries"][k].final_cost - s["summaries"][k].final_cost) / s["summaries"][k].final_cost
    hg = np.linalg.norm(g["H_cam"][k] - s["H_cam"][k]) / np.linalg.norm(s["H_cam"][k])
    qg = max(np.abs(g["q"][sl] - s["q"][sl]).max(), np.abs(g["t"][sl] - s["t"][sl]).max())
    return pg, cg, hg, qg


@pytest.mark.parametrize("name", CAMS)
def test_batch_matches_host_build_and_restatement(sv, batch, name):
    """Every problem of the batch: the statuses are the host build's; the intrinsics (in units of their sigma), final cost, H_cam and
    poses against the host build; for the problems of up to RESTATED_IMAGES images the minimiser, cost, RMS and H_cam against the
    restatement from the same start.  The problem of T + 1 images (1 550 parameters) is held against the host build, and its cost
    against the restatement's residuals at its own point.
    Measured on the MI355X (radtan / kb), worst problem: against the host build |dk| / sigma 2.19e-7 / 4.6e-6, cost 7.8e-15 / 3.69e-14,
    H_cam 1.45e-9 / 3.44e-8, pose 5.0e-10 / 1.2e-8 (device and host build contract multiply-adds differently and stop 0-7 iterations
    apart); against the restatement |dk| / sigma 2.62e-7 / 5.44e-7, cost 9.9e-15 / 6.82e-14, RMS 4.9e-15 / 3.41e-14, H_cam
    1.39e-9 / 7.82e-9."""
    e = batch[name]
    a, notes = e["a"], e["notes"]
    g = device(sv, e)
    s = e["s"]
    assert np.array_equal(g["status"], s["status"])
    free = [j for j in range(8) if not (g["hold_mask"] >> j) & 1]
    worst = dict(host_param=0.0, host_cost=0.0, host_hcam=0.0, host_pose=0.0, param=0.0, cost=0.0, rms=0.0, hcam=0.0)
    for nm, k in notes.items():
        sm, sl = g["summaries"][k], slice(a["prob_off"][k], a["prob_off"][k + 1])
        if nm == "dropped":
            assert sm.termination == 6 and np.all(g["status"][sl] == -1) and np.array_equal(g["k"][k], CH.k_of(e["start"]))
            assert np.array_equal(g["q"][sl], e["q0"][sl]) and np.array_equal(g["t"][sl], e["t0"][sl])
            assert np.all(np.isnan(g["H_cam"][k])) and np.isnan(g["rms_px"][k])
            continue
        assert sm.termination in (1, 2, 3) and s["summaries"][k].termination in (1, 2, 3), (nm, sm.termination)
        pg, cg, hg, qg = host_gaps(e, g, k, free)
        print(name, nm, "vs host build: |dk|/sigma %.3g cost %.3g H_cam %.3g pose %.3g" % (pg, cg, hg, qg), "iterations", sm.num_iterations,
              s["summaries"][k].num_iterations)
        worst.update(host_param=max(worst["host_param"], pg), host_cost=max(worst["host_cost"], cg), host_hcam=max(worst["host_hcam"], hg),
                     host_pose=max(worst["host_pose"], qg))
        drop = ~e["keep"][sl] | (np.diff(a["coff"])[sl] < 4)
        assert np.array_equal(g["q"][sl][drop], e["q0"][sl][drop]) and np.array_equal(g["t"][sl][drop], e["t0"][sl][drop])
        if sl.stop - sl.start <= RESTATED_IMAGES:
            c = CH.compare_problem(e["start"], a, k, g, e["q0"], e["t0"], keep=e["keep"])
            print("   vs restatement:", {x: float("%.3g" % c[x]) for x in ("param_sigma", "cost", "rms", "hcam")})
            worst.update(param=max(worst["param"], c["param_sigma"]), cost=max(worst["cost"], c["cost"]), rms=max(worst["rms"], c["rms"]),
                         hcam=max(worst["hcam"], c["hcam"]))
        else:
            prob, idx = CH.restatement_problem(e["start"], a, k, keep=e["keep"])
            cr = ref.cost(prob, g["k"][k], [ref.quat_wxyz_to_R(g["q"][i]) for i in idx], [g["t"][i] for i in idx])
            worst["cost"] = max(worst["cost"], abs(sm.final_cost - cr) / cr)
    print(name, "worst:", {x: float("%.3g" % v) for x, v in worst.items()})
    assert worst["host_param"] < GPU_HOST_PARAM_SIGMA and worst["host_cost"] < GPU_HOST_COST_BOUND
    assert worst["host_hcam"] < GPU_HOST_HCAM_BOUND and worst["host_pose"] < GPU_HOST_POSE_BOUND
    assert worst["param"] < GPU_PARAM_SIGMA and worst["cost"] < GPU_COST_BOUND and worst["rms"] < GPU_RMS_BOUND
    assert worst["hcam"] < GPU_HCAM_BOUND


@pytest.mark.parametrize("name", CAMS)
def test_few_image_problems_compare_the_cost(sv, shim, name):
    """1 and 2 images cannot fix the intrinsics even with the distortion held (a planar view gives 8 numbers, pose and fx fy cx cy are
    10): the minimiser is a valley, only the cost is compared — with the host build and with the restatement from the device's point.
    Measured on the MI355X: radtan 8.3e-15 / 5.3e-15 (host build / restatement), kb 3.35e-13 / 3.17e-14."""
    e = prepare(shim, name, cases.few_image_problems(name), mask=DIST_HELD)
    g = device(sv, e)
    assert np.array_equal(g["status"], e["s"]["status"]) and np.all(g["status"] == 1)
    for k in range(2):
        sm = g["summaries"][k]
        assert sm.termination in (1, 2, 3, 4)
        held = [j for j in range(8) if (g["hold_mask"] >> j) & 1]
        assert all(g["k"][k][j] == CH.k_of(e["start"])[j] for j in held)
        prob, idx = CH.restatement_problem(e["start"], e["a"], k)
        mine = (g["k"][k], [ref.quat_wxyz_to_R(g["q"][i]) for i in idx], [g["t"][i].copy() for i in idx])
        cr = min(ref.cost(prob, *mine), ref.solve(prob, *mine, hold_mask=g["hold_mask"])[3])
        hc = abs(sm.final_cost - e["s"]["summaries"][k].final_cost) / sm.final_cost
        rc = abs(sm.final_cost - cr) / cr
        print(name, k + 1, "images: cost", sm.final_cost, "vs host build %.3g vs restatement %.3g" % (hc, rc), "iterations", sm.num_iterations)
        assert hc < GPU_FEW_COST_BOUND and rc < GPU_FEW_COST_BOUND


@pytest.mark.parametrize("name", CAMS)
def test_two_runs_and_a_problem_alone_have_the_same_bits(sv, batch, name):
    e = batch[name]
    g = device(sv, e)
    same_bits(device(sv, e), g)
    a, notes = e["a"], e["notes"]
    for sel in ([notes["seeded"]], [notes["corners"], notes["dropped"]], [notes["threads+1"]]):  # calls of 1, 2 and 1 problems
        one = device(sv, e, sel)
        same_bits(one, g, images=one["images"], problems=sel)


@pytest.mark.parametrize("name", CAMS)
def test_many_small_problems(sv, shim, name):
    """257 problems of 4 images x 36 corners in one call against the host build.  Measured on the MI355X (radtan / kb): |dk| / sigma
    1.36e-6 / 3.23e-6, cost 2.63e-14 / 3.04e-13, H_cam 4.52e-8 / 9.3e-8, pose 1.16e-8 / 1.93e-8."""
    e = prepare(shim, name, cases.small_problems(name))
    g = device(sv, e)
    assert np.array_equal(g["status"], e["s"]["status"])
    free = [j for j in range(8) if not (g["hold_mask"] >> j) & 1]
    worst = np.zeros(4)
    for k in range(len(e["problems"])):
        assert g["summaries"][k].termination in (1, 2, 3) and e["s"]["summaries"][k].termination in (1, 2, 3), k
        worst = np.maximum(worst, host_gaps(e, g, k, free))
    print(name, "257 problems vs host build: |dk|/sigma %.3g cost %.3g H_cam %.3g pose %.3g" % tuple(worst))
    assert worst[0] < GPU_HOST_PARAM_SIGMA and worst[1] < GPU_HOST_COST_BOUND and worst[2] < GPU_HOST_HCAM_BOUND and worst[3] < GPU_HOST_POSE_BOUND


@pytest.mark.parametrize("name", CAMS)
def test_device_form_behind_offsets(sv, batch, name):
    """Every array, the cameras included, in device memory; the call's images and corners behind pads (problem_offsets[0] and the
    corner offsets above 0): the bits of the host-array call.  Then one problem without problem_offsets, and zero problems."""
    import torch
    e = batch[name]
    a = e["a"]
    g = device(sv, e)
    n, npb = len(a["coff"]) - 1, len(a["prob_off"]) - 1
    pi, pc = 3, 7  # images and corners that belong to nothing
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    cam_bytes = lambda cams: np.frombuffer(b"".join(bytes(c.to_c()) for c in cams), dtype=np.uint8).copy()
    dc = up(np.concatenate([np.full((pc, 2), 1e6, np.float32), a["corners"]]))
    db = up(np.concatenate([np.full((pc, 2), -3.0, np.float32), a["board"]]))
    dco = up(np.concatenate([np.zeros(pi, np.int64), a["coff"] + pc]))
    dpr = up(a["prob_off"] + pi)
    dk = up(np.concatenate([np.ones(pi, np.uint8), e["keep"].astype(np.uint8)]))
    dq = up(np.concatenate([np.full((pi, 4), -7.0), e["q0"]]))
    dt = up(np.concatenate([np.full((pi, 3), -7.0), e["t0"]]))
    dcam = up(cam_bytes(e["cams"]))
    dst = torch.full((pi + n,), -7, dtype=torch.int32, device=dev)
    dH = torch.full((npb, 64), -7.0, dtype=torch.float64, device=dev)
    drms = torch.full((npb,), -7.0, dtype=torch.float64, device=dev)
    dsm = torch.zeros(npb * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sv.camera_calibrate_device(dc.data_ptr(), db.data_ptr(), dco.data_ptr(), n, npb, dcam.data_ptr(), dq.data_ptr(), dt.data_ptr(),
                               dsm.data_ptr(), dst.data_ptr(), problem_offsets_ptr=dpr.data_ptr(), keep_ptr=dk.data_ptr(),
                               H_cam_ptr=dH.data_ptr(), rms_ptr=drms.data_ptr(), options=pose_options(), camcal=e["co"])
    cams = (ClcCamera * npb).from_buffer_copy(dcam.cpu().numpy().tobytes())
    c = dict(q=dq.cpu().numpy()[pi:], t=dt.cpu().numpy()[pi:], status=dst.cpu().numpy()[pi:],
             k=np.array([list(x.proj) + list(x.dist) for x in cams]), H_cam=dH.cpu().numpy().reshape(npb, 8, 8), rms_px=drms.cpu().numpy(),
             summaries=(_capi.Summary * npb).from_buffer_copy(dsm.cpu().numpy().tobytes()))
    same_bits(c, g)
    # what lies ahead of the call's images is left alone
    assert np.all(dq.cpu().numpy()[:pi] == -7.0) and np.all(dst.cpu().numpy()[:pi] == -7)
    # one problem, no problem_offsets: images from 0 on
    k = e["notes"]["seeded"]
    sl = slice(a["prob_off"][k], a["prob_off"][k + 1])
    m = sl.stop - sl.start
    dq1, dt1, dcam1 = up(e["q0"][sl]), up(e["t0"][sl]), up(cam_bytes([e["cams"][k]]))
    dco1 = up(a["coff"][sl.start:sl.stop + 1] + pc)
    dst1 = torch.full((m,), -7, dtype=torch.int32, device=dev)
    dsm1 = torch.zeros(C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sv.camera_calibrate_device(dc.data_ptr(), db.data_ptr(), dco1.data_ptr(), m, 1, dcam1.data_ptr(), dq1.data_ptr(), dt1.data_ptr(),
                               dsm1.data_ptr(), dst1.data_ptr(), options=pose_options(), camcal=e["co"])
    cam1 = ClcCamera.from_buffer_copy(dcam1.cpu().numpy().tobytes())
    assert np.array_equal(dq1.cpu().numpy(), g["q"][sl]) and np.array_equal(dt1.cpu().numpy(), g["t"][sl])
    assert np.array_equal(np.array(list(cam1.proj) + list(cam1.dist)), g["k"][k])
    # zero problems: nothing to do, nothing written
    sv.camera_calibrate_device(dc.data_ptr(), db.data_ptr(), dco1.data_ptr(), m, 0, dcam1.data_ptr(), dq1.data_ptr(), dt1.data_ptr(),
                               dsm1.data_ptr(), dst1.data_ptr())
    assert np.array_equal(dq1.cpu().numpy(), g["q"][sl])


@pytest.mark.parametrize("name", CAMS)
def test_guess_in_both_forms(sv, shim, batch, name):
    """clc_camera_guess on the 'corners' problem (3, 4, 63, 64, 65 and 144 corners: the 3-corner image is not usable) and on the
    T + 1 images: the device-array form (behind offsets above 0) returns the host-array form's bits; both agree with the host build.
    Measured on the MI355X: the host build's bits on all four sets (the DLT runs without multiply-add contraction on both)."""
    import torch
    e = batch[name]
    a, cam = e["a"], e["cam"]
    dev = torch.device("cuda:0")
    for nm, want_used in (("corners", 9), ("threads+1", 257)):
        k = e["notes"][nm]
        i0, i1 = a["prob_off"][k], a["prob_off"][k + 1]
        off = a["coff"][i0:i1 + 1]
        gcam, used = sv.camera_guess(cam.model, cam.width, cam.height, a["corners"], a["board"], off)
        dc, db, do = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (a["corners"], a["board"], off))
        torch.cuda.synchronize()
        dcam, dused = sv.camera_guess_device(cam.model, cam.width, cam.height, dc.data_ptr(), db.data_ptr(), do.data_ptr(), i1 - i0)
        assert dcam == gcam and dused == used == want_used
        assert gcam.proj[0] == gcam.proj[1] and gcam.proj[2:] == (cam.width / 2.0, cam.height / 2.0) and gcam.dist == (0.0,) * 4
        sub = dict(corners=a["corners"], board=a["board"], coff=off)
        f, _, st, su = CH.shim_guess(shim, cam, sub)
        print(name, nm, "f", gcam.proj[0], "host build", f, "relative", abs(gcam.proj[0] - f) / f)
        assert su == used and abs(gcam.proj[0] - f) / f < GPU_GUESS_BOUND
    with pytest.raises(_capi.ClcError):  # one usable image
        sv.camera_guess(cam.model, cam.width, cam.height, a["corners"], a["board"], a["coff"][:2])


@pytest.mark.parametrize("name", CAMS)
def test_calibrate_camera_end_to_end(sv, name):
    """calib.CalibrateCamera on a seeded 20-image set — guess, K10's poses under it, the solve — against the restatement's minimiser
    from the same start (not against the ground truth, which lies a sigma away).  Measured on the MI355X (radtan / kb): start f = 549.7 / 393.6 against
    the true 458 / 367; |dk| / sigma 5.03e-7 / 5.1e-12, cost 4.8e-15 / 1.59e-14, H_cam 2.52e-9 / 4.0e-14; 16 / 15 iterations."""
    cam = cases.CAMERAS[name]
    imgs = cases.images(name, 500 + (name == "kb"), 20)
    cp, bx = [i[0] for i in imgs], [i[1] for i in imgs]
    out, q, t, rep = calib.CalibrateCamera(cam.model, cam.width, cam.height, cp, bx, solver=sv)
    assert rep["termination"].startswith("CONVERGENCE") and rep["n_used"] == 20 and np.all(rep["status"] == 1)
    assert (out.model, out.width, out.height) == (cam.model, cam.width, cam.height)
    a = cases.arrays([imgs])
    g0 = rep["camera0"]
    q0, t0, _, st0, _ = sv.board_poses(g0, a["corners"], a["board"], a["coff"])
    res = dict(k=CH.k_of(out)[None], q=q, t=t, summaries=[rep["summary"]], H_cam=rep["H_cam"][None], rms_px=np.array([rep["rms_px"]]),
               hold_mask=rep["hold_mask"])
    c = CH.compare_problem(g0, a, 0, res, q0, t0)
    print(name, "from f =", g0.proj[0], {x: float("%.3g" % c[x]) for x in ("param_sigma", "cost", "rms", "hcam")}, "iterations", rep["iterations"])
    print("   k - truth", CH.k_of(out) - CH.k_of(cam), "\n   sigma", rep["sigma"])
    assert c["param_sigma"] < GPU_PARAM_SIGMA and c["cost"] < GPU_COST_BOUND and c["rms"] < GPU_RMS_BOUND and c["hcam"] < GPU_HCAM_BOUND
    free = [j for j in range(8) if not (rep["hold_mask"] >> j) & 1]
    assert np.allclose(rep["sigma"][free], c["sigma"][free], rtol=1e-5) and np.all(np.isnan(np.delete(rep["sigma"], free)))
    assert rep["cost"] == rep["summary"].final_cost and 0.3 < rep["rms_px"] < 0.5
    # camera0 given, an intrinsic held by index
    out2, _, _, rep2 = calib.CalibrateCamera(cam.model, cam.width, cam.height, cp, bx, hold=[2], camera0=cases.start_camera(cam), solver=sv)
    assert out2.proj[2] == cases.start_camera(cam).proj[2] and rep2["hold_mask"] == 4 and np.isnan(rep2["sigma"][2])


def test_refusals_come_back_through_the_c_abi(sv):
    cam = cases.CAMERAS["radtan"]
    a = cases.arrays([cases.images("radtan", 600, 2)])
    q0, t0, _, _, _ = sv.board_poses(cam, a["corners"], a["board"], a["coff"])
    for co in (_capi.CamcalOptions(0.0, 0, 0), _capi.CamcalOptions(0.3, 0xFF, 1), _capi.CamcalOptions(0.3, 0x1FF, 0)):
        with pytest.raises(_capi.ClcError):
            sv.camera_calibrate(cam, a["corners"], a["board"], a["coff"], q0, t0, camcal=co)
    with pytest.raises(_capi.ClcError):
        sv.camera_guess(5, 752, 480, a["corners"], a["board"], a["coff"])
    # everything but the poses held: allowed, the camera keeps its bits
    r = sv.camera_calibrate(cam, a["corners"], a["board"], a["coff"], q0, t0, camcal=_capi.CamcalOptions(0.3, 0xFF, 0))
    assert r["cameras"][0] == cam and r["summaries"][0].termination in (1, 2, 3) and np.all(r["H_cam"][0] == 0)
