"""K22 on the MI355X: clc_joint_refine_robust against the host build of the same code (tests/shim/jointrobust_shim.cpp) and the
restatement (tests/jointrobust_ref.py) on one batch per camera model sized to go wrong at the wave, lane and thread edges — the
shapes of joint_cases.edge_problems (images per problem 1, 2, W-1, W, W+1 and T+1; corners per image 3, 4, 63, 64, 65, 144; points
per image 0, 1, 63, 64, 65, 1081), contaminated where an image has 16 observations or more, keep with holes, a problem with every
image dropped; the weights and their NaN rule; two runs and a problem alone against the batch, bit for bit; 257 small problems, one
and two of them alone; the device-array form behind offsets above 0 against the host-array form; both scales 0 against
clc_joint_refine on the device, bit for bit; the Python front end and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import joint_cases as jcases  # noqa: E402
import jointrobust_cases as cases  # noqa: E402
import jointrobust_ref as rref  # noqa: E402
import test_joint_host as JH  # noqa: E402
import test_jointrobust_host as RH  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi, calib, simdata  # noqa: E402

pytestmark = pytest.mark.gpu
CAMS = RH.CAMS
# Measured on the MI355X on these batches, worst of both cameras (test_batch_matches_host_build_and_restatement's docstring),
# asserted one decade above, never above the project's gates (1e-6 on poses, 1e-8 relative on cost):
GPU_POSE_BOUND = 1e-6         # the restatement's minimiser, any R entry or t component, well-posed problems (1.64e-7: the gate binds)
GPU_COST_BOUND = 4e-13        # relative, final cost and cost shares against the restatement (3.97e-14; shares 3.3e-15)
GPU_HOST_POSE_BOUND = 4.4e-7  # device against the host build, any R entry or t component (4.39e-8)
GPU_HOST_COST_BOUND = 2.8e-14 # device against the host build, relative final cost (1.5e-15 here, 2.79e-15 over the 257 problems)
GPU_HOST_HCL_BOUND = 4.7e-7   # device against the host build, H_cl relative in the Frobenius norm (4.66e-8: it moves with the poses)
GPU_WEIGHT_BOUND = 2.7e-6     # a weight against the restatement's at its minimiser (2.63e-7), and against the host build's (9.6e-8)
GPU_WEIGHT_SAME_POINT = 3.4e-13  # a weight against the restatement's at the device's own poses (3.39e-14)
assert GPU_POSE_BOUND <= RH.POSE_GATE and GPU_HOST_POSE_BOUND <= RH.POSE_GATE and GPU_COST_BOUND <= RH.COST_GATE
ITERATIONS = 200             # as tests/test_gpu_joint.py: the unobservable shapes descend along flat valleys
RESTATED_IMAGES = 16         # the restatement is dense: problems of up to 6 + 6 * 16 parameters are compared with it


@pytest.fixture(scope="module")
def sv():
    with clc.Solver(0) as s:
        yield s


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return RH.build_shim(str(tmp_path_factory.mktemp("jrg") / "libjointrobust_shim.so"))


@pytest.fixture(scope="module")
def batch(shim):
    """Per camera: the contaminated edge problems, a contaminated seeded one, one with holes in keep and one with every image dropped
    as ONE call; the start poses by the shim's K10, the shim's result — computed once."""
    out = {}
    for name in CAMS:
        cam = jcases.CAMERAS[name]
        problems, notes = cases.contaminated_edge_problems(name)
        rng = np.random.default_rng(12)
        for nm, p in (("seeded", cases.contaminate(jcases.problem(name, 401, 10, 144, 100), rng)),
                      ("holes", cases.contaminate(jcases.problem(name, 402, 7, 144, 60), rng)),
                      ("dropped", jcases.problem(name, 403, 3, 144, 20))):
            notes[nm] = len(problems)
            problems.append(p)
        a = jcases.arrays(problems)
        keep = np.ones(len(a["coff"]) - 1, bool)
        keep[a["prob_off"][notes["holes"]] + np.array([1, 4])] = False
        keep[a["prob_off"][notes["dropped"]]:a["prob_off"][notes["dropped"] + 1]] = False
        q0, t0, st = JH.start_poses(shim, cam, a)
        jo = JH.shim_joint_options(shim, cam)
        lo = RH.loss_options(shim, jo)
        out[name] = dict(cam=cam, problems=problems, notes=notes, a=a, keep=keep, q0=q0, t0=t0, jo=jo, lo=lo,
                         s=RH.shim_robust(shim, cam, a, q0, t0, keep=keep, jo=jo, lo=lo, max_iterations=ITERATIONS))
    return out


def pose_options():
    o = _capi.default_pose_options()
    o.max_num_iterations = ITERATIONS
    return o


def device(sv, e, sel=None, joint=None, loss=None):
    """The host-array form on the batch (sel: a subset of its problems, in order)."""
    a = e["a"]
    if sel is None:
        return sv.joint_refine_robust(e["cam"], a["corners"], a["board"], a["coff"], a["pts"], a["poff"], e["q0"], e["t0"], a["poses_cl0"],
                                      problem_offsets=a["prob_off"], keep=e["keep"], joint=joint, loss=loss, options=pose_options())
    img = np.concatenate([np.arange(a["prob_off"][k], a["prob_off"][k + 1]) for k in sel])
    ci = np.concatenate([np.arange(a["coff"][i], a["coff"][i + 1]) for i in img]).astype(int)
    pi = np.concatenate([np.arange(a["poff"][i], a["poff"][i + 1]) for i in img]).astype(int)
    cs = lambda off, idx: np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in idx])]).astype(np.int64)
    pr = np.concatenate([[0], np.cumsum([a["prob_off"][k + 1] - a["prob_off"][k] for k in sel])]).astype(np.int64)
    r = sv.joint_refine_robust(e["cam"], a["corners"][ci], a["board"][ci], cs(a["coff"], img), a["pts"][pi], cs(a["poff"], img), e["q0"][img],
                               e["t0"][img], a["poses_cl0"][sel], problem_offsets=pr, keep=e["keep"][img], joint=joint, loss=loss,
                               options=pose_options())
    r["images"], r["corner_idx"], r["point_idx"] = img, ci, pi
    return r


def same_bits(x, y, images=None, problems=None, corner_idx=None, point_idx=None, weights=True):
    """x (a run on a subset, or a whole run) against the whole run y."""
    ii = slice(None) if images is None else images
    pp = slice(None) if problems is None else problems
    for key in ("q", "t", "status"):
        assert np.array_equal(x[key], y[key][ii]), key
    for key in ("poses_cl", "H_cl", "cost_parts"):
        assert np.array_equal(x[key], y[key][pp], equal_nan=True), key
    if weights:
        assert np.array_equal(x["w_corner"], y["w_corner"][slice(None) if corner_idx is None else corner_idx], equal_nan=True)
        assert np.array_equal(x["w_laser"], y["w_laser"][slice(None) if point_idx is None else point_idx], equal_nan=True)
    ys = [y["summaries"][k] for k in (range(len(y["poses_cl"])) if problems is None else problems)]
    for k, smy in enumerate(ys):
        smx = x["summaries"][k]
        assert (smx.termination, smx.num_iterations, smx.num_evaluations, smx.final_cost, smx.initial_cost) == \
               (smy.termination, smy.num_iterations, smy.num_evaluations, smy.final_cost, smy.initial_cost), k


def well_posed(prob, X, cols):
    """The minimiser is unique where the weighted normal matrix over the moving columns has full rank."""
    Hd = rref.normal_matrix(prob, *X)[0][np.ix_(cols, cols)]
    s = np.sqrt(np.diag(Hd))
    w = np.linalg.eigvalsh(Hd / np.outer(s, s))
    return w[0] > 1e-9 * w[-1]


@pytest.mark.parametrize("name", CAMS)
def test_batch_matches_host_build_and_restatement(sv, shim, batch, name):
    """Every problem of the batch: the statuses are the host build's; poses, final cost, H_cl and weights against the host build; for
    the problems of up to RESTATED_IMAGES images the minimiser (where it is unique: three images or more with laser points), the
    final cost, the cost shares and the weights against the restatement.  The shapes in which T_cl cannot be observed (1 and 2
    images) are compared on the cost only, as in K18.  The problem of T + 1 images is held against the host build, and its cost and
    weights against the restatement's at its own poses.  The weights: NaN for every image that takes no part and for the dropped
    problem, in (0, 1] elsewhere.  A second run gives the same bits.
    Measured on the MI355X (radtan / kb): against the restatement pose 9.76e-8 / 1.64e-7, cost 3.75e-15 / 3.97e-14, cost shares
    3.28e-15 / 1.06e-15, weights 1.80e-7 / 2.63e-7 (3.39e-14 / 2.76e-14 at the device's own poses); against the host build pose
    4.39e-8 / 4.02e-8, cost 1.23e-15 / 1.51e-15, H_cl 2.26e-8 / 4.66e-8, weights 9.57e-8 / 5.08e-8.  (Device and host differ by FMA
    contraction, the reciprocal square roots of the factorisations and log1p; both stop on the function tolerance.)  Iterations:
    23-93 on the few-image edge shapes (flat valleys, as in K18), 10-17 on the 7 and 10 image problems.  The module's bounds are
    one decade above the worst, never above the gates."""
    e = batch[name]
    a, notes, s = e["a"], e["notes"], e["s"]
    g = device(sv, e)
    assert np.array_equal(g["status"], s["status"])
    want = np.ones(len(e["keep"]), np.int32)
    want[~e["keep"]] = -1
    want[a["prob_off"][notes["corners"]]] = 0  # 3 corners
    assert np.array_equal(g["status"], want)
    worst = dict(host_pose=0.0, host_cost=0.0, host_hcl=0.0, host_w=0.0, pose=0.0, cost=0.0, parts=0.0, w=0.0, w_same=0.0)
    for k in range(len(e["problems"])):
        sl = slice(a["prob_off"][k], a["prob_off"][k + 1])
        smg, sms = g["summaries"][k], s["summaries"][k]
        if k == notes["dropped"]:
            assert smg.termination == 6 and np.array_equal(g["q"][sl], e["q0"][sl]) and np.array_equal(g["t"][sl], e["t0"][sl])
            assert np.array_equal(g["poses_cl"][k], a["poses_cl0"][k])
            continue
        assert smg.termination in (1, 2, 3) and sms.termination in (1, 2, 3), (k, smg.termination, sms.termination)
        assert smg.final_cost <= smg.initial_cost
        worst["host_cost"] = max(worst["host_cost"], abs(smg.final_cost - sms.final_cost) / sms.final_cost)
        prob, idx = RH.restatement_problem(shim, e["cam"], a, k, e["jo"], e["lo"], e["keep"])
        mine = JH.poses_of(g, idx, k)
        cc, cl = rref.cost_parts(prob, *mine)
        worst["cost"] = max(worst["cost"], abs(smg.final_cost - (cc + cl)) / (cc + cl))
        worst["parts"] = max(worst["parts"], max(abs(g["cost_parts"][k][0] - cc), abs(g["cost_parts"][k][1] - cl)) / (cc + cl))
        wc, wl = RH.weights_of(a, g, idx)
        wcr, wlr = rref.weights(prob, *mine)
        worst["w_same"] = max(worst["w_same"], np.abs(wc - wcr).max(initial=0.0), np.abs(wl - wlr).max(initial=0.0))
        no_laser = sum(len(p) for p in prob["pts"]) == 0
        unique = len(idx) >= 3 and not no_laser and well_posed(prob, mine, RH.ref.columns(len(idx)))
        if len(idx) <= RESTATED_IMAGES:
            c = RH.compare_problem(shim, e["cam"], a, k, g, e["q0"], e["t0"], e["jo"], e["lo"], e["keep"])
            worst["cost"] = max(worst["cost"], c["cost"])
            if unique:
                worst["pose"] = max(worst["pose"], c["pose"])
                worst["w"] = max(worst["w"], c["w"])
        if unique:
            worst["host_pose"] = max(worst["host_pose"], JH.pose_gap(mine, JH.poses_of(s, idx, k)))
            worst["host_hcl"] = max(worst["host_hcl"], np.linalg.norm(g["H_cl"][k] - s["H_cl"][k]) / np.linalg.norm(s["H_cl"][k]))
            ws = RH.weights_of(a, s, idx)
            worst["host_w"] = max(worst["host_w"], np.abs(wc - ws[0]).max(initial=0.0), np.abs(wl - ws[1]).max(initial=0.0))
        else:
            assert len(idx) < 3 or no_laser, (k, len(idx))
    # the weights' NaN rule, image by image
    for i in range(len(e["keep"])):
        wc, wl = g["w_corner"][a["coff"][i]:a["coff"][i + 1]], g["w_laser"][a["poff"][i]:a["poff"][i + 1]]
        if g["status"][i] == 1:
            assert np.all((wc > 0) & (wc <= 1)) and np.all((wl > 0) & (wl <= 1)), i
        else:
            assert np.all(np.isnan(wc)) and np.all(np.isnan(wl)), i
            assert np.array_equal(g["q"][i], e["q0"][i]) and np.array_equal(g["t"][i], e["t0"][i])
    assert np.array_equal(g["poses_cl"][notes["nolaser"]], a["poses_cl0"][notes["nolaser"]])
    # the planted observations of the seeded problem are down-weighted, the others mostly not
    k = notes["seeded"]
    idx = list(range(a["prob_off"][k], a["prob_off"][k + 1]))
    down, frac = cases.separation(*RH.weights_of(a, g, idx), *cases.planted_masks(e["problems"][k]))
    print("%s: seeded problem: planted all below 0.5: %s, others at or above 0.5: %.3f" % (name, down, frac))
    assert down and frac >= 0.95
    print("%s: worst gaps %s" % (name, {k: "%.2e" % v for k, v in worst.items()}))
    print("%s: iterations %s" % (name, [g["summaries"][k].num_iterations for k in range(len(e["problems"]))]))
    assert worst["pose"] <= GPU_POSE_BOUND and worst["cost"] <= GPU_COST_BOUND and worst["parts"] <= GPU_COST_BOUND
    assert worst["host_pose"] <= GPU_HOST_POSE_BOUND and worst["host_cost"] <= GPU_HOST_COST_BOUND
    assert worst["host_hcl"] <= GPU_HOST_HCL_BOUND
    assert worst["w"] <= GPU_WEIGHT_BOUND and worst["host_w"] <= GPU_WEIGHT_BOUND and worst["w_same"] <= GPU_WEIGHT_SAME_POINT
    # a second run gives the same bits
    same_bits(device(sv, e), g)


@pytest.mark.parametrize("name", CAMS)
def test_problem_alone_equals_the_problem_in_the_batch(sv, batch, name):
    e = batch[name]
    g = device(sv, e)
    for nm in ("images1", "images%d" % (jcases.WAVES + 1), "images%d" % (jcases.THREADS + 1), "points", "holes", "dropped"):
        k = e["notes"][nm]
        r = device(sv, e, [k])
        same_bits(r, g, r["images"], [k], r["corner_idx"], r["point_idx"])
    two = [e["notes"]["corners"], e["notes"]["seeded"]]
    r = device(sv, e, two)
    same_bits(r, g, r["images"], two, r["corner_idx"], r["point_idx"])


@pytest.mark.parametrize("name", CAMS)
def test_many_small_problems(sv, shim, name):
    """257 problems of 6 images (36 corners spread over the board, 20 points; two corners and two points planted per image) in one
    call: against the host build, and one and two problems alone bit for bit.  (Six images: with four, a few of the 257 contaminated
    problems crawl along a flat valley to the iteration cap, K18 on the same data too, and a capped run has no minimiser to
    compare.)"""
    cam = jcases.CAMERAS[name]
    rng = np.random.default_rng(77)
    problems = [cases.contaminate(jcases.problem(name, 5000 + k, 6, 36, 20, stride=4), rng) for k in range(257)]
    a = jcases.arrays(problems)
    q0, t0, st = JH.start_poses(shim, cam, a)
    assert np.all(st == 1)
    e = dict(cam=cam, a=a, keep=np.ones(len(q0), bool), q0=q0, t0=t0)
    g = device(sv, e)
    s = RH.shim_robust(shim, cam, a, q0, t0, max_iterations=ITERATIONS)
    term = np.array([g["summaries"][k].termination for k in range(257)])
    assert np.all((term >= 1) & (term <= 3))
    cost_g = np.array([g["summaries"][k].final_cost for k in range(257)])
    cost_s = np.array([s["summaries"][k].final_cost for k in range(257)])
    print(name + ", 257 problems: largest relative cost gap to the host build %.2e" % (np.abs(cost_g - cost_s) / cost_s).max())
    assert np.all(np.abs(cost_g - cost_s) <= GPU_HOST_COST_BOUND * cost_s)
    assert np.all((g["w_corner"] > 0) & (g["w_corner"] <= 1)) and np.all((g["w_laser"] > 0) & (g["w_laser"] <= 1))
    r = device(sv, e, [200])
    same_bits(r, g, r["images"], [200], r["corner_idx"], r["point_idx"])
    r = device(sv, e, [0, 256])
    same_bits(r, g, r["images"], [0, 256], r["corner_idx"], r["point_idx"])


@pytest.mark.parametrize("name", CAMS)
def test_both_scales_zero_are_clc_joint_refine_bit_for_bit(sv, batch, name):
    """loss_corner = loss_laser = 0 on the whole batch: poses, summaries, H_cl, cost_parts and status are clc_joint_refine's bits on
    the device, also with the board poses held; every weight is 1, NaN where the image takes no part."""
    e = batch[name]
    a = e["a"]
    for kw in (dict(), dict(hold_board_poses=1)):
        jo = _capi.default_joint_options(e["cam"])
        for k, v in kw.items():
            setattr(jo, k, v)
        g = device(sv, e, joint=jo, loss=_capi.JointLossOptions(0.0, 0.0))
        k18 = sv.joint_refine(e["cam"], a["corners"], a["board"], a["coff"], a["pts"], a["poff"], e["q0"], e["t0"], a["poses_cl0"],
                              problem_offsets=a["prob_off"], keep=e["keep"], joint=jo, options=pose_options())
        same_bits(g, k18, weights=False)
        part = np.repeat(g["status"] == 1, np.diff(a["coff"])), np.repeat(g["status"] == 1, np.diff(a["poff"]))
        dropped = e["notes"]["dropped"]
        assert g["summaries"][dropped].termination == 6
        assert np.all(g["w_corner"][part[0]] == 1.0) and np.all(np.isnan(g["w_corner"][~part[0]]))
        assert np.all(g["w_laser"][part[1]] == 1.0) and np.all(np.isnan(g["w_laser"][~part[1]]))


@pytest.mark.parametrize("name", CAMS)
def test_device_form_behind_offsets(sv, batch, name):
    """Every array in device memory, the call's images, corners and points behind pads (problem_offsets[0], the corner and point
    offsets all above 0): the bits of the host-array call, the weights at the absolute offsets, the pads untouched.  Then one problem
    without problem_offsets and without weight arrays, and zero problems."""
    import torch
    e = batch[name]
    a, cam = e["a"], e["cam"]
    g = device(sv, e)
    n, npb = len(a["coff"]) - 1, len(a["prob_off"]) - 1
    pi, pc, pp = 3, 7, 5  # images, corners and points that belong to nothing
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    dc = up(np.concatenate([np.full((pc, 2), 1e6, np.float32), a["corners"]]))
    db = up(np.concatenate([np.full((pc, 2), -3.0, np.float32), a["board"]]))
    dp = up(np.concatenate([np.full((pp, 3), np.nan), a["pts"]]))
    dco = up(np.concatenate([np.zeros(pi, np.int64), a["coff"] + pc]))
    dpo = up(np.concatenate([np.zeros(pi, np.int64), a["poff"] + pp]))
    dpr = up(a["prob_off"] + pi)
    dk = up(np.concatenate([np.ones(pi, np.uint8), e["keep"].astype(np.uint8)]))
    dq = up(np.concatenate([np.full((pi, 4), -7.0), e["q0"]]))
    dt = up(np.concatenate([np.full((pi, 3), -7.0), e["t0"]]))
    dcl = up(a["poses_cl0"])
    dst = torch.full((pi + n,), -7, dtype=torch.int32, device=dev)
    dH = torch.full((npb, 36), -7.0, dtype=torch.float64, device=dev)
    dparts = torch.full((npb, 2), -7.0, dtype=torch.float64, device=dev)
    dwc = torch.full((pc + len(a["corners"]),), -7.0, dtype=torch.float64, device=dev)
    dwl = torch.full((pp + len(a["pts"]),), -7.0, dtype=torch.float64, device=dev)
    dsm = torch.zeros(npb * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sv.joint_refine_robust_device(cam, dc.data_ptr(), db.data_ptr(), dco.data_ptr(), dp.data_ptr(), dpo.data_ptr(), n, npb, dq.data_ptr(),
                                  dt.data_ptr(), dcl.data_ptr(), dsm.data_ptr(), dst.data_ptr(), problem_offsets_ptr=dpr.data_ptr(),
                                  keep_ptr=dk.data_ptr(), H_cl_ptr=dH.data_ptr(), cost_parts_ptr=dparts.data_ptr(),
                                  w_corner_ptr=dwc.data_ptr(), w_laser_ptr=dwl.data_ptr(), options=pose_options())
    c = dict(q=dq.cpu().numpy()[pi:], t=dt.cpu().numpy()[pi:], status=dst.cpu().numpy()[pi:], poses_cl=dcl.cpu().numpy(),
             H_cl=dH.cpu().numpy().reshape(npb, 6, 6), cost_parts=dparts.cpu().numpy(), w_corner=dwc.cpu().numpy()[pc:],
             w_laser=dwl.cpu().numpy()[pp:], summaries=(_capi.Summary * npb).from_buffer_copy(dsm.cpu().numpy().tobytes()))
    same_bits(c, g)
    # what lies ahead of the call's images, corners and points is left alone
    assert np.all(dq.cpu().numpy()[:pi] == -7.0) and np.all(dst.cpu().numpy()[:pi] == -7)
    assert np.all(dwc.cpu().numpy()[:pc] == -7.0) and np.all(dwl.cpu().numpy()[:pp] == -7.0)
    # one problem, no problem_offsets: images from 0 on; no weight arrays
    k = e["notes"]["seeded"]
    sl = slice(a["prob_off"][k], a["prob_off"][k + 1])
    m = sl.stop - sl.start
    dq1, dt1, dcl1 = up(e["q0"][sl]), up(e["t0"][sl]), up(a["poses_cl0"][k:k + 1])
    dco1, dpo1 = up(a["coff"][sl.start:sl.stop + 1] + pc), up(a["poff"][sl.start:sl.stop + 1] + pp)
    dst1 = torch.full((m,), -7, dtype=torch.int32, device=dev)
    dsm1 = torch.zeros(C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sv.joint_refine_robust_device(cam, dc.data_ptr(), db.data_ptr(), dco1.data_ptr(), dp.data_ptr(), dpo1.data_ptr(), m, 1, dq1.data_ptr(),
                                  dt1.data_ptr(), dcl1.data_ptr(), dsm1.data_ptr(), dst1.data_ptr(), options=pose_options())
    assert np.array_equal(dq1.cpu().numpy(), g["q"][sl]) and np.array_equal(dt1.cpu().numpy(), g["t"][sl])
    assert np.array_equal(dcl1.cpu().numpy()[0], g["poses_cl"][k])
    # zero problems: nothing to do, nothing written
    sv.joint_refine_robust_device(cam, dc.data_ptr(), db.data_ptr(), dco1.data_ptr(), dp.data_ptr(), dpo1.data_ptr(), m, 0, dq1.data_ptr(),
                                  dt1.data_ptr(), dcl1.data_ptr(), dsm1.data_ptr(), dst1.data_ptr())
    assert np.array_equal(dq1.cpu().numpy(), g["q"][sl])


def test_python_front_end(sv):
    """calib.CamLaserCalibrationJointRobust and its batch variant on a contaminated seeded problem: the refined Tcl, the observation
    set with the refined tag poses, the report with the weights and inlier masks per image; the planted observations are the
    outliers it reports; closer to the truth than CamLaserCalibrationJoint on the same data; keep drops an image."""
    name = "radtan"
    cam = jcases.CAMERAS[name]
    p = cases.contaminate(jcases.problem(name, 77, 8, 144, 100), np.random.default_rng(5))
    a = jcases.arrays([p])
    q0, t0, _, st, _ = sv.board_poses(cam, a["corners"], a["board"], a["coff"])
    assert np.all(st == 1)
    obs = simdata.ObservationSet(q0, t0, a["poff"], a["pts"], a["poff"].copy(), a["pts"].copy())
    Tcl0 = simdata.T_from_pose7(p["pose_cl0"])
    cp, bx = [im[0] for im in p["images"]], [im[1] for im in p["images"]]
    Tcl, refined, rep = calib.CamLaserCalibrationJointRobust(cam, cp, bx, obs, Tcl0, solver=sv)
    raw = sv.joint_refine_robust(cam, a["corners"], a["board"], a["coff"], a["pts"], a["poff"], q0, t0, simdata.pose7_from_T(Tcl0)[None])
    assert np.array_equal(refined.tag_q, raw["q"]) and np.array_equal(refined.tag_t, raw["t"])
    assert np.allclose(Tcl, simdata.T_from_pose7(raw["poses_cl"][0]), rtol=0, atol=1e-15)
    assert rep["termination"].startswith("CONVERGENCE") and rep["summary"].final_cost == raw["summaries"][0].final_cost
    assert np.array_equal(rep["H_cl"], raw["H_cl"][0]) and rep["singular_values"].shape == (6,) and np.all(rep["singular_values"] > 0)
    assert rep["cost_corner"] + rep["cost_laser"] == pytest.approx(rep["summary"].final_cost, rel=1e-14)
    assert np.all(rep["status"] == 1) and np.array_equal(refined.pts, obs.pts)
    assert len(rep["w_corner"]) == len(rep["w_laser"]) == len(rep["inlier_corner"]) == len(rep["inlier_laser"]) == 8
    assert np.array_equal(np.concatenate(rep["w_corner"]), raw["w_corner"]) and np.array_equal(np.concatenate(rep["w_laser"]), raw["w_laser"])
    for i, (ic, ip) in enumerate(p["planted"]):
        assert rep["inlier_corner"][i].dtype == bool and rep["inlier_corner"][i].shape == (144,) and rep["inlier_laser"][i].shape == (100,)
        assert not rep["inlier_corner"][i][ic].any() and not rep["inlier_laser"][i][ip].any()
        assert np.array_equal(rep["inlier_laser"][i], rep["w_laser"][i] >= 0.5)
    truth = simdata.T_from_pose7(p["pose_cl_true"])
    Tcl18 = calib.CamLaserCalibrationJoint(cam, cp, bx, obs, Tcl0, solver=sv)[0]
    assert np.linalg.norm(Tcl[:3, 3] - truth[:3, 3]) < np.linalg.norm(Tcl18[:3, 3] - truth[:3, 3])
    # the scales come through: none at all is CamLaserCalibrationJoint
    T0, r0, rep0 = calib.CamLaserCalibrationJointRobust(cam, cp, bx, obs, Tcl0, solver=sv, loss_px_sigmas=0.0, loss_laser_m=0.0)
    assert np.array_equal(T0, Tcl18) and all(np.all(w == 1.0) for w in rep0["w_corner"] + rep0["w_laser"])
    keep = np.ones(8, bool); keep[2] = False
    both = calib.CamLaserCalibrationJointRobustBatch(cam, [dict(corners_px=cp, board_xy=bx, obs=obs, Tcl=Tcl0),
                                                           dict(corners_px=cp, board_xy=bx, obs=obs, Tcl=Tcl0, keep=keep)], solver=sv)
    assert np.array_equal(both[0][1].tag_q, refined.tag_q) and np.array_equal(both[0][0], Tcl)
    assert both[1][2]["status"][2] == -1 and np.array_equal(both[1][1].tag_q[2], q0[2]) and not np.array_equal(both[1][0], Tcl)
    assert np.all(np.isnan(both[1][2]["w_corner"][2])) and np.all(np.isnan(both[1][2]["w_laser"][2])) and not both[1][2]["inlier_laser"][2].any()


def test_refusals_come_back_through_the_c_abi(sv):
    cam = jcases.CAMERAS["radtan"]
    p = jcases.problem("radtan", 3, 3, 8, 4)
    a = jcases.arrays([p])
    q0 = np.tile([1.0, 0, 0, 0], (3, 1)); t0 = np.tile([0.0, 0, 1], (3, 1))
    call = lambda **kw: sv.joint_refine_robust(cam, a["corners"], a["board"], kw.pop("coff", a["coff"]), a["pts"], a["poff"], q0, t0,
                                               a["poses_cl0"], **kw)
    for lo in (_capi.JointLossOptions(-1.0, 5.0), _capi.JointLossOptions(3.0, float("nan")), _capi.JointLossOptions(float("inf"), 5.0)):
        with pytest.raises(_capi.ClcError) as ei:
            call(loss=lo)
        assert ei.value.code == -1 and "must be finite and >= 0" in str(ei.value)
    jo = _capi.default_joint_options(cam)
    jo.sigma_laser = float("nan")
    with pytest.raises(_capi.ClcError) as ei:
        call(joint=jo)
    assert ei.value.code == -1
    with pytest.raises(_capi.ClcError) as ei:
        call(coff=np.array([0, 8, 4, 24], dtype=np.int64))
    assert ei.value.code == -1 and "offsets not monotone" in str(ei.value)
    # a non-finite T_cl: the problem fails, the call does not, and every weight is NaN
    bad = a["poses_cl0"].copy(); bad[0, 1] = np.nan
    r = sv.joint_refine_robust(cam, a["corners"], a["board"], a["coff"], a["pts"], a["poff"], q0, t0, bad)
    assert r["summaries"][0].termination == 6 and np.array_equal(r["q"], q0)
    assert np.all(np.isnan(r["w_corner"])) and np.all(np.isnan(r["w_laser"]))
