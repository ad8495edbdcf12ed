"""K21 on the MI355X: clc_joint_refine_range against the host build of the same code (tests/shim/laserrange_shim.cpp) and the
restatement (tests/laserrange_ref.py) on one batch per camera model — the seeded sets and every edge problem of
tests/laserrange_cases.py in ONE call; two runs and a problem alone against the batch, bit for bit; the device-array form and
clc_range_correct(_device) against the host-array forms, bit for bit; the two invariants against clc_joint_refine; held parameters
and untouched outputs; the Python front end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import laserrange_cases as cases  # noqa: E402
import test_laserrange_host as LH  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi, calib, simdata  # noqa: E402

pytestmark = pytest.mark.gpu
CAMS = LH.CAMS
# Measured on the MI355X on the batch, worst of both cameras (test_batch_matches_host_build_and_restatement's docstring), asserted
# one decade above, within the project's gates (1e-6 on poses, 1e-8 relative on cost):
GPU_HOST_POSE_BOUND = 3.5e-7   # device against the host build, any R entry or t component, well-posed problems (3.43e-8)
GPU_HOST_RANGE_BOUND = 1e-5    # device against the host build, b and kappa in units of their 1 sigma from H_cr (9.91e-7)
GPU_HOST_COST_BOUND = 5.9e-14  # device against the host build, relative final cost, every problem but the single-range one (5.81e-15)
GPU_HOST_HCR_BOUND = 3.3e-7    # device against the host build, H_cr relative in the Frobenius norm, well-posed problems (3.26e-8)
GPU_K18_BOUND = 0.0            # held range against clc_joint_refine on the device: poses, cost shares, leading 6x6 of H_cr (0: the same bits)
assert GPU_HOST_POSE_BOUND <= LH.POSE_GATE and GPU_HOST_COST_BOUND <= LH.COST_GATE and GPU_K18_BOUND <= LH.POSE_GATE
ITERATIONS = 200  # as tests/test_gpu_joint.py: the shapes whose minimiser is a valley need more than the 50 of the pose options
SEEDED = len(cases.SEEDED)


@pytest.fixture(scope="module")
def sv():
    with clc.Solver(0) as s:
        yield s


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return LH.build_shim(str(tmp_path_factory.mktemp("lrg") / "liblaserrange_shim.so"))


@pytest.fixture(scope="module")
def batch(shim):
    """Per camera: the seeded sets, then the edge problems, as ONE call; the start poses by the shim's K10, the shim's result —
    computed once."""
    out = {}
    for name in CAMS:
        cam = cases.CAMERAS[name]
        problems = cases.seeded(name)
        edge, notes = cases.edge_problems(name)
        notes = {k: v + len(problems) for k, v in notes.items()}
        problems = problems + edge
        a = cases.arrays(problems)
        q0, t0, st = LH.TJ.start_poses(shim, cam, a)
        ro = LH.shim_range_options(shim, cam)
        out[name] = dict(cam=cam, problems=problems, notes=notes, a=a, q0=q0, t0=t0, ro=ro,
                         s=LH.shim_range(shim, cam, a, q0, t0, ro=ro, max_iterations=ITERATIONS))
    return out


def pose_options():
    o = _capi.default_pose_options()
    o.max_num_iterations = ITERATIONS
    return o


def device(sv, e, sel=None, ro=None, range0=None):
    """The host-array form on the batch (sel: a subset of its problems, in order)."""
    a = e["a"]
    r0 = a["range0"] if range0 is None else range0
    if sel is None:
        return sv.joint_refine_range(e["cam"], a["corners"], a["board"], a["coff"], a["pts"], a["poff"], e["q0"], e["t0"], a["poses_cl0"],
                                     range0=r0, problem_offsets=a["prob_off"], options=pose_options(), range_options=ro)
    img = np.concatenate([np.arange(a["prob_off"][k], a["prob_off"][k + 1]) for k in sel])
    ci = np.concatenate([np.arange(a["coff"][i], a["coff"][i + 1]) for i in img])
    pi = np.concatenate([np.arange(a["poff"][i], a["poff"][i + 1]) for i in img]).astype(int)
    cs = lambda off, idx: np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in idx])]).astype(np.int64)
    pr = np.concatenate([[0], np.cumsum([a["prob_off"][k + 1] - a["prob_off"][k] for k in sel])]).astype(np.int64)
    r = sv.joint_refine_range(e["cam"], a["corners"][ci], a["board"][ci], cs(a["coff"], img), a["pts"][pi], cs(a["poff"], img), e["q0"][img],
                              e["t0"][img], a["poses_cl0"][sel], range0=r0[sel], problem_offsets=pr, options=pose_options(), range_options=ro)
    r["images"] = img
    return r


def same_bits(x, y, images=None, problems=None):
    """x (a run on a subset, or a whole run) against the whole run y."""
    ii = slice(None) if images is None else images
    pp = slice(None) if problems is None else problems
    for key in ("q", "t", "status"):
        assert np.array_equal(x[key], y[key][ii]), key
    for key in ("poses_cl", "range", "H_cr", "cost_parts"):
        assert np.array_equal(x[key], y[key][pp], equal_nan=True), key
    ys = [y["summaries"][k] for k in (range(len(y["poses_cl"])) if problems is None else problems)]
    for k, smy in enumerate(ys):
        smx = x["summaries"][k]
        assert (smx.termination, smx.num_iterations, smx.num_evaluations, smx.final_cost, smx.initial_cost) == \
               (smy.termination, smy.num_iterations, smy.num_evaluations, smy.final_cost, smy.initial_cost), k


def well_posed_H(Hcr):
    """The 8x8 marginal information has full rank by test_joint_host.well_posed's threshold."""
    if not np.all(np.isfinite(Hcr)) or np.any(np.diag(Hcr) <= 0):
        return False
    sc = np.sqrt(np.diag(Hcr))
    w = np.linalg.eigvalsh(Hcr / np.outer(sc, sc))
    return w[0] > 1e-9 * w[-1]


def host_gaps(e, g, s, k):
    """Problem k of a device run g against the host build's s -> (pose gap, range gap in sigma, H_cr gap) or None where the
    minimiser is not unique."""
    a = e["a"]
    if not (well_posed_H(s["H_cr"][k]) and well_posed_H(g["H_cr"][k])):
        return None
    idx = [i for i in range(a["prob_off"][k], a["prob_off"][k + 1]) if s["status"][i] == 1]
    sig = np.sqrt(np.diag(np.linalg.inv(s["H_cr"][k])))
    return (LH.TJ.pose_gap(LH.state_of(g, idx, k)[:4], LH.state_of(s, idx, k)[:4]),
            max(abs(g["range"][k][j] - s["range"][k][j]) / sig[6 + j] for j in range(2)),
            np.linalg.norm(g["H_cr"][k] - s["H_cr"][k]) / np.linalg.norm(s["H_cr"][k]))


@pytest.mark.parametrize("name", CAMS)
def test_batch_matches_host_build_and_restatement(sv, shim, batch, name):
    """The seeded sets and every edge problem in one call: the statuses are the host build's; poses, range, final cost and H_cr against
    the host build (poses, range and H_cr where the 8x8 has full rank: not with 1 or 2 images, without a laser point or at a
    single range); the seeded sets against the restatement under the host test's bounds; a second run gives the same bits.
    Measured on the MI355X (radtan / kb): against the host build pose 9.1e-9 / 3.43e-8, b and kappa 3.2e-7 / 9.91e-7 of their sigma,
    cost 5.81e-15 / 1.84e-15, H_cr 7.7e-9 / 3.26e-8 (device and host differ by FMA contraction and the reciprocal square roots of the
    factorisations; most problems agree to 1e-15, the others stop one function-tolerance step apart); against the restatement on the
    seeded sets pose 1.4e-9 / 1.72e-8, b and kappa 4.4e-8 / 6.84e-7 sigma, cost 2.6e-15 / 2.6e-15, cost shares 1.3e-15 / 8.9e-16.
    The module's bounds are one decade above the worst."""
    e = batch[name]
    a, notes, s = e["a"], e["notes"], e["s"]
    g = device(sv, e)
    assert np.array_equal(g["status"], s["status"])
    want = np.ones(len(a["poff"]) - 1, np.int32)
    want[a["prob_off"][notes["corners"]]] = 0       # 3 corners
    want[a["prob_off"][notes["zerorange"]] + 2] = -2  # a zero-range point
    assert np.array_equal(g["status"], want)
    worst = dict(host_pose=0.0, host_range=0.0, host_cost=0.0, host_hcr=0.0)
    compared = []
    for k in range(len(e["problems"])):
        smg, sms = g["summaries"][k], s["summaries"][k]
        assert smg.termination in (1, 2, 3, 4, 5) and sms.termination in (1, 2, 3, 4, 5), (k, smg.termination, sms.termination)
        assert smg.final_cost <= smg.initial_cost
        single = k == notes["singlerange"]
        if not single:  # (there the cost is flat along (b, kappa) = (rho, -1) and the iterates part ways)
            worst["host_cost"] = max(worst["host_cost"], abs(smg.final_cost - sms.final_cost) / sms.final_cost)
        gaps = host_gaps(e, g, s, k)
        if gaps is not None:
            compared.append(k)
            print("%s problem %d: device vs host build: pose %.2e range %.2e sigma H_cr %.2e" % (name, k, *gaps))
            worst["host_pose"] = max(worst["host_pose"], gaps[0])
            worst["host_range"] = max(worst["host_range"], gaps[1])
            worst["host_hcr"] = max(worst["host_hcr"], gaps[2])
        for key in ("q", "t", "poses_cl", "range"):
            assert np.all(np.isfinite(g[key])), key
    assert set(range(SEEDED)) <= set(compared) and notes["singlerange"] not in compared and notes["nolaser"] not in compared
    assert all(notes[nm] in compared for nm in ("images%d" % (cases.WAVES + 1), "images%d" % (cases.THREADS + 1), "corners", "points", "zerorange"))
    # the images that take no part keep their poses; the problem without a laser point its T_cl and range
    for i in np.flatnonzero(g["status"] != 1):
        assert np.array_equal(g["q"][i], e["q0"][i]) and np.array_equal(g["t"][i], e["t0"][i])
    kn = notes["nolaser"]
    assert np.array_equal(g["poses_cl"][kn], a["poses_cl0"][kn]) and np.array_equal(g["range"][kn], a["range0"][kn])
    print("%s: device vs host build, worst gaps %s (problems %s)" % (name, {k: "%.2e" % v for k, v in worst.items()}, compared))
    assert worst["host_pose"] <= GPU_HOST_POSE_BOUND and worst["host_range"] <= GPU_HOST_RANGE_BOUND
    assert worst["host_cost"] <= GPU_HOST_COST_BOUND and worst["host_hcr"] <= GPU_HOST_HCR_BOUND
    # the seeded sets against the restatement, under the host test's bounds
    wr = dict(pose=0.0, range_sigma=0.0, cost=0.0, parts=0.0)
    for k in range(SEEDED):
        c = LH.compare_problem(shim, e["cam"], a, k, g, e["q0"], e["t0"], e["ro"])
        assert c["pose"] is not None
        for key in wr:
            wr[key] = max(wr[key], c[key])
        wr["cost"] = max(wr["cost"], c["cost_self"])
    print("%s: device vs the restatement on the seeded sets, worst gaps %s" % (name, {k: "%.2e" % v for k, v in wr.items()}))
    assert wr["pose"] <= LH.POSE_BOUND and wr["range_sigma"] <= LH.RANGE_SIGMA_BOUND
    assert wr["cost"] <= LH.COST_BOUND and wr["parts"] <= LH.COST_BOUND
    # a second run gives the same bits
    same_bits(device(sv, e), g)


def test_problem_alone_equals_the_problem_in_the_batch(sv, batch):
    e = batch["radtan"]
    g = device(sv, e)
    for nm in ("images1", "images%d" % (cases.THREADS + 1), "points", "zerorange", "singlerange"):
        k = e["notes"][nm]
        r = device(sv, e, [k])
        same_bits(r, g, r["images"], [k])
    two = [e["notes"]["corners"], 1]
    r = device(sv, e, two)
    same_bits(r, g, r["images"], two)


def test_device_form_and_range_correct_equal_the_host_forms(sv, batch):
    """Every array in device memory, the call's images, corners and points behind pads: the bits of the host-array call; the route
    without corners (hold_board_poses, NULL corner arrays, no camera) in both forms; clc_range_correct in both forms."""
    import torch
    e = batch["kb"]
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

    def run(ro, corners):
        dq = up(np.concatenate([np.full((pi, 4), -7.0), e["q0"]]))
        dt = up(np.concatenate([np.full((pi, 3), -7.0), e["t0"]]))
        dcl, drg = up(a["poses_cl0"]), up(a["range0"])
        dst = torch.full((pi + n,), -7, dtype=torch.int32, device=dev)
        dH = torch.full((npb, 64), -7.0, dtype=torch.float64, device=dev)
        dparts = torch.full((npb, 2), -7.0, dtype=torch.float64, device=dev)
        dsm = torch.zeros(npb * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        sv.joint_refine_range_device(cam if corners else None, dc.data_ptr() if corners else 0, db.data_ptr() if corners else 0,
                                     dco.data_ptr() if corners else 0, dp.data_ptr(), dpo.data_ptr(), n, npb, dq.data_ptr(), dt.data_ptr(),
                                     dcl.data_ptr(), drg.data_ptr(), dsm.data_ptr(), dst.data_ptr(), problem_offsets_ptr=dpr.data_ptr(),
                                     H_cr_ptr=dH.data_ptr(), cost_parts_ptr=dparts.data_ptr(), options=pose_options(), range_options=ro)
        assert np.all(dq.cpu().numpy()[:pi] == -7.0) and np.all(dst.cpu().numpy()[:pi] == -7)  # ahead of the call's images
        return dict(q=dq.cpu().numpy()[pi:], t=dt.cpu().numpy()[pi:], status=dst.cpu().numpy()[pi:], poses_cl=dcl.cpu().numpy(),
                    range=drg.cpu().numpy(), H_cr=dH.cpu().numpy().reshape(npb, 8, 8), cost_parts=dparts.cpu().numpy(),
                    summaries=(_capi.Summary * npb).from_buffer_copy(dsm.cpu().numpy().tobytes()))

    same_bits(run(None, True), g)
    held = _capi.default_range_options(None)
    held.hold_board_poses = 1
    gh = sv.joint_refine_range(None, None, None, None, a["pts"], a["poff"], e["q0"], e["t0"], a["poses_cl0"], range0=a["range0"],
                               problem_offsets=a["prob_off"], options=pose_options(), range_options=held)
    assert np.array_equal(gh["q"], e["q0"]) and np.all(gh["cost_parts"][:, 0] == 0.0)
    assert gh["status"][a["prob_off"][e["notes"]["corners"]]] == 1  # no corners needed
    same_bits(run(held, False), gh)
    # the point correction
    rg = (0.0234, -0.0071)
    out = sv.range_correct(a["pts"], *rg)
    dout = torch.empty_like(dp)
    torch.cuda.synchronize()
    sv.range_correct_device(dp.data_ptr(), len(a["pts"]) + pp, dout.data_ptr(), *rg)
    back = dout.cpu().numpy()
    assert np.all(np.isnan(back[:pp])) and np.array_equal(back[pp:], out, equal_nan=True)


def test_range_correct_against_the_formula(sv, shim):
    """clc_range_correct against the host build and numpy to 2 ulp (measured on the MI355X: 0 ulp to both), NaN for a zero or non-finite point,
    (0, 0) bit for bit."""
    from laserrange_ref import correct
    rng = np.random.default_rng(11)
    pts = rng.normal(size=(4099, 3)) * rng.uniform(0.05, 30.0, size=(4099, 1))
    pts[7] = 0.0
    pts[9, 1] = np.nan
    pts[4098, 2] = np.inf
    rg = (0.0234, -0.0071)
    out = sv.range_correct(pts, *rg)
    want = correct(pts, *rg)
    bad = [7, 9, 4098]
    ok = np.setdiff1d(np.arange(len(pts)), bad)
    assert np.all(np.isnan(out[bad]))
    ulp = (np.abs(out[ok] - want[ok]) / np.spacing(np.abs(want[ok]))).max()
    host = np.empty_like(pts)
    shim.shim_range_correct(LH.d(np.array(rg)), LH.d(pts), C.c_longlong(len(pts)), LH.d(host))
    ulp_h = (np.abs(out[ok] - host[ok]) / np.spacing(np.abs(host[ok]))).max()
    print("range_correct on the device: %.1f ulp to numpy, %.1f ulp to the host build" % (ulp, ulp_h))
    assert ulp <= 2.0 and ulp_h <= 2.0
    assert np.array_equal(sv.range_correct(pts, 0.0, 0.0)[ok], pts[ok])
    assert sv.range_correct(np.zeros((0, 3)), *rg).shape == (0, 3)


@pytest.mark.parametrize("name", CAMS)
def test_held_range_is_clc_joint_refine(sv, batch, name):
    """With both range parameters held at (0, 0) the call agrees with clc_joint_refine on poses, cost shares and the leading 6x6 of
    H_cr; with held non-zero values with clc_joint_refine on clc_range_correct'ed points.  Measured on the MI355X, both cameras, the
    seeded sets and the edge problems with 5 images, few corners, many points and no laser: no gap at all in either case, so the
    bound is zero: the same bits."""
    e = batch[name]
    a = e["a"]
    sel = list(range(SEEDED)) + [e["notes"][nm] for nm in ("images%d" % (cases.WAVES + 1), "corners", "points", "nolaser")]
    ro = _capi.default_range_options(e["cam"])
    ro.hold_range_mask = 3
    worst = 0.0
    for r0, pts in ((np.zeros((len(e["problems"]), 2)), a["pts"]),
                    (np.tile([0.015, -0.004], (len(e["problems"]), 1)), sv.range_correct(a["pts"], 0.015, -0.004))):
        g = device(sv, e, sel, ro=ro, range0=r0)
        j = device_joint(sv, e, sel, pts)
        assert np.array_equal(g["range"], r0[sel]) and np.array_equal(g["status"], j["status"])
        gap = max(np.abs(g["q"] - j["q"]).max(), np.abs(g["t"] - j["t"]).max(), np.abs(g["poses_cl"] - j["poses_cl"]).max())
        cgap = (np.abs(g["cost_parts"] - j["cost_parts"]).max(1) / j["cost_parts"].sum(1)).max()
        hn = np.linalg.norm(j["H_cl"].reshape(len(sel), -1), axis=1)
        hgap = (np.linalg.norm((g["H_cr"][:, :6, :6] - j["H_cl"]).reshape(len(sel), -1), axis=1) / np.where(hn > 0, hn, 1.0)).max()
        print("%s held at %s vs clc_joint_refine: poses %.2e cost shares %.2e H %.2e" % (name, r0[0], gap, cgap, hgap))
        worst = max(worst, gap, cgap, hgap)
        assert np.all(g["H_cr"][:, 6:, :] == 0) and np.all(g["H_cr"][:, :, 6:] == 0)
    assert worst <= GPU_K18_BOUND


def device_joint(sv, e, sel, pts):
    """clc_joint_refine on problems sel of the batch with the laser points pts."""
    a = e["a"]
    img = np.concatenate([np.arange(a["prob_off"][k], a["prob_off"][k + 1]) for k in sel])
    ci = np.concatenate([np.arange(a["coff"][i], a["coff"][i + 1]) for i in img])
    pi = np.concatenate([np.arange(a["poff"][i], a["poff"][i + 1]) for i in img]).astype(int)
    cs = lambda off, idx: np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in idx])]).astype(np.int64)
    pr = np.concatenate([[0], np.cumsum([a["prob_off"][k + 1] - a["prob_off"][k] for k in sel])]).astype(np.int64)
    return sv.joint_refine(e["cam"], a["corners"][ci], a["board"][ci], cs(a["coff"], img), pts[pi], cs(a["poff"], img), e["q0"][img],
                           e["t0"][img], a["poses_cl0"][sel], problem_offsets=pr, options=pose_options())


def test_held_parameters_and_untouched_outputs(sv, batch):
    """A held parameter comes back bit for bit while the other moves; hold_extrinsic leaves T_cl bit for bit while b and kappa move;
    a non-finite start range ends its problem CLC_FAILURE with everything untouched, and the other problems as without it."""
    e = batch["radtan"]
    a = e["a"]
    sel = list(range(SEEDED))
    r0 = np.tile([0.0123456789, -0.00456789], (len(e["problems"]), 1))
    for mask in (1, 2):
        ro = _capi.default_range_options(e["cam"])
        ro.hold_range_mask = mask
        g = device(sv, e, sel, ro=ro, range0=r0)
        held, free = mask - 1, 2 - mask
        assert np.array_equal(g["range"][:, held], r0[sel, held]) and np.all(g["range"][:, free] != r0[sel, free])
        assert np.all(g["H_cr"][:, 6 + held, :] == 0) and np.all(g["H_cr"][:, :, 6 + held] == 0) and np.all(g["H_cr"][:, 6 + free, 6 + free] > 0)
    ro = _capi.default_range_options(e["cam"])
    ro.hold_extrinsic = 1
    g = device(sv, e, sel, ro=ro)
    assert np.array_equal(g["poses_cl"], a["poses_cl0"][sel]) and np.all(g["range"] != 0)
    assert np.all(g["H_cr"][:, :6, :] == 0) and np.all(g["H_cr"][:, :, :6] == 0)
    bad = a["range0"].copy()
    bad[1, 0] = np.nan
    gb, gg = device(sv, e, sel, range0=bad), device(sv, e, sel)
    sl = slice(a["prob_off"][1], a["prob_off"][2])
    assert gb["summaries"][1].termination == 6 and np.array_equal(gb["q"][sl], e["q0"][sl]) and np.array_equal(gb["t"][sl], e["t0"][sl])
    assert np.array_equal(gb["poses_cl"][1], a["poses_cl0"][1]) and np.isnan(gb["range"][1][0]) and np.all(np.isnan(gb["H_cr"][1]))
    for k in (0, 2, 3):
        assert np.array_equal(gb["poses_cl"][k], gg["poses_cl"][k]) and np.array_equal(gb["range"][k], gg["range"][k])


def test_python_front_end(sv):
    """calib.CamLaserCalibrationRange and ApplyRangeCorrection on 10 images with a planted 0.02 m / 0.5 %: the recovered values lie
    within 4 of the report's own sigma of the planted ones, and CamLaserCalibration on the corrected set ends closer to the true T_cl
    than on the uncorrected one.  Measured on the MI355X: b 0.0204 m (sigma 1.4 mm, 0.31 sigma off), kappa 0.0015 (sigma 0.0022,
    1.57 sigma off: kappa carries the errors-in-variables bias of DESIGN.md K21); t_cl error of CamLaserCalibration 21.6 mm on the
    uncorrected set, 4.2 mm on the corrected one."""
    name = "radtan"
    cam = cases.CAMERAS[name]
    p = cases.problem(name, 102, 10, 144, 100, offset=0.02, scale=0.005)
    a = cases.arrays([p])
    q0, t0, _, st, _ = sv.board_poses(cam, a["corners"], a["board"], a["coff"])
    assert np.all(st == 1)
    obs = simdata.ObservationSet(q0, t0, a["poff"], a["pts"], a["poff"].copy(), a["pts"].copy())
    Tcl0 = simdata.T_from_pose7(p["pose_cl0"])
    cp, bx = [im[0] for im in p["images"]], [im[1] for im in p["images"]]
    Tcl, refined, rep = calib.CamLaserCalibrationRange(cam, cp, bx, obs, Tcl0, solver=sv)
    raw = sv.joint_refine_range(cam, a["corners"], a["board"], a["coff"], a["pts"], a["poff"], q0, t0, simdata.pose7_from_T(Tcl0)[None])
    assert np.array_equal(refined.tag_q, raw["q"]) and np.array_equal(refined.tag_t, raw["t"]) and np.array_equal(rep["H_cr"], raw["H_cr"][0])
    assert (rep["range_offset"], rep["range_scale"]) == (raw["range"][0][0], raw["range"][0][1])
    assert rep["termination"].startswith("CONVERGENCE") and rep["singular_values"].shape == (8,) and np.all(rep["singular_values"] > 0)
    assert rep["sigma"].shape == (8,) and np.all(rep["sigma"] > 0) and rep["corr_offset_tcl"].shape == (3,)
    assert np.all(np.abs(rep["corr_offset_tcl"]) < 1) and np.all(rep["status"] == 1)
    nb, nk = abs(rep["range_offset"] - 0.02) / rep["sigma"][6], abs(rep["range_scale"] - 0.005) / rep["sigma"][7]
    print("planted 0.02 m / 0.5 %%: b %.4f (sigma %.4f, %.2f sigma off), kappa %.5f (sigma %.5f, %.2f sigma off)" % (
        rep["range_offset"], rep["sigma"][6], nb, rep["range_scale"], rep["sigma"][7], nk))
    assert nb <= 4.0 and nk <= 4.0
    # a held scale: NaN sigma for it, its value kept
    _, _, rep2 = calib.CamLaserCalibrationRange(cam, cp, bx, obs, Tcl0, range0=(0.0, 0.005), hold=("scale",), solver=sv)
    assert rep2["range_scale"] == 0.005 and np.isnan(rep2["sigma"][7]) and rep2["sigma"][6] < rep["sigma"][6]
    # the tag poses and points alone
    Tcl3, same, rep3 = calib.CamLaserCalibrationRange(None, None, None, obs, Tcl0, hold_board_poses=True, solver=sv)
    assert np.array_equal(same.tag_q, obs.tag_q) and rep3["cost_corner"] == 0.0 and rep3["termination"].startswith("CONVERGENCE")
    # the corrected set in the point-to-plane solve
    truth = simdata.T_from_pose7(p["pose_cl_true"])
    fixed = calib.ApplyRangeCorrection(refined, rep["range_offset"], rep["range_scale"], solver=sv)
    assert np.array_equal(fixed.pts, sv.range_correct(obs.pts, rep["range_offset"], rep["range_scale"])) and np.array_equal(fixed.ptl, fixed.pts)
    errs = []
    for o in (refined, fixed):
        T = Tcl0.copy()
        calib.CamLaserCalibration(o, T, use_linefitting_data=False, solver=sv, verbose=False)
        errs.append(np.abs(T[:3, 3] - truth[:3, 3]).max())
    print("CamLaserCalibration, t_cl error: uncorrected %.1f mm, corrected %.1f mm; K21's own %.1f mm" % (
        1e3 * errs[0], 1e3 * errs[1], 1e3 * np.abs(Tcl[:3, 3] - truth[:3, 3]).max()))
    assert errs[1] < errs[0]
