"""K23 on the MI355X: clc_calibrate_full against the host build of the same code (tests/shim/fullcal_shim.cpp) and the restatement
(tests/fullcal_ref.py) on one batch per camera model — the seeded sets and the edge problems of tests/fullcal_cases.py in ONE call
(images per problem W - 1, W, W + 1, T + 1; corners 3, 4, 63, 64, 65, 144; points 0, 1, 63, 64, 65, 1 081; no laser at all), the
problems of 1 and 2 images in a call of their own with the distortion held, compared on the cost; two runs and a problem alone
against the batch, bit for bit; the device-array form behind pads (device offsets above 0), keep with holes and a dropped problem,
bit for bit against the host-array form; 257 problems in one call; held parameters; the reductions onto clc_camera_calibrate and
clc_joint_refine_range on the device; the refusals through the C ABI; the Python front end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fullcal_cases as cases  # noqa: E402
import test_fullcal_host as FH  # noqa: E402
import test_gpu_camcal as GC  # noqa: E402
import test_gpu_laserrange as GL  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi, calib, simdata  # noqa: E402
from camlasercalibratool_amd.camera import ClcCamera  # noqa: E402

pytestmark = pytest.mark.gpu
CAMS = FH.CAMS
# Measured on the MI355X on the batch, worst of both cameras (test_batch_matches_host_build_and_restatement's docstring), asserted
# one decade above, within the project's gates (1e-6 on poses, 1e-8 relative on cost):
GPU_HOST_POSE_BOUND = 6.6e-7     # device against the host build, any R entry or t component, well-posed problems (6.53e-8)
GPU_HOST_SIGMA_BOUND = 2.4e-5    # device against the host build, the free shared parameters in units of their 1 sigma from H_full (2.36e-6)
GPU_HOST_COST_BOUND = 4.5e-13     # device against the host build, relative final cost (4.48e-14)
GPU_HOST_H_BOUND = 7.3e-7        # device against the host build, H_full relative in the Frobenius norm, well-posed problems (7.29e-8)
GPU_HOST_WEIGHT_BOUND = 4.1e-6   # device against the host build, any weight of a well-posed problem (4.07e-7)
GPU_FEW_COST_BOUND = 5.4e-13      # 1 and 2 images, distortion held: relative final cost against the host build (5.39e-14)
GPU_REF_POSE_BOUND = 2.3e-7      # device against the restatement on the seeded sets: poses (2.22e-8)
GPU_REF_SIGMA_BOUND = 3.2e-5     # ... the free shared parameters in units of their sigma (3.13e-6)
GPU_REF_COST_BOUND = 2.3e-13      # ... final cost and cost shares (2.30e-14)
GPU_REF_H_BOUND = 1.2e-7         # ... H_full at the restatement's minimiser (1.13e-8)
GPU_REF_WEIGHT_BOUND = 1.2e-6    # ... the weights at the restatement's minimiser (1.19e-7)
assert GPU_HOST_POSE_BOUND <= FH.POSE_GATE and GPU_HOST_COST_BOUND <= FH.COST_GATE and GPU_REF_POSE_BOUND <= FH.POSE_GATE
ITERATIONS = 200  # as the sibling tests: the shapes whose minimiser is a valley need more than the 50 of the pose options
SEEDED = len(cases.SEEDED)
REF_COMPARED = 2  # the seeded sets held against the dense restatement here (6 and 8 images, the second contaminated): seconds each
FEW_MASK = 0xF0  # the distortion held


@pytest.fixture(scope="module")
def sv():
    with clc.Solver(0) as s:
        yield s


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return FH.build_shim(str(tmp_path_factory.mktemp("fcg") / "libfullcal_shim.so"))


def make_entry(shim, problems, notes, mask=None):
    a = cases.arrays(problems)
    cams = [p["cam0"] for p in problems]
    q0, t0 = FH.problem_starts(shim, problems, a)
    fo = FH.full_options(shim, cams[0].model) if mask is None else FH.full_options(shim, cams[0].model, hold_intrinsics_mask=mask)
    return dict(problems=problems, notes=notes, a=a, cams=cams, q0=q0, t0=t0, fo=fo,
                s=FH.shim_full(shim, cams, a, q0, t0, fo=fo, max_iterations=ITERATIONS))


@pytest.fixture(scope="module")
def batch(shim):
    """Per camera: the seeded sets, then the edge problems of more than two images, as ONE call; the problems of one and two images as
    a second call with the distortion held; the start poses by the shim's K10 under every problem's start camera; the shim's results
    — computed once."""
    out = {}
    for name in CAMS:
        problems = cases.seeded(name)
        edge, notes = cases.edge_problems(name)
        few = [edge[notes["images1"]], edge[notes["images2"]]]
        keep = [k for k in range(len(edge)) if k not in (notes["images1"], notes["images2"])]
        notes = {nm: len(problems) + keep.index(k) for nm, k in notes.items() if k in keep}
        out[name] = make_entry(shim, problems + [edge[k] for k in keep], notes)
        out[name]["few"] = make_entry(shim, few, {}, FEW_MASK)
    return out


def pose_options():
    o = _capi.default_pose_options()
    o.max_num_iterations = ITERATIONS
    return o


def device(sv, e, sel=None, fo=None, range0=None, keep=None, poses_cl=None):
    """The host-array form on the batch (sel: a subset of its problems, in order)."""
    a = e["a"]
    r0 = a["range0"] if range0 is None else range0
    cl0 = a["poses_cl0"] if poses_cl is None else poses_cl
    fo = fo or e["fo"]
    if sel is None:
        return sv.calibrate_full(e["cams"], a["corners"], a["board"], a["coff"], a["pts"], a["poff"], e["q0"], e["t0"], cl0, range0=r0,
                                 problem_offsets=a["prob_off"], keep=keep, options=pose_options(), full=fo)
    img = np.concatenate([np.arange(a["prob_off"][k], a["prob_off"][k + 1]) for k in sel])
    ci = np.concatenate([np.arange(a["coff"][i], a["coff"][i + 1]) for i in img])
    pi = np.concatenate([np.arange(a["poff"][i], a["poff"][i + 1]) for i in img]).astype(int)
    cs = lambda off, idx: np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in idx])]).astype(np.int64)
    pr = np.concatenate([[0], np.cumsum([a["prob_off"][k + 1] - a["prob_off"][k] for k in sel])]).astype(np.int64)
    r = sv.calibrate_full([e["cams"][k] for k in sel], a["corners"][ci], a["board"][ci], cs(a["coff"], img), a["pts"][pi], cs(a["poff"], img),
                          e["q0"][img], e["t0"][img], cl0[sel], range0=r0[sel], problem_offsets=pr, keep=None if keep is None else keep[img],
                          options=pose_options(), full=fo)
    r["images"], r["corner_idx"], r["point_idx"] = img, ci, pi
    return r


def k_of(r):
    return np.array([list(c.proj) + list(c.dist) for c in r["cameras"]])


def same_bits(x, y, images=None, problems=None, corners=None, points=None):
    """x (a run on a subset, or a whole run) against the whole run y."""
    ii = slice(None) if images is None else images
    pp = slice(None) if problems is None else problems
    for key in ("q", "t", "status"):
        assert np.array_equal(x[key], y[key][ii]), key
    for key in ("poses_cl", "range", "H_full", "cost_parts", "rms_px"):
        assert np.array_equal(x[key], y[key][pp], equal_nan=True), key
    assert np.array_equal(k_of(x), k_of(y)[pp])
    assert np.array_equal(x["w_corner"], y["w_corner"][slice(None) if corners is None else corners], equal_nan=True)
    assert np.array_equal(x["w_laser"], y["w_laser"][slice(None) if points is None else points], equal_nan=True)
    ys = [y["summaries"][k] for k in (range(len(y["poses_cl"])) if problems is None else problems)]
    for k, smy in enumerate(ys):
        smx = x["summaries"][k]
        assert (smx.termination, smx.num_iterations, smx.num_evaluations, smx.final_cost, smx.initial_cost) == \
               (smy.termination, smy.num_iterations, smy.num_evaluations, smy.final_cost, smy.initial_cost), k


def free_of(e, k, fo=None):
    fo = fo or e["fo"]
    a = e["a"]
    nl = a["poff"][a["prob_off"][k + 1]] == a["poff"][a["prob_off"][k]]
    return FH.ref.free_shared(no_laser=nl, **FH.hold_kw(fo))


def well_posed_H(H, free):
    """The marginal information over the free set has full rank by test_joint_host.well_posed's threshold."""
    if not free or not np.all(np.isfinite(H)):
        return False
    Hf = H[np.ix_(free, free)]
    if np.any(np.diag(Hf) <= 0):
        return False
    sc = np.sqrt(np.diag(Hf))
    w = np.linalg.eigvalsh(Hf / np.outer(sc, sc))
    return w[0] > 1e-9 * w[-1]


def host_gaps(e, g, s, k):
    """Problem k of a device run g against the host build's s -> (pose gap, shared gap in sigma, H_full gap, weight gap) or None where
    the minimiser is not unique."""
    a = e["a"]
    free = free_of(e, k)
    if not (well_posed_H(s["H_full"][k], free) and well_posed_H(g["H_full"][k], free)):
        return None
    idx = [i for i in range(a["prob_off"][k], a["prob_off"][k + 1]) if s["status"][i] == 1]
    sig = np.full(16, np.nan)
    sig[free] = np.sqrt(np.diag(np.linalg.inv(s["H_full"][k][np.ix_(free, free)])))
    G, S = FH.state_of(dict(g, k=k_of(g)), idx, k), FH.state_of(s, idx, k)
    dR = S[2].T @ G[2]
    dth = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2.0
    delta = np.r_[G[3] - S[3], dth, G[4] - S[4], G[5] - S[5], G[6] - S[6]]
    pose = max([np.abs(x - y).max() for x, y in zip(G[0], S[0])] + [np.abs(x - y).max() for x, y in zip(G[1], S[1])] +
               [np.abs(G[2] - S[2]).max(), np.abs(G[3] - S[3]).max()])
    wg, ws = FH.weights_of(a, g, idx), FH.weights_of(a, s, idx)
    return (pose, float(np.max(np.abs(delta[free]) / sig[free])), np.linalg.norm(g["H_full"][k] - s["H_full"][k]) / np.linalg.norm(s["H_full"][k]),
            max(np.abs(wg[0] - ws[0]).max(initial=0.0), np.abs(wg[1] - ws[1]).max(initial=0.0)))


@pytest.mark.parametrize("name", CAMS)
def test_batch_matches_host_build_and_restatement(sv, shim, batch, name):
    """The seeded sets and the edge problems in one call: the statuses are the host build's; poses, shared parameters, final cost,
    H_full and weights against the host build (but for the cost, where H_full has full rank on the free set); the problems of one and
    two images, distortion held, on the cost; the first two seeded sets against the restatement; a second run gives the same bits.
    Measured on the MI355X (radtan / kb): against the host build pose 1.66e-8 / 6.53e-8, the shared parameters 2.36e-6 / 2.11e-6 of their
    sigma, cost 8.77e-15 / 4.48e-14, H_full 1.53e-8 / 7.29e-8, weights 2.71e-7 / 4.07e-7 (device and host differ by FMA contraction, the
    reciprocal square roots of the factorisations and the platform's log1p; they stop up to a few iterations apart); one and two
    images 3.79e-15 / 5.39e-14; against the restatement pose 2.22e-8 / 7.13e-9, shared 3.13e-6 / 8.49e-7 sigma, cost 2.03e-15 / 2.30e-14,
    H_full 1.13e-8 / 4.23e-9, weights 1.19e-7 / 3.10e-8.  The module's bounds are one decade above the worst."""
    e = batch[name]
    a, notes, s = e["a"], e["notes"], e["s"]
    g = device(sv, e)
    assert np.array_equal(g["status"], s["status"])
    want = np.ones(len(a["poff"]) - 1, np.int32)
    want[a["prob_off"][notes["corners"]]] = 0  # 3 corners
    assert np.array_equal(g["status"], want)
    worst = dict(host_pose=0.0, host_sigma=0.0, host_cost=0.0, host_h=0.0, host_w=0.0)
    compared = []
    for k in range(len(e["problems"])):
        smg, sms = g["summaries"][k], s["summaries"][k]
        assert smg.termination in (1, 2, 3, 4, 5) and sms.termination in (1, 2, 3, 4, 5), (k, smg.termination, sms.termination)
        assert smg.final_cost <= smg.initial_cost
        gaps = host_gaps(e, g, s, k)
        print("%s problem %d: device vs host build: cost %.2e iterations %d / %d %s" % (
            name, k, abs(smg.final_cost - sms.final_cost) / sms.final_cost, smg.num_iterations, sms.num_iterations,
            "" if gaps is None else "pose %.2e shared %.2e sigma H_full %.2e w %.2e" % gaps))
        if gaps is not None:
            compared.append(k)
            worst["host_cost"] = max(worst["host_cost"], abs(smg.final_cost - sms.final_cost) / sms.final_cost)
            for key, v in zip(("host_pose", "host_sigma", "host_h", "host_w"), gaps):
                worst[key] = max(worst[key], v)
        for key in ("q", "t", "poses_cl", "range"):
            assert np.all(np.isfinite(g[key])), key
    assert set(range(SEEDED)) <= set(compared)
    assert all(notes[nm] in compared for nm in ("images%d" % (cases.WAVES + 1), "corners", "points", "nolaser"))
    # the images that take no part keep their poses and get NaN weights; the problem without a laser point its T_cl and range
    for i in np.flatnonzero(g["status"] != 1):
        assert np.array_equal(g["q"][i], e["q0"][i]) and np.array_equal(g["t"][i], e["t0"][i])
        assert np.all(np.isnan(g["w_corner"][a["coff"][i]:a["coff"][i + 1]])) and np.all(np.isnan(g["w_laser"][a["poff"][i]:a["poff"][i + 1]]))
    kn = notes["nolaser"]
    assert np.array_equal(g["poses_cl"][kn], a["poses_cl0"][kn]) and np.array_equal(g["range"][kn], a["range0"][kn])
    assert np.all(g["H_full"][kn][:8, :] == 0) and np.all(g["H_full"][kn][:, :8] == 0)
    print("%s: device vs host build, worst gaps %s (problems %s)" % (name, {k: "%.2e" % v for k, v in worst.items()}, compared))
    # one and two images, the distortion held: the cost
    f = e["few"]
    gf = device(sv, f)
    few = max(abs(gf["summaries"][k].final_cost - f["s"]["summaries"][k].final_cost) / f["s"]["summaries"][k].final_cost for k in range(2))
    print("%s: one and two images, distortion held: cost vs host build %.2e" % (name, few))
    assert np.array_equal(k_of(gf)[:, 4:], np.array([FH.TC.k_of(c)[4:] for c in f["cams"]])) and np.all(gf["status"] == 1)
    # the seeded sets against the restatement
    wr = {}
    for k in range(REF_COMPARED):
        c = FH.compare_problem(e["cams"][k], a, k, dict(g, k=k_of(g)), e["q0"], e["t0"], e["fo"])
        for key in ("pose", "tcl", "shared_sigma", "cost", "cost_self", "parts", "h", "h_same", "w", "w_same"):
            wr[key] = max(wr.get(key, 0.0), c[key])
    print("%s: device vs the restatement on the seeded sets, worst gaps %s" % (name, {k: "%.2e" % v for k, v in wr.items()}))
    assert worst["host_pose"] <= GPU_HOST_POSE_BOUND and worst["host_sigma"] <= GPU_HOST_SIGMA_BOUND and worst["host_cost"] <= GPU_HOST_COST_BOUND
    assert worst["host_h"] <= GPU_HOST_H_BOUND and worst["host_w"] <= GPU_HOST_WEIGHT_BOUND and few <= GPU_FEW_COST_BOUND
    assert max(wr["pose"], wr["tcl"]) <= GPU_REF_POSE_BOUND and wr["shared_sigma"] <= GPU_REF_SIGMA_BOUND
    assert max(wr["cost"], wr["cost_self"], wr["parts"]) <= GPU_REF_COST_BOUND and wr["h"] <= GPU_REF_H_BOUND and wr["w"] <= GPU_REF_WEIGHT_BOUND
    assert wr["h_same"] <= FH.H_SAME_POINT and wr["w_same"] <= FH.WEIGHT_SAME_POINT
    # a second run gives the same bits
    same_bits(device(sv, e), g)


def test_problem_alone_equals_the_problem_in_the_batch(sv, batch):
    e = batch["radtan"]
    g = device(sv, e)
    for nm in ("images%d" % (cases.WAVES - 1), "images%d" % (cases.THREADS + 1), "points", "nolaser"):
        k = e["notes"][nm]
        r = device(sv, e, [k])
        same_bits(r, g, r["images"], [k], r["corner_idx"], r["point_idx"])
    two = [e["notes"]["corners"], 1]
    r = device(sv, e, two)
    same_bits(r, g, r["images"], two, r["corner_idx"], r["point_idx"])
    f = batch["radtan"]["few"]
    gf = device(sv, f)
    r = device(sv, f, [1])
    same_bits(r, gf, r["images"], [1], r["corner_idx"], r["point_idx"])


def test_device_form_keep_and_dropped_problem_equal_the_host_form(sv, batch):
    """Every array in device memory, the call's images, corners and points behind pads (device offsets above 0), keep with holes and a
    problem with every image dropped: the bits of the host-array call; the dropped problem ends CLC_FAILURE with everything untouched
    and NaN weights; the entries ahead of the call's images are left as they are."""
    import torch
    e = batch["kb"]
    a = e["a"]
    n, npb = len(a["coff"]) - 1, len(a["prob_off"]) - 1
    keep = np.ones(n, bool)
    keep[[1, 4]] = False
    kd = e["notes"]["images%d" % cases.WAVES]
    keep[a["prob_off"][kd]:a["prob_off"][kd + 1]] = False
    g = device(sv, e, keep=keep)
    assert g["summaries"][kd].termination == 6 and np.all(np.isnan(g["H_full"][kd])) and np.array_equal(g["poses_cl"][kd], a["poses_cl0"][kd])
    assert np.array_equal(k_of(g)[kd], FH.TC.k_of(e["cams"][kd])) and np.all(g["status"][~keep] == -1)
    assert np.all(np.isnan(g["w_laser"][a["poff"][a["prob_off"][kd]]:a["poff"][a["prob_off"][kd + 1]]]))
    assert g["summaries"][0].termination in (1, 2, 3) and np.array_equal(g["q"][1], e["q0"][1])
    pi, pc, pp = 3, 7, 5  # images, corners and points that belong to nothing
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    dc = up(np.concatenate([np.full((pc, 2), 1e6, np.float32), a["corners"]]))
    db = up(np.concatenate([np.full((pc, 2), -3.0, np.float32), a["board"]]))
    dp = up(np.concatenate([np.full((pp, 3), np.nan), a["pts"]]))
    dco = up(np.concatenate([np.zeros(pi, np.int64), a["coff"] + pc]))
    dpo = up(np.concatenate([np.zeros(pi, np.int64), a["poff"] + pp]))
    dpr = up(a["prob_off"] + pi)
    dk = up(np.concatenate([np.ones(pi, np.uint8), keep.astype(np.uint8)]))
    cams = (ClcCamera * npb)(*[c.to_c() for c in e["cams"]])
    dcam = up(np.frombuffer(bytes(cams), dtype=np.uint8).copy())
    dq = up(np.concatenate([np.full((pi, 4), -7.0), e["q0"]]))
    dt = up(np.concatenate([np.full((pi, 3), -7.0), e["t0"]]))
    dcl, drg = up(a["poses_cl0"]), up(a["range0"])
    dst = torch.full((pi + n,), -7, dtype=torch.int32, device=dev)
    dH = torch.full((npb, 256), -7.0, dtype=torch.float64, device=dev)
    dparts = torch.full((npb, 2), -7.0, dtype=torch.float64, device=dev)
    drms = torch.full((npb,), -7.0, dtype=torch.float64, device=dev)
    dwc = torch.full((pc + len(a["corners"]),), -7.0, dtype=torch.float64, device=dev)
    dwl = torch.full((pp + len(a["pts"]),), -7.0, dtype=torch.float64, device=dev)
    dsm = torch.zeros(npb * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sv.calibrate_full_device(dcam.data_ptr(), dc.data_ptr(), db.data_ptr(), dco.data_ptr(), dp.data_ptr(), dpo.data_ptr(), n, npb, dq.data_ptr(),
                             dt.data_ptr(), dcl.data_ptr(), drg.data_ptr(), dsm.data_ptr(), dst.data_ptr(), problem_offsets_ptr=dpr.data_ptr(),
                             keep_ptr=dk.data_ptr(), H_full_ptr=dH.data_ptr(), cost_parts_ptr=dparts.data_ptr(), rms_ptr=drms.data_ptr(),
                             w_corner_ptr=dwc.data_ptr(), w_laser_ptr=dwl.data_ptr(), options=pose_options(), full=e["fo"])
    assert np.all(dq.cpu().numpy()[:pi] == -7.0) and np.all(dst.cpu().numpy()[:pi] == -7)  # ahead of the call's images
    assert np.all(dwc.cpu().numpy()[:pc] == -7.0) and np.all(dwl.cpu().numpy()[:pp] == -7.0)
    back = (ClcCamera * npb).from_buffer_copy(dcam.cpu().numpy().tobytes())
    r = dict(q=dq.cpu().numpy()[pi:], t=dt.cpu().numpy()[pi:], status=dst.cpu().numpy()[pi:], poses_cl=dcl.cpu().numpy(), range=drg.cpu().numpy(),
             H_full=dH.cpu().numpy().reshape(npb, 16, 16), cost_parts=dparts.cpu().numpy(), rms_px=drms.cpu().numpy(),
             w_corner=dwc.cpu().numpy()[pc:], w_laser=dwl.cpu().numpy()[pp:], cameras=list(back),
             summaries=(_capi.Summary * npb).from_buffer_copy(dsm.cpu().numpy().tobytes()))
    same_bits(r, g)


def test_257_problems_in_one_call(sv, batch):
    """257 problems (more than one workgroup's threads) in one call: each the bits of the problem in a call of 1 and of 2."""
    e = batch["radtan"]
    base = [0, 1, e["notes"]["corners"], e["notes"]["nolaser"]]
    sel = (base * 65)[:257]
    r = device(sv, e, sel)
    one = {k: device(sv, e, [k]) for k in base[:2]}
    two = device(sv, e, base[2:])
    a = e["a"]
    for j in (0, 1, 2, 3, 128, 129, 255, 256):
        k = sel[j]
        ref_run, kk = (one[k], 0) if k in one else (two, base[2:].index(k))
        assert np.array_equal(r["poses_cl"][j], ref_run["poses_cl"][kk]) and np.array_equal(r["range"][j], ref_run["range"][kk])
        assert np.array_equal(r["H_full"][j], ref_run["H_full"][kk], equal_nan=True) and np.array_equal(k_of(r)[j], k_of(ref_run)[kk])
        assert r["summaries"][j].final_cost == ref_run["summaries"][kk].final_cost


def test_held_parameters_keep_their_bits(sv, batch):
    """Every single held bit keeps its parameter's bits while the others move, hold_extrinsic T_cl's, hold_board_poses the board poses';
    the rows and columns of H_full of a held parameter are zero."""
    e = batch["radtan"]
    a = e["a"]
    sel = [0, 1]
    r0 = np.tile([0.0123456789, -0.00456789], (len(e["problems"]), 1))
    k0 = np.array([FH.TC.k_of(e["cams"][k]) for k in sel])
    for bit in range(10):
        fo = FH.full_options_from(e["fo"], **(dict(hold_intrinsics_mask=1 << bit) if bit < 8 else dict(hold_range_mask=1 << (bit - 8))))
        g = device(sv, e, sel, fo=fo, range0=r0)
        x0, x1 = np.c_[r0[sel], k0], np.c_[g["range"], k_of(g)]
        j = bit + 2 if bit < 8 else bit - 8
        assert np.array_equal(x1[:, j], x0[:, j]) and np.all(np.delete(x1, j, 1) != np.delete(x0, j, 1)), bit
        hj = 8 + bit if bit < 8 else 6 + bit - 8
        assert np.all(g["H_full"][:, hj, :] == 0) and np.all(g["H_full"][:, :, hj] == 0)
    g = device(sv, e, sel, fo=FH.full_options_from(e["fo"], hold_extrinsic=1))
    assert np.array_equal(g["poses_cl"], a["poses_cl0"][sel]) and np.all(g["range"] != 0) and np.all(k_of(g) != k0)
    assert np.all(g["H_full"][:, :6, :] == 0) and np.all(g["H_full"][:, :, :6] == 0)
    g = device(sv, e, sel, fo=FH.full_options_from(e["fo"], hold_board_poses=1))
    assert np.array_equal(g["q"], e["q0"][g["images"]]) and np.array_equal(g["t"], e["t0"][g["images"]]) and np.all(g["H_full"][:, :8, 8:] == 0)
    assert not np.array_equal(g["poses_cl"], a["poses_cl0"][sel])


@pytest.mark.parametrize("name", CAMS)
def test_reductions_onto_the_staged_calls(sv, batch, name):
    """Reduction (a): the problem without a laser point, loss_corner = 0: T_cl and range bit for bit; camera, poses, cost, RMS and the
    intrinsics' block of H_full against clc_camera_calibrate on the device at that call's own GPU bounds (test_gpu_camcal).
    Reduction (b): all intrinsics held, hold_board_poses, both losses 0: T_cl, b, kappa, cost and the leading 8x8 of H_full against
    clc_joint_refine_range with hold_board_poses on the device at that call's own GPU bounds (test_gpu_laserrange); loss 0 gives
    weights 1.  Measured on the MI355X (radtan / kb): (a) intrinsics 3.85e-7 sigma / 1e-17, poses 2.52e-9 / 0,
    cost 2.07e-15 / 0, RMS 1.07e-15 / 0, H_cam 4.64e-9 / 0; (b) T_cl 1.34e-8 / 1.67e-16, b and kappa 3.19e-7 / 9.45e-14 sigma, cost
    2.74e-15 / 1.66e-16, H 1.33e-8 / 3.16e-16 (two kernels of the same sums: the compiler contracts them differently in places)."""
    e = batch[name]
    a = e["a"]
    kn = e["notes"]["nolaser"]
    fo = FH.full_options_from(e["fo"], loss_corner=0.0)
    g = device(sv, e, [kn], fo=fo)
    img = g["images"]
    cs = np.concatenate([[0], np.cumsum([a["coff"][i + 1] - a["coff"][i] for i in img])]).astype(np.int64)
    co = _capi.default_camcal_options(e["cams"][kn].model)
    c19 = sv.camera_calibrate(e["cams"][kn], a["corners"][g["corner_idx"]], a["board"][g["corner_idx"]], cs, e["q0"][img], e["t0"][img],
                              options=pose_options(), camcal=co)
    assert np.array_equal(g["poses_cl"][0], a["poses_cl0"][kn]) and np.array_equal(g["range"][0], a["range0"][kn]) and np.all(g["w_corner"] == 1.0)
    free = [j for j in range(8) if not (co.hold_mask >> j) & 1]
    sg = np.sqrt(np.diag(np.linalg.inv(c19["H_cam"][0][np.ix_(free, free)])))
    k19 = k_of(c19)[0]
    gaps = dict(param=np.max(np.abs(k_of(g)[0] - k19)[free] / sg), pose=max(np.abs(g["q"] - c19["q"]).max(), np.abs(g["t"] - c19["t"]).max()),
                cost=abs(g["summaries"][0].final_cost - c19["summaries"][0].final_cost) / c19["summaries"][0].final_cost,
                rms=abs(g["rms_px"][0] - c19["rms_px"][0]) / c19["rms_px"][0],
                hcam=np.linalg.norm(g["H_full"][0][8:, 8:] - c19["H_cam"][0]) / np.linalg.norm(c19["H_cam"][0]))
    print("%s (a) no laser vs clc_camera_calibrate on the device: %s" % (name, {k: "%.2e" % v for k, v in gaps.items()}))
    assert gaps["param"] <= GC.GPU_HOST_PARAM_SIGMA and gaps["pose"] <= GC.GPU_HOST_POSE_BOUND and gaps["cost"] <= GC.GPU_HOST_COST_BOUND
    assert gaps["rms"] <= GC.GPU_HOST_COST_BOUND and gaps["hcam"] <= GC.GPU_HOST_HCAM_BOUND
    sel = list(range(SEEDED))
    fo = FH.full_options_from(e["fo"], hold_intrinsics_mask=0xFF, hold_board_poses=1, loss_corner=0.0, loss_laser=0.0)
    g = device(sv, e, sel, fo=fo)
    ro = _capi.default_range_options(None)
    ro.hold_board_poses = 1
    img, pi = g["images"], g["point_idx"]
    ps = np.concatenate([[0], np.cumsum([a["poff"][i + 1] - a["poff"][i] for i in img])]).astype(np.int64)
    k21 = sv.joint_refine_range(None, None, None, None, a["pts"][pi], ps, e["q0"][img], e["t0"][img], a["poses_cl0"][sel], range0=a["range0"][sel],
                                problem_offsets=np.concatenate([[0], np.cumsum([a["prob_off"][k + 1] - a["prob_off"][k] for k in sel])]).astype(np.int64),
                                options=pose_options(), range_options=ro)
    assert np.array_equal(g["q"], e["q0"][img]) and np.all(g["w_laser"] == 1.0) and np.all(np.isnan(g["w_corner"]))
    w = dict(pose=np.abs(g["poses_cl"] - k21["poses_cl"]).max(), range=0.0, cost=0.0, h=0.0)
    for k in range(len(sel)):
        sig = np.sqrt(np.diag(np.linalg.inv(k21["H_cr"][k])))
        w["range"] = max(w["range"], np.max(np.abs(g["range"][k] - k21["range"][k]) / sig[6:]))
        w["cost"] = max(w["cost"], abs(g["summaries"][k].final_cost - k21["summaries"][k].final_cost) / k21["summaries"][k].final_cost)
        w["h"] = max(w["h"], np.linalg.norm(g["H_full"][k][:8, :8] - k21["H_cr"][k]) / np.linalg.norm(k21["H_cr"][k]))
        assert np.all(g["H_full"][k][8:, :] == 0) and np.all(g["H_full"][k][:, 8:] == 0) and g["cost_parts"][k][0] == 0.0
    print("%s (b) held camera and board poses vs clc_joint_refine_range on the device: %s" % (name, {k: "%.2e" % v for k, v in w.items()}))
    assert w["pose"] <= GL.GPU_HOST_POSE_BOUND and w["range"] <= GL.GPU_HOST_RANGE_BOUND and w["cost"] <= GL.GPU_HOST_COST_BOUND
    assert w["h"] <= GL.GPU_HOST_HCR_BOUND


def test_refusals_through_the_c_abi(sv):
    """With a live handle: the refusals come before any device work and leave every output as it was."""
    L = _capi.lib()
    z = np.zeros(2, dtype=np.int64)
    q, t, cl, rg, st = np.full(4, 5.0), np.full(3, 5.0), np.full(7, 5.0), np.full(2, 5.0), np.full(1, 5, np.int32)
    cam = (ClcCamera * 1)(FH.H.CAMERAS["pinhole"].to_c())
    d = FH.d

    def call(fo, fn=L.clc_calibrate_full):
        return fn(sv._h, cam, None, C.byref(fo), None, None, d(z), None, d(z), None, C.c_size_t(1), None, C.c_size_t(1), d(q), d(t), d(cl), d(rg),
                  (_capi.Summary * 1)(), None, None, None, d(st), None, None)

    rows = [(dict(sigma_px=0.0), "sigma_px must be finite and > 0"), (dict(sigma_laser=float("nan")), "sigma_laser must be finite and > 0"),
            (dict(loss_corner=-1.0), "loss_corner must be finite and >= 0"), (dict(loss_laser=float("inf")), "loss_laser must be finite and >= 0"),
            (dict(hold_intrinsics_mask=0x1FF), "hold_intrinsics_mask has bits beyond the 8 intrinsics"),
            (dict(hold_range_mask=7), "hold_range_mask outside 0..3"),
            (dict(hold_intrinsics_mask=0xFF, hold_range_mask=3, hold_extrinsic=1, hold_board_poses=1), "everything is held")]
    for kw, msg in rows:
        for fn, who in ((L.clc_calibrate_full, "clc_calibrate_full: "), (L.clc_calibrate_full_device, "clc_calibrate_full_device: ")):
            assert call(FH.full_options_from(_capi.default_full_options(1), **kw), fn) == -1
            assert L.clc_last_error().decode() == who + msg
    assert np.all(q == 5.0) and np.all(cl == 5.0) and np.all(rg == 5.0) and st[0] == 5
    # zero problems: nothing to do
    assert L.clc_calibrate_full(sv._h, None, None, None, None, None, None, None, None, None, C.c_size_t(0), None, C.c_size_t(0), None, None, None,
                                None, None, None, None, None, None, None, None) == 0


def test_python_front_end(sv):
    """calib.CalibrateFull on 12 images with a planted 0.02 m / 0.5 % and K22's contamination, once from a given start camera and once
    with camera0 = None (CalibrateCamera's answer as the start): the raw call's bits, the report's shapes, every planted observation
    among the outliers, a held scale."""
    name = "radtan"
    p = cases.problem(name, 102, 12, 144, 100, dirty=True, offset=0.02, scale=0.005)
    a = cases.arrays([p])
    cam0 = p["cam0"]
    q0, t0, _, st, _ = sv.board_poses(cam0, a["corners"], a["board"], a["coff"])
    assert np.all(st == 1)
    obs = simdata.ObservationSet(q0, t0, a["poff"], a["pts"], a["poff"].copy(), a["pts"].copy())
    Tcl0 = simdata.T_from_pose7(p["pose_cl0"])
    cp, bx = [im[0] for im in p["images"]], [im[1] for im in p["images"]]
    cam, Tcl, b, kappa, refined, rep = calib.CalibrateFull(cam0, cp, bx, obs, Tcl0, hold=("scale",), solver=sv)
    fo = _capi.default_full_options(cam0.model)
    fo.hold_range_mask = 2
    raw = sv.calibrate_full(cam0, a["corners"], a["board"], a["coff"], a["pts"], a["poff"], q0, t0, simdata.pose7_from_T(Tcl0)[None], full=fo)
    assert np.array_equal(refined.tag_q, raw["q"]) and np.array_equal(refined.tag_t, raw["t"]) and np.array_equal(rep["H_full"], raw["H_full"][0])
    assert (b, kappa) == (raw["range"][0][0], 0.0) and tuple(cam.proj) == tuple(raw["cameras"][0].proj)
    assert rep["termination"].startswith("CONVERGENCE") and rep["sigma"].shape == (16,) and np.isnan(rep["sigma"][7])
    assert np.all(rep["sigma"][np.arange(16) != 7] > 0) and len(rep["names"]) == 16 and rep["rms_px"] > 0 and np.all(rep["status"] == 1)
    mc, mp = cases.planted_masks(p)
    down, frac = cases.separation(np.concatenate(rep["w_corner"]), np.concatenate(rep["w_laser"]), mc, mp)
    assert down and frac >= 0.95 and not np.any(np.concatenate(rep["inlier_corner"])[mc]) and not np.any(np.concatenate(rep["inlier_laser"])[mp])
    print("CalibrateFull (scale held): t_cl %.1f mm from the truth, b %.4f (sigma %.4f), sigma of t_cl %s mm" % (
        1e3 * cases.tcl_distance(simdata.pose7_from_T(Tcl), p["pose_cl_true"]), b, rep["sigma"][6], np.round(1e3 * rep["sigma"][:3], 2)))
    cam2, Tcl2, b2, k2, _, rep2 = calib.CalibrateFull(None, cp, bx, obs, Tcl0, hold=("scale",), model=cam0.model, width=cam0.width,
                                                      height=cam0.height, solver=sv)
    assert rep2["termination"].startswith("CONVERGENCE") and abs(rep2["cost"] - rep["cost"]) <= 1e-6 * rep["cost"]
    assert abs(cam2.proj[0] - cam.proj[0]) <= 1e-3 * rep["sigma"][8]
