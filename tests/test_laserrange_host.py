"""K21 (csrc/clc_laserrange.hpp on clc_arrow.hpp) on the host: the evaluation blocks with the range offset and scale, the traits of the
8-wide shared block and the outputs compiled with g++ (tests/shim/laserrange_shim.cpp) against the numpy / scipy restatement
tests/laserrange_ref.py on the seeded sets of tests/laserrange_cases.py: Jacobians against central differences; the minimiser, the
final cost, the cost shares and H_cr; inv(H_cr) against the dense normal matrix; recovery of a planted offset and scale; the
invariants against K18; held parameters; the route without corners; image status; the single-range problem; the refusals of the C
ABI (they need no device); the point correction; a stand-alone AddressSanitizer / UBSan program over the edge shapes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import joint_ref as jref  # noqa: E402
import laserrange_cases as cases  # noqa: E402
import laserrange_ref as ref  # noqa: E402
import test_campose_host as H  # noqa: E402
import test_joint_host as TJ  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402

CAMS = ["radtan", "kb"]
d = H._d

# The project's parity gates (test_joint_host.py).  The bounds below are one decade over the worst gaps measured in this file's tests,
# both cameras (the figures: the tests' docstrings), and lie within the gates.
POSE_GATE, COST_GATE = TJ.POSE_GATE, TJ.COST_GATE
POSE_BOUND = 2.7e-7       # largest gap of any R entry or t component (T_cl and every T_ca) to the restatement's minimiser (2.64e-8:
                          # the single-range problem with the scale held; the seeded sets 3.27e-9)
RANGE_SIGMA_BOUND = 5.4e-6  # gap of b and of kappa to the restatement's, in units of the parameter's predicted 1 sigma (5.34e-7 with
                          # the extrinsic held; the seeded sets 1.6e-7, without corners 3.9e-7, the single-range problem 4.5e-7)
COST_BOUND = 7.9e-14      # relative gap of the final cost and of the two cost shares (7.86e-15 without corners; the seeded sets 2.99e-15)
HCR_BOUND = 2.7e-8        # relative (Frobenius) gap of H_cr to the dense Schur complement at the restatement's minimiser (2.66e-9)
HCR_SAME_POINT = 2.6e-14  # the same at the answer's own point (2.51e-15)
INV_BOUND = 2.5e-12       # relative gap of inv(H_cr) to the leading 8x8 block of the inverse of the dense normal matrix (2.50e-13)
assert POSE_BOUND <= POSE_GATE and COST_BOUND <= COST_GATE


def build_shim(path):
    subprocess.check_call(TJ.GXX + ["-shared", os.path.join(HERE, "shim", "laserrange_shim.cpp"), "-o", path])
    L = C.CDLL(path)
    L.shim_kb_theta.restype = C.c_double
    L.shim_kb_theta.argtypes = [C.c_void_p, C.c_double]
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(str(tmp_path_factory.mktemp("lr") / "liblaserrange_shim.so"))


def shim_range_options(L, cam, **kw):
    ro = _capi.RangeOptions()
    c = cam.to_c() if cam is not None else None
    L.shim_range_options_default(C.byref(ro), C.byref(c) if c is not None else None)
    for k, v in kw.items():
        setattr(ro, k, v)
    return ro


def shim_range(L, cam, a, q0, t0, keep=None, ro=None, poses_cl=None, range0=None, corners=True, max_iterations=None):
    """shim_joint_refine_range on the arrays of laserrange_cases.arrays -> dict, the keys of Solver.joint_refine_range.
    corners=False: the three corner arrays are NULL (hold_board_poses)."""
    n, npb = len(a["poff"]) - 1, len(a["prob_off"]) - 1
    q, t = np.array(q0, dtype=np.float64, order="C"), np.array(t0, dtype=np.float64, order="C")
    pcl = np.array(a["poses_cl0"] if poses_cl is None else poses_cl, dtype=np.float64, order="C").reshape(npb, 7)
    rg = np.array(a["range0"] if range0 is None else range0, dtype=np.float64, order="C").reshape(npb, 2)
    sm = (_capi.Summary * max(npb, 1))()
    Hcr = np.empty((npb, 8, 8)); parts = np.empty((npb, 2)); st = np.full(n, -99, dtype=np.int32)
    k = None if keep is None else np.ascontiguousarray(np.asarray(keep).astype(np.uint8))
    o = _capi.Options()
    L.shim_pose_options_default(C.byref(o))
    if max_iterations is not None:
        o.max_num_iterations = max_iterations
    ro = ro or shim_range_options(L, cam)
    c = cam.to_c() if cam is not None else None
    L.shim_joint_refine_range(C.byref(c) if c is not None else None, C.byref(o), C.byref(ro), d(a["corners"]) if corners else None,
                              d(a["board"]) if corners else None, d(a["coff"]) if corners else None, d(a["pts"]), d(a["poff"]),
                              None if k is None else d(k), C.c_longlong(n), d(a["prob_off"]), C.c_longlong(npb), d(q), d(t), d(pcl), d(rg), sm,
                              d(Hcr), d(parts), d(st))
    return dict(q=q, t=t, poses_cl=pcl, range=rg, summaries=sm, H_cr=Hcr, cost_parts=parts, status=st)


def restatement_problem(L, cam, a, k, ro, keep=None):
    """Problem k of the arrays as laserrange_ref takes it (the participating images only) -> (prob, image indices).  With the board
    poses held no corner takes part."""
    hold = bool(ro.hold_board_poses)
    idx = [i for i in range(a["prob_off"][k], a["prob_off"][k + 1])
           if (hold or a["coff"][i + 1] - a["coff"][i] >= 4) and (keep is None or keep[i])]
    if hold:
        lifted = [np.zeros((0, 2)) for _ in idx]
        board = [np.zeros((0, 2)) for _ in idx]
    else:
        lf = H.shim_lift(L, cam, a["corners"]).astype(np.float32).astype(np.float64)
        lifted = [lf[a["coff"][i]:a["coff"][i + 1]] for i in idx]
        board = [a["board"][a["coff"][i]:a["coff"][i + 1]].astype(np.float64) for i in idx]
    prob = dict(lifted=lifted, board=board, pts=[a["pts"][a["poff"][i]:a["poff"][i + 1]] for i in idx],
                sc=1.0 if hold else ro.sigma_corner, sl=ro.sigma_laser)
    return prob, idx


def state_of(s, idx, k):
    Rs = [jref.quat_wxyz_to_R(s["q"][i]) for i in idx]
    ts = [s["t"][i].copy() for i in idx]
    Rcl, tcl = jref.pose7_to_Rt(s["poses_cl"][k])
    return Rs, ts, Rcl, tcl, float(s["range"][k][0]), float(s["range"][k][1])


def scaled_spectrum(prob, X, cols):
    Hd, _ = ref.normal_matrix(prob, *X)
    Hd = Hd[np.ix_(cols, cols)]
    s = np.sqrt(np.diag(Hd))
    return np.linalg.eigvalsh(Hd / np.outer(s, s))


def well_posed(prob, X, cols):
    """test_joint_host.well_posed over the 8-wide shared block."""
    w = scaled_spectrum(prob, X, cols)
    return w[0] > 1e-9 * w[-1]


def compare_problem(L, cam, a, k, s, q0, t0, ro, keep=None, range0=None):
    """One problem of a call against the restatement -> dict of gaps (pose / range None where the minimiser is not unique)."""
    prob, idx = restatement_problem(L, cam, a, k, ro, keep)
    r0 = a["range0"][k] if range0 is None else np.asarray(range0).reshape(-1, 2)[k]
    start = ([jref.quat_wxyz_to_R(q0[i]) for i in idx], [t0[i].copy() for i in idx], *jref.pose7_to_Rt(a["poses_cl0"][k]), float(r0[0]), float(r0[1]))
    mine = state_of(s, idx, k)
    no_laser = sum(len(p) for p in prob["pts"]) == 0
    kw = dict(hold_board=bool(ro.hold_board_poses), hold_ext=bool(ro.hold_extrinsic), mask=int(ro.hold_range_mask))
    cols = ref.columns(len(idx), no_laser=no_laser, **kw)
    # the restatement from the same start, and from the answer (scipy stops in shallow valleys: the lower of the two is its answer)
    cand = [ref.solve(prob, *start, **kw), ref.solve(prob, *mine, **kw)]
    best = min(cand, key=lambda c: c[6])
    cost = s["summaries"][k].final_cost
    cc, cl = ref.cost_parts(prob, *mine)
    out = dict(cost=abs(cost - best[6]) / best[6] if best[6] > 0 else abs(cost),
               cost_self=abs(cost - (cc + cl)) / (cc + cl) if cc + cl > 0 else abs(cost),
               parts=max(abs(s["cost_parts"][k][0] - cc), abs(s["cost_parts"][k][1] - cl)) / (cc + cl) if cc + cl > 0 else 0.0,
               pose=None, range_sigma=None, start_cost=0.5 * np.sum(ref.residuals(prob, *start, jac=False)[0] ** 2), ref_cost=best[6],
               prob=prob, idx=idx, best=best[:6], mine=mine, cols=cols)
    if well_posed(prob, best[:6], cols):
        out["pose"] = TJ.pose_gap(mine[:4], best[:4])
        Hd, _ = ref.normal_matrix(prob, *best[:6])
        free = [c for c in cols if c < 8]
        Hs = ref.schur(Hd) if not ro.hold_board_poses else Hd[:8, :8]
        sig = ref.free_sigma(Hs, free)
        gaps = [abs(mine[4 + j] - best[4 + j]) / sig[6 + j] for j in range(2) if np.isfinite(sig[6 + j])]
        out["range_sigma"] = max(gaps) if gaps else 0.0
        out["sigma"] = sig
    return out


def test_struct_layout(shim):
    assert shim.shim_range_options_size() == 32 == C.sizeof(_capi.RangeOptions)
    R = _capi.RangeOptions
    assert (R.sigma_corner.offset, R.sigma_laser.offset, R.hold_board_poses.offset, R.hold_extrinsic.offset, R.hold_range_mask.offset,
            R.reserved.offset) == (0, 8, 16, 20, 24, 28)
    cam = cases.CAMERAS["radtan"]
    ro = shim_range_options(shim, cam)
    assert ro.sigma_corner == 0.3 / np.sqrt(abs(cam.proj[0] * cam.proj[1])) and ro.sigma_laser == 0.01
    assert (ro.hold_board_poses, ro.hold_extrinsic, ro.hold_range_mask, ro.reserved) == (0, 0, 0, 0)
    assert shim_range_options(shim, None).sigma_corner == 0.0
    assert shim.shim_range_eval_doubles() == 121


def numeric_jacobian(prob, X, h=1e-6):
    """Central differences of the residual vector, column by column: the poses through the project's Plus, b and kappa additively."""
    Rs, ts, Rcl, tcl, b, k = X
    P = len(Rs)
    cols = []
    for c in range(8 + 6 * P):
        out = []
        for sgn in (1.0, -1.0):
            RR, tt, Rc, tc, bb, kk = list(Rs), list(ts), Rcl, tcl, b, k
            dl = np.zeros(6)
            if c < 6:
                dl[c] = sgn * h
                Rc, tc = jref.plus(Rcl, tcl, dl)
            elif c == 6:
                bb = b + sgn * h
            elif c == 7:
                kk = k + sgn * h
            else:
                i = (c - 8) // 6
                dl[(c - 8) % 6] = sgn * h
                RR[i], tt[i] = jref.plus(Rs[i], ts[i], dl)
            out.append(ref.residuals(prob, RR, tt, Rc, tc, bb, kk, jac=False)[0])
        cols.append((out[0] - out[1]) / (2 * h))
    return np.stack(cols, 1)


@pytest.mark.parametrize("name", CAMS)
def test_jacobians_match_central_differences(shim, name):
    """The restatement's analytic Jacobian (corner and laser rows; the 8 shared columns and every pose column) against central
    differences: relative to the largest entry of a column the differences of step 1e-6 carry ~1e-9 of truncation and rounding
    (measured: 1.15e-9), asserted at 1e-7.  The shim's per-image blocks A, B, g, C, g_c and the two cost parts are the restatement's
    J^T J and J^T r to rounding: measured 7.7e-15 relative to the largest entry of a block, asserted one decade above at 8e-14."""
    cam = cases.CAMERAS[name]
    p = cases.problem(name, 5, 3, [144, 65, 4], [100, 65, 0], offset=0.02, scale=-0.006)
    a = cases.arrays([p])
    ro = shim_range_options(shim, cam)
    prob, idx = restatement_problem(shim, cam, a, 0, ro)
    rng = np.random.default_rng(1)
    Rs = [im[2] @ jref.exp_so3(rng.normal(size=3) * 0.01) for im in p["images"]]
    ts = [im[3] + rng.normal(size=3) * 0.005 for im in p["images"]]
    Rcl, tcl = jref.pose7_to_Rt(p["pose_cl0"])
    X = (Rs, ts, Rcl, tcl, 0.013, 0.004)
    r, J, ncr = ref.residuals(prob, *X)
    Jn = numeric_jacobian(prob, X)
    scale = np.abs(J).max(0)
    gap = (np.abs(J - Jn).max(0) / scale).max()
    print("%s: analytic vs central differences, worst column gap %.2e" % (name, gap))
    assert gap <= 1e-7
    worst = 0.0
    for i in range(3):
        E = np.empty(121)
        L32 = np.ascontiguousarray(prob["lifted"][i], dtype=np.float32)
        B32 = np.ascontiguousarray(prob["board"][i], dtype=np.float32)
        pts = np.ascontiguousarray(prob["pts"][i])
        pose7 = jref.Rt_to_pose7(Rs[i], ts[i])
        shim.shim_range_eval_image(C.byref(ro), d(L32), d(B32), C.c_longlong(len(L32)), d(pts), C.c_longlong(len(pts)), d(pose7),
                                   d(np.ascontiguousarray(jref.Rt_to_pose7(Rcl, tcl))), d(np.array([X[4], X[5]])), d(E))
        rows = np.concatenate([2 * sum(len(x) for x in prob["lifted"][:i]) + np.arange(2 * len(L32)),
                               ncr + sum(len(x) for x in prob["pts"][:i]) + np.arange(len(pts))]).astype(int)
        Ji, Jc, ri = J[rows][:, 8 + 6 * i:14 + 6 * i], J[rows][:, :8], r[rows]
        iu6, iu8 = np.triu_indices(6), np.triu_indices(8)
        for got, want in ((E[0:21], (Ji.T @ Ji)[iu6]), (E[21:69], (Ji.T @ Jc).reshape(-1)), (E[69:75], Ji.T @ ri),
                          (E[75:111], (Jc.T @ Jc)[iu8]), (E[111:119], Jc.T @ ri),
                          (E[119:120], [0.5 * np.sum(ri[:2 * len(L32)] ** 2)]), (E[120:121], [0.5 * np.sum(ri[2 * len(L32):] ** 2)])):
            want = np.asarray(want)
            if np.abs(want).max() > 0:
                worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
            else:
                assert np.all(got == 0)
    print("%s: shim blocks vs J^T J of the restatement, worst relative gap %.2e" % (name, worst))
    assert worst <= 8e-14


@pytest.fixture(scope="module")
def seeded_runs(shim):
    out = {}
    for name in CAMS:
        cam = cases.CAMERAS[name]
        problems = cases.seeded(name)
        a = cases.arrays(problems)
        q0, t0, st = TJ.start_poses(shim, cam, a)
        assert np.all(st == 1)
        ro = shim_range_options(shim, cam)
        s = shim_range(shim, cam, a, q0, t0, ro=ro)
        out[name] = dict(cam=cam, problems=problems, a=a, q0=q0, t0=t0, ro=ro, s=s,
                         cmp=[compare_problem(shim, cam, a, k, s, q0, t0, ro) for k in range(len(problems))])
    return out


@pytest.mark.parametrize("name", CAMS)
def test_seeded_sets_match_restatement(seeded_runs, name):
    """Minimiser, final cost, cost shares and H_cr against the restatement on the seeded sets (0.3 px, 0.01 m, 6-15 images, an offset
    within +-0.03 m and a scale within +-1 % per problem, start (0, 0)).  Measured here, worst of both cameras: the largest pose gap
    3.27e-9 (radtan 1.4e-9), b and kappa 1.6e-7 of their predicted 1 sigma (sigma_b 1.4-2.8 mm, sigma_kappa 0.22-0.50 % on these
    sets; the recovered b lies within 1 sigma of the planted one on all eight, kappa within 2.4 sigma), the relative gap of the final
    cost 2.99e-15 and of the cost shares 1.05e-15, H_cr against the dense Schur complement at the restatement's minimiser 2.66e-9
    relative and 2.51e-15 at the answer's own point.  Asserted one decade above (the pose, range and cost bounds are shared with the
    tests below and follow their worst)."""
    e = seeded_runs[name]
    worst = dict(pose=0.0, range_sigma=0.0, cost=0.0, parts=0.0, hcr=0.0, hcr_same=0.0)
    for k, c in enumerate(e["cmp"]):
        sm = e["s"]["summaries"][k]
        assert sm.termination in (1, 2, 3), (k, sm.termination)
        assert np.all(e["s"]["status"] == 1)
        assert c["pose"] is not None, k
        Hs = ref.schur(ref.normal_matrix(c["prob"], *c["best"])[0])
        Hs2 = ref.schur(ref.normal_matrix(c["prob"], *c["mine"])[0])
        got = e["s"]["H_cr"][k]
        assert np.array_equal(got, got.T)
        worst["pose"] = max(worst["pose"], c["pose"])
        worst["range_sigma"] = max(worst["range_sigma"], c["range_sigma"])
        worst["cost"] = max(worst["cost"], c["cost"], c["cost_self"])
        worst["parts"] = max(worst["parts"], c["parts"])
        worst["hcr"] = max(worst["hcr"], np.linalg.norm(got - Hs) / np.linalg.norm(Hs))
        worst["hcr_same"] = max(worst["hcr_same"], np.linalg.norm(got - Hs2) / np.linalg.norm(Hs2))
        assert sm.final_cost <= sm.initial_cost and abs(sm.initial_cost - c["start_cost"]) <= 1e-12 * c["start_cost"]
        assert abs(e["s"]["cost_parts"][k].sum() - sm.final_cost) <= 1e-14 * sm.final_cost
        tr = e["problems"][k]["range_true"]
        print("%s problem %d: b %.4f (planted %.4f, sigma %.4f)  kappa %.5f (planted %.5f, sigma %.5f)" % (
            name, k, e["s"]["range"][k][0], tr[0], c["sigma"][6], e["s"]["range"][k][1], tr[1], c["sigma"][7]))
    print("%s: worst gaps %s" % (name, {k: "%.2e" % v for k, v in worst.items()}))
    assert worst["pose"] <= POSE_BOUND and worst["cost"] <= COST_BOUND and worst["parts"] <= COST_BOUND
    assert worst["range_sigma"] <= RANGE_SIGMA_BOUND
    assert worst["hcr"] <= HCR_BOUND and worst["hcr_same"] <= HCR_SAME_POINT


@pytest.mark.parametrize("name", CAMS)
def test_inverse_of_H_cr_is_the_marginal_covariance(seeded_runs, name):
    """inv(H_cr) equals the leading 8x8 block of the inverse of the dense normal matrix (the shared block first) at the answer's own
    point.  Measured: 2.50e-13 relative, asserted one decade above at INV_BOUND."""
    e = seeded_runs[name]
    worst = 0.0
    for k, c in enumerate(e["cmp"]):
        Hd, _ = ref.normal_matrix(c["prob"], *c["mine"])
        want = np.linalg.inv(Hd)[:8, :8]
        got = np.linalg.inv(e["s"]["H_cr"][k])
        worst = max(worst, np.linalg.norm(got - want) / np.linalg.norm(want))
    print("%s: inv(H_cr) vs the dense inverse, worst relative gap %.2e" % (name, worst))
    assert worst <= INV_BOUND


@pytest.mark.parametrize("name", CAMS)
def test_recovery_of_a_planted_offset_and_scale(shim, name):
    """Noise-free corners and points with a planted (0.02 m, 0.5 %): the free solve returns the planted values and the true T_cl to
    the accuracy the restatement reaches on the same data (the float32 rounding of the lifted corners keeps both off the truth:
    measured |b - 0.02| 1.0e-9 m (kb 1.4e-10), |kappa - 0.005| 1.0e-9 (6.5e-9), T_cl 1.4e-7 (4.5e-7), the restatement's errors the same
    to the digits printed, the two minimisers 3e-15 apart).  With both held at 0 the same data ends with a laser cost share larger
    by a factor of 5.1e11 (radtan) / 2.0e11 (kb) — the free solve's is the rounding's — and t_cl displaced by 20.9 mm / 21.0 mm."""
    cam = cases.CAMERAS[name]
    p = cases.problem(name, 55, 8, 144, 100, noise_px=0.0, noise_l=0.0, offset=0.02, scale=0.005)
    a = cases.arrays([p])
    rng = np.random.default_rng(3)
    q0 = np.stack([jref.R_to_quat_wxyz(im[2] @ jref.exp_so3(rng.normal(size=3) * 0.02)) for im in p["images"]])
    t0 = np.stack([im[3] + rng.normal(size=3) * 0.01 for im in p["images"]])
    ro = shim_range_options(shim, cam)
    s = shim_range(shim, cam, a, q0, t0, ro=ro)
    c = compare_problem(shim, cam, a, 0, s, q0, t0, ro)
    sm = s["summaries"][0]
    err_mine = (abs(s["range"][0][0] - 0.02), abs(s["range"][0][1] - 0.005), np.abs(s["poses_cl"][0] - p["pose_cl_true"]).max())
    best_cl = jref.Rt_to_pose7(c["best"][2], c["best"][3])
    err_ref = (abs(c["best"][4] - 0.02), abs(c["best"][5] - 0.005), np.abs(best_cl - p["pose_cl_true"]).max())
    print("%s noise-free, free: errors (b, kappa, T_cl) %.2e %.2e %.2e; the restatement's %.2e %.2e %.2e; pose gap %.2e" % (
        name, *err_mine, *err_ref, c["pose"]))
    assert sm.termination != 6 and sm.final_cost <= sm.initial_cost
    assert c["pose"] is not None and c["pose"] <= POSE_GATE
    assert abs(s["range"][0][0] - c["best"][4]) <= POSE_GATE and abs(s["range"][0][1] - c["best"][5]) <= POSE_GATE
    assert all(m <= r + POSE_GATE for m, r in zip(err_mine, err_ref))
    assert err_mine[0] <= 1e-4 and err_mine[1] <= 1e-4 and err_mine[2] <= 1e-4
    held = shim_range_options(shim, cam, hold_range_mask=3)
    sh = shim_range(shim, cam, a, q0, t0, ro=held)
    factor = sh["cost_parts"][0][1] / s["cost_parts"][0][1]
    moved = np.abs(sh["poses_cl"][0][:3] - p["pose_cl_true"][:3]).max()
    print("%s noise-free, both held at 0: laser cost share x %.3g, t_cl displaced by %.1f mm" % (name, factor, 1e3 * moved))
    assert np.array_equal(sh["range"][0], [0.0, 0.0])
    assert factor > 100.0 and moved > 5e-3


@pytest.mark.parametrize("name", CAMS)
def test_held_at_zero_is_K18(shim, seeded_runs, name):
    """With both range parameters held at (0, 0) the call agrees with the shim's clc_joint_refine on poses, cost and the leading 6x6 of
    H_cr.  Measured: no gap at all (p' = p bit for bit, the blocks of the six moving columns are K18's sums, and the compacted
    reduced system is K18's), so the bound is zero: the same bits."""
    e = seeded_runs[name]
    ro = shim_range_options(shim, e["cam"], hold_range_mask=3)
    s = shim_range(shim, e["cam"], e["a"], e["q0"], e["t0"], ro=ro)
    j = TJ.shim_joint(shim, e["cam"], e["a"], e["q0"], e["t0"])
    gap = max(np.abs(s["q"] - j["q"]).max(), np.abs(s["t"] - j["t"]).max(), np.abs(s["poses_cl"] - j["poses_cl"]).max())
    print("%s: held at (0, 0) vs K18: pose gap %.2e, cost gap %.2e, H gap %.2e" % (
        name, gap, max(abs(s["summaries"][k].final_cost - j["summaries"][k].final_cost) for k in range(len(e["problems"]))),
        np.abs(s["H_cr"][:, :6, :6] - j["H_cl"]).max()))
    assert np.array_equal(s["q"], j["q"]) and np.array_equal(s["t"], j["t"]) and np.array_equal(s["poses_cl"], j["poses_cl"])
    assert np.array_equal(s["cost_parts"], j["cost_parts"]) and np.array_equal(s["H_cr"][:, :6, :6], j["H_cl"])
    assert np.all(s["H_cr"][:, 6:, :] == 0) and np.all(s["H_cr"][:, :, 6:] == 0) and np.all(s["range"] == 0)
    for k in range(len(e["problems"])):
        assert s["summaries"][k].final_cost == j["summaries"][k].final_cost and s["summaries"][k].num_iterations == j["summaries"][k].num_iterations


@pytest.mark.parametrize("name", CAMS)
def test_held_nonzero_is_K18_on_corrected_points(shim, seeded_runs, name):
    """With held non-zero values the call agrees with K18 run on range_correct'ed points.  K18 then reads p' rounded once to a double
    where K21 carries it in registers — the same value: measured no gap at all, the bound is zero."""
    e = seeded_runs[name]
    npb = len(e["problems"])
    r0 = np.tile([0.015, -0.004], (npb, 1))
    ro = shim_range_options(shim, e["cam"], hold_range_mask=3)
    s = shim_range(shim, e["cam"], e["a"], e["q0"], e["t0"], ro=ro, range0=r0)
    a2 = dict(e["a"], pts=np.empty_like(e["a"]["pts"]))
    shim.shim_range_correct(d(r0[0].copy()), d(e["a"]["pts"]), C.c_longlong(len(a2["pts"])), d(a2["pts"]))
    j = TJ.shim_joint(shim, e["cam"], a2, e["q0"], e["t0"])
    print("%s: held at (0.015, -0.004) vs K18 on corrected points: pose gap %.2e, H gap %.2e" % (
        name, max(np.abs(s["q"] - j["q"]).max(), np.abs(s["t"] - j["t"]).max(), np.abs(s["poses_cl"] - j["poses_cl"]).max()),
        np.abs(s["H_cr"][:, :6, :6] - j["H_cl"]).max()))
    assert np.array_equal(s["range"], r0)
    assert np.array_equal(s["q"], j["q"]) and np.array_equal(s["t"], j["t"]) and np.array_equal(s["poses_cl"], j["poses_cl"])
    assert np.array_equal(s["cost_parts"], j["cost_parts"]) and np.array_equal(s["H_cr"][:, :6, :6], j["H_cl"])


def test_held_parameters_keep_their_bits(shim, seeded_runs):
    """A held parameter comes back bit for bit while the other moves, and the result is the restatement's over the remaining columns;
    hold_extrinsic leaves T_cl bit for bit while b and kappa move.  Measured against the restatement: poses 9.2e-9, the free range
    parameters 5.34e-7 sigma, cost 3.3e-15."""
    e = seeded_runs["radtan"]
    npb = len(e["problems"])
    r0 = np.tile([0.0123456789, -0.00456789], (npb, 1))
    for mask in (1, 2):
        ro = shim_range_options(shim, e["cam"], hold_range_mask=mask)
        s = shim_range(shim, e["cam"], e["a"], e["q0"], e["t0"], ro=ro, range0=r0)
        held, free = mask - 1, 2 - mask
        assert np.array_equal(s["range"][:, held], r0[:, held]) and np.all(s["range"][:, free] != r0[:, free])
        assert np.all(s["H_cr"][:, 6 + held, :] == 0) and np.all(s["H_cr"][:, :, 6 + held] == 0)
        for k in range(npb):
            c = compare_problem(shim, e["cam"], e["a"], k, s, e["q0"], e["t0"], ro, range0=r0)
            print("mask %d problem %d: pose %.2e range %.2e sigma cost %.2e" % (mask, k, c["pose"], c["range_sigma"], c["cost"]))
            assert c["pose"] is not None and c["pose"] <= POSE_BOUND and c["cost"] <= COST_BOUND and c["range_sigma"] <= RANGE_SIGMA_BOUND, (
                mask, k, c["pose"], c["cost"], c["range_sigma"])
    ro = shim_range_options(shim, e["cam"], hold_extrinsic=1)
    s = shim_range(shim, e["cam"], e["a"], e["q0"], e["t0"], ro=ro)
    assert np.array_equal(s["poses_cl"], e["a"]["poses_cl0"]) and np.all(s["range"] != 0) and not np.array_equal(s["q"], e["q0"])
    assert np.all(s["H_cr"][:, :6, :] == 0) and np.all(s["H_cr"][:, :, :6] == 0) and np.all(s["H_cr"][:, 6, 6] > 0)
    for k in range(npb):
        c = compare_problem(shim, e["cam"], e["a"], k, s, e["q0"], e["t0"], ro)
        print("held extrinsic problem %d: pose %.2e range %.2e sigma cost %.2e" % (k, c["pose"], c["range_sigma"], c["cost"]))
        assert c["pose"] is not None and c["pose"] <= POSE_BOUND and c["cost"] <= COST_BOUND and c["range_sigma"] <= RANGE_SIGMA_BOUND, (k, c["pose"], c["cost"])


@pytest.mark.parametrize("name", CAMS)
def test_route_without_corners(shim, seeded_runs, name):
    """hold_board_poses with NULL corner arrays and no camera: T_cl and the range parameters from the tag poses and the points alone,
    against the restatement over those 8 columns (measured: poses 1.1e-9, b and kappa 3.9e-7 sigma, cost 7.9e-15 relative); no board pose
    moves, the corner share is 0, H_cr is C.  The same bits as the call with the corner arrays given."""
    e = seeded_runs[name]
    ro = shim_range_options(shim, None, hold_board_poses=1)
    s = shim_range(shim, None, e["a"], e["q0"], e["t0"], ro=ro, corners=False)
    assert np.array_equal(s["q"], e["q0"]) and np.array_equal(s["t"], e["t0"]) and np.all(s["status"] == 1)
    s2 = shim_range(shim, e["cam"], e["a"], e["q0"], e["t0"], ro=shim_range_options(shim, e["cam"], hold_board_poses=1))
    for key in ("poses_cl", "range", "H_cr", "cost_parts"):
        assert np.array_equal(s[key], s2[key]), key
    worst = dict(pose=0.0, range_sigma=0.0, cost=0.0)
    for k in range(len(e["problems"])):
        c = compare_problem(shim, None, e["a"], k, s, e["q0"], e["t0"], ro)
        assert c["pose"] is not None
        for key in worst:
            worst[key] = max(worst[key], c[key])
        assert s["cost_parts"][k][0] == 0.0
        Hd, _ = ref.normal_matrix(c["prob"], *c["mine"])
        assert np.linalg.norm(s["H_cr"][k] - Hd[:8, :8]) <= 1e-12 * np.linalg.norm(Hd[:8, :8])
    print("%s: no corners vs the restatement: %s" % (name, {k: "%.2e" % v for k, v in worst.items()}))
    assert worst["pose"] <= POSE_BOUND and worst["range_sigma"] <= RANGE_SIGMA_BOUND and worst["cost"] <= COST_BOUND


def test_status_and_untouched_outputs(shim):
    """The image with a zero-range point gets CLC_JOINT_NONFINITE, keeps its pose, and the others solve as if it were not there; the
    problem without a laser point returns T_cl and range bit for bit; a non-finite start range ends CLC_FAILURE with everything
    untouched."""
    name = "radtan"
    cam = cases.CAMERAS[name]
    problems, notes = cases.edge_problems(name)
    pz, pn = problems[notes["zerorange"]], problems[notes["nolaser"]]
    a = cases.arrays([pz, pn])
    q0, t0, st = TJ.start_poses(shim, cam, a)
    r0 = np.array([[0.0, 0.0], [0.004, -0.002]])
    s = shim_range(shim, cam, a, q0, t0, range0=r0)
    assert list(s["status"]) == [1, 1, -2, 1, 1, 1, 1, 1, 1]
    assert np.array_equal(s["q"][2], q0[2]) and np.array_equal(s["t"][2], t0[2])
    assert s["summaries"][0].termination in (1, 2, 3) and s["summaries"][1].termination in (1, 2, 3)
    assert np.array_equal(s["poses_cl"][1], a["poses_cl0"][1]) and np.array_equal(s["range"][1], r0[1]) and s["cost_parts"][1][1] == 0.0
    good = [0, 1, 3, 4]
    ag = cases.arrays([dict(pz, images=[pz["images"][i] for i in good])])
    sg = shim_range(shim, cam, ag, q0[good], t0[good])
    for key in ("poses_cl", "range", "H_cr"):
        assert np.array_equal(sg[key][0], s[key][0]), key
    assert np.array_equal(sg["q"], s["q"][good]) and np.array_equal(sg["t"], s["t"][good])
    bad = shim_range(shim, cam, a, q0, t0, range0=np.array([[np.nan, 0.0], [0.0, np.inf]]))
    assert [bad["summaries"][k].termination for k in range(2)] == [6, 6]
    assert np.array_equal(bad["q"], q0) and np.array_equal(bad["t"], t0) and np.array_equal(bad["poses_cl"], a["poses_cl0"])
    assert np.isnan(bad["range"][0][0]) and bad["range"][0][1] == 0.0 and np.all(np.isnan(bad["H_cr"]))


def test_single_range_problem(shim):
    """Every point at |p| = 2 m: b and kappa enter only as kappa + b / 2.  Both free: the solve ends finite with a CONVERGENCE or
    NO_CONVERGENCE code, and the smallest singular value of H_cr is below 1e-9 of the largest on the Jacobi-scaled matrix
    (test_joint_host.well_posed's threshold; measured 8.6e-17).  With the scale held the problem is well posed by the same test and
    the result matches the restatement (measured: poses 2.64e-8, b 4.5e-7 sigma, cost 5.6e-16)."""
    name = "radtan"
    cam = cases.CAMERAS[name]
    problems, notes = cases.edge_problems(name)
    a = cases.arrays([problems[notes["singlerange"]]])
    assert np.abs(np.linalg.norm(a["pts"], axis=1) - cases.SINGLE_RANGE).max() < 1e-14
    q0, t0, st = TJ.start_poses(shim, cam, a)
    s = shim_range(shim, cam, a, q0, t0)
    sm = s["summaries"][0]
    assert sm.termination in (1, 2, 3, 4, 5), sm.termination
    for key in ("q", "t", "poses_cl", "range", "H_cr"):
        assert np.all(np.isfinite(s[key])), key
    Hcr = s["H_cr"][0]
    sc = np.sqrt(np.diag(Hcr))
    sv = np.linalg.svd(Hcr / np.outer(sc, sc), compute_uv=False)
    print("single range, both free: termination %d, b %.4f kappa %.5f, scaled H_cr sv min / max %.2e" % (sm.termination, *s["range"][0], sv[-1] / sv[0]))
    assert sv[-1] < 1e-9 * sv[0]
    ro = shim_range_options(shim, cam, hold_range_mask=2)
    s2 = shim_range(shim, cam, a, q0, t0, ro=ro)
    c = compare_problem(shim, cam, a, 0, s2, q0, t0, ro)
    print("single range, scale held: pose gap %s, range gap %s sigma, cost gap %.2e" % (c["pose"], c["range_sigma"], c["cost"]))
    assert s2["summaries"][0].termination in (1, 2, 3)
    assert c["pose"] is not None and c["pose"] <= POSE_BOUND and c["range_sigma"] <= RANGE_SIGMA_BOUND and c["cost"] <= COST_BOUND
    assert s2["range"][0][1] == 0.0


def range_call(L, ro, h=None, cam=True, device=False, **kw):
    c = H.CAMERAS["pinhole"].to_c()
    z = np.zeros(2, dtype=np.int64)
    args = dict(coff=d(z), poff=d(z), q=d(np.zeros(4)), t=d(np.zeros(3)), cl=d(np.zeros(7)), rg=d(np.zeros(2)), sm=(_capi.Summary * 1)(),
                st=d(np.zeros(1, np.int32)), prob=None, n_images=1, n_problems=1)
    args.update(kw)
    f = L.clc_joint_refine_range_device if device else L.clc_joint_refine_range
    return f(h, C.byref(c) if cam else None, None, C.byref(ro) if ro is not None else None, None, None, args["coff"], None,
             args["poff"], None, C.c_size_t(args["n_images"]), args["prob"], C.c_size_t(args["n_problems"]), args["q"],
             args["t"], args["cl"], args["rg"], args["sm"], None, None, args["st"])


def test_refusals_need_no_device():
    """NULL required pointers, a sigma that is not finite and positive (sigma_corner not looked at with hold_board_poses), both hold
    flags, a mask outside 0..3, reserved != 0, offsets that decrease, corner arrays NULL without hold_board_poses:
    CLC_ERR_INVALID_ARG before any device work (the handle is NULL throughout)."""
    L = _capi.lib()
    base = _capi.default_range_options(H.CAMERAS["pinhole"])
    assert base.sigma_laser == 0.01 and base.sigma_corner > 0
    assert (base.hold_board_poses, base.hold_extrinsic, base.hold_range_mask, base.reserved) == (0, 0, 0, 0)
    none = _capi.default_range_options(None)
    assert none.sigma_corner == 0.0 and none.sigma_laser == 0.01
    nan, inf = float("nan"), float("inf")
    for device in (False, True):
        who = "clc_joint_refine_range_device: " if device else "clc_joint_refine_range: "
        rows = [(dict(sigma_corner=v), "sigma_corner must be finite and > 0") for v in (nan, inf, 0.0, -1e-3)]
        rows += [(dict(sigma_laser=v), "sigma_laser must be finite and > 0") for v in (nan, inf, 0.0, -0.01)]
        rows += [(dict(hold_board_poses=1, sigma_laser=nan), "sigma_laser must be finite and > 0")]
        rows += [(dict(hold_board_poses=1, hold_extrinsic=1), "both hold flags set")]
        rows += [(dict(hold_range_mask=v), "hold_range_mask outside 0..3") for v in (-1, 4, 7)]
        rows += [(dict(reserved=1), "reserved must be 0")]
        for kw, msg in rows:
            ro = _capi.RangeOptions(base.sigma_corner, base.sigma_laser, 0, 0, 0, 0)
            for k, v in kw.items():
                setattr(ro, k, v)
            assert range_call(L, ro, device=device) == -1
            assert L.clc_last_error().decode() == who + msg
        assert range_call(L, none, device=device) == -1 and L.clc_last_error().decode() == who + "sigma_corner must be finite and > 0"
        if not device:
            bad = np.array([3, 1], dtype=np.int64)
            for kw in (dict(coff=d(bad)), dict(poff=d(bad)), dict(prob=d(bad))):
                assert range_call(L, base, **kw) == -1
                assert L.clc_last_error().decode() == who + "offsets not monotone"
        for key in ("coff", "poff", "q", "t", "cl", "rg", "sm", "st"):
            assert range_call(L, base, device=device, **{key: None}) == -1
            assert L.clc_last_error().decode() == who + "bad argument", key
        # good arguments: the call gets as far as the missing handle
        assert range_call(L, base, device=device) == -1 and L.clc_last_error().decode() == who + "bad argument"
        assert range_call(L, None, device=device) == -1 and L.clc_last_error().decode() == who + "bad argument"
        assert range_call(L, base, cam=False, device=device) == -1 and L.clc_last_error().decode() == who + "unknown camera model"
        # with the board poses held: no camera, no corner arrays, sigma_corner not looked at -> as far as the missing handle
        held = _capi.RangeOptions(nan, 0.01, 1, 0, 0, 0)
        assert range_call(L, held, cam=False, device=device, coff=None) == -1 and L.clc_last_error().decode() == who + "bad argument"
        assert range_call(L, held, cam=False, device=device, coff=None, poff=None) == -1
    rg, p, o = d(np.zeros(2)), d(np.ones(3)), d(np.zeros(3))
    for f, who in ((L.clc_range_correct, "clc_range_correct: "), (L.clc_range_correct_device, "clc_range_correct_device: ")):
        for args in ((None, rg, p, 1, o), (None, None, p, 1, o), (None, rg, None, 1, o), (None, rg, p, 1, None)):
            assert f(args[0], args[1], args[2], C.c_size_t(args[3]), args[4]) == -1
            assert L.clc_last_error().decode() == who + "bad argument"


def test_range_correct_matches_the_formula(shim):
    """p' = (1 + kappa + b / |p|) p against numpy to 2 ulp of every component (measured: 0 ulp); NaN for a zero or non-finite point;
    (0, 0) returns the points bit for bit; simdata.apply_range_error is its inverse (to 4 ulp of the range)."""
    from camlasercalibratool_amd import simdata
    rng = np.random.default_rng(11)
    pts = rng.normal(size=(1000, 3)) * rng.uniform(0.05, 30.0, size=(1000, 1))
    pts[7] = 0.0
    pts[9, 1] = np.nan
    pts[11, 2] = np.inf
    out = np.empty_like(pts)
    rg = np.array([0.0234, -0.0071])
    shim.shim_range_correct(d(rg), d(pts), C.c_longlong(len(pts)), d(out))
    want = ref.correct(pts, *rg)
    bad = [7, 9, 11]
    assert np.all(np.isnan(out[bad])) and np.all(np.isnan(want[bad]))
    ok = np.setdiff1d(np.arange(len(pts)), bad)
    ulp = np.abs(out[ok] - want[ok]) / np.spacing(np.abs(want[ok]))
    print("range_correct vs numpy: worst %.1f ulp" % ulp.max())
    assert ulp.max() <= 2.0
    same = np.empty_like(pts)
    shim.shim_range_correct(d(np.zeros(2)), d(pts), C.c_longlong(len(pts)), d(same))
    assert np.array_equal(same[ok], pts[ok])
    meas = simdata.apply_range_error(pts[ok], *rg)
    back = np.empty_like(meas)
    shim.shim_range_correct(d(rg), d(meas), C.c_longlong(len(meas)), d(back))
    assert np.abs(np.linalg.norm(back, axis=1) - np.linalg.norm(pts[ok], axis=1)).max() <= 4 * np.spacing(30.0 * 3)


def test_sanitized_standalone_program(tmp_path):
    """tests/shim/laserrange_sanitize_main.cpp: the per-problem host function on the edge shapes, every array of its exact size, built
    with -fsanitize=address,undefined and run as an ordinary process."""
    exe = str(tmp_path / "laserrange_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "shim", "laserrange_sanitize_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "shapes ok" in p.stdout, p.stdout
