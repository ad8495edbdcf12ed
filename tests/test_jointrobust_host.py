"""K22 (csrc/clc_jointrobust.hpp on clc_arrow.hpp) on the host: the robust evaluation blocks, the solve and the weights compiled with g++
(tests/shim/jointrobust_shim.cpp) against the numpy / scipy restatement tests/jointrobust_ref.py on clean and contaminated seeded sets
(tests/jointrobust_cases.py): the weighted blocks, the gradient against central differences through Plus, the minimiser, cost, cost
shares, H_cl and weights; both scales 0 against K18's shim bit for bit; one scale 0; the held-board-poses route against the
oracle's Cauchy cost; recovery of T_cl under planted outliers; the refusals of the C ABI (they need no device); a stand-alone
AddressSanitizer / UBSan program over the edge shapes."""
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
import joint_cases as jcases  # noqa: E402
import joint_ref as ref  # noqa: E402
import jointrobust_cases as cases  # noqa: E402
import jointrobust_ref as rref  # noqa: E402
import test_campose_host as H  # noqa: E402
import test_joint_host as TJ  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402

CAMS = ["radtan", "kb"]
d = H._d

# The project's parity gates: 1e-6 on poses, 1e-8 relative on cost.  The bounds below are one decade over the worst gaps measured on
# the seeded sets, clean and contaminated, both cameras (the figures: test_seeded_sets_match_restatement's docstring), never above
# the gates.
POSE_GATE, COST_GATE = 1e-6, 1e-8
POSE_BOUND = 4.7e-7        # largest gap of any R entry or t component (T_cl and every T_ca) to the restatement's minimiser (4.68e-8)
COST_BOUND = 4e-14         # relative gap of the final cost and of the two cost shares (3.76e-15)
HCL_BOUND = 6e-7           # relative (Frobenius) gap of H_cl to the weighted dense Schur complement at the restatement's minimiser (5.84e-8)
HCL_SAME_POINT = 5.1e-14   # the same at the answer's own poses (5.08e-15)
WEIGHT_BOUND = 1.5e-6      # largest gap of a weight to the restatement's at its minimiser (1.41e-7)
WEIGHT_SAME_POINT = 3.1e-13  # ... and at the answer's own poses (3.09e-14: a corner's e is a difference of lifted coordinates over sigma ~ 7e-4)
BLOCK_BOUND = 8e-14        # the per-image blocks against the weighted J^T J, J^T r (7.81e-15)
assert POSE_BOUND <= POSE_GATE and COST_BOUND <= COST_GATE


def build_shim(path):
    subprocess.check_call(TJ.GXX + ["-shared", os.path.join(HERE, "shim", "jointrobust_shim.cpp"), "-o", path])
    L = C.CDLL(path)
    L.shim_kb_theta.restype = C.c_double
    L.shim_kb_theta.argtypes = [C.c_void_p, C.c_double]
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(str(tmp_path_factory.mktemp("jr") / "libjointrobust_shim.so"))


def loss_options(L, jo, **kw):
    lo = _capi.JointLossOptions()
    L.shim_joint_loss_options_default(C.byref(lo), C.byref(jo))
    for k, v in kw.items():
        setattr(lo, k, v)
    return lo


def shim_robust(L, cam, a, q0, t0, keep=None, jo=None, lo=None, poses_cl=None, max_iterations=None, weights=True):
    """shim_joint_refine_robust on the arrays of joint_cases.arrays -> dict, the keys of Solver.joint_refine_robust."""
    n, npb = len(a["coff"]) - 1, len(a["prob_off"]) - 1
    q, t = np.array(q0, dtype=np.float64, order="C"), np.array(t0, dtype=np.float64, order="C")
    pcl = np.array(a["poses_cl0"] if poses_cl is None else poses_cl, dtype=np.float64, order="C").reshape(npb, 7)
    sm = (_capi.Summary * max(npb, 1))()
    Hcl = np.empty((npb, 6, 6)); parts = np.empty((npb, 2)); st = np.full(n, -99, dtype=np.int32)
    wc, wl = np.full(len(a["corners"]), -7.0), np.full(len(a["pts"]), -7.0)
    k = None if keep is None else np.ascontiguousarray(np.asarray(keep).astype(np.uint8))
    o = _capi.Options()
    L.shim_pose_options_default(C.byref(o))
    if max_iterations is not None:
        o.max_num_iterations = max_iterations
    jo = jo or TJ.shim_joint_options(L, cam)
    lo = lo or loss_options(L, jo)
    c = cam.to_c()
    L.shim_joint_refine_robust(C.byref(c), C.byref(o), C.byref(jo), C.byref(lo), d(a["corners"]), d(a["board"]), d(a["coff"]), d(a["pts"]),
                               d(a["poff"]), None if k is None else d(k), C.c_longlong(n), d(a["prob_off"]), C.c_longlong(npb), d(q), d(t),
                               d(pcl), sm, d(Hcl), d(parts), d(st), d(wc) if weights else None, d(wl) if weights else None)
    return dict(q=q, t=t, poses_cl=pcl, summaries=sm, H_cl=Hcl, cost_parts=parts, status=st, w_corner=wc, w_laser=wl)


def restatement_problem(L, cam, a, k, jo, lo, keep=None):
    prob, idx = TJ.restatement_problem(L, cam, a, k, jo, keep)
    prob["lc"], prob["ll"] = lo.loss_corner, lo.loss_laser
    return prob, idx


def weights_of(a, s, idx):
    """The call's weights of the images idx, in the restatement's order."""
    wc = np.concatenate([s["w_corner"][a["coff"][i]:a["coff"][i + 1]] for i in idx]) if idx else np.zeros(0)
    wl = np.concatenate([s["w_laser"][a["poff"][i]:a["poff"][i + 1]] for i in idx]) if idx else np.zeros(0)
    return wc, wl


def compare_problem(L, cam, a, k, s, q0, t0, jo, lo, keep=None):
    """One problem of a call against the restatement: its minimiser from the same start and from the call's own answer (the lower of
    the two) -> dict of gaps."""
    prob, idx = restatement_problem(L, cam, a, k, jo, lo, keep)
    start = ([ref.quat_wxyz_to_R(q0[i]) for i in idx], [t0[i].copy() for i in idx], *ref.pose7_to_Rt(a["poses_cl0"][k]))
    mine = TJ.poses_of(s, idx, k)
    hb, he = bool(jo.hold_board_poses), bool(jo.hold_extrinsic)
    cand = [rref.solve(prob, *mine, hold_board=hb, hold_ext=he), rref.solve(prob, *start, hold_board=hb, hold_ext=he)]
    best = min(cand, key=lambda c: c[4])
    cost = s["summaries"][k].final_cost
    cc, cl = rref.cost_parts(prob, *mine)
    wc, wl = weights_of(a, s, idx)
    wc_same, wl_same = rref.weights(prob, *mine)
    wc_best, wl_best = rref.weights(prob, *best[:4])
    Hs = rref.schur(rref.normal_matrix(prob, *best[:4])[0])
    Hs2 = rref.schur(rref.normal_matrix(prob, *mine)[0])
    got = s["H_cl"][k]
    nz = lambda M: np.linalg.norm(M) or 1.0  # (H_cl is zero without laser points)
    return dict(cost=abs(cost - best[4]) / best[4], cost_self=abs(cost - (cc + cl)) / (cc + cl),
                parts=max(abs(s["cost_parts"][k][0] - cc), abs(s["cost_parts"][k][1] - cl)) / (cc + cl),
                pose=TJ.pose_gap(mine, best[:4]), hcl=np.linalg.norm(got - Hs) / nz(Hs),
                hcl_same=np.linalg.norm(got - Hs2) / nz(Hs2),
                w=max(np.abs(wc - wc_best).max(initial=0.0), np.abs(wl - wl_best).max(initial=0.0)),
                w_same=max(np.abs(wc - wc_same).max(initial=0.0), np.abs(wl - wl_same).max(initial=0.0)),
                ref_cost=best[4], prob=prob, idx=idx, best=best[:4], mine=mine)


def test_struct_layout_and_defaults(shim):
    assert shim.shim_joint_loss_options_size() == 16 == C.sizeof(_capi.JointLossOptions)
    assert (_capi.JointLossOptions.loss_corner.offset, _capi.JointLossOptions.loss_laser.offset) == (0, 8)
    assert shim.shim_robust_image_doubles() == shim.shim_joint_image_doubles()
    L = _capi.lib()
    for fn in (shim.shim_joint_loss_options_default, L.clc_joint_loss_options_default):
        lo = _capi.JointLossOptions(-1.0, -1.0)
        fn(C.byref(lo), None)
        assert (lo.loss_corner, lo.loss_laser) == (3.0, 5.0)
        jo = _capi.JointOptions(1e-3, 0.01, 0, 0)
        fn(C.byref(lo), C.byref(jo))
        assert (lo.loss_corner, lo.loss_laser) == (3.0, 0.05 / 0.01)
        jo.sigma_laser = 0.02
        fn(C.byref(lo), C.byref(jo))
        assert (lo.loss_corner, lo.loss_laser) == (3.0, 0.05 / 0.02)
    lo = _capi.default_joint_loss_options(_capi.JointOptions(1e-3, 0.025, 0, 0))
    assert (lo.loss_corner, lo.loss_laser) == (3.0, 0.05 / 0.025)
    assert _capi.default_joint_loss_options().loss_laser == 5.0
    for name in ("clc_joint_loss_options_default", "clc_joint_refine_robust", "clc_joint_refine_robust_device"):
        assert name in _capi.EXPORTED and hasattr(L, name)


def robust_call(L, jo, lo, h=None, cam=True, **kw):
    c = H.CAMERAS["pinhole"].to_c()
    z = np.zeros(2, dtype=np.int64)
    args = dict(coff=d(z), poff=d(z), q=d(np.zeros(4)), t=d(np.zeros(3)), cl=d(np.zeros(7)), sm=(_capi.Summary * 1)(), st=d(np.zeros(1, np.int32)),
                prob=None, n_images=1, n_problems=1)
    args.update(kw)
    return L.clc_joint_refine_robust(h, C.byref(c) if cam else None, None, C.byref(jo) if jo is not None else None,
                                     C.byref(lo) if lo is not None else None, None, None, args["coff"], None, args["poff"], None,
                                     C.c_size_t(args["n_images"]), args["prob"], C.c_size_t(args["n_problems"]), args["q"], args["t"],
                                     args["cl"], args["sm"], None, None, args["st"], None, None)


def test_refusals_need_no_device():
    """A loss scale that is negative or not finite, and everything clc_joint_refine refuses with its messages behind the new name:
    CLC_ERR_INVALID_ARG before any device work (the handle is NULL throughout)."""
    L = _capi.lib()
    base = _capi.default_joint_options(H.CAMERAS["pinhole"])
    who = "clc_joint_refine_robust: "
    nan, inf = float("nan"), float("inf")
    for field in ("loss_corner", "loss_laser"):
        for v in (nan, inf, -inf, -1e-3):
            lo = _capi.JointLossOptions(3.0, 5.0)
            setattr(lo, field, v)
            assert robust_call(L, base, lo) == -1
            assert L.clc_last_error().decode() == who + field + " must be finite and >= 0"
    rows = [(dict(sigma_corner=v), "sigma_corner must be finite and > 0") for v in (nan, inf, 0.0, -1e-3)]
    rows += [(dict(sigma_laser=v), "sigma_laser must be finite and > 0") for v in (nan, inf, 0.0, -0.01)]
    rows += [(dict(hold_board_poses=1, hold_extrinsic=1), "both hold flags set")]
    for kw, msg in rows:
        jo = _capi.JointOptions(base.sigma_corner, base.sigma_laser, 0, 0)
        for k, v in kw.items():
            setattr(jo, k, v)
        assert robust_call(L, jo, None) == -1
        assert L.clc_last_error().decode() == who + msg
    bad = np.array([3, 1], dtype=np.int64)
    for kw in (dict(coff=d(bad)), dict(poff=d(bad)), dict(prob=d(bad))):
        assert robust_call(L, base, None, **kw) == -1
        assert L.clc_last_error().decode() == who + "offsets not monotone"
    for key in ("coff", "poff", "q", "t", "cl", "sm", "st"):
        assert robust_call(L, base, None, **{key: None}) == -1
        assert L.clc_last_error().decode() == who + "bad argument"
    # good arguments, zero scales included: the call gets as far as the missing handle
    for lo in (None, _capi.JointLossOptions(0.0, 0.0), _capi.JointLossOptions(0.0, 5.0)):
        assert robust_call(L, base, lo) == -1 and L.clc_last_error().decode() == who + "bad argument"
    assert robust_call(L, None, None) == -1 and L.clc_last_error().decode() == who + "bad argument"
    assert robust_call(L, base, None, cam=False) == -1 and L.clc_last_error().decode() == who + "unknown camera model"
    c = H.CAMERAS["pinhole"].to_c()
    z = np.zeros(2, dtype=np.int64)
    r = L.clc_joint_refine_robust_device(None, C.byref(c), None, C.byref(base), C.byref(_capi.JointLossOptions(-1.0, 5.0)), None, None, d(z),
                                         None, d(z), None, C.c_size_t(1), None, C.c_size_t(1), d(np.zeros(4)), d(np.zeros(3)),
                                         d(np.zeros(7)), (_capi.Summary * 1)(), None, None, d(np.zeros(1, np.int32)), None, None)
    assert r == -1 and L.clc_last_error().decode() == "clc_joint_refine_robust_device: loss_corner must be finite and >= 0"


def eval_point(name, seed=5):
    """A small contaminated problem away from its minimiser -> cam, a, prob pieces."""
    cam = jcases.CAMERAS[name]
    p = cases.contaminate(jcases.problem(name, seed, 3, [144, 65, 20], [100, 65, 0]), np.random.default_rng(seed))
    a = jcases.arrays([p])
    rng = np.random.default_rng(1)
    Rs = [im[2] @ ref.exp_so3(rng.normal(size=3) * 0.01) for im in p["images"]]
    ts = [im[3] + rng.normal(size=3) * 0.005 for im in p["images"]]
    Rcl, tcl = ref.pose7_to_Rt(p["pose_cl0"])
    return cam, p, a, (Rs, ts, Rcl, tcl)


@pytest.mark.parametrize("name", CAMS)
@pytest.mark.parametrize("scales", [(3.0, 5.0), (0.0, 5.0), (3.0, 0.0), (0.5, 0.7)])
def test_blocks_match_weighted_normal_equations(shim, name, scales):
    """The shim's per-image blocks A, B, g, C, g_c are the restatement's J^T W J and J^T W r, and the two cost parts its 1/2 sum rho,
    at a point away from the minimiser of a contaminated problem (weights from ~0.01 to 1; scales (0.5, 0.7) put most observations
    on the loss's tail).  Measured: 7.81e-15 relative to the largest entry of a block, asserted one decade above at BLOCK_BOUND."""
    cam, p, a, X = eval_point(name)
    jo = TJ.shim_joint_options(shim, cam)
    lo = loss_options(shim, jo, loss_corner=scales[0], loss_laser=scales[1])
    prob, idx = restatement_problem(shim, cam, a, 0, jo, lo)
    Rs, ts, Rcl, tcl = X
    r, J, ncr = ref.residuals(prob, *X)
    w = rref.row_weights(prob, *X)
    assert w.min() < 0.2 and w.max() > 0.9 or scales == (0.5, 0.7)
    zc, zl, _, _ = rref.block_z(prob, *X)
    worst = 0.0
    nc0, np0 = 0, 0
    for i in range(3):
        E = np.empty(92)
        L32 = np.ascontiguousarray(prob["lifted"][i], dtype=np.float32)
        B32 = np.ascontiguousarray(prob["board"][i], dtype=np.float32)
        pts = np.ascontiguousarray(prob["pts"][i])
        pose7 = ref.Rt_to_pose7(Rs[i], ts[i])
        shim.shim_robust_eval_image(C.byref(jo), C.byref(lo), d(L32), d(B32), C.c_longlong(len(L32)), d(pts), C.c_longlong(len(pts)), d(pose7),
                                    d(np.ascontiguousarray(ref.Rt_to_pose7(Rcl, tcl))), d(E))
        rows = np.concatenate([2 * nc0 + np.arange(2 * len(L32)), ncr + np0 + np.arange(len(pts))]).astype(int)
        Ji, Jc, ri, wi = J[rows][:, 6 + 6 * i:12 + 6 * i], J[rows][:, :6], r[rows], w[rows]
        iu = np.triu_indices(6)
        cc = 0.5 * np.sum(rref.rho(zc[nc0:nc0 + len(L32)], lo.loss_corner))
        cl = 0.5 * np.sum(rref.rho(zl[np0:np0 + len(pts)], lo.loss_laser))
        for got, want in ((E[0:21], (Ji.T @ (Ji * wi[:, None]))[iu]), (E[21:57], (Ji.T @ (Jc * wi[:, None])).reshape(-1)),
                          (E[57:63], Ji.T @ (wi * ri)), (E[63:84], (Jc.T @ (Jc * wi[:, None]))[iu]), (E[84:90], Jc.T @ (wi * ri)),
                          (E[90:91], [cc]), (E[91:92], [cl])):
            want = np.asarray(want)
            if np.abs(want).max() > 0:
                worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
            else:
                assert np.all(got == 0)
        nc0 += len(L32)
        np0 += len(pts)
    print("%s %s: shim blocks vs weighted J^T J of the restatement, worst relative gap %.2e" % (name, scales, worst))
    assert worst <= BLOCK_BOUND


@pytest.mark.parametrize("name", CAMS)
def test_gradient_matches_central_differences(shim, name):
    """The gradient of the robust cost — the shim's g_i per image and the sum of its g_c — against central differences of the
    restatement's cost through a five-point difference stencil along the project's Plus, h = 1e-5 (truncation O(h^4): the three-point
    stencil at 1e-6 leaves 6e-8, its own error, the corner residuals' curvature over sigma ~ 7e-4).  The bound is the differences' own
    error, not the code's: a value f is known to eps |f|, the stencil divides 1.5 of it by h, relative to the largest gradient entry,
    times ten, plus 1e-9 for what is left of the truncation.  The restatement's smooth equivalent residuals: 1/2 |r~|^2 is the cost
    (measured 2.5e-16 relative, asserted 1e-14) and their analytic Jacobian matches the same stencil, each column relative to its
    largest entry, bounded the same way from the largest residual and the smallest column scale."""
    cam, p, a, X = eval_point(name)
    jo = TJ.shim_joint_options(shim, cam)
    lo = loss_options(shim, jo)
    prob, idx = restatement_problem(shim, cam, a, 0, jo, lo)
    Rs, ts, Rcl, tcl = X
    g = np.zeros(6 + 18)
    for i in range(3):
        E = np.empty(92)
        L32 = np.ascontiguousarray(prob["lifted"][i], dtype=np.float32)
        B32 = np.ascontiguousarray(prob["board"][i], dtype=np.float32)
        pts = np.ascontiguousarray(prob["pts"][i])
        shim.shim_robust_eval_image(C.byref(jo), C.byref(lo), d(L32), d(B32), C.c_longlong(len(L32)), d(pts), C.c_longlong(len(pts)),
                                    d(ref.Rt_to_pose7(Rs[i], ts[i])), d(np.ascontiguousarray(ref.Rt_to_pose7(Rcl, tcl))), d(E))
        g[6 + 6 * i:12 + 6 * i] = E[57:63]
        g[:6] += E[84:90]

    def moved(c, step):
        dl = np.zeros(6)
        dl[c % 6] = step
        RR, tt, Rc, tc = list(Rs), list(ts), Rcl, tcl
        if c < 6:
            Rc, tc = ref.plus(Rcl, tcl, dl)
        else:
            i = c // 6 - 1
            RR[i], tt[i] = ref.plus(Rs[i], ts[i], dl)
        return RR, tt, Rc, tc

    h = 1e-5

    def five_point(f):
        """(-f(2h) + 8 f(h) - 8 f(-h) + f(-2h)) / 12h per column: truncation O(h^4)."""
        return np.stack([(-f(*moved(c, 2 * h)) + 8 * f(*moved(c, h)) - 8 * f(*moved(c, -h)) + f(*moved(c, -2 * h))) / (12 * h) for c in range(24)], -1)

    gn = five_point(lambda *Y: sum(rref.cost_parts(prob, *Y)))
    gap = np.abs(g - gn).max() / np.abs(gn).max()
    rs = rref.smooth_residuals(prob, *X)
    cost = sum(rref.cost_parts(prob, *X))
    Jn = five_point(lambda *Y: rref.smooth_residuals(prob, *Y))
    Js = rref.smooth_jacobian(prob, *X)
    jgap = (np.abs(Js - Jn).max(0) / np.abs(Js).max(0)).max()
    tol = 10 * 1.5 * np.finfo(float).eps * cost / (h * np.abs(gn).max()) + 1e-9
    jtol = 10 * 1.5 * np.finfo(float).eps * np.abs(rs).max() / (h * np.abs(Js).max(0).min()) + 1e-9
    print("%s: gradient vs differences %.2e (bound %.2e); smooth residuals: cost %.2e, Jacobian %.2e (bound %.2e)" % (
        name, gap, tol, abs(0.5 * rs @ rs - cost) / cost, jgap, jtol))
    assert gap <= tol and jgap <= jtol
    assert abs(0.5 * rs @ rs - cost) <= 1e-14 * cost
    # and the Gauss-Newton gradient is the smooth residuals' own: J~^T r~ = J^T W r
    assert np.abs(Js.T @ rs - rref.normal_matrix(prob, *X)[1]).max() <= 1e-11 * np.abs(gn).max()


SEEDED = [(101, 6, 144, 100), (103, 12, 64, 40)]  # (seed, images, corners, points): two of joint_cases' shapes, clean and contaminated


def seeded_problems(name):
    out = []
    for seed, *shape in SEEDED:
        clean = jcases.problem(name, seed + (0 if name == "radtan" else 1000), *shape)
        out += [clean, cases.contaminate(clean, np.random.default_rng(seed))]
    return out


@pytest.fixture(scope="module")
def seeded_runs(shim):
    out = {}
    for name in CAMS:
        cam = jcases.CAMERAS[name]
        problems = seeded_problems(name)
        a = jcases.arrays(problems)
        q0, t0, st = TJ.start_poses(shim, cam, a)
        assert np.all(st == 1)
        jo = TJ.shim_joint_options(shim, cam)
        lo = loss_options(shim, jo)
        s = shim_robust(shim, cam, a, q0, t0, jo=jo, lo=lo)
        out[name] = dict(cam=cam, problems=problems, a=a, q0=q0, t0=t0, jo=jo, lo=lo, s=s,
                         cmp=[compare_problem(shim, cam, a, k, s, q0, t0, jo, lo) for k in range(len(problems))])
    return out


@pytest.mark.parametrize("name", CAMS)
def test_seeded_sets_match_restatement(seeded_runs, name):
    """Minimiser, robust cost, cost shares, H_cl and weights against the restatement on clean and contaminated seeded sets (0.3 px,
    0.01 m; 6 and 12 images; default scales 3 and 5).  Measured here, worst of both cameras and of clean / contaminated: the largest
    pose gap 4.68e-8 (radtan 1.11e-8; both solvers stop on a function tolerance of 1e-15, which leaves the iterate ~sqrt(1e-15) of the
    problem's scale from the minimiser), the relative gap of the final cost 3.76e-15 and of the cost shares 9.1e-16, H_cl against the
    weighted dense Schur complement at the restatement's minimiser 5.84e-8 and 5.08e-15 at the answer's own poses, the weights
    1.41e-7 against the restatement's minimiser (8.4e-8 on these sets, 1.41e-7 with one scale 0) and 3.09e-14 at the answer's own
    poses.  Asserted one decade above, never above the gates.  Iterations: 8-11 (radtan) and 10-15 (kb), clean and contaminated alike."""
    e = seeded_runs[name]
    worst = dict(pose=0.0, cost=0.0, parts=0.0, hcl=0.0, hcl_same=0.0, w=0.0, w_same=0.0)
    for k, c in enumerate(e["cmp"]):
        sm = e["s"]["summaries"][k]
        assert sm.termination in (1, 2, 3), (k, sm.termination)
        assert np.all(e["s"]["status"] == 1)
        got = e["s"]["H_cl"][k]
        assert np.array_equal(got, got.T)
        for key in ("pose", "parts", "hcl", "hcl_same", "w", "w_same"):
            worst[key] = max(worst[key], c[key])
        worst["cost"] = max(worst["cost"], c["cost"], c["cost_self"])
        assert sm.final_cost <= sm.initial_cost
        assert abs(e["s"]["cost_parts"][k].sum() - sm.final_cost) <= 1e-14 * sm.final_cost
        print("%s problem %d: iterations %d, cost %.6g -> %.6g" % (name, k, sm.num_iterations, sm.initial_cost, sm.final_cost))
    print("%s: worst gaps %s" % (name, {k: "%.2e" % v for k, v in worst.items()}))
    assert np.all((e["s"]["w_corner"] > 0) & (e["s"]["w_corner"] <= 1)) and np.all((e["s"]["w_laser"] > 0) & (e["s"]["w_laser"] <= 1))
    assert worst["pose"] <= POSE_BOUND and worst["cost"] <= COST_BOUND and worst["parts"] <= COST_BOUND
    assert worst["hcl"] <= HCL_BOUND and worst["hcl_same"] <= HCL_SAME_POINT
    assert worst["w"] <= WEIGHT_BOUND and worst["w_same"] <= WEIGHT_SAME_POINT


def same_bits(s, k18):
    for key in ("q", "t", "poses_cl", "status"):
        assert np.array_equal(s[key], k18[key], equal_nan=key != "status"), key
    assert np.array_equal(s["H_cl"], k18["H_cl"], equal_nan=True) and np.array_equal(s["cost_parts"], k18["cost_parts"], equal_nan=True)
    for a, b in zip(s["summaries"], k18["summaries"]):
        for f in ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_evaluations", "initial_cost", "final_cost"):
            va, vb = getattr(a, f), getattr(b, f)
            assert va == vb or (va != va and vb != vb), f


@pytest.mark.parametrize("name", CAMS)
def test_both_scales_zero_are_k18_bit_for_bit(shim, seeded_runs, name):
    """loss_corner = loss_laser = 0: poses, summaries, H_cl, cost_parts and status are the bits of the shim's K18, on the seeded sets
    (clean and contaminated), with the hold flags, and on a call with images that take no part; every weight is 1, NaN where the
    image takes no part."""
    e = seeded_runs[name]
    cam = e["cam"]
    for kw in (dict(), dict(hold_board_poses=1), dict(hold_extrinsic=1)):
        jo = TJ.shim_joint_options(shim, cam, **kw)
        lo = loss_options(shim, jo, loss_corner=0.0, loss_laser=0.0)
        s = shim_robust(shim, cam, e["a"], e["q0"], e["t0"], jo=jo, lo=lo)
        k18 = TJ.shim_joint(shim, cam, e["a"], e["q0"], e["t0"], jo=jo)
        same_bits(s, k18)
        assert np.all(s["w_corner"] == 1.0) and np.all(s["w_laser"] == 1.0)
    p = jcases.problem(name, 9, 7, [144, 3, 144, 144, 144, 144, 144], 60)
    p["images"][3][4][5, 1] = np.nan
    p2 = jcases.problem(name, 10, 2, [3, 2], 10)
    a = jcases.arrays([p, p2])
    keep = np.ones(9, bool); keep[2] = False
    q0, t0, st = TJ.start_poses(shim, cam, a)
    jo = TJ.shim_joint_options(shim, cam)
    s = shim_robust(shim, cam, a, q0, t0, keep=keep, jo=jo, lo=loss_options(shim, jo, loss_corner=0.0, loss_laser=0.0))
    same_bits(s, TJ.shim_joint(shim, cam, a, q0, t0, keep=keep, jo=jo))
    part = s["status"] == 1
    assert list(s["status"]) == [1, 0, -1, -2, 1, 1, 1, 0, 0]
    for i in range(9):
        wc, wl = s["w_corner"][a["coff"][i]:a["coff"][i + 1]], s["w_laser"][a["poff"][i]:a["poff"][i + 1]]
        assert (np.all(wc == 1.0) and np.all(wl == 1.0)) if part[i] else (np.all(np.isnan(wc)) and np.all(np.isnan(wl))), i


def test_weights_nan_rule_and_untouched_poses(shim):
    """With the loss on: an image that takes no part (keep == 0, too few corners, a non-finite point) and every image of a problem that
    ended CLC_FAILURE get NaN weights and keep their poses bit for bit; the others get weights in (0, 1]; without the weight arrays
    the solve's outputs are the same bits."""
    name = "radtan"
    cam = jcases.CAMERAS[name]
    p = cases.contaminate(jcases.problem(name, 9, 7, [144, 3, 144, 144, 144, 144, 144], 60), np.random.default_rng(3))
    p["images"][3][4][5, 1] = np.nan
    p2 = jcases.problem(name, 10, 2, [3, 2], 10)
    p3 = jcases.problem(name, 11, 4, 144, 50)
    a = jcases.arrays([p, p2, p3])
    a["poses_cl0"][2, 1] = np.nan  # a non-finite start T_cl: the third problem fails
    keep = np.ones(13, bool); keep[2] = False
    q0, t0, st = TJ.start_poses(shim, cam, a)
    s = shim_robust(shim, cam, a, q0, t0, keep=keep)
    assert list(s["status"]) == [1, 0, -1, -2, 1, 1, 1, 0, 0, 1, 1, 1, 1]
    assert [s["summaries"][k].termination == 6 for k in range(3)] == [False, True, True]
    for i in range(13):
        wc, wl = s["w_corner"][a["coff"][i]:a["coff"][i + 1]], s["w_laser"][a["poff"][i]:a["poff"][i + 1]]
        if i in (0, 4, 5, 6):
            assert np.all((wc > 0) & (wc <= 1)) and np.all((wl > 0) & (wl <= 1)), i
        else:
            assert np.all(np.isnan(wc)) and np.all(np.isnan(wl)), i
            assert np.array_equal(s["q"][i], q0[i]) and np.array_equal(s["t"][i], t0[i])
    s2 = shim_robust(shim, cam, a, q0, t0, keep=keep, weights=False)
    same_bits(s2, s)
    assert np.all(s2["w_corner"] == -7.0) and np.all(s2["w_laser"] == -7.0)


@pytest.mark.parametrize("scales", [(0.0, 5.0), (3.0, 0.0)])
def test_one_scale_zero_matches_restatement(shim, seeded_runs, scales):
    """One term with its loss, the other plain least squares: against the restatement on the contaminated set, within the bounds of the
    seeded sets; the weights of the term without a loss are exactly 1."""
    e = seeded_runs["radtan"]
    cam = e["cam"]
    a = jcases.arrays([e["problems"][1]])
    n = len(a["coff"]) - 1
    q0, t0 = e["q0"][e["a"]["prob_off"][1]:e["a"]["prob_off"][2]], e["t0"][e["a"]["prob_off"][1]:e["a"]["prob_off"][2]]
    assert len(q0) == n
    lo = loss_options(shim, e["jo"], loss_corner=scales[0], loss_laser=scales[1])
    s = shim_robust(shim, cam, a, q0, t0, jo=e["jo"], lo=lo)
    c = compare_problem(shim, cam, a, 0, s, q0, t0, e["jo"], lo)
    print("one scale zero %s: %s" % (scales, {k: "%.2e" % c[k] for k in ("pose", "cost", "cost_self", "parts", "hcl", "hcl_same", "w", "w_same")}))
    assert c["pose"] <= POSE_BOUND and max(c["cost"], c["cost_self"], c["parts"]) <= COST_BOUND
    assert c["hcl"] <= HCL_BOUND and c["hcl_same"] <= HCL_SAME_POINT and c["w"] <= WEIGHT_BOUND and c["w_same"] <= WEIGHT_SAME_POINT
    assert np.all((s["w_corner"] if scales[0] == 0.0 else s["w_laser"]) == 1.0)
    assert np.any((s["w_laser"] if scales[0] == 0.0 else s["w_corner"]) < 0.5)


@pytest.mark.parametrize("name", CAMS)
def test_held_board_poses_reach_the_oracles_cauchy_solve(shim, seeded_runs, name):
    """hold_board_poses = 1 with only the laser loss: T_cl and the laser share of the cost against the oracle's solve with use_loss = 1
    on the records {n_i, d_i, p, scale} of the start poses.  The scale mapping: the oracle's residual is scale * (n . (R_cl p + t_cl)
    + d) under CauchyLoss(loss_scale_factor * scale) (the reference's CauchyLoss(0.05 * scale)), so with scale = 1 / sigma_laser for
    every record (no per-pose 1 / sqrt(n): the records are built here, not by the reference's front end) the residual is K22's r and
    the loss scale a = loss_scale_factor / sigma_laser = loss_laser: loss_scale_factor = loss_laser * sigma_laser, exactly 0.05 at
    the defaults.  The mapping is exact, so the comparison is made on the oracle and held to the parity gates (measured: poses
    2.54e-8, cost 2.26e-14 relative)."""
    import oracle
    e = seeded_runs[name]
    jo = TJ.shim_joint_options(shim, e["cam"], hold_board_poses=1)
    lo = loss_options(shim, jo, loss_corner=0.0)
    s = shim_robust(shim, e["cam"], e["a"], e["q0"], e["t0"], jo=jo, lo=lo)
    assert np.array_equal(s["q"], e["q0"]) and np.array_equal(s["t"], e["t0"])
    worst = [0.0, 0.0]
    for k in range(len(e["problems"])):
        rec = TJ.plane_records(e["a"], k, e["q0"], e["t0"], jo.sigma_laser)
        o = oracle.default_options()
        o.use_loss = 1
        o.loss_scale_factor = lo.loss_laser * jo.sigma_laser
        o.max_num_iterations = 50
        o.function_tolerance, o.parameter_tolerance, o.gradient_tolerance = 1e-15, 1e-14, 1e-16
        r = oracle.solve(rec, np.asarray(e["a"]["poses_cl0"][k], np.float64), o)
        R, t = ref.pose7_to_Rt(r.pose)
        Rm, tm = ref.pose7_to_Rt(s["poses_cl"][k])
        worst[0] = max(worst[0], np.abs(R - Rm).max(), np.abs(t - tm).max())
        worst[1] = max(worst[1], abs(s["cost_parts"][k][1] - r.summary.final_cost) / r.summary.final_cost)
        prob, idx = restatement_problem(shim, e["cam"], e["a"], k, jo, lo)
        Hd = rref.normal_matrix(prob, *TJ.poses_of(s, idx, k))[0]
        assert np.linalg.norm(s["H_cl"][k] - Hd[:6, :6]) <= 1e-12 * np.linalg.norm(Hd[:6, :6])
    print("%s: held board poses, laser loss only, vs the oracle with use_loss = 1: poses %.2e, cost %.2e" % (name, *worst))
    assert worst[0] <= POSE_GATE and worst[1] <= COST_GATE


def recovery_table(shim, name="radtan", n_sets=8):
    """K18 and K22 on clean and contaminated data of the recovery sets -> rows (set, K18 clean, K18 contaminated, K22 clean, K22
    contaminated: |t_cl - truth| in metres), the K22 runs on the contaminated data."""
    cam = jcases.CAMERAS[name]
    rows, runs = [], []
    for k, (clean, dirty) in enumerate(cases.recovery_sets(name, n_sets)):
        err = []
        for prob in (clean, dirty):
            a = jcases.arrays([prob])
            q0, t0, st = TJ.start_poses(shim, cam, a)
            s18 = TJ.shim_joint(shim, cam, a, q0, t0)
            s22 = shim_robust(shim, cam, a, q0, t0)
            err.append((cases.tcl_distance(s18["poses_cl"][0], prob["pose_cl_true"]), cases.tcl_distance(s22["poses_cl"][0], prob["pose_cl_true"]),
                        s18["summaries"][0].num_iterations, s22["summaries"][0].num_iterations))
        rows.append((k, err[0][0], err[1][0], err[0][1], err[1][1], err[0][2], err[1][2], err[0][3], err[1][3]))
        runs.append((dirty, a, s22))
    return rows, runs


def test_recovery_under_planted_outliers(shim):
    """8 seeded sets of 30 images (144 corners, 100 points), 10 % of each image's points pulled 0.10-0.30 m towards the scanner and 5 %
    of its corners moved 3-10 px (jointrobust_cases.contaminate; the case file asserts the same separation at the true poses).  At
    K22's answer every planted observation has w < 0.5 and >= 95 % of the others w >= 0.5, and the mean distance of t_cl from the
    truth is smaller for K22 than for K18 on the same contaminated data.  No ratio is fixed in advance; measured here (radtan, means):
    K18 1.92 mm clean and 31.06 mm contaminated, K22 1.89 mm clean and 2.64 mm contaminated (profiles/joint_robust.md has every set)."""
    rows, runs = recovery_table(shim)
    for dirty, a, s in runs:
        assert s["summaries"][0].termination in (1, 2, 3) and np.all(s["status"] == 1)
        down, frac = cases.separation(s["w_corner"], s["w_laser"], *cases.planted_masks(dirty))
        assert down and frac >= 0.95, (down, frac)
    print("set  K18 clean  K18 contaminated  K22 clean  K22 contaminated   (|t_cl - truth|, mm; iterations K18 c/d, K22 c/d)")
    for r in rows:
        print("%3d  %9.2f  %16.2f  %9.2f  %16.2f   %d/%d %d/%d" % (r[0], *(1e3 * np.array(r[1:5])), *r[5:]))
    m = np.mean(np.array([r[1:5] for r in rows]), 0)
    print("mean %9.2f  %16.2f  %9.2f  %16.2f" % tuple(1e3 * m))
    assert m[3] < m[1]


def test_sanitized_standalone_program(tmp_path):
    """tests/shim/jointrobust_sanitize_main.cpp: the per-problem host functions (solve and weights) on the edge shapes, every array of
    its exact size, built with -fsanitize=address,undefined and run as an ordinary process."""
    exe = str(tmp_path / "jointrobust_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "shim", "jointrobust_sanitize_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "shapes ok" in p.stdout, p.stdout
