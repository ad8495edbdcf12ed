"""K23 (csrc/clc_fullcal.hpp on clc_arrow.hpp) on the host: the evaluation blocks of the one robust cost, the solve over the 16-wide shared
block and the weights compiled with g++ (tests/shim/fullcal_shim.cpp) against the numpy / scipy restatement tests/fullcal_ref.py on
seeded sets with a planted range error, clean and contaminated (tests/fullcal_cases.py): the Jacobians of every row against central
differences through Plus, the weighted blocks and the exactly-zero cross block of C, the minimiser, cost, cost shares, RMS, H_full
and weights; the reductions onto K19's and K21's host builds and onto the oracle; held parameters; status, keep and failed-problem
semantics; recovery of T_cl against K21 and K22; the refusals of the C ABI (they need no device); a stand-alone AddressSanitizer /
UBSan program over the edge shapes."""
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
import fullcal_cases as cases  # noqa: E402
import fullcal_ref as ref  # noqa: E402
import joint_ref as jref  # noqa: E402
import test_campose_host as H  # noqa: E402
import test_camcal_host as TC  # noqa: E402
import test_joint_host as TJ  # noqa: E402
import test_jointrobust_host as TR  # noqa: E402
import test_laserrange_host as TL  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402
from camlasercalibratool_amd.camera import ClcCamera  # noqa: E402

CAMS = ["radtan", "kb"]
d = H._d
GXX = TJ.GXX


def build_shim(path):
    subprocess.check_call(GXX + ["-shared", os.path.join(HERE, "shim", "fullcal_shim.cpp"), "-o", path])
    L = C.CDLL(path)
    L.shim_kb_theta.restype = C.c_double
    L.shim_kb_theta.argtypes = [C.c_void_p, C.c_double]
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(str(tmp_path_factory.mktemp("fc") / "libfullcal_shim.so"))


def full_options(L, model, **kw):
    fo = _capi.FullOptions()
    L.shim_full_options_default(C.byref(fo), C.c_int(model))
    for k, v in kw.items():
        setattr(fo, k, v)
    return fo


def full_options_from(fo, **kw):
    """A copy of the options fo with the given fields replaced."""
    out = _capi.FullOptions.from_buffer_copy(bytes(fo))
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def start_poses(L, cam, a):
    """K10 (the shim's) on every image under `cam` -> q [n, 4], t [n, 3], status [n]."""
    q, t, _, st, _ = H.shim_board_poses(L, cam, a["corners"], a["board"], a["coff"])
    return q, t, st


def shim_full(L, cams, a, q0, t0, keep=None, fo=None, poses_cl=None, range0=None, max_iterations=None, weights=True, corners=True,
              prob_off=True):
    """shim_calibrate_full on the arrays of fullcal_cases.arrays -> dict, the keys of Solver.calibrate_full (+ k [np, 8])."""
    n, npb = len(a["poff"]) - 1, len(a["prob_off"]) - 1
    q, t = np.array(q0, dtype=np.float64, order="C"), np.array(t0, dtype=np.float64, order="C")
    pcl = np.array(a["poses_cl0"] if poses_cl is None else poses_cl, dtype=np.float64, order="C").reshape(npb, 7)
    rg = np.array(a["range0"] if range0 is None else range0, dtype=np.float64, order="C").reshape(npb, 2)
    o = _capi.Options()
    L.shim_pose_options_default(C.byref(o))
    if max_iterations is not None:
        o.max_num_iterations = max_iterations
    fo = fo or full_options(L, cams[0].model)
    cc = (ClcCamera * max(npb, 1))(*[c.to_c() for c in cams])
    sm = (_capi.Summary * max(npb, 1))()
    Hf = np.empty((npb, 16, 16)); parts = np.empty((npb, 2)); rms = np.empty(npb); st = np.full(n, -99, dtype=np.int32)
    wc, wl = np.full(len(a["corners"]), -7.0), np.full(len(a["pts"]), -7.0)
    k = None if keep is None else np.ascontiguousarray(np.asarray(keep).astype(np.uint8))
    first = int(a["prob_off"][0]) if prob_off else 0
    L.shim_calibrate_full(C.byref(o), C.byref(fo), d(a["corners"]) if corners else None, d(a["board"]) if corners else None,
                          d(a["coff"]) if corners else None, d(a["pts"]), d(a["poff"]), None if k is None else d(k), C.c_longlong(n - first),
                          d(a["prob_off"]) if prob_off else None, C.c_longlong(npb), cc, d(q), d(t), d(pcl), d(rg), sm, d(Hf), d(parts), d(rms),
                          d(st), d(wc) if weights else None, d(wl) if weights else None)
    ks = np.array([list(c.proj) + list(c.dist) for c in cc][:npb]).reshape(npb, 8)
    return dict(k=ks, cameras=[TC.with_k(cams[i], ks[i]) for i in range(npb)], q=q, t=t, poses_cl=pcl, range=rg, summaries=sm, H_full=Hf,
                cost_parts=parts, rms_px=rms, status=st, w_corner=wc, w_laser=wl)


def uses_corners(fo):
    return not (fo.hold_board_poses and fo.hold_intrinsics_mask == 0xFF)


def restatement_problem(cam, a, k, fo, keep=None):
    """Problem k of the arrays as fullcal_ref takes it (the participating images only) -> (prob, image indices)."""
    uc = uses_corners(fo)
    idx = [i for i in range(a["prob_off"][k], a["prob_off"][k + 1])
           if (not uc or a["coff"][i + 1] - a["coff"][i] >= 4) and (keep is None or keep[i])]
    empty = np.zeros((0, 2))
    prob = dict(model=cam.model, px=[a["corners"][a["coff"][i]:a["coff"][i + 1]].astype(np.float64) if uc else empty for i in idx],
                board=[a["board"][a["coff"][i]:a["coff"][i + 1]].astype(np.float64) if uc else empty for i in idx],
                pts=[a["pts"][a["poff"][i]:a["poff"][i + 1]] for i in idx], spx=fo.sigma_px if uc else 1.0, sl=fo.sigma_laser,
                lc=fo.loss_corner, ll=fo.loss_laser)
    return prob, idx


def state_of(s, idx, k):
    Rs = [jref.quat_wxyz_to_R(s["q"][i]) for i in idx]
    ts = [s["t"][i].copy() for i in idx]
    Rcl, tcl = jref.pose7_to_Rt(s["poses_cl"][k])
    return Rs, ts, Rcl, tcl, float(s["range"][k][0]), float(s["range"][k][1]), s["k"][k].copy()


def hold_kw(fo):
    return dict(hold_ext=bool(fo.hold_extrinsic), range_mask=int(fo.hold_range_mask), intr_mask=int(fo.hold_intrinsics_mask))


def weights_of(a, s, idx):
    wc = np.concatenate([s["w_corner"][a["coff"][i]:a["coff"][i + 1]] for i in idx]) if idx else np.zeros(0)
    wl = np.concatenate([s["w_laser"][a["poff"][i]:a["poff"][i + 1]] for i in idx]) if idx else np.zeros(0)
    return wc, wl


def compare_problem(cam0, a, k, s, q0, t0, fo, keep=None):
    """One problem of a call against the restatement: its minimiser from the same start and from the call's own answer (the lower of
    the two) -> dict of gaps; the shared parameters in units of their own predicted 1 sigma."""
    prob, idx = restatement_problem(cam0, a, k, fo, keep)
    start = ([jref.quat_wxyz_to_R(q0[i]) for i in idx], [t0[i].copy() for i in idx], *jref.pose7_to_Rt(a["poses_cl0"][k]),
             float(a["range0"][k][0]), float(a["range0"][k][1]), TC.k_of(cam0))
    mine = state_of(s, idx, k)
    kw = hold_kw(fo)
    hb = bool(fo.hold_board_poses)
    cand = [ref.solve(prob, mine, hold_board=hb, **kw), ref.solve(prob, start, hold_board=hb, **kw)]
    best, best_cost = min(cand, key=lambda c: c[1])
    free = ref.free_shared(no_laser=ref.no_laser(prob), **kw)
    Hr = ref.schur(ref.normal_matrix(prob, *best)[0], free, hb)
    Hs = ref.schur(ref.normal_matrix(prob, *mine)[0], free, hb)
    sg = ref.free_sigma(Hr, free)
    # the shared block's gap in the tangent of the restatement's minimiser: [dt_cl, dtheta_cl, b, kappa, intrinsics]
    dth = jref.skew(np.zeros(3))
    dR = best[2].T @ mine[2]
    dth = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2.0
    delta = np.r_[mine[3] - best[3], dth, mine[4] - best[4], mine[5] - best[5], mine[6] - best[6]]
    cost = s["summaries"][k].final_cost
    cc, cl = ref.cost_parts(prob, *mine)
    wc, wl = weights_of(a, s, idx)
    wc_same, wl_same = ref.weights(prob, *mine)
    wc_best, wl_best = ref.weights(prob, *best)
    n_corners = sum(len(p) for p in prob["px"])
    rms_ref = fo.sigma_px * np.sqrt(2 * ref.cost_parts(prob, *best)[0] / n_corners) if n_corners else np.nan
    nz = lambda M: np.linalg.norm(M) or 1.0
    got = s["H_full"][k]
    gap = lambda x, y: np.abs(x - y).max(initial=0.0)
    return dict(shared_sigma=float(np.max(np.abs(delta[free]) / sg[free])) if free else 0.0,
                pose=max([np.abs(Ra - Rb).max() for Ra, Rb in zip(mine[0], best[0])] + [np.abs(ta - tb).max() for ta, tb in zip(mine[1], best[1])]),
                tcl=max(np.abs(mine[2] - best[2]).max(), np.abs(mine[3] - best[3]).max()),
                cost=abs(cost - best_cost) / best_cost, cost_self=abs(cost - (cc + cl)) / (cc + cl),
                parts=max(abs(s["cost_parts"][k][0] - cc), abs(s["cost_parts"][k][1] - cl)) / (cc + cl),
                rms=abs(s["rms_px"][k] - rms_ref) / rms_ref if n_corners else 0.0,
                h=np.linalg.norm(got - Hr) / nz(Hr), h_same=np.linalg.norm(got - Hs) / nz(Hs),
                w=max(gap(wc, wc_best) if uses_corners(fo) else 0.0, gap(wl, wl_best)),
                w_same=max(gap(wc, wc_same) if uses_corners(fo) else 0.0, gap(wl, wl_same)),
                sigma=sg, free=free, prob=prob, idx=idx, best=best, mine=mine, ref_cost=best_cost)


# The project's parity gates: 1e-6 on poses, 1e-8 relative on cost.  The bounds below are one decade over the worst gaps measured on
# the seeded sets of both cameras (the figures: test_seeded_sets_match_restatement's docstring), never above the gates.
POSE_GATE, COST_GATE = 1e-6, 1e-8
POSE_BOUND = 2e-7             # largest gap of any R entry or t component (T_cl and every T_ca) to the restatement's minimiser (1.98e-8)
SHARED_SIGMA_BOUND = 2.1e-5   # largest gap of a free shared parameter to the restatement's, in units of its own predicted 1 sigma (2.08e-6)
COST_BOUND = 3.5e-13          # relative gap of the final cost and of the two cost shares (3.48e-14)
RMS_BOUND = 6e-8              # relative gap of the RMS in pixels to the one of the restatement's minimiser (5.98e-9)
H_BOUND = 1.9e-7              # relative (Frobenius) gap of H_full to the weighted dense Schur complement at the restatement's minimiser (1.83e-8)
H_SAME_POINT = 1.9e-14        # the same at the answer's own point: what the blocks and the reduction themselves leave (1.90e-15)
WEIGHT_BOUND = 2.8e-6         # largest gap of a weight to the restatement's at its minimiser (2.71e-7)
WEIGHT_SAME_POINT = 1e-11     # ... and at the answer's own point (9.98e-13: a corner's e is a difference of pixels of a few hundred over 0.3)
BLOCK_BOUND = 4.9e-13         # the per-image blocks against the weighted J^T J, J^T r (4.82e-14)


def test_struct_layout_and_defaults(shim):
    F = _capi.FullOptions
    assert shim.shim_full_options_size() == 48 == C.sizeof(F)
    assert [getattr(F, n).offset for n, _ in F._fields_] == [0, 8, 16, 24, 32, 36, 40, 44]
    assert shim.shim_full_eval_doubles() == 277 and shim.shim_full_image_doubles() * 8 < 8704  # < 8.5 KB per image
    L = _capi.lib()
    for fn in (shim.shim_full_options_default, L.clc_full_options_default):
        for model, mask in ((1, 0), (2, 0xC0)):
            fo = F(-1.0, -1.0, -1.0, -1.0, 7, 7, 7, 7)
            fn(C.byref(fo), C.c_int32(model))
            assert (fo.sigma_px, fo.sigma_laser, fo.loss_corner, fo.loss_laser) == (0.3, 0.01, 3.0, 5.0)
            assert (fo.hold_intrinsics_mask, fo.hold_range_mask, fo.hold_board_poses, fo.hold_extrinsic) == (mask, 0, 0, 0)
    assert _capi.default_full_options(2).hold_intrinsics_mask == 0xC0
    for name in ("clc_full_options_default", "clc_calibrate_full", "clc_calibrate_full_device"):
        assert name in _capi.EXPORTED and hasattr(L, name)
    assert L.clc_version() == 210
    import camlasercalibratool_amd as pkg
    for name in ("CalibrateFull", "CalibrateFullBatch", "FullOptions", "default_full_options"):
        assert name in pkg.__all__ and hasattr(pkg, name)


def full_call(L, fo, device=False, cams=True, model=1, **kw):
    c = (ClcCamera * 1)(H.CAMERAS["pinhole"].to_c())
    c[0].model = model
    z = np.zeros(2, dtype=np.int64)
    args = dict(coff=d(z), poff=d(z), q=d(np.zeros(4)), t=d(np.zeros(3)), cl=d(np.zeros(7)), rg=d(np.zeros(2)), sm=(_capi.Summary * 1)(),
                st=d(np.zeros(1, np.int32)), prob=None, n_images=1, n_problems=1, opt=None)
    args.update(kw)
    fn = L.clc_calibrate_full_device if device else L.clc_calibrate_full
    return fn(None, c if cams else None, C.byref(args["opt"]) if args["opt"] is not None else None, C.byref(fo) if fo is not None else None,
              None, None, args["coff"], None, args["poff"], None, C.c_size_t(args["n_images"]), args["prob"], C.c_size_t(args["n_problems"]),
              args["q"], args["t"], args["cl"], args["rg"], args["sm"], None, None, None, args["st"], None, None)


def test_refusals_need_no_device():
    """What K19, K21 and K22 refuse for their share of the options, with their messages behind the new name; mask bits out of range; all
    16 shared parameters held together with hold_board_poses: CLC_ERR_INVALID_ARG before any device work (the handle is NULL
    throughout).  sigma_px is looked at only while the corners take part."""
    L = _capi.lib()
    who = "clc_calibrate_full: "
    nan, inf = float("nan"), float("inf")
    base = lambda **kw: _capi.FullOptions(**dict(dict(sigma_px=0.3, sigma_laser=0.01, loss_corner=3.0, loss_laser=5.0), **kw))
    rows = [(dict(sigma_px=v), "sigma_px must be finite and > 0") for v in (nan, inf, 0.0, -1e-3)]
    rows += [(dict(sigma_laser=v), "sigma_laser must be finite and > 0") for v in (nan, inf, 0.0, -0.01)]
    rows += [(dict(loss_corner=v), "loss_corner must be finite and >= 0") for v in (nan, inf, -inf, -1e-3)]
    rows += [(dict(loss_laser=v), "loss_laser must be finite and >= 0") for v in (nan, inf, -inf, -1e-3)]
    rows += [(dict(hold_intrinsics_mask=0x100), "hold_intrinsics_mask has bits beyond the 8 intrinsics"),
             (dict(hold_range_mask=4), "hold_range_mask outside 0..3"), (dict(hold_range_mask=-1), "hold_range_mask outside 0..3"),
             (dict(hold_intrinsics_mask=0xFF, hold_range_mask=3, hold_extrinsic=1, hold_board_poses=1), "everything is held")]
    for kw, msg in rows:
        assert full_call(L, base(**kw)) == -1
        assert L.clc_last_error().decode() == who + msg, (kw, L.clc_last_error())
    assert full_call(L, base(sigma_px=nan), device=True) == -1
    assert L.clc_last_error().decode() == "clc_calibrate_full_device: sigma_px must be finite and > 0"
    # the good ones get as far as the missing handle: zero scales; a sigma_px that is not looked at; both hold flags while b moves
    for fo in (None, base(loss_corner=0.0, loss_laser=0.0), base(sigma_px=nan, hold_intrinsics_mask=0xFF, hold_board_poses=1),
               base(hold_intrinsics_mask=0xFF, hold_range_mask=2, hold_extrinsic=1, hold_board_poses=1)):
        assert full_call(L, fo) == -1 and L.clc_last_error().decode() == who + "bad argument", L.clc_last_error()
    assert full_call(L, None, model=7) == -1 and L.clc_last_error().decode() == who + "unknown camera model"
    assert full_call(L, None, cams=False) == -1 and L.clc_last_error().decode() == who + "bad argument"
    o = _capi.default_options()
    o.use_loss = 1
    assert full_call(L, None, opt=o) == -1 and "use_loss must be 0" in L.clc_last_error().decode()
    bad = np.array([3, 1], dtype=np.int64)
    for kw in (dict(coff=d(bad)), dict(poff=d(bad)), dict(prob=d(bad))):
        assert full_call(L, None, **kw) == -1 and L.clc_last_error().decode() == who + "offsets not monotone"
    for key in ("coff", "poff", "q", "t", "cl", "rg", "sm", "st"):
        assert full_call(L, None, **{key: None}) == -1 and L.clc_last_error().decode() == who + "bad argument", key
    # without the corners their offsets are not needed
    assert full_call(L, base(hold_intrinsics_mask=0xFF, hold_board_poses=1), coff=d(bad)) == -1
    assert L.clc_last_error().decode() == who + "bad argument"


def eval_point(name, seed=5):
    """A small contaminated problem with a planted range error, away from its minimiser -> cam, problem, arrays, state."""
    p = cases.problem(name, seed, 3, [144, 65, 20], [100, 65, 0], dirty=True)
    a = cases.arrays([p])
    rng = np.random.default_rng(1)
    Rs = [im[2] @ jref.exp_so3(rng.normal(size=3) * 0.01) for im in p["images"]]
    ts = [im[3] + rng.normal(size=3) * 0.005 for im in p["images"]]
    Rcl, tcl = jref.pose7_to_Rt(p["pose_cl0"])
    return p["cam0"], p, a, (Rs, ts, Rcl, tcl, 0.004, -0.003, TC.k_of(p["cam0"]))


def shim_records(shim, cam, fo, prob, X):
    """The evaluation record of every image of the restatement's problem at X -> [P, 277]."""
    out = []
    for i in range(len(X[0])):
        E = np.full(277, np.nan)
        px = np.ascontiguousarray(prob["px"][i], dtype=np.float32)
        B = np.ascontiguousarray(prob["board"][i], dtype=np.float32)
        pts = np.ascontiguousarray(prob["pts"][i])
        c = TC.with_k(cam, X[6]).to_c()
        shim.shim_full_eval_image(C.byref(c), C.byref(fo), d(px), d(B), C.c_longlong(len(px)), d(pts), C.c_longlong(len(pts)),
                                  d(jref.Rt_to_pose7(X[0][i], X[1][i])), d(np.ascontiguousarray(jref.Rt_to_pose7(X[2], X[3]))),
                                  d(np.array([X[4], X[5]])), d(E))
        out.append(E)
    return np.array(out)


TRI16 = np.triu_indices(16)


@pytest.mark.parametrize("name", CAMS)
@pytest.mark.parametrize("scales", [(3.0, 5.0), (0.0, 0.0), (0.5, 0.7)])
def test_blocks_match_weighted_normal_equations(shim, name, scales):
    """The shim's per-image blocks A, B, g, C, g_c are the restatement's J^T W J and J^T W r and the two cost parts its 1/2 sum rho, at a
    point away from the minimiser of a contaminated problem; the [T_cl, b, kappa] x intrinsics block of C is exactly zero in every
    record.  Measured: 4.82e-14 relative to the largest entry of a block, asserted one decade above at BLOCK_BOUND."""
    cam, p, a, X = eval_point(name)
    fo = full_options(shim, cam.model, loss_corner=scales[0], loss_laser=scales[1])
    prob, idx = restatement_problem(cam, a, 0, fo)
    E = shim_records(shim, cam, fo, prob, X)
    r, J, ncr = ref.residuals(prob, *X)
    w = ref.row_weights(prob, *X)
    zc, zl, _, _ = ref.block_z(prob, *X)
    worst, nc0, np0 = 0.0, 0, 0
    for i in range(3):
        nci, npi = len(prob["px"][i]), len(prob["pts"][i])
        rows = np.concatenate([2 * nc0 + np.arange(2 * nci), ncr + np0 + np.arange(npi)]).astype(int)
        Ji, Jc, ri, wi = J[rows][:, 16 + 6 * i:22 + 6 * i], J[rows][:, :16], r[rows], w[rows]
        cc = 0.5 * np.sum(ref.rho(zc[nc0:nc0 + nci], fo.loss_corner))
        cl = 0.5 * np.sum(ref.rho(zl[np0:np0 + npi], fo.loss_laser))
        Cm = np.zeros((16, 16))
        Cm[TRI16] = E[i][123:259]
        assert np.all(Cm[:8, 8:] == 0.0) and not np.any(np.isnan(E[i]))
        for got, want in ((E[i][0:21], (Ji.T @ (Ji * wi[:, None]))[np.triu_indices(6)]), (E[i][21:117], (Ji.T @ (Jc * wi[:, None])).reshape(-1)),
                          (E[i][117:123], Ji.T @ (wi * ri)), (Cm[:8, :8], np.triu(Jc[:, :8].T @ (Jc[:, :8] * wi[:, None]))),
                          (Cm[8:, 8:], np.triu(Jc[:, 8:].T @ (Jc[:, 8:] * wi[:, None]))), (E[i][259:275], Jc.T @ (wi * ri)),
                          (E[i][275:276], [cc]), (E[i][276:277], [cl])):
            want = np.asarray(want)
            if np.abs(want).max() > 0:
                worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
            else:
                assert np.all(got == 0)
        nc0 += nci
        np0 += npi
    print("%s %s: shim blocks vs weighted J^T J of the restatement, worst relative gap %.2e" % (name, scales, worst))
    assert worst <= BLOCK_BOUND


@pytest.mark.parametrize("name", CAMS)
def test_jacobians_match_central_differences(shim, name):
    """Every row of the dense Jacobian — the corner rows over the intrinsics and the image's tangent, the laser rows over T_cl's tangent,
    b, kappa and the image's tangent — against central differences of the residuals through the project's Plus, five-point stencil,
    h = 1e-4 (truncation O(h^4); the intrinsics, in which the residuals are linear: 1e-3 of each one's size); the shim's laser row (range_point) against
    the restatement's.  The bound is the differences' own error: a residual is a difference of two numbers over sigma — pixels of a few hundred over 0.3, metres of about one
    over 0.01 — and is known to eps times the larger of those quotients, the stencil divides 1.5 of that by h, per column relative to
    the column's largest entry, times ten, plus 1e-9 for what is left of the truncation."""
    cam, p, a, X = eval_point(name)
    fo = full_options(shim, cam.model)
    prob, idx = restatement_problem(cam, a, 0, fo)
    r, J, ncr = ref.residuals(prob, *X)
    P = 3
    hs = np.r_[np.full(8, 1e-4), 1e-3 * np.maximum(np.abs(X[6]), 1e-2), np.full(6 * P, 1e-4)]  # (the intrinsics differ by five orders of magnitude)
    noise = np.finfo(float).eps * max(np.abs(np.concatenate(prob["px"])).max() / fo.sigma_px, np.abs(np.concatenate(prob["pts"])).max() / fo.sigma_laser)

    def moved(c, step):
        Rs, ts, Rcl, tcl, b, kap, k = list(X[0]), list(X[1]), X[2], X[3], X[4], X[5], X[6].copy()
        dl = np.zeros(6)
        if c < 6:
            dl[c] = step
            Rcl, tcl = jref.plus(Rcl, tcl, dl)
        elif c == 6:
            b += step
        elif c == 7:
            kap += step
        elif c < 16:
            k[c - 8] += step
        else:
            i = (c - 16) // 6
            dl[(c - 16) % 6] = step
            Rs[i], ts[i] = jref.plus(Rs[i], ts[i], dl)
        return Rs, ts, Rcl, tcl, b, kap, k

    f = lambda Y: ref.residuals(prob, *Y, jac=False)[0]
    Jn = np.empty_like(J)
    for c in range(J.shape[1]):
        h = hs[c]
        Jn[:, c] = (-f(moved(c, 2 * h)) + 8 * f(moved(c, h)) - 8 * f(moved(c, -h)) + f(moved(c, -2 * h))) / (12 * h)
    colmax = np.abs(J).max(0)
    gap = np.abs(J - Jn).max(0) / colmax
    tol = 10 * 1.5 * noise / (hs * colmax) + 1e-9
    print("%s: Jacobian vs differences, worst column %.2e (its bound %.2e)" % (name, gap.max(), tol[np.argmax(gap / tol)]))
    assert np.all(gap <= tol), (gap / tol).max()
    # the shim's laser row is the restatement's
    worst = 0.0
    for i in range(2):
        for kk in (0, len(prob["pts"][i]) - 1):
            Ji, Jc, rr = np.empty(6), np.empty(8), np.empty(1)
            shim.shim_full_point(d(jref.Rt_to_pose7(X[0][i], X[1][i])), d(np.ascontiguousarray(jref.Rt_to_pose7(X[2], X[3]))),
                                 d(np.array([X[4], X[5]])), d(np.ascontiguousarray(prob["pts"][i][kk])), C.c_double(1.0 / fo.sigma_laser),
                                 d(Ji), d(Jc), d(rr))
            row = ncr + sum(len(prob["pts"][j]) for j in range(i)) + kk
            worst = max(worst, np.abs(Jc - J[row, :8]).max() / np.abs(J[row, :8]).max(), np.abs(Ji - J[row, 16 + 6 * i:22 + 6 * i]).max() /
                        np.abs(J[row]).max(), abs(rr[0] - r[row]) / max(abs(r[row]), 1.0))
    print("%s: range_point vs the restatement's laser row %.2e" % (name, worst))
    assert worst <= 1e-12


def problem_starts(L, problems, a):
    """K10's poses under every problem's own start camera -> q0, t0."""
    n = len(a["coff"]) - 1
    q0, t0 = np.zeros((n, 4)), np.zeros((n, 3))
    for k, p in enumerate(problems):
        q, t, st = start_poses(L, p["cam0"], a)
        sl = slice(a["prob_off"][k], a["prob_off"][k + 1])
        q0[sl], t0[sl] = q[sl], t[sl]
    return q0, t0


@pytest.fixture(scope="module")
def seeded_runs(shim):
    out = {}
    for name in CAMS:
        problems = cases.seeded(name)
        a = cases.arrays(problems)
        cams = [p["cam0"] for p in problems]
        q0, t0 = problem_starts(shim, problems, a)
        fo = full_options(shim, cams[0].model)
        s = shim_full(shim, cams, a, q0, t0, fo=fo)
        out[name] = dict(problems=problems, a=a, cams=cams, q0=q0, t0=t0, fo=fo, s=s,
                         cmp=[compare_problem(cams[k], a, k, s, q0, t0, fo) for k in range(len(problems))])
    return out


def check_bounds(c, tag=""):
    assert c["pose"] <= POSE_BOUND and c["tcl"] <= POSE_BOUND and c["shared_sigma"] <= SHARED_SIGMA_BOUND, (tag, c["pose"], c["tcl"], c["shared_sigma"])
    assert max(c["cost"], c["cost_self"], c["parts"]) <= COST_BOUND and c["rms"] <= RMS_BOUND, (tag, c["cost"], c["cost_self"], c["parts"], c["rms"])
    assert c["h"] <= H_BOUND and c["h_same"] <= H_SAME_POINT and c["w"] <= WEIGHT_BOUND and c["w_same"] <= WEIGHT_SAME_POINT, (
        tag, c["h"], c["h_same"], c["w"], c["w_same"])


@pytest.mark.parametrize("name", CAMS)
def test_seeded_sets_match_restatement(seeded_runs, name):
    """Minimiser, robust cost, cost shares, RMS, H_full and weights against the restatement on the seeded sets (6-16 images, planted b and
    kappa, two of the four contaminated; default options: 0.3 px, 0.01 m, scales 3 and 5, Kannala-Brandt's k4, k5 held), from a start
    camera 1 % off in the focal lengths.  Measured here, worst of both cameras: the
    shared parameters 2.08e-6 of their own sigma, the largest pose gap 1.98e-8 (T_cl 1.41e-8), the relative gap of the final cost
    3.48e-14 and of the cost shares 1.19e-14, the RMS 5.98e-9, H_full against the weighted dense Schur complement at the restatement's
    minimiser 1.83e-8 and 1.90e-15 at the answer's own point, the weights 2.71e-7 and 9.98e-13.  Asserted one decade above, never above
    the gates.  Iterations: 13-18 (radtan), 20-25 (kb)."""
    e = seeded_runs[name]
    worst = {}
    for k, c in enumerate(e["cmp"]):
        sm = e["s"]["summaries"][k]
        assert sm.termination in (1, 2, 3), (k, sm.termination)
        got = e["s"]["H_full"][k]
        assert np.array_equal(got, got.T)
        for key in ("shared_sigma", "pose", "tcl", "cost", "cost_self", "parts", "rms", "h", "h_same", "w", "w_same"):
            worst[key] = max(worst.get(key, 0.0), c[key])
        assert sm.final_cost <= sm.initial_cost and abs(e["s"]["cost_parts"][k].sum() - sm.final_cost) <= 1e-14 * sm.final_cost
        held = [j for j in range(16) if j not in c["free"]]
        assert np.all(got[held, :] == 0) and np.all(got[:, held] == 0)
        assert np.all(e["s"]["k"][k][[j - 8 for j in held]] == TC.k_of(e["cams"][k])[[j - 8 for j in held]])
        print("%s problem %d: iterations %d, cost %.6g -> %.6g" % (name, k, sm.num_iterations, sm.initial_cost, sm.final_cost))
        check_bounds(c, (name, k))
    assert np.all(e["s"]["status"] == 1)
    assert np.all((e["s"]["w_corner"] > 0) & (e["s"]["w_corner"] <= 1)) and np.all((e["s"]["w_laser"] > 0) & (e["s"]["w_laser"] <= 1))
    print("%s: worst gaps %s" % (name, {k: "%.2e" % v for k, v in worst.items()}))


@pytest.mark.parametrize("name", CAMS)
def test_reduction_no_laser_is_the_camera_calibration(shim, name):
    """Reduction (a): a problem without a laser point.  T_cl and range come back bit for bit, their rows and columns of H_full are
    zero, and with loss_corner = 0 camera, poses, cost, RMS and the intrinsics' block of H_full are clc_camera_calibrate's host build,
    compared at K19's own bounds (TC.*).  Measured: no gap at all — the corner passes with w = 1 are K19's sums, the rows
    and columns of the held leading block drop out of the compacted system, and the run-time-n Cholesky does chol_solve's operations
    in its order: the same bits."""
    p = cases.problem(name, 77, 8, 144, 0)
    a = cases.arrays([p])
    LC = TC.build_shim(os.path.join(os.path.dirname(shim._name), "libcamcal_shim.so"))
    q0, t0, st = start_poses(shim, p["cam0"], a)
    r0 = np.array([[0.0123, -0.0045]])
    fo = full_options(shim, p["cam0"].model, loss_corner=0.0)
    s = shim_full(shim, [p["cam0"]], a, q0, t0, fo=fo, range0=r0)
    k19 = TC.shim_calibrate(LC, [p["cam0"]], a, q0, t0)
    assert np.array_equal(s["poses_cl"], a["poses_cl0"]) and np.array_equal(s["range"], r0)
    Hf = s["H_full"][0]
    assert np.all(Hf[:8, :] == 0) and np.all(Hf[:, :8] == 0) and s["cost_parts"][0][1] == 0.0
    free = [j for j in range(8) if not (fo.hold_intrinsics_mask >> j) & 1]
    sg = cref_sigmas(k19["H_cam"][0], free)
    gaps = dict(param_sigma=np.max(np.abs(s["k"][0] - k19["k"][0])[free] / sg[free]),
                pose=max(np.abs(np.array([jref.quat_wxyz_to_R(x) for x in s["q"]]) - np.array([jref.quat_wxyz_to_R(x) for x in k19["q"]])).max(),
                         np.abs(s["t"] - k19["t"]).max()),
                cost=abs(s["summaries"][0].final_cost - k19["summaries"][0].final_cost) / k19["summaries"][0].final_cost,
                rms=abs(s["rms_px"][0] - k19["rms_px"][0]) / k19["rms_px"][0],
                hcam=np.linalg.norm(Hf[8:, 8:] - k19["H_cam"][0]) / np.linalg.norm(k19["H_cam"][0]))
    print("%s: no laser vs K19's host build: %s" % (name, {k: "%.2e" % v for k, v in gaps.items()}))
    assert gaps["param_sigma"] <= TC.PARAM_BOUND_SIGMA and gaps["pose"] <= TC.POSE_BOUND and gaps["cost"] <= TC.COST_BOUND
    assert gaps["rms"] <= TC.RMS_BOUND and gaps["hcam"] <= TC.HCAM_BOUND
    # with the loss on the corners the weights are in (0, 1] and T_cl, range still keep their bits
    s2 = shim_full(shim, [p["cam0"]], a, q0, t0, range0=r0)
    assert np.array_equal(s2["poses_cl"], a["poses_cl0"]) and np.array_equal(s2["range"], r0) and np.all((s2["w_corner"] > 0) & (s2["w_corner"] <= 1))


def cref_sigmas(H, free):
    out = np.full(8, np.nan)
    out[free] = np.sqrt(np.diag(np.linalg.inv(H[np.ix_(free, free)])))
    return out


@pytest.mark.parametrize("name", CAMS)
def test_reduction_held_camera_and_poses_is_the_range_refinement(shim, seeded_runs, name):
    """Reduction (b): all intrinsics held, hold_board_poses, both losses 0: T_cl, b, kappa, the cost and the leading 8x8 of H_full
    against K21's host build with hold_board_poses, at K21's bounds (TL.*); no corner is read (the corner arrays are NULL) and the
    trailing rows and columns of H_full are zero.  Reduction (c): the same with the range held at 0 against the oracle's no-loss solve of
    the plane records, as K18's test does, at the parity gates.  Reduction (d): loss = 0 gives weights 1.  Measured: (b) no gap at all (the laser
    passes with w = 1 are K21's sums in K21's order), (c) poses 5.09e-8, cost 5.25e-15 relative."""
    e = seeded_runs[name]
    LL = TL.build_shim(os.path.join(os.path.dirname(shim._name), "liblaserrange_shim.so"))
    fo = full_options(shim, e["cams"][0].model, hold_intrinsics_mask=0xFF, hold_board_poses=1, loss_corner=0.0, loss_laser=0.0)
    s = shim_full(shim, e["cams"], e["a"], e["q0"], e["t0"], fo=fo, corners=False)
    k21 = TL.shim_range(LL, None, e["a"], e["q0"], e["t0"], ro=TL.shim_range_options(LL, None, hold_board_poses=1), corners=False)
    assert np.array_equal(s["q"], e["q0"]) and np.array_equal(s["t"], e["t0"]) and np.all(s["status"] == 1)
    assert np.all(s["w_laser"] == 1.0) and np.all(s["w_corner"] == -7.0)  # (d); no corner weight is written without the corners
    worst = dict(pose=0.0, range_sigma=0.0, cost=0.0, h=0.0)
    for k in range(len(e["problems"])):
        A, B = jref.pose7_to_Rt(s["poses_cl"][k]), jref.pose7_to_Rt(k21["poses_cl"][k])
        sg = np.sqrt(np.diag(np.linalg.inv(k21["H_cr"][k])))
        worst["pose"] = max(worst["pose"], np.abs(A[0] - B[0]).max(), np.abs(A[1] - B[1]).max())
        worst["range_sigma"] = max(worst["range_sigma"], np.max(np.abs(s["range"][k] - k21["range"][k]) / sg[6:]))
        worst["cost"] = max(worst["cost"], abs(s["summaries"][k].final_cost - k21["summaries"][k].final_cost) / k21["summaries"][k].final_cost)
        worst["h"] = max(worst["h"], np.linalg.norm(s["H_full"][k][:8, :8] - k21["H_cr"][k]) / np.linalg.norm(k21["H_cr"][k]))
        assert np.all(s["H_full"][k][8:, :] == 0) and np.all(s["H_full"][k][:, 8:] == 0) and s["cost_parts"][k][0] == 0.0
        assert np.all(s["k"][k] == TC.k_of(e["cams"][k])) and np.isnan(s["rms_px"][k])
    print("%s: (b) held camera and board poses vs K21's host build: %s" % (name, {k: "%.2e" % v for k, v in worst.items()}))
    assert worst["pose"] <= TL.POSE_BOUND and worst["range_sigma"] <= TL.RANGE_SIGMA_BOUND and worst["cost"] <= TL.COST_BOUND
    assert worst["h"] <= TL.HCR_BOUND
    fo.hold_range_mask = 3
    s = shim_full(shim, e["cams"], e["a"], e["q0"], e["t0"], fo=fo, corners=False)
    w2 = [0.0, 0.0]
    for k in range(len(e["problems"])):
        rec = TJ.plane_records(e["a"], k, e["q0"], e["t0"], fo.sigma_laser)
        R, t, cost = TJ.oracle_plane_solve(rec, e["a"]["poses_cl0"][k])
        Rm, tm = jref.pose7_to_Rt(s["poses_cl"][k])
        w2[0] = max(w2[0], np.abs(R - Rm).max(), np.abs(t - tm).max())
        w2[1] = max(w2[1], abs(s["summaries"][k].final_cost - cost) / cost)
        assert np.all(s["range"][k] == 0.0)
    print("%s: (c) range held at 0 vs the oracle's no-loss solve: poses %.2e, cost %.2e" % (name, *w2))
    assert w2[0] <= POSE_GATE and w2[1] <= COST_GATE


def test_every_held_parameter_keeps_its_bits(shim, seeded_runs):
    """Every single held intrinsic bit and range bit keeps its bits while the others move, its row and column of H_full are zero, and
    the answer is the restatement's over the remaining columns; hold_extrinsic keeps T_cl's bits while the rest moves; hold_board_poses
    keeps every board pose and H_full is C itself."""
    e = seeded_runs["radtan"]
    a = cases.arrays([e["problems"][0]])
    cams = [e["cams"][0]]
    n = len(a["coff"]) - 1
    q0, t0 = e["q0"][:n], e["t0"][:n]
    r0 = np.array([[0.0123456789, -0.00456789]])
    k0 = TC.k_of(cams[0])
    for bit in range(10):
        kw = dict(hold_intrinsics_mask=1 << bit) if bit < 8 else dict(hold_range_mask=1 << (bit - 8))
        fo = full_options(shim, 1, **kw)
        s = shim_full(shim, cams, a, q0, t0, fo=fo, range0=r0)
        x0 = np.r_[r0[0], k0]
        x1 = np.r_[s["range"][0], s["k"][0]]
        j = bit + 2 if bit < 8 else bit - 8
        assert x1[j] == x0[j] and np.all(np.delete(x1, j) != np.delete(x0, j)), bit
        hj = 8 + bit if bit < 8 else 6 + bit - 8
        assert np.all(s["H_full"][0][hj, :] == 0) and np.all(s["H_full"][0][:, hj] == 0) and np.all(np.diag(s["H_full"][0])[np.arange(16) != hj] > 0)
        if bit in (0, 5, 8, 9):  # (the dense restatement on four of the ten)
            aa = dict(a, range0=r0)
            c = compare_problem(cams[0], aa, 0, s, q0, t0, fo)
            print("held bit %d: %s" % (bit, {k: "%.2e" % c[k] for k in ("shared_sigma", "pose", "cost", "h")}))
            check_bounds(c, bit)
    fo = full_options(shim, 1, hold_extrinsic=1)
    s = shim_full(shim, cams, a, q0, t0, fo=fo)
    assert np.array_equal(s["poses_cl"], a["poses_cl0"]) and np.all(s["range"] != 0) and not np.array_equal(s["q"], q0) and np.all(s["k"][0] != k0)
    assert np.all(s["H_full"][0][:6, :] == 0) and np.all(s["H_full"][0][:, :6] == 0) and np.all(np.diag(s["H_full"][0])[6:] > 0)
    check_bounds(compare_problem(cams[0], a, 0, s, q0, t0, fo), "hold_extrinsic")
    fo = full_options(shim, 1, hold_board_poses=1)
    s = shim_full(shim, cams, a, q0, t0, fo=fo)
    assert np.array_equal(s["q"], q0) and np.array_equal(s["t"], t0) and not np.array_equal(s["poses_cl"], a["poses_cl0"])
    c = compare_problem(cams[0], a, 0, s, q0, t0, fo)
    assert np.all(s["H_full"][0][:8, 8:] == 0.0) and c["h_same"] <= H_SAME_POINT  # C itself: the cross block is exactly zero
    check_bounds(c, "hold_board_poses")


def test_status_keep_failed_problem_and_nan_weights(shim):
    """An image that takes no part (keep == 0, too few corners, a non-finite corner, a zero-range point) keeps its pose and gets NaN
    weights; the problem solves as if it were not there; a problem that fails (a non-finite start range, a non-finite camera) ends
    CLC_FAILURE with everything of the problem untouched, NaN weights, NaN H_full; without the weight arrays the outputs are the same
    bits."""
    name = "radtan"
    p = cases.problem(name, 9, 7, [144, 3, 144, 144, 144, 144, 144], 60, dirty=True)
    p["images"][3][0][5, 1] = np.nan      # a non-finite corner
    p["images"][5][4][17] = 0.0           # the scanner's "no return"
    p2 = cases.problem(name, 10, 2, [3, 2], 10)
    p3 = cases.problem(name, 11, 4, 144, 50)
    p4 = cases.problem(name, 12, 4, 144, 50)
    problems = [p, p2, p3, p4]
    a = cases.arrays(problems)
    a["range0"][2, 0] = np.nan
    cams = [q["cam0"] for q in problems]
    cams[3] = TC.with_k(cams[3], np.r_[np.inf, TC.k_of(cams[3])[1:]])
    keep = np.ones(17, bool); keep[2] = False
    q0, t0 = problem_starts(shim, [dict(q, cam0=q["cam0"]) for q in problems], a)
    s = shim_full(shim, cams, a, q0, t0, keep=keep)
    assert list(s["status"]) == [1, 0, -1, -2, 1, -2, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    assert [s["summaries"][k].termination == 6 for k in range(4)] == [False, True, True, True]
    for i in range(17):
        wc, wl = s["w_corner"][a["coff"][i]:a["coff"][i + 1]], s["w_laser"][a["poff"][i]:a["poff"][i + 1]]
        if i in (0, 4, 6):
            assert np.all((wc > 0) & (wc <= 1)) and np.all((wl > 0) & (wl <= 1)), i
            assert not np.array_equal(s["q"][i], q0[i])
        else:
            assert np.all(np.isnan(wc)) and np.all(np.isnan(wl)), i
            assert np.array_equal(s["q"][i], q0[i]) and np.array_equal(s["t"][i], t0[i])
    for k in (1, 2, 3):
        assert np.array_equal(s["poses_cl"][k], a["poses_cl0"][k]) and np.array_equal(s["range"][k], a["range0"][k], equal_nan=True)
        assert np.array_equal(s["k"][k], TC.k_of(cams[k])) and np.all(np.isnan(s["H_full"][k])) and np.all(np.isnan(s["cost_parts"][k]))
        assert np.isnan(s["rms_px"][k])
    good = [0, 4, 6]
    ag = cases.arrays([dict(p, images=[p["images"][i] for i in good])])
    sg = shim_full(shim, cams[:1], ag, q0[good], t0[good])
    for key in ("poses_cl", "range", "H_full", "k", "cost_parts", "rms_px"):
        assert np.array_equal(sg[key][0], s[key][0]), key
    assert np.array_equal(sg["q"], s["q"][good]) and np.array_equal(sg["t"], s["t"][good])
    s2 = shim_full(shim, cams, a, q0, t0, keep=keep, weights=False)
    for key in ("q", "t", "poses_cl", "range", "k", "H_full", "cost_parts", "rms_px", "status"):
        assert np.array_equal(s2[key], s[key], equal_nan=True), key
    assert np.all(s2["w_corner"] == -7.0) and np.all(s2["w_laser"] == -7.0)
    # a call whose first problem does not start at image 0: the workspace starts at that image
    a5 = dict(a, prob_off=a["prob_off"][2:].copy(), poses_cl0=a["poses_cl0"][2:], range0=np.zeros((2, 2)))
    s5 = shim_full(shim, [problems[2]["cam0"], problems[3]["cam0"]], a5, q0, t0)
    a6 = cases.arrays(problems[2:])
    s6 = shim_full(shim, [problems[2]["cam0"], problems[3]["cam0"]], a6, q0[9:], t0[9:])
    assert np.array_equal(s5["q"][9:], s6["q"]) and np.array_equal(s5["H_full"], s6["H_full"]) and np.all(s5["status"][:9] == -99)
    assert np.array_equal(s5["w_laser"][a["poff"][9]:], s6["w_laser"]) and np.all(s5["w_laser"][:a["poff"][9]] == -7.0)


RECOVERY_SETS, RECOVERY_SEED0 = 8, 600


def recovery_table(shim, name="radtan", n_sets=RECOVERY_SETS, seed0=RECOVERY_SEED0):
    """K21, K22 and K23 on the recovery sets, the camera taken from K19 on the same corners -> rows (|t_cl - truth| in metres after K21,
    K22, K23 with the scale held, K23 at its defaults), the K23 runs with the scale held."""
    tmp = os.path.dirname(shim._name)
    LC, LL, LR = (TC.build_shim(os.path.join(tmp, "libcamcal_shim.so")), TL.build_shim(os.path.join(tmp, "liblaserrange_shim.so")),
                  TR.build_shim(os.path.join(tmp, "libjointrobust_shim.so")))
    rows, runs = [], []
    for p in cases.recovery_sets(name, n_sets, seed0=seed0):
        a = cases.arrays([p])
        q, t, st = start_poses(LC, p["cam0"], a)
        k19 = TC.shim_calibrate(LC, [p["cam0"]], a, q, t)
        cam, q0, t0 = k19["cameras"][0], k19["q"], k19["t"]
        s21 = TL.shim_range(LL, cam, a, q0, t0)
        s22 = TR.shim_robust(LR, cam, a, q0, t0)
        s23 = shim_full(shim, [cam], a, q0, t0, fo=full_options(shim, cam.model, hold_range_mask=2))
        s23d = shim_full(shim, [cam], a, q0, t0)
        rows.append([cases.tcl_distance(s["poses_cl"][0], p["pose_cl_true"]) for s in (s21, s22, s23, s23d)])
        runs.append((p, s23))
    return np.array(rows), runs


def test_recovery_against_the_staged_routes(shim):
    """8 seeded sets of 30 images (144 corners, 100 points) with a planted range error (0.02 m and 0.5 %, K21's figures), 10 % of each
    image's points pulled 0.10-0.30 m towards the scanner and 5 % of its corners moved 3-10 px (K22's contamination), the camera taken
    from K19 on the same corners, which K21 and K22 then take as exact and K23 as its start.  Mean distance of t_cl from the truth
    (radtan): K21 141.38 mm (no loss: the pulled points), K22 26.69 mm (no range terms), K23 with the range scale held 7.52 mm, K23 at
    its defaults 31.42 mm.  Asserted: K23 with the scale held is below half of K21's and of K22's mean, and at its answer every planted
    observation has w < 0.5 and >= 95 % of the others w >= 0.5.
    K23 AT ITS DEFAULTS HAS NO SUCH MARGIN on these data (31.42 mm against K22's 26.69 mm), and the figure is printed, not asserted.
    The cause is a property of the cost, not of the solve (the restatement has the same minimiser to 1e-8): with the intrinsics free,
    the focal length, the boards' depth, the range scale and t_cl trade against each other along one weakly held direction, and the
    pulled points, all on the scanner's side of the board, pull along it through the Cauchy tail (kappa ends near -0.045 and fx 15 px
    low; the laser share of the cost falls by 390 while the corner share rises by 70).  With laser outliers of one sign the scale
    wants holding, which is K21's advice for recordings with little spread of ranges, and these boards stand at 0.8-1.5 m.  On clean
    data of the same sets K23 at its defaults ends 8.2 mm from the truth, 5.4 mm with the scale held."""
    rows, runs = recovery_table(shim)
    for p, s in runs:
        assert s["summaries"][0].termination in (1, 2, 3) and np.all(s["status"] == 1)
        down, frac = cases.separation(s["w_corner"], s["w_laser"], *cases.planted_masks(p))
        assert down and frac >= 0.95, (down, frac)
    print("set  K21  K22  K23 (scale held)  K23 (defaults)   (|t_cl - truth|, mm)")
    for k, r in enumerate(rows):
        print("%3d  %7.2f  %7.2f  %7.2f  %7.2f" % (k, *(1e3 * r)))
    m = rows.mean(0)
    print("mean %7.2f  %7.2f  %7.2f  %7.2f" % tuple(1e3 * m))
    assert m[2] < 0.5 * m[0] and m[2] < 0.5 * m[1]


def test_sanitized_standalone_program(tmp_path):
    """tests/shim/fullcal_sanitize_main.cpp: the per-problem host functions (solve and weights) on the edge shapes, every array of its
    exact size, built with -fsanitize=address,undefined and run as an ordinary process."""
    exe = str(tmp_path / "fullcal_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "shim", "fullcal_sanitize_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "shapes ok" in p.stdout, p.stdout
