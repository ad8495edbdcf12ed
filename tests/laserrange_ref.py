"""Numpy / scipy restatement of K21 (the joint cost of K18 with a range offset b and a range scale kappa of the scanner), written from
the model:
  p'      (1 + kappa + b / |p|) p                                    the measured laser point moved along its ray
  corner  ((R_i X + t_i)_xy / (R_i X + t_i)_z - x_lifted) / sigma_corner
  laser   e3^T R_i^T (R_cl p' + t_cl - t_i) / sigma_laser
  d laser / d b = (u . p / |p|) / sigma_laser,  d laser / d kappa = (u . p) / sigma_laser,  u = R_cl^T R_i e3
The dense Jacobian has the columns [T_cl tangent (6), b, kappa, T_ca,0 tangent (6), ...]; the corner rows are tests/joint_ref.py's,
the laser rows are written out here.  scipy.optimize.least_squares over the moving columns, the dense normal matrix and its
Schur complement onto the leading 8x8.  A problem is joint_ref's dict: lifted, board, pts (the MEASURED points), sc, sl."""
from __future__ import annotations

import numpy as np
from scipy.optimize import least_squares

import joint_ref as jref

NS = 8  # the shared block


def correct(p, b, kappa):
    """p' of the measured points p [N, 3]; NaN where |p| = 0 or p is not finite."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    rho = np.sqrt(np.sum(p * p, axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (1.0 + kappa + b / rho)[:, None] * p
    out[~(np.isfinite(rho) & (rho > 0))] = np.nan
    return out


def residuals(prob, Rs, ts, Rcl, tcl, b, kappa, jac=True):
    """-> r [corner residuals image by image, then laser residuals image by image], J dense [rows, 8 + 6P] or None, n_corner_res"""
    P = len(Rs)
    sl = prob["sl"]
    # the corner rows: joint_ref's (a problem without any corner, the board poses held, has none)
    rc, Jc6 = np.zeros(0), np.zeros((0, 6 + 6 * P))
    if any(len(x) for x in prob["board"]):
        rc, Jc6, _ = jref.residuals(dict(prob, pts=[np.zeros((0, 3))] * P), Rs, ts, Rcl, tcl, jac=jac)
    rl, Jl = [], []
    for i in range(P):
        p = np.asarray(prob["pts"][i], np.float64).reshape(-1, 3)
        pc = correct(p, b, kappa)
        n = Rs[i][:, 2]
        m = (pc @ Rcl.T + tcl - ts[i]) @ Rs[i]  # rows: R_i^T (R_cl p' + t_cl - t_i)
        rl.append(m[:, 2] / sl)
        if jac:
            u = Rcl.T @ n
            J = np.zeros((len(p), NS + 6 * P))
            J[:, 0:3] = n
            J[:, 3:6] = np.cross(pc, u)
            J[:, 6] = (p @ u) / np.sqrt(np.sum(p * p, axis=1))
            J[:, 7] = p @ u
            J[:, NS + 6 * i:NS + 6 * i + 3] = -n
            J[:, NS + 6 * i + 3] = -m[:, 1]
            J[:, NS + 6 * i + 4] = m[:, 0]
            Jl.append(J / sl)
    r = np.concatenate([rc] + rl)
    if not jac:
        return r, None, len(rc)
    Jc = np.zeros((len(rc), NS + 6 * P))
    Jc[:, :6] = Jc6[:, :6]
    Jc[:, NS:] = Jc6[:, 6:]
    return r, np.concatenate([Jc] + Jl), len(rc)


def cost_parts(prob, Rs, ts, Rcl, tcl, b, kappa):
    r, _, ncr = residuals(prob, Rs, ts, Rcl, tcl, b, kappa, jac=False)
    return 0.5 * np.sum(r[:ncr] ** 2), 0.5 * np.sum(r[ncr:] ** 2)


def columns(P, hold_board=False, hold_ext=False, mask=0, no_laser=False):
    """The columns of the dense Jacobian that move."""
    cols = []
    if not no_laser:
        if not hold_ext:
            cols += list(range(6))
        cols += [6 + j for j in range(2) if not (mask >> j) & 1]
    if not hold_board:
        cols += list(range(NS, NS + 6 * P))
    return np.array(cols, dtype=int)


def solve(prob, Rs0, ts0, Rcl0, tcl0, b0, k0, hold_board=False, hold_ext=False, mask=0, rounds=6):
    """scipy least_squares over the moving columns (rotations as R0 Exp(dtheta), the chain rule through the right Jacobian; b and
    kappa additive), tolerances 1e-15; restarted at its own answer until the cost stops falling.  -> Rs, ts, Rcl, tcl, b, kappa, cost"""
    P = len(Rs0)
    no_laser = sum(len(np.asarray(p).reshape(-1, 3)) for p in prob["pts"]) == 0
    cols = columns(P, hold_board, hold_ext, mask, no_laser)
    state = ([R.copy() for R in Rs0], [t.copy() for t in ts0], Rcl0.copy(), tcl0.copy(), float(b0), float(k0))
    if len(cols) == 0:
        return (*state, 0.5 * np.sum(residuals(prob, *state, jac=False)[0] ** 2))

    def unpack(x, base):
        bRs, bts, bRcl, btcl, bb, bk = base
        full = np.zeros(NS + 6 * P)
        full[cols] = x
        Rc, tc = bRcl @ jref.exp_so3(full[3:6]), btcl + full[0:3]
        RR = [bRs[i] @ jref.exp_so3(full[NS + 6 * i + 3:NS + 6 * i + 6]) for i in range(P)]
        tt = [bts[i] + full[NS + 6 * i:NS + 6 * i + 3] for i in range(P)]
        return (RR, tt, Rc, tc, bb + full[6], bk + full[7]), full

    best = None
    for _ in range(rounds):
        base = state

        def fun(x):
            return residuals(prob, *unpack(x, base)[0], jac=False)[0]

        def jac(x):
            s, full = unpack(x, base)
            J = residuals(prob, *s)[1].copy()
            J[:, 3:6] = J[:, 3:6] @ jref.right_jacobian(full[3:6])
            for i in range(P):
                c = NS + 6 * i + 3
                J[:, c:c + 3] = J[:, c:c + 3] @ jref.right_jacobian(full[c:c + 3])
            return J[:, cols]

        sol = least_squares(fun, np.zeros(len(cols)), jac=jac, method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=300)
        state = unpack(sol.x, base)[0]
        cost = 0.5 * np.sum(sol.fun ** 2)
        if best is not None and not cost < best * (1 - 1e-14):
            break
        best = cost
    return (*state, 0.5 * np.sum(residuals(prob, *state, jac=False)[0] ** 2))


def normal_matrix(prob, Rs, ts, Rcl, tcl, b, kappa):
    r, J, _ = residuals(prob, Rs, ts, Rcl, tcl, b, kappa)
    return J.T @ J, J.T @ r


def schur(H):
    """H_cr = C - sum B_i^T A_i^-1 B_i of the dense normal matrix (the shared block first)."""
    C = H[:NS, :NS].copy()
    for k in range((H.shape[0] - NS) // 6):
        sl = slice(NS + 6 * k, NS + 6 * k + 6)
        C -= H[:NS, sl] @ np.linalg.solve(H[sl, sl], H[sl, :NS])
    return C


def free_sigma(Hcr, free):
    """1 sigma of the 8 shared parameters from the inverse of H_cr restricted to the free ones; NaN for a held one."""
    out = np.full(NS, np.nan)
    free = np.asarray(free, dtype=int)
    if len(free):
        cov = np.linalg.inv(Hcr[np.ix_(free, free)])
        out[free] = np.sqrt(np.diag(cov))
    return out
