"""Numpy / scipy restatement of K23 (csrc/clc_fullcal.hpp), written from its definitions on the rows of the earlier restatements:
  corner  (project(cam, R_i X + t_i) - u) / sigma_px                      camcal_ref.residuals (pixels, no lift)
  laser   e3^T R_i^T (R_cl p' + t_cl - t_i) / sigma_laser, p' = (1 + kappa + b / |p|) p      laserrange_ref.residuals' laser rows
  cost = 1/2 sum rho_lc(|e_j|^2) + 1/2 sum rho_ll(r_k^2),  rho_a(z) = a^2 log1p(z / a^2), a = 0: z        jointrobust_ref.rho
The dense Jacobian has the columns [T_cl tangent (6), b, kappa, intrinsics (8: proj[0..3], dist[0..3]), T_ca,0 tangent (6), ...].  The
weights w = rho'(z), the Gauss-Newton normal matrix J^T W J and gradient J^T W r, its Schur complement onto the leading 16x16, and
an independent minimiser: scipy least_squares on the smooth equivalent residuals r~ = r sqrt(rho(z) / z), re-linearised in rounds.
A state X is (Rs, ts, Rcl, tcl, b, kappa, k); a problem is a dict: model, px, board [lists per image], pts, spx, sl, lc, ll."""
from __future__ import annotations

import numpy as np
from scipy.optimize import least_squares

import camcal_ref as cref
import joint_ref as jref
import laserrange_ref as lref
from jointrobust_ref import rho, rho_prime

NS = 16  # the shared block
NX = 8   # its leading part [T_cl, b, kappa]


def residuals(prob, Rs, ts, Rcl, tcl, b, kappa, k, jac=True):
    """-> r [corner residuals image by image (x, y interleaved), then laser residuals image by image], J dense [rows, 16 + 6P] or None,
    n_corner_res"""
    P = len(Rs)
    rc, Jc = np.zeros(0), np.zeros((0, 8 + 6 * P))
    if any(len(x) for x in prob["board"]):
        rc, Jc = cref.residuals(dict(model=prob["model"], px=prob["px"], board=prob["board"], sigma=prob["spx"]), k, Rs, ts, jac=jac)
    empty = [np.zeros((0, 2))] * P
    rl, Jl, _ = lref.residuals(dict(lifted=empty, board=empty, pts=prob["pts"], sc=1.0, sl=prob["sl"]), Rs, ts, Rcl, tcl, b, kappa, jac=jac)
    r = np.concatenate([rc, rl])
    if not jac:
        return r, None, len(rc)
    J = np.zeros((len(r), NS + 6 * P))
    J[:len(rc), NX:NS] = Jc[:, :8]
    J[:len(rc), NS:] = Jc[:, 8:]
    J[len(rc):, :NX] = Jl[:, :NX]
    J[len(rc):, NS:] = Jl[:, NX:]
    return r, J, len(rc)


def block_z(prob, *X):
    """-> z per corner, z per laser point, r, ncr"""
    r, _, ncr = residuals(prob, *X, jac=False)
    rc = r[:ncr].reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        return rc[:, 0] ** 2 + rc[:, 1] ** 2, r[ncr:] ** 2, r, ncr


def cost_parts(prob, *X):
    zc, zl, _, _ = block_z(prob, *X)
    return 0.5 * np.sum(rho(zc, prob["lc"])), 0.5 * np.sum(rho(zl, prob["ll"]))


def weights(prob, *X):
    """-> w per corner, w per laser point (image by image, in the problem's order)."""
    zc, zl, _, _ = block_z(prob, *X)
    return rho_prime(zc, prob["lc"]), rho_prime(zl, prob["ll"])


def row_weights(prob, *X):
    wc, wl = weights(prob, *X)
    return np.concatenate([np.repeat(wc, 2), wl])


def normal_matrix(prob, *X):
    """-> J^T W J, J^T W r"""
    r, J, _ = residuals(prob, *X)
    w = row_weights(prob, *X)
    return J.T @ (J * w[:, None]), J.T @ (w * r)


def _factor_terms(z, a):
    """f = sqrt(rho / z) and df/dz = (rho' - f^2) / (2 f z); f = 1, df/dz -> 0 term at z = 0."""
    f, g = np.ones_like(z), np.zeros_like(z)
    nz = z > 0
    f[nz] = np.sqrt(rho(z[nz], a) / z[nz])
    g[nz] = (rho_prime(z[nz], a) - f[nz] ** 2) / (2.0 * f[nz] * z[nz])
    return f, g


def smooth_residuals(prob, *X):
    """r~ = r sqrt(rho(z) / z) per block: 1/2 |r~|^2 = the cost."""
    zc, zl, r, ncr = block_z(prob, *X)
    return r * np.concatenate([np.repeat(_factor_terms(zc, prob["lc"])[0], 2), _factor_terms(zl, prob["ll"])[0]])


def smooth_jacobian(prob, *X):
    zc, zl, r, ncr = block_z(prob, *X)
    _, J, _ = residuals(prob, *X)
    out = np.empty_like(J)
    f, g = _factor_terms(zc, prob["lc"])
    Jc, rc = J[:ncr].reshape(-1, 2, J.shape[1]), r[:ncr].reshape(-1, 2)
    dz = 2.0 * np.einsum("nk,nkc->nc", rc, Jc)
    out[:ncr] = (f[:, None, None] * Jc + rc[:, :, None] * (g[:, None] * dz)[:, None, :]).reshape(ncr, -1)
    f, g = _factor_terms(zl, prob["ll"])
    Jl, rl = J[ncr:], r[ncr:]
    out[ncr:] = f[:, None] * Jl + (rl * g)[:, None] * (2.0 * rl[:, None] * Jl)
    return out


def free_shared(hold_ext=False, range_mask=0, intr_mask=0, no_laser=False):
    """The free members of the shared block."""
    cols = []
    if not no_laser:
        if not hold_ext:
            cols += list(range(6))
        cols += [6 + j for j in range(2) if not (range_mask >> j) & 1]
    cols += [NX + j for j in range(8) if not (intr_mask >> j) & 1]
    return cols


def columns(P, hold_board=False, **kw):
    """The columns of the dense Jacobian that move."""
    cols = free_shared(**kw)
    if not hold_board:
        cols += list(range(NS, NS + 6 * P))
    return np.array(cols, dtype=int)


def no_laser(prob):
    return sum(len(np.asarray(p).reshape(-1, 3)) for p in prob["pts"]) == 0


def solve(prob, X0, hold_board=False, hold_ext=False, range_mask=0, intr_mask=0, rounds=6):
    """scipy least_squares on the smooth equivalent residuals over the moving columns (rotations as R0 Exp(dtheta), the chain rule
    through the right Jacobian; b, kappa and the intrinsics additive), tolerances 1e-15; re-linearised at its own answer until the
    cost stops falling.  -> X, cost"""
    P = len(X0[0])
    cols = columns(P, hold_board, hold_ext=hold_ext, range_mask=range_mask, intr_mask=intr_mask, no_laser=no_laser(prob))
    state = ([R.copy() for R in X0[0]], [t.copy() for t in X0[1]], X0[2].copy(), X0[3].copy(), float(X0[4]), float(X0[5]), np.array(X0[6], np.float64))
    if len(cols) == 0:
        return state, float(sum(cost_parts(prob, *state)))

    def unpack(x, base):
        bRs, bts, bRcl, btcl, bb, bk, bi = base
        full = np.zeros(NS + 6 * P)
        full[cols] = x
        Rc, tc = bRcl @ jref.exp_so3(full[3:6]), btcl + full[0:3]
        RR = [bRs[i] @ jref.exp_so3(full[NS + 6 * i + 3:NS + 6 * i + 6]) for i in range(P)]
        tt = [bts[i] + full[NS + 6 * i:NS + 6 * i + 3] for i in range(P)]
        return (RR, tt, Rc, tc, bb + full[6], bk + full[7], bi + full[NX:NS]), full

    best = None
    for _ in range(rounds):
        base = state

        def fun(x):
            with np.errstate(all="ignore"):
                return smooth_residuals(prob, *unpack(x, base)[0])

        def jac(x):
            s, full = unpack(x, base)
            J = smooth_jacobian(prob, *s)
            J[:, 3:6] = J[:, 3:6] @ jref.right_jacobian(full[3:6])
            for i in range(P):
                c = NS + 6 * i + 3
                J[:, c:c + 3] = J[:, c:c + 3] @ jref.right_jacobian(full[c:c + 3])
            return J[:, cols]

        sol = least_squares(fun, np.zeros(len(cols)), jac=jac, method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=400)
        state = unpack(sol.x, base)[0]
        c = 0.5 * np.sum(sol.fun ** 2)
        if best is not None and not c < best * (1 - 1e-14):
            break
        best = c
    return state, float(sum(cost_parts(prob, *state)))


def schur(H, free, hold_board=False):
    """H_full = C - sum B_i^T A_i^-1 B_i of the dense normal matrix (the shared block first), rows and columns of the parameters outside
    `free` zero; C itself with the board poses held."""
    C = H[:NS, :NS].copy()
    if not hold_board:
        for i in range((H.shape[0] - NS) // 6):
            s = slice(NS + 6 * i, NS + 6 * i + 6)
            C -= H[:NS, s] @ np.linalg.solve(H[s, s], H[s, :NS])
    out = np.zeros_like(C)
    free = np.asarray(free, dtype=int)
    out[np.ix_(free, free)] = C[np.ix_(free, free)]
    return out


def free_sigma(H_full, free):
    """1 sigma of the 16 shared parameters from the inverse of H_full restricted to the free ones; NaN for a held one."""
    out = np.full(NS, np.nan)
    free = np.asarray(free, dtype=int)
    if len(free):
        out[free] = np.sqrt(np.diag(np.linalg.inv(np.asarray(H_full)[np.ix_(free, free)])))
    return out
