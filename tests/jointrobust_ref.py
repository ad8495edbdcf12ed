"""Numpy / scipy restatement of K22 (csrc/clc_jointrobust.hpp), written from its definitions on joint_ref.residuals: the joint cost
of K18 under a Cauchy loss per corner (on the squared norm of its residual 2-vector) and per laser point,

  cost = 1/2 sum rho_a(z),   rho_a(z) = a^2 log1p(z / a^2),   rho_a'(z) = 1 / (1 + z / a^2),   a = 0: rho(z) = z

with a = lc for corners and a = ll for laser points, both in units of sigma.  The weights w = rho'(z); the Gauss-Newton normal
matrix J^T W J and gradient J^T W r (Ceres' corrector for rho'' <= 0: rows and residual scaled by sqrt(rho')) and its Schur
complement; an independent minimiser: scipy least_squares on the smooth equivalent residuals r~ = r sqrt(rho(z) / z) per block
(r~ = r at z = 0), for which 1/2 sum |r~|^2 is the cost exactly.  A problem is joint_ref's dict plus lc, ll."""
from __future__ import annotations

import numpy as np
from scipy.optimize import least_squares

import joint_ref as ref


def rho(z, a):
    z = np.asarray(z, np.float64)
    if a == 0:
        return z.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        return a * a * np.log1p(z / (a * a))


def rho_prime(z, a):
    z = np.asarray(z, np.float64)
    if a == 0:
        return np.ones_like(z)
    return 1.0 / (1.0 + z / (a * a))


def block_z(prob, Rs, ts, Rcl, tcl):
    """-> z per corner [ncr / 2], z per laser point, r, ncr"""
    r, _, ncr = ref.residuals(prob, Rs, ts, Rcl, tcl, jac=False)
    rc = r[:ncr].reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        return rc[:, 0] ** 2 + rc[:, 1] ** 2, r[ncr:] ** 2, r, ncr


def cost_parts(prob, Rs, ts, Rcl, tcl):
    zc, zl, _, _ = block_z(prob, Rs, ts, Rcl, tcl)
    return 0.5 * np.sum(rho(zc, prob["lc"])), 0.5 * np.sum(rho(zl, prob["ll"]))


def weights(prob, Rs, ts, Rcl, tcl):
    """-> w per corner, w per laser point (image by image, in the problem's order)."""
    zc, zl, _, _ = block_z(prob, Rs, ts, Rcl, tcl)
    return rho_prime(zc, prob["lc"]), rho_prime(zl, prob["ll"])


def row_weights(prob, Rs, ts, Rcl, tcl):
    """w of every row of joint_ref.residuals (a corner's two rows share its weight)."""
    wc, wl = weights(prob, Rs, ts, Rcl, tcl)
    return np.concatenate([np.repeat(wc, 2), wl])


def normal_matrix(prob, Rs, ts, Rcl, tcl):
    """-> J^T W J, J^T W r (columns as joint_ref: T_cl's block first)."""
    r, J, _ = ref.residuals(prob, Rs, ts, Rcl, tcl)
    w = row_weights(prob, Rs, ts, Rcl, tcl)
    return J.T @ (J * w[:, None]), J.T @ (w * r)


schur = ref.schur


def smooth_residuals(prob, Rs, ts, Rcl, tcl):
    """r~ = r sqrt(rho(z) / z) per block, r~ = r at z = 0: 1/2 |r~|^2 = the cost."""
    zc, zl, r, ncr = block_z(prob, Rs, ts, Rcl, tcl)

    def factor(z, a):
        f = np.ones_like(z)
        nz = z > 0
        f[nz] = np.sqrt(rho(z[nz], a) / z[nz])
        return f

    return r * np.concatenate([np.repeat(factor(zc, prob["lc"]), 2), factor(zl, prob["ll"])])


def smooth_jacobian(prob, Rs, ts, Rcl, tcl):
    """d r~ / d x = f J + r (df/dz) (dz/dx) per block, f = sqrt(rho / z): df/dz = (rho' - f^2) / (2 f z); at z = 0, f = 1 and the second
    term vanishes (f = 1 - z / (4 a^2) + ..., r = 0)."""
    zc, zl, r, ncr = block_z(prob, Rs, ts, Rcl, tcl)
    _, J, _ = ref.residuals(prob, Rs, ts, Rcl, tcl)
    out = np.empty_like(J)

    def terms(z, a):
        f, g = np.ones_like(z), np.zeros_like(z)
        nz = z > 0
        f[nz] = np.sqrt(rho(z[nz], a) / z[nz])
        g[nz] = (rho_prime(z[nz], a) - f[nz] ** 2) / (2.0 * f[nz] * z[nz])
        return f, g

    f, g = terms(zc, prob["lc"])
    Jc, rc = J[:ncr].reshape(-1, 2, J.shape[1]), r[:ncr].reshape(-1, 2)
    dz = 2.0 * np.einsum("nk,nkc->nc", rc, Jc)
    out[:ncr] = (f[:, None, None] * Jc + rc[:, :, None] * (g[:, None] * dz)[:, None, :]).reshape(ncr, -1)
    f, g = terms(zl, prob["ll"])
    Jl, rl = J[ncr:], r[ncr:]
    out[ncr:] = f[:, None] * Jl + (rl * g)[:, None] * (2.0 * rl[:, None] * Jl)
    return out


def solve(prob, Rs0, ts0, Rcl0, tcl0, hold_board=False, hold_ext=False, rounds=6):
    """joint_ref.solve on the smooth equivalent residuals: scipy least_squares over the stacked tangents at the start, tolerances
    1e-15; restarted at its own answer until the cost stops falling.  -> Rs, ts, Rcl, tcl, cost"""
    P = len(Rs0)
    no_laser = sum(len(np.asarray(p).reshape(-1, 3)) for p in prob["pts"]) == 0
    cols = ref.columns(P, hold_board, hold_ext, no_laser)
    Rs, ts, Rcl, tcl = [R.copy() for R in Rs0], [t.copy() for t in ts0], Rcl0.copy(), tcl0.copy()

    def unpack(x, base):
        bRs, bts, bRcl, btcl = base
        full = np.zeros(6 + 6 * P)
        full[cols] = x
        Rc, tc = bRcl @ ref.exp_so3(full[3:6]), btcl + full[0:3]
        RR = [bRs[i] @ ref.exp_so3(full[9 + 6 * i:12 + 6 * i]) for i in range(P)]
        tt = [bts[i] + full[6 + 6 * i:9 + 6 * i] for i in range(P)]
        return RR, tt, Rc, tc, full

    best = None
    for _ in range(rounds):
        base = (Rs, ts, Rcl, tcl)

        def fun(x):
            RR, tt, Rc, tc, _ = unpack(x, base)
            return smooth_residuals(prob, RR, tt, Rc, tc)

        def jac(x):
            RR, tt, Rc, tc, full = unpack(x, base)
            J = smooth_jacobian(prob, RR, tt, Rc, tc)
            for k in range(P + 1):
                J[:, 6 * k + 3:6 * k + 6] = J[:, 6 * k + 3:6 * k + 6] @ ref.right_jacobian(full[6 * k + 3:6 * k + 6])
            return J[:, cols]

        if len(cols) == 0:
            break
        sol = least_squares(fun, np.zeros(len(cols)), jac=jac, method="trf", x_scale="jac", ftol=1e-15, xtol=1e-15, gtol=1e-15,
                            max_nfev=300)
        Rs, ts, Rcl, tcl, _ = unpack(sol.x, base)
        cost = 0.5 * np.sum(sol.fun ** 2)
        if best is not None and not cost < best * (1 - 1e-14):
            break
        best = cost
    return Rs, ts, Rcl, tcl, float(sum(cost_parts(prob, Rs, ts, Rcl, tcl)))
