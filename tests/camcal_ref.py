"""Numpy / scipy restatement of K19 (csrc/clc_camcal.hpp), for 8 + 6P <= ~130 parameters: the residual vector of
  r_ij = (project(cam, R_i X_j + t_i) - u_j) / sigma_px
and its dense analytic Jacobian, columns [intrinsics (8: proj[0..3], dist[0..3]), T_ca,0 (6: dt, dtheta), T_ca,1, ...] with t += dt,
R <- R Exp(dtheta); scipy.optimize.least_squares (method "lm") run in rounds re-linearised about the current poses; the dense
normal matrix and its Schur complement onto the intrinsics; the closed-form focal start from an SVD-based DLT.
A problem is a dict: model, px [list of (n_i, 2) float64 pixels], board [list of (n_i, 2)], sigma."""
from __future__ import annotations

import numpy as np
from scipy.optimize import least_squares

from joint_ref import exp_so3, right_jacobian, skew, quat_wxyz_to_R, R_to_quat_wxyz, plus  # noqa: F401  (re-exported)

PINHOLE, KANNALA_BRANDT = 1, 2
NK = 8


def project(model, k, P, jac=True):
    """Pixels [n, 2] of the camera-frame points P [n, 3] under the intrinsics k [8]; with jac also d px / d P [n, 2, 3] and
    d px / d k [n, 2, 8]."""
    k = np.asarray(k, np.float64)
    P = np.asarray(P, np.float64).reshape(-1, 3)
    n = len(P)
    fx, fy, cx, cy = k[:4]
    dP, dk = np.zeros((n, 2, 3)), np.zeros((n, 2, NK))
    if model == PINHOLE:
        k1, k2, p1, p2 = k[4:]
        z = P[:, 2]
        x, y = P[:, 0] / z, P[:, 1] / z
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 ** 2
        xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * rad + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)
        px = np.stack([fx * xd + cx, fy * yd + cy], 1)
        if not jac:
            return px
        drad = k1 + 2 * k2 * r2  # d rad / d r2
        D = np.zeros((n, 2, 2))  # d (xd, yd) / d (x, y)
        D[:, 0, 0] = rad + 2 * x * x * drad + 2 * p1 * y + 6 * p2 * x
        D[:, 0, 1] = 2 * x * y * drad + 2 * p1 * x + 2 * p2 * y
        D[:, 1, 0] = 2 * x * y * drad + 2 * p2 * y + 2 * p1 * x
        D[:, 1, 1] = rad + 2 * y * y * drad + 2 * p2 * x + 6 * p1 * y
        N = np.zeros((n, 2, 3))  # d (x, y) / d P
        N[:, 0, 0] = 1 / z; N[:, 1, 1] = 1 / z
        N[:, 0, 2] = -x / z; N[:, 1, 2] = -y / z
        dP = np.einsum("a,nab,nbc->nac", np.array([fx, fy]), D, N)
        dk[:, 0, 0] = xd; dk[:, 1, 1] = yd; dk[:, 0, 2] = 1; dk[:, 1, 3] = 1
        dk[:, 0, 4] = fx * x * r2; dk[:, 1, 4] = fy * y * r2
        dk[:, 0, 5] = fx * x * r2 ** 2; dk[:, 1, 5] = fy * y * r2 ** 2
        dk[:, 0, 6] = fx * 2 * x * y; dk[:, 1, 6] = fy * (r2 + 2 * y * y)
        dk[:, 0, 7] = fx * (r2 + 2 * x * x); dk[:, 1, 7] = fy * 2 * x * y
        return px, dP, dk
    nrm = np.linalg.norm(P, axis=1)
    rho = np.hypot(P[:, 0], P[:, 1])
    th = np.arccos(P[:, 2] / nrm)
    ph = np.arctan2(P[:, 1], P[:, 0])
    pw = np.stack([th ** 3, th ** 5, th ** 7, th ** 9], 1)
    r = th + pw @ k[4:]
    px = np.stack([fx * r * np.cos(ph) + cx, fy * r * np.sin(ph) + cy], 1)
    if not jac:
        return px
    dr = 1 + 3 * k[4] * th ** 2 + 5 * k[5] * th ** 4 + 7 * k[6] * th ** 6 + 9 * k[7] * th ** 8
    dth = np.stack([P[:, 0] * P[:, 2] / (nrm ** 2 * rho), P[:, 1] * P[:, 2] / (nrm ** 2 * rho), -rho / nrm ** 2], 1)
    dph = np.stack([-P[:, 1] / rho ** 2, P[:, 0] / rho ** 2, np.zeros(n)], 1)
    c, s = np.cos(ph), np.sin(ph)
    dP[:, 0, :] = fx * ((dr * c)[:, None] * dth - (r * s)[:, None] * dph)
    dP[:, 1, :] = fy * ((dr * s)[:, None] * dth + (r * c)[:, None] * dph)
    dk[:, 0, 0] = r * c; dk[:, 1, 1] = r * s; dk[:, 0, 2] = 1; dk[:, 1, 3] = 1
    dk[:, 0, 4:] = fx * pw * c[:, None]
    dk[:, 1, 4:] = fy * pw * s[:, None]
    return px, dP, dk


def residuals(prob, k, Rs, ts, jac=True):
    """-> r [image by image, (x, y) interleaved], J dense [2 N, 8 + 6 P] or None"""
    P = len(Rs)
    rows, Jrows = [], []
    for i in range(P):
        R, t = Rs[i], ts[i]
        b = np.asarray(prob["board"][i], np.float64)
        X = np.concatenate([b, np.zeros((len(b), 1))], 1)
        Pc = X @ R.T + t
        with np.errstate(all="ignore"):
            out = project(prob["model"], k, Pc, jac)
        px = out[0] if jac else out
        r = (px - prob["px"][i]) / prob["sigma"]
        r[Pc[:, 2] <= 0] = np.inf  # not in front of the camera: an invalid evaluation
        rows.append(r.reshape(-1))
        if jac:
            n = len(b)
            J = np.zeros((n, 2, NK + 6 * P))
            J[:, :, :NK] = out[2]
            J[:, :, NK + 6 * i:NK + 6 * i + 3] = out[1]
            Xx = np.stack([skew(x) for x in X]) if n else np.zeros((0, 3, 3))
            J[:, :, NK + 6 * i + 3:NK + 6 * i + 6] = -np.einsum("nab,bc,ncd->nad", out[1], R, Xx)
            Jrows.append(J.reshape(2 * n, -1) / prob["sigma"])
    r = np.concatenate(rows) if P else np.zeros(0)
    return (r, np.concatenate(Jrows)) if jac else (r, None)


def cost(prob, k, Rs, ts):
    return 0.5 * np.sum(residuals(prob, k, Rs, ts, jac=False)[0] ** 2)


def columns(P, hold_mask=0, hold_board=False):
    """The columns of the dense Jacobian that move."""
    cols = [j for j in range(NK) if not (hold_mask >> j) & 1]
    if not hold_board:
        cols += list(range(NK, NK + 6 * P))
    return np.array(cols, dtype=int)


def solve(prob, k0, Rs0, ts0, hold_mask=0, hold_board=False, rounds=6):
    """scipy least_squares (method "lm", Jacobian-scaled) over x = [intrinsics offsets, the stacked pose tangents at the round's start]
    (R = R0 Exp(dtheta), exact chain rule through the right Jacobian), tolerances 1e-15; restarted at its own answer until the cost
    stops falling.  Fewer residuals than parameters: "trf".  -> k, Rs, ts, cost"""
    P = len(Rs0)
    cols = columns(P, hold_mask, hold_board)
    k, Rs, ts = np.array(k0, np.float64), [R.copy() for R in Rs0], [t.copy() for t in ts0]
    m = 2 * sum(len(b) for b in prob["board"])

    def unpack(x, base):
        bk, bRs, bts = base
        full = np.zeros(NK + 6 * P)
        full[cols] = x
        RR = [bRs[i] @ exp_so3(full[NK + 6 * i + 3:NK + 6 * i + 6]) for i in range(P)]
        tt = [bts[i] + full[NK + 6 * i:NK + 6 * i + 3] for i in range(P)]
        return bk + full[:NK], RR, tt, full

    best = None
    for _ in range(rounds):
        base = (k, Rs, ts)

        def fun(x):
            kk, RR, tt, _ = unpack(x, base)
            return residuals(prob, kk, RR, tt, jac=False)[0]

        def jac(x):
            kk, RR, tt, full = unpack(x, base)
            J = residuals(prob, kk, RR, tt)[1].copy()
            for i in range(P):
                s = slice(NK + 6 * i + 3, NK + 6 * i + 6)
                J[:, s] = J[:, s] @ right_jacobian(full[s])
            return J[:, cols]

        sol = least_squares(fun, np.zeros(len(cols)), jac=jac, method="lm" if m >= len(cols) else "trf", x_scale="jac", ftol=1e-15,
                            xtol=1e-15, gtol=1e-15, max_nfev=400)
        k, Rs, ts, _ = unpack(sol.x, base)
        c = 0.5 * np.sum(sol.fun ** 2)
        if best is not None and not c < best * (1 - 1e-14):
            break
        best = c
    return k, Rs, ts, cost(prob, k, Rs, ts)


def normal_matrix(prob, k, Rs, ts):
    r, J = residuals(prob, k, Rs, ts)
    return J.T @ J, J.T @ r


def schur(H, hold_mask=0, hold_board=False):
    """H_cam = C - sum B_i^T A_i^-1 B_i of the dense normal matrix (the intrinsics' block first), rows and columns of held intrinsics
    zero; C itself with the board poses held."""
    C = H[:NK, :NK].copy()
    if not hold_board:
        for i in range((H.shape[0] - NK) // 6):
            s = slice(NK + 6 * i, NK + 6 * i + 6)
            C -= H[:NK, s] @ np.linalg.solve(H[s, s], H[s, :NK])
    for j in range(NK):
        if (hold_mask >> j) & 1:
            C[j, :] = 0.0
            C[:, j] = 0.0
    return C


def sigmas(H_cam, hold_mask=0):
    """1 sigma of the free intrinsics from inv(H_cam restricted to the free set); NaN for a held one."""
    free = [j for j in range(NK) if not (hold_mask >> j) & 1]
    out = np.full(NK, np.nan)
    if free:
        out[free] = np.sqrt(np.diag(np.linalg.inv(np.asarray(H_cam)[np.ix_(free, free)])))
    return out


def homography(px, board):
    """board (X, Y, 1) -> px by the Hartley-normalized DLT (SVD), unit Frobenius norm; None where rank-deficient."""
    px, board = np.asarray(px, np.float64), np.asarray(board, np.float64)

    def norm(p):
        c = p.mean(0)
        s = np.sqrt(2.0 / np.mean(np.sum((p - c) ** 2, 1)))
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])

    Ti, Tb = norm(px), norm(board)
    x = np.c_[px, np.ones(len(px))] @ Ti.T
    X = np.c_[board, np.ones(len(board))] @ Tb.T
    A = []
    for (u, v, _), Xh in zip(x, X):
        A.append(np.r_[Xh, np.zeros(3), -u * Xh])
        A.append(np.r_[np.zeros(3), Xh, -v * Xh])
    _, s, Vt = np.linalg.svd(np.array(A))
    if not s[7] ** 2 > 1e-10 * s[0] ** 2:
        return None
    H = np.linalg.inv(Ti) @ Vt[8].reshape(3, 3) @ Tb
    return H / np.linalg.norm(H)


def guess(width, height, px_list, board_list):
    """The closed-form start: (f, n_used), f None when it does not exist."""
    c = np.array([width / 2.0, height / 2.0])
    sab = saa = 0.0
    used = 0
    for px, b in zip(px_list, board_list):
        if len(px) < 4 or not (np.isfinite(px).all() and np.isfinite(b).all()):
            continue
        H = homography(np.asarray(px, np.float64) - c, b)
        if H is None:
            continue
        h1, h2 = H[:, 0], H[:, 1]
        a1, b1 = h1[0] * h2[0] + h1[1] * h2[1], h1[2] * h2[2]
        a2, b2 = (h1[0] ** 2 + h1[1] ** 2) - (h2[0] ** 2 + h2[1] ** 2), h1[2] ** 2 - h2[2] ** 2
        sab += a1 * b1 + a2 * b2
        saa += a1 * a1 + a2 * a2
        used += 1
    if used < 2:
        return None, used
    u = -sab / saa
    return (1.0 / np.sqrt(u) if np.isfinite(u) and u > 0 else None), used
