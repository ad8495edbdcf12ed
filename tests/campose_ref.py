"""Test-side restatements (numpy) of the camera models and board geometry of the reference's camera side:
camodocal PinholeCamera / EquidistantCamera (liftProjective, spaceToPlane) and CamPoseEst::EstimatePose as a least-squares problem.
The Kannala-Brandt lift takes the roots of the odd polynomial with np.roots — the companion-matrix eigenvalues, the reference's own
method (EquidistantCamera.cc:632-733) — and keeps the smallest real one >= -1e-10."""
from __future__ import annotations

import numpy as np

PINHOLE, KANNALA_BRANDT = 1, 2


def lift(model, proj, dist, px):
    """liftProjective of pixels px [n, 2] (float32 values) -> x/z, y/z [n, 2] (float64, unrounded)."""
    px = np.asarray(px, dtype=np.float64).reshape(-1, 2)
    f0, f1, c0, c1 = proj
    ik11, ik13, ik22, ik23 = 1.0 / f0, -c0 / f0, 1.0 / f1, -c1 / f1  # PinholeCamera.cc:208-211
    mx = ik11 * px[:, 0] + ik13
    my = ik22 * px[:, 1] + ik23
    if model == PINHOLE:
        if all(d == 0.0 for d in dist):
            return np.stack([mx, my], 1)
        mxu, myu = mx.copy(), my.copy()
        du = distortion(dist, mx, my)
        mxu, myu = mx - du[0], my - du[1]
        for _ in range(1, 8):
            du = distortion(dist, mxu, myu)
            mxu, myu = mx - du[0], my - du[1]
        return np.stack([mxu / 1.0, myu / 1.0], 1)
    out = np.empty((len(px), 2))
    for i in range(len(px)):
        pn = np.sqrt(mx[i] * mx[i] + my[i] * my[i])
        phi = 0.0 if pn < 1e-10 else np.arctan2(my[i], mx[i])
        th = kb_theta_roots(dist, pn)
        st, ct = np.sin(th), np.cos(th)
        out[i] = (st * np.cos(phi)) / ct, (st * np.sin(phi)) / ct
    return out


def distortion(dist, mx, my):
    """PinholeCamera::distortion, :554-571."""
    k1, k2, p1, p2 = dist
    mx2, my2, mxy = mx * mx, my * my, mx * my
    rho2 = mx2 + my2
    rad = k1 * rho2 + k2 * rho2 * rho2
    return (mx * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2),
            my * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2))


def kb_theta_roots(k, p, polish=True):
    """backprojectSymmetric's theta (:632-733): the degree drops by 2 per zero k, coefficient slots fixed; the smallest real root
    >= -1e-10 (clamped to 0) of the companion matrix, |p| when none.  polish: four Newton steps on the chosen root (they remove the
    eigen-solver's rounding, not the choice)."""
    k2, k3, k4, k5 = k
    npow = 9 - 2 * sum(1 for v in (k5, k4, k3, k2) if v == 0.0)
    coeffs = np.zeros(npow + 1)
    coeffs[0] = -p
    coeffs[1] = 1.0
    for i, v in ((3, k2), (5, k3), (7, k4), (9, k5)):
        if npow >= i:
            coeffs[i] = v
    if npow == 1 or not np.isfinite(p):
        return p
    roots = np.roots(coeffs[::-1])  # highest degree first; leading zeros are dropped
    cand = []
    for r in roots:
        if abs(r.imag) > 1e-10:
            continue
        t = r.real
        if t < -1e-10:
            continue
        cand.append(max(t, 0.0))
    if not cand:
        return p
    th = min(cand)
    if polish and th > 0:
        c = coeffs
        for _ in range(4):
            f = sum(c[j] * th ** j for j in range(len(c)))
            d = sum(j * c[j] * th ** (j - 1) for j in range(1, len(c)))
            if d != 0:
                th = th - f / d
    return th


def project(model, proj, dist, P):
    """spaceToPlane of camera-frame points P [n, 3]."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    f0, f1, c0, c1 = proj
    if model == PINHOLE:
        x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
        if not all(d == 0.0 for d in dist):
            du = distortion(dist, x, y)
            x, y = x + du[0], y + du[1]
        return np.stack([f0 * x + c0, f1 * y + c1], 1)
    nrm = np.sqrt(P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1] + P[:, 2] * P[:, 2])
    th = np.arccos(P[:, 2] / nrm)
    phi = np.arctan2(P[:, 1], P[:, 0])
    k2, k3, k4, k5 = dist
    t = th
    r = t + k2 * t * t * t + k3 * t * t * t * t * t + k4 * t * t * t * t * t * t * t + k5 * t * t * t * t * t * t * t * t * t
    return np.stack([f0 * (r * np.cos(phi)) + c0, f1 * (r * np.sin(phi)) + c1], 1)


def quat_wxyz_to_R(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rotvec_to_R(v):
    th = np.linalg.norm(v)
    if th < 1e-300:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def pnp_lsq(xy_lifted, board_xy, R0, t0):
    """The least-squares minimiser of sum |(R X + t)_xy / (R X + t)_z - x|^2 (scipy, rotation as a right perturbation of R0)."""
    from scipy.optimize import least_squares
    X = np.concatenate([np.asarray(board_xy, np.float64).reshape(-1, 2), np.zeros((len(xy_lifted), 1))], 1)
    x = np.asarray(xy_lifted, np.float64).reshape(-1, 2)

    def res(p):
        R = R0 @ rotvec_to_R(p[3:])
        P = X @ R.T + (t0 + p[:3])
        return (P[:, :2] / P[:, 2:3] - x).ravel()

    sol = least_squares(res, np.zeros(6), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    return R0 @ rotvec_to_R(sol.x[3:]), t0 + sol.x[:3], sol
