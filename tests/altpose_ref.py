"""Test-side restatement (numpy / scipy) of K17, the planar fit's second minimum (include/clc.h, clc_board_poses_alternate): steps 1-5
for one image with the fit by campose_ref.pnp_lsq, and brute_minima(), a search for every minimum of an image from 32 tilted
starts that knows nothing of the mirror construction."""
from __future__ import annotations

import numpy as np

import campose_ref as cref

NONE, SAME, DISTINCT = 0, 1, 2


def residual_cost(lifted, board, R, t):
    """1/2 sum |r|^2 of the K = I reprojection error; inf when a corner lies behind the camera.  -> (cost, all in front)"""
    X = np.concatenate([np.asarray(board, np.float64).reshape(-1, 2), np.zeros((len(board), 1))], 1)
    P = X @ R.T + t
    front = bool(np.all(P[:, 2] > 0))
    r = P[:, :2] / P[:, 2:3] - np.asarray(lifted, np.float64).reshape(-1, 2)
    c = 0.5 * float(np.sum(r * r))
    return (c if front else np.inf), front


def rotation_angle(A, B):
    D = A.T @ B
    v = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.linalg.norm(v), np.trace(D) - 1.0))


def normal_angle(A, B):
    a, b = A[:, 2], B[:, 2]
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))


def mirror_start(R, t, Xbar):
    """Step 2 -> (R', t') or None."""
    X3 = np.array([Xbar[0], Xbar[1], 0.0])
    c = R @ X3 + t
    nn = np.linalg.norm(c)
    if not (np.isfinite(nn) and nn > 0):
        return None
    s = c / nn
    Rm = (np.eye(3) - 2.0 * np.outer(s, s)) @ R @ np.diag([1.0, 1.0, -1.0])
    tm = c - Rm @ X3
    if not (np.all(np.isfinite(Rm)) and np.all(np.isfinite(tm))):
        return None
    return Rm, tm


def none():
    nan = float("nan")
    return dict(kind=NONE, ambiguous=0, better=0, R=np.eye(3), t=np.zeros(3), rms=nan, cost_in=nan, cost_alt=nan, ratio=nan,
                rot_angle=nan, normal_angle=nan)


def alt_pose(lifted, board, mask, R_in, t_in, status_in, same_angle=0.01, ratio_gate=2.0):
    """lifted [n, 2]: the float32-rounded lift as float64; board [n, 2]; mask [n] bool or None; (R_in, t_in, status_in): the earlier
    call's pose.  -> dict."""
    lifted = np.asarray(lifted, np.float64).reshape(-1, 2)
    board = np.asarray(board, np.float64).reshape(-1, 2)
    if status_in != 1:
        return none()
    if mask is not None:
        m = np.asarray(mask, bool)
        lifted, board = lifted[m], board[m]
    if len(lifted) < 4 or not (np.all(np.isfinite(lifted)) and np.all(np.isfinite(board))):
        return none()
    start = mirror_start(R_in, t_in, board.mean(0))
    if start is None:
        return none()
    if not residual_cost(lifted, board, *start)[1]:  # the fit's first evaluation is invalid: a failure at the start
        return none()
    R, t, _ = cref.pnp_lsq(lifted, board, *start)
    for _ in range(5):  # restarted at its own answer while that still lowers the cost: scipy's stopping in a shallow minimum leaves
        R1, t1, _ = cref.pnp_lsq(lifted, board, R, t)  # the first answer ~1e-4 rad off
        better = residual_cost(lifted, board, R1, t1)[0] < residual_cost(lifted, board, R, t)[0] * (1 - 1e-14)
        R, t = R1, t1
        if not better:
            break
    cost_alt, front = residual_cost(lifted, board, R, t)
    if not (front and np.isfinite(cost_alt) and np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        return none()
    cost_in, _ = residual_cost(lifted, board, R_in, t_in)
    ratio = cost_alt / cost_in if (cost_in != 0 and np.isfinite(cost_in) and np.isfinite(cost_alt)) else float("nan")
    ra, na = rotation_angle(R_in, R), normal_angle(R_in, R)
    distinct = not (ra < same_angle)
    return dict(kind=DISTINCT if distinct else SAME, ambiguous=int(distinct and ratio < ratio_gate), better=int(distinct and cost_alt < cost_in),
                R=R, t=t, R_in=np.asarray(R_in, np.float64), rms=float(np.sqrt(2.0 * cost_alt / len(lifted))), cost_in=cost_in, cost_alt=cost_alt,
                ratio=ratio, rot_angle=ra, normal_angle=na)


def rot_axis(a, ang):
    return cref.rotvec_to_R(np.asarray(a, np.float64) / np.linalg.norm(a) * ang)


def brute_minima(lifted, board, R, t, tilts_deg=(10.0, 25.0, 40.0, 60.0), n_az=8, apart_deg=0.5):
    """Every minimum of the image's reprojection cost reachable from 32 starts: the board turned to face the camera along the line of
    sight to its centroid (the minimal rotation of R that does it, so the in-plane orientation stays), then tilted by each of
    tilts_deg about 8 axes perpendicular to the line of sight, the centroid staying where (R, t) puts it.  Kept: minima with every
    corner in front, more than apart_deg apart.  -> [(R, t, cost)] by ascending cost."""
    lifted = np.asarray(lifted, np.float64).reshape(-1, 2)
    board = np.asarray(board, np.float64).reshape(-1, 2)
    X3 = np.array([*board.mean(0), 0.0])
    c = R @ X3 + t
    s = c / np.linalg.norm(c)
    n = R[:, 2]
    target = s if n @ s >= 0 else -s
    ax = np.cross(n, target)
    Rf = R if np.linalg.norm(ax) < 1e-12 else rot_axis(ax, np.arctan2(np.linalg.norm(ax), n @ target)) @ R
    e1 = np.cross(s, [1.0, 0.0, 0.0] if abs(s[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(s, e1)
    found = []
    for tilt in tilts_deg:
        for k in range(n_az):
            az = 2 * np.pi * k / n_az
            R0 = rot_axis(np.cos(az) * e1 + np.sin(az) * e2, np.deg2rad(tilt)) @ Rf
            t0 = c - R0 @ X3
            if not residual_cost(lifted, board, R0, t0)[1]:
                continue
            R1, t1, _ = cref.pnp_lsq(lifted, board, R0, t0)
            cost, front = residual_cost(lifted, board, R1, t1)
            if not front:
                continue
            if all(rotation_angle(R1, f[0]) > np.deg2rad(apart_deg) for f in found):
                found.append((R1, t1, cost))
            else:  # keep the best-converged member of a cluster
                for i, f in enumerate(found):
                    if rotation_angle(R1, f[0]) <= np.deg2rad(apart_deg) and cost < f[2]:
                        found[i] = (R1, t1, cost)
    return sorted(found, key=lambda f: f[2])
