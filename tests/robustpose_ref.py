"""Test-side sequential restatement of K16 (robust board poses, include/clc.h): the per-tag homography hypotheses, their scores and the
winner ONE FLOAT AT A TIME in Python floats (IEEE doubles: every product, sum and division rounded on its own, which is what the
kernel's __dmul_rn / __dadd_rn spell), and the fit / re-gate loop with scipy's least squares as the fit (campose_ref.pnp_lsq).
Counts, costs and the winner are meant to be compared for equality; poses to the tolerance between two least-squares solvers."""
from __future__ import annotations

import math

import numpy as np

from campose_ref import lift, pnp_lsq, quat_wxyz_to_R

OK, NO_CONSENSUS = 1, -3


def _div(a, b):
    """IEEE division of Python floats (which raise on a zero divisor)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def square_to_quad(p):
    """S(p), rows in a list of 9, and den = d1 x d2."""
    x0, y0, x1, y1, x2, y2, x3, y3 = p
    sx = ((x0 - x1) + x2) - x3
    sy = ((y0 - y1) + y2) - y3
    d1x = x1 - x2; d1y = y1 - y2; d2x = x3 - x2; d2y = y3 - y2
    den = (d1x * d2y) - (d1y * d2x)
    g = _div((sx * d2y) - (sy * d2x), den)
    h = _div((d1x * sy) - (d1y * sx), den)
    gx1 = g * x1; hx3 = h * x3; gy1 = g * y1; hy3 = h * y3
    return [(x1 - x0) + gx1, (x3 - x0) + hx3, x0, (y1 - y0) + gy1, (y3 - y0) + hy3, y0, g, h, 1.0], den


def hypothesis(quad_lifted, quad_board):
    """H_g = S(lifted quad) adj(S(board quad)) -> (H [9], w0, valid)."""
    Si, den_i = square_to_quad(quad_lifted)
    Sb, den_b = square_to_quad(quad_board)
    a, b, c, d, e, f, g, h, i = Sb
    A = [(e * i) - (f * h), (c * h) - (b * i), (b * f) - (c * e),
         (f * g) - (d * i), (a * i) - (c * g), (c * d) - (a * f),
         (d * h) - (e * g), (b * g) - (a * h), (a * e) - (b * d)]
    valid = math.isfinite(den_i) and math.isfinite(den_b) and den_i != 0.0 and den_b != 0.0
    H = []
    for r in range(3):
        for k in range(3):
            p0 = Si[3 * r] * A[k]; p1 = Si[3 * r + 1] * A[3 + k]; p2 = Si[3 * r + 2] * A[6 + k]
            v = (p0 + p1) + p2
            H.append(v)
            valid = valid and math.isfinite(v)
    w0 = ((H[6] * quad_board[0]) + (H[7] * quad_board[1])) + H[8]
    return H, w0, valid


def score(H, w0, X, Y, x, y, thr2):
    """-> (min(e, thr2), inlier, e)."""
    u = ((H[0] * X) + (H[1] * Y)) + H[2]
    v = ((H[3] * X) + (H[4] * Y)) + H[5]
    w = ((H[6] * X) + (H[7] * Y)) + H[8]
    du = _div(u, w) - x
    dv = _div(v, w) - y
    e = (du * du) + (dv * dv)
    below = math.isfinite(e) and e < thr2
    return (e if below else thr2), (below and (w * w0) > 0.0), e


def consensus(L, B, hyp_threshold):
    """L, B [n, 2] (float32 values) -> dict: counts [G] (-1: invalid group), costs [G], winner (-1: none), runner_up, mask [n] of the
    winner, H of the winner."""
    L = [(float(a), float(b)) for a, b in np.asarray(L).reshape(-1, 2)]
    B = [(float(a), float(b)) for a, b in np.asarray(B).reshape(-1, 2)]
    n = len(L)
    thr2 = hyp_threshold * hyp_threshold
    counts, costs, hyps = [], [], []
    for g in range(n // 4):
        ql = [c for k in range(4 * g, 4 * g + 4) for c in L[k]]
        qb = [c for k in range(4 * g, 4 * g + 4) for c in B[k]]
        H, w0, valid = hypothesis(ql, qb)
        count, cost = 0, 0.0
        for k in range(n):
            e, inl, _ = score(H, w0, B[k][0], B[k][1], L[k][0], L[k][1], thr2)
            cost = cost + e
            count += 1 if inl else 0
        counts.append(count if valid else -1)
        costs.append(cost)
        hyps.append((H, w0))
    order = sorted((g for g in range(len(counts)) if counts[g] >= 0), key=lambda g: (-counts[g], costs[g], g))
    winner = order[0] if order else -1
    mask = np.zeros(n, dtype=bool)
    if winner >= 0:
        H, w0 = hyps[winner]
        for k in range(n):
            mask[k] = score(H, w0, B[k][0], B[k][1], L[k][0], L[k][1], thr2)[1]
    return {"counts": np.array(counts, dtype=np.int32), "costs": np.array(costs), "winner": winner,
            "runner_up": order[1] if len(order) > 1 else -1, "mask": mask, "H": hyps[winner] if winner >= 0 else None}


def regate(R, t, L, B, threshold):
    """Step 7 -> (mask [n], e [n])."""
    thr2 = threshold * threshold
    R = [[float(v) for v in row] for row in np.asarray(R)]
    t = [float(v) for v in t]
    mask, es = [], []
    for (x, y), (X, Y) in zip(np.asarray(L, dtype=np.float64).reshape(-1, 2).tolist(), np.asarray(B, dtype=np.float64).reshape(-1, 2).tolist()):
        P0 = ((R[0][0] * X) + (R[0][1] * Y)) + t[0]
        P1 = ((R[1][0] * X) + (R[1][1] * Y)) + t[1]
        P2 = ((R[2][0] * X) + (R[2][1] * Y)) + t[2]
        du = _div(P0, P2) - x
        dv = _div(P1, P2) - y
        e = (du * du) + (dv * dv)
        mask.append(P2 > 0.0 and math.isfinite(e) and e < thr2)
        es.append(e)
    return np.array(mask, dtype=bool), np.array(es)


def pose_from_homography(H, w0):
    """A start for the least squares: H ~ [r1 r2 t] with the group's first corner in front."""
    Hm = np.array(H, dtype=np.float64).reshape(3, 3)
    lam = 2.0 / (np.linalg.norm(Hm[:, 0]) + np.linalg.norm(Hm[:, 1]))
    if w0 < 0:
        lam = -lam
    r1, r2, t = lam * Hm[:, 0], lam * Hm[:, 1], lam * Hm[:, 2]
    U, _, Vt = np.linalg.svd(np.stack([r1, r2, np.cross(r1, r2)], 1))
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R = U @ np.diag([1, 1, -1]) @ Vt
    return R, t


def robust_pose(L, B, hyp_threshold, threshold, min_inliers=4, max_fits=4):
    """One image from its lifted corners L (float32-rounded) and board points B.  -> dict: status, R, t (None without a pose), rms,
    mask, first_mask, n_inliers, best_group, n_fits, counts, costs, runner_up, and `gate_e`: the e of every corner at every re-gate (for
    the margin check of the tests)."""
    L = np.asarray(L, dtype=np.float64).reshape(-1, 2)
    B = np.asarray(B, dtype=np.float64).reshape(-1, 2)
    n = len(L)
    c = consensus(L, B, hyp_threshold)
    out = {"status": NO_CONSENSUS, "R": None, "t": None, "rms": math.nan, "mask": np.zeros(n, dtype=bool), "first_mask": c["mask"].copy(),
           "n_inliers": 0, "best_group": -1, "n_fits": 0, "counts": c["counts"], "costs": c["costs"], "winner": c["winner"],
           "runner_up": c["runner_up"], "gate_e": []}
    if c["winner"] < 0 or c["counts"][c["winner"]] < min_inliers:
        return out
    out["best_group"] = c["winner"]
    cur = c["mask"].copy()
    R, t = pose_from_homography(*c["H"])
    while True:
        R, t, sol = pnp_lsq(L[cur], B[cur], R, t)
        out["n_fits"] += 1
        new, e = regate(R, t, L, B, threshold)
        out["gate_e"].append(e)
        if np.array_equal(new, cur):
            break
        if new.sum() < min_inliers:
            return out
        if out["n_fits"] == max_fits:
            break
        cur = new
    out.update(status=OK, R=R, t=t, rms=float(np.sqrt(np.sum(sol.fun ** 2) / cur.sum())), mask=cur, n_inliers=int(cur.sum()),
               cost=0.5 * float(np.sum(sol.fun ** 2)))
    return out


def lifted32(model, proj, dist, px):
    """Step 1: K10's lift, x/z and y/z rounded to float32 (as float64 values)."""
    return lift(model, proj, dist, px).astype(np.float32).astype(np.float64)


__all__ = ["consensus", "hypothesis", "score", "regate", "robust_pose", "lifted32", "quat_wxyz_to_R", "OK", "NO_CONSENSUS"]
