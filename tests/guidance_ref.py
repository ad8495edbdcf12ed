"""Pose guidance (K20) restated in numpy from the definitions of the feature, independently of csrc/clc_guidance.hpp: the cast of the
scanner's rays onto a candidate board, the information H_add the pose would add, eigvalsh of M + H_add, the score, the greedy rounds.

  candidate   n = R_ca e3, d = -n.t_ca, m = R_cl^T n, d_l = n.t_cl + d
  ray i       dir = (cos th, sin th, 0), th = angle_min + i angle_increment;  rho = -d_l / (m.dir);  p = rho dir;
              X = R_ca^T (R_cl p + t_cl - t_ca);  hit: rho finite, range_min <= rho < range_max, board_min <= X_xy <= board_max
  seen        c = #hits >= min_points: H_add = (1 / c) sum u u^T, u = [n, p x m];  otherwise H_add = 0 (non-finite candidate: n_hits -1)
"""
from dataclasses import dataclass

import numpy as np

LOGDET, MIN_EIG = 0, 1


@dataclass
class Model:
    n_rays: int = 1081
    min_points: int = 50
    angle_min: float = -np.deg2rad(270.0) / 2
    angle_increment: float = np.deg2rad(270.0) / 1080
    range_min: float = 0.05
    range_max: float = 30.0
    board_min: tuple = (-0.043, -0.043)
    board_max: tuple = (0.457, 0.457)
    eig_floor: float = 1e-8
    criterion: int = LOGDET


def rot_wxyz(q):
    """Eigen's toRotationMatrix of (w, x, y, z), not normalised."""
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def pose_cl_Rt(pose_cl):
    p = np.asarray(pose_cl, dtype=np.float64)
    return rot_wxyz([p[6], p[3], p[4], p[5]]), p[:3].copy()


def cast(model, pose_cl, q, t):
    """One candidate -> dict(n_hits, hit [n_rays] bool, rho, p [n_rays, 3], X [n_rays, 2], n, m, finite)."""
    q, t = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)
    if not (np.all(np.isfinite(q)) and np.all(np.isfinite(t))):
        return dict(n_hits=-1, finite=False)
    Rcl, tcl = pose_cl_Rt(pose_cl)
    R = rot_wxyz(q)
    n = R[:, 2]
    d = -n @ t
    m = Rcl.T @ n
    dl = n @ tcl + d
    th = model.angle_min + np.arange(model.n_rays) * model.angle_increment
    dirs = np.stack([np.cos(th), np.sin(th), np.zeros_like(th)], 1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rho = -dl / (dirs @ m)
        p = rho[:, None] * dirs
        X = (Rcl @ p.T).T + (tcl - t)
        X = X @ R  # rows R^T w
        in_range = np.isfinite(rho) & (rho >= model.range_min) & (rho < model.range_max)
        inside = (X[:, 0] >= model.board_min[0]) & (X[:, 0] <= model.board_max[0]) & \
                 (X[:, 1] >= model.board_min[1]) & (X[:, 1] <= model.board_max[1])
    hit = in_range & inside
    return dict(n_hits=int(hit.sum()), hit=hit, rho=rho, p=p, X=X[:, :2], n=n, m=m, finite=True, in_range=in_range)


def h_add(model, pose_cl, q, t):
    """-> (n_hits, H_add [6, 6], hit points [c, 3] in the laser frame)."""
    c = cast(model, pose_cl, q, t)
    if not c["finite"] or c["n_hits"] < model.min_points:
        pts = c["p"][c["hit"]] if c["finite"] else np.zeros((0, 3))
        return c["n_hits"], np.zeros((6, 6)), pts
    P = c["p"][c["hit"]]
    U = np.concatenate([np.tile(c["n"], (P.shape[0], 1)), np.cross(P, c["m"])], 1)
    return c["n_hits"], (U.T @ U) / P.shape[0], P


def margin(model, pose_cl, q, t):
    """Smallest distance (m) of an in-range intersection to the rectangle's edge, and of any finite positive range to the two range
    limits: what a last-bit change of a direction would have to cross to change the count."""
    c = cast(model, pose_cl, q, t)
    if not c["finite"]:
        return np.inf
    g = np.inf
    r = c["in_range"]
    if r.any():
        X = c["X"][r]
        for a in range(2):
            g = min(g, np.abs(X[:, a] - model.board_min[a]).min(), np.abs(X[:, a] - model.board_max[a]).min())
    rho = c["rho"][np.isfinite(c["rho"])]
    if rho.size:
        g = min(g, np.abs(rho - model.range_min).min(), np.abs(rho - model.range_max).min())
    return float(g)


def eig_desc(M):
    return np.linalg.eigvalsh(M)[::-1].copy()


def score_of(model, sv):
    if model.criterion == MIN_EIG:
        return float(sv[5])
    return float(np.sum(np.log(np.maximum(sv, model.eig_floor))))


def score_all(model, pose_cl, H0, q, t):
    """-> dict(n_hits [n], H_add [n, 6, 6], sv [n, 6], score [n], pts: list of hit points)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    n = q.shape[0]
    M0 = np.zeros((6, 6)) if H0 is None else np.asarray(H0, dtype=np.float64).reshape(6, 6)
    out = dict(n_hits=np.zeros(n, dtype=np.int32), H_add=np.zeros((n, 6, 6)), sv=np.zeros((n, 6)), score=np.zeros(n), pts=[])
    for i in range(n):
        c, Ha, P = h_add(model, pose_cl, q[i], t[i])
        out["n_hits"][i] = c
        out["H_add"][i] = Ha
        out["sv"][i] = eig_desc(M0 + Ha)
        out["score"][i] = score_of(model, out["sv"][i])
        out["pts"].append(P)
    return out


def greedy(model, H0, n_hits, H_add, k):
    """The greedy rounds on given H_add -> dict(chosen [k] (-1 padded), sv_after [k, 6], score_after [k], H_after, gaps: per round the
    relative gap between the best and the second-best score (inf with one candidate left))."""
    n = len(n_hits)
    M = np.zeros((6, 6)) if H0 is None else np.array(H0, dtype=np.float64).reshape(6, 6)
    taken = np.zeros(n, dtype=bool)
    chosen = np.full(k, -1, dtype=np.int64)
    sva = np.full((k, 6), np.nan)
    sca = np.full(k, np.nan)
    gaps = []
    for r in range(k):
        idx = [i for i in range(n) if n_hits[i] >= model.min_points and not taken[i]]
        if not idx:
            break
        svs = [eig_desc(M + H_add[i]) for i in idx]
        sc = np.array([score_of(model, s) for s in svs])
        b = int(np.argmax(sc))  # (the first of equal scores: the lowest index)
        if len(sc) > 1:
            second = np.partition(sc, -2)[-2]
            gaps.append(float((sc[b] - second) / max(abs(sc[b]), abs(second), 1e-300)))
        else:
            gaps.append(np.inf)
        chosen[r] = idx[b]
        sva[r] = svs[b]
        sca[r] = sc[b]
        taken[idx[b]] = True
        M = M + H_add[idx[b]]
    return dict(chosen=chosen, sv_after=sva, score_after=sca, H_after=M, gaps=gaps)


def information(obs, pose_cl):
    """H = sum J^T J of the analysis pass over the scan points of an ObservationSet at pose_cl, restated: per pose (1 / c) sum u u^T."""
    Rcl, _ = pose_cl_Rt(pose_cl)
    H = np.zeros((6, 6))
    for i in range(obs.n_poses):
        P = obs.pts[obs.pts_off[i]:obs.pts_off[i + 1]]
        if P.shape[0] == 0:
            continue
        n = rot_wxyz(obs.tag_q[i])[:, 2]
        m = Rcl.T @ n
        U = np.concatenate([np.tile(n, (P.shape[0], 1)), np.cross(P, m)], 1)
        H += (U.T @ U) / P.shape[0]
    return H
