"""Seeded inputs of the K22 tests (robust joint refinement): the problems of joint_cases with planted outliers of the kind that
neither `keep` (per image), K16 (per tag) nor K12 (per pose) removes.

contaminate(problem, rng): 10 % of each image's laser points are pulled along their ray towards the scanner by U(0.10, 0.30) m (a
leg or a cable in front of the board), 5 % of its corners are moved U(3, 10) px in a random direction (a mis-refined corner); the
planted indices are kept.  At the true poses every planted point lies >= 8 sigma_laser off its board plane and every planted
corner >= 10 sigma_px from its projection: asserted here, each observation redrawn with the seed's stream until it holds.
truth_check(problem): at the true poses, under the default scales, the restatement gives every planted observation w < 0.5 and
>= 95 % of the others w >= 0.5 — what the recovery test asks of K22's answer, asked of the data first."""
from __future__ import annotations

import numpy as np

import campose_ref as cref
import joint_cases as jcases
import joint_ref as ref
import jointrobust_ref as rref

SIGMA_PX, SIGMA_LASER = 0.3, 0.01   # joint_cases' noise levels, the defaults of clc_joint_options
LOSS_CORNER, LOSS_LASER = 3.0, 5.0  # the defaults of clc_joint_loss_options at those sigmas
POINT_FRACTION, CORNER_FRACTION = 0.10, 0.05
MIN_POINT_SIGMAS, MIN_CORNER_SIGMAS = 8.0, 10.0


def plane_distance(R, t, Rcl, tcl, p):
    """e3^T R^T (R_cl p + t_cl - t): the signed distance of laser point(s) p from the board plane of pose (R, t)."""
    return (np.atleast_2d(p) @ Rcl.T + tcl - t) @ R[:, 2]


def true_pixels(cam, board, R, t):
    X = np.concatenate([np.asarray(board, np.float64), np.zeros((len(board), 1))], 1)
    return cref.project(cam.model, cam.proj, cam.dist, X @ R.T + t)


def contaminate(problem, rng, point_fraction=POINT_FRACTION, corner_fraction=CORNER_FRACTION):
    """-> a new problem with the outliers planted, and `planted`: per image (corner indices, point indices)."""
    cam = problem["cam"]
    Rcl, tcl = ref.pose7_to_Rt(problem["pose_cl_true"])
    images, planted = [], []
    for px, bb, R, t, pts in problem["images"]:
        px, pts = np.array(px, dtype=np.float32), np.array(pts, dtype=np.float64)
        kc, kp = int(round(corner_fraction * len(px))), int(round(point_fraction * len(pts)))
        truth = true_pixels(cam, bb, R, t) if len(bb) else np.zeros((0, 2))
        # an observation — which one, and by how much it moves — is redrawn until it lies far enough out (a ray that grazes its
        # board cannot leave the plane by 8 sigma however far the point is pulled)
        ic, ip = [], []
        for _ in range(kc):
            for _ in range(10000):
                j, ang, d = int(rng.integers(len(px))), rng.uniform(0.0, 2.0 * np.pi), rng.uniform(3.0, 10.0)
                cand = (px[j].astype(np.float64) + d * np.array([np.cos(ang), np.sin(ang)])).astype(np.float32)
                if j not in ic and np.linalg.norm(cand.astype(np.float64) - truth[j]) >= MIN_CORNER_SIGMAS * SIGMA_PX:
                    break
            else:
                raise AssertionError("no displaced corner far enough from its projection")
            px[j] = cand
            ic.append(j)
        for _ in range(kp):
            for _ in range(10000):
                k, d = int(rng.integers(len(pts))), rng.uniform(0.10, 0.30)
                cand = pts[k] * (1.0 - d / np.linalg.norm(pts[k]))
                if k not in ip and abs(plane_distance(R, t, Rcl, tcl, cand)[0]) >= MIN_POINT_SIGMAS * SIGMA_LASER:
                    break
            else:
                raise AssertionError("no pulled point far enough from its board plane")
            pts[k] = cand
            ip.append(k)
        ic, ip = np.sort(np.array(ic, dtype=int)), np.sort(np.array(ip, dtype=int))
        # the file's own statement about what it planted
        assert np.all(np.linalg.norm(px[ic].astype(np.float64) - truth[ic], axis=1) >= MIN_CORNER_SIGMAS * SIGMA_PX)
        assert np.all(np.abs(plane_distance(R, t, Rcl, tcl, pts[ip])) >= MIN_POINT_SIGMAS * SIGMA_LASER) if len(ip) else True
        images.append((px, bb, R, t, pts))
        planted.append((ic, ip))
    return dict(problem, images=images, planted=planted)


def restatement_at_truth(problem, lc=LOSS_CORNER, ll=LOSS_LASER):
    """The problem as jointrobust_ref takes it, with the Python lift (rounded to float32 as the library's), and the true poses."""
    cam = problem["cam"]
    f = float(np.sqrt(abs(cam.proj[0] * cam.proj[1])))
    lifted = [cref.lift(cam.model, cam.proj, cam.dist, np.asarray(im[0], np.float64)).astype(np.float32).astype(np.float64)
              for im in problem["images"]]
    prob = dict(lifted=lifted, board=[np.asarray(im[1], np.float64) for im in problem["images"]], pts=[im[4] for im in problem["images"]],
                sc=SIGMA_PX / f, sl=SIGMA_LASER, lc=lc, ll=ll)
    X = ([im[2] for im in problem["images"]], [im[3] for im in problem["images"]], *ref.pose7_to_Rt(problem["pose_cl_true"]))
    return prob, X


def planted_masks(problem):
    """-> planted corners [all corners of the problem] bool, planted points [all points] bool, image by image."""
    mc = [np.isin(np.arange(len(im[0])), pl[0]) for im, pl in zip(problem["images"], problem["planted"])]
    mp = [np.isin(np.arange(len(im[4])), pl[1]) for im, pl in zip(problem["images"], problem["planted"])]
    return np.concatenate(mc), np.concatenate(mp)


def separation(w_corner, w_laser, mc, mp):
    """-> (every planted observation has w < 0.5, the fraction of the others with w >= 0.5)."""
    planted_down = bool(np.all(w_corner[mc] < 0.5) and np.all(w_laser[mp] < 0.5))
    others = np.concatenate([w_corner[~mc], w_laser[~mp]])
    return planted_down, float(np.mean(others >= 0.5)) if len(others) else 1.0


def truth_check(problem):
    prob, X = restatement_at_truth(problem)
    wc, wl = rref.weights(prob, *X)
    down, frac = separation(wc, wl, *planted_masks(problem))
    assert down and frac >= 0.95, (down, frac)
    return frac


def recovery_sets(name, n_sets=8, n_images=30, seed0=400):
    """The seeded sets of the recovery test -> list of (clean problem, contaminated problem); truth_check holds for each."""
    out = []
    for s in range(n_sets):
        clean = jcases.problem(name, seed0 + s, n_images, 144, 100)
        dirty = contaminate(clean, np.random.default_rng(9000 + seed0 + s))
        truth_check(dirty)
        out.append((clean, dirty))
    return out


def contaminated_edge_problems(name, seed=7):
    """joint_cases.edge_problems with every image of >= 16 observations contaminated -> (problems, notes)."""
    problems, notes = jcases.edge_problems(name, seed)
    rng = np.random.default_rng(seed + 5000)
    out = []
    for p in problems:
        c = contaminate(p, rng)
        # images with fewer than 16 observations stay as they were
        imgs = [ci if len(im[0]) + len(im[4]) >= 16 else im for im, ci in zip(p["images"], c["images"])]
        out.append(dict(p, images=imgs))
    return out, notes


def tcl_distance(pose_a, pose_b):
    """|t_a - t_b| of two pose7."""
    return float(np.linalg.norm(np.asarray(pose_a)[:3] - np.asarray(pose_b)[:3]))
