"""Seeded inputs of the K23 tests (one robust cost over intrinsics, board poses, T_cl and range): the problems of
tests/laserrange_cases.py (joint_cases' board images and scan lines with a planted range offset b and scale kappa), optionally
contaminated by tests/jointrobust_cases.contaminate (10 % of an image's points pulled 0.10-0.30 m, 5 % of its corners moved 3-10 px),
and a start camera a little off the true one, as a camera estimated from other images would be.
A problem: laserrange_cases' dict (images, pose_cl_true, pose_cl0, range_true, range0, cam) and cam0, the start camera."""
from __future__ import annotations

import numpy as np

import joint_cases as jcases
import jointrobust_cases as rcases
import laserrange_cases as lcases
from camlasercalibratool_amd.camera import Camera

CAMERAS = jcases.CAMERAS
WAVES, THREADS = jcases.WAVES, jcases.THREADS
SIGMA_PX, SIGMA_LASER = rcases.SIGMA_PX, rcases.SIGMA_LASER
LOSS_CORNER, LOSS_LASER = rcases.LOSS_CORNER, rcases.LOSS_LASER
KB_HOLD = (1 << 6) | (1 << 7)  # clc_full_options_default: k4, k5 of Kannala-Brandt


def default_mask(name):
    return KB_HOLD if name == "kb" else 0


def start_camera(cam, seed):
    """The true camera with the focal lengths off by up to 1 %, the principal point by up to 2 px and the distortion by up to 10 % of
    itself (held Kannala-Brandt coefficients keep their true value only where the test holds them)."""
    rng = np.random.default_rng(seed + 770001)
    proj = np.array(cam.proj, np.float64)
    proj[:2] *= 1.0 + rng.uniform(-0.01, 0.01, 2)
    proj[2:] += rng.uniform(-2.0, 2.0, 2)
    dist = np.array(cam.dist, np.float64) * (1.0 + rng.uniform(-0.1, 0.1, 4))
    if cam.model == 2:
        dist[2:] = cam.dist[2:]
    return Camera(cam.model, tuple(float(v) for v in proj), tuple(float(v) for v in dist), cam.width, cam.height)


def problem(name, seed, *a, dirty=False, **kw):
    p = lcases.problem(name, seed, *a, **kw)
    if dirty:
        p = rcases.contaminate(p, np.random.default_rng(seed + 9000))
    p["cam0"] = start_camera(p["cam"], seed)
    return p


arrays = lcases.arrays

# the seeded sets of the host test: (seed, images, corners, points, contaminated); the dense restatement keeps them at <= 16 images
SEEDED = [(201, 6, 144, 100, False), (202, 8, 144, 100, True), (203, 12, 64, 40, True), (204, 16, 144, 60, False)]


def seeded(name):
    return [problem(name, seed + (0 if name == "radtan" else 1000), n, c, p, dirty=dirty) for seed, n, c, p, dirty in SEEDED]


def edge_problems(name, seed=7):
    """The problems of the shape tests -> (problems, notes {name: index}).  Images per problem 1, 2, W-1, W, W+1 and T+1 (4 corners and 2
    points per image); corners per image 3 (dropped), 4, 63, 64, 65, 144; points per image 0, 1, 63, 64, 65, 1081; no laser at all."""
    problems, notes = [], {}

    def add(nm, *a, **kw):
        notes[nm] = len(problems)
        problems.append(problem(name, seed + 31 * len(problems), *a, **kw))

    for n in (1, 2, WAVES - 1, WAVES, WAVES + 1):
        add("images%d" % n, n, 144, 100)
    add("images%d" % (THREADS + 1), THREADS + 1, 4, 2, spread4=True)
    add("corners", 6, [3, 4, 63, 64, 65, 144], 100, dirty=True)
    add("points", 6, 144, [0, 1, 63, 64, 65, 1081], dirty=True)
    add("nolaser", 4, 144, 0)
    return problems, notes


def recovery_sets(name, n_sets=8, n_images=30, seed0=600, offset=0.02, scale=0.005):
    """The seeded sets of the recovery test: a planted range error (K21's figures: 0.02 m and 0.5 %) and K22's planted outliers on the
    same problem -> list of contaminated problems; every planted observation lies where contaminate puts it."""
    return [problem(name, seed0 + s, n_images, 144, 100, dirty=True, offset=offset, scale=scale) for s in range(n_sets)]


planted_masks = rcases.planted_masks
separation = rcases.separation
tcl_distance = rcases.tcl_distance
