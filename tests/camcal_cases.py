"""Seeded inputs of the K19 tests (camera intrinsics from the board images): images of the 6x6 Kalibr board under the cameras of
tests/golden (altpose_cases.CAMERAS), 0.3 px noise.  The pose sampler is this file's own: board centre up to +-0.3 x distance off the
optical axis, 0.5-1.2 m away, tilted 10-40 degrees about a random in-plane axis, any roll — the spread of views an intrinsic
calibration needs (altpose_cases.tilted_pose keeps the board within 5 % of the axis).  Everything is float32 pixels / board points."""
from __future__ import annotations

import numpy as np

import altpose_cases as acases
import campose_ref as pref
import robustpose_cases as rcases

CAMERAS = acases.CAMERAS
CORNER_TAGS = (0, 5, 30, 35)  # the board's four corner tags


def board_of(ids):
    return acases.board_of(ids)


def pose(rng, b):
    dist = rng.uniform(0.5, 1.2)
    tilt = np.deg2rad(rng.uniform(10.0, 40.0))
    ax = rng.uniform(0, 2 * np.pi)
    R = pref.rotvec_to_R(np.array([np.cos(ax), np.sin(ax), 0.0]) * tilt) @ pref.rotvec_to_R(np.array([0.0, 0.0, rng.uniform(-np.pi, np.pi)]))
    full = rcases.board()
    c = np.r_[0.5 * (full.min(0) + full.max(0)).astype(np.float64), 0.0]
    t = -R @ c + np.array([rng.uniform(-0.3, 0.3) * dist, rng.uniform(-0.3, 0.3) * dist, dist])
    return R, t


def images(name, seed, n_images, ids=None, n_corners=None):
    """-> list of (px float32 [n, 2], board float32 [n, 2], R, t); n_corners: the first n corners of the board only."""
    cam = CAMERAS[name]
    rng = np.random.default_rng(seed)
    b = rcases.board() if ids is None else board_of(ids)
    if n_corners is not None:
        b = b[:n_corners]
    out = []
    for _ in range(n_images):
        R, t = pose(rng, b)
        out.append((rcases.project(cam, b, R, t, rng), b, R, t))
    return out


def arrays(problems):
    """problems: list of image lists -> dict corners [M, 2] float32, board [M, 2] float32, coff [n + 1] int64, prob_off [np + 1]."""
    corners, board, coff, poff = [], [], [0], [0]
    for imgs in problems:
        for px, b, _, _ in imgs:
            corners.append(np.asarray(px, np.float32).reshape(-1, 2))
            board.append(np.asarray(b, np.float32).reshape(-1, 2))
            coff.append(coff[-1] + len(px))
        poff.append(poff[-1] + len(imgs))
    cat = lambda v: np.ascontiguousarray(np.concatenate(v)) if v else np.zeros((0, 2), np.float32)
    return dict(corners=cat(corners), board=cat(board), coff=np.array(coff, dtype=np.int64), prob_off=np.array(poff, dtype=np.int64))


# (seed, images) of the sets the host build is compared with the restatement on, per camera
SEEDED = [(201, 6), (202, 12), (203, 20)]


def seeded(name):
    off = 0 if name == "radtan" else 50
    return [images(name, seed + off, n) for seed, n in SEEDED]


def start_camera(cam):
    """A start off the truth: focal lengths 1 % out, the principal point 2 and 1.5 px, the free distortion 5 %."""
    k = np.r_[cam.proj, cam.dist] * np.array([1.01, 0.99, 1, 1, 1.05, 0.95, 1.05, 0.95]) + np.array([0, 0, 2.0, -1.5, 0, 0, 0, 0])
    return type(cam)(cam.model, tuple(float(v) for v in k[:4]), tuple(float(v) for v in k[4:]), cam.width, cam.height)


def edge_problems(name, seed=300):
    """The problems of the GPU test's one batch, sized to go wrong at the wave, lane and thread edges -> (problems, notes {name: index}):
    images per problem W - 1, W, W + 1 (W = 4 waves) and T + 1 (T = 256 threads; 4 x 4 corners from the board's corner tags each);
    corners per image 3 (dropped), 4, 63, 64, 65, 144 in one problem with five full images; a problem for keep with holes, one to be
    dropped whole, a seeded one."""
    problems, notes = [], {}

    def add(nm, imgs):
        notes[nm] = len(problems)
        problems.append(imgs)

    for j, P in enumerate((3, 4, 5)):
        add("images%d" % P, images(name, seed + j, P))
    mixed = [images(name, seed + 10 + j, 1, n_corners=n)[0] for j, n in enumerate((3, 4, 63, 64, 65))]
    add("corners", mixed + images(name, seed + 20, 5))
    add("holes", images(name, seed + 30, 7))
    add("dropped", images(name, seed + 31, 3))
    add("seeded", images(name, seed + 32, 10))
    add("threads+1", images(name, seed + 40, 257, ids=CORNER_TAGS))
    return problems, notes


def few_image_problems(name, seed=350):
    """1 and 2 images: they cannot fix 8 intrinsics (run with the distortion held; only the cost is compared)."""
    return [images(name, seed, 1), images(name, seed + 1, 2)]


def small_problems(name, n_problems=257, seed=400):
    """Many small problems: 4 images of 9 tags (36 corners) each."""
    return [images(name, seed + k, 4, ids=(0, 2, 5, 14, 17, 21, 30, 33, 35)) for k in range(n_problems)]
