"""Seeded inputs of the K21 tests (range offset and scale in the joint refinement): the problems of tests/joint_cases.py with
simdata.apply_range_error applied to the laser points — what a scanner with that offset and scale would have measured.  Offset and
scale are drawn per problem from +-0.03 m and +-1 % unless given.  A problem: joint_cases' dict and range_true = [b, kappa],
range0 = [0, 0] (the start)."""
from __future__ import annotations

import numpy as np

import joint_cases as jcases
from camlasercalibratool_amd import simdata

CAMERAS = jcases.CAMERAS
SEEDED = jcases.SEEDED
WAVES, THREADS = jcases.WAVES, jcases.THREADS


def problem(name, seed, *a, offset=None, scale=None, **kw):
    p = jcases.problem(name, seed, *a, **kw)
    rng = np.random.default_rng(seed + 900001)
    b, k = rng.uniform(-0.03, 0.03), rng.uniform(-0.01, 0.01)
    b = b if offset is None else float(offset)
    k = k if scale is None else float(scale)
    p["images"] = [(px, bb, R, t, simdata.apply_range_error(pts, b, k)) for px, bb, R, t, pts in p["images"]]
    p["range_true"] = np.array([b, k])
    p["range0"] = np.zeros(2)
    return p


def arrays(problems):
    a = jcases.arrays(problems)
    a["range0"] = np.stack([p["range0"] for p in problems]) if problems else np.zeros((0, 2))
    return a


def seeded(name):
    return [problem(name, seed + (0 if name == "radtan" else 1000), *shape) for seed, *shape in SEEDED]


SINGLE_RANGE = 2.0  # metres


def edge_problems(name, seed=7):
    """The problems of the shape tests -> (problems, notes {name: index}).  Images per problem 1, 2, 3, 4, 5 and 257 (4 corners and 2
    points per image); corners per image 3 (dropped), 4, 63, 64, 65, 144; points per image 0, 1, 63, 64, 65, 1081; no laser at all; one
    image with a zero-range point; a single-range problem (every point of every image scaled to |p| = 2 m)."""
    problems, notes = [], {}

    def add(nm, *a, **kw):
        notes[nm] = len(problems)
        problems.append(problem(name, seed + 31 * len(problems), *a, **kw))
        return problems[-1]

    for n in (1, 2, WAVES - 1, WAVES, WAVES + 1):
        add("images%d" % n, n, 144, 100)
    add("images%d" % (THREADS + 1), THREADS + 1, 4, 2, spread4=True)
    add("corners", 6, [3, 4, 63, 64, 65, 144], 100)
    add("points", 6, 144, [0, 1, 63, 64, 65, 1081])
    add("nolaser", 4, 144, 0)
    p = add("zerorange", 5, 144, 60)
    p["images"][2][4][17] = 0.0  # the scanner's "no return"
    p = add("singlerange", 8, 144, 100)
    p["images"] = [(px, bb, R, t, pts * (SINGLE_RANGE / np.linalg.norm(pts, axis=1))[:, None]) for px, bb, R, t, pts in p["images"]]
    return problems, notes
