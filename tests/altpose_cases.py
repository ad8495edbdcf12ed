"""Seeded inputs of the K17 tests (the planar fit's second minimum): Kalibr-board images from camera.kalibr_board_points with 0.3 px of
noise under the two camera models of tests/golden/camera_*.yaml (PINHOLE with distortion, KANNALA_BRANDT): unambiguous views (36
tags at 1 m), ambiguous ones (36 tags at 4 m tilted 15 degrees; a 2 x 2 block of tags at 2.5 m), single tags, contaminated boards
(robustpose_cases.contaminate, to be used with K16's mask) and the edge shapes of the GPU test.  Float32 pixels / board points.
The seeds are chosen so that the restatement's own numbers meet the input condition (test_altpose_host.assert_input_condition)."""
from __future__ import annotations

import os

import numpy as np

import campose_ref as cref
import robustpose_cases as rcases
from camlasercalibratool_amd import camera as cam_mod

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAMERAS = {"radtan": cam_mod.Camera.from_yaml(os.path.join(GOLDEN, "camera_radtan.yaml")),
           "kb": cam_mod.Camera.from_yaml(os.path.join(GOLDEN, "camera_kannala_brandt.yaml"))}
BLOCK4 = (0, 1, 6, 7)  # a 2 x 2 block of tags
# seeds per (camera, view): see the module docstring
SEEDS = {("radtan", "near"): 11, ("radtan", "far"): 12, ("radtan", "block4"): 13, ("radtan", "tag1"): 14, ("radtan", "dirty"): 15,
         ("kb", "near"): 21, ("kb", "far"): 22, ("kb", "block4"): 23, ("kb", "tag1"): 24, ("kb", "dirty"): 25}


def board_of(ids):
    return cam_mod.kalibr_board_points(np.asarray(ids), rcases.ROWS, rcases.COLS, rcases.TAG, rcases.SPACING).astype(np.float32)


def tilted_pose(rng, b, dist, tilt_deg):
    """The centroid of the board points b near the optical axis at `dist` metres, the board tilted tilt_deg about a random in-plane
    axis from facing the camera and turned a little about its normal."""
    az = rng.uniform(0, 2 * np.pi)
    R = cref.rotvec_to_R(np.array([np.cos(az), np.sin(az), 0.0]) * np.deg2rad(tilt_deg)) @ cref.rotvec_to_R(np.array([0, 0, rng.uniform(-0.3, 0.3)]))
    c = np.array([*np.asarray(b, np.float64).mean(0), 0.0])
    t = -R @ c + np.array([rng.uniform(-0.05, 0.05) * dist, rng.uniform(-0.05, 0.05) * dist, dist])
    return R, t


def view(name, kind, n_images):
    """-> list of (px, board, R, t).  kind: near | far | block4 | tag1."""
    cam = CAMERAS[name]
    rng = np.random.default_rng(SEEDS[(name, kind)])
    ids, dist, tilt = {"near": (np.arange(36), 1.0, 10.0), "far": (np.arange(36), 4.0, 15.0), "block4": (BLOCK4, 2.5, 15.0),
                       "tag1": ((14,), 0.8, 20.0)}[kind]
    b = board_of(ids)
    out = []
    for _ in range(n_images):
        R, t = tilted_pose(rng, b, dist, tilt)
        out.append((rcases.project(cam, b, R, t, rng), b, R, t))
    return out


def dirty(name, n_images):
    """Contaminated 36-tag boards at 0.6-1.5 m (two swapped tag pairs, five displaced corners) -> list of (px, board, clean, R, t)."""
    cam = CAMERAS[name]
    rng = np.random.default_rng(SEEDS[(name, "dirty")])
    b = rcases.board()
    out = []
    for _ in range(n_images):
        R, t = rcases.pose(rng)
        px, clean = rcases.contaminate(rng, rcases.project(cam, b, R, t, rng))
        out.append((px, b, clean, R, t))
    return out


def edge_shapes(name, seed=7):
    """The one batch of the GPU test, sized to go wrong at the lane and slot edges -> (images, notes {name: index}); an image is a
    dict: px, board (what the call gets), px_pose, board_pose (what its input pose is fitted on: the same before a corner or a board
    point was spoilt), mask (every image carries one; all ones where the case needs none), bad_status (its status_in is to be forced
    != OK)."""
    cam = CAMERAS[name]
    rng = np.random.default_rng(seed)
    full = rcases.board()
    images, notes = [], {}

    def add(nm, px, bb, mask=None, px_pose=None, board_pose=None, bad_status=False):
        notes[nm] = len(images)
        images.append(dict(px=px, px_pose=px if px_pose is None else px_pose, board=bb, board_pose=bb if board_pose is None else board_pose,
                           bad_status=bad_status,
                           mask=np.ones(len(px), bool) if mask is None else mask))

    def image(n_corners, dist=1.0, tilt=10.0):
        bb = full[:n_corners]
        R, t = tilted_pose(rng, bb, dist, tilt)
        return rcases.project(cam, bb, R, t, rng), bb

    for n in (4, 5, 63, 64, 65, 144):
        add("n%d" % n, *image(n))
    add("far144", *image(144, 4.0, 15.0))
    px, bb = image(144)  # a mask that leaves exactly 4 corners, spread over lanes and chunks
    m = np.zeros(144, bool); m[[3, 64, 70, 143]] = True
    add("mask4", px, bb, m)
    px, bb = image(144)  # and one that leaves 3
    m = np.zeros(144, bool); m[[0, 63, 128]] = True
    add("mask3", px, bb, m)
    px, bb = image(144)  # 65 corners in the set: the second chunk's ranks
    m = np.zeros(144, bool); m[np.r_[0:60, 100:105]] = True
    add("mask65", px, bb, m)
    add("bad_status", *image(144), bad_status=True)
    add("after_bad_status", *image(144))
    px, bb = image(144)  # a non-finite corner inside the set
    bad = px.copy(); bad[77, 1] = np.nan
    add("nan_inside", bad, bb, px_pose=px)
    px, bb = image(144)  # and one outside it: ignored
    bad = px.copy(); bad[77, 0] = np.inf
    m = np.ones(144, bool); m[76:80] = False
    add("nan_outside", bad, bb, m, px_pose=px)
    px, bb = image(144)  # a non-finite board point inside the set (under a mask that drops other corners)
    bad = bb.copy(); bad[130, 0] = np.nan
    m = np.ones(144, bool); m[0:8] = False
    add("nan_board_inside", px, bad, m, board_pose=bb)
    add("empty", np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
    add("tail", *image(144, 2.0, 10.0))
    return images, notes
