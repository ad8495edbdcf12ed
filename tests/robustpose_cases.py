"""Seeded inputs of the K16 tests (robust board poses): the contaminated 6x6 Kalibr images of the issue's numpy experiment and the edge
shapes.  Everything is float32 pixels / board points, as the detector hands them over."""
from __future__ import annotations

import numpy as np

import campose_ref as ref
from camlasercalibratool_amd import camera as cam_mod

ROWS = COLS = 6
TAG, SPACING = 0.055, 0.3


def board(n_tags=36, origin=(0.0, 0.0)):
    b = cam_mod.kalibr_board_points(np.arange(n_tags), ROWS, COLS, TAG, SPACING).astype(np.float64)
    return (b + np.asarray(origin)).astype(np.float32)


def pose(rng, zlo=0.6, zhi=1.5):
    """The board's centre near the optical axis, 0.6-1.5 m away, tilted up to ~0.3 rad."""
    R = ref.rotvec_to_R(rng.normal(size=3) * 0.3)
    c = np.array([0.5, 0.5, 0.0]) * (TAG * (1 + SPACING) * (COLS - 1) + TAG)
    t = -R @ c + np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(zlo, zhi)])
    return R, t


def project(cam, b, R, t, rng, noise=0.3):
    X = np.concatenate([np.asarray(b, np.float64), np.zeros((len(b), 1))], 1)
    px = ref.project(cam.model, cam.proj, cam.dist, X @ R.T + t)
    return (px + rng.normal(size=px.shape) * noise).astype(np.float32)


def contaminate(rng, px, n_swaps=2, n_displaced=5):
    """Two pairs of swapped tag ids (the pixels of tag a arrive under b's board points and the other way round) plus five corners
    displaced by 10-40 px.  -> (px, clean [n] bool)."""
    px = px.copy()
    clean = np.ones(len(px), dtype=bool)
    tags = rng.choice(len(px) // 4, size=2 * n_swaps, replace=False)
    for a, b in tags.reshape(-1, 2):
        sa, sb = slice(4 * a, 4 * a + 4), slice(4 * b, 4 * b + 4)
        px[sa], px[sb] = px[sb].copy(), px[sa].copy()
        clean[sa] = clean[sb] = False
    for k in rng.choice(np.flatnonzero(clean), size=n_displaced, replace=False):
        ang, mag = rng.uniform(0, 2 * np.pi), rng.uniform(10.0, 40.0)
        px[k] += np.array([np.cos(ang), np.sin(ang)], dtype=np.float32) * np.float32(mag)
        clean[k] = False
    return px, clean


def contaminated_set(cam, n_images=60, seed=1):
    """The issue's set: 21 of 144 corners bad per image.  -> list of (px, board, clean, R, t)."""
    rng = np.random.default_rng(seed)
    b = board()
    out = []
    for _ in range(n_images):
        R, t = pose(rng)
        px, clean = contaminate(rng, project(cam, b, R, t, rng))
        out.append((px, b, clean, R, t))
    return out


def swapped_far_set(cam, n_images=20, seed=2, min_pitches=3):
    """Images whose only fault is two pairs of swapped tag ids, the two tags of a pair at least min_pitches tag pitches apart.
    A swap a <-> b displaces a's corners by d = x_b - x_a and b's by -d: the displacements cancel in translation, and being parallel to
    the lever arm they exert no torque either — what the least squares absorbs is a contraction along a - b, of strain about
    8 |d|^2 / sum |X_k - centre|^2, i.e. growing with the SQUARE of the distance: ~1 % for neighbouring tags (half a pixel at this
    board's size, within ten times the ~0.07 px at which 0.3 px of noise leaves a clean 144-corner fit), ~8 % at three pitches.
    -> list of (px, board, clean, R, t)."""
    rng = np.random.default_rng(seed)
    b = board()
    out = []
    for _ in range(n_images):
        R, t = pose(rng)
        px = project(cam, b, R, t, rng)
        clean = np.ones(len(px), dtype=bool)
        used = set()
        for _pair in range(2):
            while True:
                a, c = (int(v) for v in rng.choice(ROWS * COLS, size=2, replace=False))
                far = max(abs(a // COLS - c // COLS), abs(a % COLS - c % COLS)) >= min_pitches
                if far and a not in used and c not in used:
                    break
            used |= {a, c}
            sa, sc = slice(4 * a, 4 * a + 4), slice(4 * c, 4 * c + 4)
            px[sa], px[sc] = px[sc].copy(), px[sa].copy()
            clean[sa] = clean[sc] = False
        out.append((px, b, clean, R, t))
    return out


def csr(seq):
    """[(px, board), ...] -> corners, board, offsets."""
    corners = np.concatenate([np.asarray(s[0], np.float32).reshape(-1, 2) for s in seq])
    brd = np.concatenate([np.asarray(s[1], np.float32).reshape(-1, 2) for s in seq])
    off = np.concatenate([[0], np.cumsum([len(np.asarray(s[0]).reshape(-1, 2)) for s in seq])]).astype(np.int64)
    return corners, brd, off


def repeated_board(cam, rng, n_groups):
    """n_groups tags: the 36-tag board repeated with shifted origins (63, 64, 65 groups: the lane-chunk edge)."""
    pitch = TAG * (1 + SPACING) * COLS
    parts, g = [], 0
    while g < n_groups:
        m = min(36, n_groups - g)
        parts.append(board(m, origin=(pitch * (len(parts) % 2), pitch * (len(parts) // 2))))
        g += m
    b = np.concatenate(parts)
    R, t = pose(rng, 1.0, 1.5)
    return project(cam, b, R, t, rng), b, R, t


def edge_shapes(cam, seed=5):
    """The shapes the GPU test covers, a few images each, with what is expected of them -> (seq [(px, board)], notes {name: index})."""
    rng = np.random.default_rng(seed)
    b = board()
    seq, notes = [], {}

    def add(name, px, bb):
        notes[name] = len(seq)
        seq.append((px, bb))

    def clean_image(n_corners=144):
        R, t = pose(rng)
        return project(cam, b, R, t, rng)[:n_corners], b[:n_corners]

    add("n0", np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
    for n in (3, 4, 5, 7, 8, 144):
        add("n%d" % n, *clean_image(n))
    px, bb = clean_image(5)  # one tag plus a stray corner far off: scored, never an inlier
    px[4] += 60.0
    add("stray", px, bb)
    for G in (63, 64, 65):
        px, bb, _, _ = repeated_board(cam, rng, G)
        add("g%d" % G, px, bb)
    # the best group is the last one: every other tag's first corner displaced (their hypotheses lose corners), 64 groups
    px, bb, _, _ = repeated_board(cam, rng, 64)
    px[0:4 * 63:4] += np.float32(25.0)
    add("best_last", px, bb)
    # the best group lies in the second chunk: 65 groups, the first 64 spoilt the same way
    px, bb, _, _ = repeated_board(cam, rng, 65)
    px[0:4 * 64:4] += np.float32(25.0)
    add("best_second_chunk", px, bb)
    # all outliers: every tag's pixels from another pose
    R, t = pose(rng)
    px = project(cam, b, R, t, rng)
    px = rng.uniform([100, 100], [600, 400], size=px.shape).astype(np.float32)
    add("all_outliers", px, b)
    # a group with three collinear corners inside a good board: invalid (den == 0).  Corner 2 sits on corner 1 — the collinearity
    # that survives the lift and its float32 rounding exactly
    px, bb = clean_image()
    px = px.copy(); px[4 * 7 + 2] = px[4 * 7 + 1]
    add("collinear_group", px, bb)
    # a NaN corner inside a good board
    px, bb = clean_image()
    px = px.copy(); px[4 * 11 + 1, 0] = np.nan
    add("nan_corner", px, bb)
    # two tags only, both exact (noise-free): equal counts, the tie goes to the cost
    R, t = pose(rng)
    px = project(cam, b[:8], R, t, rng, noise=0.05)
    add("two_tags_tie", px, b[:8])
    # a contaminated board between good ones
    R, t = pose(rng)
    px, _ = contaminate(rng, project(cam, b, R, t, rng))
    add("contaminated", px, b)
    add("tail_clean", *clean_image())
    return seq, notes
