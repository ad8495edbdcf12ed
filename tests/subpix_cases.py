"""Seeded inputs of the K24 tests (no image is committed): rendered boards and single-corner patches, the batches every form runs on,
the edge cases, and the restatement's results on them (computed once per process and shared).

Rendering: per 4 x 4 sub-sample of every pixel the intensity of the scene (30 dark / 220 light), a Gaussian blur of sigma 0.8 px at the
sub-sample resolution, the mean over each pixel, Gaussian noise of sigma 2 grey levels, rounded to uint8.  Integer pixel coordinates are
pixel centres (the convention of cornerSubPix).  A board is seen through campose_ref.lift: every sub-sample's ray meets the board's
plane, and the square it lands in gives the intensity."""
from __future__ import annotations

import functools

import numpy as np

import campose_ref
import subpix_ref as ref

SS = 4            # sub-samples per pixel and axis
BLUR_PX = 0.8
NOISE = 2.0
DARK, LIGHT = 30.0, 220.0

SIZES = [(33, 21, 40), (61, 47, 61)]  # width, height, pitch
WINDOWS = [ref.Options(1, 1), ref.Options(3, 3), ref.Options(5, 3), ref.Options(11, 11), ref.Options(15, 15), ref.Options(5, 5, 1, 1)]
FIRST = 5         # offsets[0] of the batches
COUNTS = (0, 1, 257)


def _blur_axis(a, sigma, axis):
    r = int(np.ceil(4 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode="edge")
    out = np.zeros_like(a)
    n = a.shape[axis]
    for i, w in enumerate(k):
        out += w * (p[i:i + n, :] if axis == 0 else p[:, i:i + n])
    return out


def finish(hi, rng):
    """The sub-sample intensities [height SS, width SS] -> the uint8 image [height, width]."""
    hi = _blur_axis(_blur_axis(hi, BLUR_PX * SS, 0), BLUR_PX * SS, 1)
    h, w = hi.shape[0] // SS, hi.shape[1] // SS
    img = hi.reshape(h, SS, w, SS).mean(axis=(1, 3))
    img = img + rng.normal(0.0, NOISE, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def subsample_grid(width, height):
    """The pixel coordinates of every sub-sample -> u, v [height SS, width SS]."""
    u = (np.arange(width * SS) + 0.5) / SS - 0.5
    v = (np.arange(height * SS) + 0.5) / SS - 0.5
    return np.meshgrid(u, v)


def junction_patch(kind, width, height, centre, rng):
    """One junction at `centre` under a random rotation and skew.  kind 'saddle': an X-junction (two opposite dark quadrants);
    'ell': a tag-style L-corner (one dark quadrant)."""
    u, v = subsample_grid(width, height)
    th = rng.uniform(0, 2 * np.pi)
    skew = rng.uniform(-0.35, 0.35)
    A = np.array([[np.cos(th), np.sin(th)], [-np.sin(th) + skew * np.cos(th), np.cos(th) + skew * np.sin(th)]])
    q0 = A[0, 0] * (u - centre[0]) + A[0, 1] * (v - centre[1])
    q1 = A[1, 0] * (u - centre[0]) + A[1, 1] * (v - centre[1])
    dark = (q0 * q1 > 0) if kind == "saddle" else ((q0 > 0) & (q1 > 0))
    return finish(np.where(dark, DARK, LIGHT), rng)


def padded(img, pitch, fill=7):
    """[..., height, width] -> [..., height, pitch], the padding bytes `fill` (never read by a correct implementation: the results
    with two fills are compared in the tests)."""
    out = np.full(img.shape[:-1] + (pitch,), fill, dtype=np.uint8)
    out[..., :img.shape[-1]] = img
    return out


@functools.lru_cache(maxsize=None)
def batch(size):
    """3 images of SIZES[size] holding 0, 1 and 257 corners, offsets[0] = FIRST > 0; the corner array has FIRST rows ahead and 3 behind
    that no call may touch.  Image 1: a saddle; image 2: a saddle and an L-corner.  The 257 starts: 160 within 2.5 px of a junction,
    the rest anywhere in the image, the four borders and the four corners of the image among them."""
    width, height, pitch = SIZES[size]
    rng = np.random.default_rng(2400 + size)
    c1 = np.array([width * 0.45 + rng.uniform(-1, 1), height * 0.55 + rng.uniform(-1, 1)])
    cs = np.array([width * 0.3 + rng.uniform(-1, 1), height * 0.4 + rng.uniform(-1, 1)])
    ce = np.array([width * 0.72 + rng.uniform(-1, 1), height * 0.62 + rng.uniform(-1, 1)])
    img1 = junction_patch("saddle", width, height, c1, rng)
    # two junctions in one image: the saddle on the left half, the L-corner on the right
    a, b = junction_patch("saddle", width, height, cs, rng), junction_patch("ell", width, height, ce, rng)
    img2 = np.where(np.arange(width)[None, :] < width // 2, a, b).astype(np.uint8)
    img0 = junction_patch("ell", width, height, c1, rng)
    images = padded(np.stack([img0, img1, img2]), pitch)
    near = np.concatenate([cs + rng.uniform(-2.5, 2.5, (100, 2)), ce + rng.uniform(-2.5, 2.5, (60, 2))])
    e = 0.25
    border = np.array([[e, height / 2], [width - 1 + e, height / 2], [width / 2, e], [width / 2, height - 1 + e],
                       [0, 0], [width - 1 + e, 0], [0, height - 1 + e], [width - 1 + e, height - 1 + e]])
    anywhere = rng.uniform([0, 0], [width - 0.01, height - 0.01], (COUNTS[2] - len(near) - len(border), 2))
    starts2 = np.concatenate([near, border, anywhere])
    starts2 = np.clip(starts2, 0, [width - 0.01, height - 0.01])
    M = sum(COUNTS)
    corners = np.full((FIRST + M + 3, 2), -7.5, dtype=np.float32)
    corners[FIRST] = np.rint(c1)
    corners[FIRST + 1:FIRST + 1 + COUNTS[2]] = starts2[rng.permutation(COUNTS[2])]
    offsets = FIRST + np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    return dict(images=images, width=width, height=height, pitch=pitch, corners=corners, offsets=offsets,
                truth=dict(c1=c1, cs=cs, ce=ce))


@functools.lru_cache(maxsize=None)
def reference(size, win):
    """The restatement on batch(size) with WINDOWS[win] -> (results, traces: every iteration's err per corner)."""
    b = batch(size)
    traces = {}
    return ref.refine(b["images"], b["width"], b["corners"], b["offsets"], WINDOWS[win], traces), traces


def near_eps(traces, o, rel):
    """The corners with an iteration whose err lies within `rel` relative of eps^2: there the stopping test may fall either way
    under another summation order."""
    e2 = o.eps * o.eps
    return sorted(c for c, tr in traces.items() if any(abs(err - e2) <= rel * e2 for err in tr))


# ---------------------------------------------------------------------------------------------------------------------------------
# Edge cases: each a dict(images [n, h, pitch], width, corners [M, 2], offsets, options, expect: {corner index: status})
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ell_corners(n=40):
    """n images of 33 x 21 (pitch 40), one L-corner each, the start = the true corner rounded to integers; half-window 1."""
    rng = np.random.default_rng(2417)
    width, height, pitch = SIZES[0]
    truth = np.stack([rng.uniform(8, width - 8, n), rng.uniform(6, height - 6, n)], 1)
    images = padded(np.stack([junction_patch("ell", width, height, truth[i], rng) for i in range(n)]), pitch)
    return dict(images=images, width=width, corners=np.rint(truth).astype(np.float32), offsets=np.arange(n + 1, dtype=np.int64),
                options=ref.Options(1, 1), truth=truth)


@functools.lru_cache(maxsize=None)
def edge_cases():
    width, height, pitch = SIZES[0]
    rng = np.random.default_rng(2431)
    flat = np.full((1, height, pitch), 128, dtype=np.uint8)
    saddle = padded(junction_patch("saddle", width, height, (16.3, 10.6), rng)[None], pitch)
    one = np.array([0, 1], dtype=np.int64)
    out = {
        "flat": dict(images=flat, width=width, corners=np.array([[10.25, 9.5]], np.float32), offsets=one, options=ref.Options(3, 3),
                     expect=ref.SINGULAR),
        "max_iter_1": dict(images=saddle, width=width, corners=np.array([[15.0, 12.0]], np.float32), offsets=one,
                           options=ref.Options(3, 3, max_iter=1, eps=0.001), expect=ref.MAX_ITER),
        "converged": dict(images=saddle, width=width, corners=np.array([[16.0, 11.0]], np.float32), offsets=one, options=ref.Options(5, 5, eps=0.01),
                          expect=ref.CONVERGED),
        "nan": dict(images=saddle, width=width, corners=np.array([[np.nan, 4.0]], np.float32), offsets=one, options=ref.Options(3, 3),
                    expect=ref.NONFINITE),
        "inf": dict(images=saddle, width=width, corners=np.array([[4.0, np.inf]], np.float32), offsets=one, options=ref.Options(3, 3),
                    expect=ref.NONFINITE),
        "outside": dict(images=saddle, width=width, corners=np.array([[-1.0, 5.0]], np.float32), offsets=one, options=ref.Options(3, 3),
                        expect=ref.LEFT_IMAGE),
        "outside_far": dict(images=saddle, width=width, corners=np.array([[3e9, 5.0]], np.float32), offsets=one, options=ref.Options(3, 3),
                            expect=ref.LEFT_IMAGE),
        "at_width": dict(images=saddle, width=width, corners=np.array([[float(width), 5.0]], np.float32), offsets=one, options=ref.Options(3, 3),
                         expect=ref.LEFT_IMAGE),
    }
    out["leaving"] = leaving_case()
    return out


def leaving_case():
    """A start whose first step leaves the image: a saddle whose junction lies just outside the left border.  The candidates are tried
    in a fixed order and the first one on which the restatement leaves at its first step is the case."""
    width, height, pitch = SIZES[0]
    for k, (cx, sx, w) in enumerate([(-0.8, 1.0, 3), (-1.2, 1.0, 3), (-0.6, 0.0, 3), (-1.5, 1.0, 5), (-2.0, 2.0, 5), (-1.0, 0.0, 2)]):
        rng = np.random.default_rng(2450 + k)
        img = padded(junction_patch("saddle", width, height, (cx, 10.4), rng)[None], pitch)
        start = np.array([[sx, 10.0]], np.float32)
        o = ref.Options(w, w)
        x, y, st, it, _, _ = ref.refine_one(img[0], width, start[0], o)
        if st == ref.LEFT_IMAGE and it == 0:
            return dict(images=img, width=width, corners=start, offsets=np.array([0, 1], dtype=np.int64), options=o, expect=ref.LEFT_IMAGE)
    raise AssertionError("no candidate leaves the image at its first step")


# ---------------------------------------------------------------------------------------------------------------------------------
# Boards: a 5 x 4 inner-corner chessboard of 40 mm squares at 0.5 m, pinhole fx = fy = 150, 160 x 120
# ---------------------------------------------------------------------------------------------------------------------------------
# The seeds, chosen on the restatement and on campose_ref.pnp_lsq alone (of seeds 1..10): refined / start RMS 0.11-0.13 at half-window 3
# and 0.08-0.10 at 5, and the least-squares pose from the refined corners closer to the truth than from the rounded ones by more than 3x
# in translation and in rotation.  (Left out: seeds 2 and 4, whose steep tilt gives 0.24 at half-window 3, and seed 3,
# where the rounded corners' pose happens to lie 0.31 degrees from the truth and the refined ones' 0.46.)
BOARD_SEEDS = (1, 5, 7, 8)
PROJ, DIST = (150.0, 150.0, 79.5, 59.5), (0.0, 0.0, 0.0, 0.0)
BOARD_W, BOARD_H = 160, 120
SQUARE = 0.04
INNER = (5, 4)


def render_chessboard(width, height, proj, inner, square, R, t, rng):
    """A chessboard of inner[0] x inner[1] inner corners (one more square each way, light around it) at the pose (R, t) of the board in
    the camera frame, seen by the pinhole camera `proj` -> dict(image [height, width] uint8, truth [n, 2] pixels, board_xy [n, 2] metres)."""
    u, v = subsample_grid(width, height)
    m = campose_ref.lift(campose_ref.PINHOLE, proj, DIST, np.stack([u.ravel(), v.ravel()], 1))
    d = np.concatenate([m, np.ones((len(m), 1))], 1)  # the rays
    # lambda d = R X + t with X_z = 0:  lambda = (R^T t)_z / (R^T d)_z
    Rt_t = R.T @ t
    Rt_d = d @ R
    lam = Rt_t[2] / Rt_d[:, 2]
    X = lam[:, None] * Rt_d - Rt_t
    ix, iy = np.floor(X[:, 0] / square).astype(int), np.floor(X[:, 1] / square).astype(int)
    on_board = (ix >= -1) & (ix < inner[0]) & (iy >= -1) & (iy < inner[1])
    dark = on_board & (((ix + iy) & 1) == 0)
    hi = np.where(dark, DARK, LIGHT).reshape(u.shape)
    gx, gy = np.meshgrid(np.arange(inner[0]), np.arange(inner[1]))
    board_xy = np.stack([gx.ravel() * square, gy.ravel() * square], 1)
    P = np.concatenate([board_xy, np.zeros((len(board_xy), 1))], 1) @ R.T + t
    truth = campose_ref.project(campose_ref.PINHOLE, proj, DIST, P)
    return dict(image=finish(hi, rng), truth=truth, board_xy=board_xy.astype(np.float32))


@functools.lru_cache(maxsize=None)
def board_scene(seed):
    """-> dict(image [120, 160] uint8, truth [20, 2] pixels, board_xy [20, 2] metres, R, t: the board in the camera frame)."""
    rng = np.random.default_rng(2460 + seed)
    R = campose_ref.rotvec_to_R(rng.uniform(-0.25, 0.25, 3))
    centre = np.array([(INNER[0] - 1) / 2 * SQUARE, (INNER[1] - 1) / 2 * SQUARE, 0.0])
    t = np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), 0.5]) - R @ centre
    return dict(render_chessboard(BOARD_W, BOARD_H, PROJ, INNER, SQUARE, R, t, rng), R=R, t=t)


# ---------------------------------------------------------------------------------------------------------------------------------
# The host shim (tests/shim/subpix_shim.cpp), for the host tests and as the GPU tests' reference
# ---------------------------------------------------------------------------------------------------------------------------------
KEYS = ("corners", "status", "iterations", "strength")


def options_c(o):
    """A subpix_ref.Options as clc_subpix_options."""
    from camlasercalibratool_amd import _capi
    return _capi.SubpixOptions(o.win_x, o.win_y, o.zero_x, o.zero_y, o.max_iter, 0, o.eps)


def build_shim(path):
    import ctypes
    import os
    import subprocess
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim", "subpix_shim.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", src, "-o", path])
    return ctypes.CDLL(path)


def shim_refine(L, images, width, corners, offsets, o, in_place=False):
    """shim_corner_subpix -> dict, the keys of Solver.corner_subpix (rows outside the offsets: the input, -99, 0, NaN)."""
    import ctypes as C
    V = lambda a: a.ctypes.data_as(C.c_void_p)
    img = np.ascontiguousarray(images, dtype=np.uint8)
    cin = np.array(corners, dtype=np.float32).reshape(-1, 2)
    out = cin if in_place else cin.copy()
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    st = np.full(len(cin), -99, dtype=np.int32); it = np.zeros(len(cin), dtype=np.int32); lam = np.full(len(cin), np.nan)
    oc = options_c(o)
    L.shim_corner_subpix(C.byref(oc), V(img), C.c_int32(width), C.c_int32(img.shape[1]), C.c_longlong(img.shape[2]), C.c_longlong(img.shape[0]),
                         V(cin), V(off), V(out), V(st), V(it), V(lam))
    return dict(corners=out, status=st, iterations=it, strength=lam)


def same_bits(a, b):
    """Two result dicts equal bit for bit (NaN equal to NaN of the same bits)."""
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in KEYS)


def rms(a, b):
    return float(np.sqrt(np.mean(np.sum((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2, axis=1))))
