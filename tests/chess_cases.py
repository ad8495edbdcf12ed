"""Seeded inputs of the K25 tests (no image is committed), built on the renderer of tests/subpix_cases.py: the detection cases every
form runs on, the boards of the ordering tests, and the host shim (tests/shim/chess_shim.cpp) as the GPU tests' reference."""
from __future__ import annotations

import functools

import numpy as np

import campose_ref
import chess_ref as ref
import subpix_cases as sp

TILE_W, TILE_H = 64, 16   # the kernel's tile (asserted against the shim's)
CHUNK = 170               # images per launch of the device forms
COUNTS = sp.COUNTS        # 0, 1, 257
SCENE_SEEDS = tuple(range(12))
KEYS = ("xy", "r5", "count", "count_raw", "status")
# the names of cases() (the tests are parametrised by them without rendering anything at collection time)
NAMES = ("empty_domain", "junctions0", "junctions1", "junctions_low", "max_1", "max_1024", "one_pixel", "overflow", "rel_0", "rel_1000", "scenes",
         "tie_far", "tie_mid", "tie_near", "tile_edges", "tile_edges_r7")


def clean_saddle(width, height, centre):
    """A 45-degree X-junction at `centre` without noise (dark where |x - cx| > |y - cy|): the renderer's blur and pixel mean, rounded."""
    u, v = sp.subsample_grid(width, height)
    hi = np.where(np.abs(u - centre[0]) > np.abs(v - centre[1]), sp.DARK, sp.LIGHT)
    hi = sp._blur_axis(sp._blur_axis(hi, sp.BLUR_PX * sp.SS, 0), sp.BLUR_PX * sp.SS, 1)
    img = hi.reshape(height, sp.SS, width, sp.SS).mean(axis=(1, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def tie_image():
    """61 x 47: the same noise-free saddle twice, at (28, 23) and (32, 23), the left copy the mirror image of the right one about the
    column x = 30, bit for bit.  R5 is invariant under that mirror and under the one about the row y = 23, so its maxima come in
    equal fours: (28, 22), (32, 22), (28, 24), (32, 24), all R5 = 1117 — ties 4 pixels apart in x and 2 in y."""
    width, height, cx = 61, 47, 30
    img = clean_saddle(width, height, (cx + 2.0, 23.0))
    img[:, :cx] = img[:, :cx:-1]
    assert np.array_equal(img, img[:, ::-1])
    return img[None]


@functools.lru_cache(maxsize=None)
def edge_images():
    """100 x 40, one saddle each, the junctions on both sides of the tile edges x = 63 | 64 and y = 15 | 16, 31 | 32."""
    rng = np.random.default_rng(2501)
    centres = [(63, 15), (64, 16), (63, 16), (64, 15), (30, 31), (30, 32), (63, 31), (64, 32), (63.5, 15.5), (20, 15), (20, 16)]
    return np.stack([sp.junction_patch("saddle", 100, 40, c, rng) for c in centres])


@functools.lru_cache(maxsize=None)
def scenes():
    return np.stack([sp.board_scene(s)["image"] for s in SCENE_SEEDS])


@functools.lru_cache(maxsize=None)
def noise_image():
    return np.random.default_rng(2502).integers(0, 256, (1, 400, 640), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(images [n, height, pitch] uint8, width, options)."""
    rng = np.random.default_rng(2503)
    out = {}
    for k in range(len(sp.SIZES)):
        b = sp.batch(k)
        out["junctions%d" % k] = dict(images=b["images"], width=b["width"], options=ref.Options())
    out["junctions_low"] = dict(images=sp.batch(0)["images"], width=sp.SIZES[0][0], options=ref.Options(threshold=1, nms_radius=1, rel_permille=0))
    out["scenes"] = dict(images=scenes(), width=sp.BOARD_W, options=ref.Options())
    out["one_pixel"] = dict(images=sp.junction_patch("saddle", 11, 11, (5.2, 4.9), rng)[None], width=11, options=ref.Options())
    out["empty_domain"] = dict(images=sp.junction_patch("saddle", 10, 30, (5.0, 15.0), rng)[None], width=10, options=ref.Options())
    out["tie_far"] = dict(images=tie_image(), width=61, options=ref.Options(nms_radius=1))
    out["tie_mid"] = dict(images=tie_image(), width=61, options=ref.Options(nms_radius=3))
    out["tie_near"] = dict(images=tie_image(), width=61, options=ref.Options(nms_radius=7))
    out["tile_edges"] = dict(images=edge_images(), width=100, options=ref.Options())
    out["tile_edges_r7"] = dict(images=sp.padded(edge_images(), 107), width=100, options=ref.Options(nms_radius=7, threshold=50))
    out["overflow"] = dict(images=noise_image(), width=640, options=ref.Options(threshold=1, nms_radius=1))
    out["rel_0"] = dict(images=scenes()[:3], width=sp.BOARD_W, options=ref.Options(threshold=20, rel_permille=0))
    out["rel_1000"] = dict(images=scenes()[:3], width=sp.BOARD_W, options=ref.Options(rel_permille=1000))
    out["max_1"] = dict(images=scenes()[:3], width=sp.BOARD_W, options=ref.Options(max_per_image=1))
    out["max_1024"] = dict(images=scenes()[:2], width=sp.BOARD_W, options=ref.Options(threshold=1, nms_radius=1, rel_permille=0, max_per_image=1024))
    assert sorted(out) == sorted(NAMES)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    c = cases()[name]
    return ref.detect(c["images"], c["width"], c["options"])


@functools.lru_cache(maxsize=None)
def batch(count):
    """`count` images of 160 x 120: the 12 scenes in turn."""
    return scenes()[np.arange(count) % len(SCENE_SEEDS)]


# ---------------------------------------------------------------------------------------------------------------------------------
# The boards of the ordering tests
# ---------------------------------------------------------------------------------------------------------------------------------
TILTED_PROJ, TILTED_W, TILTED_H, TILTED_SQUARE = (300.0, 300.0, 160.0, 120.0), 320, 240, 0.03


@functools.lru_cache(maxsize=None)
def tilted_boards():
    """16 boards of 320 x 240: 9 x 6 and 6 x 6 inner corners in turn, square 0.03 m, the in-plane rotation uniform over +-pi, the tilt
    +-0.5 rad about x and about y, the depth 0.45-0.6 m -> [dict(image, truth, inner)]."""
    rng = np.random.default_rng(7)
    out = []
    for k in range(16):
        inner = (9, 6) if k % 2 == 0 else (6, 6)
        R = campose_ref.rotvec_to_R(np.array([0.0, 0.0, rng.uniform(-np.pi, np.pi)])) @ campose_ref.rotvec_to_R(
            np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 0.0]))
        centre = np.array([(inner[0] - 1) / 2 * TILTED_SQUARE, (inner[1] - 1) / 2 * TILTED_SQUARE, 0.0])
        t = np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), rng.uniform(0.45, 0.6)]) - R @ centre
        s = sp.render_chessboard(TILTED_W, TILTED_H, TILTED_PROJ, inner, TILTED_SQUARE, R, t, rng)
        out.append(dict(image=s["image"], truth=s["truth"], inner=inner))
    return out


def grid_rotations(cols, rows):
    """The right-handed relabelings of a cols x rows grid onto itself: the permutations p with new node m = old node p[m]."""
    idx = np.arange(cols * rows).reshape(rows, cols)
    out = [idx, idx[::-1, ::-1]]
    if cols == rows:
        out += [np.rot90(idx, 1), np.rot90(idx, 3)]
    return [p.ravel() for p in out]


def relabel_truth(truth, cols, rows, cand_px, with_permutation=False):
    """`truth` [cols rows, 2] relabelled as the ordering's rule says: of the right-handed relabelings the one whose node (0, 0) — taken
    at the detected integer pixel nearest to it — comes first in raster order (y, then x).  with_permutation: -> (truth[p], p)."""
    best = None
    for p in grid_rotations(cols, rows):
        t0 = truth[p[0]]
        near = cand_px[np.argmin(np.linalg.norm(cand_px - t0, axis=1))]
        key = (float(near[1]), float(near[0]))
        if best is None or key < best[0]:
            best = (key, truth[p], p)
    return (best[1], best[2]) if with_permutation else best[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# The host shim
# ---------------------------------------------------------------------------------------------------------------------------------
def options_c(o):
    from camlasercalibratool_amd import _capi
    return _capi.ChessOptions(o.threshold, o.nms_radius, o.rel_permille, o.max_per_image, 0)


def build_shim(path):
    import ctypes
    import os
    import subprocess
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim", "chess_shim.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", path])
    L = ctypes.CDLL(path)
    assert (L.shim_chess_tile_w(), L.shim_chess_tile_h()) == (TILE_W, TILE_H)
    return L


def empty_result(n, stride):
    """What Solver.chess_corners hands to the library: every entry a value no call writes."""
    return dict(xy=np.full((n, stride, 2), -7.0, np.float32), r5=np.full((n, stride), -7, np.int32), count=np.full(n, -7, np.int32),
                count_raw=np.full(n, -7, np.int32), status=np.full(n, -99, np.int32))


def shim_detect(L, images, width, o, chunk=CHUNK):
    """shim_chess_corners -> the dict of Solver.chess_corners."""
    import ctypes as C
    V = lambda a: a.ctypes.data_as(C.c_void_p)
    img = np.ascontiguousarray(images, dtype=np.uint8)
    r = empty_result(img.shape[0], o.max_per_image)
    oc = options_c(o)
    L.shim_chess_corners(C.byref(oc), V(img), C.c_int32(width), C.c_int32(img.shape[1]), C.c_longlong(img.shape[2]), C.c_longlong(img.shape[0]),
                         C.c_longlong(chunk), V(r["xy"]), V(r["r5"]), V(r["count"]), V(r["count_raw"]), V(r["status"]))
    return r


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in KEYS)


def assert_same_bits(got, want, what):
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape)
        bad = np.flatnonzero(a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1))
        assert len(bad) == 0, (what, k, len(bad), a.reshape(-1)[:8], b.reshape(-1)[:8])
