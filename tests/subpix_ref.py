"""Test-side restatement (numpy) of K24, cv::cornerSubPix as DESIGN.md K24 states it: the getRectSubPix patch with one fractional
pair and a replicated border, central differences, the Gaussian mask, five double sums, the 2 x 2 solve and the four ways out.  Every
float32 step is a numpy float32 operation and every double step a float64 one, so the restatement differs from the kernel's code
(csrc/clc_subpix.hpp) in the ORDER of the five sums only: numpy's pairwise sum over the whole window here, a lane's strided partial
sums and a butterfly there."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

CONVERGED, MAX_ITER, SINGULAR, LEFT_IMAGE, REVERTED, NONFINITE = 1, 0, -1, -2, -3, -4
MAX_WIN = 15
F = np.float32
DBL_EPS = 2.220446049250313e-16


@dataclass(frozen=True)
class Options:
    win_x: int = 3
    win_y: int = 3
    zero_x: int = -1
    zero_y: int = -1
    max_iter: int = 30
    eps: float = 0.1


def table(w):
    """v[j] = expf(-x^2), x = (float)(j - w) / w: x and x^2 in float32; exp in double, rounded once to float32."""
    x = (np.arange(2 * w + 1) - w).astype(F) / F(w)
    return np.array([F(math.exp(float(-(v * v)))) for v in x], dtype=F)


def zone_of(o):
    on = o.zero_x >= 0 and o.zero_y >= 0 and 2 * o.zero_x + 1 < 2 * o.win_x + 1 and 2 * o.zero_y + 1 < 2 * o.win_y + 1
    return (o.zero_x, o.zero_y) if on else (-1, -1)


def mask_of(o):
    """mask[i][j] = vy[i] * vx[j] as a float32 product, 0 inside the zero zone -> float32 [2 wy + 1, 2 wx + 1]."""
    m = table(o.win_y)[:, None] * table(o.win_x)[None, :]
    zx, zy = zone_of(o)
    if zx >= 0:
        m[o.win_y - zy:o.win_y + zy + 1, o.win_x - zx:o.win_x + zx + 1] = 0
    return m.astype(F)


def inside(x, y, width, height):
    return bool(x >= 0 and x < F(width) and y >= 0 and y < F(height))


def refine_one(img, width, start, o, mask=None, trace=None):
    """One corner on img [height, pitch] uint8 -> (x, y, status, iterations, strength, scale); scale = (a + c) / sum m at the last
    evaluated iterate, what the rounding of the strength is relative to.  trace: a list that gets every iteration's err."""
    height = img.shape[0]
    wx, wy = o.win_x, o.win_y
    mask = mask_of(o) if mask is None else mask
    msum = float(mask.astype(np.float64).sum())  # (row-major in the kernel's code; see subpix_cases: the strength is compared to 1e-12)
    md = mask.astype(np.float64)
    px = (np.arange(2 * wx + 1) - wx).astype(np.float64)[None, :]
    py = (np.arange(2 * wy + 1) - wy).astype(np.float64)[:, None]
    sx, sy = F(start[0]), F(start[1])
    if not (np.isfinite(sx) and np.isfinite(sy)):
        return sx, sy, NONFINITE, 0, float("nan"), float("nan")
    if not inside(sx, sy, width, height):
        return sx, sy, LEFT_IMAGE, 0, float("nan"), float("nan")
    cx, cy = sx, sy
    status, it, strength, scale = MAX_ITER, 0, float("nan"), float("nan")
    eps2 = o.eps * o.eps
    while True:
        tlx, tly = F(cx - F(wx + 1)), F(cy - F(wy + 1))
        fx, fy = np.floor(tlx), np.floor(tly)
        a, b = F(tlx - fx), F(tly - fy)
        one = F(1.0)
        w00, w01, w10, w11 = F((one - a) * (one - b)), F(a * (one - b)), F((one - a) * b), F(a * b)
        xs = np.clip(int(fx) + np.arange(2 * wx + 4), 0, width - 1)
        ys = np.clip(int(fy) + np.arange(2 * wy + 4), 0, height - 1)
        nb = img[np.ix_(ys, xs)].astype(F)
        S = ((nb[:-1, :-1] * w00 + nb[:-1, 1:] * w01) + nb[1:, :-1] * w10) + nb[1:, 1:] * w11
        assert S.dtype == F
        tgx = (S[1:-1, 2:] - S[1:-1, :-2]).astype(np.float64)
        tgy = (S[2:, 1:-1] - S[:-2, 1:-1]).astype(np.float64)
        gxx, gxy, gyy = (tgx * tgx) * md, (tgx * tgy) * md, (tgy * tgy) * md
        A, B, C = float(gxx.sum()), float(gxy.sum()), float(gyy.sum())
        bb1, bb2 = float((gxx * px + gxy * py).sum()), float((gxy * px + gyy * py).sum())
        dac = A - C
        strength = (((A + C) - math.sqrt(dac * dac + (4.0 * B) * B)) / 2.0) / msum
        scale = (A + C) / msum
        det = A * C - B * B
        if abs(det) <= DBL_EPS * DBL_EPS:
            status = SINGULAR
            break
        s = 1.0 / det
        nx = F((float(cx) + (C * s) * bb1) - (B * s) * bb2)
        ny = F((float(cy) - (B * s) * bb1) + (A * s) * bb2)
        ex, ey = float(nx) - float(cx), float(ny) - float(cy)
        err = ex * ex + ey * ey
        if trace is not None:
            trace.append(err)
        cx, cy = nx, ny
        if not inside(cx, cy, width, height):
            status = LEFT_IMAGE
            break
        it += 1
        if not err > eps2:
            status = CONVERGED
            break
        if it >= o.max_iter:
            break
    if abs(F(cx - sx)) > F(wx) or abs(F(cy - sy)) > F(wy):
        cx, cy, status = sx, sy, REVERTED
    return cx, cy, status, it, strength, scale


def refine(images, width, corners, offsets, o, traces=None):
    """clc_corner_subpix: images [n, height, pitch] uint8, corners [M', 2] float32 indexed by the absolute offsets [n + 1] ->
    dict(corners, status, iterations, strength, scale) for the corners [offsets[0], offsets[-1]) (the other rows: the input, -99, 0, NaN)."""
    corners = np.asarray(corners, dtype=F).reshape(-1, 2)
    out = dict(corners=corners.copy(), status=np.full(len(corners), -99, np.int32), iterations=np.zeros(len(corners), np.int32),
               strength=np.full(len(corners), np.nan), scale=np.full(len(corners), np.nan))
    mask = mask_of(o)
    for i in range(len(offsets) - 1):
        for c in range(int(offsets[i]), int(offsets[i + 1])):
            tr = [] if traces is not None else None
            x, y, st, it, lam, sc = refine_one(images[i], width, corners[c], o, mask, tr)
            out["corners"][c] = (x, y)
            out["status"][c], out["iterations"][c], out["strength"][c] = st, it, lam
            out["scale"][c] = sc
            if traces is not None:
                traces[c] = tr
    return out
