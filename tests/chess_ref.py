"""K25 restated in numpy from its contract (the response, the candidates per image, the ordering into the board's grid),
independent of the C++: whole-image array arithmetic for the response and the suppression, a sort for the selection, LAPACK solves for
the homographies.

Integer pixel coordinates are pixel centres.  R5 = 5 SR - 5 DR - |5 ring - 16 loc| in exact integers on the domain
5 <= x < width - 5, 5 <= y < height - 5."""
from __future__ import annotations

import itertools
from dataclasses import dataclass

import numpy as np

RING = [(0, -5), (2, -5), (3, -3), (5, -2), (5, 0), (5, 2), (3, 3), (2, 5), (0, 5), (-2, 5), (-3, 3), (-5, 2), (-5, 0), (-5, -2), (-3, -3),
        (-2, -5)]
CROSS = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)]
MAX_CANDIDATES, RAW_CAP = 1024, 4096
OK, FOUND, TOO_FEW, NO_GRID, OVERFLOW = 1, 1, 0, -1, -2


@dataclass(frozen=True)
class Options:
    threshold: int = 500
    nms_radius: int = 3
    rel_permille: int = 250
    max_per_image: int = 256


def response(img):
    """[height, width] uint8 -> R5 [height - 10, width - 10] int64 on the domain (entry [y - 5, x - 5]); an empty array where the domain is."""
    I = np.asarray(img).astype(np.int64)
    h, w = I.shape
    if h < 11 or w < 11:
        return np.zeros((0, 0), np.int64)
    s = [I[5 + dy:h - 5 + dy, 5 + dx:w - 5 + dx] for dx, dy in RING]
    sr = sum(np.abs((s[n] + s[n + 8]) - (s[n + 4] + s[n + 12])) for n in range(4))
    dr = sum(np.abs(s[n] - s[n + 8]) for n in range(8))
    ring = sum(s)
    loc = sum(I[5 + dy:h - 5 + dy, 5 + dx:w - 5 + dx] for dx, dy in CROSS)
    return 5 * sr - 5 * dr - np.abs(5 * ring - 16 * loc)


def raw_candidates(R, threshold, r):
    """The domain's R5 -> the raw candidates as (x, y, R5) image coordinates, in raster order."""
    if R.size == 0:
        return np.zeros((0, 3), np.int64)
    h, w = R.shape
    P = np.full((h + 2 * r, w + 2 * r), -10 ** 9, np.int64)  # outside the domain: no pixel, never a rival
    P[r:r + h, r:r + w] = R
    keep = R >= threshold
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx == 0 and dy == 0:
                continue
            N = P[r + dy:r + dy + h, r + dx:r + dx + w]
            after = dy > 0 or (dy == 0 and dx > 0)
            keep &= (N < R) | ((N == R) & after)
    y, x = np.nonzero(keep)
    return np.stack([x + 5, y + 5, R[y, x]], 1)


def select(raw, o):
    """-> (kept [k, 3] ordered by (-R5, y, x) and cut to max_per_image, status)."""
    if len(raw) > RAW_CAP:
        return raw[:0], OVERFLOW
    if len(raw) == 0:
        return raw, OK
    m = int(raw[:, 2].max())
    kept = raw[[1000 * int(v) >= o.rel_permille * m for v in raw[:, 2]]]
    order = np.lexsort((kept[:, 0], kept[:, 1], -kept[:, 2]))
    return kept[order][:o.max_per_image], OK


def detect(images, width, o=Options()):
    """images [n, height, pitch] uint8 -> the dict of Solver.chess_corners."""
    images = np.asarray(images)
    n, stride = images.shape[0], o.max_per_image
    xy = np.full((n, stride, 2), np.nan, np.float32); r5 = np.zeros((n, stride), np.int32)
    count = np.zeros(n, np.int32); count_raw = np.zeros(n, np.int32); status = np.zeros(n, np.int32)
    for k in range(n):
        raw = raw_candidates(response(images[k][:, :width]), o.threshold, o.nms_radius)
        kept, status[k] = select(raw, o)
        count[k], count_raw[k] = len(kept), len(raw)
        xy[k, :len(kept)] = kept[:, :2]
        r5[k, :len(kept)] = kept[:, 2]
    return dict(xy=xy, r5=r5, count=count, count_raw=count_raw, status=status)


# ---------------------------------------------------------------------------------------------------------------------------------
# The ordering
# ---------------------------------------------------------------------------------------------------------------------------------
def cross(a, b, c):
    return (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0])


def hull(points):
    """Integer points [(x, y)] -> the indices of the convex hull's vertices, from the smallest in (x, y), every turn a positive cross
    product; collinear points are no vertices (monotone chain)."""
    order = sorted(set((int(p[0]), int(p[1])) for p in points))
    first = {}
    for k, p in enumerate(points):
        first.setdefault((int(p[0]), int(p[1])), k)
    if len(order) < 3:
        return [first[p] for p in order]
    def chain(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and cross(out[-2], out[-1], p) <= 0:
                out.pop()
            out.append(p)
        return out
    lower, upper = chain(order), chain(order[::-1])
    return [first[p] for p in lower[:-1] + upper[:-1]]


def largest_quad(P, hv):
    """The 4 hull vertices (positions in hv, increasing) of the largest shoelace area; the first tuple on ties."""
    combos = np.array(list(itertools.combinations(range(len(hv)), 4)), dtype=np.int64)
    X, Y = P[hv, 0][combos], P[hv, 1][combos]
    area = sum(X[:, k] * Y[:, (k + 1) % 4] - X[:, (k + 1) % 4] * Y[:, k] for k in range(4))
    return combos[int(np.argmax(area))]


def dlt_rows(g, p):
    X, Y = g
    u, v = p
    return [[X, Y, 1, 0, 0, 0, -u * X, -u * Y], [0, 0, 0, X, Y, 1, -v * X, -v * Y]], [u, v]


def homography(grid, px):
    A, b = [], []
    for g, p in zip(grid, px):
        r, c = dlt_rows(g, p)
        A += r; b += c
    A, b = np.array(A, float), np.array(b, float)
    h = np.linalg.solve(A, b) if len(A) == 8 else np.linalg.lstsq(A, b, rcond=None)[0]
    return np.append(h, 1.0).reshape(3, 3)


def apply_h(H, g):
    q = np.concatenate([g, np.ones((len(g), 1))], 1) @ H.T
    return q[:, :2] / q[:, 2:3]


RATIOS = []  # every pass's largest distance / spacing ratio since the list was last cleared (the tests look for decisions near tol)


def match(H, nodes, cand, cols, rows, tol):
    pred = apply_h(H, nodes).reshape(rows, cols, 2)
    sp = min(np.linalg.norm(pred[:, 1:] - pred[:, :-1], axis=2).min(), np.linalg.norm(pred[1:] - pred[:-1], axis=2).min())
    d = np.linalg.norm(pred.reshape(-1, 1, 2) - cand[None], axis=2)
    m = d.argmin(axis=1)
    far = d[np.arange(len(m)), m].max()
    RATIOS.append(float(far / sp))
    return len(set(m.tolist())) == len(m) and far <= tol * sp, m, far / sp


def order_image(xy, cols, rows, tol=0.3):
    """The cols rows strongest candidates [n, 2] (integer pixels) -> (status, index [n] or None, n_labelings, worst)."""
    n = cols * rows
    P = np.rint(np.asarray(xy[:n], float)).astype(np.int64)
    hv = hull(P)
    if len(hv) < 4:
        return NO_GRID, None, 0, np.nan
    hv = np.array(hv)
    quad = hv[largest_quad(P, hv)]
    # the fits run on coordinates brought to [-1, 1] (the algebraic least squares depends on the scaling; the ratios tested do not):
    # the nodes (2 j / (cols - 1) - 1, 2 i / (rows - 1) - 1), the pixels about their mean over their largest deviation in x or y
    gx, gy = np.meshgrid(2.0 * np.arange(cols) / (cols - 1) - 1.0, 2.0 * np.arange(rows) / (rows - 1) - 1.0)
    nodes = np.stack([gx.ravel(), gy.ravel()], 1)
    corners = nodes[[0, cols - 1, n - 1, n - cols]]
    mean = P.astype(float).mean(axis=0)
    cand = (P - mean) / max(1.0, np.abs(P - mean).max())
    valid = []
    for k in range(4):
        try:
            H = homography(corners, cand[np.roll(quad, -k)])
            ok, m, worst = match(H, nodes, cand, cols, rows, tol)
            if not ok:
                continue
            ok, m, worst = match(homography(nodes, cand[m]), nodes, cand, cols, rows, tol)
        except np.linalg.LinAlgError:
            continue
        if ok:
            valid.append((int(P[m[0], 1]), int(P[m[0], 0]), k, m, worst))
    if not valid:
        return NO_GRID, None, 0, np.nan
    best = min(valid, key=lambda v: v[:3])
    return FOUND, best[3].astype(np.int32), len(valid), float(best[4])


def order(cand_xy, count, cols, rows, status=None, tol=0.3):
    """-> the dict of camlasercalibratool_amd.chessboard_order."""
    n_img, per = len(cand_xy), cols * rows
    index = np.full((n_img, per), -1, np.int32); st = np.zeros(n_img, np.int32); lab = np.zeros(n_img, np.int32); worst = np.full(n_img, np.nan)
    for k in range(n_img):
        if status is not None and status[k] == OVERFLOW:
            st[k] = OVERFLOW
        elif count[k] < per:
            st[k] = TOO_FEW
        else:
            st[k], ix, lab[k], worst[k] = order_image(cand_xy[k], cols, rows, tol)
            if ix is not None:
                index[k] = ix
    return dict(index=index.reshape(n_img, rows, cols), status=st, n_labelings=lab, worst=worst)
