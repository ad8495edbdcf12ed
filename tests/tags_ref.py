"""K27 restated in numpy from its contract (directed edges between K25's candidates, the quads as directed 4-cycles, the
decode of each quad against the family, the grid by tag id, the compaction), independent of the C++: python integers for the edge
samples, a set of canonical cycles for the quads, a LAPACK solve for the homography, numpy rotations for the four readings of a word.

Everything before the homography is exact integer arithmetic; the homography only chooses the pixel nearest each cell centre, and
HALF records how close any sample coordinate came to a half-integer (the tests require a margin, so that rint cannot differ), and
AMBIGUOUS, for the scenes whose quads are too many for such a margin, the samples at a half-integer where that could change a cell."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import chess_ref

S, MAX_OUT = 8, 4
OK, OVERFLOW = 1, -2
HALF = []  # min |frac(coordinate) - 0.5| of every decoded quad since the list was last cleared
AMBIGUOUS = []  # per decoded quad since the list was last cleared: its samples within TIE of a half-integer that rint could decide either way
TIE = 1e-9


@dataclass(frozen=True)
class Options:
    min_side_px: int = 16
    max_side_px: int = 0
    contrast: int = 40
    max_border_errors: int = 0
    max_quads: int = 256


@dataclass(frozen=True)
class Family:
    side: int
    border: int
    codes: tuple
    max_hamming: int = 1


CHESS = chess_ref.Options(max_per_image=1024)  # K25's defaults with every slot


def rdiv(a, den):
    return (2 * a + den) // (2 * den)


def edge(img, width, p, q, fam, o):
    """The directed edge p -> q (integer pixels) -> (sum inside, sum outside) or None."""
    dd = fam.side + 2 * fam.border
    den = 4 * S * dd
    vx, vy = q[0] - p[0], q[1] - p[1]
    hi = o.max_side_px or min(width, img.shape[0])
    if not o.min_side_px ** 2 <= vx * vx + vy * vy <= hi ** 2:
        return None
    nx, ny = -vy, vx
    ins, outs = [], []
    for i in range(1, S - 1):
        bx, by = p[0] * den + vx * (2 * i + 1) * 2 * dd, p[1] * den + vy * (2 * i + 1) * 2 * dd
        for sign, dst in ((1, ins), (-1, outs)):
            x, y = rdiv(bx + sign * nx * fam.border * 2 * S, den), rdiv(by + sign * ny * fam.border * 2 * S, den)
            if not (0 <= x < width and 0 <= y < img.shape[0]):
                return None
            dst.append(int(img[y, x]))
    if min(outs) - max(ins) < o.contrast:
        return None
    return sum(ins), sum(outs)


def edges(img, width, cand, fam, o):
    """-> ({(p, q): (sum inside, sum outside)} of the kept edges, the number dropped)."""
    kept, dropped = {}, 0
    P = [(int(x), int(y)) for x, y in cand]
    A = np.array(P, dtype=np.int64).reshape(-1, 2)
    hi = o.max_side_px or min(width, img.shape[0])
    for p in range(len(P)):
        d2 = ((A - A[p]) ** 2).sum(axis=1)
        n_out = 0
        for q in np.flatnonzero((d2 >= o.min_side_px ** 2) & (d2 <= hi ** 2)):
            if q == p:
                continue
            e = edge(img, width, P[p], P[int(q)], fam, o)
            if e is None:
                continue
            if n_out < MAX_OUT:
                kept[(p, int(q))] = e
                n_out += 1
            else:
                dropped += 1
    return kept, dropped


def quads(kept):
    """The directed 4-cycles over distinct slots, each from its smallest slot, in lexicographic order."""
    succ = {}
    for p, q in kept:
        succ.setdefault(p, []).append(q)
    found = set()
    for a in succ:
        for b in succ[a]:
            for c in succ.get(b, ()):
                for d in succ.get(c, ()):
                    if a in succ.get(d, ()) and len({a, b, c, d}) == 4:
                        cyc = (a, b, c, d)
                        k = cyc.index(min(cyc))
                        found.add(cyc[k:] + cyc[:k])
    return sorted(found)


def cells_of(word, d):
    return np.array([(int(word) >> (d * d - 1 - k)) & 1 for k in range(d * d)], dtype=np.int64).reshape(d, d)


def word_of(cells):
    w = 0
    for v in np.asarray(cells).reshape(-1):
        w = (w << 1) | int(v)
    return w


def undecidable(img, width, uv, thr):
    """The samples uv [m, 2] whose pixel is not decidable: a coordinate within TIE of a half-integer (either neighbour may be the nearest
    pixel) and the two or four pixels it may round to not all inside the image, or inside and not all on one side of 48 I > thr -> their
    number.  (All of them outside is decidable: the quad is refused either way.)"""
    n = 0
    for x, y in uv:
        xs = [np.floor(x), np.floor(x) + 1] if abs(x - np.floor(x) - 0.5) <= TIE else [np.rint(x)]
        ys = [np.floor(y), np.floor(y) + 1] if abs(y - np.floor(y) - 0.5) <= TIE else [np.rint(y)]
        if len(xs) * len(ys) == 1:
            continue
        inside = [0 <= i < width and 0 <= j < img.shape[0] for j in ys for i in xs]
        if not any(inside):
            continue
        if not all(inside) or len({48 * int(img[int(j), int(i)]) > thr for j in ys for i in xs}) != 1:
            n += 1
    return n


def decode(img, width, cand, quad, kept, fam, o):
    """-> None (rejected) or (hamming, id, rotation) of the accepted decode."""
    d, b = fam.side, fam.border
    dd = d + 2 * b
    thr = sum(sum(kept[(quad[j], quad[(j + 1) % 4])]) for j in range(4))
    px = np.array([cand[s] for s in quad], dtype=float)
    try:
        H = chess_ref.homography(np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]), px)
    except np.linalg.LinAlgError:
        return None
    centres = np.array([[(c + 0.5) / dd, (r + 0.5) / dd] for r in range(dd) for c in range(dd)])
    uv = chess_ref.apply_h(H, centres)
    if not np.isfinite(uv).all():
        return None
    HALF.append(float(np.abs(uv - np.floor(uv) - 0.5).min()))
    AMBIGUOUS.append(undecidable(img, width, uv, thr))
    ij = np.rint(uv).astype(np.int64)
    if (ij[:, 0] < 0).any() or (ij[:, 0] >= width).any() or (ij[:, 1] < 0).any() or (ij[:, 1] >= img.shape[0]).any():
        return None
    white = (48 * img[ij[:, 1], ij[:, 0]].astype(np.int64) > thr).astype(np.int64).reshape(dd, dd)
    ring = np.ones((dd, dd), bool)
    ring[b:dd - b, b:dd - b] = False
    if white[ring].sum() > o.max_border_errors:
        return None
    payload = white[b:dd - b, b:dd - b]
    words = [word_of(np.rot90(payload, k)) for k in range(4)]  # the word as read from the corner p_k
    best = min((bin(words[rot] ^ int(code)).count("1"), i, rot) for i, code in enumerate(fam.codes) for rot in range(4))
    return best if best[0] <= fam.max_hamming else None


def image_graph(img, width, cand, fam, o):
    """-> (the kept edges, the number dropped, the quads): what depends on neither the code table nor max_quads."""
    kept, dropped = edges(img, width, cand, fam, o)
    return kept, dropped, quads(kept)


def image_tags(img, width, cand, fam, o, cols, rows, graph=None):
    """One image's candidates [n, 2] -> dict(corners [T, 4, 2], hamming [T], count, n_quads, n_foreign, n_edges_dropped; and of every id
    the rank [T] and the rotation [T] of the quad it was accepted from, -1 not seen; quads: the list of all quads).  graph: image_graph's
    result for the same image, family geometry and edge options."""
    T = cols * rows
    kept, dropped, Q = graph if graph is not None else image_graph(img, width, cand, fam, o)
    best, foreign = {}, 0
    for rank, quad in enumerate(Q[:o.max_quads]):
        r = decode(img, width, cand, quad, kept, fam, o)
        if r is None:
            continue
        ham, i, rot = r
        if i >= T:
            foreign += 1
        elif i not in best or (ham, rank) < best[i][:2]:
            best[i] = (ham, rank, rot, quad)
    corners = np.full((T, 4, 2), np.nan, np.float32); hamming = np.full(T, -1, np.int32)
    ranks = np.full(T, -1, np.int32); rotation = np.full(T, -1, np.int32)
    for i, (ham, rank, rot, quad) in best.items():
        hamming[i], ranks[i], rotation[i] = ham, rank, rot
        for j in range(4):  # the tag's corner 0 is its bottom-left one: the quad's corner rot + 3
            corners[i, j] = cand[quad[(rot + 3 - j) % 4]]
    return dict(corners=corners, hamming=hamming, count=len(best), n_quads=len(Q), n_foreign=foreign, n_edges_dropped=dropped, rank=ranks,
                rotation=rotation, quads=Q)


def tag_grid(images, width, fam, cols, rows, o=Options(), chess=CHESS):
    """images [n, height, pitch] uint8 -> the dict of Solver.tag_grid without the refinement (strength NaN)."""
    images = np.asarray(images)
    det = chess_ref.detect(images, width, chess)
    n, T = len(images), cols * rows
    out = dict(corners=np.full((n, T, 4, 2), np.nan, np.float32), hamming=np.full((n, T), -1, np.int32), count=np.zeros(n, np.int32),
               status=np.zeros(n, np.int32), n_quads=np.zeros(n, np.int32), n_foreign=np.zeros(n, np.int32),
               n_edges_dropped=np.zeros(n, np.int32), strength=np.full((n, T, 4), np.nan))
    for k in range(n):
        if det["status"][k] == chess_ref.OVERFLOW:
            out["status"][k] = OVERFLOW
            continue
        out["status"][k] = OK
        r = image_tags(images[k][:, :width], width, det["xy"][k, :det["count"][k]].astype(np.int64), fam, o, cols, rows)
        for key in ("corners", "hamming", "count", "n_quads", "n_foreign", "n_edges_dropped"):
            out[key][k] = r[key]
    return out


def points(corners, hamming, cols, rows, tag_size, tag_spacing):
    """-> (corners_px [M, 2] float32, board_xy [M, 2] float32, offsets [n + 1] int64): the seen tags image by image in id order."""
    px, bd, off = [], [], [0]
    period = tag_size * (1.0 + tag_spacing)
    for k in range(len(hamming)):
        for i in np.flatnonzero(hamming[k] >= 0):
            x0, y0 = (i % cols) * period, (i // cols) * period
            px.append(corners[k, i])
            bd.append([[x0, y0], [x0 + tag_size, y0], [x0 + tag_size, y0 + tag_size], [x0, y0 + tag_size]])
        off.append(4 * len(bd))
    cat = lambda a: np.array(a, dtype=np.float64).reshape(-1, 2).astype(np.float32)
    return cat(px), cat(bd), np.array(off, dtype=np.int64)
