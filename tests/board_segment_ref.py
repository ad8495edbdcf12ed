"""Pure-Python restatement of AutoGetLinePts (src/selectScanPoints.cpp:17-190, the detection part) for the tests of
clc_board_segments: the reference's loop, statement for statement, on one scan.  A test helper only — the package has
no CPU path.  Returns (first, last, status) with status 1 found, 0 none, -1 where the reference's points.at() raises."""
import math

import numpy as np

FOUND, NONE, THROWS = 1, 0, -1


def _norm2(p):
    x, y = float(p[0]), float(p[1])
    xx = x * x  # each square rounded, then the sum (Eigen's squaredNorm; no FMA in Python)
    yy = y * y
    return math.sqrt(xx + yy)


def auto_get_line_pts(points):
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = P.shape[0]

    def at(i):
        if i < 0 or i >= n:
            raise IndexError(i)
        return P[i]

    try:
        idm = n // 2
        delta = int(80 / 0.3)
        id_left = min(idm + delta, n - 1)
        id_right = max(idm - delta, 0)
        at(id_left)
        at(id_right)
        segs = []
        skip = 3
        cur, nxt = id_right, id_right + skip
        new_seg = True
        s_start = s_end = 0
        i = id_right
        while i < id_left - skip:
            if new_seg:
                s_start, s_end = cur, nxt
                new_seg = False
            d1, d2 = _norm2(at(cur)), _norm2(at(nxt))
            if d1 < 100 and d2 < 100:
                if abs(d1 - d2) < 0.05:
                    s_end = nxt
                else:
                    new_seg = True
                    with np.errstate(invalid="ignore"):
                        dist = at(s_start) - at(s_end)
                    if (_norm2(dist) > 0.2 and _norm2(at(s_start)) < 2 and _norm2(at(s_end)) < 2
                            and s_end - s_start > 50):
                        segs.append([s_start, s_end])
                cur = nxt
                nxt += skip
            else:
                if d1 > 100:
                    cur = nxt
                nxt += skip
            i += skip
        for k in range(len(segs)):
            a0, b0 = segs[k]
            for j in (1, 2, 3):
                if abs(_norm2(at(b0)) - _norm2(at(b0 + j))) < 0.05:
                    segs[k][1] = b0 + j
            for j in (-1, -2, -3):
                if abs(_norm2(at(a0)) - _norm2(at(a0 + j))) < 0.05:
                    segs[k][0] = a0 + j
    except IndexError:
        return -1, -1, THROWS
    best, maxpts = None, -1
    for a, b in segs:
        if b - a > maxpts:
            best, maxpts = (a, b), b - a
    if best is None:
        return -1, -1, NONE
    return best[0], best[1], FOUND


def board_segments(points, offsets):
    """auto_get_line_pts for every scan of a CSR batch -> (seg [S,2] int64, status [S] int32)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    S = len(offsets) - 1
    seg = np.full((S, 2), -1, dtype=np.int64)
    st = np.zeros(S, dtype=np.int32)
    for k in range(S):
        a, b, s = auto_get_line_pts(points[offsets[k]:offsets[k + 1]])
        seg[k] = (a, b)
        st[k] = s
    return seg, st
