"""Seeded candidate sets of the K26 tests (the ordering on the device, csrc/clc_boardorder.hpp); no image is committed.  Every case is
a batch of images for one grid: dict(xy [k, stride, 2] float32, count [k], status [k] as it is on entry, cols, rows).

The yardstick of the tests is the product library's clc_chessboard_order (host C++).  The restatement here (tests/chess_ref.py's hull,
quadrilateral and fits, with the host's rounding half away from zero, which np.rint does not do) only shows that the inputs leave every
decision a margin, so that rounding cannot flip one: no pass's ratio within 10 % of tol, and in every pass that the ratio gate lets
through, every node's second-nearest candidate position at least (1 + 1e-6) x as far (squared) as its nearest.  A pass whose ratio is
beyond 1.1 tol is rejected whatever it matched, so its matches decide nothing; the exact lattice has such passes with exact ties (a
quarter turn of a rectangular lattice puts predicted nodes midway between candidates)."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess

import numpy as np

import chess_cases
import chess_ref as ref
import subpix_cases as sp

TOL = 0.3
# of the seeds from 2610 on the first eight whose boards are found with no pass's ratio within 20 % of tol (the restatement decides)
JITTER_SEEDS = (2612, 2613, 2615, 2616, 2617, 2619, 2620, 2622)
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("scenes", "tilted_9x6", "tilted_6x6", "lattice", "lattice_dup", "jitter", "grid_2x2", "grid_2x7", "grid_32x32", "circle_20", "circle_64",
         "octagon", "half", "count_gt", "stride_gt", "refusals")


def _case(xy, cols, rows, count=None, status=None):
    xy = np.ascontiguousarray(xy, dtype=np.float32)
    k = xy.shape[0]
    count = np.full(k, cols * rows, np.int32) if count is None else np.asarray(count, np.int32)
    status = np.ones(k, np.int32) if status is None else np.asarray(status, np.int32)
    return dict(xy=xy, count=count, status=status, cols=cols, rows=rows)


def lattice_points(cols, rows, pitch, H=None, origin=(0.0, 0.0)):
    gx, gy = np.meshgrid(np.arange(cols) * float(pitch), np.arange(rows) * float(pitch))
    p = np.stack([gx.ravel() + origin[0], gy.ravel() + origin[1]], 1)
    if H is not None:
        q = np.concatenate([p, np.ones((len(p), 1))], 1) @ np.asarray(H, float).T
        p = q[:, :2] / q[:, 2:3]
    return p


def shuffled(points, rng):
    return points[rng.permutation(len(points))]


@functools.lru_cache(maxsize=None)
def circle_points():
    """The 108 integer points of x^2 + y^2 = 1105^2 (1105 = 5 x 13 x 17), moved to positive coordinates: in strictly convex position."""
    R = 1105
    pts = []
    for x in range(-R, R + 1):
        y2 = R * R - x * x
        y = int(round(y2 ** 0.5))
        if y * y == y2:
            pts += [(x, y)] if y == 0 else [(x, y), (x, -y)]
    pts = np.array(sorted(set(pts)), float) + 1200.0
    assert len(pts) == 108
    return pts


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    det = ref.detect(chess_cases.scenes(), sp.BOARD_W)
    assert (det["count"] == 20).all()
    out["scenes"] = _case(det["xy"][:, :20], 5, 4)
    out["stride_gt"] = _case(det["xy"], 5, 4)  # stride 256: the slots beyond cols x rows are NaN and are not read
    more = det["xy"][:, :32].copy()
    more[:, 20:] = np.random.default_rng(2601).integers(0, 160, (12, 12, 2))
    out["count_gt"] = _case(more, 5, 4, count=np.full(12, 27))  # 27 candidates: those beyond the strongest 20 are ignored
    for inner in ((9, 6), (6, 6)):
        bs = [b for b in chess_cases.tilted_boards() if b["inner"] == inner]
        d = ref.detect(np.stack([b["image"] for b in bs]), chess_cases.TILTED_W)
        assert (d["count"] == inner[0] * inner[1]).all()
        out["tilted_%dx%d" % inner] = _case(d["xy"][:, :inner[0] * inner[1]], *inner)
    rng = np.random.default_rng(2602)
    lat = shuffled(lattice_points(9, 6, 10, origin=(30.0, 20.0)), rng)
    out["lattice"] = _case(lat[None], 9, 6)
    dup = lat.copy()
    dup[17] = dup[40]
    out["lattice_dup"] = _case(dup[None], 9, 6)
    jit = []
    for seed in JITTER_SEEDS:
        r = np.random.default_rng(seed)
        jit.append(shuffled(lattice_points(9, 6, 12, origin=(25.0, 40.0)) + r.integers(-1, 2, (54, 2)), r))
    out["jitter"] = _case(np.stack(jit), 9, 6)
    out["grid_2x2"] = _case(np.array([[[60, 14], [8, 47], [10, 10], [57, 50]]], float), 2, 2)
    c, s = np.cos(0.4), np.sin(0.4)
    out["grid_2x7"] = _case(np.rint(shuffled(lattice_points(2, 7, 12, [[c, -s, 80], [s, c, 30], [0, 0, 1]]), rng))[None], 2, 7)
    big = lattice_points(32, 32, 12, [[1.0, 0.05, 40.0], [-0.03, 1.0, 60.0], [2e-5, 1e-5, 1.0]])
    out["grid_32x32"] = _case(np.rint(shuffled(big, rng))[None], 32, 32)
    circ = circle_points()
    out["circle_20"] = _case(circ[np.random.default_rng(2603).choice(108, 20, replace=False)][None], 5, 4)
    out["circle_64"] = _case(circ[np.random.default_rng(2604).choice(108, 64, replace=False)][None], 8, 8)
    octagon = np.array([[30, 10], [10, 30], [-10, 30], [-30, 10], [-30, -10], [-10, -30], [10, -30], [30, -10]], float)
    inner = np.array([[5, 5], [-5, 5], [-5, -5], [5, -5], [12, 0], [0, 12], [-12, 0], [0, -12]], float)
    out["octagon"] = _case((shuffled(np.concatenate([octagon, inner]), rng) + 100.0)[None], 4, 4)
    # coordinates ending in .5 on both sides of zero: half away from zero moves them apart, half to even would not
    half = []
    for seed in range(2):
        r = np.random.default_rng(2620 + seed)
        p = lattice_points(9, 6, 12, origin=(-48.0, -30.0)) + np.where(r.random((54, 2)) < 0.5, 0.5, 0.0) * (1 if seed == 0 else -1)
        half.append(shuffled(p, r))
    out["half"] = _case(np.stack(half), 9, 6)
    # every refusal of order_image / order_images
    xy = det["xy"][:7, :20].copy()
    count = np.full(7, 20, np.int32); status = np.ones(7, np.int32)
    count[0] = 19                                             # one candidate short
    status[1] = ref.OVERFLOW                                  # passes through
    good = ref.order(xy[2:3], count[2:3], 5, 4)["index"][0]
    corner, inward = good[3, 4], good[3, 3]
    xy[2, corner] += xy[2, corner] - xy[2, inward]            # a corner moved by one spacing: the tol gate
    xy[3] = np.stack([10 + 3 * np.arange(20), 20 + 2 * np.arange(20)], 1)  # collinear
    xy[4] = 50.0                                              # 20 coincident
    xy[5, 7, 1] = np.nan                                      # a NaN
    xy[6, 11, 0] = 2.0 ** 25                                  # beyond 2^24
    out["refusals"] = _case(xy, 5, 4, count, status)
    assert sorted(out) == sorted(NAMES)
    return out


REFUSALS_STATUS = [ref.TOO_FEW, ref.OVERFLOW, ref.NO_GRID, ref.NO_GRID, ref.NO_GRID, ref.NO_GRID, ref.NO_GRID]


def batch(count):
    """`count` images: the 12 scenes' candidates in turn (stride 256)."""
    c = cases()["stride_gt"]
    k = np.arange(count) % 12
    return dict(xy=c["xy"][k], count=c["count"][k], status=c["status"][k], cols=5, rows=4)


# ---------------------------------------------------------------------------------------------------------------------------------
# The restatement with what it saw
# ---------------------------------------------------------------------------------------------------------------------------------
def round_away(v):
    v = np.asarray(v, float)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def restate_image(xy, cols, rows, tol=TOL):
    """One image (its count and status already passed) -> dict(status, index, n_labelings, worst, hull, quad, ties, passes), passes a
    list of (ratio, margin, bijection): margin the smallest second-nearest / nearest ratio of squared distances over the nodes, taken
    over the distinct candidate positions (coincident candidates tie exactly: the first wins by rule)."""
    n = cols * rows
    out = dict(status=ref.NO_GRID, index=None, n_labelings=0, worst=np.nan, hull=[], quad=None, ties=0, passes=[])
    v = np.asarray(xy[:n], np.float32)
    if not (np.abs(v) <= 16777216.0).all():
        return out
    P = round_away(v)
    hv = ref.hull(P)
    out["hull"] = list(hv)
    if len(hv) < 4:
        return out
    hv = np.array(hv)
    import itertools
    combos = np.array(list(itertools.combinations(range(len(hv)), 4)), dtype=np.int64)
    X, Y = P[hv, 0][combos], P[hv, 1][combos]
    area = sum(X[:, k] * Y[:, (k + 1) % 4] - X[:, (k + 1) % 4] * Y[:, k] for k in range(4))
    out["quad"] = combos[int(np.argmax(area))]
    out["ties"] = int((area == area.max()).sum())
    quad = hv[out["quad"]]
    gx, gy = np.meshgrid(2.0 * np.arange(cols) / (cols - 1) - 1.0, 2.0 * np.arange(rows) / (rows - 1) - 1.0)
    nodes = np.stack([gx.ravel(), gy.ravel()], 1)
    corners = nodes[[0, cols - 1, n - 1, n - cols]]
    mean = P.astype(float).mean(axis=0)
    cand = (P - mean) / max(1.0, np.abs(P - mean).max())
    distinct = np.unique(cand, axis=0)

    def one_pass(H):
        pred = ref.apply_h(H, nodes)
        g = pred.reshape(rows, cols, 2)
        spacing = min(np.linalg.norm(g[:, 1:] - g[:, :-1], axis=2).min(), np.linalg.norm(g[1:] - g[:-1], axis=2).min())
        d = ((pred[:, None] - cand[None]) ** 2).sum(axis=2)
        m = d.argmin(axis=1)
        far = np.sqrt(d[np.arange(n), m].max())
        dd = np.sort(((pred[:, None] - distinct[None]) ** 2).sum(axis=2), axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            margin = np.where(dd[:, 0] > 0, dd[:, 1] / dd[:, 0], np.inf).min() if len(distinct) > 1 else np.inf
        bij = len(set(m.tolist())) == n
        out["passes"].append((float(far / spacing), float(margin), bij))
        return bij and far <= tol * spacing, m, far / spacing

    valid = []
    for k in range(4):
        try:
            ok, m, worst = one_pass(ref.homography(corners, cand[np.roll(quad, -k)]))
            if not ok:
                continue
            ok, m, worst = one_pass(ref.homography(nodes, cand[m]))
        except np.linalg.LinAlgError:
            continue
        if ok:
            valid.append((int(P[m[0], 1]), int(P[m[0], 0]), k, m, worst))
    if valid:
        best = min(valid, key=lambda t: t[:3])
        out.update(status=ref.FOUND, index=best[3].astype(np.int32), n_labelings=len(valid), worst=float(best[4]))
    return out


@functools.lru_cache(maxsize=None)
def restated(name):
    """Per image of the case: restate_image's dict, or dict(status) where the count or the status on entry decides."""
    c = cases()[name]
    out = []
    for k in range(len(c["xy"])):
        if c["status"][k] == ref.OVERFLOW:
            out.append(dict(status=ref.OVERFLOW, passes=[], hull=[], quad=None, ties=0, n_labelings=0))
        elif c["count"][k] < c["cols"] * c["rows"]:
            out.append(dict(status=ref.TOO_FEW, passes=[], hull=[], quad=None, ties=0, n_labelings=0))
        else:
            out.append(restate_image(c["xy"][k], c["cols"], c["rows"]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# The yardstick and the host shim
# ---------------------------------------------------------------------------------------------------------------------------------
def V(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def empty_out(k, n, optional=True):
    return dict(index=np.full((k, n), -7, np.int32), n_labelings=np.full(k, -7, np.int32) if optional else None,
                worst=np.full(k, -7.0) if optional else None)


def host_order(c, library=None):
    """clc_chessboard_order of the product library (host code: no device) -> dict(index [k, n], status, n_labelings, worst)."""
    from camlasercalibratool_amd import _capi
    L = _capi.lib() if library is None else library
    k, n = len(c["xy"]), c["cols"] * c["rows"]
    r = empty_out(k, n)
    r["status"] = c["status"].copy()
    code = L.clc_chessboard_order(V(c["xy"]), V(c["count"]), C.c_int64(c["xy"].shape[1]), C.c_size_t(k), c["cols"], c["rows"], None, V(r["index"]),
                                  V(r["status"]), V(r["n_labelings"]), V(r["worst"]))
    assert code == 0, L.clc_last_error()
    return r


def build_shim(path):
    src = os.path.join(HERE, "shim", "boardorder_shim.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", path])
    L = C.CDLL(path)
    L.shim_board_lds_bytes.restype = C.c_longlong
    return L


def shim_order(L, c):
    """shim_board_order -> host_order's dict + nh [k], hull [k, n], quad [k, 4]."""
    k, n = len(c["xy"]), c["cols"] * c["rows"]
    r = empty_out(k, n)
    r.update(status=c["status"].copy(), nh=np.zeros(k, np.int32), hull=np.full((k, n), -7, np.int32), quad=np.full((k, 4), -7, np.int32))
    L.shim_board_order(V(c["xy"]), V(c["count"]), C.c_longlong(c["xy"].shape[1]), C.c_longlong(k), C.c_int32(c["cols"]), C.c_int32(c["rows"]),
                       C.c_double(TOL), V(r["index"]), V(r["status"]), V(r["n_labelings"]), V(r["worst"]), V(r["nh"]), V(r["hull"]), V(r["quad"]))
    return r


def write_cases(path):
    """Every case for tests/shim/boardorder_main.cpp: int32 n_cases; per case int32 cols, rows, stride, k, count[k], status[k], xy."""
    with open(path, "wb") as f:
        f.write(np.array([len(NAMES)], np.int32).tobytes())
        for name in NAMES:
            c = cases()[name]
            f.write(np.array([c["cols"], c["rows"], c["xy"].shape[1], len(c["xy"])], np.int32).tobytes())
            f.write(c["count"].tobytes() + c["status"].tobytes() + c["xy"].tobytes())


EPS = 2.0 ** -52


def assert_same_order(got, want, what, worst_exact=False):
    """index, status and n_labelings equal; worst NaN where the yardstick's is, else within 16 eps relative (the spacing is
    sqrt(dx dx + dy dy) against hypot: about 2 ulp, so about 4 eps on the ratio; the gate leaves that 4 x the room)."""
    for key in ("index", "status", "n_labelings"):
        assert np.array_equal(got[key].reshape(-1), want[key].reshape(-1)), (what, key, got[key].reshape(-1)[:24], want[key].reshape(-1)[:24])
    a, b = got["worst"], want["worst"]
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, "worst", a, b)
    ok = ~np.isnan(b)
    if worst_exact:
        assert np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64)), (what, "worst bits", a, b)
    elif ok.any():
        rel = np.abs(a[ok] - b[ok]) / np.abs(b[ok])
        print(what, "worst: largest relative difference", rel.max() / EPS, "eps")
        assert (rel <= 16 * EPS).all(), (what, "worst", rel.max() / EPS)
