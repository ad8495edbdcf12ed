"""Host side of the scan front-end fuzz (tests/test_gpu_scan_frontend.py imports its generators and references from here): what the
oracle alone must satisfy on the fuzz inputs, so that the GPU gates need no exemptions.

  * fuzz_scans: seeded scans of five kinds (geometry and noise of _scans in test_gpu_parity.py).
  * Reorder invariance of oracle.line_fit: every scan as given and in the 16-way strided order line_fit_kernel sums in.  Required: the
    same termination and iteration count, lines within 1e-12 relative, costs within 1e-13.  Measured (2 000 scans per kind and loss
    setting, seed 5): 0 flips in 22 000 scans; worst line difference 8.9e-15, worst cost difference 3.2e-14 (both: long, without the
    loss); sentinel 3.3e-16 / 1.5e-16 with the loss, 1.9e-15 / 2.2e-15 without; start 2.2e-16 / 1.7e-16 and 8.2e-16 / 3.6e-15;
    sentinel_skew (with the loss only) 4.6e-15 / 1.2e-15.  The sentinel generator had to change for this: see fuzz_scans.
  * oracle.scan_to_points against an extended-precision restatement (theta in fp64 exactly as the source forms it, cos / sin in
    np.longdouble, times the float32 range): measured maximum |oracle - restatement| / r = 1.598e-16 = 1.44 x 2^-53 over 63 311
    in-range rays, theta up to 74 rad.
  * exact_closed_form: the 45 sums of K5 (accumulate_normal9: bb x nn, then A^T b) with products in np.longdouble split into two
    doubles and summed by math.fsum, expanded to the 9 x 9 system as clc_closed_form does, solved in rational arithmetic.
    oracle.closed_form's distance from it over the case list of the GPU module (closed_form_cases): sv9 3.34e-14 of sv9[0], Tlc
    4.27e-12 of max|Tlc| at worst (both at 250 000 observations: the oracle's sequential sums); `unobservable` equal everywhere.
  * oracle fix that this module's GPU twin needed: a non-finite cost at iteration 0 now ends lm_minimize with FAILURE and the
    parameters untouched, as Ceres does (it reported CONVERGENCE at iteration 0 before: max(0, NaN) made the gradient norm 0)."""
import math
import os
import time
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np
import pytest

from camlasercalibratool_amd import simdata as sd

KINDS = ("mid", "short", "long", "sentinel", "start")
ALL_KINDS = KINDS + ("sentinel_skew",)  # with the loss only: see fuzz_scans
SHORT_LENGTHS = (0, 1, 2, 3, 15, 16, 17)
LINE_REL, COST_ABS = 1e-12, 1e-13  # reorder gates of the oracle alone


def n_threads(oracle_mod) -> int:
    """Oracle thread pool: the environment's thread count (OMP_NUM_THREADS where set), never the machine's CPU count; 16 at most."""
    env = os.environ.get("OMP_NUM_THREADS", "")
    return max(1, min(16, int(env) if env.isdigit() else min(16, oracle_mod.max_threads())))


def fuzz_scans(seed, n_scans, kind):
    """-> (xy [M, 2], offsets [n_scans + 1], lines0 [n_scans, 2], truth [n_scans, 2]).  Kinds: mid 40-400 points; short 0-40 points
    (0, 1, 2, 3, 15, 16, 17 among the first seven, rotated by the seed so that small batches see all of them over the seeds); long
    400-3000; start: mid with a start line around the truth, +-30 %.

    sentinel: mid scans that lie on a line through (1000, 1000), with 1-3 points replaced by (1000, 1000), started +-30 % around the
    truth.  A fit without the loss has to pass the sentinel; on these scans its optimum cost is then O(1), where the absolute 1e-13
    cost gate means something, and the first evaluations weigh the sentinel at loss arguments 1 + (r / a)^2 of 1e6-1e8.
    sentinel_skew: the same with the scan's own direction, so that the sentinel is a true outlier the loss has to reject (arguments
    to 2e9).  The oracle alone meets the reorder gates on it with the loss (line 4.6e-15, cost 1.2e-15); without the loss its final
    costs are ~190 (ulp 2.8e-14) and the oracle alone moves by 2.1e-13 under reordering, more than the host cost gate, so the host
    module runs it with the loss only.  With sentinels on scans of any direction AND a start line of (0, 0) the oracle alone misses
    the gates with the loss as well (2 000 scans, seed 5: line 2.2e-12, cost 9.3e-13, nearly every scan out of iterations): that
    combination is not generated."""
    assert kind in ALL_KINDS
    rng = np.random.default_rng([seed, ALL_KINDS.index(kind)])
    xs, truth, off = [], [], [0]
    for k in range(n_scans):
        if kind == "short":
            n = SHORT_LENGTHS[(k + seed) % 7] if k < 7 else int(rng.integers(0, 41))
        elif kind == "long":
            n = int(rng.integers(400, 3001))
        else:
            n = int(rng.integers(40, 401))
        th = rng.uniform(-1.3, 1.3); c = rng.uniform(0.8, 5.0)
        if kind == "sentinel":
            th = -np.pi / 4 + np.arcsin(c / (1000.0 * np.sqrt(2.0)))  # the scan's line passes through (1000, 1000)
        t = np.sort(rng.uniform(-0.5, 0.5, n))
        xy = np.stack([c * np.cos(th) - t * np.sin(th), c * np.sin(th) + t * np.cos(th)], 1) + rng.normal(size=(n, 2)) * 0.004
        bad = rng.random(n) < 0.08
        xy[bad] += rng.normal(size=(int(bad.sum()), 2)) * 0.3
        if kind.startswith("sentinel"):
            xy[rng.choice(n, size=int(rng.integers(1, 4)), replace=False)] = 1000.0
        xs.append(xy); truth.append([-np.cos(th) / c, -np.sin(th) / c]); off.append(off[-1] + n)
    truth = np.array(truth).reshape(n_scans, 2)
    lines0 = truth * (1.0 + rng.uniform(-0.3, 0.3, size=truth.shape)) if kind in ("start", "sentinel", "sentinel_skew") else np.zeros((n_scans, 2))
    return np.concatenate(xs).reshape(-1, 2), np.array(off, dtype=np.int64), lines0, truth


def line_options(mod, use_loss=1, max_it=None):
    o = mod.default_line_options()
    o.use_loss = int(use_loss)
    if max_it is not None:
        o.max_num_iterations = max_it
    return o


def oracle_line_fits(oracle_mod, xy, off, lines0, use_loss=1, loss_a=0.05, max_it=None, order=None):
    """oracle.line_fit of every scan (thread pool) -> list of SolveResult.  order: a function applied to each scan's points."""
    o = line_options(oracle_mod, use_loss, max_it)
    o.loss_scale_factor = loss_a

    def one(k):
        p = xy[off[k]:off[k + 1]]
        return oracle_mod.line_fit(p if order is None else order(p), lines0[k], options=o, loss_a=loss_a, linear_solver="qr", trace_cap=1)

    with ThreadPoolExecutor(n_threads(oracle_mod)) as ex:
        return list(ex.map(one, range(len(off) - 1)))


def strided16(p):
    """The order line_fit_kernel sums a scan in: lane s of the 16-lane row takes points s, s + 16, ..."""
    return np.concatenate([p[s::16] for s in range(16)]) if p.shape[0] else p


def reorder_report(oracle_mod, seed, n_scans, kind, use_loss):
    xy, off, l0, _ = fuzz_scans(seed, n_scans, kind)
    a = oracle_line_fits(oracle_mod, xy, off, l0, use_loss)
    b = oracle_line_fits(oracle_mod, xy, off, l0, use_loss, order=strided16)
    flips, dl, dc = 0, 0.0, 0.0
    for ra, rb in zip(a, b):
        flips += (ra.summary.termination != rb.summary.termination) or (ra.summary.num_iterations != rb.summary.num_iterations)
        dl = max(dl, np.abs(ra.pose - rb.pose).max() / max(1.0, np.abs(ra.pose).max()))
        dc = max(dc, abs(ra.summary.final_cost - rb.summary.final_cost))
    return flips, dl, dc


@pytest.mark.parametrize("kind,use_loss", [(k, u) for k in KINDS for u in (1, 0)] + [("sentinel_skew", 1)])
def test_oracle_line_fit_does_not_depend_on_the_summation_order(oracle_mod, kind, use_loss):
    n = int(os.environ.get("CLC_FRONTEND_FUZZ_SCANS", "2000"))
    if kind == "short":
        assert set(SHORT_LENGTHS) <= set(np.diff(fuzz_scans(5, n, kind)[1]).tolist())
    flips, dl, dc = reorder_report(oracle_mod, 5, n, kind, use_loss)
    print(f"reorder {kind} loss={use_loss}: {n} scans, flips {flips}, line {dl:.2e}, cost {dc:.2e}")
    assert flips == 0
    assert dl <= LINE_REL and dc <= COST_ABS, (dl, dc)


def test_fuzz_scans_kinds():
    for kind, lo, hi in (("mid", 40, 400), ("short", 0, 40), ("long", 400, 3000), ("sentinel", 40, 400), ("start", 40, 400), ("sentinel_skew", 40, 400)):
        xy, off, l0, truth = fuzz_scans(3, 64, kind)
        n = np.diff(off)
        assert n.min() >= lo and n.max() <= hi and xy.shape == (off[-1], 2) and l0.shape == truth.shape == (64, 2)
        xy2 = fuzz_scans(3, 64, kind)[0]
        assert np.array_equal(xy, xy2)  # seeded
        sent = (xy == 1000.0).all(1)
        if kind.startswith("sentinel"):
            per = np.add.reduceat(sent.astype(int), off[:-1])
            assert per.min() >= 1 and per.max() <= 3
        else:
            assert not sent.any()
        if kind in ("start", "sentinel", "sentinel_skew"):
            rel = np.abs(l0 / truth - 1.0)
            assert rel.max() <= 0.3 and rel.max() > 0.1
        else:
            assert not l0.any()


# ---- scan conversion ---------------------------------------------------------------------------------------------------------------
def scan_points_extended(ranges, angle_min, angle_increment, range_min):
    """TranScanToPoints of one scan with cos / sin in np.longdouble -> (points [n, 3] longdouble, sentinel mask [n])."""
    r = np.ascontiguousarray(ranges, dtype=np.float32)
    th = np.float64(np.float32(angle_min)) + np.arange(r.shape[0], dtype=np.float64) * np.float64(np.float32(angle_increment))  # fp64, as the source
    thl = th.astype(np.longdouble)
    rl = r.astype(np.longdouble)
    with np.errstate(invalid="ignore"):
        ok = (r.astype(np.float64) < 30.0) & (r >= np.float32(range_min))
        P = np.zeros((r.shape[0], 3), dtype=np.longdouble)
        P[:, 0] = np.where(ok, rl * np.cos(thl), np.longdouble(1000.0))
        P[:, 1] = np.where(ok, rl * np.sin(thl), np.longdouble(1000.0))
    return P, ~ok


def scan_cases():
    """One call's worth of scans for scan conversion -> dict(ranges, offsets, angle_min, angle_increment, range_min).  Ragged lengths
    with empty scans first, last and adjacent; a scan beyond 64 x 256 rays (the grid-stride loop of the 2-D kernel); the range edge
    values planted in every non-empty scan; angle_min / angle_increment that take theta beyond 2 pi at the far rays."""
    rng = np.random.default_rng(77)
    lens = [0, 1, 255, 0, 0, 256, 257, 1081, 16384, 0, 16385, 40000, 0]
    S = len(lens)
    amin = rng.uniform(-2.4, -2.3, S).astype(np.float32)
    ainc = np.full(S, np.float32(np.deg2rad(0.25)))
    ainc[8], amin[10], ainc[11] = np.float32(0.001), np.float32(3.0), np.float32(0.0005)  # theta to 16.4 - 2.3, 3 + 71, 20 - 2.3 rad
    rmin = rng.choice(np.array([0.05, 0.1, 0.45], dtype=np.float32), S)
    rs = []
    for k, n in enumerate(lens):
        r = rng.uniform(0.02, 35.0, n).astype(np.float32)
        edge = np.array([rmin[k], np.nextafter(rmin[k], np.float32(0)), np.nextafter(np.float32(30), np.float32(0)), 30.0, np.nan, np.inf, -np.inf,
                         -1.0, 0.0], dtype=np.float32)
        if n >= 2 * edge.size:
            r[rng.choice(n, edge.size, replace=False)] = edge
            r[-1] = rmin[k]  # the far ray: in range
        elif n == 1:
            r[0] = rmin[k]
        rs.append(r)
    off = np.zeros(S + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    return dict(ranges=np.concatenate(rs), offsets=off, angle_min=amin, angle_increment=ainc, range_min=rmin)


def scan_error(points, c):
    """max over in-range rays of |points - extended restatement| / r, and the sentinel mask of the restatement, scan by scan."""
    worst = 0.0
    mask = np.zeros(points.shape[0], dtype=bool)
    off = c["offsets"]
    for k in range(len(off) - 1):
        r = c["ranges"][off[k]:off[k + 1]]
        P, sent = scan_points_extended(r, c["angle_min"][k], c["angle_increment"][k], c["range_min"][k])
        mask[off[k]:off[k + 1]] = sent
        ok = ~sent
        if ok.any():
            d = np.abs(points[off[k]:off[k + 1]][ok, :2].astype(np.longdouble) - P[ok, :2]).max(1) / r[ok].astype(np.longdouble)
            worst = max(worst, float(d.max()))
    return worst, mask


def test_oracle_scan_to_points_against_extended_precision(oracle_mod):
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not an extended type here"
    c = scan_cases()
    off = c["offsets"]
    pts = np.concatenate([oracle_mod.scan_to_points(c["ranges"][off[k]:off[k + 1]], c["angle_min"][k], c["angle_increment"][k], c["range_min"][k])
                          for k in range(len(off) - 1)])
    worst, mask = scan_error(pts, c)
    print(f"oracle scan_to_points vs extended precision: {worst:.3e} of r ({worst * 2 ** 53:.2f} x 2^-53), {int(mask.sum())} sentinels of {mask.size}")
    assert np.array_equal((pts[:, :2] == 1000.0).all(1), mask) and not pts[:, 2].any()
    assert worst <= 3 * 2.0 ** -53  # the C library's cos / sin within 1 ulp (2^-52 of a value <= 1) and the product's rounding (2^-53)
    # the edge values sit where the source's comparison puts them (range < 30.0 && range >= range_min, float range against double 30)
    k = 7
    r = c["ranges"][off[k]:off[k + 1]]
    sent = mask[off[k]:off[k + 1]]
    rm = c["range_min"][k]
    assert not sent[r == rm].any() and sent[r == np.nextafter(rm, np.float32(0))].all()
    assert not sent[r == np.nextafter(np.float32(30), np.float32(0))].any() and sent[r == np.float32(30)].all()
    assert sent[np.isnan(r)].all() and sent[np.isinf(r)].all() and sent[r <= 0].all()


# ---- closed form (K5) --------------------------------------------------------------------------------------------------------------
def _fsum_ld(t):
    """Sum of longdouble terms: each split into two doubles, math.fsum over all parts (exact for the parts)."""
    hi = t.astype(np.float64)
    lo = (t - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(np.concatenate([hi, lo]).tolist())


def exact_normal9(rec):
    """The 45 sums of K5 (layout of accumulate_normal9: [bb(6: xx xy x yy y 1)] x [nn(6: 00 01 02 11 12 22)], then the 9 of A^T b =
    sum [x, y, 1] x n * (-d)) -> (AtA [9, 9], Atb [9]) expanded as clc_closed_form does."""
    L = np.longdouble
    nx, ny, nz, d, x, y = (rec[:, i].astype(L) for i in range(6))
    one = np.ones_like(x)
    nn = [nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz]
    bb = [x * x, x * y, x, y * y, y, one]
    r = np.empty(45)
    for i in range(6):
        for j in range(6):
            r[6 * i + j] = _fsum_ld(bb[i] * nn[j])
    for i, b in enumerate((x, y, one)):
        for j, n in enumerate((nx, ny, nz)):
            r[36 + 3 * i + j] = _fsum_ld(b * n * (-d))

    def tri3(a, b):
        a, b = min(a, b), max(a, b)
        return a * 3 - (a * (a - 1)) // 2 + (b - a)

    AtA, Atb = np.empty((9, 9)), np.empty(9)
    for ci in range(3):
        for ri in range(3):
            for cj in range(3):
                for rj in range(3):
                    AtA[3 * ci + ri, 3 * cj + rj] = r[6 * tri3(ci, cj) + tri3(ri, rj)]
            Atb[3 * ci + ri] = r[36 + 3 * ci + ri]
    return AtA, Atb


def _solve_rational(A, b):
    n = len(b)
    M = [[Fraction(float(A[i, j])) for j in range(n)] + [Fraction(float(b[i]))] for i in range(n)]
    for k in range(n):
        p = max(range(k, n), key=lambda i: abs(M[i][k]))
        if M[p][k] == 0:
            return None
        M[k], M[p] = M[p], M[k]
        for i in range(k + 1, n):
            f = M[i][k] / M[k][k]
            if f:
                M[i] = [a - f * c for a, c in zip(M[i], M[k])]
    x = [Fraction(0)] * n
    for i in range(n - 1, -1, -1):
        x[i] = (M[i][n] - sum(M[i][j] * x[j] for j in range(i + 1, n))) / M[i][i]
    return np.array([float(v) for v in x])


def exact_closed_form(rec):
    """-> (sv9 descending, unobservable, Tlc or None when the system is singular, (AtA, Atb)): the closed form on the exact sums."""
    AtA, Atb = exact_normal9(rec)
    sv9 = np.linalg.eigvalsh(AtA)[::-1].copy()
    unobs = bool((sv9 < 1e-10).any())
    T = None
    h = None if unobs else _solve_rational(AtA, Atb)
    if h is not None:
        h1, h2, h3 = h[:3], h[3:6], h[6:]
        Rlc = np.stack([h1, h2, np.cross(h1, h2)])  # Rcl columns = h1, h2, h1 x h2; Rlc = Rcl^T
        U, _, Vt = np.linalg.svd(Rlc)
        T = np.eye(4)
        T[:3, :3] = U @ Vt
        T[:3, 3] = -Rlc @ h3  # before the orthogonalisation, as the source
    return sv9, unobs, T, (AtA, Atb)


def _records(seed, lens, with_z):
    K = max(int(max(lens)), 1)
    import oracle  # (the records come from the oracle's own assembly loop: this module needs nothing but the oracle)
    rec = oracle.flatten(sd.sim_fixed_count(seed, len(lens), K, noise_sigma=0.01), False, False).reshape(len(lens), K, 8)
    out = np.ascontiguousarray(np.concatenate([rec[s, :l] for s, l in enumerate(lens)]))
    if with_z:
        out[::3, 6] = np.random.default_rng(seed).normal(size=out[::3].shape[0]) * 0.02
    return out


def closed_form_cases(big=True):
    """(label, records [n, 8], rank_deficient) of the K5 case list: n on the tile (128), row (64) and 4 x 16 partial-row edges."""
    out = []
    for i, n in enumerate((1, 2, 127, 128, 129, 255, 256, 257, 128 * 97 + 5)):
        per = 25 if n < 1000 else 97
        lens = [per] * (n // per) + ([n % per] if n % per else [])
        out.append((f"n={n}", _records(20 + i, lens, with_z=(i % 3 == 2)), n < 9))
    for i, K in enumerate((63, 64, 65)):
        out.append((f"12 scans of {K}", _records(40 + i, [K] * 12, with_z=(i == 1)), False))
    out.append(("scans of 63/64/65/1/16/17", _records(44, [63, 64, 65, 1, 16, 17, 48, 49, 64, 128, 129, 5], with_z=True), False))
    out.append(("one scan of 200", _records(45, [200], with_z=False), True))
    if big:
        out.append(("n=250000", _records(46, [500] * 500, with_z=False), False))
    return out


def closed_form_distance(ex, T, unobs, sv9, rank_deficient):
    """(sv9 distance relative to sv9[0], Tlc distance relative to max|Tlc| or None) of a result from the exact reference `ex`."""
    e_sv, e_un, e_T, _ = ex
    dsv = float(np.abs(np.asarray(sv9) - e_sv).max() / e_sv[0])
    dT = None
    if not rank_deficient:
        assert not e_un and e_T is not None and not unobs
        dT = float(np.abs(np.asarray(T).reshape(4, 4) - e_T).max() / np.abs(e_T).max())
    return dsv, dT


def oracle_closed_form_yardstick(oracle_mod, cases, exact=None):
    """The oracle's worst distances from the exact reference over `cases` -> (worst sv9, worst Tlc, [exact results])."""
    exact = exact or [exact_closed_form(rec) for _, rec, _ in cases]
    wsv, wT = 0.0, 0.0
    for (label, rec, rd), ex in zip(cases, exact):
        T, un, s9 = oracle_mod.closed_form(rec)
        assert un == ex[1], label
        assert rd == ex[1], label  # the list's rank-deficient cases are the unobservable ones
        dsv, dT = closed_form_distance(ex, T, un, s9, rd)
        wsv, wT = max(wsv, dsv), max(wT, dT or 0.0)
    return wsv, wT, exact


def test_exact_closed_form_reference_against_the_oracle(oracle_mod):
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not an extended type here"
    t0 = time.perf_counter()
    cases = closed_form_cases()
    wsv, wT, exact = oracle_closed_form_yardstick(oracle_mod, cases)
    print(f"oracle closed form vs exact sums: sv9 {wsv:.2e} of sv9[0], Tlc {wT:.2e} of max|Tlc| ({time.perf_counter() - t0:.1f} s)")
    # the reference restates the oracle's algebra independently: at these sizes the oracle's sequential fp64 sums sit within 1e-13
    # (sv9) and, through a 9 x 9 system of condition ~1e5 at worst, 1e-9 (Tlc) of it — the bound of the existing parity tests
    assert wsv <= 1e-13 and wT <= 1e-9
    # the sums themselves: the oracle's A^T A is kron(bb, nn) of the same records
    rec = cases[3][1]
    AtA, Atb = exact[3][3]
    A = np.stack([np.kron(np.array([r[4], r[5], 1.0]), r[:3]) for r in rec])
    assert np.abs(A.T @ A - AtA).max() <= 1e-13 * np.abs(AtA).max() and np.abs(A.T @ (-rec[:, 3]) - Atb).max() <= 1e-13 * np.abs(Atb).max()
    assert np.array_equal(AtA, AtA.T)
