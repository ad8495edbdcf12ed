"""Seeded, constructed cases for the shape fuzz of clc_solve_subsets and clc_score_blocks (tests/test_gpu_subsets_fuzz.py; checked
without a GPU by tests/test_subsets_fuzz_cases.py).  A test helper: numpy only, no GPU, no oracle.

One problem per (form, points per lane) on the capacity edges of the resident kernel — EDGES of tests/test_gpu_batched_fuzz.py, whose
Pool and edge_lens build the problems — with at least 16 scans, at least one lane with padding (ppl > 1) and at least one scan dealt to
two or more lanes (ppl > 1; the 'short' style, which has none of its own, gets one split scan of q ppl - r points in exchange for q of its
short scans).  The styles short / split / dense rotate over the cases.

Block cuts of a problem (offsets with repeated values = empty blocks):
  scan      one block per scan
  multi     blocks of 1-5 whole scans, empty blocks at the front, at the back and in runs in the middle
  multi300, multi2nl   `multi` with more empty blocks: 300 blocks, and 2 NL + 1 blocks (block_scores_kernel stages NL blocks at a time)
  lanecut   `multi` plus boundaries INSIDE scans, exactly on lane cuts of resident_plan_ref.lane_cuts: all of them in the scan with the
            most lanes (the 'long scan'), some in the others
  offcut    `lanecut` with one such boundary moved by one record into a lane of two or more records: to be refused
Weight rows on scan / multi / lanecut (ROW_KINDS): every row meant to be solved keeps at least 8 scans and materialises to at most
2e5 records — asserted here — except wave0_on, which may keep fewer (Row.pinned says so)."""
import functools

import numpy as np

import resident_plan_ref as R
import test_gpu_batched_fuzz as BF   # Pool, edge_lens, EDGES, NL (the module is imported, not its tests)
from camlasercalibratool_amd import resample, simdata as sd

SEED = 20261018
EDGES = BF.EDGES
NL = BF.NL
FORMS = (256, 512, "z")
STYLES = ("short", "split", "dense")
CASES = [(form, t) for form in FORMS for t in EDGES[form]]
SOLVE_CUTS = ("scan", "multi", "lanecut")
SCORE_CUTS = ("scan", "multi", "multi300", "multi2nl", "lanecut")
ROW_KINDS = ("ones", "rand01", "rand01_sparse", "bootstrap", "bootstrap_nonempty", "mult255", "wave0_off", "wave0_on", "wave0_dead",
             "zeros", "empties_only")          # + "alt03" on lanecut; empties_only where the cut has empty blocks
DEGENERATE = ("zeros", "empties_only")
MIN_SCANS = 8
MAX_RECORDS = 200_000


class _Reject(Exception):
    """This draw does not give the case what it needs: the builder draws again (same stream)."""


class Row:
    def __init__(self, kind, w, scans, records):
        self.kind, self.w, self.scans, self.records = kind, w, scans, records
        self.degenerate = kind in DEGENERATE
        self.pinned = scans >= MIN_SCANS     # enough scans to pin the pose: T_cl is gated


class Cut:
    def __init__(self, name, off):
        self.name, self.off = name, np.ascontiguousarray(off, dtype=np.int64)
        self.rows = {}
        self.inside = np.zeros(0, dtype=np.int64)    # (lanecut, offcut) the boundaries inside scans
        self.long_blocks = np.zeros(0, dtype=np.int64)  # (lanecut) the consecutive lane-blocks of the long scan

    @property
    def n_blocks(self):
        return self.off.size - 1

    @property
    def empty(self):
        return np.diff(self.off) == 0

    def W(self, kinds=None):
        kinds = list(self.rows) if kinds is None else kinds
        return np.stack([self.rows[k].w for k in kinds])


class Case:
    pass


@functools.lru_cache(maxsize=None)
def pool():
    return BF.Pool(SEED, BF.N_SCANS, BF.K, 0.01)


def lane_blocks(off, first, cnt):
    """-> (block of every used lane, served): the block with off[b] <= first < off[b + 1]; served: no lane reaches beyond its block."""
    used = cnt > 0
    b = np.searchsorted(off, first[used], side="right") - 1
    return b, bool(np.all(first[used] + cnt[used] <= off[b + 1]))


def pose_plus(x, d):
    """p + dp, q * [dtheta / 2, 1] normalised (what resample.local_delta inverts)."""
    q = resample._quat_mul(x[3:7], np.array([0.5 * d[3], 0.5 * d[4], 0.5 * d[5], 1.0]))
    return np.concatenate([x[0:3] + d[0:3], q / np.linalg.norm(q)])


def _add_split_scan(lens, t, rng):
    """'short' style: q of the scans below t points (one lane each at t and at t - 1 points per lane) make room for one scan of
    q t - r points, 0 <= r < q: q lanes or fewer at t, more than q at t - 1 — the points per lane stay t."""
    q = int(rng.integers(2, 5))
    r = int(rng.integers(0, q))
    small = np.flatnonzero(lens < t)
    if small.size < q or q * t - r > BF.K:
        raise _Reject
    keep = np.delete(lens, rng.choice(small, q, replace=False))
    return np.insert(keep, int(rng.integers(0, keep.size + 1)), q * t - r)


def _problem_lens(form, t, rng, style):
    nl = NL[form]
    lens = BF.edge_lens(nl, t, rng, style if t > 1 else "short")
    if t > 1 and style == "short":
        lens = _add_split_scan(lens, t, rng)
    if len(lens) < 16 or R.problem_ppl(lens, nl, 10**6) != t:
        raise _Reject
    if form == 512 and R.problem_ppl(lens, 256, R.CAP[256]) is not None:   # (it would be served on 256 lanes)
        raise _Reject
    return lens


def _with_empties(off, n_blocks, rng):
    """Offsets with repeated values added until there are n_blocks blocks."""
    extra = n_blocks - (off.size - 1)
    assert extra >= 0, (off.size - 1, n_blocks)
    return np.sort(np.concatenate([off, rng.choice(off, extra)]))


def _multi_cut(starts, n, rng):
    ns = starts.size
    firsts, s = [], 0
    while s < ns:
        firsts.append(s)
        s += int(rng.integers(1, 6))
    off = np.append(starts[firsts], n)
    mid = off[1:-1]
    runs = [np.repeat(0, int(rng.integers(1, 4))), np.repeat(n, int(rng.integers(1, 4)))]
    if mid.size:
        for v in rng.choice(mid, min(3, mid.size), replace=False):
            runs.append(np.repeat(v, int(rng.integers(1, 5))))
    return np.sort(np.concatenate([off] + runs))


def _lane_cut(multi, lens, scan, first, cnt, rng):
    """-> Cut: multi + boundaries inside the scans of two or more lanes, on lane cuts."""
    used = cnt > 0
    lanes_of = np.bincount(scan[used], minlength=lens.size)
    if lanes_of.max() < 2:
        raise _Reject
    long_scan = int(np.argmax(lanes_of))
    inner = used & (np.concatenate([[-1], scan[:-1]]) == scan)       # a lane that is not its scan's first
    take = inner & ((scan == long_scan) | (rng.random(scan.size) < 0.3))
    cut = Cut("lanecut", np.sort(np.concatenate([multi.off, first[take]])))
    cut.inside = first[take]
    # (the first and the last of them may hold neighbouring scans too, where the scan does not start or end a block of `multi`)
    cut.long_blocks = np.unique(lane_blocks(cut.off, first, cnt)[0][scan[used] == long_scan])
    assert cut.long_blocks.size == lanes_of[long_scan] and np.all(np.diff(cut.long_blocks) == 1)
    return cut


def _off_cut(lanecut, first, cnt, rng):
    """-> Cut: one inside boundary moved by one record into a lane of two or more records."""
    used = np.flatnonzero(cnt > 0)
    cands = []
    for v in lanecut.inside:
        t = int(used[np.searchsorted(first[used], v)])   # the lane that starts at v
        if cnt[t] >= 2:
            cands.append((v, v + 1))
        if cnt[t - 1] >= 2:
            cands.append((v, v - 1))
    if not cands:
        raise _Reject
    v, moved = cands[int(rng.integers(0, len(cands)))]
    off = lanecut.off.copy()
    off[int(np.flatnonzero(off == v)[0])] = moved
    cut = Cut("offcut", np.sort(off))
    cut.inside = np.array([moved])
    return cut


def _row(kind, w, cut, scan, cnt, lb):
    w = np.asarray(w)
    assert w.shape == (cut.n_blocks,) and w.min() >= 0 and w.max() <= 255, kind
    w = w.astype(np.uint8)
    scans = int(np.unique(scan[cnt > 0][w[lb] > 0]).size)
    records = int((w.astype(np.int64) * np.diff(cut.off)).sum())
    row = Row(kind, w, scans, records)
    if row.degenerate:
        assert records == 0, kind
    elif records > MAX_RECORDS or (scans < MIN_SCANS and kind != "wave0_on") or records == 0:
        raise _Reject
    return row


def _rows(cut, scan, first, cnt, rng):
    B, size, ne = cut.n_blocks, np.diff(cut.off), ~cut.empty
    lb, served = lane_blocks(cut.off, first, cnt)
    assert served, cut.name
    mk = lambda kind, w: _row(kind, w, cut, scan, cnt, lb)   # noqa: E731
    rows = {"ones": mk("ones", np.ones(B, dtype=np.int64))}
    rows["rand01"] = mk("rand01", (rng.random(B) < 0.6).astype(np.int64))
    rows["rand01_sparse"] = mk("rand01_sparse", (rng.random(B) < 0.3).astype(np.int64))
    rows["bootstrap"] = mk("bootstrap", np.bincount(rng.integers(0, B, B), minlength=B))
    nei = np.flatnonzero(ne)
    rows["bootstrap_nonempty"] = mk("bootstrap_nonempty", np.bincount(nei[rng.integers(0, nei.size, nei.size)], minlength=B))
    w = rng.integers(2, 8, B)
    room = MAX_RECORDS - int((w * size).sum())
    fits = nei[(255 - w[nei]) * size[nei] <= room]
    if fits.size == 0:
        raise _Reject
    w[int(rng.choice(fits))] = 255
    rows["mult255"] = mk("mult255", w)
    # wave 0 (lanes 0..63) is the controller wave
    lanes = np.flatnonzero(cnt > 0)
    touch = np.zeros(B, dtype=bool)
    touch[lb[lanes < 64]] = True
    beyond = np.zeros(B, dtype=bool)
    beyond[lb[lanes >= 64]] = True
    inside0 = touch & ~beyond
    if not inside0.any():
        raise _Reject
    rows["wave0_off"] = mk("wave0_off", np.where(inside0, 0, 1))      # a block that straddles lanes 63 | 64 keeps wave 0 alive
    rows["wave0_on"] = mk("wave0_on", np.where(inside0, 1, 0))
    rows["wave0_dead"] = mk("wave0_dead", np.where(touch, 0, 1))      # every lane of wave 0 at weight 0
    if cut.name == "lanecut":
        w = np.ones(B, dtype=np.int64)
        w[cut.long_blocks] = np.where(np.arange(cut.long_blocks.size) % 2 == 0, 0, 3)
        rows["alt03"] = mk("alt03", w)
    rows["zeros"] = mk("zeros", np.zeros(B, dtype=np.int64))
    if (~ne).any():
        w = np.zeros(B, dtype=np.int64)
        w[~ne] = rng.integers(1, 256, int((~ne).sum()))
        rows["empties_only"] = mk("empties_only", w)
    return rows


def _build(index, form, t):
    rng = np.random.default_rng([SEED, index])
    nl = NL[form]
    want_style = STYLES[index % 3] if t > 1 else "short"
    for attempt in range(400):
        style = want_style if attempt < 300 else "split"
        try:
            lens = _problem_lens(form, t, rng, style)
            scan, first, cnt = R.lane_cuts(lens, nl, t)
            if t > 1 and not np.any((cnt > 0) & (cnt < t)):
                raise _Reject
            n = int(lens.sum())
            starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
            cuts = {"scan": Cut("scan", np.append(starts, n))}
            cuts["multi"] = Cut("multi", _multi_cut(starts, n, rng))
            cuts["multi300"] = Cut("multi300", _with_empties(cuts["multi"].off, 300, rng))
            cuts["multi2nl"] = Cut("multi2nl", _with_empties(cuts["multi"].off, 2 * nl + 1, rng))
            if t > 1:
                cuts["lanecut"] = _lane_cut(cuts["multi"], lens, scan, first, cnt, rng)
                cuts["offcut"] = _off_cut(cuts["lanecut"], first, cnt, rng)
                assert not lane_blocks(cuts["offcut"].off, first, cnt)[1]
            for name in SOLVE_CUTS:
                if name in cuts:
                    cuts[name].rows = _rows(cuts[name], scan, first, cnt, rng)
        except _Reject:
            continue
        break
    else:
        raise AssertionError((form, t, "no admissible draw"))
    c = Case()
    c.index, c.form, c.t, c.style, c.nl, c.lens, c.cuts = index, form, t, style, nl, lens, cuts
    c.scan, c.first, c.cnt = scan, first, cnt
    p = pool()
    c.rec = p.build(p.pieces(lens, rng))
    if form == "z":
        BF._with_z([c.rec], rng)
    c.use_loss = index % 5 != 3
    d = rng.uniform(0.01, 0.02, 6) * rng.choice([-1.0, 1.0], 6)     # 1-2 cm, 0.01-0.02 rad off the truth
    c.x0 = pose_plus(p.gt, d)
    c.gt = p.gt
    for cut in cuts.values():
        assert cut.off[0] == 0 and cut.off[-1] == c.rec.shape[0] and np.all(np.diff(cut.off) >= 0), cut.name
    return c


@functools.lru_cache(maxsize=None)
def case(form, t):
    return _build(CASES.index((form, t)), form, t)


def past_capacity_lens(form):
    """Scan lengths one point per lane past the form's capacity: 256 lanes at 43 (served on 512 lanes), 512 lanes / z at 23 (not held
    by a workgroup)."""
    rng = np.random.default_rng([SEED, 1000 + FORMS.index(form)])
    for _ in range(200):
        if form == 256:
            lens = BF.edge_lens(256, 43, rng, "short")
            plan = R.plan_lens([lens], 0, False)
            if plan.form == 512 and len(lens) >= 16:
                return lens
        else:
            lens = BF.edge_lens(512, 23, rng, "dense")
            if not R.plan_lens([lens], 0, form == "z").resident:
                return lens
    raise AssertionError(form)


def past_capacity_records(form):
    rng = np.random.default_rng([SEED, 2000 + FORMS.index(form)])
    p = pool()
    rec = p.build(p.pieces(past_capacity_lens(form), rng))
    if form == "z":
        BF._with_z([rec], rng)
    return rec


TINY_R0 = (2e-6, -2.5e-6, 3e-6, -4e-6)


def tiny_residual_problem():
    """The regression shape of the block scores' logarithm: 32 scans of ONE record, one block each, whose planes are shifted so that
    the record lies TINY_R0 (micrometres) off its plane at the ground truth.  r0^2 / lf^2 is then ~2e-9, and log(fl(1 + x)) is off by
    up to 1.1e-16 / x = 6e-8 of itself — which a block of one record shows in its cost, where a pose's hundred records hide it.
    -> (records [32, 8], block offsets [33], pose [7], the wanted r0 per record)."""
    p = pool()
    rng = np.random.default_rng([SEED, 3000])
    rec = p.build(p.pieces(np.ones(32, dtype=np.int64), rng)).copy()
    T = sd.T_from_pose7(p.gt)
    r0 = np.einsum("ij,ij->i", rec[:, 0:3], rec[:, 4:7] @ T[:3, :3].T + T[:3, 3]) + rec[:, 3]
    want = np.resize(np.array(TINY_R0), 32)
    rec[:, 3] += want - r0
    return rec, np.arange(33, dtype=np.int64), p.gt, want
