"""Seeded shape fuzz of clc_solve_subsets (the WEIGHTED resident_solve_kernel + subset_lane_map_kernel) and clc_score_blocks
(block_scores_kernel) at the lane and block edges, on the constructed cases of tests/subsets_fuzz_cases.py (checked without a GPU by
tests/test_subsets_fuzz_cases.py): one problem per (form, points per lane) on the capacity edges of the resident kernel, every one with
padded lanes, cut into blocks per scan, per 1-5 scans with empty blocks (up to 2 NL + 1 blocks), and on lane cuts INSIDE scans.

Per case: path_info() equals the planner's restatement; every weight row against the oracle's DENSE_QR solve of the materialised
records inside the gates of test_gpu_subsets.py (|dT|inf <= 1e-6, |d final cost| <= 1e-8, same termination and iteration count; a flip
only as a near tie of the oracle's own trace, at most one row per case and 1 % of the module's rows — the oracle alone stays inside
that cap: test_subsets_fuzz_cases.py); the all-ones row bitwise clc_solve_multistart; a second call, a row alone and the neighbours of
the degenerate rows bitwise; block scores of 16 poses against the oracle's residuals (the helpers, tolerance and exact inlier counts
of test_gpu_consensus.py), empty blocks exactly 0 / 0 / 0 and a non-finite pose NaN / NaN / 0 in every block, also past index NL; the
two kernels against each other (initial cost = sum_b w_b cost[start, b]; refining a cut keeps the block sums); a boundary one record
off a lane cut refused by both calls, the handle and the map left usable.  The last test prints what the module saw."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import camlasercalibratool_amd as clc
import lm_near_tie as NT
import resident_plan_ref as R
import subsets_fuzz_cases as F
import test_gpu_batched_fuzz as BF
import test_gpu_consensus as GC
from camlasercalibratool_amd import _capi, resample, simdata as sd

pytestmark = pytest.mark.gpu

T_TOL = 1e-6            # the gates of test_gpu_subsets.py
COST_TOL = 1e-8
EXCUSED_SHARE = 0.01
EXCUSED_PER_CASE = 1
REL_TOL = GC.REL_TOL    # block scores against the oracle, and the two kernels against each other
N_POSES, START, BAD = 16, 1, 6     # score poses: index START (< BAD) is the solves' start pose, index BAD is made non-finite
STATS = {"rows": 0, "excused": 0, "dT": 0.0, "dcost": 0.0, "ssq": 0.0, "cost": 0.0, "initial": 0.0, "refine": 0.0, "cases": {}}
FAILURE = {v: k for k, v in _capi.TERMINATION.items()}["FAILURE"]
IDS = [f"{f}-ppl{t}" for f, t in F.CASES]
PAST_CAPACITY_ROWS = 4


@pytest.fixture(scope="module")
def sv():
    with clc.Solver(0) as s:
        if not s._L.has_hooks:
            pytest.fail("the suite runs on the hooks build (tests/conftest.py)")
        yield s


@pytest.fixture(scope="module")
def workers(oracle_mod):
    with ThreadPoolExecutor(max_workers=min(16, oracle_mod.max_threads())) as ex:
        yield ex


def _module_rows():
    """Rows this module gates against the oracle when all of it runs: known from the cases alone, so the module's cap on excused rows
    does not depend on which tests were selected, or in what order they ran."""
    return PAST_CAPACITY_ROWS + sum(not row.degenerate for f, t in F.CASES for n in F.SOLVE_CUTS if n in F.case(f, t).cuts
                                    for row in F.case(f, t).cuts[n].rows.values())


def _excuse(label, excused):
    """A test's near-tie exemptions: at most one per case, and the running total inside 1 % of the module's rows — asserted where they
    arise (whatever the selection or order of the tests)."""
    assert excused <= EXCUSED_PER_CASE, (label, excused)
    STATS["excused"] += excused
    assert STATS["excused"] <= EXCUSED_SHARE * _module_rows(), (label, STATS["excused"], _module_rows())


def _dT(a, b):
    return float(np.abs(sd.T_from_pose7(a) - sd.T_from_pose7(b)).max())


def _same(pa, sa, i, pb, sb, j):
    return np.array_equal(pa[i], pb[j]) and BF._key(sa[i]) == BF._key(sb[j])


def _upload(sv, rec):
    off1 = np.array([0, rec.shape[0]], dtype=np.int64)
    plan = R.plan(rec, off1)
    sv.upload_batched(rec, off1)
    assert BF._path(sv) == plan.path_info(), (BF._path(sv), plan.path_info())
    return plan


def _score_poses(oracle_mod, c, seed):
    poses = GC._poses(oracle_mod, N_POSES, seed, c.gt)   # the truth, millimetres to decimetres away, and 12 poses metres / radians away
    poses[START] = c.x0
    bad = poses.copy()
    bad[BAD, seed % 7] = (np.nan, np.inf, -np.inf)[seed % 3]
    return poses, bad


def _check_scores(sv, oracle_mod, label, rec, cut, poses, bad, o, use_loss, tau):
    """score_blocks on `cut` against the oracle's tables; -> (ssq, cost, inl) with the BAD row checked and then left out."""
    ok = np.arange(N_POSES) != BAD
    want_q, want_c, r0 = GC._oracle_tables(oracle_mod, rec, cut.off, poses[ok], use_loss)
    assert np.abs(np.abs(r0) - tau).min() > GC.TAU_MARGIN
    want_i = np.stack([GC._group((np.abs(r) <= tau).astype(np.int64), cut.off) for r in r0])
    ssq, cost, inl = sv.score_blocks(cut.off, bad, tau, o)
    assert ssq.shape == cost.shape == inl.shape == (N_POSES, cut.n_blocks) and inl.dtype == np.int32
    assert np.isnan(ssq[BAD]).all() and np.isnan(cost[BAD]).all() and not inl[BAD].any(), (label, "the non-finite pose")
    ssq, cost, inl = ssq[ok], cost[ok], inl[ok]
    e = cut.empty
    assert not ssq[:, e].any() and not cost[:, e].any() and not inl[:, e].any(), (label, "empty blocks")
    assert np.all(ssq[:, ~e] > 0) and np.all(cost[:, ~e] > 0)
    rq, rc = GC._rel(ssq, want_q), GC._rel(cost, want_c)
    print(f"{label}: {cut.n_blocks} blocks ({int(e.sum())} empty), tau {tau:.6f}: relative difference ssq {rq:.3e} cost {rc:.3e}, "
          f"differing inlier cells {int((inl != want_i).sum())}")
    assert rq <= REL_TOL and rc <= REL_TOL, (label, rq, rc)
    assert np.array_equal(inl, want_i), label
    STATS["ssq"], STATS["cost"] = max(STATS["ssq"], rq), max(STATS["cost"], rc)
    return ssq, cost, inl


def _gate_rows(oracle_mod, workers, label, rec, off, rows, x0, oo, poses, sms):
    """rows: [(index into poses / sms, Row)] of the solved rows -> number of near-tie exemptions."""
    subs = [resample.materialize(rec, off, row.w) for _, row in rows]
    refs = list(workers.map(lambda sub: oracle_mod.solve(sub, x0, oo, linear_solver="qr"), subs))
    excused = 0
    for (k, row), sub, ref in zip(rows, subs, refs):
        got = (sms[k].termination, sms[k].num_iterations, sms[k].final_cost)
        want = (ref.summary.termination, ref.summary.num_iterations, ref.summary.final_cost)
        dT, dc = _dT(poses[k], ref.pose), abs(got[2] - want[2])
        print(f"{label} {row.kind}: scans {row.scans} records {row.records} w max {int(row.w.max())} it {got[1]}/{want[1]} "
              f"term {got[0]}/{want[0]} dT {dT:.3e} dcost {dc:.3e}")
        STATS["rows"] += 1
        if NT.check_flip(oracle_mod, sub, x0, oo, got, want, f"{label} {row.kind}"):
            excused += 1
            continue
        assert dc <= COST_TOL, (label, row.kind, got, want)
        STATS["dcost"] = max(STATS["dcost"], dc)
        if row.pinned:   # (fewer than 8 scans do not pin the pose: cost, termination and iteration count only)
            assert dT <= T_TOL, (label, row.kind, dT)
            STATS["dT"] = max(STATS["dT"], dT)
    return excused


def _solve_cut(sv, oracle_mod, workers, label, c, cut, o, oo, ms, cost_at_start, rng):
    kinds = list(cut.rows)
    W = cut.W(kinds)
    solved = [i for i, k in enumerate(kinds) if not cut.rows[k].degenerate]
    poses, sms = sv.solve_subsets(cut.off, W, c.x0, o)
    again, asm = sv.solve_subsets(cut.off, W, c.x0, o)
    assert all(_same(poses, sms, i, again, asm, i) for i in range(len(kinds))), (label, "a second call")
    i1 = kinds.index("ones")
    assert _same(poses, sms, i1, ms[0], ms[1], 0), (label, "the all-ones row against clc_solve_multistart")
    for i, k in enumerate(kinds):
        if cut.rows[k].degenerate:
            assert sms[i].termination == FAILURE and np.array_equal(poses[i], c.x0), (label, k)
    crowd, csm = sv.solve_subsets(cut.off, W[solved], c.x0, o)       # without the degenerate rows: the neighbours' bits are the same
    assert all(_same(poses, sms, i, crowd, csm, j) for j, i in enumerate(solved)), (label, "next to the degenerate rows")
    i = int(rng.choice(solved))
    one, osm = sv.solve_subsets(cut.off, W[i:i + 1], c.x0, o)
    assert _same(poses, sms, i, one, osm, 0), (label, "alone", kinds[i])
    # the two kernels against each other: the cost a solve starts from = the block costs at the start pose, weighted
    for i in solved:
        want = float((W[i].astype(np.float64) * cost_at_start).sum())
        rel = abs(sms[i].initial_cost - want) / want
        STATS["initial"] = max(STATS["initial"], rel)
        assert rel <= REL_TOL, (label, kinds[i], sms[i].initial_cost, want)
    return _gate_rows(oracle_mod, workers, label, c.rec, cut.off, [(i, cut.rows[kinds[i]]) for i in solved], c.x0, oo, poses, sms), \
        (W[solved[:3]], crowd[:3], csm[:3])


@pytest.mark.parametrize("form,t", F.CASES, ids=IDS)
def test_subsets_and_scores_at_the_edge(sv, oracle_mod, workers, form, t):
    c = F.case(form, t)
    rng = np.random.default_rng([F.SEED, 77, c.index])
    o, oo = BF._options(c.use_loss, oracle_mod)
    plan = _upload(sv, c.rec)
    assert plan.form == form and plan.max_ppl == t
    label = f"{form} ppl {t} {c.style}{'' if c.use_loss else ' no loss'}"
    ms = sv.solve_multistart(c.x0[None], o)
    poses, bad = _score_poses(oracle_mod, c, c.index)
    r0 = GC._oracle_tables(oracle_mod, c.rec, np.array([0, c.rec.shape[0]], dtype=np.int64), poses[np.arange(N_POSES) != BAD], c.use_loss)[2]
    tau = GC._pick_tau(r0)
    # ---- scores on every cut
    sc = {}
    for name in F.SCORE_CUTS:
        if name in c.cuts:
            sc[name] = _check_scores(sv, oracle_mod, f"{label} {name}", c.rec, c.cuts[name], poses, bad, o, c.use_loss, tau)
    ne = ~c.cuts["multi"].empty
    for name in ("multi300", "multi2nl"):      # more empty blocks: the same lanes added in the same order
        e = ~c.cuts[name].empty
        assert all(np.array_equal(a[:, e], b[:, ne]) for a, b in zip(sc[name], sc["multi"])), (label, name)
    if "lanecut" in sc:                         # refining a cut leaves the block sums unchanged
        m, l = c.cuts["multi"], c.cuts["lanecut"]
        lne = np.flatnonzero(~l.empty)
        parent = np.searchsorted(m.off, l.off[lne], side="right") - 1
        for a, b, exact in zip(sc["lanecut"], sc["multi"], (False, False, True)):
            s = np.zeros_like(b)
            np.add.at(s, (slice(None), parent), a[:, lne])
            if exact:
                assert np.array_equal(s, b), (label, "inliers under refinement")
            else:
                STATS["refine"] = max(STATS["refine"], float(np.abs(s - b).max() / b.max()))
                assert np.abs(s - b).max() <= 1e-12 * b.max(), (label, "sums under refinement")
    # ---- solves
    excused, kept = 0, None
    for name in F.SOLVE_CUTS:
        if name in c.cuts:
            ex, kept = _solve_cut(sv, oracle_mod, workers, f"{label} {name}", c, c.cuts[name], o, oo, ms, sc[name][1][START], rng)
            excused += ex
    _excuse(label, excused)
    # ---- a boundary one record off a lane cut: refused by both calls; the handle and the previous map's offsets still serve
    if t > 1:
        l, bad_cut = c.cuts["lanecut"], c.cuts["offcut"]
        n0 = GC._map_builds()       # (the lane cut's map is the current one)
        for call in (lambda: sv.solve_subsets(bad_cut.off, np.ones((1, bad_cut.n_blocks), dtype=np.uint8), c.x0, o),
                     lambda: sv.score_blocks(bad_cut.off, poses, tau, o)):
            with pytest.raises(clc.ClcError, match="CLC_ERR_INVALID_ARG") as e:
                call()
            assert "whole scans" in str(e.value)
        q = sv.score_blocks(l.off, bad, tau, o)
        okr = np.arange(N_POSES) != BAD
        assert all(np.array_equal(a[okr], b) for a, b in zip(q, sc["lanecut"])), (label, "scores after the refusals")
        p, s = sv.solve_subsets(l.off, kept[0], c.x0, o)
        assert all(_same(p, s, j, kept[1], kept[2], j) for j in range(len(s))), (label, "solves after the refusals")
        assert GC._map_builds() == n0 + 3, (label, "two refused builds and one rebuild")
    st = STATS["cases"].setdefault(str(form), {"ppl": [], "styles": set(), "cuts": set(), "kinds": set()})
    st["ppl"].append(t)
    st["styles"].add(c.style)
    st["cuts"].update(c.cuts)
    st["kinds"].update(k for n in F.SOLVE_CUTS if n in c.cuts for k in c.cuts[n].rows)


def _plain_rows(n_blocks, seed):
    rng = np.random.default_rng(seed)
    w = np.stack([np.ones(n_blocks, dtype=np.int64), (rng.random(n_blocks) < 0.6).astype(np.int64),
                  np.bincount(rng.integers(0, n_blocks, n_blocks), minlength=n_blocks), rng.integers(2, 8, n_blocks)])
    return w.astype(np.uint8)


def test_one_past_capacity_256_lanes_moves_to_512(sv, oracle_mod, workers):
    """43 points per lane at 256 lanes: the problem is held on 512 lanes and both calls serve it."""
    rec = F.past_capacity_records(256)
    plan = _upload(sv, rec)
    assert plan.form == 512 and BF._path(sv)[:2] == (1, 512)
    lens = R.scan_lengths(rec, [0, rec.shape[0]])[0]
    assert R.problem_ppl(lens, 256, 10**6) == 43
    c = F.Case()
    c.rec, c.gt, c.index = rec, F.pool().gt, 0
    c.x0 = F.pose_plus(c.gt, np.array([.015, -.012, .018, -.011, .02, .013]))
    cut = F.Cut("scan", np.concatenate([[0], np.cumsum(lens)]))
    o, oo = BF._options(True, oracle_mod)
    poses, bad = _score_poses(oracle_mod, c, 21)
    r0 = GC._oracle_tables(oracle_mod, rec, cut.off, poses[np.arange(N_POSES) != BAD], True)[2]
    _check_scores(sv, oracle_mod, "256 lanes past capacity", rec, cut, poses, bad, o, True, GC._pick_tau(r0))
    W = _plain_rows(cut.n_blocks, 5)
    p, s = sv.solve_subsets(cut.off, W, c.x0, o)
    ms = sv.solve_multistart(c.x0[None], o)
    assert _same(p, s, 0, ms[0], ms[1], 0)
    rows = [(i, F.Row(k, W[i], int(np.count_nonzero(W[i])), int((W[i].astype(np.int64) * lens).sum())))   # (a block is a scan)
            for i, k in enumerate(("ones", "rand01", "bootstrap", "mult"))]
    assert all(row.pinned for _, row in rows)
    ex = _gate_rows(oracle_mod, workers, "256 lanes past capacity", rec, cut.off, rows, c.x0, oo, p, s)
    assert len(rows) == PAST_CAPACITY_ROWS
    _excuse("256 lanes past capacity", ex)


@pytest.mark.parametrize("form", [512, "z"], ids=["512", "z"])
def test_one_past_capacity_512_lanes_is_refused(sv, oracle_mod, form):
    """23 points per lane at 512 lanes (with and without z): no workgroup holds the problem; both calls say so."""
    rec = F.past_capacity_records(form)
    plan = _upload(sv, rec)
    assert not plan.resident and sv.path_info().batched_resident == 0
    lens = R.scan_lengths(rec, [0, rec.shape[0]])[0]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x0 = F.pool().gt
    for call in (lambda: sv.solve_subsets(off, np.ones((2, len(lens)), dtype=np.uint8), x0),
                 lambda: sv.score_blocks(off, x0[None], 0.03)):
        with pytest.raises(clc.ClcError, match="CLC_ERR_INVALID_ARG") as e:
            call()
        assert "workgroup" in str(e.value)


def test_solve_subsets_refuses_weights_that_do_not_fit_a_byte(sv):
    """256 used to wrap to 0 — a block silently left out: refused on the host (resample.as_weight_rows), nothing is launched."""
    c = F.case(256, 3)
    _upload(sv, c.rec)
    cut = c.cuts["scan"]
    for wrong in (256, -1, 2.5):
        w = np.ones((2, cut.n_blocks), dtype=np.float64)
        w[1, 3] = wrong
        with pytest.raises(ValueError):
            sv.solve_subsets(cut.off, w, c.x0)
    with pytest.raises(ValueError):
        sv.solve_subsets(cut.off, np.ones((2, cut.n_blocks + 1), dtype=np.uint8), c.x0)
    p, s = sv.solve_subsets(cut.off, np.ones((1, cut.n_blocks)), c.x0)       # integral floats are weights
    q, r = sv.solve_subsets(cut.off, np.ones(cut.n_blocks, dtype=np.uint8), c.x0)
    assert _same(p, s, 0, q, r, 0)


def test_scores_of_one_record_blocks_with_micrometre_residuals(sv, oracle_mod):
    """Regression (found by the scan cut of the 256-lane ppl 2 case, measured on an MI355X: one block's cost 4.3e-8 off, relative): blocks of one record a few micrometres off their
    plane.  block_scores_kernel took log(fl(1 + r0^2 / lf^2)), which loses the low bits of an argument of ~2e-9 — up to 6e-8 of the
    block's cost; it now takes log1p.  Against the oracle's tables at REL_TOL, as every other score."""
    rec, off, x, want = F.tiny_residual_problem()
    _upload(sv, rec)
    poses = GC._poses(oracle_mod, 16, 31, x)[:4]       # the pose the residuals were set at, and three near it
    r0 = GC._oracle_tables(oracle_mod, rec, off, poses[:1])[2][0]
    assert np.abs(r0 / want - 1.0).max() <= 1e-8       # (the oracle sees the residuals the problem was built with)
    _, _, _, rq, rc = GC._check_case(oracle_mod, sv, "one-record blocks, micrometre residuals", rec, off, poses)
    STATS["ssq"], STATS["cost"] = max(STATS["ssq"], rq), max(STATS["cost"], rc)


def test_summary_of_the_module():
    """What the tests of this module that ran before this one exercised, the worst differences they saw, and their excused rows against
    the module's cap (which every test also asserts as it goes: _excuse).  With the whole module selected: every edge was there."""
    for form, st in STATS["cases"].items():
        print(f"subsets fuzz [{form}]: ppl {sorted(st['ppl'])}, styles {sorted(st['styles'])}, cuts {sorted(st['cuts'])}, "
              f"rows {sorted(st['kinds'])}")
    print(f"subsets fuzz: {STATS['rows']} of the module's {_module_rows()} rows against the oracle, {STATS['excused']} excused as near ties "
          f"(cap {int(EXCUSED_SHARE * _module_rows())}); worst |dT| {STATS['dT']:.3e} |dcost| {STATS['dcost']:.3e}; block scores relative ssq "
          f"{STATS['ssq']:.3e} cost {STATS['cost']:.3e}; initial cost against weighted block costs {STATS['initial']:.3e}; "
          f"block sums under refinement {STATS['refine']:.3e} of the largest cell")
    assert STATS["excused"] <= EXCUSED_SHARE * _module_rows(), (STATS["excused"], _module_rows())
    if STATS["rows"] == _module_rows():   # (the whole module ran)
        for form in F.FORMS:
            assert sorted(STATS["cases"][str(form)]["ppl"]) == sorted(F.EDGES[form])
