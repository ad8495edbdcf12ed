"""The constructed cases of tests/subsets_fuzz_cases.py, checked without a GPU: every (form, points per lane) edge gets the plan it was
built for, every cut and row kind it is meant to have, rows that keep enough scans and stay small, and lanes with padding; the cuts
are what they claim (served on lane cuts, refused one record off).

And the reference alone: the oracle's own trace of every solved row's materialised problem is scanned for near ties (lm_near_tie).  The
GPU test (tests/test_gpu_subsets_fuzz.py) excuses a difference in iteration count or termination only at such a tie, for at most 1 % of
the module's rows and at most one row per case — so the oracle's own share of near ties, for the seed chosen in subsets_fuzz_cases.py,
must lie inside that cap.  It is printed."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import lm_near_tie as NT
import resident_plan_ref as R
import subsets_fuzz_cases as F
from camlasercalibratool_amd import resample

EXCUSED_SHARE = 0.01     # of all rows of the module
EXCUSED_PER_CASE = 1


@pytest.mark.parametrize("form,t", F.CASES, ids=[f"{f}-ppl{t}" for f, t in F.CASES])
def test_case_is_what_it_was_built_for(form, t):
    c = F.case(form, t)
    off1 = np.array([0, c.rec.shape[0]], dtype=np.int64)
    plan = R.plan(c.rec, off1)
    assert plan.form == form and plan.ppl == [t], (plan.path_info(), plan.ppl)
    assert [int(v) for v in R.scan_lengths(c.rec, off1)[0]] == [int(v) for v in c.lens] and len(c.lens) >= 16
    scan, first, cnt = R.lane_cuts(c.lens, F.NL[form], t)
    used = cnt > 0
    assert t == 1 or np.any(cnt[used] < t), "no lane with padding"
    assert cnt.max() == t
    want_cuts = {"scan", "multi", "multi300", "multi2nl"} | ({"lanecut", "offcut"} if t > 1 else set())
    assert set(c.cuts) == want_cuts
    n = c.rec.shape[0]
    starts = np.concatenate([[0], np.cumsum(c.lens)])
    for name, cut in c.cuts.items():
        assert cut.off[0] == 0 and cut.off[-1] == n and np.all(np.diff(cut.off) >= 0), name
        lb, served = F.lane_blocks(cut.off, first, cnt)
        assert served == (name != "offcut"), name
        if name in ("scan", "multi", "multi300", "multi2nl"):
            assert np.isin(cut.off, starts).all(), name         # whole scans
    assert np.array_equal(c.cuts["scan"].off, starts) and not c.cuts["scan"].empty.any()
    e = c.cuts["multi"].empty
    ne = np.flatnonzero(~e)
    assert e[0] and e[-1] and np.any(e[ne[0]:ne[-1]]), "empty blocks at the front, at the back and in the middle"
    sizes = np.diff(np.searchsorted(starts, c.cuts["multi"].off[np.concatenate([ne, [ne[-1] + 1]])]))
    assert sizes.min() >= 1 and sizes.max() <= 5
    assert c.cuts["multi300"].n_blocks == 300 and c.cuts["multi2nl"].n_blocks == 2 * F.NL[form] + 1
    for name in ("multi300", "multi2nl"):
        assert np.array_equal(np.unique(c.cuts[name].off), np.unique(c.cuts["multi"].off)), name
    if t > 1:
        lc, oc = c.cuts["lanecut"], c.cuts["offcut"]
        assert lc.inside.size >= 1 and not np.isin(lc.inside, starts).any() and np.isin(lc.inside, first[used]).all()
        assert np.array_equal(np.unique(lc.off), np.union1d(c.cuts["multi"].off, lc.inside))
        assert lc.long_blocks.size >= 2
        moved = np.setdiff1d(oc.off, lc.off)
        assert moved.size == 1 and not np.isin(moved, first[used]).any() and oc.n_blocks == lc.n_blocks
        k = int(np.flatnonzero((first <= moved[0]) & (moved[0] < first + cnt))[0])
        assert cnt[k] >= 2 and (np.isin(moved[0] - 1, lc.inside) or np.isin(moved[0] + 1, lc.inside))
    for name in F.SOLVE_CUTS:
        if name not in c.cuts:
            continue
        cut = c.cuts[name]
        want_rows = set(F.ROW_KINDS) | ({"alt03"} if name == "lanecut" else set())
        if not cut.empty.any():
            want_rows -= {"empties_only"}
        assert set(cut.rows) == want_rows, (name, sorted(cut.rows))
        assert name == "scan" or "empties_only" in cut.rows
        lb, _ = F.lane_blocks(cut.off, first, cnt)
        for kind, row in cut.rows.items():
            assert row.w.dtype == np.uint8 and row.w.shape == (cut.n_blocks,)
            sub = resample.materialize(c.rec, cut.off, row.w)
            assert sub.shape[0] == row.records <= F.MAX_RECORDS, (name, kind)
            assert len(R.scan_lengths(sub, [0, sub.shape[0]])[0]) >= row.scans or row.records == 0   # (a repeated block: more scans)
            if row.degenerate:
                assert row.records == 0
            elif kind != "wave0_on":
                assert row.scans >= F.MIN_SCANS and row.pinned, (name, kind, row.scans)
        lane_w = {k: r.w[lb] for k, r in cut.rows.items()}
        assert lane_w["mult255"].max() == 255 and lane_w["mult255"].min() >= 2
        assert lane_w["bootstrap"].max() >= 2 and lane_w["rand01"].max() == 1 and lane_w["rand01"].min() == 0
        n0 = min(64, int(used.sum()))
        # every lane of wave 0 off, and beyond it only the rest of a block that straddles lanes 63 | 64
        assert not lane_w["wave0_dead"][:n0].any() and np.all(np.diff(lane_w["wave0_dead"][n0:].astype(int)) >= 0)
        assert lane_w["wave0_dead"][-1] == 1 and np.all(lb[n0:][lane_w["wave0_dead"][n0:] == 0] == lb[n0 - 1])
        assert not lane_w["wave0_on"][n0:].any() and lane_w["wave0_on"][:n0].any()
        assert np.array_equal(lane_w["wave0_on"] == 0, lane_w["wave0_off"] == 1)
        assert not cut.rows["empties_only"].w[~cut.empty].any() if "empties_only" in cut.rows else True
        if name == "lanecut":
            a = cut.rows["alt03"].w[cut.long_blocks]
            assert a.tolist() == [0 if i % 2 == 0 else 3 for i in range(a.size)]
            lw = lane_w["alt03"]
            assert np.any((lw[:-1] == 0) & (lw[1:] == 3) & (scan[used][:-1] == scan[used][1:]))   # 0 | 3 between two lanes of one scan
    assert c.use_loss == (c.index % 5 != 3)
    d = resample.local_delta(c.gt, c.x0)
    assert np.all((np.abs(d) >= 0.0099) & (np.abs(d) <= 0.0201)), d


def test_the_cases_cover_styles_and_options():
    cs = [F.case(f, t) for f, t in F.CASES]
    assert {c.style for c in cs} == set(F.STYLES)
    for form in F.FORMS:
        assert {c.style for c in cs if c.form == form and c.t > 1} >= {"short", "split"}
    n_plain = sum(not c.use_loss for c in cs)
    assert n_plain == 4 and len(cs) == 20       # about one case in five without the loss
    assert any(not c.cuts[n].rows["wave0_on"].pinned for c in cs for n in F.SOLVE_CUTS if n in c.cuts)
    assert F.past_capacity_lens(256).size >= 16
    for form in (512, "z"):
        assert not R.plan_lens([F.past_capacity_lens(form)], 0, form == "z").resident


def test_the_tiny_residual_problem_is_what_it_says(oracle_mod):
    rec, off, x, want = F.tiny_residual_problem()
    assert R.plan(rec, [0, rec.shape[0]]).path_info() == (1, 256, 1, 1, 0) and off.tolist() == list(range(33))
    r, _ = oracle_mod.factor_evaluate_batch(rec, np.ascontiguousarray(x), want_jac=False)
    assert np.abs(r / rec[:, 7] / want - 1.0).max() <= 1e-8 and np.abs(want).max() <= 4e-6
    arg = (r / rec[:, 7]) ** 2 / 0.05 ** 2
    assert np.abs(np.log(1.0 + arg) / np.log1p(arg) - 1.0).max() > 1e-8     # what rounding 1 + x costs here: beyond the score gate


def test_the_oracle_alone_stays_inside_the_near_tie_cap(oracle_mod):
    """near_tie of the oracle's solve with itself: any decision within TIE_REL of its threshold up to the iteration it stopped at."""
    jobs = []
    for form, t in F.CASES:
        c = F.case(form, t)
        for name in F.SOLVE_CUTS:
            if name in c.cuts:
                jobs += [(c, name, row) for row in c.cuts[name].rows.values() if not row.degenerate]

    def one(job):
        c, name, row = job
        oo = oracle_mod.default_options()
        oo.use_loss = int(c.use_loss)
        sub = resample.materialize(c.rec, c.cuts[name].off, row.w)
        ref = oracle_mod.solve(sub, c.x0, oo, linear_solver="qr")
        a = (ref.summary.termination, ref.summary.num_iterations)
        return NT.near_tie(oracle_mod, sub, c.x0, oo, a, a)

    with ThreadPoolExecutor(max_workers=min(16, oracle_mod.max_threads())) as ex:
        why = list(ex.map(one, jobs))
    per_case = {}
    for (c, name, row), w in zip(jobs, why):
        if w is not None:
            print(f"near tie in the oracle's own trace: {c.form} ppl {c.t} {name} {row.kind}: {w}")
            per_case[(c.form, c.t)] = per_case.get((c.form, c.t), 0) + 1
    ties = sum(per_case.values())
    print(f"seed {F.SEED}: {ties} of {len(jobs)} rows have a near tie in the oracle's own trace ({100.0 * ties / len(jobs):.2f} %; "
          f"cap {100 * EXCUSED_SHARE:.0f} % = {int(EXCUSED_SHARE * len(jobs))} rows, {EXCUSED_PER_CASE} per case)")
    assert ties <= EXCUSED_SHARE * len(jobs), (ties, len(jobs))
    assert all(v <= EXCUSED_PER_CASE for v in per_case.values()), per_case
