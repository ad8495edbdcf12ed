"""GPU tests of the LM controller's rare branches INSIDE the cooperative solve (csrc/clc_coop.hpp, csrc/clc_lmuni.hpp): rejected steps
(lmu_post's `success == false`: the totals buffers do not swap, the system at x is read again), invalid steps (lmu_pre's
LMU_INVALID_STEP: the pass under way is thrown away uncounted, the radius shrinks, the step is computed again), the deferred gradient
stop (LMU_STOP_GRADIENT: one discarded pass after the iteration that met the tolerance), the parameter and radius stops, the
iteration cap on a rejected step and a non-finite first evaluation.  The controller runs redundantly on the fifth wave of every
workgroup, and every one of these is a way out of the pass loop that the four point waves, the controller wave and the gather wave of
all 32 or 256 workgroups must take together: a workgroup that decided differently would time the launch out, and the step chain
would still answer correctly — so every case asserts that it ran on chip and that nothing timed out.

The cases, their oracle outcomes and the absence of near ties in them: tests/coop_controller_cases.py, checked on the CPU by
tests/test_coop_controller_cases.py.  Each runs on the one-hop form (32 workgroups) and the two-hop form (256 workgroups,
clc_set_auto_paths(8) at upload); R1, G9, NAN and A5 also in the 24-byte-slot form.  Held to
  * the oracle (DENSE_QR) on the same records and options: termination, counts, (iteration, valid, successful) record by record —
    no near-tie exemption —, pose within T_TOL, final cost within COST_TOL (x the cost where it is above 1), initial cost to 1e-11;
  * the step chain on the GPU: the summary key with num_evaluations (where the discarded passes show that they are not counted) and
    the trace record by record;
  * the number of evaluations the decisions imply: the first pass, one per valid step recorded, one for the pass a parameter or
    function stop ends on — a discarded pass is none;
  * for the exact cases (every step invalid by construction) the closed-form trace, bit for bit;
  * itself: a second solve gives the same bits, and a default solve after it the bits of the default solve before it.
A5, A2, Acap and Arad also run at 2 000 records on the single-workgroup kernel and the step chain, to the same exact expectations.

Measured on MI355X (worst over the cases of a form, against the oracle; `python -m pytest -s` prints them per case).  Every case took
the oracle's decisions record by record in every form; the gates are T_TOL = 1e-6 and COST_TOL = 1e-8:
  form      |dT|               |dcost|             initial cost, rel   trace cost, rel    trust-region radius, rel
  one-hop   1.25e-10 (Aok)     2.89e-13 (R1cap3)   1.8e-14 (Aok)       1.4e-13 (R1)       1.7e-15 (R0S)
  two-hop   3.36e-11 (Aok)     2.79e-13 (R1cap3)   1.8e-14 (Aok)       1.0e-13 (RMAX)     1.7e-15 (R0S)
  z slots   6.66e-16 (R1)      1.79e-15 (A5)       1.8e-14 (A5)        2.0e-13 (R1)       0
  (R1cap3 stops at a cost of 6.73: 4.3e-14 relative; no final cost differs by more than 3e-13, so the absolute gate holds as well.)
  The exact cases on the single-workgroup kernel and the step chain at 2 000 records: pose and radii bit-equal, initial cost 3.9e-15.
One finding when the file first ran: NAN returned num_iterations = -1 on every clc_solve path (the kernels' summary epilogue says
"recorded iterations - 1" and a solve that fails in iteration zero records none) where the oracle counts 0; clc_solve now reports 0
(csrc/abi_solve.hip, finish_solve).  Nothing timed out, and no controller branch differed from the oracle or the step chain."""
import numpy as np
import pytest

import camlasercalibratool_amd as clc
import coop_controller_cases as K
from camlasercalibratool_amd import simdata as sd

pytestmark = pytest.mark.gpu

X0 = K.STARTS["X0"]
T_TOL = 1e-6          # tests/test_gpu_coop.py
COST_TOL = 1e-8
STEP_CHAIN = 2 | 16 | 32 | 128 | 256 | 512   # the explicit default flag set: clc_solve as the step chain
PARAMETER, FUNCTION = 2, 3
FORMS = {"one_hop": (32, 0, 0), "two_hop": (256, 0, 8), "z": (32, 1, 0)}     # workgroups, points carry z, clc_set_auto_paths at upload
RUNS = [(c.name, f) for c in K.CASES for f in ("one_hop", "two_hop") + (("z",) if c.z_form else ())]
_FLOATS = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius")


@pytest.fixture(scope="module")
def sv():
    s = clc.Solver(0)
    yield s
    s.set_auto_paths(0)
    s.set_launch(0, -1)
    s.close()


@pytest.fixture(scope="module")
def refs(oracle_mod):
    """(case name, z form) -> the oracle's solve, computed once."""
    cache = {}

    def get(case, z=False, small=False):
        k = (case.name, z, small)
        if k not in cache:
            cache[k] = oracle_mod.solve(K.records(case, z_form=z, small=small), K.start(case), K.options(case, oracle_mod.default_options), linear_solver="qr")
        return cache[k]

    return get


def _dT(a, b):
    return np.abs(sd.T_from_pose7(a) - sd.T_from_pose7(b)).max()


def _key(s):
    return (s.termination, s.num_iterations, s.num_evaluations, s.num_successful_steps, s.num_unsuccessful_steps)


def _n_records(s):
    return s.num_successful_steps + s.num_unsuccessful_steps     # (a solve that fails before iteration zero is recorded: none)


def _bits(r):
    s = r.summary
    n = _n_records(s)
    return (r.pose.tobytes(), _key(s), np.array([s.initial_cost, s.final_cost]).tobytes(),
            [(t.iteration, t.step_is_valid, t.step_is_successful, np.array([getattr(t, f) for f in _FLOATS]).tobytes()) for t in r.trace[:n]])


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0.0 else abs(a)


def _check_decisions(case, r, what):
    """What the case was built for (= the oracle's outcome, tests/test_coop_controller_cases.py), and the evaluations it implies."""
    s = r.summary
    n = _n_records(s)
    want = "" if case.data == "nan" else case.pattern
    assert (s.termination, s.num_iterations, K.pattern(r.trace[:n])) == (case.termination, case.iterations, want), what
    assert [t.iteration for t in r.trace[:n]] == list(range(n)), what
    evals = 1 + sum(1 for t in r.trace[1:n] if t.step_is_valid) + (1 if s.termination in (PARAMETER, FUNCTION) else 0)
    assert s.num_evaluations == evals, (what, s.num_evaluations, evals)


def _check_against_oracle(case, r, ref, what):
    s, q = r.summary, ref.summary
    assert (s.termination, s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps) == \
           (q.termination, q.num_iterations, q.num_successful_steps, q.num_unsuccessful_steps), what
    n = _n_records(q)
    assert K.decisions(r.trace[:n]) == K.decisions(ref.trace[:n]), what
    if case.data == "nan":      # no finite cost anywhere to compare: FAILURE, and the start point's bits returned
        assert r.pose.tobytes() == K.start(case).tobytes() == ref.pose.tobytes(), what
        print(f"{what}: termination {s.termination}, {s.num_iterations} iterations, no record, {s.num_evaluations} evaluation; the pose is the start's bits")
        return
    dT, dc, di = _dT(r.pose, ref.pose), abs(s.final_cost - q.final_cost), _rel(s.initial_cost, q.initial_cost)
    worst_cost = max([_rel(a.cost, b.cost) for a, b in zip(r.trace[:n], ref.trace[:n])])
    worst_radius = max([_rel(a.trust_region_radius, b.trust_region_radius) for a, b in zip(r.trace[:n], ref.trace[:n])])
    print(f"{what}: termination {s.termination}, {s.num_iterations} iterations, {K.pattern(r.trace[:n])}, {s.num_evaluations} evaluations; against the "
          f"oracle |dT| {dT:.2e}, |dcost| {dc:.2e} (cost {q.final_cost:.3g}), initial cost rel {di:.1e}, trace cost rel {worst_cost:.1e}, radius rel {worst_radius:.1e}")
    assert dT <= T_TOL, (what, dT)
    assert dc <= COST_TOL * max(1.0, abs(q.final_cost)), (what, dc)
    assert di <= 1e-11, (what, di)


def _check_against_step_chain(r, r2, what):
    """The tolerances of test_cooperative_solve_is_the_default_and_matches_oracle_and_step_chain (tests/test_gpu_coop.py)."""
    assert _key(r.summary) == _key(r2.summary), what
    n = _n_records(r.summary)
    if not np.isfinite(r2.summary.final_cost):
        assert np.array_equal(r.pose, r2.pose) and not np.isfinite(r.summary.final_cost), what
    else:
        assert np.abs(r.pose - r2.pose).max() <= 1e-9 and abs(r.summary.final_cost - r2.summary.final_cost) <= 1e-11 * abs(r2.summary.final_cost), what
    assert len(r.trace) == len(r2.trace) == max(0, r.summary.num_iterations + 1), what
    assert K.decisions(r.trace[:n]) == K.decisions(r2.trace[:n]), what
    for a, b in zip(r.trace[:n], r2.trace[:n]):
        assert abs(a.cost - b.cost) <= 1e-10 * abs(b.cost), what
        assert abs(a.trust_region_radius - b.trust_region_radius) <= 1e-9 * abs(b.trust_region_radius), what


def _check_exact(case, r, what):
    """Every step invalid: nothing here depends on a sum's order, so it holds bit for bit on every path."""
    want = K.exact_invalid_expectation(case)
    assert [(t.iteration, t.step_is_valid, t.step_is_successful) for t in r.trace] == [w[:3] for w in want], what
    assert [t.trust_region_radius for t in r.trace] == [w[3] for w in want], what
    s = r.summary
    for t in r.trace:
        assert t.cost == s.initial_cost and t.cost_change == 0.0 and t.step_norm == 0.0 and t.relative_decrease == 0.0, what
    assert r.pose.tobytes() == K.start(case).tobytes() and s.final_cost == s.initial_cost, what
    assert s.num_evaluations == 1 and s.num_successful_steps == 1 and s.num_unsuccessful_steps == len(want) - 1, what


@pytest.mark.parametrize("name,form", RUNS, ids=[f"{n}-{f}" for n, f in RUNS])
def test_controller_branch_in_the_cooperative_solve(sv, refs, name, form):
    case = K.BY_NAME[name]
    wgs, z, auto = FORMS[form]
    what = f"{name} {form}"
    rec = K.records(case, z_form=form == "z")
    o = K.options(case, clc.default_options)
    x = K.start(case)
    try:
        sv.debug_coop_control(reenable=True)
        sv.set_launch(0, -1)
        sv.set_auto_paths(auto)   # (takes effect at upload)
        sv.upload(rec)
        pi = sv.path_info()
        assert pi.coop_resident == 1 and pi.coop_workgroups == wgs and pi.coop_points_carry_z == z and not pi.coop_resting, what
        before = sv.solve(X0)
        pi = sv.path_info()
        n0, t0 = pi.coop_solves, pi.coop_timeouts
        r = sv.solve(x, o)
        pi = sv.path_info()
        assert pi.coop_solves == n0 + 1 and pi.coop_timeouts == t0 and not pi.coop_resting, what      # it ran on chip, nothing timed out
        again = sv.solve(x, o)
        after = sv.solve(X0)
        pi = sv.path_info()
        assert pi.coop_solves == n0 + 3 and pi.coop_timeouts == t0 and not pi.coop_resting, what
        assert pi.coop_workgroups == wgs and pi.coop_points_carry_z == z, what
        sv.set_launch(0, STEP_CHAIN)
        chain = sv.solve(x, o)
        assert sv.path_info().coop_solves == n0 + 3, what   # explicit flags: the step chain
    finally:
        sv.set_launch(0, -1)
        sv.set_auto_paths(0)
    _check_decisions(case, r, what)
    _check_decisions(case, chain, what + " (step chain)")
    _check_against_oracle(case, r, refs(case, z=form == "z"), what)
    _check_against_step_chain(r, chain, what)
    if case.exact:
        _check_exact(case, r, what)
        _check_exact(case, chain, what + " (step chain)")
    assert _bits(again) == _bits(r), what             # repeatable
    assert _bits(after) == _bits(before), what        # the exit left boards and tags fit for the next solve


SMALL = [c.name for c in K.CASES if c.small]


@pytest.mark.parametrize("name", SMALL)
def test_exact_invalid_steps_on_the_single_workgroup_kernel_and_the_step_chain(sv, refs, name):
    """2 000 records of the flat set: what one workgroup holds.  The invalid-step path of the single-workgroup kernel and of the step
    chain against the closed-form trace and the oracle, not against another GPU controller."""
    case = K.BY_NAME[name]
    rec = K.records(case, small=True)
    o = K.options(case, clc.default_options)
    x = K.start(case)
    try:
        sv.set_launch(0, -1)
        sv.set_auto_paths(0)
        sv.upload(rec)
        pi = sv.path_info()
        assert pi.single_resident == 1 and pi.coop_resident == 0, name
        n0 = pi.coop_solves
        single = sv.solve(x, o)
        single2 = sv.solve(x, o)
        sv.set_launch(0, STEP_CHAIN)
        chain = sv.solve(x, o)
        assert sv.path_info().coop_solves == n0, name
    finally:
        sv.set_launch(0, -1)
    ref = refs(case, small=True)
    for r, what in ((single, name + " single workgroup"), (chain, name + " step chain")):
        _check_decisions(case, r, what)
        _check_exact(case, r, what)
        _check_against_oracle(case, r, ref, what)
    _check_against_step_chain(single, chain, name)
    assert _bits(single2) == _bits(single), name
