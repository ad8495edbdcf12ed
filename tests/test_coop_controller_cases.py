"""The cases of tests/coop_controller_cases.py against the oracle alone, without a GPU: every case takes the controller branch it was
built for — the oracle's termination, iteration count and S / r / i pattern are the ones the module records —, and no decision of the
oracle's own trace lies within lm_near_tie.TIE_REL of its threshold.  That second condition is what lets the GPU test
(tests/test_gpu_coop_controller.py) hold every form of the cooperative solve to the oracle's decisions record by record with no
near-tie exemption: a case that sits on a tie is replaced, not exempted.

The exact cases (every step invalid) are also held to the closed-form trace: nothing in it depends on the solver."""
import numpy as np
import pytest

import coop_controller_cases as K
import lm_near_tie as NT

VARIANTS = [(c.name, v) for c in K.CASES for v in ("plain",) + (("z",) if c.z_form else ()) + (("small",) if c.small else ())]


def _solve(oracle_mod, case, variant, linear_solver="qr"):
    rec = K.records(case, z_form=variant == "z", small=variant == "small")
    o = K.options(case, oracle_mod.default_options)
    return rec, o, oracle_mod.solve(rec, K.start(case), o, linear_solver=linear_solver)


def test_the_table_is_what_the_issue_lists():
    assert [c.name for c in K.CASES] == ["R1", "R1cap3", "R1cap6", "R2", "R3", "R4", "R5", "R6", "G9", "G0", "P", "RAD0", "J0", "R0S", "RMAX",
                                         "NAN", "A5", "A2", "A1", "Acap", "Arad", "Aok"]
    assert [c.name for c in K.CASES if c.z_form] == ["R1", "G9", "NAN", "A5"]
    assert [c.name for c in K.CASES if c.small] == ["A5", "A2", "Acap", "Arad"]
    assert [c.name for c in K.CASES if c.exact] == ["A5", "A2", "A1", "Acap", "Arad"]
    for c in K.CASES:
        assert len(c.pattern) == c.iterations + 1 and c.pattern[0] == "S", c.name
        assert c.exact == (c.data == "flat" and c.options.get("max_lm_diagonal") == 0.0), c.name
    kinds = "".join(c.pattern for c in K.CASES)
    assert "r" in kinds and "i" in kinds
    assert {c.termination for c in K.CASES} == {1, 2, 3, 4, 5, 6}


def test_the_record_sets_are_what_the_module_says():
    base, flat = K.base_records(), K.flat_records()
    assert base.shape == flat.shape == (K.N_RECORDS, 8) and K.flat_records(K.SMALL_SCANS).shape == (2000, 8)
    assert np.all(base[:, 6] == 0.0) and np.isfinite(base).all()
    # the flat set: n = (0, 0, 1) and p.z = 0 exactly, 24 scans of 500 records that share (n, d, scale)
    assert np.all(flat[:, 0] == 0.0) and np.all(flat[:, 1] == 0.0) and np.all(flat[:, 2] == 1.0) and np.all(flat[:, 6] == 0.0)
    assert np.all(flat[:, 7] == 1.0 / np.sqrt(500.0))
    d = flat[:, 3].reshape(K.N_SCANS, K.PTS)
    assert np.all(d == d[:, :1]) and len(set(d[:, 0])) == K.N_SCANS and np.abs(d + 0.25).max() < 0.05
    assert 0.5 <= flat[:, 4].min() and flat[:, 4].max() <= 4.0 and -2.0 <= flat[:, 5].min() and flat[:, 5].max() <= 2.0
    nan = K.records(K.BY_NAME["NAN"])
    assert np.isnan(nan[17, 4]) and np.isnan(nan).sum() == 1
    z = K.records(K.BY_NAME["A5"], z_form=True)
    assert z[7, 6] == 1e-3 and np.count_nonzero(z[:, 6]) == 1 and np.all(z[:, :2] == 0.0)


def test_the_flat_sets_translation_rows_are_exact_zeros(oracle_mod):
    """J_t = s n with n = (0, 0, 1): the t_x and t_y entries of g and H are zero in the oracle's sums too, at the start and at a pose
    away from it, with and without the loss, with and without the one point off the lidar plane."""
    c = K.BY_NAME["A5"]
    for z in (False, True):
        rec = K.records(c, z_form=z)
        for pose in (K.STARTS["X0"], K.STARTS["s2"]):
            for loss in (True, False):
                _, g, H = oracle_mod.evaluate_ne(rec, pose, with_loss=loss)
                assert g[0] == 0.0 and g[1] == 0.0 and np.all(H[:6] == 0.0) and np.all(H[6:11] == 0.0), (z, loss)
                assert H[11] > 0.0 and g[2] != 0.0     # (t_z is an ordinary row)


@pytest.mark.parametrize("name,variant", VARIANTS, ids=[f"{n}-{v}" for n, v in VARIANTS])
def test_the_oracle_takes_the_recorded_branch_and_sits_on_no_tie(oracle_mod, name, variant):
    case = K.BY_NAME[name]
    rec, o, ref = _solve(oracle_mod, case, variant)
    s = ref.summary
    n_rec = s.num_successful_steps + s.num_unsuccessful_steps    # records the solve wrote (NAN: none — it fails before iteration zero is recorded)
    got = K.pattern(ref.trace[:n_rec])
    print(f"{name} {variant}: termination {s.termination}, {s.num_iterations} iterations, {got!r}, cost {s.initial_cost!r} -> {s.final_cost!r}")
    want = "" if case.data == "nan" else case.pattern
    assert (s.termination, s.num_iterations, got) == (case.termination, case.iterations, want)
    assert [it.iteration for it in ref.trace[:n_rec]] == list(range(n_rec))
    assert got.count("S") == s.num_successful_steps and len(got) - got.count("S") == s.num_unsuccessful_steps
    key = (s.termination, s.num_iterations)
    assert NT.near_tie(oracle_mod, rec, K.start(case), o, key, key) is None
    if case.data == "nan":
        assert np.array_equal(ref.pose, K.start(case)) and not np.isfinite(s.initial_cost)
    # the normal-equation solve takes the same decisions: no case hangs on how the linear system is solved either
    ne = oracle_mod.solve(rec, K.start(case), o, linear_solver="ne")
    assert (ne.summary.termination, ne.summary.num_iterations) == key and K.decisions(ne.trace[:n_rec]) == K.decisions(ref.trace[:n_rec])


@pytest.mark.parametrize("name,variant", [(n, v) for n, v in VARIANTS if K.BY_NAME[n].exact], ids=lambda v: v)
def test_the_exact_cases_follow_the_closed_form_trace(oracle_mod, name, variant):
    """Every step invalid: radius 1e4 * 2**-(k (k + 1) / 2) after the k-th one, every record at the initial cost, x never moves."""
    case = K.BY_NAME[name]
    _, _, ref = _solve(oracle_mod, case, variant)
    want = K.exact_invalid_expectation(case)
    assert [w[3] for w in want[1:5]] == [5000.0, 1250.0, 156.25, 9.765625][:len(want) - 1]
    assert [(it.iteration, it.step_is_valid, it.step_is_successful, it.trust_region_radius) for it in ref.trace] == want
    for it in ref.trace:
        assert it.cost == ref.summary.initial_cost
        assert it.cost_change == 0.0 and it.step_norm == 0.0 and it.relative_decrease == 0.0
    assert np.array_equal(ref.pose, K.start(case)) and ref.summary.final_cost == ref.summary.initial_cost
