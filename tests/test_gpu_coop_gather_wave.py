"""GPU tests of the cooperative solve's workgroup shape (csrc/clc_coop.hpp): four point waves, the controller wave, and — on the 8 group
leaders of the 256-workgroup form — a sixth wave that gathers the group's 32 rows and publishes the group row, so that every
controller wave is a follower.  The arithmetic and its order are those of the five-wave kernel: tests/golden/
coop_gather_wave_parent.json holds that build's bits (scripts/coop_golden_bits.py, which also defines the inputs), and every case is
held to them bit for bit, besides the usual gates against the oracle and the step chain.

The shapes are the smallest at which each form runs: the two-hop form begins above 32 x 256 x 13 = 106 496 observations."""
import importlib.util
import json
import os

import numpy as np
import pytest

import camlasercalibratool_amd as clc
from camlasercalibratool_amd import simdata as sd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X0 = sd.pose7_from_T(np.eye(4))
T_TOL = 1e-6
COST_TOL = 1e-8
STEP_CHAIN = 2 | 16 | 32 | 128 | 256 | 512   # the explicit default flag set: clc_solve as the step chain


def _golden_module():
    spec = importlib.util.spec_from_file_location("coop_golden_bits", os.path.join(ROOT, "scripts", "coop_golden_bits.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def gb():
    return _golden_module()


@pytest.fixture(scope="module")
def inputs(gb):
    return gb.cases()


@pytest.fixture(scope="module")
def golden(gb):
    with open(gb.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def sv():
    s = clc.Solver(0)
    yield s
    s.close()


def _dT(a, b):
    return np.abs(sd.T_from_pose7(a) - sd.T_from_pose7(b)).max()


def _key(s):
    return (s.termination, s.num_iterations, s.num_evaluations, s.num_successful_steps, s.num_unsuccessful_steps)


def _check_case(name, sv, oracle_mod, gb, inputs, golden):
    """Ran on the expected workgroups with no new abort; oracle: termination, iterations, T_cl, cost; step chain: key, pose, trace
    length; the five-wave build's bits."""
    rec, wgs, z = inputs[name]
    sv.debug_coop_control(reenable=True)
    sv.set_launch(0, -1)
    sv.set_auto_paths(0)
    sv.upload(rec)
    pi = sv.path_info()
    assert pi.coop_resident == 1 and pi.coop_workgroups == wgs and pi.coop_points_carry_z == z, name
    n0, t0 = pi.coop_solves, pi.coop_timeouts
    r = sv.solve(X0)
    pi = sv.path_info()
    assert pi.coop_solves == n0 + 1 and pi.coop_timeouts == t0 and not pi.coop_resting, name
    ref = oracle_mod.solve(rec, X0, linear_solver="qr")
    assert r.summary.termination == ref.summary.termination and r.summary.num_iterations == ref.summary.num_iterations, name
    dT, dc = _dT(r.pose, ref.pose), abs(r.summary.final_cost - ref.summary.final_cost)
    print(f"{name}: n = {rec.shape[0]}, {pi.coop_points_per_lane} points per lane, |dT| {dT:.2e}, |dcost| {dc:.2e} against the oracle")
    assert dT <= T_TOL and dc <= COST_TOL, name
    sv.set_launch(0, STEP_CHAIN)
    r2 = sv.solve(X0)
    sv.set_launch(0, -1)
    assert sv.path_info().coop_solves == n0 + 1, name  # explicit flags: the step chain
    assert _key(r.summary) == _key(r2.summary), name
    assert np.abs(r.pose - r2.pose).max() <= 1e-9, name
    assert len(r.trace) == len(r2.trace) == r.summary.num_iterations + 1, name
    g = golden["cases"][name]
    assert g["observations"] == rec.shape[0] and g["workgroups"] == wgs, name
    assert gb.bits(r) == {k: g[k] for k in ("pose", "final_cost", "key")}, name
    return r


def test_two_hop_form_at_its_smallest(sv, oracle_mod, gb, inputs, golden):
    """107 000 observations, 2 points per lane: 256 workgroups, 8 gather waves."""
    _check_case("two_hop_smallest", sv, oracle_mod, gb, inputs, golden)
    assert sv.path_info().coop_points_per_lane == 2


@pytest.mark.parametrize("kw", [dict(max_num_iterations=0), dict(max_num_iterations=1), dict(max_num_iterations=2), dict(use_loss=0),
                                dict(function_tolerance=1e-12)], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_every_way_out_of_the_pass_loop(sv, oracle_mod, inputs, kw):
    """The sixth wave leaves with the others: at pass 0, at pass 1, at a late pass, without the loss, at a tighter tolerance.  Each such
    solve is followed by a default solve; the default solves are bit-equal to the one before, and nothing timed out."""
    rec, wgs, _ = inputs["two_hop_smallest"]
    sv.debug_coop_control(reenable=True)
    sv.set_launch(0, -1)
    sv.set_auto_paths(0)
    sv.upload(rec)
    assert sv.path_info().coop_workgroups == wgs
    first = sv.solve(X0)
    pi = sv.path_info()
    n0, t0 = pi.coop_solves, pi.coop_timeouts
    o, oo = clc.default_options(), oracle_mod.default_options()
    for k, v in kw.items():
        setattr(o, k, v)
        setattr(oo, k, v)
    r = sv.solve(X0, o)
    ref = oracle_mod.solve(rec, X0, options=oo, linear_solver="qr")
    assert r.summary.termination == ref.summary.termination and r.summary.num_iterations == ref.summary.num_iterations, kw
    assert _dT(r.pose, ref.pose) <= T_TOL and abs(r.summary.final_cost - ref.summary.final_cost) <= COST_TOL, kw
    if "max_num_iterations" in kw:
        assert r.summary.num_iterations == kw["max_num_iterations"]
    after = sv.solve(X0)
    assert np.array_equal(after.pose, first.pose) and after.summary.final_cost == first.summary.final_cost and _key(after.summary) == _key(first.summary), kw
    pi = sv.path_info()
    assert pi.coop_solves == n0 + 2 and pi.coop_timeouts == t0 and not pi.coop_resting, kw


def test_z_form(sv, oracle_mod, gb, inputs, golden):
    """The same records with one point off the lidar plane: the 24-byte-slot form of the kernel."""
    _check_case("z_form", sv, oracle_mod, gb, inputs, golden)


def test_ragged_scans(sv, oracle_mod, gb, inputs, golden):
    """Scans of 0..180 points: chunks cut scans, lanes are short, padding is masked."""
    _check_case("ragged_scans", sv, oracle_mod, gb, inputs, golden)


def test_block_boundary(sv, oracle_mod, gb, inputs, golden):
    """530 000 observations: 9 points per lane, a second block of 8 with masked padding."""
    _check_case("block_boundary", sv, oracle_mod, gb, inputs, golden)
    assert sv.path_info().coop_points_per_lane == 9


def test_one_hop_form_is_untouched(sv, oracle_mod, gb, inputs, golden):
    """24 000 observations on 32 workgroups: no gather wave there; the same bits as before."""
    _check_case("one_hop", sv, oracle_mod, gb, inputs, golden)


def test_golden_file_covers_the_cases_and_names_its_build(gb, inputs, golden):
    assert sorted(golden["cases"]) == sorted(inputs) == ["block_boundary", "one_hop", "ragged_scans", "two_hop_smallest", "z_form"]
    assert golden["recorded_on_commit"] and len(golden["recorded_on_commit"]) >= 7
