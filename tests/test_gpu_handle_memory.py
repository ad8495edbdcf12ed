"""One handle taken through growing and then shrinking inputs: single uploads (host-planned small path, device pipeline, cooperative
layout), stored scans, trace and partial-row capacity, batch sizes, multi-start counts and gather capacities.  Every buffer the handle
and its communicator own is grown in place or kept; each result must be bit-identical to the same call on a fresh handle."""
import numpy as np
import pytest

import camlasercalibratool_amd as clc
from camlasercalibratool_amd import simdata as sd
from camlasercalibratool_amd.solver import Comm

pytestmark = pytest.mark.gpu

X_TRUE = sd.pose7_from_T(sd.tlc_to_tcl(sd.GT_RLC, sd.GT_TLC))
X0 = sd.pose7_from_T(np.eye(4))


def _summary(s):
    return (s.termination, s.num_iterations, s.num_evaluations, s.initial_cost, s.final_cost)


def _single(s, rec, max_iterations=100, grid=0):
    s.set_launch(grid, -1)
    s.upload(rec)
    o = clc.default_options()
    o.max_num_iterations = max_iterations
    r = s.solve(X0, o, trace_cap=max_iterations + 1)
    cost, g, H = s.eval(X_TRUE)
    s.set_launch(0, -1)
    return [r.pose, _summary(r.summary), [(t.cost, t.step_norm) for t in r.trace], cost, g, H]


def _stored(s, obs):
    s.store_observations(obs)
    n = s.select_observations(True, False)
    r = s.solve(X0)
    return [n, r.pose, _summary(r.summary)]


def _batched(s, rec, off, x0):
    s.upload_batched(rec, off)
    poses, sms = s.solve_batched(x0)
    return [poses, [_summary(m) for m in sms]]


def _multistart(s, rec, starts):
    s.upload_batched(rec, np.array([0, rec.shape[0]], dtype=np.int64))
    poses, sms = s.solve_multistart(starts)
    return [poses, [_summary(m) for m in sms]]


def _gather(s, rec, off, x0, lo, cap):
    s.upload_batched(rec, off)
    s.solve_batched(x0)
    c = Comm(s, None, 1, 3)  # (hooks build: a layout-only communicator, rank 1 of 3)
    try:
        two = c.gather_results(lo, cap)
        one, st = c.solve_gather(x0, lo, cap)
        return [two, one, (st.problems, st.evaluations, st.fused)]
    finally:
        c.close()


def _same(a, b, what):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y), what
        else:
            assert x == y, what


def test_one_handle_grown_and_shrunk_matches_fresh_handles():
    small = clc.flatten_observations(sd.sim_fixed_count(1, 20, 50, noise_sigma=0.01), False)      # host-planned, one workgroup
    mid = clc.flatten_observations(sd.sim_fixed_count(2, 60, 500, noise_sigma=0.01), False)       # cooperative layout
    big = clc.flatten_observations(sd.sim_fixed_count(3, 200, 1500, noise_sigma=0.01), False)     # rows, many tiles
    obs_small, obs_big = sd.sim_fixed_count(4, 30, 100, noise_sigma=0.01), sd.sim_fixed_count(5, 80, 400, noise_sigma=0.01)
    batches = {P: sd.sim_shard_records(6, 0, P, 7, 80, 0.01) for P in (5, 300)}
    rec1 = clc.flatten_observations(sd.sim_fixed_count(7, 20, 300, noise_sigma=0.01), False)
    s_all = np.tile(X_TRUE, (96, 1))
    s_all[:, :3] += np.random.default_rng(5).normal(size=(96, 3)) * 0.05  # (translations moved up to ~15 cm)
    steps = [
        ("single small", lambda s: _single(s, small)),
        ("single big, long trace, wide grid", lambda s: _single(s, big, max_iterations=300, grid=600)),
        ("single mid", lambda s: _single(s, mid)),
        ("single small again", lambda s: _single(s, small)),
        ("stored small", lambda s: _stored(s, obs_small)),
        ("stored big", lambda s: _stored(s, obs_big)),
        ("stored small again", lambda s: _stored(s, obs_small)),
        ("batch 5", lambda s: _batched(s, batches[5][0], batches[5][1], batches[5][2])),
        ("batch 300", lambda s: _batched(s, batches[300][0], batches[300][1], batches[300][2])),
        ("batch 5 again", lambda s: _batched(s, batches[5][0], batches[5][1], batches[5][2])),
        ("multistart 8", lambda s: _multistart(s, rec1, s_all[:8])),
        ("multistart 96", lambda s: _multistart(s, rec1, s_all)),
        ("multistart 8 again", lambda s: _multistart(s, rec1, s_all[:8])),
        ("gather cap 5", lambda s: _gather(s, batches[5][0], batches[5][1], batches[5][2], 5, 5)),
        ("gather cap 400", lambda s: _gather(s, batches[300][0], batches[300][1], batches[300][2], 400, 400)),
        ("gather cap 7", lambda s: _gather(s, batches[5][0], batches[5][1], batches[5][2], 7, 7)),
    ]
    with clc.Solver(0, library="hooks") as one:
        for what, step in steps:
            got = step(one)
            with clc.Solver(0, library="hooks") as fresh:
                _same(got, step(fresh), what)
