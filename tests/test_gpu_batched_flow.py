"""clc_closed_form_batched / clc_information_batched (csrc/clc_batchflow.hpp, K8 / K9) and calib.CamLaserCalibrationBatch: every
problem of a batch against the oracle (oracle.closed_form / oracle.information) and against the single-problem calls on that
problem alone, with the gates of tests/test_gpu_parity.py:
  Tlc 1e-9, sv9 rtol 1e-9 (unobservable: 1e-9 x the largest), `unobservable` equal, start pose = pose7_from_T(inv(Tlc)) to 1e-12,
  H rtol 1e-11, b and sv rtol 1e-9, chi2 1e-11 relative, n_null equal.
On unobservable problems Tlc is only required to be finite and to match the single-handle clc_closed_form (a near-singular system
amplifies rounding; the oracle is the same host restatement)."""
import numpy as np
import pytest

import camlasercalibratool_amd as clc
import lm_near_tie as NT
from camlasercalibratool_amd import _build, simdata as sd

pytestmark = pytest.mark.gpu

CLC_ERR_NO_DATA = -5


@pytest.fixture(scope="module")
def sv():
    s = clc.Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def single():
    s = clc.Solver(0)
    yield s
    s.close()


def _upload(sv, recs):
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([r.shape[0] for r in recs])
    sv.upload_batched(np.concatenate(recs) if off[-1] else np.zeros((0, 8)), off)


def _pose_ref(T):
    return sd.pose7_from_T(np.linalg.inv(T))


def _check_closed_form(sv, single, oracle_mod, recs, oracle_for=None):
    """Closed form of every problem of the uploaded batch against the oracle and the single-handle call."""
    P = len(recs)
    poses_in = np.full((P, 7), 7.0)
    T, un, sv9, st, poses = sv.closed_form_batched(poses_in.copy())
    for k, rec in enumerate(recs):
        if rec.shape[0] == 0:
            assert st[k] == CLC_ERR_NO_DATA and np.all(poses[k] == 7.0), k
            continue
        assert st[k] == 0, (k, st[k])
        single.upload(rec)
        T1, un1, s91 = single.closed_form()
        T0, un0, s90 = oracle_mod.closed_form(rec if oracle_for is None else oracle_for[k])
        assert bool(un[k]) == un0 == un1, k
        assert np.isfinite(T[k]).all()
        if un0:
            assert np.abs(sv9[k] - s90).max() <= 1e-9 * s90[0], k
            assert np.abs(T[k] - T1).max() < 1e-6 or np.abs(T1).max() > 1e6, (k, T[k], T1)
        else:
            assert np.allclose(sv9[k], s90, rtol=1e-9), k
            assert np.abs(T[k] - T0).max() < 1e-9 and np.abs(T[k] - T1).max() < 1e-9, k
        assert np.abs(poses[k] - _pose_ref(T[k])).max() <= 1e-12, k
    return T, un, sv9, st, poses


def _check_information(sv, single, oracle_mod, recs, poses):
    H, b, chi2, s6, V, nn = sv.information_batched(poses)
    for k, rec in enumerate(recs):
        if rec.shape[0] == 0:
            assert chi2[k] == 0.0 and np.all(H[k] == 0.0) and nn[k] == 6, k
            continue
        H0, b0, c0, s60, V0, nn0 = oracle_mod.information(rec, poses[k])
        assert np.allclose(H[k], H0, rtol=1e-11), k
        assert np.allclose(b[k], b0, rtol=1e-9, atol=1e-14), k
        assert abs(chi2[k] - c0) <= 1e-11 * c0 + 1e-26, k  # (+ a floor: a noise-free problem's chi2 at its exact pose is rounding)
        assert np.allclose(s6[k], s60, rtol=1e-9, atol=1e-9 * s60[0]) and nn[k] == nn0, k
        # V: an eigenvector basis of H (columns up to sign where the eigenvalues are apart)
        assert np.abs(H0 @ V[k] - V[k] * s6[k]).max() <= 1e-9 * s60[0], k
        single.upload(rec)
        H1, b1, c1, s61, V1, nn1 = single.information(poses[k])
        assert np.allclose(H[k], H1, rtol=1e-11) and abs(chi2[k] - c1) <= 1e-11 * c1 + 1e-26 and nn[k] == nn1, k
    return H, b, chi2, s6, V, nn


def test_noisy_batch_of_64(sv, single, oracle_mod):
    probs, _ = sd.sim_batch(606, 64, 20, 200, 0.01)
    recs = [clc.flatten_observations(S, True, False) for S in probs]
    _upload(sv, recs)
    T, un, sv9, st, poses = _check_closed_form(sv, single, oracle_mod, recs)
    assert not un.any() and (st == 0).all()
    _check_information(sv, single, oracle_mod, recs, poses)


def test_mixed_batch_degenerate_empty_one_record_and_z(sv, single, oracle_mod):
    probs, _ = sd.sim_batch(707, 6, 12, 80, 0.01)
    base = [clc.flatten_observations(S, True, False) for S in probs]
    deg = [clc.flatten_observations(sd.sim_degenerate(kind), True, False) for kind in ("parallel_boards", "only_pitch")]
    one = base[0][:1].copy()
    zrec = base[1].copy()
    zrec[:, 6] = np.random.default_rng(3).normal(size=len(zrec)) * 0.05  # points off the lidar plane: the closed form ignores z
    recs = [base[2], deg[0], base[3], np.zeros((0, 8)), deg[1], one, zrec, base[4]]
    _upload(sv, recs)
    zero_z = zrec.copy(); zero_z[:, 6] = 0.0
    oracle_for = [r if i != 6 else zero_z for i, r in enumerate(recs)]
    T, un, sv9, st, poses = _check_closed_form(sv, single, oracle_mod, recs, oracle_for)
    assert un[1] and un[4] and un[5] and not un[0] and not un[2] and not un[7]
    # z: the same answer as with z zeroed
    single.upload(zero_z)
    Tz, _, _ = single.closed_form()
    assert np.abs(T[6] - Tz).max() < 1e-9
    # neighbours of the degenerate problems are unaffected: the same as in a batch of their own (to rounding: a batch of another
    # size splits its problems over another number of workgroups)
    _upload(sv, [base[2], base[3], base[4]])
    T2, un2, sv92, st2, p2 = sv.closed_form_batched()
    for a, b in ((0, 0), (2, 1), (7, 2)):
        assert np.abs(T[a] - T2[b]).max() < 1e-12 and np.allclose(sv9[a], sv92[b], rtol=1e-12) and st2[b] == 0, (a, b)
    _upload(sv, recs)
    good = np.where(st == 0, True, False)
    info_poses = np.where(good[:, None], poses, sd.pose7_from_T(np.eye(4))[None, :])
    H, b, chi2, s6, V, nn = _check_information(sv, single, oracle_mod, recs, info_poses)
    assert nn[1] > 0 and nn[3] == 6


def test_sparse_rows_read_the_tiles(sv, single, oracle_mod):
    """One point per scan: rows of 64 lanes would carry one point each, the upload keeps no row layout and K8 / K9 read the
    64-byte tiles."""
    recs = []
    for k in range(5):
        probs, _ = sd.sim_batch(900 + k, 1, 300, 1, 0.01)
        recs.append(clc.flatten_observations(probs[0], True, False))
    _upload(sv, recs)
    assert not sv.debug_rows()[2]  # batched_rows_layout
    T, un, sv9, st, poses = _check_closed_form(sv, single, oracle_mod, recs)
    _check_information(sv, single, oracle_mod, recs, np.where((st == 0)[:, None], poses, sd.pose7_from_T(np.eye(4))[None, :]))


def test_one_problem_of_a_million_observations(sv, single, oracle_mod):
    probs, _ = sd.sim_batch(4711, 1, 1000, 1000, 0.01)
    rec = clc.flatten_observations(probs[0], True, False)
    assert rec.shape[0] == 10**6
    _upload(sv, [rec])
    T, un, sv9, st, poses = _check_closed_form(sv, single, oracle_mod, [rec])
    _check_information(sv, single, oracle_mod, [rec], poses)


def test_full_flow_against_the_oracle(oracle_mod):
    probs, _ = sd.sim_batch(808, 24, 20, 150, 0.01)
    out = clc.CamLaserCalibrationBatch(probs)
    o_opts = oracle_mod.default_options()
    flips = 0
    for k, S in enumerate(probs):
        rec = oracle_mod.flatten(S, True, False)
        T0, un0, _ = oracle_mod.closed_form(rec)
        assert not out["unobservable"][k] and out["closed_form_status"][k] == 0
        assert np.abs(out["Tlc_initial"][k] - T0).max() < 1e-9
        x0 = _pose_ref(T0)
        ref = oracle_mod.solve(rec, x0)
        got = (int(out["termination"][k]), int(out["num_iterations"][k]), float(out["final_cost"][k]))
        want = (ref.summary.termination, ref.summary.num_iterations, ref.summary.final_cost)
        flips += NT.check_flip(oracle_mod, rec, x0, o_opts, got, want, f"problem {k}")
        assert np.abs(out["Tcl"][k] - sd.T_from_pose7(ref.pose)).max() < 1e-6, k
        assert abs(out["final_cost"][k] - ref.summary.final_cost) <= 1e-8 * max(ref.summary.final_cost, 1e-300) + 1e-300, k
        H0, b0, c0, s60, V0, nn0 = oracle_mod.information(rec, out["poses"][k])
        assert np.allclose(out["H"][k], H0, rtol=1e-11) and abs(out["chi2"][k] - c0) <= 1e-11 * c0 and out["n_null"][k] == nn0
    assert flips <= 2


def test_flow_with_board_edge_terms_uploads_per_step(oracle_mod):
    probs, _ = sd.sim_batch(909, 4, 20, 150, 0.01)
    out = clc.CamLaserCalibrationBatch(probs, use_boundary_constraint=True)
    for k, S in enumerate(probs):
        T0, _, _ = oracle_mod.closed_form(oracle_mod.flatten(S, True, False))
        assert np.abs(out["Tlc_initial"][k] - T0).max() < 1e-9
        rec_i = oracle_mod.flatten(S, True, False)
        H0, _, c0, _, _, _ = oracle_mod.information(rec_i, out["poses"][k])
        assert np.allclose(out["H"][k], H0, rtol=1e-11) and abs(out["chi2"][k] - c0) <= 1e-11 * c0


def test_two_calls_are_bitwise_equal(sv):
    probs, _ = sd.sim_batch(1001, 40, 20, 200, 0.01)
    recs = [clc.flatten_observations(S, True, False) for S in probs]
    _upload(sv, recs)
    a = sv.closed_form_batched()
    b = sv.closed_form_batched()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    i1 = sv.information_batched(a[4])
    i2 = sv.information_batched(a[4])
    for x, y in zip(i1, i2):
        assert np.array_equal(x, y)


def test_in_place_on_the_handle_buffers(sv):
    probs, _ = sd.sim_batch(1102, 16, 20, 200, 0.01)
    recs = [clc.flatten_observations(S, True, False) for S in probs]
    _upload(sv, recs)
    T, un, sv9, st, p_copy = sv.closed_form_batched()
    poses, _ = sv.batched_buffers()
    poses[...] = 0.0
    sv.closed_form_batched(poses)
    assert np.array_equal(poses, p_copy)
    res, sms = sv.solve_batched_inplace()
    H1 = sv.information_batched(poses)[0]
    H2 = sv.information_batched(np.array(poses))[0]
    assert np.array_equal(H1, H2)


def test_product_library_matches_the_hooks_build():
    probs, _ = sd.sim_batch(1203, 32, 20, 200, 0.01)
    recs = [clc.flatten_observations(S, True, False) for S in probs]
    prod = clc.Solver(0, library=_build.PRODUCT_LIB_PATH)
    hooks = clc.Solver(0, library="hooks")
    try:
        outs = []
        for s in (prod, hooks):
            _upload(s, recs)
            cf = s.closed_form_batched()
            outs.append((cf, s.information_batched(cf[4])))
        for x, y in zip(outs[0][0] + outs[0][1], outs[1][0] + outs[1][1]):
            assert np.array_equal(x, y)
    finally:
        prod.close()
        hooks.close()
