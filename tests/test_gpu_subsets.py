"""GPU tests of clc_solve_subsets (csrc/clc_resident.hpp WEIGHTED, csrc/abi_batched.hip): resampled calibrations — jackknife, bootstrap,
random subsets of the poses — as weight rows on ONE uploaded problem, a workgroup per row.

The contract: subset k IS the problem in which every record of block b appears w[k, b] times (resample.materialize).  So every row is
checked against the oracle's DENSE_QR solve of the materialised records, inside the project's gates (|dT|inf <= 1e-6, |d final cost|
<= 1e-8, same iteration count and termination); where iteration count or termination differ, only if lm_near_tie finds one of the
controller's decisions within TIE_REL of its threshold on the oracle's own trace (a weighted sum and repeated records are summed in
different orders), and for at most 1 % of a test's rows."""
import os
import re
import subprocess

import numpy as np
import pytest

import camlasercalibratool_amd as clc
import lm_near_tie as NT
from camlasercalibratool_amd import _capi, resample, simdata as sd

pytestmark = pytest.mark.gpu

T_TOL = 1e-6
COST_TOL = 1e-8
EXCUSED_SHARE = 0.01
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _x_true():
    return sd.pose7_from_T(sd.tlc_to_tcl(sd.GT_RLC, sd.GT_TLC))


def _dT(a, b):
    return np.abs(sd.T_from_pose7(a) - sd.T_from_pose7(b)).max()


def _offsets(n_poses, per):
    return np.arange(n_poses + 1, dtype=np.int64) * per


def _gate_rows(oracle_mod, rec, off, W, starts, poses, sms, label, rows=None):
    """Every row (or `rows`) against the oracle on the materialised records; -> number of near-tie exemptions (capped)."""
    oo = oracle_mod.default_options()
    starts = np.broadcast_to(np.asarray(starts).reshape(-1, 7), (W.shape[0], 7))
    rows = range(W.shape[0]) if rows is None else rows
    excused, n = 0, 0
    for k in rows:
        n += 1
        sub = resample.materialize(rec, off, W[k])
        ref = oracle_mod.solve(sub, starts[k], oo, linear_solver="qr")
        got = (sms[k].termination, sms[k].num_iterations, sms[k].final_cost)
        want = (ref.summary.termination, ref.summary.num_iterations, ref.summary.final_cost)
        dT, dc = _dT(poses[k], ref.pose), abs(sms[k].final_cost - ref.summary.final_cost)
        print(f"{label} row {k}: w max {int(W[k].max())} sum {int(W[k].sum())} it {got[1]}/{want[1]} term {got[0]}/{want[0]} "
              f"dT {dT:.3e} dcost {dc:.3e}")
        if NT.check_flip(oracle_mod, sub, starts[k], oo, got, want, f"{label} row {k}"):
            excused += 1
            continue
        assert dc <= COST_TOL, (label, k, sms[k].final_cost, ref.summary.final_cost)
        assert dT <= T_TOL, (label, k, dT)
    assert excused <= EXCUSED_SHARE * n, (label, excused, n)
    return excused


def _reference_problem():
    """50 poses x 100 points, the start 1-2 cm / 0.01-0.02 rad off the truth; 50 leave-one-out rows, 60 bootstrap rows (largest
    multiplicity 6), 20 random 8-of-50 subsets and the all-ones row."""
    S = sd.sim_fixed_count(7, 50, 100, noise_sigma=0.01)
    rec = clc.flatten_observations(S, False, False)
    off = clc.calib.pose_block_offsets(S, False, False)
    assert np.array_equal(off, _offsets(50, 100))
    W = [resample.jackknife_weights(50)]
    rng = np.random.default_rng(3)
    W.append(np.stack([np.bincount(rng.integers(0, 50, 50), minlength=50) for _ in range(60)]).astype(np.uint8))
    sub = np.zeros((20, 50), dtype=np.uint8)
    for k in range(20):
        sub[k, rng.choice(50, 8, replace=False)] = 1
    W.append(sub)
    W.append(np.ones((1, 50), dtype=np.uint8))
    W = np.concatenate(W)
    assert W.shape == (131, 50) and W.max() == 6
    return rec, off, W


def _start(oracle_mod):
    return oracle_mod.pose_plus(_x_true(), np.array([.02, -.02, .01, .01, -.01, .02]))


def test_subsets_against_the_oracle_and_multistart(oracle_mod):
    """The 131 weight rows of the reference-size problem: the all-ones row is bit-identical to clc_solve_multistart from the same start
    (weight 1 multiplies scale^2 by 1.0: a no-op); every other row against the oracle; a second call returns the same bits; a row alone
    returns what it returned in the crowd; clc_solve_multistart before and after the subsets call: the same bits (shared layout untouched)."""
    rec, off, W = _reference_problem()
    x0 = _start(oracle_mod)
    with clc.Solver(0) as s:
        s.upload_batched(rec, np.array([0, rec.shape[0]], dtype=np.int64))
        pi = s.path_info()
        assert pi.batched_resident == 1 and pi.batched_lanes == 256
        ms_before, msm = s.solve_multistart(x0[None])
        poses, sms = s.solve_subsets(off, W, x0)
        again, asm = s.solve_subsets(off, W, x0)
        ms_after, msm2 = s.solve_multistart(x0[None])
        one, osm = s.solve_subsets(off, W[57:58], x0)
        other, _ = s.solve_subsets(_offsets(25, 200), np.ones((1, 25), dtype=np.uint8), x0)   # other offsets: the map is rebuilt
        back, _ = s.solve_subsets(off, W[57:58], x0)
    assert np.array_equal(ms_before, ms_after) and msm[0].final_cost == msm2[0].final_cost
    assert np.array_equal(poses, again) and all(sms[k].final_cost == asm[k].final_cost for k in range(len(W)))
    assert np.array_equal(poses[130], ms_before[0])
    assert (sms[130].final_cost, sms[130].num_iterations, sms[130].termination, sms[130].initial_cost) == \
        (msm[0].final_cost, msm[0].num_iterations, msm[0].termination, msm[0].initial_cost)
    assert np.array_equal(one[0], poses[57]) and osm[0].num_iterations == sms[57].num_iterations
    assert np.array_equal(other[0], ms_before[0]) and np.array_equal(back[0], poses[57])
    assert all(sms[k].termination == _capi_termination("CONVERGENCE(function)") for k in range(len(W)))
    _gate_rows(oracle_mod, rec, off, W, x0, poses, sms, "reference")
    # leaving a pose out matters: the rows do differ
    assert len({poses[k].tobytes() for k in range(len(W))}) == len(W)


def _capi_termination(name):
    return {v: k for k, v in _capi.TERMINATION.items()}[name]


def test_subsets_against_the_batch_of_materialised_problems(oracle_mod):
    """Each row against clc_solve_batched of the materialised sub-problems (the route without this call): inside the gates — not bit
    for bit, the lane plans differ."""
    rec, off, W = _reference_problem()
    x0 = _start(oracle_mod)
    subs = [resample.materialize(rec, off, w) for w in W]
    boff = np.zeros(len(subs) + 1, dtype=np.int64)
    boff[1:] = np.cumsum([r.shape[0] for r in subs])
    with clc.Solver(0) as s:
        s.upload_batched(rec, np.array([0, rec.shape[0]], dtype=np.int64))
        poses, sms = s.solve_subsets(off, W, x0)
        s.upload_batched(np.concatenate(subs), boff)
        bp, bsm = s.solve_batched(np.tile(x0, (len(subs), 1)))
    for k in range(len(W)):
        print(f"row {k}: dT {_dT(poses[k], bp[k]):.3e} dcost {abs(sms[k].final_cost - bsm[k].final_cost):.3e}")
        assert (sms[k].num_iterations, sms[k].termination) == (bsm[k].num_iterations, bsm[k].termination), k
        assert _dT(poses[k], bp[k]) <= T_TOL and abs(sms[k].final_cost - bsm[k].final_cost) <= COST_TOL, k


def _mixed_rows(P, n, seed):
    """n rows: leave-one-out, bootstrap (multiplicities > 1), random half, all-ones."""
    rng = np.random.default_rng(seed)
    W = [resample.jackknife_weights(P)[[0, P // 2, P - 1]], resample.bootstrap_weights(P, n - 6, seed),
         resample.random_subset_weights(P, 2, P // 2, seed), np.ones((1, P), dtype=np.uint8)]
    W = np.concatenate(W)
    assert W.shape[0] == n and W.max() > 1
    return W[rng.permutation(n)]


def test_subsets_on_512_lanes(oracle_mod):
    """More than 256 scans: the 512-lane form (300 poses x 20 points)."""
    S = sd.sim_fixed_count(305, 300, 20, noise_sigma=0.01)
    rec = clc.flatten_observations(S, False, False)
    off = clc.calib.pose_block_offsets(S, False, False)
    W = _mixed_rows(300, 12, 5)
    x0 = oracle_mod.pose_plus(_x_true(), np.array([.01, .02, -.01, -.02, .01, .01]))
    with clc.Solver(0) as s:
        s.upload_batched(rec, np.array([0, rec.shape[0]], dtype=np.int64))
        pi = s.path_info()
        assert pi.batched_resident == 1 and pi.batched_lanes == 512
        poses, sms = s.solve_subsets(off, W, x0)
        ms, msm = s.solve_multistart(x0[None])
    ones = int(np.flatnonzero((W == 1).all(axis=1))[0])
    assert np.array_equal(poses[ones], ms[0]) and sms[ones].final_cost == msm[0].final_cost
    _gate_rows(oracle_mod, rec, off, W, x0, poses, sms, "512 lanes")


def test_subsets_with_points_off_the_lidar_plane(oracle_mod):
    """The points carry z (512 lanes, 24-byte slots, masked padding), as test_multistart_with_points_off_the_lidar_plane_and_timed;
    per-row starts; profile_events = 1 reports the one launch."""
    rng = np.random.default_rng(4)
    S = sd.sim_fixed_count(12, 18, 400, noise_sigma=0.01)
    rec = clc.flatten_observations(S, False, False)
    rec[:, 6] = rng.normal(size=rec.shape[0]) * 0.01
    off = clc.calib.pose_block_offsets(S, False, False)
    W = _mixed_rows(18, 10, 9)
    with clc.Solver(0) as s:
        starts = s.pose_plus(np.tile(_x_true(), (10, 1)), rng.normal(size=(10, 6)) * 0.02)
        s.upload_batched(rec, np.array([0, rec.shape[0]], dtype=np.int64))
        pi = s.path_info()
        assert pi.batched_resident == 1 and pi.batched_points_carry_z == 1 and pi.batched_lanes == 512
        o = clc.default_options()
        o.profile_events = 1
        poses, sms = s.solve_subsets(off, W, starts, o)
    assert all(sm.eval_kernel_launches == 1 and sm.eval_kernel_ms > 0 for sm in sms)
    _gate_rows(oracle_mod, rec, off, W, starts, poses, sms, "z form")


def test_subsets_with_board_edge_terms(oracle_mod):
    """use_boundary_constraint: a pose's block spans three scans — its point rows and its two edge rows (planes of their own)."""
    S = sd.GenerateSimData(3, noise_sigma=0.01)
    rec = clc.flatten_observations(S, True, True)
    off = clc.calib.pose_block_offsets(S, True, True)
    P = S.n_poses
    assert off[-1] == rec.shape[0] and np.all(np.diff(off) >= 3)
    W = _mixed_rows(P, 11, 2)
    x0 = oracle_mod.pose_plus(_x_true(), np.array([-.01, .01, .02, .01, .02, -.01]))
    with clc.Solver(0) as s:
        s.upload_batched(rec, np.array([0, rec.shape[0]], dtype=np.int64))
        assert s.path_info().batched_resident == 1
        poses, sms = s.solve_subsets(off, W, x0)
    _gate_rows(oracle_mod, rec, off, W, x0, poses, sms, "edge terms")


def test_subsets_refusals_and_empty_rows(oracle_mod):
    """Decided on the host or by the flag of the lane-map kernel; nothing here reaches the solve kernel with bad input."""
    rec, off, W = _reference_problem()
    x0 = _start(oracle_mod)
    n = rec.shape[0]
    with clc.Solver(0) as s:
        s.upload_batched(rec, np.array([0, n], dtype=np.int64))
        # a block boundary inside a scan: pose 7's points cut in two blocks with different weights
        cut = np.concatenate([off[:8], [off[7] + 50], off[8:]])
        wc = np.ones((1, 51), dtype=np.uint8)
        wc[0, 7] = 2
        with pytest.raises(clc.ClcError, match="CLC_ERR_INVALID_ARG"):
            s.solve_subsets(cut, wc, x0)
        for bad in (off + 1, off[:-1], np.concatenate([off[:3], [off[2] - 1], off[3:]])):   # start, end, monotone
            with pytest.raises(clc.ClcError, match="CLC_ERR_INVALID_ARG"):
                s.solve_subsets(bad, np.ones((1, len(bad) - 1), dtype=np.uint8), x0)
        # the refusals left the handle usable; an all-zero row fails alone
        Wz = np.concatenate([W[:2], np.zeros((1, 50), dtype=np.uint8), W[2:4]])
        poses, sms = s.solve_subsets(off, Wz, x0)
        ref_p, ref_s = s.solve_subsets(off, W[:4], x0)
        assert sms[2].termination == _capi_termination("FAILURE") and np.array_equal(poses[2], x0)
        for a, b in ((0, 0), (1, 1), (3, 2), (4, 3)):
            assert np.array_equal(poses[a], ref_p[b]) and sms[a].final_cost == ref_s[b].final_cost
        _gate_rows(oracle_mod, rec, off, Wz, x0, poses, sms, "next to an empty row", rows=(0, 1, 3, 4))
        # a batch of two problems is not ONE shared problem
        s.upload_batched(np.tile(rec, (2, 1)), np.array([0, n, 2 * n], dtype=np.int64))
        with pytest.raises(clc.ClcError, match="CLC_ERR_NO_DATA"):
            s.solve_subsets(off, W[:2], x0)
        # a problem beyond one workgroup
        big = clc.flatten_observations(sd.sim_fixed_count(9, 60, 500, noise_sigma=0.01), False)
        s.upload_batched(big, np.array([0, big.shape[0]], dtype=np.int64))
        assert s.path_info().batched_resident == 0
        with pytest.raises(clc.ClcError, match="CLC_ERR_INVALID_ARG") as e:
            s.solve_subsets(_offsets(60, 500), np.ones((2, 60), dtype=np.uint8), x0)
        assert "workgroup" in str(e.value)


def test_calibration_resample_jackknife_and_the_dropin_program(oracle_mod, tmp_path):
    """clc.CamLaserCalibrationResample (jackknife) on the simulation node's observations: its covariance equals
    resample.jackknife_covariance of the oracle's solves of the materialised subsets to 1e-9 relative on the diagonal; the drop-in
    program returns the same poses through clc_adapter::Session::CalibrationSubsets."""
    S = sd.GenerateSimData(3, noise_sigma=0.01)
    T0 = sd.T_from_pose7(oracle_mod.pose_plus(_x_true(), np.array([.02, -.01, .01, -.01, .02, .01])))
    T = T0.copy()
    out = clc.CamLaserCalibrationResample(S, T, False, False, mode="jackknife")
    rec = clc.flatten_observations(S, False, False)
    off = clc.calib.pose_block_offsets(S, False, False)
    P = S.n_poses
    full = oracle_mod.solve(rec, sd.pose7_from_T(T0), linear_solver="qr")
    assert np.abs(T - sd.T_from_pose7(full.pose)).max() <= T_TOL
    W = resample.jackknife_weights(P)
    assert np.array_equal(out["weights"], W)
    X = np.stack([oracle_mod.solve(resample.materialize(rec, off, W[k]), out["pose"], linear_solver="qr").pose for k in range(P)])
    want = resample.jackknife_covariance(out["pose"], X)
    rel = np.abs(np.diag(out["covariance"]) - np.diag(want)) / np.diag(want)
    print("jackknife covariance diagonal", np.diag(out["covariance"]), "relative difference", rel)
    assert np.all(rel <= 1e-9)
    assert out["influence"].shape == (P,) and np.allclose(out["influence"], np.linalg.norm(resample.local_deltas(out["pose"], X), axis=1),
                                                          rtol=0, atol=1e-7)
    # the same through the C++ header: the program reads the same observations and the full solution as its start, solves the
    # leave-one-out rows and one all-zero row, and prints every Tcl
    Tfull = sd.T_from_pose7(out["pose"])
    path = str(tmp_path / "obs.txt")
    with open(path, "w") as f:
        f.write(f"{P}\n" + " ".join(repr(float(v)) for v in Tfull.reshape(-1)) + "\n")
        for i in range(P):
            pts = S.pts[S.pts_off[i]:S.pts_off[i + 1]]
            f.write(" ".join(repr(float(v)) for v in list(S.tag_q[i]) + list(S.tag_t[i])) + f" {pts.shape[0]}\n")
            f.write("\n".join(" ".join(repr(float(v)) for v in p) for p in pts) + "\n")
    p = subprocess.run([_build_subsets_exe(), path, "0", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = re.findall(r"^SUBSET (\d+) term=(\d+) cost=(\S+) T=(.*)$", p.stdout, flags=re.M)
    assert len(rows) == P + 1
    worst = 0.0
    for k in range(P):
        Tk = np.array([float(v) for v in rows[k][3].split()]).reshape(4, 4)
        assert int(rows[k][0]) == k and int(rows[k][1]) == out["summaries"][k].termination
        # (the program starts from the full solution after a pose -> matrix -> pose round trip: the same solve to rounding, not to the bit)
        worst = max(worst, np.abs(Tk - sd.T_from_pose7(out["poses"][k])).max())
        assert abs(float(rows[k][2]) - out["summaries"][k].final_cost) <= COST_TOL, k
    print("drop-in program against the Python path: largest |dT|", worst)
    assert worst <= T_TOL
    Tz = np.array([float(v) for v in rows[P][3].split()]).reshape(4, 4)
    assert int(rows[P][1]) == _capi_termination("FAILURE") and np.array_equal(Tz, Tfull)   # the empty row: reported, its Tcl untouched


def _build_subsets_exe():
    from camlasercalibratool_amd import _build
    exe = os.path.join(ROOT, "tests", "dropin", "subsets_main")
    src = os.path.join(ROOT, "tests", "dropin", "subsets_main.cpp")
    deps = [src, os.path.join(ROOT, "include", "LaseCamCalCeres.h"), os.path.join(ROOT, "include", "clc.h"), _build.LIB_PATH]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        lib_dir = os.path.dirname(_build.LIB_PATH)
        subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(ROOT, "tests", "dropin", "eigen_stub"), src, "-o", exe,
                               "-L", lib_dir, "-lclc_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


FLAG_RESIDENT_WG512 = 8192     # clc_set_launch: the 512-lane form even where 256 lanes hold the problem (include/clc.h)


@pytest.mark.parametrize("use_loss", [True, False], ids=["loss", "no-loss"])
@pytest.mark.parametrize("form", [256, 512, "z"])
def test_subsets_in_every_form_of_the_launch(oracle_mod, form, use_loss):
    """The three forms the weighted launch takes — 256 lanes, 512 lanes by launch flag 8192, 512 lanes with z (ONE record with p.z != 0)
    — each with and without the loss, at the smallest shape: 6 blocks of one scan each, 4 weight rows, one of them empty.  Every
    solved row against clc_solve_batched of the materialised subsets: the rows of weights 0 / 1 that keep every kept lane where it is
    (all ones; the last block left out) bit for bit — weight 1 multiplies by 1.0, a lane of weight 0 adds exact zeros, the lanes in
    front of it are dealt as in the materialised problem, so every sum has the same terms in the same order —, the row with
    multiplicities inside the gates of test_subsets_against_the_batch_of_materialised_problems (repeated records are other lanes).
    The all-ones row bitwise clc_solve_multistart; clc_solve_multistart before and after the subsets call: the same bits."""
    S = sd.sim_fixed_count(21, 6, 30, noise_sigma=0.01)
    rec = clc.flatten_observations(S, False, False)
    off = clc.calib.pose_block_offsets(S, False, False)
    assert np.array_equal(off, _offsets(6, 30))
    if form == "z":
        rec[47, 6] = 0.01
    W = np.array([[1, 1, 1, 1, 1, 1], [2, 1, 1, 0, 1, 3], [0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 0]], dtype=np.uint8)
    x0 = oracle_mod.pose_plus(_x_true(), np.array([.01, -.01, .01, .01, -.01, .01]))
    o = clc.default_options()
    o.use_loss = int(use_loss)
    solved = [0, 1, 3]
    subs = [resample.materialize(rec, off, W[k]) for k in solved]
    boff = np.zeros(len(subs) + 1, dtype=np.int64)
    boff[1:] = np.cumsum([r.shape[0] for r in subs])
    with clc.Solver(0) as s:
        if form == 512:
            s.set_launch(0, FLAG_RESIDENT_WG512 | 2 | 16 | 32 | 128 | 256 | 512)     # (the default flags + 8192)
        s.upload_batched(rec, np.array([0, rec.shape[0]], dtype=np.int64))
        pi = s.path_info()
        assert (pi.batched_resident, pi.batched_lanes, pi.batched_points_carry_z) == (1, 256 if form == 256 else 512, int(form == "z"))
        ms_before, msm = s.solve_multistart(x0[None], o)
        poses, sms = s.solve_subsets(off, W, x0, o)
        again, asm = s.solve_subsets(off, W, x0, o)
        ms_after, msm2 = s.solve_multistart(x0[None], o)
        s.upload_batched(np.concatenate(subs), boff)
        pb = s.path_info()
        assert (pb.batched_resident, pb.batched_lanes, pb.batched_points_carry_z) == (1, 256 if form == 256 else 512, int(form == "z"))
        bp, bsm = s.solve_batched(np.tile(x0, (len(subs), 1)), o)
    key = lambda m: (m.termination, m.num_iterations, m.num_evaluations, m.initial_cost, m.final_cost)
    assert np.array_equal(ms_before, ms_after) and key(msm[0]) == key(msm2[0])
    assert np.array_equal(poses, again) and all(key(sms[k]) == key(asm[k]) for k in range(4))
    assert np.array_equal(poses[0], ms_before[0]) and key(sms[0]) == key(msm[0])
    assert sms[2].termination == _capi_termination("FAILURE") and np.array_equal(poses[2], x0)
    for j, k in enumerate(solved):
        bits = np.array_equal(poses[k], bp[j]) and sms[k].final_cost == bsm[j].final_cost
        print(f"{form} {'loss' if use_loss else 'no loss'} row {k}: it {sms[k].num_iterations}/{bsm[j].num_iterations} dT {_dT(poses[k], bp[j]):.3e} "
              f"dcost {abs(sms[k].final_cost - bsm[j].final_cost):.3e} same bits {bits}")
        assert (sms[k].num_iterations, sms[k].termination) == (bsm[j].num_iterations, bsm[j].termination), k
        assert _dT(poses[k], bp[j]) <= T_TOL and abs(sms[k].final_cost - bsm[j].final_cost) <= COST_TOL, k
        if W[k].max() == 1:
            assert bits and key(sms[k]) == key(bsm[j]), k
