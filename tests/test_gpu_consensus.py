"""GPU tests of clc_score_blocks (csrc/clc_consensus.hpp, csrc/abi_batched.hip) and of the consensus calibration built on it.

Scores: per candidate pose k and block b (one block per recorded pose) ssq = sum r^2, cost = 1/2 sum rho(r^2) and the count of records
within tau of their plane.  The expected value is ALWAYS the oracle: oracle.factor_evaluate_batch on the flattened records, grouped by
block with np.add.reduceat — never the code under test.  The two sums are gated at the project's cost gate, 1e-8 relative; what they
actually reach is printed per case and recorded in profiles/consensus.md: at most 2.8e-13, five orders of magnitude inside the gate
(the kernels form the residual as m.p + c0, the oracle as n.(R p + t) + d: metre-sized terms cancelling to a centimetre differ by
~1e-16 * 5 m / 0.01 m per residual; against clc_eval / clc_information, which share the formulation, the sums agree to 3e-16).
Inlier counts must be EQUAL: tau is chosen on the CPU, from the oracle's values, so that no record lies within 1e-12 of it, and that
is asserted first.

The consensus itself: the scenario and its frozen oracle result come from tests/tools/consensus_scenario.py
(tests/golden/consensus_oracle.json); the GPU pipeline must pick the same winning row and the same inlier mask, and its refit must lie
within the parity gates (1e-6 on T_cl, 1e-8 on the cost) of the oracle's refit.

Shared with tests/test_gpu_subsets_fuzz.py, which imports this module: REL_TOL, TAU_MARGIN, LF, _poses, _group, _oracle_tables,
_pick_tau, _rel, _check_case and _map_builds.  Change them with that caller in mind."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import camlasercalibratool_amd as clc
from camlasercalibratool_amd import _capi, resample, simdata as sd

pytestmark = pytest.mark.gpu

REL_TOL = 1e-8     # the project's cost gate
T_TOL = 1e-6
COST_TOL = 1e-8
TAU_MARGIN = 1e-12
LF = 0.05
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scenario():
    spec = importlib.util.spec_from_file_location("consensus_scenario", os.path.join(ROOT, "tests", "tools", "consensus_scenario.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _x_true():
    return sd.pose7_from_T(sd.tlc_to_tcl(sd.GT_RLC, sd.GT_TLC))


def _poses(oracle_mod, n, seed, solution=None):
    """n >= 64 poses: the solution (or the truth), poses perturbed by millimetres to decimetres, and far poses (metres, radians)."""
    rng = np.random.default_rng(seed)
    x = _x_true() if solution is None else solution
    out = [x]
    for k in range(1, n):
        mag = [1e-3, 1e-2, 1e-1][k % 3] if k < n - 12 else [1.0, 3.0, 10.0][k % 3]
        d = rng.normal(size=6) * mag
        if k >= n - 12:
            d[3:] = rng.uniform(-1.5, 1.5, 3)
        out.append(oracle_mod.pose_plus(x, d))
    return np.stack(out)


def _group(v, off):
    """Sums of v over the blocks [off[b], off[b + 1]) with np.add.reduceat (which wants non-empty segments: empty blocks are 0)."""
    out = np.zeros(off.size - 1, dtype=v.dtype)
    ne = np.flatnonzero(np.diff(off) > 0)
    if ne.size:
        out[ne] = np.add.reduceat(v, off[ne])   # (consecutive non-empty blocks: a segment ends where the next one starts)
    return out


def _oracle_tables(oracle_mod, rec, off, poses, use_loss=True):
    """-> ssq [S, B], cost [S, B], plane expressions r0 [S, N] — from the oracle's residuals alone."""
    S, N = len(poses), rec.shape[0]
    ssq = np.empty((S, off.size - 1))
    cost = np.empty_like(ssq)
    r0 = np.empty((S, N))
    a2 = (LF * rec[:, 7]) ** 2
    for k, x in enumerate(poses):
        r, _ = oracle_mod.factor_evaluate_batch(rec, np.ascontiguousarray(x), want_jac=False)
        ssq[k] = _group(r * r, off)
        cost[k] = _group(0.5 * a2 * np.log1p(r * r / a2), off) if use_loss else 0.5 * ssq[k]
        r0[k] = r / rec[:, 7]
    return ssq, cost, r0


def _pick_tau(r0, lo=0.02, hi=0.04):
    """A tau in [lo, hi] that no |r0| comes within TAU_MARGIN of: the middle of the widest gap between the values that fall there."""
    a = np.abs(r0).reshape(-1)
    inside = np.sort(a[(a >= lo) & (a <= hi)])
    edges = np.concatenate([[lo], inside, [hi]])
    i = int(np.argmax(np.diff(edges)))
    tau = 0.5 * (edges[i] + edges[i + 1])
    assert np.abs(a - tau).min() > TAU_MARGIN, "no admissible tau"
    return float(tau)


def _rel(got, want):
    """largest |got - want| / want over the cells with want != 0; cells with want == 0 (empty blocks) must be exactly 0."""
    z = want == 0
    assert np.array_equal(got[z], want[z])
    return float(np.max(np.abs(got[~z] - want[~z]) / np.abs(want[~z]))) if (~z).any() else 0.0


def _check_case(oracle_mod, s, label, rec, off, poses, use_loss=True):
    want_q, want_c, r0 = _oracle_tables(oracle_mod, rec, off, poses, use_loss)
    tau = _pick_tau(r0)
    want_i = np.stack([_group((np.abs(r0[k]) <= tau).astype(np.int64), off) for k in range(len(poses))])
    o = clc.default_options()
    o.use_loss = int(use_loss)
    ssq, cost, inl = s.score_blocks(off, poses, tau, o)
    rq, rc = _rel(ssq, want_q), _rel(cost, want_c)
    print(f"{label}: {len(poses)} poses x {off.size - 1} blocks, {rec.shape[0]} records, tau {tau:.6f}: largest relative difference "
          f"ssq {rq:.3e}  cost {rc:.3e}; inliers {int(want_i.sum())} of {len(poses) * rec.shape[0]}, "
          f"differing cells {int((inl != want_i).sum())}")
    assert rq <= REL_TOL and rc <= REL_TOL, (label, rq, rc)
    assert inl.dtype == np.int32 and np.array_equal(inl, want_i), label
    return ssq, cost, inl, rq, rc


def _upload(s, rec):
    s.upload_batched(rec, np.array([0, rec.shape[0]], dtype=np.int64))
    assert s.path_info().batched_resident == 1


def test_scores_on_the_reference_size_problem_and_consistency(oracle_mod):
    """(a) 50 x 100 points, noise 0.01: 96 poses against the oracle; with and without the loss; the sum over the blocks against
    clc_eval(with_loss = 1) and against chi2 of clc_information, to the same tolerance; two calls return identical bits; nullable
    tables."""
    S = sd.sim_fixed_count(7, 50, 100, noise_sigma=0.01)
    rec = clc.flatten_observations(S, False, False)
    off = clc.calib.pose_block_offsets(S, False, False)
    sol = oracle_mod.solve(rec, _x_true(), linear_solver="qr").pose
    poses = _poses(oracle_mod, 96, 1, sol)
    with clc.Solver(0) as s:
        _upload(s, rec)
        assert s.path_info().batched_lanes == 256
        ssq, cost, inl, _, _ = _check_case(oracle_mod, s, "(a) 50 x 100", rec, off, poses)
        _check_case(oracle_mod, s, "(a) 50 x 100, no loss", rec, off, poses, use_loss=False)
        tau = 0.03
        again = s.score_blocks(off, poses, tau)
        once = s.score_blocks(off, poses, tau)
        assert all(np.array_equal(a, b) for a, b in zip(again, once))
        assert np.array_equal(again[0], ssq) and np.array_equal(again[1], cost)   # (tau moves the counts only)
        # a pose alone returns what it returned in the crowd
        one = s.score_blocks(off, poses[17:18], tau)
        assert all(np.array_equal(a[0], b[17]) for a, b in zip(one, again))
        # nullable tables, straight through the C-ABI
        L, q = s._L, np.full((96, 50), -1.0)
        offc = np.ascontiguousarray(off, dtype=np.int64)
        rc = L.clc_score_blocks(s._h, None, 50, offc.ctypes.data_as(C.POINTER(C.c_int64)), 96, _capi.dptr(np.ascontiguousarray(poses)),
                                C.c_double(tau), None, _capi.dptr(q), None)
        assert rc == 0 and np.array_equal(q, cost)
        # what the library already returns for the whole problem
        s.upload(rec)
        worst_c = worst_q = 0.0
        for k in range(0, 96, 5):
            c, _, _ = s.eval(poses[k], True, LF, want_jacobian=False)
            chi2 = s.information(poses[k])[2]
            worst_c = max(worst_c, abs(cost[k].sum() - c) / c)
            worst_q = max(worst_q, abs(ssq[k].sum() - chi2) / chi2)
        print(f"sum over blocks: cost against clc_eval {worst_c:.3e}, ssq against chi2 of clc_information {worst_q:.3e} (relative)")
        assert worst_c <= REL_TOL and worst_q <= REL_TOL


def test_scores_on_ragged_scans_with_an_empty_pose(oracle_mod):
    """(b) GenerateSimData: ragged scans, among them poses without a point — their blocks score 0 / 0 / 0."""
    S = None
    for seed in range(1, 40):
        S = sd.GenerateSimData(seed, noise_sigma=0.01)
        if np.any(np.diff(S.pts_off) == 0):
            break
    assert np.any(np.diff(S.pts_off) == 0), "no seed with an empty pose"
    rec = clc.flatten_observations(S, False, False)
    off = clc.calib.pose_block_offsets(S, False, False)
    empty = np.flatnonzero(np.diff(off) == 0)
    poses = _poses(oracle_mod, 64, 2)
    with clc.Solver(0) as s:
        _upload(s, rec)
        ssq, cost, inl, _, _ = _check_case(oracle_mod, s, f"(b) ragged, seed {seed}, empty poses {empty.tolist()}", rec, off, poses)
    assert not ssq[:, empty].any() and not cost[:, empty].any() and not inl[:, empty].any()


def test_scores_with_board_edge_terms(oracle_mod):
    """(c) use_boundary_constraint: one block = a pose's point rows and its two edge rows (three planes, three scales)."""
    S = sd.GenerateSimData(3, noise_sigma=0.01)
    rec = clc.flatten_observations(S, True, True)
    off = clc.calib.pose_block_offsets(S, True, True)
    assert off[-1] == rec.shape[0] and np.all(np.diff(off) >= 3)
    with clc.Solver(0) as s:
        _upload(s, rec)
        _check_case(oracle_mod, s, "(c) edge terms", rec, off, _poses(oracle_mod, 64, 3))


def test_scores_with_points_off_the_lidar_plane_and_on_512_lanes(oracle_mod):
    """(d) rows that carry z (512 lanes, a third array); and the 512-lane (x, y) form (more than 256 scans)."""
    rng = np.random.default_rng(4)
    S = sd.sim_fixed_count(12, 18, 400, noise_sigma=0.01)
    rec = clc.flatten_observations(S, False, False)
    rec[:, 6] = rng.normal(size=rec.shape[0]) * 0.01
    off = clc.calib.pose_block_offsets(S, False, False)
    with clc.Solver(0) as s:
        _upload(s, rec)
        pi = s.path_info()
        assert pi.batched_points_carry_z == 1 and pi.batched_lanes == 512
        _check_case(oracle_mod, s, "(d) z rows", rec, off, _poses(oracle_mod, 64, 5))
        S2 = sd.sim_fixed_count(305, 300, 20, noise_sigma=0.01)
        rec2 = clc.flatten_observations(S2, False, False)
        _upload(s, rec2)
        assert s.path_info().batched_lanes == 512
        _check_case(oracle_mod, s, "512 lanes, 300 blocks", rec2, clc.calib.pose_block_offsets(S2, False, False), _poses(oracle_mod, 64, 6))


def _map_builds():
    n = C.c_longlong(-1)
    assert _capi.hooks_lib().clc_debug_lane_map_builds(C.byref(n)) == 0
    return n.value


def test_score_blocks_shares_the_map_and_leaves_the_solves_alone(oracle_mod):
    """A score call between two clc_solve_subsets calls (and two clc_solve_multistart calls) leaves their bits alone; the lane -> block
    map is built ONCE for the three calls, again only when the offsets change or a new upload arrives."""
    S = sd.sim_fixed_count(7, 50, 100, noise_sigma=0.01)
    rec = clc.flatten_observations(S, False, False)
    off = clc.calib.pose_block_offsets(S, False, False)
    x0 = oracle_mod.pose_plus(_x_true(), np.array([.02, -.02, .01, .01, -.01, .02]))
    W = resample.random_subset_weights(50, 24, 8, 3)
    poses = _poses(oracle_mod, 64, 7)
    with clc.Solver(0) as s:
        if not s._L.has_hooks:
            pytest.fail("the suite runs on the hooks build (tests/conftest.py)")
        _upload(s, rec)
        n0 = _map_builds()
        m1, _ = s.solve_multistart(x0[None])
        p1, sm1 = s.solve_subsets(off, W, x0)
        assert _map_builds() == n0 + 1
        q1 = s.score_blocks(off, poses, 0.03)
        assert _map_builds() == n0 + 1            # the map of clc_solve_subsets is reused
        p2, sm2 = s.solve_subsets(off, W, x0)
        m2, _ = s.solve_multistart(x0[None])
        assert _map_builds() == n0 + 1
        assert np.array_equal(p1, p2) and all(a.final_cost == b.final_cost and a.num_iterations == b.num_iterations for a, b in zip(sm1, sm2))
        assert np.array_equal(m1, m2)
        # the other way round: a fresh upload drops the map, the score call builds it, the subsets call reuses it
        _upload(s, rec)
        q2 = s.score_blocks(off, poses, 0.03)
        assert _map_builds() == n0 + 2
        p3, _ = s.solve_subsets(off, W, x0)
        assert _map_builds() == n0 + 2 and np.array_equal(p3, p1)
        assert all(np.array_equal(a, b) for a, b in zip(q1, q2))
        # other offsets (25 blocks of two poses): rebuilt; a block of two poses scores the sum of the two
        off2 = off[::2].copy()
        q3 = s.score_blocks(off2, poses, 0.03)
        assert _map_builds() == n0 + 3
        assert np.array_equal(q3[2], q1[2][:, 0::2] + q1[2][:, 1::2])
        assert np.abs(q3[0] - (q1[0][:, 0::2] + q1[0][:, 1::2])).max() <= 1e-12 * q3[0].max()


def test_score_blocks_refusals_and_non_finite_poses(oracle_mod):
    S = sd.sim_fixed_count(7, 50, 100, noise_sigma=0.01)
    rec = clc.flatten_observations(S, False, False)
    off = clc.calib.pose_block_offsets(S, False, False)
    n = rec.shape[0]
    poses = _poses(oracle_mod, 8, 9)
    with clc.Solver(0) as s:
        with pytest.raises(clc.ClcError, match="CLC_ERR_NO_DATA"):   # nothing uploaded
            s.score_blocks(off, poses, 0.03)
        _upload(s, rec)
        cut = np.concatenate([off[:8], [off[7] + 50], off[8:]])     # a block boundary inside a scan
        with pytest.raises(clc.ClcError, match="CLC_ERR_INVALID_ARG") as e:
            s.score_blocks(cut, poses, 0.03)
        assert "whole scans" in str(e.value)
        for bad in (off + 1, off[:-1], np.concatenate([off[:3], [off[2] - 1], off[3:]])):   # start, end, monotone
            with pytest.raises(clc.ClcError, match="CLC_ERR_INVALID_ARG"):
                s.score_blocks(bad, poses, 0.03)
        with pytest.raises(clc.ClcError, match="CLC_ERR_INVALID_ARG"):
            s.score_blocks(off, poses, float("nan"))
        o = clc.default_options()
        o.loss_scale_factor = 0.0
        with pytest.raises(clc.ClcError, match="CLC_ERR_INVALID_ARG"):
            s.score_blocks(off, poses, 0.03, o)
        # the refusals left the handle usable; a non-finite pose does not fail the call: NaN / NaN / 0 in its row, the others untouched
        want = s.score_blocks(off, poses, 0.03)
        bad_poses = poses.copy()
        bad_poses[2, 1] = np.nan
        bad_poses[5, 4] = np.inf
        ssq, cost, inl = s.score_blocks(off, bad_poses, 0.03)
        for k in range(8):
            if k in (2, 5):
                assert np.isnan(ssq[k]).all() and np.isnan(cost[k]).all() and not inl[k].any()
            else:
                assert np.array_equal(ssq[k], want[0][k]) and np.array_equal(cost[k], want[1][k]) and np.array_equal(inl[k], want[2][k])
        # a negative tau: nothing is an inlier
        assert not s.score_blocks(off, poses, -1.0)[2].any()
        # a batch of two problems is not ONE shared problem
        s.upload_batched(np.tile(rec, (2, 1)), np.array([0, n, 2 * n], dtype=np.int64))
        with pytest.raises(clc.ClcError, match="CLC_ERR_NO_DATA"):
            s.score_blocks(off, poses, 0.03)
        # a problem beyond one workgroup
        big = clc.flatten_observations(sd.sim_fixed_count(9, 60, 500, noise_sigma=0.01), False)
        s.upload_batched(big, np.array([0, big.shape[0]], dtype=np.int64))
        assert s.path_info().batched_resident == 0
        with pytest.raises(clc.ClcError, match="CLC_ERR_INVALID_ARG") as e:
            s.score_blocks(np.arange(61, dtype=np.int64) * 500, poses, 0.03)
        assert "workgroup" in str(e.value)


def test_consensus_calibration_against_the_frozen_oracle_and_the_dropin_program(oracle_mod, tmp_path):
    """The scenario of tests/tools/consensus_scenario.py: 10 of 50 poses 0.08 m off along the board normal.  The GPU pipeline must pick
    the oracle's winning row and inlier mask (exactly the 40 clean poses) and refit within the parity gates of the oracle's refit; the
    drop-in program, given the same rows, returns the same."""
    sc = _scenario()
    want = json.load(open(sc.FIXTURE))
    S, bad, off = sc.build()
    T0 = sd.T_from_pose7(sc.start_pose(oracle_mod))
    T = T0.copy()
    out = clc.CamLaserCalibrationConsensus(S, T, False, False, n=sc.N_ROWS, m=sc.M, rms_max=sc.RMS_MAX, seed=want["seed"])
    mask = np.array(want["inlier_mask"], dtype=bool)
    print("winning row", out["best"], "support", int(out["sizes"][out["best"]]), "of", S.n_poses, "| oracle:", want["best"], want["support"])
    assert out["best"] == want["best"]
    assert np.array_equal(out["inliers"], mask) and np.array_equal(np.flatnonzero(~out["inliers"]), bad)
    dT = np.abs(T - sd.T_from_pose7(np.array(want["refit_pose"]))).max()
    dc = abs(out["summary"].final_cost - want["refit_cost"])
    gt = sd.T_from_pose7(sc.ground_truth())
    print(f"refit against the oracle's refit: |dT| {dT:.3e} |dcost| {dc:.3e}; against the ground truth: consensus "
          f"{np.abs(T - gt).max():.3e} (oracle {want['consensus_max_abs_dT_vs_ground_truth']:.3e}), plain oracle solve "
          f"{want['plain_max_abs_dT_vs_ground_truth']:.3e}")
    assert dT <= T_TOL and dc <= COST_TOL
    assert np.array_equal(T, sd.T_from_pose7(out["pose"]))
    # per-pose RMS at the result: the oracle's residuals at the GPU's refit
    rec = clc.flatten_observations(S, False, False)
    rms_want = np.sqrt(sc.oracle_scores(oracle_mod, rec, off, [out["pose"]])[0])
    assert np.abs(out["rms"] - rms_want).max() <= 1e-8 * rms_want.max()
    assert out["rms"][mask].max() <= sc.RMS_MAX < out["rms"][~mask].min()
    # the same through the C++ header, on the same rows
    path = str(tmp_path / "obs.txt")
    W = out["weights"]
    with open(path, "w") as f:
        f.write(f"{S.n_poses} {sc.RMS_MAX!r} {W.shape[0]}\n" + " ".join(repr(float(v)) for v in T0.reshape(-1)) + "\n")
        f.write("\n".join(" ".join(str(int(v)) for v in row) for row in W) + "\n")
        for i in range(S.n_poses):
            pts = S.pts[S.pts_off[i]:S.pts_off[i + 1]]
            f.write(" ".join(repr(float(v)) for v in list(S.tag_q[i]) + list(S.tag_t[i])) + f" {pts.shape[0]}\n")
            f.write("\n".join(" ".join(repr(float(v)) for v in p) for p in pts) + "\n")
    p = subprocess.run([_build_consensus_exe(), path, "0", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    m = re.search(r"^BEST (\d+) cost=(\S+)$", p.stdout, flags=re.M)
    assert m and int(m.group(1)) == want["best"] and abs(float(m.group(2)) - want["refit_cost"]) <= COST_TOL
    got_mask = [int(v) for v in re.search(r"^MASK (.*)$", p.stdout, flags=re.M).group(1).split()]
    assert got_mask == want["inlier_mask"]
    assert [int(v) for v in re.search(r"^SIZES (.*)$", p.stdout, flags=re.M).group(1).split()] == out["sizes"].tolist()
    Tc = np.array([float(v) for v in re.search(r"^TCL (.*)$", p.stdout, flags=re.M).group(1).split()]).reshape(4, 4)
    # (the program's start went through a pose -> matrix -> pose round trip: the same solves to rounding, not to the bit)
    print("drop-in program against the Python path: |dT|", np.abs(Tc - T).max())
    assert np.abs(Tc - T).max() <= T_TOL and np.abs(Tc - sd.T_from_pose7(np.array(want["refit_pose"]))).max() <= T_TOL
    rms_c = np.array([float(v) for v in re.search(r"^RMS (.*)$", p.stdout, flags=re.M).group(1).split()])
    assert np.abs(rms_c - out["rms"]).max() <= 1e-7
    # rows drawn by the header itself (std::mt19937, a stream of its own): the call runs and reports a winner with a support
    d = re.search(r"^DRAWN ok=(\d) best=(-?\d+) support=(\d+)$", p.stdout, flags=re.M)
    assert d and d.group(1) == "1" and 0 <= int(d.group(2)) < 64 and int(d.group(3)) >= sc.M


def _build_consensus_exe():
    from camlasercalibratool_amd import _build
    exe = os.path.join(ROOT, "tests", "dropin", "consensus_main")
    src = os.path.join(ROOT, "tests", "dropin", "consensus_main.cpp")
    deps = [src, os.path.join(ROOT, "include", "LaseCamCalCeres.h"), os.path.join(ROOT, "include", "clc.h"), _build.LIB_PATH]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        lib_dir = os.path.dirname(_build.LIB_PATH)
        subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(ROOT, "tests", "dropin", "eigen_stub"), src, "-o", exe,
                               "-L", lib_dir, "-lclc_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe
