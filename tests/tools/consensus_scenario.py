#!/usr/bin/env python3
"""The scenario of the consensus calibration test (tests/test_gpu_consensus.py) and the generator of its frozen ORACLE result,
tests/golden/consensus_oracle.json.  Needs no GPU: everything here is computed with the CPU oracle alone.

Scenario: sim_fixed_count(7, 50, 100, noise 0.01) — 50 poses x 100 points, sigma = 0.01 m.  K_BAD = 10 of the 50 poses (drawn with
default_rng(CORRUPT_SEED)) get a wrong tag pose: their tag translation moved OFFSET = 0.08 m along the board normal (the third column
of R_ca) — a whole scan consistently off by centimetres, as a tag pose taken from the wrong camera frame gives.  The start is the
ground truth moved by START_DELTA (centimetres / hundredths of a radian).  Candidates: N_ROWS random M-of-50 rows
(resample.random_subset_weights(50, N_ROWS, M, seed)), threshold RMS_MAX = 3 sigma.

The oracle's pipeline is the adapters' pipeline with every GPU call replaced by its definition: resample.materialize + oracle.solve for
the subset solves and the refit, oracle.factor_evaluate_batch grouped with np.add.reduceat for the scores, the same
resample.consensus_select.

Conditions on the scenario (checked here, not in the test; a seed that misses one is skipped, none is loosened):
  * the plain oracle solve of all 50 poses is visibly off the ground truth, the consensus refit recovers it (both RECORDED);
  * the winner's inlier mask is exactly the 40 clean poses (support = P - K_BAD);
  * the best candidate with a DIFFERENT mask lies at least 2 blocks behind;
  * many clean candidates tie on support and are separated by the sum of ssq only: the winner's sum is below the runner-up's (same
    support, any mask) by a relative gap of at least 1e-6 (GPU and oracle subset solves differ around 1e-12).

usage: python tests/tools/consensus_scenario.py [--write]      (prints the figures; --write refreshes the fixture)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from camlasercalibratool_amd import resample, simdata as sd  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "consensus_oracle.json")
SIM_SEED, N_POSES, N_PTS, SIGMA = 7, 50, 100, 0.01
K_BAD, OFFSET, CORRUPT_SEED = 10, 0.08, 11
N_ROWS, M = 128, 5
RMS_MAX = 3 * SIGMA
START_DELTA = np.array([0.03, -0.02, 0.04, 0.02, -0.03, 0.02])


def ground_truth():
    return sd.pose7_from_T(sd.tlc_to_tcl(sd.GT_RLC, sd.GT_TLC))


def build():
    """-> (observation set with the K_BAD wrong tag poses, indices of the wrong poses (sorted), block offsets [P + 1])."""
    S = sd.sim_fixed_count(SIM_SEED, N_POSES, N_PTS, noise_sigma=SIGMA)
    bad = np.sort(np.random.default_rng(CORRUPT_SEED).choice(N_POSES, K_BAD, replace=False))
    for i in bad:
        S.tag_t[i] = S.tag_t[i] + OFFSET * sd.quat_wxyz_to_rot(S.tag_q[i])[:, 2]
    return S, bad, np.arange(N_POSES + 1, dtype=np.int64) * N_PTS


def start_pose(oracle):
    return oracle.pose_plus(ground_truth(), START_DELTA)


def oracle_scores(oracle, rec, off, poses):
    """ssq [S, B] from the oracle's residuals, grouped by block."""
    out = np.empty((len(poses), off.size - 1))
    for k, x in enumerate(poses):
        r, _ = oracle.factor_evaluate_batch(rec, np.ascontiguousarray(x), want_jac=False)
        out[k] = np.add.reduceat(r * r, off[:-1])
    return out


def oracle_pipeline(oracle, seed):
    S, bad, off = build()
    rec = oracle.flatten(S, False, False)
    x0 = start_pose(oracle)
    W = resample.random_subset_weights(N_POSES, N_ROWS, M, seed)
    cands = np.stack([oracle.solve(resample.materialize(rec, off, w), x0, linear_solver="qr").pose for w in W])
    ssq = oracle_scores(oracle, rec, off, cands)
    best, mask, sizes = resample.consensus_select(ssq, RMS_MAX)
    refit = oracle.solve(resample.materialize(rec, off, mask.astype(np.uint8)), cands[best], linear_solver="qr")
    plain = oracle.solve(rec, x0, linear_solver="qr")
    rms = np.sqrt(oracle_scores(oracle, rec, off, [refit.pose])[0])
    # separation: the best candidate with another mask; the runner-up on the tie-break among the candidates with the winner's support
    sup = np.sqrt(ssq) <= RMS_MAX
    other = [int(sizes[k]) for k in range(N_ROWS) if not np.array_equal(sup[k], mask)]
    total = np.where(sup, ssq, 0.0).sum(axis=1)
    ties = sorted(float(total[k]) for k in range(N_ROWS) if k != best and sizes[k] == sizes[best])
    gt = sd.T_from_pose7(ground_truth())
    return {
        "seed": int(seed), "bad_poses": [int(i) for i in bad], "best": int(best), "inlier_mask": [int(v) for v in mask],
        "support": int(sizes[best]), "support_of_best_other_mask": max(other) if other else 0,
        "tie_break_gap": (ties[0] - float(total[best])) / float(total[best]) if ties else None,
        "candidates_tied_on_support": len(ties) + 1,
        "refit_pose": [float(v) for v in refit.pose], "refit_cost": float(refit.summary.final_cost),
        "refit_termination": int(refit.summary.termination),
        "plain_pose": [float(v) for v in plain.pose], "plain_cost": float(plain.summary.final_cost),
        "plain_max_abs_dT_vs_ground_truth": float(np.abs(sd.T_from_pose7(plain.pose) - gt).max()),
        "consensus_max_abs_dT_vs_ground_truth": float(np.abs(sd.T_from_pose7(refit.pose) - gt).max()),
        "rms_at_refit_clean_max": float(rms[mask].max()), "rms_at_refit_bad_min": float(rms[~mask].min()),
        "scenario": {"sim": [SIM_SEED, N_POSES, N_PTS, SIGMA], "k_bad": K_BAD, "offset_m": OFFSET, "corrupt_seed": CORRUPT_SEED,
                     "rows": N_ROWS, "m": M, "rms_max": RMS_MAX, "start_delta": [float(v) for v in START_DELTA]},
    }


def separates(res):
    clean = np.ones(N_POSES, dtype=bool)
    clean[res["bad_poses"]] = False
    return (np.array_equal(np.array(res["inlier_mask"], dtype=bool), clean) and res["support"] == N_POSES - K_BAD
            and res["support"] - res["support_of_best_other_mask"] >= 2
            and res["tie_break_gap"] is not None and res["tie_break_gap"] >= 1e-6
            and res["consensus_max_abs_dT_vs_ground_truth"] < res["plain_max_abs_dT_vs_ground_truth"])


def main():
    import oracle
    oracle.build()
    for seed in range(16):
        res = oracle_pipeline(oracle, seed)
        ok = separates(res)
        print(f"seed {seed}: best row {res['best']}, support {res['support']} (best other mask {res['support_of_best_other_mask']}), "
              f"tie-break gap {res['tie_break_gap']:.3e} over {res['candidates_tied_on_support']} tied, plain |dT| "
              f"{res['plain_max_abs_dT_vs_ground_truth']:.3e}, consensus |dT| {res['consensus_max_abs_dT_vs_ground_truth']:.3e}, "
              f"rms clean <= {res['rms_at_refit_clean_max']:.4f}, bad >= {res['rms_at_refit_bad_min']:.4f}: "
              f"{'separates' if ok else 'does NOT separate'}")
        if ok:
            if "--write" in sys.argv:
                with open(FIXTURE, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")
                print("wrote", FIXTURE)
            return 0
    print("no seed separates: the scenario itself has to change")
    return 1


if __name__ == "__main__":
    sys.exit(main())
