"""clc_score_blocks against the two routes it is measured against (profiles/consensus.md):
  (i)  the route it replaces — one clc_factor_evaluate per candidate (N residuals over PCIe each) + numpy grouping by block;
  (ii) clc_solve_multistart of the same candidates on the same upload: the same workgroups on the same layout, plus an LM controller.
S candidates (the solutions of S random 5-of-P subsets) on a P x points problem.  Warm-up calls first, then `--reps` timed calls of
each leg, interleaved; medians with min / max of host wall time.  Kernel times: run this script under
`rocprofv3 --kernel-trace --stats` (block_scores_kernel, resident_solve_kernel) — clc_score_blocks has no summary to report an event
pair in; the multi-start leg also reports its own event pair (profile_events = 1).
Then the whole consensus calibration, split by step.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import resample, simdata as sd  # noqa: E402


def stats(v):
    v = np.asarray(v) * 1e3
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=1024)
    ap.add_argument("--poses", type=int, default=50)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--route-reps", type=int, default=5)
    a = ap.parse_args()
    S, P = a.candidates, a.poses
    obs = sd.sim_fixed_count(7, P, a.points, noise_sigma=0.01)
    rec = clc.flatten_observations(obs, False, False)
    off = clc.calib.pose_block_offsets(obs, False, False)
    one = np.array([0, rec.shape[0]], dtype=np.int64)
    W = resample.random_subset_weights(P, S, 5, 0)
    out = {"candidates": S, "poses": P, "points": a.points, "records": int(rec.shape[0]),
           "table_bytes": int(S * P * 20), "route_residual_bytes": int(S * rec.shape[0] * 8)}
    with clc.Solver(0) as s, clc.Solver(0) as sf:
        x_true = sd.pose7_from_T(sd.tlc_to_tcl(sd.GT_RLC, sd.GT_TLC))
        x0 = s.pose_plus(x_true[None], np.array([[.02, -.02, .01, .01, -.01, .02]]))[0]
        s.upload_batched(rec, one)
        sf.upload(rec)
        cands, _ = s.solve_subsets(off, W, x0)
        tau = 0.03

        def route():
            q = np.empty((S, P))
            for k in range(S):
                r, _ = sf.factor_evaluate(cands[k], want_jacobian=False)
                q[k] = np.add.reduceat(r * r, off[:-1])
            return q

        q_route = route()
        q, _, _ = s.score_blocks(off, cands, tau)
        out["agreement_max_rel"] = float(np.max(np.abs(q - q_route) / q_route))
        opt = clc.default_options()
        opt.profile_events = 1
        legs = {"score_blocks": [], "multistart": []}
        ms_kernel, iters = [], set()
        for i in range(a.warmup + a.reps):
            t = time.perf_counter(); s.score_blocks(off, cands, tau); d1 = time.perf_counter() - t
            t = time.perf_counter(); _, m2 = s.solve_multistart(cands.copy(), opt); d2 = time.perf_counter() - t
            if i < a.warmup:
                continue
            legs["score_blocks"].append(d1); legs["multistart"].append(d2)
            ms_kernel.append(m2[0].eval_kernel_ms * 1e-3)
            iters |= {int(m.num_iterations) for m in m2}
        out["wall"] = {k: stats(v) for k, v in legs.items()}
        out["multistart_kernel_events"] = stats(ms_kernel)
        out["multistart_iterations"] = sorted(iters)
        whole = []
        for i in range(1 + a.route_reps):   # the replaced route: S synchronous calls per repetition
            t = time.perf_counter(); route(); d = time.perf_counter() - t
            if i >= 1:
                whole.append(d)
        out["route_factor_evaluate"] = stats(whole)
        # the consensus calibration, step by step (what clc.CamLaserCalibrationConsensus does), n = 256 rows
        Wc = resample.random_subset_weights(P, 256, 5, 0)
        steps = {k: [] for k in ("upload", "solve_subsets", "score_blocks", "select", "refit", "score_refit", "whole_call")}
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter(); s.upload_batched(rec, one)
            t1 = time.perf_counter(); c, _ = s.solve_subsets(off, Wc, x0)
            t2 = time.perf_counter(); qq, _, _ = s.score_blocks(off, c, tau)
            t3 = time.perf_counter(); best, mask, _ = resample.consensus_select(qq, tau)
            t4 = time.perf_counter(); rf, _ = s.solve_subsets(off, mask.astype(np.uint8)[None], c[best])
            t5 = time.perf_counter(); s.score_blocks(off, rf, tau)
            t6 = time.perf_counter()
            T = sd.T_from_pose7(x0)
            clc.CamLaserCalibrationConsensus(obs, T, False, False, n=256, m=5, rms_max=tau, seed=0, solver=s)
            t7 = time.perf_counter()
            if i < a.warmup:
                continue
            for k, d in zip(steps, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t6 - t5, t7 - t6)):
                steps[k].append(d)
        out["consensus_steps"] = {k: stats(v) for k, v in steps.items()}
        out["consensus_support"] = int(mask.sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
