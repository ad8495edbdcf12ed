"""clc_solve_subsets against the two routes it is measured against (profiles/subset_solves.md):
  (a) the route without it — host materialize + clc_upload_batched + clc_solve_batched of the same S sub-problems — whole route and
      solve alone;
  (b) clc_solve_multistart of S copies of the start on the full problem (the same S workgroups, unweighted).
S bootstrap rows on a 50 x 100 problem.  Warm-up calls first, then `--reps` timed calls of each leg, interleaved; medians and the
min-max spread of host wall time, and of the kernel's event time (profile_events = 1) in a second round.  Prints one JSON line."""
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
    ap.add_argument("--subsets", type=int, default=1024)
    ap.add_argument("--poses", type=int, default=50)
    ap.add_argument("--points", type=int, default=100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    S, P = a.subsets, a.poses
    obs = sd.sim_fixed_count(7, P, a.points, noise_sigma=0.01)
    rec = clc.flatten_observations(obs, False, False)
    off = clc.calib.pose_block_offsets(obs, False, False)
    one = np.array([0, rec.shape[0]], dtype=np.int64)
    W = resample.bootstrap_weights(P, S, 3)
    out = {"subsets": S, "poses": P, "points": a.points, "records": int(rec.shape[0]), "weight_bytes": int(W.nbytes)}
    with clc.Solver(0) as s, clc.Solver(0) as sb:
        x_true = sd.pose7_from_T(sd.tlc_to_tcl(sd.GT_RLC, sd.GT_TLC))
        x0 = s.pose_plus(x_true[None], np.array([[.02, -.02, .01, .01, -.01, .02]]))[0]
        starts = np.tile(x0, (S, 1))
        s.upload_batched(rec, one)

        def materialised():
            subs = [resample.materialize(rec, off, w) for w in W]
            boff = np.zeros(S + 1, dtype=np.int64)
            boff[1:] = np.cumsum([r.shape[0] for r in subs])
            return np.concatenate(subs), boff

        def route():
            t0 = time.perf_counter()
            big, boff = materialised()
            t1 = time.perf_counter()
            sb.upload_batched(big, boff)
            t2 = time.perf_counter()
            p, sm = sb.solve_batched(starts)
            t3 = time.perf_counter()
            return p, sm, (t3 - t0, t1 - t0, t2 - t1, t3 - t2)

        pr, smr, _ = route()
        out["materialised_bytes"] = int(sum(int(w.astype(np.int64).sum()) for w in W) * a.points * 64)
        ps, sms = s.solve_subsets(off, W, x0)
        out["agreement_max_dT"] = float(max(np.abs(sd.T_from_pose7(ps[k]) - sd.T_from_pose7(pr[k])).max() for k in range(S)))
        out["iterations"] = sorted({int(m.num_iterations) for m in sms})
        for opt_name, o in (("wall", None), ("kernel", "events")):
            opt = clc.default_options()
            if o:
                opt.profile_events = 1
            legs = {"subsets": [], "multistart": [], "batched_solve": []}
            kern = {"subsets": [], "multistart": [], "batched_solve": []}
            whole, mat, upl = [], [], []
            for i in range(a.warmup + a.reps):
                t = time.perf_counter(); _, m1 = s.solve_subsets(off, W, x0, opt); d1 = time.perf_counter() - t
                t = time.perf_counter(); _, m2 = s.solve_multistart(starts, opt); d2 = time.perf_counter() - t
                t = time.perf_counter(); _, m3 = sb.solve_batched(starts, opt); d3 = time.perf_counter() - t
                if i < a.warmup:
                    continue
                legs["subsets"].append(d1); legs["multistart"].append(d2); legs["batched_solve"].append(d3)
                kern["subsets"].append(m1[0].eval_kernel_ms * 1e-3); kern["multistart"].append(m2[0].eval_kernel_ms * 1e-3)
                kern["batched_solve"].append(m3[0].eval_kernel_ms * 1e-3)
            out[opt_name] = {k: stats(v) for k, v in (kern if o else legs).items()}
        for i in range(2 + max(3, a.reps // 5)):   # the whole route is slow (hundreds of ms of host work): fewer repetitions
            _, _, (tw, tm, tu, tsv) = route()
            if i >= 2:
                whole.append(tw); mat.append(tm); upl.append(tu)
        out["route_whole"] = stats(whole)
        out["route_materialize"] = stats(mat)
        out["route_upload"] = stats(upl)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
