"""Timing of the batched flow (clc_closed_form_batched -> clc_solve_batched in place -> clc_information_batched) at C3
(sim_batch(4242, 1024, 20, 500, 0.01), the bench.py batch) and at the C4 shard size (8 192 problems x 20 scans x 500 points,
simdata.sim_shard_records), against the per-problem single-handle loop the batched calls replace (upload, clc_closed_form,
clc_information per problem).  Prints one JSON line; `python scripts/batched_flow.py [c3|c4|both] [reps]`."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import simdata as sd  # noqa: E402


def _ms(f, reps):
    f()  # warm
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def run(name, rec, off, reps, loop_problems):
    sv = clc.Solver(0)
    sv.upload_batched(rec, off)
    P = len(off) - 1
    poses, _ = sv.batched_buffers()

    def cf():
        sv.closed_form_batched(poses)

    def solve():
        sv.closed_form_batched(poses)  # (every solve starts from the closed form, not from the last result)
        sv.solve_batched_inplace()

    def info():
        sv.information_batched(poses)

    def flow():
        sv.closed_form_batched(poses)
        sv.solve_batched_inplace()
        sv.information_batched(poses)

    out = {"config": name, "problems": P, "observations": int(off[-1])}
    out["closed_form_ms"] = _ms(cf, reps)
    out["closed_form_plus_solve_ms"] = _ms(solve, reps)
    out["solve_ms"] = out["closed_form_plus_solve_ms"] - out["closed_form_ms"]
    out["information_ms"] = _ms(info, reps)
    out["flow_ms"] = _ms(flow, reps)
    # the per-problem loop it replaces, on the first `loop_problems` problems, scaled to P
    one = clc.Solver(0)
    t0 = time.perf_counter()
    for k in range(loop_problems):
        one.upload(rec[off[k]:off[k + 1]])
        T, _, _ = one.closed_form()
        one.information(sd.pose7_from_T(np.linalg.inv(T)))
    loop = (time.perf_counter() - t0) * 1e3
    out["per_problem_loop_ms_measured"] = loop
    out["per_problem_loop_problems"] = loop_problems
    out["per_problem_loop_ms_scaled_to_P"] = loop * P / loop_problems
    one.close()
    sv.close()
    return out


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    res = []
    if which in ("c3", "both"):
        probs, _ = sd.sim_batch(4242, 1024, 20, 500, 0.01)
        recs = [clc.flatten_observations(S, True, False) for S in probs]
        off = np.zeros(len(recs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([r.shape[0] for r in recs])
        res.append(run("C3", np.concatenate(recs), off, reps, 128))
    if which in ("c4", "both"):
        rec, off, _, _ = sd.sim_shard_records(65536, 0, 8192, 20, 500, 0.01)
        res.append(run("C4 shard", rec, off, reps, 128))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
