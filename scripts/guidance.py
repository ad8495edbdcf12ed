"""K20 pose guidance: warm device time of clc_score_board_poses_device (10^4 and 10^5 candidates x 1 081 rays) and of
clc_select_board_poses_device (k = 10 of 10^5) on device arrays, beside the numpy restatement tests/guidance_ref.py on the same inputs
in the same run; the cast with the direction table against the cast with a sincos per ray, and the two mappings of the score stage
(hooks build).  Medians of `repeats` warm calls, each a host clock around a call that ends in a stream synchronisation.  Writes
profiles/guidance.md.

  python scripts/guidance.py [repeats=5] [out=profiles/guidance.md] [sizes=10000,100000]

Needs the GPU (torch for the device arrays)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guidance_cases as cases  # noqa: E402
import guidance_ref as ref  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import simdata  # noqa: E402

K = 10


def med(f, repeats):
    f()  # warms
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    import torch
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "guidance.md")
    sizes = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [10000, 100000]
    if not torch.cuda.is_available():
        raise SystemExit("scripts/guidance.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    case = cases.degenerate("only_pitch")
    pose, H0, model = case["pose_cl"], case["H0"], case["model"]
    sv = clc.Solver(library="hooks")
    name, cus = sv.device_info()
    set_dirs = sv._hook("clc_debug_guidance_dirs")
    lines = ["# K20 pose guidance: device time beside the numpy restatement", "",
             f"`python scripts/guidance.py {repeats}` on {name} ({cus} CUs).  Device arrays; a time is the median (min - max) of {repeats} warm calls,",
             "each a host clock around one call that ends in its stream synchronisation.  The restatement (tests/guidance_ref.py, one",
             "process, one thread of numpy) runs once on the same inputs in the same run.  1 081 rays, the defaults of",
             "`clc_guidance_options_default`, H0 of `sim_degenerate(\"only_pitch\")`.", "",
             "| call | candidates | device ms | restatement s | ratio | agree |", "|---|---|---|---|---|---|"]
    cast_lines = ["", "## The ray directions: table against a sincos per ray", "",
                  "`clc_score_board_poses_device` with n_hits and H_add only (the direction kernel and the cast, no score), alternating the two forms:", "",
                  "| candidates | table ms | sincos per ray ms |", "|---|---|---|"]
    rows_lines = ["", "## The score stage: one candidate per lane against one matrix row per lane", "",
                  "The whole `clc_score_board_poses_device` call (cast included), alternating the two mappings of the 6x6 eigenvalue stage:", "",
                  "| candidates | one candidate per lane ms | one wave per candidate ms | same bits |", "|---|---|---|---|"]
    rows_ms = {}
    set_rows = sv._hook("clc_debug_guidance_score_rows")
    for n in sizes:
        q, t = simdata.candidate_board_poses(7, n, cases.TCL)
        dq, dt = torch.from_numpy(q).to(dev), torch.from_numpy(np.ascontiguousarray(t)).to(dev)
        nh = torch.zeros(n, dtype=torch.int32, device=dev)
        Ha = torch.zeros((n, 36), dtype=torch.float64, device=dev)
        e = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        s = torch.zeros(n, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        score = lambda: sv.score_board_poses_device(pose, n, dq.data_ptr(), dt.data_ptr(), nh.data_ptr(), Ha.data_ptr(), e.data_ptr(), s.data_ptr(), H0)
        cast = lambda: sv.score_board_poses_device(pose, n, dq.data_ptr(), dt.data_ptr(), nh.data_ptr(), Ha.data_ptr())
        m = med(score, repeats)
        t0 = time.perf_counter()
        r = ref.score_all(model, pose, H0, q, t)
        t_ref = time.perf_counter() - t0
        agree = bool(np.array_equal(nh.cpu().numpy(), r["n_hits"])) and float(np.abs(s.cpu().numpy() - r["score"]).max()) < 1e-5
        lines.append(f"| score | {n} | {m[0]:.3f} ({m[1]:.3f} - {m[2]:.3f}) | {t_ref:.2f} | {t_ref * 1e3 / m[0]:.0f}x | {'yes' if agree else 'NO'} |")
        print(lines[-1], flush=True)
        res = {}
        for _ in range(2):  # alternating
            for table in (1, 0):
                set_dirs(table)
                res.setdefault(table, []).append(med(cast, repeats)[0])
        set_dirs(1)
        want = (e.cpu().numpy(), s.cpu().numpy())
        for _ in range(2):
            for rows in (0, 1):
                set_rows(rows)
                rows_ms.setdefault((n, rows), []).append(med(score, repeats)[0])
        same = bool(np.array_equal(e.cpu().numpy(), want[0]) and np.array_equal(s.cpu().numpy(), want[1]))  # (the row-per-lane form ran last)
        set_rows(0)
        rows_lines.append(f"| {n} | {min(rows_ms[(n, 0)]):.3f} | {min(rows_ms[(n, 1)]):.3f} | {'yes' if same else 'NO'} |")
        print(rows_lines[-1], flush=True)
        cast_lines.append(f"| {n} | {min(res[1]):.3f} | {min(res[0]):.3f} |")
        print(cast_lines[-1], flush=True)
        if n == max(sizes):
            sel = {}
            m = med(lambda: sel.update(sv.select_board_poses_device(pose, n, dq.data_ptr(), dt.data_ptr(), K, H0)), repeats)
            t0 = time.perf_counter()
            g = ref.greedy(model, H0, r["n_hits"], r["H_add"], K)
            t_g = time.perf_counter() - t0
            agree = bool(np.array_equal(sel["chosen"], g["chosen"]))
            lines.append(f"| select k = {K} (cast included) | {n} | {m[0]:.3f} ({m[1]:.3f} - {m[2]:.3f}) | {t_ref + t_g:.2f} | "
                         f"{(t_ref + t_g) * 1e3 / m[0]:.0f}x | {'yes' if agree else 'NO'} (smallest round gap {min(g['gaps']):.1e}) |")
            print(lines[-1], flush=True)
    text = "\n".join(lines + cast_lines + rows_lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
