"""K22, the joint refinement under a Cauchy loss per corner and per laser point: warm device time of clc_joint_refine_robust_device
beside clc_joint_refine_device on the same problems in the same run, clean and contaminated, with the iteration counts; and on seeded
sets of 30 images the distance of T_cl from the truth for K18 and K22 on clean and on contaminated data, set by set.  Writes the
timing and recovery part of profiles/joint_robust.md.

  python scripts/joint_robust.py [repeats=5] [batch=1024] [recovery_sets=8] [out=profiles/joint_robust.md]

Needs the GPU (torch for the device arrays)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_cases as jcases  # noqa: E402
import jointrobust_cases as cases  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402

NAME = "radtan"


def timed_pair(sv, cam, a, q0, t0, repeats):
    """clc_joint_refine_device and clc_joint_refine_robust_device (weights requested) on the same device arrays, alternating, fresh
    start poses every call -> (ms of K18, ms of K22, summaries of the last K18 call, of the last K22 call)."""
    import torch
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    n, npb = len(a["coff"]) - 1, len(a["prob_off"]) - 1
    dc, db, dp, dco, dpo, dpr = up(a["corners"]), up(a["board"]), up(a["pts"]), up(a["coff"]), up(a["poff"]), up(a["prob_off"])
    q_in, t_in, cl_in = up(q0), up(t0), up(a["poses_cl0"])
    dst = torch.zeros(n, dtype=torch.int32, device=dev)
    dsm = [torch.zeros(npb * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev) for _ in range(2)]
    dH = torch.zeros((npb, 36), dtype=torch.float64, device=dev)
    dwc = torch.zeros(len(a["corners"]), dtype=torch.float64, device=dev)
    dwl = torch.zeros(len(a["pts"]), dtype=torch.float64, device=dev)
    ms = ([], [])
    for _ in range(repeats + 1):  # the first pair warms
        for which in (0, 1):
            dq, dt, dcl = q_in.clone(), t_in.clone(), cl_in.clone()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if which == 0:
                sv.joint_refine_device(cam, dc.data_ptr(), db.data_ptr(), dco.data_ptr(), dp.data_ptr(), dpo.data_ptr(), n, npb,
                                       dq.data_ptr(), dt.data_ptr(), dcl.data_ptr(), dsm[0].data_ptr(), dst.data_ptr(),
                                       problem_offsets_ptr=dpr.data_ptr(), H_cl_ptr=dH.data_ptr())
            else:
                sv.joint_refine_robust_device(cam, dc.data_ptr(), db.data_ptr(), dco.data_ptr(), dp.data_ptr(), dpo.data_ptr(), n, npb,
                                              dq.data_ptr(), dt.data_ptr(), dcl.data_ptr(), dsm[1].data_ptr(), dst.data_ptr(),
                                              problem_offsets_ptr=dpr.data_ptr(), H_cl_ptr=dH.data_ptr(), w_corner_ptr=dwc.data_ptr(),
                                              w_laser_ptr=dwl.data_ptr())
            ms[which].append((time.perf_counter() - t1) * 1e3)
    sms = [(_capi.Summary * npb).from_buffer_copy(d.cpu().numpy().tobytes()) for d in dsm]
    return ms[0][1:], ms[1][1:], sms[0], sms[1]


def its(sm, n):
    v = [sm[k].num_iterations for k in range(n)]
    return "%d" % v[0] if n == 1 else "%d – %d (median %d)" % (min(v), max(v), int(np.median(v)))


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n_batch = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    n_sets = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "joint_robust.md")
    cam = jcases.CAMERAS[NAME]
    lines, terms = [], []
    with clc.Solver(0) as sv:
        one = jcases.problem(NAME, 900, 100, 144, 100)
        distinct = [jcases.problem(NAME, 1000 + k, 50, 144, 100) for k in range(min(32, n_batch))]
        for label, dirty in (("clean", False), ("contaminated", True)):
            rng = np.random.default_rng(31)
            # ---- one problem of 100 images x (144 corners + 100 points) ----
            a1 = jcases.arrays([cases.contaminate(one, rng) if dirty else one])
            q1, t1, _, st, _ = sv.board_poses(cam, a1["corners"], a1["board"], a1["coff"])
            assert np.all(st == 1)
            k18, k22, s18, s22 = timed_pair(sv, cam, a1, q1, t1, repeats)
            lines.append("| 1 problem, 100 images x (144 corners + 100 points), %s | %.3f (%.3f – %.3f) | %s | %.3f (%.3f – %.3f) | %s | %.2f |" % (
                label, np.median(k18), min(k18), max(k18), its(s18, 1), np.median(k22), min(k22), max(k22), its(s22, 1),
                np.median(k22) / np.median(k18)))
            # ---- n_batch problems of 50 such images: 32 distinct problems, tiled ----
            dd = [cases.contaminate(p, rng) for p in distinct] if dirty else distinct
            ab = jcases.arrays([dd[k % len(dd)] for k in range(n_batch)])
            qb, tb, _, st, _ = sv.board_poses(cam, ab["corners"], ab["board"], ab["coff"])
            assert np.all(st == 1)
            k18, k22, s18, s22 = timed_pair(sv, cam, ab, qb, tb, repeats)
            lines.append("| %d problems of 50 such images (32 distinct, tiled), %s | %.3f (%.3f – %.3f) | %s | %.3f (%.3f – %.3f) | %s | %.2f |" % (
                n_batch, label, np.median(k18), min(k18), max(k18), its(s18, n_batch), np.median(k22), min(k22), max(k22), its(s22, n_batch),
                np.median(k22) / np.median(k18)))
            terms.append((label, [int(v) for v in np.bincount([s22[k].termination for k in range(n_batch)], minlength=7)[1:]]))
        # ---- recovery: |t_cl - truth| for K18 and K22 on clean and contaminated data, set by set ----
        rows = []
        for k, (clean, dirty) in enumerate(cases.recovery_sets(NAME, n_sets)):
            row = [k]
            sep = None
            for p in (clean, dirty):
                a = jcases.arrays([p])
                q0, t0, _, st, _ = sv.board_poses(cam, a["corners"], a["board"], a["coff"])
                r18 = sv.joint_refine(cam, a["corners"], a["board"], a["coff"], a["pts"], a["poff"], q0, t0, a["poses_cl0"])
                r22 = sv.joint_refine_robust(cam, a["corners"], a["board"], a["coff"], a["pts"], a["poff"], q0, t0, a["poses_cl0"])
                row += [1e3 * cases.tcl_distance(r18["poses_cl"][0], p["pose_cl_true"]), 1e3 * cases.tcl_distance(r22["poses_cl"][0], p["pose_cl_true"]),
                        r18["summaries"][0].num_iterations, r22["summaries"][0].num_iterations]
                if p is dirty:
                    sep = cases.separation(r22["w_corner"], r22["w_laser"], *cases.planted_masks(p))
            rows.append(row + [sep[0], sep[1]])
    with open(out, "w") as f:
        f.write("## Timing: K22 beside K18 on the same problems (MI355X)\n\n")
        f.write("`python scripts/joint_robust.py %d %d %d`: camera `%s`, 0.3 px and 0.01 m of noise, start poses from `clc_board_poses`, T_cl "
                "from a perturbed truth; contaminated: 10 %% of each image's points pulled 0.10 – 0.30 m towards the scanner, 5 %% of its "
                "corners moved 3 – 10 px (`tests/jointrobust_cases.py`).  Device arrays, `clc_joint_refine_device` and "
                "`clc_joint_refine_robust_device` (default scales, both weight arrays requested) alternating on the same arrays with the "
                "default options (H requested), one pair to warm; median of %d (min – max), each call ending in its stream synchronise "
                "(wall clock around the call, so the read of the offsets' ends, the lift and, for K22, the weights kernel are inside).  "
                "The two costs have different minimisers, so the iteration counts differ.  No time target was set.\n\n" % (
                    repeats, n_batch, n_sets, NAME, repeats))
        f.write("| problems | K18 ms | K18 LM iterations | K22 ms | K22 LM iterations | K22 / K18 |\n|---|---|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n\n")
        for label, term in terms:
            f.write("Terminations of the K22 batch, %s (gradient, parameter, function, radius, no convergence, failure): %s.\n" % (label, term))
        f.write("\n## T_cl against the truth under planted outliers: K18 and K22, set by set (MI355X)\n\n")
        f.write("%d seeded sets of 30 images x (144 corners + 100 points), 0.3 px, 0.01 m; the same sets clean and contaminated "
                "(`jointrobust_cases.recovery_sets`).  |t_cl − truth| in mm; LM iterations in brackets.  The last two columns: at K22's answer "
                "on the contaminated set, whether every planted observation has w < 0.5, and the share of the others with w ≥ 0.5.  No ratio "
                "was fixed in advance.\n\n" % n_sets)
        f.write("| set | K18 clean | K22 clean | K18 contaminated | K22 contaminated | planted all down | others up |\n|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %d | %.2f (%d) | %.2f (%d) | %.2f (%d) | %.2f (%d) | %s | %.3f |\n" % (r[0], r[1], r[3], r[2], r[4], r[5], r[7], r[6], r[8], r[9], r[10]))
        m = np.array([[r[1], r[2], r[5], r[6]] for r in rows]).mean(0)
        f.write("| mean | %.2f | %.2f | %.2f | %.2f | | |\n" % tuple(m))
    print(open(out).read())


if __name__ == "__main__":
    main()
