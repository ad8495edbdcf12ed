"""K21, the joint refinement with the scanner's range offset and scale: warm device time of clc_joint_refine_range_device beside
clc_joint_refine_device on the same problems in the same run, and on seeded sets with a planted offset and scale the error of T_cl
with K18 alone and with K21, and the recovered b, kappa against their predicted 1 sigma.  Writes the timing and accuracy part of
profiles/laser_range.md.

  python scripts/laser_range.py [repeats=5] [batch=1024] [accuracy_seeds=20] [out=profiles/laser_range.md]

Needs the GPU (torch for the device arrays)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_ref as jref  # noqa: E402
import laserrange_cases as cases  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402

NAME = "radtan"
PLANTED = (0.02, 0.005)


def timed_pair(sv, cam, a, q0, t0, repeats):
    """clc_joint_refine_device and clc_joint_refine_range_device on the same device arrays, alternating, fresh start poses every call
    -> (ms of K18, ms of K21, summaries of the last K18 call, of the last K21 call)."""
    import torch
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    n, npb = len(a["coff"]) - 1, len(a["prob_off"]) - 1
    dc, db, dp, dco, dpo, dpr = up(a["corners"]), up(a["board"]), up(a["pts"]), up(a["coff"]), up(a["poff"]), up(a["prob_off"])
    q_in, t_in, cl_in = up(q0), up(t0), up(a["poses_cl0"])
    dst = torch.zeros(n, dtype=torch.int32, device=dev)
    dsm = [torch.zeros(npb * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev) for _ in range(2)]
    dH = torch.zeros((npb, 64), dtype=torch.float64, device=dev)
    ms = ([], [])
    for _ in range(repeats + 1):  # the first pair warms
        for which in (0, 1):
            dq, dt, dcl = q_in.clone(), t_in.clone(), cl_in.clone()
            drg = torch.zeros((npb, 2), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if which == 0:
                sv.joint_refine_device(cam, dc.data_ptr(), db.data_ptr(), dco.data_ptr(), dp.data_ptr(), dpo.data_ptr(), n, npb,
                                       dq.data_ptr(), dt.data_ptr(), dcl.data_ptr(), dsm[0].data_ptr(), dst.data_ptr(),
                                       problem_offsets_ptr=dpr.data_ptr(), H_cl_ptr=dH.data_ptr())
            else:
                sv.joint_refine_range_device(cam, dc.data_ptr(), db.data_ptr(), dco.data_ptr(), dp.data_ptr(), dpo.data_ptr(), n, npb,
                                             dq.data_ptr(), dt.data_ptr(), dcl.data_ptr(), drg.data_ptr(), dsm[1].data_ptr(), dst.data_ptr(),
                                             problem_offsets_ptr=dpr.data_ptr(), H_cr_ptr=dH.data_ptr())
            ms[which].append((time.perf_counter() - t1) * 1e3)
    sms = [(_capi.Summary * npb).from_buffer_copy(d.cpu().numpy().tobytes()) for d in dsm]
    return ms[0][1:], ms[1][1:], sms[0], sms[1]


def rot_angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n_batch = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    n_seeds = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "laser_range.md")
    cam = cases.CAMERAS[NAME]
    lines = []
    with clc.Solver(0) as sv:
        # ---- one problem of 100 images x (144 corners + 100 points) ----
        a1 = cases.arrays([cases.problem(NAME, 900, 100, 144, 100, offset=PLANTED[0], scale=PLANTED[1])])
        q1, t1, _, st, _ = sv.board_poses(cam, a1["corners"], a1["board"], a1["coff"])
        assert np.all(st == 1)
        k18, k21, s18, s21 = timed_pair(sv, cam, a1, q1, t1, repeats)
        lines.append("| 1 problem, 100 images x (144 corners + 100 points) | %.3f (%.3f – %.3f) | %d | %.3f (%.3f – %.3f) | %d | %.2f |" % (
            np.median(k18), min(k18), max(k18), s18[0].num_iterations, np.median(k21), min(k21), max(k21), s21[0].num_iterations,
            np.median(k21) / np.median(k18)))
        # ---- n_batch problems of 50 such images: 32 distinct problems, tiled ----
        distinct = [cases.problem(NAME, 1000 + k, 50, 144, 100, offset=PLANTED[0], scale=PLANTED[1]) for k in range(min(32, n_batch))]
        ab = cases.arrays([distinct[k % len(distinct)] for k in range(n_batch)])
        qb, tb, _, st, _ = sv.board_poses(cam, ab["corners"], ab["board"], ab["coff"])
        assert np.all(st == 1)
        k18, k21, s18, s21 = timed_pair(sv, cam, ab, qb, tb, repeats)
        it18 = [s18[k].num_iterations for k in range(n_batch)]
        it21 = [s21[k].num_iterations for k in range(n_batch)]
        lines.append("| %d problems of 50 such images (32 distinct, tiled) | %.3f (%.3f – %.3f) | %d – %d | %.3f (%.3f – %.3f) | %d – %d | %.2f |" % (
            n_batch, np.median(k18), min(k18), max(k18), min(it18), max(it18), np.median(k21), min(k21), max(k21), min(it21), max(it21),
            np.median(k21) / np.median(k18)))
        term = np.bincount([s21[k].termination for k in range(n_batch)], minlength=7)
        # ---- accuracy: T_cl against the truth with K18 alone and with K21, 30 images, planted offset and scale ----
        rows = []
        for seed in range(n_seeds):
            p = cases.problem(NAME, 2000 + seed, 30, 144, 100, offset=PLANTED[0], scale=PLANTED[1])
            a = cases.arrays([p])
            q0, t0, _, st, _ = sv.board_poses(cam, a["corners"], a["board"], a["coff"])
            truth_R, truth_t = jref.pose7_to_Rt(p["pose_cl_true"])
            r18 = sv.joint_refine(cam, a["corners"], a["board"], a["coff"], a["pts"], a["poff"], q0, t0, a["poses_cl0"])
            r21 = sv.joint_refine_range(cam, a["corners"], a["board"], a["coff"], a["pts"], a["poff"], q0, t0, a["poses_cl0"])
            row = []
            for r in (r18, r21):
                R, t = jref.pose7_to_Rt(r["poses_cl"][0])
                row += [np.linalg.norm(t - truth_t) * 1e3, np.degrees(rot_angle(R, truth_R))]
            sig = np.sqrt(np.diag(np.linalg.inv(r21["H_cr"][0])))
            row += [r21["range"][0][0], sig[6], r21["range"][0][1], sig[7]]
            rows.append(row)
        rows = np.array(rows)
    with open(out, "w") as f:
        f.write("## Timing: K21 beside K18 on the same problems (MI355X)\n\n")
        f.write("`python scripts/laser_range.py %d %d %d`: camera `%s`, 0.3 px and 0.01 m of noise, a planted offset of %.3f m and scale of "
                "%.3f, start poses from `clc_board_poses`, T_cl from a perturbed truth, range start (0, 0); device arrays, "
                "`clc_joint_refine_device` and `clc_joint_refine_range_device` alternating on the same arrays with the default options "
                "(H requested), one pair to warm; median of %d (min – max), each call ending in its stream synchronise (wall clock around "
                "the call, so the read of the offsets' ends and the lift are inside both).  K18 has no parameter for the planted error "
                "and ends at another point, so the iteration counts differ.  No time gate was set.\n\n" % (
                    repeats, n_batch, n_seeds, NAME, PLANTED[0], PLANTED[1], repeats))
        f.write("| problems | K18 ms | K18 LM iterations | K21 ms | K21 LM iterations | K21 / K18 |\n|---|---|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n\n")
        f.write("Terminations of the K21 batch (gradient, parameter, function, radius, no convergence, failure): %s.\n\n" % [int(v) for v in term[1:]])
        f.write("## T_cl against the truth with a planted offset and scale: K18 alone and K21\n\n")
        f.write("%d seeded sets of 30 images x (144 corners + 100 points), 0.3 px, 0.01 m, planted %.3f m and %.3f.  K18: `clc_joint_refine` "
                "on the points as measured.  K21: `clc_joint_refine_range`, everything free, start (0, 0).  Reported whatever it shows.\n\n" % (
                    n_seeds, PLANTED[0], PLANTED[1]))
        f.write("| route | translation error mm: mean / median / max | rotation error degrees: mean / median / max |\n|---|---|---|\n")
        for nm, c in (("K18", 0), ("K21", 2)):
            f.write("| %s | %.3f / %.3f / %.3f | %.4f / %.4f / %.4f |\n" % (nm, rows[:, c].mean(), np.median(rows[:, c]), rows[:, c].max(),
                                                                         rows[:, c + 1].mean(), np.median(rows[:, c + 1]), rows[:, c + 1].max()))
        f.write("\nK21 nearer the truth in translation on %d of %d sets, in rotation on %d of %d.\n\n" % (
            (rows[:, 2] < rows[:, 0]).sum(), n_seeds, (rows[:, 3] < rows[:, 1]).sum(), n_seeds))
        zb, zk = (rows[:, 4] - PLANTED[0]) / rows[:, 5], (rows[:, 6] - PLANTED[1]) / rows[:, 7]
        f.write("Recovered offset: mean %.4f m, standard deviation over the sets %.4f m; predicted 1 sigma (from H_cr) %.4f – %.4f m; "
                "(b - planted) / sigma: rms %.2f, largest %.2f.\n" % (rows[:, 4].mean(), rows[:, 4].std(), rows[:, 5].min(), rows[:, 5].max(),
                                                                   np.sqrt(np.mean(zb ** 2)), np.abs(zb).max()))
        f.write("Recovered scale: mean %.5f, standard deviation over the sets %.5f; predicted 1 sigma %.5f – %.5f; "
                "(kappa - planted) / sigma: rms %.2f, largest %.2f.\n" % (rows[:, 6].mean(), rows[:, 6].std(), rows[:, 7].min(), rows[:, 7].max(),
                                                                       np.sqrt(np.mean(zk ** 2)), np.abs(zk).max()))
    print(open(out).read())


if __name__ == "__main__":
    main()
