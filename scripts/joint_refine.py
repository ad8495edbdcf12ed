"""K18 joint refinement: warm device time of clc_joint_refine_device beside the host route (scipy.optimize.least_squares on the
restatement tests/joint_ref.py) for the same problems in the same run, and the distance of T_cl to the truth after the two-stage
route and after the joint one on seeded sets.  Writes profiles/joint_refine.md.

  python scripts/joint_refine.py [repeats=5] [batch=1024] [accuracy_seeds=20]

Needs the GPU (torch for the device arrays) and scipy."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_cases as cases  # noqa: E402
import joint_ref as ref  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402

NAME = "radtan"


def timed_device(sv, cam, a, q0, t0, repeats):
    """clc_joint_refine_device on device arrays, fresh start poses every call -> (ms list, result of the last call)."""
    import torch
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    n, npb = len(a["coff"]) - 1, len(a["prob_off"]) - 1
    dc, db, dp, dco, dpo, dpr = up(a["corners"]), up(a["board"]), up(a["pts"]), up(a["coff"]), up(a["poff"]), up(a["prob_off"])
    q_in, t_in, cl_in = up(q0), up(t0), up(a["poses_cl0"])
    dst = torch.zeros(n, dtype=torch.int32, device=dev)
    dsm = torch.zeros(npb * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev)
    dH = torch.zeros((npb, 36), dtype=torch.float64, device=dev)
    ms = []
    for _ in range(repeats + 1):  # the first call warms
        dq, dt, dcl = q_in.clone(), t_in.clone(), cl_in.clone()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        sv.joint_refine_device(cam, dc.data_ptr(), db.data_ptr(), dco.data_ptr(), dp.data_ptr(), dpo.data_ptr(), n, npb, dq.data_ptr(),
                               dt.data_ptr(), dcl.data_ptr(), dsm.data_ptr(), dst.data_ptr(), problem_offsets_ptr=dpr.data_ptr(),
                               H_cl_ptr=dH.data_ptr())
        ms.append((time.perf_counter() - t1) * 1e3)
    sm = (_capi.Summary * npb).from_buffer_copy(dsm.cpu().numpy().tobytes())
    return ms[1:], dict(q=dq.cpu().numpy(), t=dt.cpu().numpy(), poses_cl=dcl.cpu().numpy(), summaries=sm)


def host_route(sv, cam, a, k, q0, t0, jo):
    """scipy on the restatement for problem k from the same start -> (seconds, cost)."""
    lifted = sv.camera_lift(cam, a["corners"]).astype(np.float32).astype(np.float64)
    idx = range(a["prob_off"][k], a["prob_off"][k + 1])
    prob = dict(lifted=[lifted[a["coff"][i]:a["coff"][i + 1]] for i in idx],
                board=[a["board"][a["coff"][i]:a["coff"][i + 1]].astype(np.float64) for i in idx],
                pts=[a["pts"][a["poff"][i]:a["poff"][i + 1]] for i in idx], sc=jo.sigma_corner, sl=jo.sigma_laser)
    start = ([ref.quat_wxyz_to_R(q0[i]) for i in idx], [t0[i].copy() for i in idx], *ref.pose7_to_Rt(a["poses_cl0"][k]))
    t1 = time.perf_counter()
    out = ref.solve(prob, *start, rounds=1)
    return time.perf_counter() - t1, out[4]


def rot_angle(Ra, Rb):
    return float(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1)))


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n_batch = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    n_seeds = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    cam = cases.CAMERAS[NAME]
    lines = []
    with clc.Solver(0) as sv:
        jo = _capi.default_joint_options(cam)
        # ---- one problem of 100 images x (144 corners + 100 points) ----
        a1 = cases.arrays([cases.problem(NAME, 900, 100, 144, 100)])
        q1, t1, _, st, _ = sv.board_poses(cam, a1["corners"], a1["board"], a1["coff"])
        assert np.all(st == 1)
        ms1, r1 = timed_device(sv, cam, a1, q1, t1, repeats)
        hs1, hc1 = host_route(sv, cam, a1, 0, q1, t1, jo)
        sm = r1["summaries"][0]
        lines.append("| 1 problem, 100 images x (144 corners + 100 points) | %.3f (%.3f – %.3f) | %d | %.1f | %.2e |" % (
            np.median(ms1), min(ms1), max(ms1), sm.num_iterations, hs1 * 1e3, abs(sm.final_cost - hc1) / hc1))
        # ---- n_batch problems of 50 such images: 32 distinct problems, tiled ----
        distinct = [cases.problem(NAME, 1000 + k, 50, 144, 100) for k in range(min(32, n_batch))]
        problems = [distinct[k % len(distinct)] for k in range(n_batch)]
        ab = cases.arrays(problems)
        qb, tb, _, st, _ = sv.board_poses(cam, ab["corners"], ab["board"], ab["coff"])
        assert np.all(st == 1)
        msb, rb = timed_device(sv, cam, ab, qb, tb, repeats)
        hb = [host_route(sv, cam, ab, k, qb, tb, jo) for k in range(2)]
        its = [rb["summaries"][k].num_iterations for k in range(n_batch)]
        term = np.bincount([rb["summaries"][k].termination for k in range(n_batch)], minlength=7)
        gap = max(abs(rb["summaries"][k].final_cost - hb[k][1]) / hb[k][1] for k in range(2))
        lines.append("| %d problems of 50 such images (32 distinct, tiled) | %.3f (%.3f – %.3f) | %d – %d | %.1f per problem (2 timed) = %.0f s for all | %.2e |" % (
            n_batch, np.median(msb), min(msb), max(msb), min(its), max(its), np.mean([h[0] for h in hb]) * 1e3,
            np.mean([h[0] for h in hb]) * n_batch, gap))
        # ---- accuracy: T_cl against the truth, two-stage and joint, 30 images ----
        hold = _capi.default_joint_options(cam)
        hold.hold_board_poses = 1
        rows = []
        for seed in range(n_seeds):
            p = cases.problem(NAME, 2000 + seed, 30, 144, 100)
            a = cases.arrays([p])
            q0, t0, _, st, _ = sv.board_poses(cam, a["corners"], a["board"], a["coff"])
            truth_R, truth_t = ref.pose7_to_Rt(p["pose_cl_true"])
            row = []
            for j in (hold, jo):
                r = sv.joint_refine(cam, a["corners"], a["board"], a["coff"], a["pts"], a["poff"], q0, t0, a["poses_cl0"], joint=j)
                R, t = ref.pose7_to_Rt(r["poses_cl"][0])
                row += [np.linalg.norm(t - truth_t) * 1e3, np.degrees(rot_angle(R, truth_R))]
            rows.append(row)
        rows = np.array(rows)
    out = os.path.join(ROOT, "profiles", "joint_refine.md")
    with open(out, "w") as f:
        f.write("# K18 joint refinement of board poses and T_cl — timing and accuracy (MI355X)\n\n")
        f.write("`python scripts/joint_refine.py %d %d %d`: camera `%s`, 0.3 px and 0.01 m of noise, start poses from `clc_board_poses`, T_cl from a "
                "perturbed truth; device arrays, `clc_joint_refine_device` with the default options (H_cl requested), warmed once; median of %d "
                "(min – max), each call ending in its stream synchronise.  Host route: `scipy.optimize.least_squares` (trf, analytic dense "
                "Jacobian, tolerances 1e-15, one round) on the restatement `tests/joint_ref.py`, same problems, same start, same run, on the "
                "host's CPU.  No time gate was set.\n\n" % (repeats, n_batch, n_seeds, NAME, repeats))
        f.write("| problems | device ms | LM iterations | host route ms | relative cost gap device / host |\n|---|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n\n")
        f.write("Terminations of the batch (gradient, parameter, function, radius, no convergence, failure): %s.\n\n" % [int(v) for v in term[1:]])
        f.write("## T_cl against the truth: two-stage and joint\n\n")
        f.write("%d seeded sets of 30 images x (144 corners + 100 points), 0.3 px, 0.01 m.  Two-stage: the board poses of `clc_board_poses` frozen, "
                "T_cl from the laser points (`hold_board_poses = 1`, which tests/test_gpu_joint.py holds to `clc_solve` on the records).  Joint: "
                "everything free.  Reported whatever it shows.\n\n" % n_seeds)
        f.write("| route | translation error mm: mean / median / max | rotation error degrees: mean / median / max |\n|---|---|---|\n")
        for nm, c in (("two-stage", 0), ("joint", 2)):
            f.write("| %s | %.3f / %.3f / %.3f | %.4f / %.4f / %.4f |\n" % (nm, rows[:, c].mean(), np.median(rows[:, c]), rows[:, c].max(),
                                                                         rows[:, c + 1].mean(), np.median(rows[:, c + 1]), rows[:, c + 1].max()))
        f.write("\nJoint nearer the truth in translation on %d of %d sets, in rotation on %d of %d.\n" % (
            (rows[:, 2] < rows[:, 0]).sum(), n_seeds, (rows[:, 3] < rows[:, 1]).sum(), n_seeds))
    print(open(out).read())


if __name__ == "__main__":
    main()
