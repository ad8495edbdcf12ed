"""K23, one robust cost over intrinsics, board poses, T_cl and range: warm device time of clc_calibrate_full_device beside
clc_camera_calibrate_device (K19), clc_joint_refine_range_device (K21) and clc_joint_refine_robust_device (K22) on the same data in
the same run, with the iteration counts; and on seeded sets of 30 images with a planted range error and planted outliers the
distance of T_cl from the truth for K23 against the staged routes, the ratio of T_cl's predicted 1 sigma with the intrinsics free to
that with them held, and the recovered b, kappa and intrinsics against their predicted sigma.  Writes profiles/full_calibration.md.

  python scripts/full_calibration.py [repeats=5] [batch=1024] [recovery_sets=20] [out=profiles/full_calibration.md]

Needs the GPU (torch for the device arrays)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fullcal_cases as cases  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402
from camlasercalibratool_amd.camera import ClcCamera  # noqa: E402

NAME = "radtan"
CALLS = ("K19", "K21", "K22", "K23")


def timed_calls(sv, cam, cams0, a, q0, t0, repeats):
    """The four device calls on the same device arrays, in turn, fresh starts every call -> ({call: [ms]}, {call: summaries})."""
    import torch
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    n, npb = len(a["coff"]) - 1, len(a["prob_off"]) - 1
    dc, db, dp, dco, dpo, dpr = up(a["corners"]), up(a["board"]), up(a["pts"]), up(a["coff"]), up(a["poff"]), up(a["prob_off"])
    q_in, t_in, cl_in, rg_in = up(q0), up(t0), up(a["poses_cl0"]), up(a["range0"])
    cam_in = up(np.frombuffer(bytes((ClcCamera * npb)(*[c.to_c() for c in cams0])), dtype=np.uint8).copy())
    dst = torch.zeros(n, dtype=torch.int32, device=dev)
    dsm = {c: torch.zeros(npb * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev) for c in CALLS}
    dH = torch.zeros((npb, 256), dtype=torch.float64, device=dev)
    dparts, drms = torch.zeros((npb, 2), dtype=torch.float64, device=dev), torch.zeros(npb, dtype=torch.float64, device=dev)
    dwc = torch.zeros(len(a["corners"]), dtype=torch.float64, device=dev)
    dwl = torch.zeros(len(a["pts"]), dtype=torch.float64, device=dev)
    ms = {c: [] for c in CALLS}
    for _ in range(repeats + 1):  # the first round warms
        for which in CALLS:
            dq, dt, dcl, drg, dcam = q_in.clone(), t_in.clone(), cl_in.clone(), rg_in.clone(), cam_in.clone()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if which == "K19":
                sv.camera_calibrate_device(dc.data_ptr(), db.data_ptr(), dco.data_ptr(), n, npb, dcam.data_ptr(), dq.data_ptr(), dt.data_ptr(),
                                           dsm[which].data_ptr(), dst.data_ptr(), problem_offsets_ptr=dpr.data_ptr(), H_cam_ptr=dH.data_ptr(),
                                           rms_ptr=drms.data_ptr())
            elif which == "K21":
                sv.joint_refine_range_device(cam, dc.data_ptr(), db.data_ptr(), dco.data_ptr(), dp.data_ptr(), dpo.data_ptr(), n, npb,
                                             dq.data_ptr(), dt.data_ptr(), dcl.data_ptr(), drg.data_ptr(), dsm[which].data_ptr(), dst.data_ptr(),
                                             problem_offsets_ptr=dpr.data_ptr(), H_cr_ptr=dH.data_ptr())
            elif which == "K22":
                sv.joint_refine_robust_device(cam, dc.data_ptr(), db.data_ptr(), dco.data_ptr(), dp.data_ptr(), dpo.data_ptr(), n, npb,
                                              dq.data_ptr(), dt.data_ptr(), dcl.data_ptr(), dsm[which].data_ptr(), dst.data_ptr(),
                                              problem_offsets_ptr=dpr.data_ptr(), H_cl_ptr=dH.data_ptr(), w_corner_ptr=dwc.data_ptr(),
                                              w_laser_ptr=dwl.data_ptr())
            else:
                sv.calibrate_full_device(dcam.data_ptr(), dc.data_ptr(), db.data_ptr(), dco.data_ptr(), dp.data_ptr(), dpo.data_ptr(), n, npb,
                                         dq.data_ptr(), dt.data_ptr(), dcl.data_ptr(), drg.data_ptr(), dsm[which].data_ptr(), dst.data_ptr(),
                                         problem_offsets_ptr=dpr.data_ptr(), H_full_ptr=dH.data_ptr(), cost_parts_ptr=dparts.data_ptr(),
                                         rms_ptr=drms.data_ptr(), w_corner_ptr=dwc.data_ptr(), w_laser_ptr=dwl.data_ptr())
            ms[which].append((time.perf_counter() - t1) * 1e3)
    sms = {c: (_capi.Summary * npb).from_buffer_copy(dsm[c].cpu().numpy().tobytes()) for c in CALLS}
    return {c: v[1:] for c, v in ms.items()}, sms


def its(sm, n):
    v = [sm[k].num_iterations for k in range(n)]
    return "%d" % v[0] if n == 1 else "%d – %d (median %d)" % (min(v), max(v), int(np.median(v)))


def timing_row(label, ms, sms, n):
    cells = " | ".join("%.3f (%.3f – %.3f) | %s" % (np.median(ms[c]), min(ms[c]), max(ms[c]), its(sms[c], n)) for c in CALLS)
    return "| %s | %s |" % (label, cells)


def sigma_of(H, free):
    out = np.full(16, np.nan)
    out[free] = np.sqrt(np.diag(np.linalg.inv(H[np.ix_(free, free)])))
    return out


def recovery(sv, p, rows, zrows):
    """One recovery set: the staged routes and K23 from the same K19 camera -> a row of |t_cl - truth| in mm; the sigma ratio and the
    z scores of K23 at its defaults and with the scale held."""
    a = cases.arrays([p])
    q, t, _, st, _ = sv.board_poses(p["cam0"], a["corners"], a["board"], a["coff"])
    k19 = sv.camera_calibrate(p["cam0"], a["corners"], a["board"], a["coff"], q, t)
    cam, q0, t0 = k19["cameras"][0], k19["q"], k19["t"]
    args = (a["corners"], a["board"], a["coff"], a["pts"], a["poff"], q0, t0, a["poses_cl0"])
    r21 = sv.joint_refine_range(cam, *args)
    r22 = sv.joint_refine_robust(cam, *args)
    # K21 -> corrected points -> K22, from K21's poses
    fixed = sv.range_correct(a["pts"], *r21["range"][0])
    r2122 = sv.joint_refine_robust(cam, a["corners"], a["board"], a["coff"], fixed, a["poff"], r21["q"], r21["t"], r21["poses_cl"])
    fo = _capi.default_full_options(cam.model)
    r23 = sv.calibrate_full(cam, *args, full=fo)
    fo.hold_range_mask = 2
    r23k = sv.calibrate_full(cam, *args, full=fo)
    err = lambda r: 1e3 * cases.tcl_distance(r["poses_cl"][0], p["pose_cl_true"])
    rows.append([err(r21), err(r22), err(r2122), err(r23), err(r23k), r23["summaries"][0].num_iterations, r23k["summaries"][0].num_iterations])
    truth = np.r_[p["range_true"], p["cam"].proj, p["cam"].dist]
    for r, free in ((r23, list(range(16))), (r23k, [j for j in range(16) if j != 7])):
        H = r["H_full"][0]
        sg = sigma_of(H, free)
        held = [j for j in free if j < 8]
        ratio = sg[:6] / sigma_of(H, held)[:6]  # H restricted to [T_cl, range] is the information with the intrinsics held
        got = np.r_[r["range"][0], r["cameras"][0].proj, r["cameras"][0].dist]
        zrows.append((ratio, (got - truth) / sg[6:], sg))


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n_batch = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    n_sets = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    out = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "full_calibration.md")
    cam = cases.CAMERAS[NAME]
    lines, terms = [], []
    tables = {}
    with clc.Solver(0) as sv:
        one = cases.problem(NAME, 900, 100, 144, 100, offset=0.02, scale=0.005)
        distinct = [cases.problem(NAME, 1000 + k, 50, 144, 100, offset=0.02, scale=0.005) for k in range(min(32, n_batch))]
        for label, probs, n in (("1 problem, 100 images x (144 corners + 100 points)", [one], 1),
                                ("%d problems of 50 such images (32 distinct, tiled)" % n_batch, [distinct[k % len(distinct)] for k in range(n_batch)], n_batch)):
            a = cases.arrays(probs)
            q0, t0, _, st, _ = sv.board_poses(cam, a["corners"], a["board"], a["coff"])
            assert np.all(st == 1)
            ms, sms = timed_calls(sv, cam, [cam] * n, a, q0, t0, repeats)
            lines.append(timing_row(label, ms, sms, n))
            terms.append((label, [int(v) for v in np.bincount([sms["K23"][k].termination for k in range(n)], minlength=7)[1:]]))
        for label, dirty in (("clean", False), ("contaminated", True)):
            rows, zrows = [], []
            for s in range(n_sets):
                recovery(sv, cases.problem(NAME, 600 + s, 30, 144, 100, dirty=dirty, offset=0.02, scale=0.005), rows, zrows)
            tables[label] = (np.array(rows), zrows)
    names = ("b", "kappa", "fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")
    with open(out, "w") as f:
        f.write("# K23: one robust cost over intrinsics, board poses, T_cl and range (MI355X)\n\n")
        f.write("## Timing: K23 beside K19, K21 and K22 on the same data\n\n")
        f.write("`python scripts/full_calibration.py %d %d %d`: camera `%s`, 0.3 px and 0.01 m of noise, a planted range error of 0.02 m and "
                "0.5 %%, start poses from `clc_board_poses` under the true camera, which is also every call's start camera (K21, K22: their "
                "fixed camera), T_cl from a perturbed truth.  Device arrays, the four `_device` calls in turn on the same arrays with "
                "their default options (H and, for K22 and K23, both weight arrays requested), one round to warm; median of %d (min – max), "
                "each call ending in its stream synchronise (wall clock around the call).  The four costs have different minimisers and "
                "unknowns, so the iteration counts differ.  K23's workspace is 8.3 KB per image (435 MB for the batch, one pool block).  No "
                "time target was set.\n\n" % (repeats, n_batch, n_sets, NAME, repeats))
        f.write("| problems | K19 ms | K19 LM iterations | K21 ms | K21 LM iterations | K22 ms | K22 LM iterations | K23 ms | K23 LM iterations |\n"
                "|---|---|---|---|---|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n\n")
        for label, term in terms:
            f.write("Terminations of K23, %s (gradient, parameter, function, radius, no convergence, failure): %s.\n" % (label, term))
        f.write("\n## T_cl against the truth: K23 and the staged routes, %d seeded sets of 30 images\n\n" % n_sets)
        f.write("Sets `fullcal_cases.problem(\"%s\", 600 + s, 30, 144, 100, offset=0.02, scale=0.005)`, clean and contaminated (10 %% of each "
                "image's points pulled 0.10 – 0.30 m towards the scanner, 5 %% of its corners moved 3 – 10 px).  Every route starts from the "
                "camera `clc_camera_calibrate` gives on the same corners (started 1 %% off the truth) and its poses; K21, K22 and K21 → "
                "`clc_range_correct` → K22 take that camera as exact, K23 refines it.  Mean (median, max) of |t_cl − truth| in mm.\n\n" % NAME)
        f.write("| data | K19 → K21 | K19 → K22 | K19 → K21 → K22 | K23, defaults | K23, scale held | K23 LM iterations (defaults / scale held) |\n"
                "|---|---|---|---|---|---|---|\n")
        for label, (rows, _) in tables.items():
            f.write("| %s | %s | %d – %d / %d – %d |\n" % (label, " | ".join("%.2f (%.2f, %.2f)" % (rows[:, j].mean(), np.median(rows[:, j]), rows[:, j].max())
                                                                           for j in range(5)),
                                                        rows[:, 5].min(), rows[:, 5].max(), rows[:, 6].min(), rows[:, 6].max()))
        f.write("\n## What the free intrinsics do to T_cl's predicted 1 sigma\n\n")
        f.write("At K23's answer, sigma of T_cl's six tangent parameters from inv(H_full over the free set) over the same from inv(H_full "
                "restricted to [T_cl, b, kappa]) — the information with the intrinsics held at that point; mean over the sets (min – max).\n\n")
        f.write("| data, options | t_x | t_y | t_z | theta_x | theta_y | theta_z |\n|---|---|---|---|---|---|---|\n")
        for label, (_, zrows) in tables.items():
            for j, opt in enumerate(("defaults", "scale held")):
                R = np.array([z[0] for z in zrows[j::2]])
                f.write("| %s, %s | %s |\n" % (label, opt, " | ".join("%.2f (%.2f – %.2f)" % (R[:, c].mean(), R[:, c].min(), R[:, c].max()) for c in range(6))))
        f.write("\n## Recovered b, kappa and intrinsics against their predicted sigma\n\n")
        f.write("(recovered − truth) / sigma over the sets: mean ± standard deviation (a calibrated estimate gives 0 ± 1), and the mean "
                "predicted sigma.  kappa carries the errors-in-variables bias of a scale on a noisy range (DESIGN.md K21), and on the "
                "contaminated sets the one-sided pull of the planted points along the focal length / depth / scale direction (DESIGN.md K23).\n\n")
        f.write("| data, options | %s |\n|---|%s\n" % (" | ".join(names), "---|" * len(names)))
        for label, (_, zrows) in tables.items():
            for j, opt in enumerate(("defaults", "scale held")):
                Z = np.array([z[1] for z in zrows[j::2]])
                S = np.array([z[2][6:] for z in zrows[j::2]])
                f.write("| %s, %s | %s |\n" % (label, opt, " | ".join("held" if np.all(np.isnan(Z[:, c])) else "%+.2f ± %.2f (σ %.2g)" % (
                    Z[:, c].mean(), Z[:, c].std(), S[:, c].mean()) for c in range(10))))
    print(open(out).read())


if __name__ == "__main__":
    main()
