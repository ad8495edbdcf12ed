"""K19 camera intrinsics from the board images: warm device time of clc_camera_calibrate_device beside the host route
(scipy.optimize.least_squares on the restatement tests/camcal_ref.py) for the same problems in the same run, and the parameter error
against the ground truth on seeded sets next to the 1 sigma that H_cam predicts.  Writes profiles/camera_calibrate.md.

  python scripts/camera_calibrate.py [repeats=5] [batch=1024] [accuracy_seeds=20]

Needs the GPU (torch for the device arrays) and scipy."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import camcal_cases as cases  # noqa: E402
import camcal_ref as ref  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi, calib  # noqa: E402
from camlasercalibratool_amd.camera import ClcCamera  # noqa: E402

NAMES = ("radtan", "kb")
PARAMS = {"radtan": ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"), "kb": ("mu", "mv", "u0", "v0", "k2", "k3", "k4", "k5")}


def k_of(cam):
    return np.r_[cam.proj, cam.dist].astype(np.float64)


def timed_device(sv, start, a, q0, t0, co, repeats):
    """clc_camera_calibrate_device on device arrays, fresh start poses and cameras every call -> (ms list, summaries, k [np, 8])."""
    import torch
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    n, npb = len(a["coff"]) - 1, len(a["prob_off"]) - 1
    dc, db, dco, dpr = up(a["corners"]), up(a["board"]), up(a["coff"]), up(a["prob_off"])
    q_in, t_in = up(q0), up(t0)
    cam_in = up(np.frombuffer(bytes(start.to_c()) * npb, dtype=np.uint8).copy())
    dst = torch.zeros(n, dtype=torch.int32, device=dev)
    dsm = torch.zeros(npb * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev)
    dH = torch.zeros((npb, 64), dtype=torch.float64, device=dev)
    drms = torch.zeros(npb, dtype=torch.float64, device=dev)
    ms = []
    for _ in range(repeats + 1):  # the first call warms
        dq, dt, dcam = q_in.clone(), t_in.clone(), cam_in.clone()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        sv.camera_calibrate_device(dc.data_ptr(), db.data_ptr(), dco.data_ptr(), n, npb, dcam.data_ptr(), dq.data_ptr(), dt.data_ptr(),
                                   dsm.data_ptr(), dst.data_ptr(), problem_offsets_ptr=dpr.data_ptr(), H_cam_ptr=dH.data_ptr(),
                                   rms_ptr=drms.data_ptr(), camcal=co)
        ms.append((time.perf_counter() - t1) * 1e3)
    sm = (_capi.Summary * npb).from_buffer_copy(dsm.cpu().numpy().tobytes())
    cams = (ClcCamera * npb).from_buffer_copy(dcam.cpu().numpy().tobytes())
    return ms[1:], sm, np.array([list(c.proj) + list(c.dist) for c in cams])


def host_route(start, a, k, q0, t0, co):
    """scipy on the restatement for problem k from the same start -> (seconds, cost)."""
    idx = range(a["prob_off"][k], a["prob_off"][k + 1])
    prob = dict(model=start.model, px=[a["corners"][a["coff"][i]:a["coff"][i + 1]].astype(np.float64) for i in idx],
                board=[a["board"][a["coff"][i]:a["coff"][i + 1]].astype(np.float64) for i in idx], sigma=co.sigma_px)
    t1 = time.perf_counter()
    out = ref.solve(prob, k_of(start), [ref.quat_wxyz_to_R(q0[i]) for i in idx], [t0[i].copy() for i in idx], hold_mask=co.hold_mask, rounds=1)
    return time.perf_counter() - t1, out[3]


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n_batch = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    n_seeds = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    lines, acc = [], {}
    with clc.Solver(0) as sv:
        name = "radtan"
        cam = cases.CAMERAS[name]
        start = cases.start_camera(cam)
        co = _capi.default_camcal_options(cam.model)
        # ---- one problem of 100 images x 144 corners ----
        a1 = cases.arrays([cases.images(name, 900, 100)])
        q1, t1, _, st, _ = sv.board_poses(start, a1["corners"], a1["board"], a1["coff"])
        assert np.all(st == 1)
        ms1, sm1, _ = timed_device(sv, start, a1, q1, t1, co, repeats)
        hs1, hc1 = host_route(start, a1, 0, q1, t1, co)
        lines.append("| 1 problem, 100 images x 144 corners | %.3f (%.3f – %.3f) | %d | %.1f | %.2e |" % (
            np.median(ms1), min(ms1), max(ms1), sm1[0].num_iterations, hs1 * 1e3, abs(sm1[0].final_cost - hc1) / hc1))
        # ---- n_batch problems of 20 images: 32 distinct, tiled ----
        distinct = [cases.images(name, 1000 + k, 20) for k in range(min(32, n_batch))]
        ab = cases.arrays([distinct[k % len(distinct)] for k in range(n_batch)])
        qb, tb, _, st, _ = sv.board_poses(start, ab["corners"], ab["board"], ab["coff"])
        assert np.all(st == 1)
        msb, smb, _ = timed_device(sv, start, ab, qb, tb, co, repeats)
        hb = [host_route(start, ab, k, qb, tb, co) for k in range(2)]
        its = [smb[k].num_iterations for k in range(n_batch)]
        term = np.bincount([smb[k].termination for k in range(n_batch)], minlength=7)
        gap = max(abs(smb[k].final_cost - hb[k][1]) / hb[k][1] for k in range(2))
        lines.append("| %d problems of 20 images x 144 corners (32 distinct, tiled) | %.3f (%.3f – %.3f) | %d – %d | %.1f per problem (2 timed) = %.0f s for all | %.2e |" % (
            n_batch, np.median(msb), min(msb), max(msb), min(its), max(its), np.mean([h[0] for h in hb]) * 1e3,
            np.mean([h[0] for h in hb]) * n_batch, gap))
        # ---- accuracy: the whole flow from the closed-form start, 20 images ----
        for nm in NAMES:
            c = cases.CAMERAS[nm]
            rows, f0 = [], []
            for seed in range(n_seeds):
                imgs = cases.images(nm, 2000 + seed + 100 * (nm == "kb"), 20)
                out, _, _, rep = calib.CalibrateCamera(c.model, c.width, c.height, [i[0] for i in imgs], [i[1] for i in imgs], solver=sv)
                assert rep["termination"].startswith("CONVERGENCE"), (nm, seed, rep["termination"])
                truth = k_of(c)
                held = [(rep["hold_mask"] >> j) & 1 for j in range(8)]
                truth = np.where(held, k_of(out), truth)  # a held intrinsic is not estimated
                rows.append(np.r_[k_of(out) - truth, rep["sigma"], rep["rms_px"]])
                f0.append(rep["camera0"].proj[0])
            acc[nm] = (np.array(rows), np.array(f0))
    out = os.path.join(ROOT, "profiles", "camera_calibrate.md")
    with open(out, "w") as f:
        f.write("# K19 camera intrinsics from the board images — timing and accuracy (MI355X)\n\n")
        f.write("`python scripts/camera_calibrate.py %d %d %d`: camera `radtan`, 0.3 px of noise, board 0.5-1.2 m away, tilted 10-40 degrees, up to "
                "0.3 x distance off the axis; the start camera 1 %% off in the focal lengths, 2 px in the principal point, 5 %% in the distortion; "
                "start poses from `clc_board_poses` under it; device arrays, `clc_camera_calibrate_device` with the default options (H_cam and "
                "the RMS requested), warmed once; median of %d (min – max), each call ending in its stream synchronise.  Host route: "
                "`scipy.optimize.least_squares` (lm, analytic dense Jacobian, tolerances 1e-15, one round) on the restatement "
                "`tests/camcal_ref.py`, same problems, same start, same run, on the host's CPU.  No time gate was set.\n\n" % (repeats, n_batch, n_seeds, repeats))
        f.write("| problems | device ms | LM iterations | host route ms | relative cost gap device / host |\n|---|---|---|---|---|\n")
        f.write("\n".join(lines) + "\n\n")
        f.write("Terminations of the batch (gradient, parameter, function, radius, no convergence, failure): %s.\n\n" % [int(v) for v in term[1:]])
        f.write("## The intrinsics against the truth, next to the predicted 1 sigma\n\n")
        f.write("%d seeded sets of 20 images x 144 corners per camera through `calib.CalibrateCamera`: the closed-form start "
                "(`clc_camera_guess`), `clc_board_poses` under it, `clc_camera_calibrate` with the default mask.  Error: estimate - truth; "
                "sigma: from inv(H_cam) over the free intrinsics.  Reported whatever it shows.\n\n" % n_seeds)
        for nm in NAMES:
            rows, f0 = acc[nm]
            c = cases.CAMERAS[nm]
            f.write("`%s` (closed-form start f = %.0f – %.0f against the true %.0f; RMS %.3f – %.3f px):\n\n" % (
                nm, f0.min(), f0.max(), c.proj[0], rows[:, 16].min(), rows[:, 16].max()))
            f.write("| parameter | RMS error | largest error | mean predicted sigma | largest error / sigma |\n|---|---|---|---|---|\n")
            for j, p in enumerate(PARAMS[nm]):
                if np.all(np.isnan(rows[:, 8 + j])):
                    f.write("| %s | held | | | |\n" % p)
                    continue
                e, s = rows[:, j], rows[:, 8 + j]
                f.write("| %s | %.3g | %.3g | %.3g | %.2f |\n" % (p, np.sqrt(np.mean(e ** 2)), np.abs(e).max(), s.mean(), np.abs(e / s).max()))
            f.write("\n")
    print(open(out).read())


if __name__ == "__main__":
    main()
