"""Timing of clc_board_poses (K10: lift + one wave per image) on a full 6x6 Kalibr board (144 corners per image, 0.3 px noise) for
10^3 / 10^4 / 10^5 images, both camera models: the host call (copies in and out included) and the _device call on resident
arrays, warm medians.  Prints one JSON line; `python scripts/board_poses.py [reps]`.  Kernel-only numbers: run it under
`rocprofv3 --kernel-trace --stats` (profiles/board_poses.md)."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import camera as cm  # noqa: E402

PROJ = (367.049931000148, 366.94446918887405, 368.7202381120387, 241.13814795878562)
CAMERAS = {"pinhole_radtan": cm.Camera.pinhole(*PROJ, k1=-0.012, k2=0.0015, p1=2e-4, p2=-1.5e-4),
           "kannala_brandt": cm.Camera.kannala_brandt(*PROJ, -0.02276964, -0.00056958, -0.0026224, 0.00017455)}


def _rot(v):
    th = np.linalg.norm(v, axis=1)[:, None, None]
    k = v / np.maximum(th[:, :, 0], 1e-300)
    K = np.zeros((len(v), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def images(sv, cam, n, seed=0):
    rng = np.random.default_rng(seed)
    b = cm.kalibr_board_points(np.arange(36), 6, 6, 0.055, 0.3)
    X = np.concatenate([b.astype(np.float64), np.zeros((len(b), 1))], 1)
    R = _rot(rng.normal(size=(n, 3)) * 0.3)
    t = np.array([-0.2, -0.2, 0.0]) + rng.uniform([-0.2, -0.2, 0.8], [0.2, 0.2, 1.6], size=(n, 3))
    Pc = np.einsum("nij,mj->nmi", R, X) + t[:, None, :]
    px = sv.camera_project(cam, Pc.reshape(-1, 3)) + rng.normal(size=(n * len(b), 2)) * 0.3
    off = np.arange(n + 1, dtype=np.int64) * len(b)
    return px.astype(np.float32), np.tile(b, (n, 1)), off


def _ms(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = {"what": "clc_board_poses, 6x6 Kalibr board (144 corners / image), warm median ms", "reps": reps, "runs": []}
    dev = torch.device("cuda:0")
    with clc.Solver(0) as sv:
        for name, cam in CAMERAS.items():
            for n in (1000, 10000, 100000):
                px, b, off = images(sv, cam, n)
                host_ms = _ms(lambda: sv.board_poses(cam, px, b, off), reps)
                q, t, rms, st, sm = sv.board_poses(cam, px, b, off, want_summaries=True)
                dc, db, do = (torch.from_numpy(a).to(dev) for a in (px, b, off))
                dq = torch.empty((n, 4), dtype=torch.float64, device=dev); dt = torch.empty((n, 3), dtype=torch.float64, device=dev)
                ds = torch.empty(n, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                dev_ms = _ms(lambda: sv.board_poses_device(cam, dc.data_ptr(), db.data_ptr(), do.data_ptr(), n, dq.data_ptr(),
                                                           dt.data_ptr(), 0, ds.data_ptr()), reps)
                its = np.array([s.num_iterations for s in sm])
                out["runs"].append({"camera": name, "images": n, "host_call_ms": round(host_ms, 3), "device_call_ms": round(dev_ms, 3),
                                    "ok": int((st == 1).sum()), "lm_iterations_mean": round(float(its.mean()), 2),
                                    "rms_median": float(np.median(rms))})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
