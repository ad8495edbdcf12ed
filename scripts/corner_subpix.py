"""Timing of clc_corner_subpix_device (K24: one wave per corner) beside the pose fit it feeds, clc_board_poses_device (K10), on the same
images in the same run: 10^4 images of 752 x 480 (8 chessboards of 12 x 12 = 144 inner corners rendered by the test generator
tests/subpix_cases.py, tiled; 3.6 GB resident on the device), the starts = the true corners rounded to integers, half-windows 3 (the
reference's Kalibr call) and 11 (its chessboard call), 30 iterations, eps 0.1; warm medians, the two kernels alternating.  With them the
iteration histogram, the status counts, the refined corners against the truth, and the numpy restatement's time per corner on one core.
Prints one JSON line; `python scripts/corner_subpix.py [reps] [--images N] [--profile]`
(--profile: three calls of each and nothing else, for a run under `rocprofv3 --kernel-trace --stats`; profiles/corner_subpix.md)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402
import campose_ref  # noqa: E402
import subpix_cases as cases  # noqa: E402
import subpix_ref as ref  # noqa: E402

WIDTH, HEIGHT = 752, 480
PROJ = (460.0, 460.0, 375.5, 239.5)
INNER, SQUARE = (12, 12), 0.03
N_RENDERED = 8


def scenes():
    out = []
    for k in range(N_RENDERED):
        rng = np.random.default_rng(2480 + k)
        R = campose_ref.rotvec_to_R(rng.uniform(-0.2, 0.2, 3))
        centre = np.array([(INNER[0] - 1) / 2 * SQUARE, (INNER[1] - 1) / 2 * SQUARE, 0.0])
        t = np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02), rng.uniform(0.5, 0.6)]) - R @ centre
        out.append(cases.render_chessboard(WIDTH, HEIGHT, PROJ, INNER, SQUARE, R, t, rng))
    return out


def _ms(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    profile = "--profile" in sys.argv
    n = int(sys.argv[sys.argv.index("--images") + 1]) if "--images" in sys.argv else 10000
    sc = scenes()
    m = len(sc[0]["truth"])
    dev = torch.device("cuda:0")
    base = torch.from_numpy(np.stack([s["image"] for s in sc])).to(dev)
    images = base.repeat((n + N_RENDERED - 1) // N_RENDERED, 1, 1)[:n].contiguous()
    pick = np.arange(n) % N_RENDERED
    truth = np.stack([s["truth"] for s in sc])[pick].reshape(-1, 2)
    starts = np.rint(truth).astype(np.float32)
    board = np.stack([s["board_xy"] for s in sc])[pick].reshape(-1, 2)
    off = np.arange(n + 1, dtype=np.int64) * m
    d_in, d_board, d_off = (torch.from_numpy(a).to(dev) for a in (starts, board, off))
    d_out = torch.empty_like(d_in)
    d_st = torch.empty(n * m, dtype=torch.int32, device=dev); d_it = torch.empty_like(d_st)
    d_lam = torch.empty(n * m, dtype=torch.float64, device=dev)
    dq = torch.empty((n, 4), dtype=torch.float64, device=dev); dt = torch.empty((n, 3), dtype=torch.float64, device=dev)
    ds = torch.empty(n, dtype=torch.int32, device=dev)
    cam = clc.Camera.pinhole(*PROJ, width=WIDTH, height=HEIGHT)
    torch.cuda.synchronize()
    out = {"what": "clc_corner_subpix_device beside clc_board_poses_device, warm median ms", "images": n, "corners_per_image": m,
           "image": [WIDTH, HEIGHT], "image_bytes": int(images.numel()), "reps": reps, "runs": []}
    with clc.Solver(0) as sv:
        def subpix(w):
            sv.corner_subpix_device(images.data_ptr(), WIDTH, HEIGHT, WIDTH, n, d_in.data_ptr(), d_off.data_ptr(), d_out.data_ptr(),
                                    d_st.data_ptr(), d_it.data_ptr(), d_lam.data_ptr(), _capi.default_subpix_options(w))

        def poses():
            sv.board_poses_device(cam, d_out.data_ptr(), d_board.data_ptr(), d_off.data_ptr(), n, dq.data_ptr(), dt.data_ptr(), 0, ds.data_ptr())

        if profile:
            for _ in range(3):
                for w in (3, 11):
                    subpix(w)
                poses()
            print(json.dumps({"profile": True, "images": n}))
            return
        for w in (3, 11):
            subpix(w); poses()  # warm
            ts, tp = [], []
            for _ in range(reps):
                ts.append(_ms(lambda: subpix(w)))
                tp.append(_ms(poses))
            it, st = d_it.cpu().numpy(), d_st.cpu().numpy()
            refined = d_out.cpu().numpy()
            err = np.sqrt(np.sum((refined.astype(np.float64) - truth) ** 2, axis=1))
            ok = st >= 0
            run = {"half_window": w, "subpix_ms": round(statistics.median(ts), 3), "subpix_ms_min_max": [round(min(ts), 3), round(max(ts), 3)],
                   "board_poses_ms": round(statistics.median(tp), 3), "board_poses_ms_min_max": [round(min(tp), 3), round(max(tp), 3)],
                   "ns_per_corner": round(statistics.median(ts) * 1e6 / (n * m), 2),
                   "iterations_histogram": {int(k): int(v) for k, v in zip(*np.unique(it, return_counts=True))},
                   "iterations_mean": round(float(it.mean()), 3),
                   "status": {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
                   "start_rms_px": round(float(np.sqrt(np.mean(np.sum((starts - truth) ** 2, axis=1)))), 4),
                   "refined_rms_px": round(float(np.sqrt(np.mean(err[ok] ** 2))), 4), "poses_ok": int((ds.cpu().numpy() == 1).sum())}
            # the numpy restatement on the corners of one image, one core; and the device against it on those corners
            t0 = time.perf_counter()
            r = ref.refine(sc[0]["image"][None], WIDTH, starts[:m], [0, m], ref.Options(w, w))
            run["numpy_us_per_corner"] = round((time.perf_counter() - t0) * 1e6 / m, 1)
            run["bitwise_equal_to_numpy_of_144"] = int((r["corners"].view(np.uint32) == refined[:m].view(np.uint32)).all(axis=1).sum())
            out["runs"].append(run)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
