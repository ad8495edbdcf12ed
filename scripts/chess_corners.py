"""Timing of clc_chess_corners_device (K25: the detection's two kernels) beside clc_corner_subpix_device (K24) at half-window 11 on the
corners it finds, and of the host ordering between them (clc_chessboard_order), all in one run: 10^4 images of 752 x 480 resident on the
device (8 chessboards of 9 x 6 inner corners rendered by the test generator tests/subpix_cases.py, tiled; 3.6 GB), default options;
warm medians.  With them the detection's bytes per second (the image bytes, read once, over the call's time) against the 8 TB/s of the
HBM, the boards found, and the refined corners against the truth.  Prints one JSON line;
`python scripts/chess_corners.py [reps] [--images N] [--profile]` (--profile: three detection calls and nothing else, for a run under
`rocprofv3 --kernel-trace --stats`, which gives the two kernels' own times; profiles/chess_corners.md)."""
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

WIDTH, HEIGHT = 752, 480
PROJ = (460.0, 460.0, 375.5, 239.5)
INNER, SQUARE = (9, 6), 0.03
N_RENDERED = 8
HBM_BYTES_PER_S = 8.0e12


def scenes():
    out = []
    for k in range(N_RENDERED):
        rng = np.random.default_rng(2520 + k)
        R = campose_ref.rotvec_to_R(rng.uniform(-0.25, 0.25, 3))
        centre = np.array([(INNER[0] - 1) / 2 * SQUARE, (INNER[1] - 1) / 2 * SQUARE, 0.0])
        t = np.array([rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02), rng.uniform(0.45, 0.6)]) - R @ centre
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
    cols, rows = INNER
    per = cols * rows
    dev = torch.device("cuda:0")
    base = torch.from_numpy(np.stack([s["image"] for s in sc])).to(dev)
    images = base.repeat((n + N_RENDERED - 1) // N_RENDERED, 1, 1)[:n].contiguous()
    o = _capi.default_chess_options()
    stride = o.max_per_image
    d_xy = torch.empty((n, stride, 2), dtype=torch.float32, device=dev)
    d_r5 = torch.empty((n, stride), dtype=torch.int32, device=dev)
    d_count = torch.empty(n, dtype=torch.int32, device=dev); d_raw = torch.empty_like(d_count); d_status = torch.empty_like(d_count)
    torch.cuda.synchronize()
    out = {"what": "clc_chess_corners_device, clc_chessboard_order (host), clc_corner_subpix_device at half-window 11; warm median ms", "images": n,
           "image": [WIDTH, HEIGHT], "inner": list(INNER), "image_bytes": int(images.numel()), "reps": reps}
    with clc.Solver(0) as sv:
        def detect():
            sv.chess_corners_device(images.data_ptr(), WIDTH, HEIGHT, WIDTH, n, d_xy.data_ptr(), d_count.data_ptr(), d_status.data_ptr(),
                                    d_r5.data_ptr(), d_raw.data_ptr(), o)

        if profile:
            for _ in range(3):
                detect()
            print(json.dumps({"profile": True, "images": n}))
            return
        detect()  # warm
        td = [_ms(detect) for _ in range(reps)]
        xy, count, status = d_xy.cpu().numpy(), d_count.cpu().numpy(), d_status.cpu().numpy()
        order = None
        to = []
        for _ in range(min(reps, 3)):
            t0 = time.perf_counter()
            order = clc.chessboard_order(xy, count, cols, rows, status)
            to.append((time.perf_counter() - t0) * 1e3)
        found = order["status"] == 1
        starts = np.full((n, per, 2), np.nan, np.float32)
        idx = order["index"].reshape(n, per)
        starts[found] = np.take_along_axis(xy[found], idx[found][:, :, None].astype(np.int64), axis=1)
        d_in = torch.from_numpy(starts.reshape(-1, 2)).to(dev)
        d_off = torch.from_numpy(np.arange(n + 1, dtype=np.int64) * per).to(dev)
        d_out = torch.empty_like(d_in)
        d_st = torch.empty(n * per, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        so = _capi.default_subpix_options(11)

        def subpix():
            sv.corner_subpix_device(images.data_ptr(), WIDTH, HEIGHT, WIDTH, n, d_in.data_ptr(), d_off.data_ptr(), d_out.data_ptr(), d_st.data_ptr(), 0, 0, so)

        subpix()  # warm
        ts = [_ms(subpix) for _ in range(reps)]
        refined = d_out.cpu().numpy().reshape(n, per, 2)
        # the truth under the labeling's two readings (the board as rendered, or turned by a half turn)
        err_px, err_ref = [], []
        for k in range(min(n, N_RENDERED)):
            if not found[k]:
                continue
            truth = sc[k]["truth"]
            e = min((np.linalg.norm(starts[k] - t, axis=1).max(), np.sqrt(np.mean(np.sum((refined[k] - t) ** 2, axis=1)))) for t in (truth, truth[::-1]))
            err_px.append(float(e[0])); err_ref.append(float(e[1]))
        med = statistics.median(td)
        out.update({
            "detect_ms": round(med, 3), "detect_ms_min_max": [round(min(td), 3), round(max(td), 3)],
            "detect_bytes_per_s": round(images.numel() / (med * 1e-3), 1), "detect_fraction_of_8TBps": round(images.numel() / (med * 1e-3) / HBM_BYTES_PER_S, 4),
            "detect_us_per_image": round(med * 1e3 / n, 3),
            "order_host_ms": round(statistics.median(to), 3), "order_host_us_per_image": round(statistics.median(to) * 1e3 / n, 3),
            "subpix11_ms": round(statistics.median(ts), 3), "subpix11_ms_min_max": [round(min(ts), 3), round(max(ts), 3)],
            "found": int(found.sum()), "candidates_per_image_min_max": [int(count.min()), int(count.max())],
            "raw_per_image_min_max": [int(d_raw.cpu().numpy().min()), int(d_raw.cpu().numpy().max())],
            "status": {int(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))},
            "subpix_status": {int(k): int(v) for k, v in zip(*np.unique(d_st.cpu().numpy(), return_counts=True))},
            "ordered_pixel_farthest_from_truth_px": round(max(err_px), 3) if err_px else None,
            "refined_rms_px_worst_image": round(max(err_ref), 4) if err_ref else None,
        })
    print(json.dumps(out))


if __name__ == "__main__":
    main()
