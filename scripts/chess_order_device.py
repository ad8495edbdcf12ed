"""Timing of clc_chessboard_order_device (K26: the ordering on the device) beside the host ordering it restates (clc_chessboard_order),
the detection it follows (clc_chess_corners_device) and clc_find_chessboard_device whole (detection, ordering, gather, refinement at
half-window 11), all in one run on the workload of scripts/chess_corners.py: 10^4 images of 752 x 480 resident on the device, a 9 x 6
board, default options; warm medians.  The device ordering's index, status and n_labelings are compared with the host's on the whole
workload.  Prints one JSON line; `python scripts/chess_order_device.py [reps] [--images N] [--profile]` (--profile: one detection and
three ordering calls and nothing else, for a run under `rocprofv3 --kernel-trace --stats`, which gives the kernel's own time;
profiles/chess_order_device.md)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402
import chess_corners as workload  # noqa: E402

WIDTH, HEIGHT, INNER = workload.WIDTH, workload.HEIGHT, workload.INNER


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
    sc = workload.scenes()
    cols, rows = INNER
    per = cols * rows
    dev = torch.device("cuda:0")
    base = torch.from_numpy(np.stack([s["image"] for s in sc])).to(dev)
    images = base.repeat((n + len(sc) - 1) // len(sc), 1, 1)[:n].contiguous()
    o = _capi.default_chess_options()
    stride = o.max_per_image
    d_xy = torch.empty((n, stride, 2), dtype=torch.float32, device=dev)
    d_count = torch.empty(n, dtype=torch.int32, device=dev); d_status = torch.empty_like(d_count); d_st = torch.empty_like(d_count)
    d_index = torch.empty((n, per), dtype=torch.int32, device=dev); d_lab = torch.empty_like(d_count)
    d_worst = torch.empty(n, dtype=torch.float64, device=dev)
    d_corners = torch.empty((n, per, 2), dtype=torch.float32, device=dev); d_found = torch.empty_like(d_count)
    d_lam = torch.empty((n, per), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    out = {"what": "clc_chessboard_order_device, clc_chessboard_order (host), clc_chess_corners_device, clc_find_chessboard_device; warm median ms",
           "images": n, "image": [WIDTH, HEIGHT], "inner": list(INNER), "reps": reps}
    with clc.Solver(0) as sv:
        def detect():
            sv.chess_corners_device(images.data_ptr(), WIDTH, HEIGHT, WIDTH, n, d_xy.data_ptr(), d_count.data_ptr(), d_status.data_ptr(), 0, 0, o)

        def order():
            d_st.copy_(d_status)  # (the status is read and written; the copy of 40 KB is inside the timed call)
            torch.cuda.synchronize()
            sv.chessboard_order_device(d_xy.data_ptr(), d_count.data_ptr(), stride, n, cols, rows, d_index.data_ptr(), d_st.data_ptr(), d_lab.data_ptr(),
                                       d_worst.data_ptr())

        so = _capi.default_subpix_options(11)

        def find():
            sv.find_chessboard_device(images.data_ptr(), WIDTH, HEIGHT, WIDTH, n, cols, rows, d_corners.data_ptr(), d_found.data_ptr(), d_lam.data_ptr(),
                                      o, None, so)

        detect()  # warm
        if profile:
            for _ in range(3):
                order()
            print(json.dumps({"profile": True, "images": n}))
            return
        td = [_ms(detect) for _ in range(reps)]
        order()
        to = [_ms(order) for _ in range(reps)]
        find()
        tf = [_ms(find) for _ in range(reps)]
        xy, count, status = d_xy.cpu().numpy(), d_count.cpu().numpy(), d_status.cpu().numpy()
        th, host = [], None
        for _ in range(min(reps, 3)):
            t0 = time.perf_counter()
            host = clc.chessboard_order(xy, count, cols, rows, status)
            th.append((time.perf_counter() - t0) * 1e3)
        index, st, lab, worst = d_index.cpu().numpy(), d_st.cpu().numpy(), d_lab.cpu().numpy(), d_worst.cpu().numpy()
        ok = ~np.isnan(host["worst"])
        rel = np.abs(worst[ok] - host["worst"][ok]) / np.abs(host["worst"][ok])
        # clc_find_chessboard_device against the pixels the device ordering indexes, refined by the existing call
        whole_found = d_found.cpu().numpy()
        med_o, med_d, med_h = statistics.median(to), statistics.median(td), statistics.median(th)
        out.update({
            "order_device_ms": round(med_o, 3), "order_device_ms_min_max": [round(min(to), 3), round(max(to), 3)],
            "order_device_us_per_image": round(med_o * 1e3 / n, 3),
            "order_host_ms": round(med_h, 3), "order_host_us_per_image": round(med_h * 1e3 / n, 3),
            "detect_ms": round(med_d, 3), "detect_ms_min_max": [round(min(td), 3), round(max(td), 3)],
            "find_device_ms": round(statistics.median(tf), 3), "find_device_ms_min_max": [round(min(tf), 3), round(max(tf), 3)],
            "order_device_over_detect": round(med_o / med_d, 4), "order_host_over_order_device": round(med_h / med_o, 2),
            "index_equal": bool(np.array_equal(index, host["index"].reshape(n, per))), "status_equal": bool(np.array_equal(st, host["status"])),
            "n_labelings_equal": bool(np.array_equal(lab, host["n_labelings"])),
            "worst_largest_relative_difference_eps": float(rel.max() / 2.0 ** -52) if rel.size else None,
            "found": int((st == 1).sum()), "find_device_found": int(whole_found.sum()),
        })
    print(json.dumps(out))


if __name__ == "__main__":
    main()
