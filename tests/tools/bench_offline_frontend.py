#!/usr/bin/env python3
"""Board-segment detection (clc_board_segments*, K7) on simulated 1 081-ray scans: the warm device call (arrays already on the
device; wall time including its stream synchronisation), the host call (points copied in, segments copied out), and the test
restatement on one host core for scale.  Run under `rocprofv3 --kernel-trace --stats` for the kernel time alone.

    python tests/tools/bench_offline_frontend.py [n_scans ...]        # default 20000 100000; one JSON line per size"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import board_segment_ref as R  # noqa: E402
import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import simdata as sd  # noqa: E402

RAYS = 1081
WINDOW_BYTES = (2 * 266 + 1) * 24  # the points of the search window: every cache line of it is read


def main():
    import torch
    sizes = [int(a) for a in sys.argv[1:]] or [20000, 100000]
    base = sd.scan_points_host(sd.sim_laser_scans(7, 2000))  # tiled up to the requested count
    t0 = time.perf_counter()
    seg_py, _ = R.board_segments(base[:200 * RAYS], np.arange(201, dtype=np.int64) * RAYS)
    py_us = (time.perf_counter() - t0) / 200 * 1e6
    dev = torch.device("cuda:0")
    with clc.Solver(0) as sv:
        for S in sizes:
            P = np.tile(base, (S // 2000 + 1, 1))[:S * RAYS]
            off = np.arange(S + 1, dtype=np.int64) * RAYS
            d_p, d_off = torch.from_numpy(P).to(dev), torch.from_numpy(off).to(dev)
            d_seg = torch.empty((S, 2), dtype=torch.int64, device=dev)
            d_st = torch.empty((S,), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ts = []
            for _ in range(25):
                t0 = time.perf_counter()
                sv.board_segments_device(d_p.data_ptr(), d_off.data_ptr(), S, d_seg.data_ptr(), d_st.data_ptr())
                ts.append(time.perf_counter() - t0)
            dev_ms = float(np.median(ts[5:]) * 1e3)
            th = []
            for _ in range(5):
                t0 = time.perf_counter()
                seg, st = sv.board_segments(P, off)
                th.append(time.perf_counter() - t0)
            assert np.array_equal(seg, d_seg.cpu().numpy())
            assert np.array_equal(seg[:200], seg_py)
            print(json.dumps(dict(scans=S, rays=RAYS, found=int((st == 1).sum()), device_call_ms=dev_ms,
                                  device_call_window_GBps=S * WINDOW_BYTES / (dev_ms * 1e-3) / 1e9,
                                  host_call_ms_incl_copies=float(np.median(th[1:]) * 1e3), points_MB=P.nbytes / 1e6,
                                  python_restatement_ms_one_core=py_us * S / 1e3)))
            del d_p, d_off, d_seg, d_st


if __name__ == "__main__":
    main()
