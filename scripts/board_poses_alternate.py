"""Timing of clc_board_poses_alternate (K17: lift + mirror start + the LM stage from it) against clc_board_poses on the SAME images in
the SAME run: 10^4 images of the full 6x6 Kalibr board (144 corners per image, 0.3 px noise), device arrays, warm medians, (a) the
near views of scripts/board_poses.py (0.8-1.6 m) and (b) far views (3.5-4.5 m), where most images have a distinct second minimum.
The input poses are clc_board_poses' own.  Also prints what the default same_angle rests on: the largest rot_angle of a SAME image
and the smallest of a DISTINCT one.  One JSON line; `python scripts/board_poses_alternate.py [reps] [images]`
(profiles/board_poses_alternate.md)."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import camera as cm  # noqa: E402
from board_poses import CAMERAS, _rot  # noqa: E402


def images(sv, cam, n, zlo, zhi, seed=0):
    """scripts/board_poses.py's images with the depth range given (the lateral offsets grow with it)."""
    rng = np.random.default_rng(seed)
    b = cm.kalibr_board_points(np.arange(36), 6, 6, 0.055, 0.3)
    X = np.concatenate([b.astype(np.float64), np.zeros((len(b), 1))], 1)
    R = _rot(rng.normal(size=(n, 3)) * 0.3)
    z = rng.uniform(zlo, zhi, size=n)
    t = np.array([-0.2, -0.2, 0.0]) + np.stack([rng.uniform(-0.2, 0.2, n) * z, rng.uniform(-0.2, 0.2, n) * z, z], 1)
    Pc = np.einsum("nij,mj->nmi", R, X) + t[:, None, :]
    px = sv.camera_project(cam, Pc.reshape(-1, 3)) + rng.normal(size=(n * len(b), 2)) * 0.3
    off = np.arange(n + 1, dtype=np.int64) * len(b)
    return px.astype(np.float32), np.tile(b, (n, 1)), off


def _ms_pair(f, g, reps):
    """Both calls warmed once, then timed alternately (each ends in a stream synchronise) -> (median, min, max) ms of each."""
    f()
    g()
    tf, tg = [], []
    for _ in range(reps):
        for h, ts in ((f, tf), (g, tg)):
            t0 = time.perf_counter()
            h()
            ts.append((time.perf_counter() - t0) * 1e3)
    return tuple((statistics.median(ts), min(ts), max(ts)) for ts in (tf, tg))


def main():
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    out = {"what": "clc_board_poses_alternate vs clc_board_poses, 6x6 Kalibr board (144 corners / image), device arrays, warm median ms",
           "reps": reps, "images": n, "runs": []}
    dev = torch.device("cuda:0")
    with clc.Solver(0) as sv:
        for name, cam in CAMERAS.items():
            for view, (zlo, zhi) in (("near 0.8-1.6 m", (0.8, 1.6)), ("far 3.5-4.5 m", (3.5, 4.5))):
                px, b, off = images(sv, cam, n, zlo, zhi)
                dc, db, do = (torch.from_numpy(a).to(dev) for a in (px, b, off))
                f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
                dq, dt, dqa, dta, dra, dratio, dcin, dcalt = f64(n, 4), f64(n, 3), f64(n, 4), f64(n, 3), f64(n), f64(n), f64(n), f64(n)
                ds = torch.empty(n, dtype=torch.int32, device=dev); dk = torch.empty(n, dtype=torch.int32, device=dev)
                da = torch.empty(n, dtype=torch.uint8, device=dev); dbt = torch.empty(n, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                f = lambda: sv.board_poses_device(cam, dc.data_ptr(), db.data_ptr(), do.data_ptr(), n, dq.data_ptr(), dt.data_ptr(), 0, ds.data_ptr())
                g = lambda: sv.board_poses_alternate_device(cam, dc.data_ptr(), db.data_ptr(), do.data_ptr(), n, dq.data_ptr(), dt.data_ptr(),
                                                            ds.data_ptr(), dk.data_ptr(), q_ptr=dqa.data_ptr(), t_ptr=dta.data_ptr(),
                                                            cost_in_ptr=dcin.data_ptr(), cost_alt_ptr=dcalt.data_ptr(),
                                                            ratio_ptr=dratio.data_ptr(), rot_angle_ptr=dra.data_ptr(),
                                                            ambiguous_ptr=da.data_ptr(), better_ptr=dbt.data_ptr())
                plain, alt = _ms_pair(f, g, reps)
                kind, ra, ratio = dk.cpu().numpy(), dra.cpu().numpy(), dratio.cpu().numpy()
                same, dist = kind == 1, kind == 2
                out["runs"].append({
                    "camera": name, "view": view, "board_poses_ms": round(plain[0], 3), "board_poses_min_max": [round(plain[1], 3), round(plain[2], 3)],
                    "alternate_ms": round(alt[0], 3), "alternate_min_max": [round(alt[1], 3), round(alt[2], 3)],
                    "ratio_of_times": round(alt[0] / plain[0], 3), "ok_in": int((ds.cpu().numpy() == 1).sum()),
                    "none_same_distinct": np.bincount(kind, minlength=3).tolist(), "ambiguous": int(da.cpu().numpy().sum()),
                    "better": int(dbt.cpu().numpy().sum()),
                    "largest_same_rot_angle": float(ra[same].max()) if same.any() else None,
                    "smallest_distinct_rot_angle": float(ra[dist].min()) if dist.any() else None,
                    "distinct_cost_ratio_min_median": [float(np.min(ratio[dist])), float(np.median(ratio[dist]))] if dist.any() else None})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
