"""clc_assemble_observations_device (K13) against the only route the library offered before it for the same result
(profiles/offline_assemble.md):
  device form   every input already in device memory -> the observations stored on the handle, one call;
  host route    clc_scan_to_points_device + clc_board_segments_device, read-back of points / segments / status, key frames
                (tests/offline_ref.py's sequential walk), scan -> pose matching and the gather in numpy, calib.points_on_fitted_lines
                (clc_line_fit_batched + the end points), clc_store_observations.
                The matching is a vectorised numpy search over the sorted key-frame stamps, not offline_ref's walk per scan (10^5 x 10^3
                Python steps): the route is timed at its best.
`--scans` scans of 1 081 rays (64 simulated scans tiled) against `--poses` stamped poses (a random walk at 30 Hz, part of it still).
Warm-up calls first (the first is reported apart: it grows the handle's arrays and the pool), then `--reps` timed calls, host clock
around calls that end in a stream wait; medians with min / max.  Both results are compared before anything is timed.
Kernel times: run with --profile under `rocprofv3 --kernel-trace --stats` (a run of its own: device form only).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import simdata as sd  # noqa: E402
from camlasercalibratool_amd.simdata import ObservationSet  # noqa: E402


def stats(v):
    v = np.asarray(v) * 1e3
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "n": int(v.size)}


def make_poses(n, seed=3):
    """A walk at 30 Hz with still runs: every 3rd block of 50 poses does not move."""
    rng = np.random.default_rng(seed)
    moving = ((np.arange(n) // 50) % 3 != 0)[:, None]
    t = np.cumsum(rng.normal(0, 0.15, (n, 3)) * moving, axis=0)
    ang = np.cumsum(rng.normal(0, 0.01, (n, 3)) * moving, axis=0)
    q = sd.rot_to_quat_wxyz(sd.rot_zyx(ang[:, 0], ang[:, 1], ang[:, 2])).reshape(n, 4)
    return 100.0 + np.arange(n) / 30.0, q, t


def host_route(sv, torch, d, n_poses, S, n, pose_stamp, q, t, scan_stamp, R):
    """-> (ObservationSet stored on the handle, scan_pose)."""
    d_pts = torch.empty((n, 3), dtype=torch.float64, device=d["ranges"].device)
    d_seg = torch.empty((S, 2), dtype=torch.int64, device=d_pts.device)
    d_st = torch.empty((S,), dtype=torch.int32, device=d_pts.device)
    torch.cuda.synchronize()
    sv.scan_to_points_device(d["ranges"].data_ptr(), d["offsets"].data_ptr(), S, n, d["angle_min"].data_ptr(), d["angle_increment"].data_ptr(),
                             d["range_min"].data_ptr(), d_pts.data_ptr())
    sv.board_segments_device(d_pts.data_ptr(), d["offsets"].data_ptr(), S, d_seg.data_ptr(), d_st.data_ptr())
    P3, seg, status = d_pts.cpu().numpy(), d_seg.cpu().numpy(), d_st.cpu().numpy()
    keep = R.keyframes(q, t)
    kf = np.nonzero(keep)[0]
    ks = pose_stamp[kf]  # increasing here
    right = np.searchsorted(ks, scan_stamp, side="left")
    left = np.clip(right - 1, 0, len(ks) - 1)
    rightc = np.clip(right, 0, len(ks) - 1)
    dl, dr = np.abs(ks[left] - scan_stamp), np.abs(ks[rightc] - scan_stamp)
    best = np.where(dl <= dr, left, rightc)
    ok = (status == 1) & (np.minimum(dl, dr) < 0.02)
    scan_pose = np.where(status == 1, np.where(ok, kf[best], -3), np.where(status == -1, -2, -1)).astype(np.int32)
    kept = np.nonzero(ok)[0]
    lens = seg[kept, 1] - seg[kept, 0] + 1
    pts_off = np.zeros(len(kept) + 1, dtype=np.int64)
    pts_off[1:] = np.cumsum(lens)
    start = kept * 1081 + seg[kept, 0]
    idx = np.repeat(start - pts_off[:-1], lens) + np.arange(int(pts_off[-1]))
    pts = np.ascontiguousarray(P3[idx])
    qk = q[scan_pose[kept]]
    qi = qk * np.array([1.0, -1.0, -1.0, -1.0]) / np.sum(qk * qk, axis=1, keepdims=True)
    ti = -np.einsum("nij,nj->ni", sd.quat_wxyz_to_rot(qi).reshape(-1, 3, 3), t[scan_pose[kept]])
    obs = ObservationSet(qi, ti, pts_off, pts, pts_off.copy(), pts)
    obs = clc.points_on_fitted_lines(obs, solver=sv)
    sv.store_observations(obs)
    return obs, scan_pose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=20000)
    ap.add_argument("--poses", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route-reps", type=int, default=2)
    ap.add_argument("--profile", action="store_true", help="device form only (for a run under rocprofv3)")
    a = ap.parse_args()
    import torch
    import offline_ref as R
    dev = torch.device("cuda:0")
    S, n_poses = a.scans, a.poses
    base = sd.sim_laser_scans(7, 64)
    pose_stamp, q, t = make_poses(n_poses)
    rng = np.random.default_rng(5)
    scan_stamp = np.sort(rng.uniform(pose_stamp[0], pose_stamp[-1], S))
    idx = torch.from_numpy((np.arange(S) * 7) % 64).to(dev)
    d = {"ranges": torch.from_numpy(base["ranges"].reshape(64, 1081)).to(dev)[idx].contiguous().reshape(-1),
         "offsets": torch.arange(S + 1, dtype=torch.int64, device=dev) * 1081}
    for k in ("angle_min", "angle_increment", "range_min"):
        d[k] = torch.from_numpy(base[k]).to(dev)[idx].contiguous()
    d_ps, d_q, d_t, d_ss = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pose_stamp, q, t, scan_stamp))
    n = S * 1081
    torch.cuda.synchronize()
    out = {"scans": S, "rays": n, "poses": n_poses}
    with clc.Solver(0) as sv:
        def device_form():
            return sv.assemble_observations_device(n_poses, d_ps.data_ptr(), d_q.data_ptr(), d_t.data_ptr(), d["ranges"].data_ptr(),
                                                   d["offsets"].data_ptr(), S, n, d["angle_min"].data_ptr(), d["angle_increment"].data_ptr(),
                                                   d["range_min"].data_ptr(), d_ss.data_ptr())
        t0 = time.perf_counter(); info = device_form(); out["device_form_first_call_ms"] = (time.perf_counter() - t0) * 1e3
        out["info"] = {f[0]: int(getattr(info, f[0])) for f in info._fields_}
        for _ in range(a.warmup):
            device_form()
        tt = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); device_form(); tt.append(time.perf_counter() - t0)
        out["device_form"] = stats(tt)
        if not a.profile:
            got = sv.stored_observations()
            obs, scan_pose = host_route(sv, torch, d, n_poses, S, n, pose_stamp, q, t, scan_stamp, R)  # warm-up + the comparison
            same = (np.array_equal(got.pts_off, obs.pts_off) and got.pts.tobytes() == obs.pts.tobytes() and np.array_equal(got.ptl_off, obs.ptl_off))
            out["routes_agree"] = {"offsets_and_points_bitwise": bool(same),
                                   "max_abs_ptl": float(np.abs(got.ptl - obs.ptl).max()) if same and got.ptl.size else None,
                                   "max_abs_tag": float(max(np.abs(got.tag_q - obs.tag_q).max(), np.abs(got.tag_t - obs.tag_t).max())) if same and got.n_poses else None}
            tt = []
            for _ in range(a.route_reps):
                t0 = time.perf_counter(); host_route(sv, torch, d, n_poses, S, n, pose_stamp, q, t, scan_stamp, R); tt.append(time.perf_counter() - t0)
            out["host_route"] = stats(tt)
            tt = []
            for _ in range(max(3, a.reps // 2)):  # the device form again, after the route: the order of the legs does not decide
                t0 = time.perf_counter(); device_form(); tt.append(time.perf_counter() - t0)
            out["device_form_after"] = stats(tt)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
