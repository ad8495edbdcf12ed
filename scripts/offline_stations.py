"""clc_assemble_stations_device (K14) against the route the library offered before it for the same result
(profiles/offline_stations.md):
  device form   every input already in device memory -> the observations stored on the handle, one call;
  host route    the sequential restatement of GetStaticPose's walk and average in numpy on the host (tests/stations_ref.py),
                clc_scan_to_points_device + clc_board_segments_device, read-back of points / segments / status, scan -> station
                matching and the gather in numpy, calib.points_on_fitted_lines (clc_line_fit_batched + the end points),
                clc_store_observations.  The matching is a vectorised numpy search over the sorted station stamps: the route is
                timed at its best.
`--scans` scans of 1 081 rays (64 simulated scans tiled) against `--poses` stamped poses at 30 Hz: stations of 60 still frames
(0.2 mm / 2 mrad of jitter) with 20 moving frames in between.  Warm-up calls first (the first is reported apart), then `--reps`
timed calls, host clock around calls that end in a stream wait; medians with min / max.  Both results are compared before anything
is timed.  The stations alone (clc_static_poses, host arrays: upload + walk + averages + read-back) are timed too.
Kernel times: run with --profile under `rocprofv3 --kernel-trace --stats` (a run of its own: device form only).
--ground-truth: station mode and key-frame mode on the same jittered simoffline.station_recording, errors against the simulated
extrinsics.  Prints one JSON line."""
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
from camlasercalibratool_amd import simdata as sd, simoffline as so  # noqa: E402
from camlasercalibratool_amd.simdata import ObservationSet  # noqa: E402


def stats(v):
    v = np.asarray(v) * 1e3
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "n": int(v.size)}


def make_poses(n, seed=3, still=60, move=20):
    """Stations of `still` frames (0.2 mm, 2 mrad of jitter) and `move` frames on the way to the next one, 30 Hz."""
    rng = np.random.default_rng(seed)
    n_st = n // (still + move) + 2
    c = rng.uniform(-1.0, 1.0, (n_st, 3)); a = rng.uniform(-0.6, 0.6, (n_st, 3))
    k, ph = np.divmod(np.arange(n), still + move)
    f = np.clip((ph - still + 1) / (move + 1.0), 0.0, 1.0)[:, None]
    t = c[k] * (1 - f) + c[k + 1] * f + rng.normal(0, 0.0002, (n, 3))
    ang = a[k] * (1 - f) + a[k + 1] * f + rng.normal(0, 0.002, (n, 3))
    q = sd.rot_to_quat_wxyz(sd.rot_zyx(ang[:, 0], ang[:, 1], ang[:, 2])).reshape(n, 4)
    return 100.0 + np.arange(n) / 30.0, q, t


def host_route(sv, torch, d, S, n, pose_stamp, q, t, scan_stamp, SR):
    """-> (ObservationSet stored on the handle, scan_station)."""
    d_pts = torch.empty((n, 3), dtype=torch.float64, device=d["ranges"].device)
    d_seg = torch.empty((S, 2), dtype=torch.int64, device=d_pts.device)
    d_st = torch.empty((S,), dtype=torch.int32, device=d_pts.device)
    torch.cuda.synchronize()
    sv.scan_to_points_device(d["ranges"].data_ptr(), d["offsets"].data_ptr(), S, n, d["angle_min"].data_ptr(), d["angle_increment"].data_ptr(),
                             d["range_min"].data_ptr(), d_pts.data_ptr())
    sv.board_segments_device(d_pts.data_ptr(), d["offsets"].data_ptr(), S, d_seg.data_ptr(), d_st.data_ptr())
    P3, seg, status = d_pts.cpu().numpy(), d_seg.cpu().numpy(), d_st.cpu().numpy()
    w = SR.walk(t)
    a = SR.average(pose_stamp, q, t, w)
    start, end = a["start_time"], a["end_time"]  # increasing here, no two stations overlap
    i = np.clip(np.searchsorted(end, scan_stamp, side="left"), 0, max(len(end) - 1, 0))
    ok = (status == 1) & (len(end) > 0)
    if len(end):
        ok &= (start[i] <= scan_stamp) & (scan_stamp <= end[i]) & (a["status"][i] == 1)
    scan_station = np.where(status == 1, np.where(ok, i, -3), np.where(status == -1, -2, -1)).astype(np.int32)
    kept = np.nonzero(ok)[0]
    lens = seg[kept, 1] - seg[kept, 0] + 1
    pts_off = np.zeros(len(kept) + 1, dtype=np.int64)
    pts_off[1:] = np.cumsum(lens)
    first = kept * 1081 + seg[kept, 0]
    idx = np.repeat(first - pts_off[:-1], lens) + np.arange(int(pts_off[-1]))
    pts = np.ascontiguousarray(P3[idx])
    qk = a["q"][scan_station[kept]]
    qi = qk * np.array([1.0, -1.0, -1.0, -1.0]) / np.sum(qk * qk, axis=1, keepdims=True)
    ti = -np.einsum("nij,nj->ni", sd.quat_wxyz_to_rot(qi).reshape(-1, 3, 3), a["t"][scan_station[kept]])
    obs = ObservationSet(qi, ti, pts_off, pts, pts_off.copy(), pts)
    obs = clc.points_on_fitted_lines(obs, solver=sv)
    sv.store_observations(obs)
    return obs, scan_station


def ground_truth(sv):
    """Station mode and key-frame mode on the same jittered recording -> max |R - R_gt|, max |t - t_gt| of T_lc."""
    out = {}
    for sig_t, sig_r in ((2e-4, 1e-3), (5e-4, 5e-3)):
        rec = so.station_recording(1, pose_sigma_t=sig_t, pose_sigma_r=sig_r)
        args = (rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"])
        row = {}
        for name, fn in (("stations", clc.CalibrateOfflineStations), ("keyframes", clc.CalibrateOffline)):
            r = fn(*args, solver=sv, verbose=False)
            row[name] = None if r is None else {
                "observations": int(r["info"].n_observations), "err_R": float(np.abs(r["Tlc"][:3, :3] - sd.GT_RLC).max()),
                "err_t_m": float(np.abs(r["Tlc"][:3, 3] - sd.GT_TLC).max()), "iterations": int(r["report"].result.summary.num_iterations)}
        out[f"sigma_t={sig_t:g},sigma_r={sig_r:g}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=20000)
    ap.add_argument("--poses", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route-reps", type=int, default=2)
    ap.add_argument("--profile", action="store_true", help="device form only (for a run under rocprofv3)")
    ap.add_argument("--ground-truth", action="store_true", help="the two modes' errors on a jittered recording, nothing else")
    a = ap.parse_args()
    import torch
    import stations_ref as SR
    if a.ground_truth:
        with clc.Solver(0) as sv:
            print(json.dumps({"ground_truth": ground_truth(sv)}))
        return
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
            return sv.assemble_stations_device(n_poses, d_ps.data_ptr(), d_q.data_ptr(), d_t.data_ptr(), d["ranges"].data_ptr(),
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
            obs, scan_station = host_route(sv, torch, d, S, n, pose_stamp, q, t, scan_stamp, SR)  # warm-up + the comparison
            same = (np.array_equal(got.pts_off, obs.pts_off) and got.pts.tobytes() == obs.pts.tobytes() and np.array_equal(got.ptl_off, obs.ptl_off))
            out["routes_agree"] = {"offsets_and_points_bitwise": bool(same),
                                   "max_abs_ptl": float(np.abs(got.ptl - obs.ptl).max()) if same and got.ptl.size else None,
                                   "max_abs_tag": float(max(np.abs(got.tag_q - obs.tag_q).max(), np.abs(got.tag_t - obs.tag_t).max())) if same and got.n_poses else None}
            tt, tw = [], []
            for _ in range(a.route_reps):
                t0 = time.perf_counter(); host_route(sv, torch, d, S, n, pose_stamp, q, t, scan_stamp, SR); tt.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); w = SR.walk(t); SR.average(pose_stamp, q, t, w); tw.append(time.perf_counter() - t0)
            out["host_route"] = stats(tt)
            out["host_route_walk_and_average_alone"] = stats(tw)
            tt = []
            for _ in range(max(3, a.reps // 2)):  # the device form again, after the route: the order of the legs does not decide
                t0 = time.perf_counter(); device_form(); tt.append(time.perf_counter() - t0)
            out["device_form_after"] = stats(tt)
            sv.static_poses(pose_stamp, q, t)
            tt = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); sv.static_poses(pose_stamp, q, t); tt.append(time.perf_counter() - t0)
            out["static_poses_host_arrays"] = stats(tt)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
