"""clc_assemble_interpolated_device and clc_clock_offset_sweep_device (K15) against the routes the library offered before them
(profiles/offline_interpolated.md):
  assembly      `--scans` scans of 1 081 rays (64 simulated scans tiled) against `--poses` stamped poses at 30 Hz, every input already
                in device memory: clc_assemble_interpolated_device next to clc_assemble_observations_device (key frames) in the same
                run, and the host route — clc_scan_to_points_device + clc_board_segments_device, read-back, brackets by
                np.searchsorted and a vectorised slerp in numpy (the route at its best: the stamps are sorted), the gather in numpy,
                calib.points_on_fitted_lines, clc_store_observations.
  sweep         --sweep: `--offsets` candidates on simoffline.moving_recording's default shape (708 poses, ~940 scans):
                clc_clock_offset_sweep_device next to the host route — the restated decimated records per candidate in numpy
                (vectorised), then clc_upload + clc_solve per candidate.
  accuracy      --accuracy: the associations the library offers on the same moving recording with a clock offset of 7 ms, errors
                against the simulated extrinsics.
Warm-up calls first, then `--reps` timed calls, host clock around calls that end in a stream wait; medians with min / max.
Kernel times: run with --profile under `rocprofv3 --kernel-trace --stats` (a run of its own: device forms only).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import simdata as sd, simoffline as so  # noqa: E402
from camlasercalibratool_amd.simdata import ObservationSet  # noqa: E402


def stats(v):
    v = np.asarray(v) * 1e3
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "n": int(v.size)}


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    tt = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); tt.append(time.perf_counter() - t0)
    return stats(tt)


def make_poses(n, seed=3):
    """A smooth random path at 30 Hz."""
    rng = np.random.default_rng(seed)
    ang = np.cumsum(rng.normal(0, 0.01, (n, 3)), axis=0) * 0.1 + rng.uniform(-0.5, 0.5, 3)
    t = np.cumsum(rng.normal(0, 0.01, (n, 3)), axis=0)
    return 100.0 + np.arange(n) / 30.0, sd.rot_to_quat_wxyz(sd.rot_zyx(ang[:, 0], ang[:, 1], ang[:, 2])).reshape(n, 4), t


def np_interpolate(ps, q, t, x, max_gap=0.1):
    """Sorted stamps, unit quaternions: bracket by searchsorted, slerp / lerp vectorised -> (ok [m], q [m, 4], t [m, 3])."""
    i = np.clip(np.searchsorted(ps, x, side="left") - 1, 0, len(ps) - 2)
    gap = ps[i + 1] - ps[i]
    ok = (ps[i] <= x) & (x <= ps[i + 1]) & (gap > 0) & (gap <= max_gap)
    u = np.where(ok, (x - ps[i]) / np.where(gap > 0, gap, 1.0), 0.0)
    q0, q1 = q[i], q[i + 1]
    dot = np.sum(q0 * q1, axis=1)
    q1 = np.where(dot[:, None] < 0, -q1, q1)
    dot = np.abs(dot)
    th = np.arccos(np.minimum(dot, 1.0))
    s = np.sin(th)
    lin = dot > 1.0 - 1e-10
    s = np.where(lin, 1.0, s)
    w0 = np.where(lin, 1.0 - u, np.sin((1.0 - u) * th) / s)
    w1 = np.where(lin, u, np.sin(u * th) / s)
    qi = w0[:, None] * q0 + w1[:, None] * q1
    return ok, qi / np.linalg.norm(qi, axis=1, keepdims=True), t[i] + u[:, None] * (t[i + 1] - t[i])


def tag_poses(qk, tk):
    qi = qk * np.array([1.0, -1.0, -1.0, -1.0]) / np.sum(qk * qk, axis=1, keepdims=True)
    return qi, -np.einsum("nij,nj->ni", sd.quat_wxyz_to_rot(qi).reshape(-1, 3, 3), tk)


def device_front(sv, torch, d, S, n):
    d_pts = torch.empty((n, 3), dtype=torch.float64, device=d["ranges"].device)
    d_seg = torch.empty((S, 2), dtype=torch.int64, device=d_pts.device)
    d_st = torch.empty((S,), dtype=torch.int32, device=d_pts.device)
    torch.cuda.synchronize()
    sv.scan_to_points_device(d["ranges"].data_ptr(), d["offsets"].data_ptr(), S, n, d["angle_min"].data_ptr(), d["angle_increment"].data_ptr(),
                             d["range_min"].data_ptr(), d_pts.data_ptr())
    sv.board_segments_device(d_pts.data_ptr(), d["offsets"].data_ptr(), S, d_seg.data_ptr(), d_st.data_ptr())
    return d_pts.cpu().numpy(), d_seg.cpu().numpy(), d_st.cpu().numpy()


def host_assembly(sv, torch, d, S, n, rays, ps, q, t, ss):
    P3, seg, status = device_front(sv, torch, d, S, n)
    ok, qi, ti = np_interpolate(ps, q, t, ss)
    kept = np.nonzero(ok & (status == 1))[0]
    lens = seg[kept, 1] - seg[kept, 0] + 1
    pts_off = np.zeros(len(kept) + 1, dtype=np.int64)
    pts_off[1:] = np.cumsum(lens)
    first = kept * rays + seg[kept, 0]
    idx = np.repeat(first - pts_off[:-1], lens) + np.arange(int(pts_off[-1]))
    pts = np.ascontiguousarray(P3[idx])
    tq, tt = tag_poses(qi[kept], ti[kept])
    obs = clc.points_on_fitted_lines(ObservationSet(tq, tt, pts_off, pts, pts_off.copy(), pts), solver=sv)
    sv.store_observations(obs)
    return obs


def host_sweep(sv, torch, d, S, n, rays, ps, q, t, ss, x0, cands, m):
    """The restated records per candidate (numpy), then one clc_upload + clc_solve each -> final costs."""
    P3, seg, status = device_front(sv, torch, d, S, n)
    per = [np_interpolate(ps, q, t, ss + c) for c in cands]
    used = status == 1
    for ok, _, _ in per:
        used &= ok
    kept = np.nonzero(used)[0]
    L = seg[kept, 1] - seg[kept, 0] + 1
    take = np.where(L > m, m, L) if m > 0 else L
    off = np.zeros(len(kept) + 1, dtype=np.int64)
    off[1:] = np.cumsum(take)
    r = np.arange(int(off[-1])) - np.repeat(off[:-1], take)
    Lr, mr = np.repeat(L, take), np.repeat(take, take)
    p = np.where(mr < Lr, ((2 * r + 1) * Lr) // (2 * mr), r)
    pts = P3[np.repeat(kept * rays + seg[kept, 0], take) + p]
    scale = 1.0 / np.sqrt(np.repeat(take, take).astype(np.float64))
    cost = []
    for ok, qi, ti in per:
        tq, tt = tag_poses(qi[kept], ti[kept])
        nrm = sd.quat_wxyz_to_rot(tq).reshape(-1, 3, 3)[:, :, 2]
        dd = -np.sum(nrm * tt, axis=1)
        rec = np.ascontiguousarray(np.concatenate([np.repeat(nrm, take, axis=0), np.repeat(dd, take)[:, None], pts, scale[:, None]], axis=1))
        sv.upload(rec)
        cost.append(sv.solve(x0).summary.final_cost)
    return np.array(cost)


def to_dev(torch, dev, rec_scans):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in rec_scans.items()}


def accuracy(sv):
    rec = so.moving_recording(1, clock_offset=0.007)
    args = (rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"])
    every = clc.default_assemble_options(); every.keyframe_dist_min = -1.0  # every pose a key frame: the nearest of ALL poses within 20 ms
    rows = {"key frames + nearest within 20 ms": clc.CalibrateOffline(*args, solver=sv, verbose=False),
            "nearest of all poses within 20 ms": clc.CalibrateOffline(*args, assemble_options=every, solver=sv, verbose=False),
            "interpolated, offset 0": clc.CalibrateOfflineInterpolated(*args, time_offset=0.0, solver=sv, verbose=False),
            "interpolated, offset +7 ms": clc.CalibrateOfflineInterpolated(*args, time_offset=0.007, solver=sv, verbose=False),
            "interpolated, offset estimated": clc.CalibrateOfflineInterpolated(*args, time_offset="estimate", solver=sv, verbose=False)}
    out = {"poses": len(rec["pose_stamp"]), "scans": len(rec["scan_stamp"])}
    for name, r in rows.items():
        out[name] = None if r is None else {
            "observations": int(r["info"].n_observations), "final_cost": float(r["report"].result.summary.final_cost),
            "err_t_m": float(np.linalg.norm(r["Tlc"][:3, 3] - sd.GT_TLC)), "err_R": float(np.abs(r["Tlc"][:3, :3] - sd.GT_RLC).max()),
            "time_offset": r.get("time_offset")}
    sw = rows["interpolated, offset estimated"]["sweep"]
    out["sweep"] = {"offsets": sw["offsets"].tolist(), "final_cost": sw["final_cost"].tolist(), "best_offset": sw["best_offset"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=20000)
    ap.add_argument("--poses", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--route-reps", type=int, default=2)
    ap.add_argument("--offsets", type=int, default=41)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--profile", action="store_true", help="device forms only (for a run under rocprofv3)")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    out = {}
    with clc.Solver(0) as sv:
        if a.accuracy:
            out["accuracy"] = accuracy(sv)
        elif a.sweep:
            rec = so.moving_recording(1, clock_offset=0.007)
            ps, q, t, ss = rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scan_stamp"]
            S, n = len(ss), int(rec["scans"]["offsets"][-1])
            d = to_dev(torch, dev, rec["scans"])
            d_ps, d_q, d_t, d_ss = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (ps, q, t, ss))
            torch.cuda.synchronize()
            r0 = clc.CalibrateOfflineInterpolated(ps, q, t, rec["scans"], ss, time_offset=0.0, solver=sv, verbose=False)
            x0 = sd.pose7_from_T(np.linalg.inv(r0["Tlc_initial"]))
            o = clc.default_time_offset_options(); o.n_offsets = a.offsets
            dev_sweep = lambda: sv.time_offset_sweep_device(len(ps), d_ps.data_ptr(), d_q.data_ptr(), d_t.data_ptr(), d["ranges"].data_ptr(),
                                                            d["offsets"].data_ptr(), S, n, d["angle_min"].data_ptr(),
                                                            d["angle_increment"].data_ptr(), d["range_min"].data_ptr(), d_ss.data_ptr(), x0, o)
            res = dev_sweep()
            out.update({"poses": len(ps), "scans": S, "offsets": a.offsets, "scans_used": res["n_scans_used"],
                        "records_per_problem": res["records_per_problem"], "best_offset": res["best_offset"],
                        "iterations": [int(s.num_iterations) for s in res["summaries"]], "sweep_device": timed(dev_sweep, a.reps, 2)})
            if not a.profile:
                cost = host_sweep(sv, torch, d, S, n, 1081, ps, q, t, ss, x0, res["offsets"], o.points_per_scan)
                out["routes_agree_max_abs_cost"] = float(np.abs(cost - res["final_cost"]).max())
                out["sweep_host_route"] = timed(lambda: host_sweep(sv, torch, d, S, n, 1081, ps, q, t, ss, x0, res["offsets"], o.points_per_scan),
                                                a.route_reps, 0)
                out["sweep_device_after"] = timed(dev_sweep, max(3, a.reps // 2), 0)
        else:
            S, n_poses = a.scans, a.poses
            base = sd.sim_laser_scans(7, 64)
            ps, q, t = make_poses(n_poses)
            ss = np.sort(np.random.default_rng(5).uniform(ps[0], ps[-1], S))
            idx = torch.from_numpy((np.arange(S) * 7) % 64).to(dev)
            d = {"ranges": torch.from_numpy(base["ranges"].reshape(64, 1081)).to(dev)[idx].contiguous().reshape(-1),
                 "offsets": torch.arange(S + 1, dtype=torch.int64, device=dev) * 1081}
            for k in ("angle_min", "angle_increment", "range_min"):
                d[k] = torch.from_numpy(base[k]).to(dev)[idx].contiguous()
            d_ps, d_q, d_t, d_ss = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (ps, q, t, ss))
            n = S * 1081
            torch.cuda.synchronize()
            common = (n_poses, d_ps.data_ptr(), d_q.data_ptr(), d_t.data_ptr(), d["ranges"].data_ptr(), d["offsets"].data_ptr(), S, n,
                      d["angle_min"].data_ptr(), d["angle_increment"].data_ptr(), d["range_min"].data_ptr(), d_ss.data_ptr())
            interp = lambda: sv.assemble_interpolated_device(*common)
            keyfr = lambda: sv.assemble_observations_device(*common)
            out.update({"scans": S, "rays": n, "poses": n_poses})
            ik = keyfr(); out["keyframes_info"] = {f[0]: int(getattr(ik, f[0])) for f in ik._fields_}
            ii = interp(); out["interpolated_info"] = {f[0]: int(getattr(ii, f[0])) for f in ii._fields_}
            out["keyframes_device"] = timed(keyfr, a.reps, 2)
            out["interpolated_device"] = timed(interp, a.reps, 2)
            if not a.profile:
                got = sv.stored_observations()
                obs = host_assembly(sv, torch, d, S, n, 1081, ps, q, t, ss)
                same = np.array_equal(got.pts_off, obs.pts_off) and got.pts.tobytes() == obs.pts.tobytes()
                out["routes_agree"] = {"offsets_and_points_bitwise": bool(same),
                                       "max_abs_tag": float(max(np.abs(got.tag_q - obs.tag_q).max(), np.abs(got.tag_t - obs.tag_t).max())) if same else None}
                out["host_route"] = timed(lambda: host_assembly(sv, torch, d, S, n, 1081, ps, q, t, ss), a.route_reps, 0)
                out["interpolated_device_after"] = timed(interp, max(3, a.reps // 2), 0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
