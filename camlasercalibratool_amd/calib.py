"""Host-side mirror of the reference's call surface (include/LaseCamCalCeres.h:27-28):

    CamLaserCalClosedSolution(obs, Tlc)                          src/LaseCamCalCeres.cpp:112
    CamLaserCalibration(obs, Tcl, use_linefitting_data=True,
                        use_boundary_constraint=False)           src/LaseCamCalCeres.cpp:213

Same names, argument meaning and in/out conventions (4x4 matrices are modified in place, like
the Eigen::Matrix4d& of the reference); the bodies flatten the observations and call the HIP
library through the C-ABI.  Diagnostics the reference prints to stdout (summary, singular
values of H, null space, "recover chi2") are printed too and also returned."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from . import _capi, simdata
from ._capi import (AssembleOptions, ClcError, InterpOptions, Options, StationOptions, TimeOffsetOptions, default_interp_options,
                    default_time_offset_options, TERMINATION, default_line_options, default_options)
from .simdata import Oberserve, ObservationSet
from .solver import SolveResult, Solver, flatten_observations

ObsLike = Union[ObservationSet, Sequence[Oberserve]]


_shared: Optional[Solver] = None


def _shared_solver() -> Solver:
    """One solver context per process for the calls below (like the C++ drop-in header): creating a
    context costs milliseconds, the calls themselves a few hundred microseconds."""
    global _shared
    if _shared is None or _shared._h is None:
        _shared = Solver()
    return _shared


def _as_set(obs: ObsLike) -> ObservationSet:
    return obs if isinstance(obs, ObservationSet) else ObservationSet.from_list(list(obs))


@dataclass
class CalibrationReport:
    result: SolveResult
    H: np.ndarray
    b: np.ndarray
    chi2: float
    singular_values: np.ndarray
    null_space: np.ndarray  # [6, n_null]


class Session:
    """The observations of one calibration run resident on the GPU: the pose-major data of std::vector<Oberserve> (tag
    poses + scan points) is uploaded ONCE; closed form, refinement and the analysis pass — the sequence of
    main/calibr_offline.cpp:166-170 — then select their residual blocks on the device (clc_select_observations) instead
    of re-flattening and re-uploading 64-byte records per call.  The module-level functions below are one-call sessions."""

    def __init__(self, obs: Optional[ObsLike], solver: Optional[Solver] = None):
        """obs None: adopt the scans the solver's handle already holds (Solver.assemble_observations built them on the device) — no
        host copy is kept and nothing is uploaded; see Session.adopt."""
        self.sv = solver or _shared_solver()
        if obs is None:
            self.S = None
            self._generation = self.sv.store_generation
            if self._generation <= 0:
                raise ClcError(-5, "Session", "no scans stored on the solver's handle to adopt")
        else:
            self.S = _as_set(obs)
            self._store()

    @classmethod
    def adopt(cls, solver: Solver) -> "Session":
        """A session on the scans `solver` holds right now.  It keeps no host copy, so it cannot put them back: once another caller
        has replaced the stored scans every call of the session raises ClcError instead of solving somebody else's data."""
        return cls(None, solver)

    def _store(self):
        self.sv.store_observations(self.S)
        self._generation = self.sv.store_generation

    def _ensure_stored(self):
        """The stored scans belong to the (possibly shared) solver handle: if somebody else — another Session, one of the
        module-level calls below — stored theirs since, put ours back before selecting from them."""
        if self.sv.store_generation != self._generation:
            if self.S is None:
                raise ClcError(-5, "Session", "the scans this session adopted were replaced on the solver's handle (store generation "
                               f"{self._generation} -> {self.sv.store_generation}); it keeps no host copy to put back")
            self._store()

    def CamLaserCalClosedSolution(self, Tlc: np.ndarray, verbose: bool = True):
        """Closed-form initialiser; overwrites Tlc (camera->laser) like LaseCamCalCeres.cpp:198-200."""
        sv = self.sv
        self._ensure_stored()
        sv.select_observations(True, False)  # points_on_line only, :143
        T, unobservable, sv9 = sv.closed_form()
        if unobservable and verbose:  # :173-178
            print("\n~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~")
            print(" Notice Notice Notice: system unobservable !!!!!!!")
            print("~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~~\n")
        Tlc[...] = T
        if verbose:
            print("------- Closed-form solution Tlc: -------\n", Tlc)  # :202
        return unobservable, sv9

    def CamLaserCalibration(self, Tcl: np.ndarray, use_linefitting_data: bool = True, use_boundary_constraint: bool = False,
                            options: Optional[Options] = None, verbose: bool = True) -> CalibrationReport:
        """Nonlinear refinement; Tcl (laser->camera) is in/out like LaseCamCalCeres.cpp:215,:311-314."""
        sv = self.sv
        self._ensure_stored()
        n_rec = sv.select_observations(use_linefitting_data, use_boundary_constraint)
        pose0 = simdata.pose7_from_T(np.asarray(Tcl, dtype=np.float64))  # :215-219
        res = sv.solve(pose0, options)
        if verbose:  # stands in for summary.FullReport(), :309: the per-iteration table, then the totals
            print("iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius  step")
            for it in res.trace:
                print(f"{it.iteration:4d}  {it.cost:.6e}  {it.cost_change:9.2e}  {it.gradient_max_norm:9.2e}  {it.step_norm:9.2e}  "
                      f"{it.relative_decrease:9.2e}  {it.trust_region_radius:9.2e}  "
                      f"{'invalid' if not it.step_is_valid else ('accepted' if it.step_is_successful else 'rejected')}")
            s = res.summary
            print(f"Solver Summary: iterations {s.num_iterations} (successful {s.num_successful_steps - 1}, "
                  f"unsuccessful {s.num_unsuccessful_steps}), initial cost {s.initial_cost:.6e}, "
                  f"final cost {s.final_cost:.6e}, termination {TERMINATION.get(s.termination)}, "
                  f"residuals {n_rec}, passes {s.num_evaluations}, time {s.solve_ms:.3f} ms")
        Tcl[...] = simdata.T_from_pose7(res.pose)  # :311-314
        # analysis pass: no loss, no boundary terms (:316-362) — re-selected on the device, nothing crosses PCIe
        if use_boundary_constraint and use_linefitting_data:
            sv.select_observations(use_linefitting_data, False)
        H, b, chi2, svals, V, n_null = sv.information(res.pose)
        null = V[:, 6 - n_null:] if n_null > 0 else np.zeros((6, 0))
        if verbose:  # :365-381
            print("----- H singular values--------:")
            print(svals)
            if n_null > 0:
                print("====== null space basis, it's means the unobservable direction for Tcl ======")
                print("       please note the unobservable direction is for Tcl, not for Tlc        ")
                print(null)
            print("\nrecover chi2: ", chi2 / 2.0)
        return CalibrationReport(res, H, b, chi2, svals, null)


def CamLaserCalibrationFromStarts(obs: ObsLike, Tcls: np.ndarray, use_linefitting_data: bool = True, use_boundary_constraint: bool = False,
                                  options: Optional[Options] = None, solver: Optional[Solver] = None):
    """Multi-hypothesis refinement (mirror of clc_adapter::Session::CalibrationFromStarts): every Tcl of Tcls [S, 4, 4] refined on the SAME
    observations by clc_solve_multistart — a workgroup per start on ONE copy of the data.  Tcls is overwritten with the refined matrices;
    -> (index of the lowest final cost, final costs [S], summaries)."""
    S = _as_set(obs)
    sv = solver or _shared_solver()
    rec = flatten_observations(S, use_linefitting_data, use_boundary_constraint)
    sv.upload_batched(rec, np.array([0, rec.shape[0]], dtype=np.int64))
    T = np.asarray(Tcls, dtype=np.float64).reshape(-1, 4, 4)
    poses, sms = sv.solve_multistart(np.stack([simdata.pose7_from_T(t) for t in T]), options)
    for k in range(T.shape[0]):
        T[k] = simdata.T_from_pose7(poses[k])
    np.asarray(Tcls)[...] = T.reshape(np.asarray(Tcls).shape)
    costs = np.array([s.final_cost for s in sms])
    return int(np.argmin(costs)), costs, sms


def pose_block_offsets(obs: ObsLike, use_linefitting_data: bool = True, use_boundary_constraint: bool = False) -> np.ndarray:
    """Record offsets [P + 1] of flatten_observations' output, one block per Oberserve: its point rows, then (board-edge terms on) its
    two edge rows."""
    S = _as_set(obs)
    off = np.asarray(S.ptl_off if use_linefitting_data else S.pts_off, dtype=np.int64)
    extra = 2 if (use_boundary_constraint and use_linefitting_data) else 0
    out = np.zeros(S.n_poses + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.diff(off) + extra)
    return out


def _group_blocks(off: np.ndarray, block_offsets) -> np.ndarray:
    """Record offsets of blocks of consecutive observations: block_offsets [B + 1] in observations (None: one block per observation)."""
    if block_offsets is None:
        return off
    b = np.asarray(block_offsets, dtype=np.int64).reshape(-1)
    if b.size < 2 or b[0] != 0 or b[-1] != len(off) - 1 or np.any(np.diff(b) < 0):
        raise ValueError("block_offsets: [B + 1] non-decreasing observation indices from 0 to the number of observations")
    return np.ascontiguousarray(off[b])


def CamLaserCalibrationResample(obs: ObsLike, Tcl: np.ndarray, use_linefitting_data: bool = True, use_boundary_constraint: bool = False,
                                mode: str = "jackknife", n: int = 0, seed: int = 0, m: int = 0,
                                options: Optional[Options] = None, solver: Optional[Solver] = None, block_offsets=None) -> Dict[str, object]:
    """How much does Tcl depend on the poses that were recorded?  The full problem is solved from Tcl (refined in place), then — on the
    same upload, one launch (clc_solve_subsets) — its resampled versions from the full solution: mode "jackknife" (every pose left out
    once), "bootstrap" (n rows of P draws with replacement) or "subsets" (n random m-of-P subsets).
    -> {"pose": full solution [7], "summary", "weights" [S, P], "poses" [S, 7], "summaries", "deltas" [S, 6] (local coordinates of
    every resampled solution about the full one), "covariance" [6, 6] (jackknife / bootstrap estimate; None for "subsets"),
    "influence" [P] (jackknife only: |delta_k|, how far leaving pose k out moves the solution)}.
    block_offsets [B + 1] (optional): resample blocks of consecutive observations instead of single ones — the stations of
    CalibrateOfflineStations (its "station_block_offsets"), whose observations share one averaged tag pose; P is then B."""
    from . import resample
    S = _as_set(obs)
    sv = solver or _shared_solver()
    rec = flatten_observations(S, use_linefitting_data, use_boundary_constraint)
    off = _group_blocks(pose_block_offsets(S, use_linefitting_data, use_boundary_constraint), block_offsets)
    sv.upload_batched(rec, np.array([0, rec.shape[0]], dtype=np.int64))
    P = len(off) - 1
    full, fsm = sv.solve_multistart(simdata.pose7_from_T(np.asarray(Tcl, dtype=np.float64).reshape(4, 4))[None], options)
    x_full = full[0]
    if mode == "jackknife":
        W = resample.jackknife_weights(P)
    elif mode == "bootstrap":
        W = resample.bootstrap_weights(P, n, seed)
    elif mode == "subsets":
        W = resample.random_subset_weights(P, n, m, seed)
    else:
        raise ValueError("mode: 'jackknife', 'bootstrap' or 'subsets'")
    poses, sms = sv.solve_subsets(off, W, x_full, options)
    np.asarray(Tcl)[...] = simdata.T_from_pose7(x_full).reshape(np.asarray(Tcl).shape)
    D = resample.local_deltas(x_full, poses)
    cov = None
    if mode == "jackknife":
        cov = resample.jackknife_covariance(x_full, poses)
    elif mode == "bootstrap":
        cov = resample.bootstrap_covariance(x_full, poses)
    return {"pose": x_full, "summary": fsm[0], "weights": W, "poses": poses, "summaries": sms, "deltas": D, "covariance": cov,
            "influence": np.linalg.norm(D, axis=1) if mode == "jackknife" else None}


def CamLaserCalibrationConsensus(obs: ObsLike, Tcl: np.ndarray, use_linefitting_data: bool = True, use_boundary_constraint: bool = False,
                                 n: int = 256, m: int = 5, rms_max: Optional[float] = None, seed: int = 0,
                                 options: Optional[Options] = None, solver: Optional[Solver] = None, block_offsets=None) -> Dict[str, object]:
    """Calibration by consensus over the recorded poses: which recordings are bad, and the answer without them.  A whole scan can be
    consistently off by centimetres (its tag pose taken from the wrong camera frame, its board segment cut wrongly); the per-point
    Cauchy loss has its largest influence exactly there and all of that scan's points pull the same way.  Steps, on ONE upload:
      1. n random m-of-P subsets (resample.random_subset_weights(P, n, m, seed)) solved from Tcl          — solve_subsets, one launch
      2. every candidate scored against every pose: ssq [n, P]                                          — score_blocks, one launch
      3. resample.consensus_select(ssq, rms_max): the candidate most poses agree with, and those poses   — numpy
      4. one refit on the supporting poses only (the mask as weights), started at the winner            — solve_subsets, one launch
      5. the refit scored against every pose                                                            — score_blocks
    m defaults to 5: the reference refuses fewer than 5 observations (main/calibr_offline.cpp:158).
    rms_max (required) is the largest RMS point-to-plane distance, in metres, that a pose consistent with a candidate may show (with
    point rows only sqrt(ssq) is exactly that RMS).  Base it on the scanner's range noise: a few sigma — the tests use 3 sigma of the
    simulated noise.  A wrong recording must stand clear of it: at sigma = 0.01 m and rms_max = 0.03 m, poses 0.08 m off are
    separated exactly, poses 0.05 m off slip into the support and the refit is no better than the plain solve.
    Tcl is refined in place (left alone when no candidate finds support).
    -> {"pose" [7], "summary", "inliers" [P] bool, "rms" [P] (per-pose RMS at the result), "sizes" [n] (support of every candidate),
        "best" (the winning row; -1: none), "weights" [n, P], "candidates" [n, 7], "ssq" [n, P]}.
    block_offsets [B + 1] (optional): the blocks are runs of consecutive observations (stations, see CamLaserCalibrationResample)."""
    from . import resample
    if rms_max is None:
        raise TypeError("rms_max is required: a few sigma of the scanner's range noise, in metres (see the docstring)")
    S = _as_set(obs)
    sv = solver or _shared_solver()
    rec = flatten_observations(S, use_linefitting_data, use_boundary_constraint)
    off = _group_blocks(pose_block_offsets(S, use_linefitting_data, use_boundary_constraint), block_offsets)
    sv.upload_batched(rec, np.array([0, rec.shape[0]], dtype=np.int64))
    P = len(off) - 1
    x0 = simdata.pose7_from_T(np.asarray(Tcl, dtype=np.float64).reshape(4, 4))
    W = resample.random_subset_weights(P, n, m, seed)
    cands, _ = sv.solve_subsets(off, W, x0, options)
    ssq, _, _ = sv.score_blocks(off, cands, rms_max, options)
    best, mask, sizes = resample.consensus_select(ssq, rms_max)
    if best < 0:
        return {"pose": x0, "summary": None, "inliers": mask, "rms": np.full(P, np.nan), "sizes": sizes, "best": -1, "weights": W,
                "candidates": cands, "ssq": ssq}
    refit, sms = sv.solve_subsets(off, mask.astype(np.uint8)[None], cands[best], options)
    q, _, _ = sv.score_blocks(off, refit, rms_max, options)
    np.asarray(Tcl)[...] = simdata.T_from_pose7(refit[0]).reshape(np.asarray(Tcl).shape)
    return {"pose": refit[0], "summary": sms[0], "inliers": mask, "rms": np.sqrt(q[0]), "sizes": sizes, "best": best, "weights": W,
            "candidates": cands, "ssq": ssq}


def _upload_problems(sv: Solver, sets: Sequence[ObservationSet], use_linefitting_data: bool, use_boundary_constraint: bool):
    recs = [flatten_observations(S, use_linefitting_data, use_boundary_constraint) for S in sets]
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([r.shape[0] for r in recs])
    sv.upload_batched(np.concatenate(recs) if recs else np.zeros((0, 8)), off)


def CamLaserCalibrationBatch(problems: Sequence[ObsLike], use_linefitting_data: bool = True, use_boundary_constraint: bool = False,
                             options: Optional[Options] = None, solver: Optional[Solver] = None) -> Dict[str, np.ndarray]:
    """The reference's three steps (main/calibr_offline.cpp:166-170) for a list of independent problems, every step batched on the
    device: the closed form on the points_on_line records (clc_closed_form_batched), the solve from those starts in place on the
    handle's buffers (clc_solve_batched), the analysis pass on the solve's point set without board-edge terms
    (clc_information_batched).  With the default flags the three record sets are the same and one upload serves every step;
    otherwise the batch is uploaded again between the steps.  A problem whose closed form fails (status != 0: no records, a
    non-finite solution) starts from the identity pose.
    -> dict of per-problem arrays: Tlc_initial [P,4,4], unobservable [P], sv9 [P,9], closed_form_status [P], poses [P,7],
    Tcl [P,4,4], termination / num_iterations [P], initial_cost / final_cost [P], summaries (ctypes array), Tlc [P,4,4]
    (the inverse of Tcl), H [P,6,6], b [P,6], chi2 [P], sv [P,6], V [P,6,6], n_null [P]."""
    sets = [_as_set(p) for p in problems]
    sv = solver or _shared_solver()
    P = len(sets)
    if P == 0:
        raise ValueError("CamLaserCalibrationBatch: no problems")
    cf_same = use_linefitting_data and not use_boundary_constraint  # solve records == points_on_line records
    _upload_problems(sv, sets, True, False)  # :143, points_on_line only
    poses, _ = sv.batched_buffers()
    poses[...] = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    Tlc0, unobs, sv9, st, _ = sv.closed_form_batched(poses)
    start = poses.copy()
    if not cf_same:
        _upload_problems(sv, sets, use_linefitting_data, use_boundary_constraint)
        poses, _ = sv.batched_buffers()
        poses[...] = start
    poses, sms = sv.solve_batched_inplace(options)
    res = poses.copy()
    summaries = (type(sms[0]) * P)(*sms)
    if use_boundary_constraint:  # the analysis pass: no board-edge terms (:316-362)
        _upload_problems(sv, sets, use_linefitting_data, False)
    H, b, chi2, s6, V, nn = sv.information_batched(res)
    Tcl = np.stack([simdata.T_from_pose7(p) for p in res])
    return {
        "Tlc_initial": Tlc0, "unobservable": unobs, "sv9": sv9, "closed_form_status": st, "start_poses": start,
        "poses": res, "Tcl": Tcl, "Tlc": np.linalg.inv(Tcl), "summaries": summaries,
        "termination": np.array([s.termination for s in summaries], dtype=np.int32),
        "num_iterations": np.array([s.num_iterations for s in summaries], dtype=np.int32),
        "initial_cost": np.array([s.initial_cost for s in summaries]), "final_cost": np.array([s.final_cost for s in summaries]),
        "H": H, "b": b, "chi2": chi2, "sv": s6, "V": V, "n_null": nn,
    }


def CamLaserCalClosedSolution(obs: ObsLike, Tlc: np.ndarray, solver: Optional[Solver] = None, verbose: bool = True):
    """Closed-form initialiser; overwrites Tlc (camera->laser) like LaseCamCalCeres.cpp:198-200."""
    return Session(obs, solver).CamLaserCalClosedSolution(Tlc, verbose)


def CamLaserCalibration(obs: ObsLike, Tcl: np.ndarray, use_linefitting_data: bool = True,
                        use_boundary_constraint: bool = False, options: Optional[Options] = None,
                        solver: Optional[Solver] = None, verbose: bool = True) -> CalibrationReport:
    """Nonlinear refinement; Tcl (laser->camera) is in/out like LaseCamCalCeres.cpp:215,:311-314."""
    return Session(obs, solver).CamLaserCalibration(Tcl, use_linefitting_data, use_boundary_constraint, options, verbose)


def CalibrateOffline(pose_stamp, q_wc, t_wc, scans: dict, scan_stamp, assemble_options: Optional[AssembleOptions] = None,
                     options: Optional[Options] = None, solver: Optional[Solver] = None, verbose: bool = True):
    """The offline node, main/calibr_offline.cpp:51-175, from its two inputs: the stamped tag poses of apriltag_pose.txt (pose_stamp
    [n], q_wc [n, 4] (w, x, y, z), t_wc [n, 3]) and the laser scans (`scans` as simdata.sim_laser_scans returns them, scan_stamp [S]).
    Key frames, board segments, scan -> pose matching, line fits and the Oberserve records are built on the device
    (Solver.assemble_observations) and stay there; then the closed form on points_on_line (:167), Tcl = inv(Tlc) (:169) and
    CamLaserCalibration(obs, Tcl, false) with its analysis pass (:170).
    Returns None under the reference's gates — fewer than 10 poses (:56), fewer than 5 observations (:158) — otherwise
    {"Tlc_initial", "Tcl", "Tlc" [4, 4], "report" (CalibrationReport), "info" (AssembleInfo), "scan_pose" [S], "session"}."""
    if len(np.asarray(pose_stamp).reshape(-1)) < 10:
        if verbose:
            print("apriltag pose less than 10.")
        return None
    sv = solver or _shared_solver()
    info, scan_pose = sv.assemble_observations(pose_stamp, q_wc, t_wc, scans, scan_stamp, assemble_options)
    if info.n_observations < 5:
        if verbose:
            print("Valid Calibra Data Less")
        return None
    if verbose:
        print("obs size: ", info.n_observations)
    ses = Session.adopt(sv)
    Tlc0 = np.eye(4)
    ses.CamLaserCalClosedSolution(Tlc0, verbose)
    Tcl = np.linalg.inv(Tlc0)
    report = ses.CamLaserCalibration(Tcl, False, False, options, verbose)
    Tlc = np.linalg.inv(Tcl)
    if verbose:
        print("\n----- Transform from Camera to Laser Tlc is: -----\n")
        print(Tlc)
    return {"Tlc_initial": Tlc0, "Tcl": Tcl, "Tlc": Tlc, "report": report, "info": info, "scan_pose": scan_pose, "session": ses}


def GetStaticPose(pose_stamp, q_wc, t_wc, options: Optional[StationOptions] = None, solver: Optional[Solver] = None) -> dict:
    """The static stations of a pose list — mirror of GetStaticPose(Poses, avergeStaticPoses), src/utilities.cpp:86-155: the runs
    of poses that stay within 2 mm of their running centre, those of more than 30 members averaged into one pose each (mean
    translation; quaternion mean by the dominant eigenvector of sum q q^T) and stamped with the run's start_time / end_time.
    -> Solver.static_poses' dict; the member poses of station k are first[k] (twice, as in the reference) .. last[k]."""
    return (solver or _shared_solver()).static_poses(pose_stamp, q_wc, t_wc, options)


def station_block_offsets(scan_station: np.ndarray):
    """Observation ranges per station [B + 1] for the observations an assemble_stations call left (one per scan with
    scan_station >= 0, in scan order), one block per station that took a scan -> (offsets, the stations' indices), or
    (None, None) when the observations of a station are not consecutive (scan stamps that decrease)."""
    kept = np.asarray(scan_station)[np.asarray(scan_station) >= 0]
    if kept.size == 0 or np.any(np.diff(kept) < 0):
        return None, None
    ids, start = np.unique(kept, return_index=True)
    return np.concatenate([start, [kept.size]]).astype(np.int64), ids.astype(np.int64)


def CalibrateOfflineStations(pose_stamp, q_wc, t_wc, scans: dict, scan_stamp, station_options: Optional[StationOptions] = None,
                             options: Optional[Options] = None, solver: Optional[Solver] = None, verbose: bool = True):
    """CalibrateOffline for recordings where the board is held still at stations: the tag poses are averaged per station
    (GetStaticPose) and every scan taken while the board stood still becomes an observation with its station's averaged pose
    (Solver.assemble_stations) — no key frames, no 20 ms gate; then the closed form, Tcl = inv(Tlc), CamLaserCalibration(obs, Tcl,
    false) and its analysis pass as in main/calibr_offline.cpp:166-170.  The same gates: fewer than 10 poses, fewer than 5 observations.
    Returns None under the gates, otherwise CalibrateOffline's dict with "info" (StationInfo), "scan_station" [S] and
    "station_block_offsets" [B + 1] / "station_block_ids" [B]: the observation ranges of the stations that took scans — blocks for
    CamLaserCalibrationResample / CamLaserCalibrationConsensus (block_offsets=) — or None when a station's observations are not
    consecutive (scan stamps that decrease)."""
    if len(np.asarray(pose_stamp).reshape(-1)) < 10:
        if verbose:
            print("apriltag pose less than 10.")
        return None
    sv = solver or _shared_solver()
    info, scan_station = sv.assemble_stations(pose_stamp, q_wc, t_wc, scans, scan_stamp, station_options)
    if info.n_observations < 5:
        if verbose:
            print("Valid Calibra Data Less")
        return None
    if verbose:
        print("stations: ", info.n_stations, " obs size: ", info.n_observations)
    ses = Session.adopt(sv)
    Tlc0 = np.eye(4)
    ses.CamLaserCalClosedSolution(Tlc0, verbose)
    Tcl = np.linalg.inv(Tlc0)
    report = ses.CamLaserCalibration(Tcl, False, False, options, verbose)
    Tlc = np.linalg.inv(Tcl)
    if verbose:
        print("\n----- Transform from Camera to Laser Tlc is: -----\n")
        print(Tlc)
    blocks, ids = station_block_offsets(scan_station)
    return {"Tlc_initial": Tlc0, "Tcl": Tcl, "Tlc": Tlc, "report": report, "info": info, "scan_station": scan_station, "session": ses,
            "station_block_offsets": blocks, "station_block_ids": ids}


def CalibrateOfflineInterpolated(pose_stamp, q_wc, t_wc, scans: dict, scan_stamp, time_offset: Union[str, float] = "estimate",
                                 interp_options: Optional[InterpOptions] = None, sweep_options: Optional[TimeOffsetOptions] = None,
                                 options: Optional[Options] = None, solver: Optional[Solver] = None, verbose: bool = True):
    """CalibrateOffline for recordings where the board moves: every scan with a board segment becomes an observation with the tag
    pose interpolated at its stamp + time_offset (Solver.assemble_interpolated) — no key frames, no 20 ms gate; then the closed form,
    Tcl = inv(Tlc), CamLaserCalibration(obs, Tcl, false) and its analysis pass as in main/calibr_offline.cpp:166-170.
    time_offset: seconds to add to the laser's stamps to get camera time, or "estimate": the observations are first assembled at
    offset 0 for a closed-form start, Solver.time_offset_sweep (sweep_options; its interpolation settings are interp_options') runs
    from that start, and the assembly is repeated at the sweep's best_offset with all points.
    The same gates: fewer than 10 poses, fewer than 5 observations.  Returns None under the gates, otherwise CalibrateOffline's dict
    with "info" (AssembleInfo), "scan_bracket" [S], "scan_u" [S], "time_offset" (the offset used) and "sweep" (time_offset_sweep's
    dict — the table of offsets and final costs — or None)."""
    if len(np.asarray(pose_stamp).reshape(-1)) < 10:
        if verbose:
            print("apriltag pose less than 10.")
        return None
    sv = solver or _shared_solver()
    o = InterpOptions.from_buffer_copy(interp_options) if interp_options is not None else default_interp_options()
    sweep = None
    if isinstance(time_offset, str):
        if time_offset != "estimate":
            raise ValueError("CalibrateOfflineInterpolated: time_offset is a number of seconds or \"estimate\"")
        o.time_offset = 0.0
        info, _, _ = sv.assemble_interpolated(pose_stamp, q_wc, t_wc, scans, scan_stamp, o)
        if info.n_observations < 5:
            if verbose:
                print("Valid Calibra Data Less")
            return None
        Tlc_start = np.eye(4)
        Session.adopt(sv).CamLaserCalClosedSolution(Tlc_start, False)
        so = TimeOffsetOptions.from_buffer_copy(sweep_options) if sweep_options is not None else default_time_offset_options()
        so.interp = o
        if options is not None:
            so.solve = options
        sweep = sv.time_offset_sweep(pose_stamp, q_wc, t_wc, scans, scan_stamp, simdata.pose7_from_T(np.linalg.inv(Tlc_start)), so)
        if sweep["best_index"] < 0:
            if verbose:
                print("Valid Calibra Data Less")
            return None
        o.time_offset = float(sweep["best_offset"])
    else:
        o.time_offset = float(time_offset)
    info, scan_bracket, scan_u = sv.assemble_interpolated(pose_stamp, q_wc, t_wc, scans, scan_stamp, o)
    if info.n_observations < 5:
        if verbose:
            print("Valid Calibra Data Less")
        return None
    if verbose:
        print("time offset: ", o.time_offset, " obs size: ", info.n_observations)
    ses = Session.adopt(sv)
    Tlc0 = np.eye(4)
    ses.CamLaserCalClosedSolution(Tlc0, verbose)
    Tcl = np.linalg.inv(Tlc0)
    report = ses.CamLaserCalibration(Tcl, False, False, options, verbose)
    Tlc = np.linalg.inv(Tcl)
    if verbose:
        print("\n----- Transform from Camera to Laser Tlc is: -----\n")
        print(Tlc)
    return {"Tlc_initial": Tlc0, "Tcl": Tcl, "Tlc": Tlc, "report": report, "info": info, "scan_bracket": scan_bracket, "scan_u": scan_u,
            "time_offset": o.time_offset, "sweep": sweep, "session": ses}


def LineFittingCeres(Points: np.ndarray, Line: np.ndarray, solver: Optional[Solver] = None,
                     options: Optional[Options] = None) -> None:
    """Robust 2-parameter line fit of one scan, `Line` (m0, m1 of m0 x + m1 y + 1 = 0) in/out —
    mirror of LineFittingCeres(Points, Line), src/LaseCamCalCeres.cpp:401-433."""
    P = np.asarray(Points, dtype=np.float64).reshape(-1, 3)
    sv = solver or _shared_solver()
    lines, _ = sv.line_fit_batched(P[:, :2], np.array([0, P.shape[0]], dtype=np.int64),
                                   np.asarray(Line, dtype=np.float64).reshape(1, 2), options, want_summaries=False)

    Line[...] = lines[0]


def CalcCamPoses(camera, corners_px: Sequence[np.ndarray], board_xy: Sequence[np.ndarray], solver: Optional[Solver] = None,
                 options: Optional[Options] = None):
    """CamPoseEst::calcCamPose (src/calcCamPose.cpp:270-303) for many images at once, from detected corners: corners_px[k] [m_k, 2]
    pixels and board_xy[k] [m_k, 2] board-plane points of image k (camera: camera.Camera).  Returns (tag_q [n, 4] (w, x, y, z),
    tag_t [n, 3], status [n], rms [n]): T_ca = (R_cw, t_cw), the tagPose_Qca / tagPose_tca of Oberserve
    (main/calibr_offline.cpp:145-146); an image with status != CLC_POSE_OK (1) has no pose."""
    counts = [len(np.asarray(c).reshape(-1, 2)) for c in corners_px]
    if counts != [len(np.asarray(b).reshape(-1, 2)) for b in board_xy]:
        raise ValueError("CalcCamPoses: corners_px and board_xy differ in length")
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cat = lambda seq: (np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in seq]) if len(seq)
                       else np.zeros((0, 2), np.float32))
    sv = solver or _shared_solver()
    q, t, rms, st, _ = sv.board_poses(camera, cat(corners_px), cat(board_xy), off, options)
    return q, t, st, rms


def CornerSubPix(images, corners_px: Sequence[np.ndarray], win: int = 3, zero_zone: int = -1, max_iter: int = 30, eps: float = 0.1,
                 solver: Optional[Solver] = None):
    """cv::cornerSubPix as the reference calls it on every detection (src/calcCamPose.cpp:20-22: win 11 on the chessboard; :86-89: win 3
    on the Kalibr tag grid; TermCriteria(EPS + MAX_ITER, 30, 0.1)), for many images at once (clc_corner_subpix, K24): images uint8
    [n, H, W] grey, corners_px[k] [m_k, 2] the coarse corners of image k, e.g. the integer corners of a tag decoder.  Returns (refined,
    status, strength), one array per image: the refined float32 corners as CalcCamPoses takes them, the CLC_SUBPIX_* codes (1 converged,
    0 max_iter; < 0: -1 singular window, -2 left the image, -3 moved farther than the window and was put back, -4 non-finite start)
    and the smaller eigenvalue of the window's gradient matrix, to drop weak corners by."""
    counts = [len(np.asarray(c).reshape(-1, 2)) for c in corners_px]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cat = (np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in corners_px]) if len(corners_px)
           else np.zeros((0, 2), np.float32))
    o = _capi.SubpixOptions(win, win, zero_zone, zero_zone, max_iter, 0, eps)
    sv = solver or _shared_solver()
    r = sv.corner_subpix(images, cat, off, o)
    cut = lambda a: [a[off[k]:off[k + 1]] for k in range(len(counts))]
    return cut(r["corners"]), cut(r["status"]), cut(r["strength"])


def FindChessboardCorners(images, pattern_size, square_size: float, refine_win: int = 11, max_iter: int = 30, eps: float = 0.1,
                          chess_options=None, order_options=None, solver: Optional[Solver] = None, ordering: str = "host"):
    """The front of CamPoseEst::chessBoardPose (src/calcCamPose.cpp:10-47: cv::findChessboardCorners, cornerSubPix at half-window 11,
    p3ds = (j square, i square, 0) row by row) for many images at once (clc_find_chessboard, K25 + K24): images uint8 [n, H, W] grey,
    pattern_size = (cols, rows) inner corners.  Returns (corners_px, board_xy, found): per image the refined float32 corners
    [cols rows, 2] (NaN where no board was found; refine_win 0: the detector's integer pixels), the board points (j square, i square)
    in the same order, and found [n] bool — corners_px[found] and board_xy[found] are ready for CalcCamPoses, CalibrateCamera and
    CalibrateFull.  The board is taken to be seen from its front; which of the two (square pattern: four) labelings a half turn apart
    is returned is decided by position (node (0, 0) first in raster order), not by the squares' colour, as with OpenCV.
    ordering="device" runs the ordering on the device as well (clc_find_chessboard_gpu, K26): the same arrays, without the read-back
    and the host core between detection and refinement."""
    cols, rows = int(pattern_size[0]), int(pattern_size[1])
    sv = solver or _shared_solver()
    so = _capi.SubpixOptions(refine_win, refine_win, -1, -1, max_iter, 0, eps) if refine_win > 0 else None
    r = sv.find_chessboard(images, cols, rows, chess_options, order_options, so, ordering=ordering)
    gx, gy = np.meshgrid(np.arange(cols), np.arange(rows))
    board = np.stack([gx.ravel() * square_size, gy.ravel() * square_size], 1).astype(np.float32)
    n = len(r["found"])
    return [r["corners"][k] for k in range(n)], [board.copy() for _ in range(n)], r["found"]


def FindTagGridCorners(images, grid_size, tag_size: float, tag_spacing: float, family, refine_win: int = 3, max_iter: int = 30,
                       eps: float = 0.1, tag_options=None, chess_options=None, solver: Optional[Solver] = None):
    """The front of CamPoseEst's Kalibr branch (src/calcCamPose.cpp:48-139: the tag detector, cornerSubPix at half-window 3, the board
    points by tag id) for many images at once (clc_tag_grid, K27 + K24): images uint8 [n, H, W] grey, grid_size = (cols, rows) tags,
    tag id = row cols + col, `family` a solver.TagFamily (the board's code table: this package ships none).  Returns (corners_px,
    board_xy, tag_ids), one array per image: the corners [4 m_k, 2] float32 of the m_k tags seen, in id order and within a tag in the
    order of the reference's detector (counter-clockwise on the upright printed tag from its bottom-left corner), refined at half-window
    refine_win (0: the integer pixels); their board points (X0, Y0), (X0 + a, Y0), (X0 + a, Y0 + a), (X0, Y0 + a) with
    (X0, Y0) = (col, row) tag_size (1 + tag_spacing); and the ids [m_k].  The lists go straight into CalcCamPoses, CalibrateCamera and
    CalibrateFull; a board cut by the image border gives the tags fully in view."""
    cols, rows = int(grid_size[0]), int(grid_size[1])
    sv = solver or _shared_solver()
    so = _capi.SubpixOptions(refine_win, refine_win, -1, -1, max_iter, 0, eps) if refine_win > 0 else None
    r = sv.tag_grid(images, family, cols, rows, tag_options, chess_options, so)
    period = tag_size * (1.0 + tag_spacing)
    corners_px, board_xy, tag_ids = [], [], []
    for k in range(len(r["count"])):
        ids = np.flatnonzero(r["hamming"][k] >= 0)
        x0, y0 = (ids % cols) * period, (ids // cols) * period
        b = np.stack([np.stack([x0, y0], 1), np.stack([x0 + tag_size, y0], 1), np.stack([x0 + tag_size, y0 + tag_size], 1),
                      np.stack([x0, y0 + tag_size], 1)], 1)
        corners_px.append(r["corners"][k, ids].reshape(-1, 2))
        board_xy.append(b.reshape(-1, 2).astype(np.float32))
        tag_ids.append(ids.astype(np.int32))
    return corners_px, board_xy, tag_ids


def CalcCamPosesRobust(camera, corners_px: Sequence[np.ndarray], board_xy: Sequence[np.ndarray], solver: Optional[Solver] = None,
                       options: Optional[Options] = None, robust=None):
    """CalcCamPoses with a consensus over the tags of every image ahead of the fit (clc_board_poses_robust, K16): a tag decoded with a
    wrong id or a mis-refined corner is left out of the fit instead of bending the pose.  corners_px[k] must list its tags four
    corners at a time (the order FindTargetCorner emits them).  robust: _capi.RobustPoseOptions (None: 8 px / 2 px gates over the
    focal length).  Returns (tag_q [n, 4], tag_t [n, 3], status [n] (1 = pose, -3 = no consensus), rms [n], inlier_masks (one bool array
    per image), info {"n_inliers", "best_group", "n_fits"})."""
    counts = [len(np.asarray(c).reshape(-1, 2)) for c in corners_px]
    if counts != [len(np.asarray(b).reshape(-1, 2)) for b in board_xy]:
        raise ValueError("CalcCamPosesRobust: corners_px and board_xy differ in length")
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cat = lambda seq: (np.concatenate([np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in seq]) if len(seq)
                       else np.zeros((0, 2), np.float32))
    sv = solver or _shared_solver()
    q, t, rms, st, _, inl, ni, bg, nf = sv.board_poses_robust(camera, cat(corners_px), cat(board_xy), off, options, robust)
    masks = [inl[off[k]:off[k + 1]] for k in range(len(counts))]
    return q, t, st, rms, masks, {"n_inliers": ni, "best_group": bg, "n_fits": nf}


def checked_poses(q, t, status, alt):
    """The host half of BoardPosesChecked from the outputs of the two calls (alt: the dict of Solver.board_poses_alternate): the
    lower-cost solution where `better`, and keep = status OK and not ambiguous.  -> (q [n, 4], t [n, 3], keep [n] bool)"""
    q, t = np.array(q, dtype=np.float64, copy=True), np.array(t, dtype=np.float64, copy=True)
    swap = np.asarray(alt["better"], dtype=bool)
    q[swap], t[swap] = alt["q"][swap], alt["t"][swap]
    keep = (np.asarray(status) == 1) & ~np.asarray(alt["ambiguous"], dtype=bool)
    return q, t, keep


def BoardPosesChecked(camera, corners, board, offsets, robust: bool = True, ratio_gate: float = 2.0, solver: Optional[Solver] = None):
    """Board poses with the planar ambiguity checked (K17): clc_board_poses_robust (robust=False: clc_board_poses) and then
    clc_board_poses_alternate on its poses and mask.  corners [M, 2] pixels, board [M, 2] board-plane points, CSR offsets [n+1].
    Returns (q [n, 4] (w, x, y, z), t [n, 3], status [n], keep [n] bool, table): where the other minimum has the lower cost (`better`)
    it is the pose returned; keep = status OK and not ambiguous (the mirror pose does not fit within ratio_gate of the cost) — the mask
    to select the images fed to CalibrateOffline*; table: the per-image dict of Solver.board_poses_alternate plus "rms" of the first
    call as "rms_in" and, with robust, "inlier", "n_inliers"."""
    from ._capi import default_alt_pose_options
    sv = solver or _shared_solver()
    ao = default_alt_pose_options()
    ao.ratio_gate = float(ratio_gate)
    extra = {}
    if robust:
        q, t, rms, st, _, inl, ni, _, _ = sv.board_poses_robust(camera, corners, board, offsets)
        extra = {"inlier": inl, "n_inliers": ni}
    else:
        q, t, rms, st, _ = sv.board_poses(camera, corners, board, offsets)
        inl = None
    alt = sv.board_poses_alternate(camera, corners, board, offsets, q, t, st, inlier=inl, alt=ao)
    q2, t2, keep = checked_poses(q, t, st, alt)
    return q2, t2, st, keep, dict(alt, rms_in=rms, **extra)


def _joint_arrays(corners_px, board_xy, sets: Sequence[ObservationSet], use_linefitting_data: bool):
    """The CSR arrays of Solver.joint_refine over a list of problems: corners_px / board_xy one list of per-image arrays per problem."""
    imgs_c = [np.asarray(c, np.float32).reshape(-1, 2) for prob in corners_px for c in prob]
    imgs_b = [np.asarray(b, np.float32).reshape(-1, 2) for prob in board_xy for b in prob]
    co = np.concatenate([[0], np.cumsum([len(c) for c in imgs_c])]).astype(np.int64)
    pts, po = [], [0]
    for s in sets:
        off, P = (s.ptl_off, s.ptl) if use_linefitting_data else (s.pts_off, s.pts)
        pts.append(P[off[0]:off[-1]])
        po += list(po[-1] + (off[1:] - off[0]))
    pr = np.concatenate([[0], np.cumsum([s.n_poses for s in sets])]).astype(np.int64)
    if not (len(imgs_c) == len(imgs_b) == pr[-1]) or any(len(c) != len(b) for c, b in zip(imgs_c, imgs_b)):
        raise ValueError("CamLaserCalibrationJoint: one image (corners and as many board points) per pose of the observation set")
    cat = lambda xs, w, dt: np.concatenate(xs) if len(xs) else np.zeros((0, w), dt)
    return (cat(imgs_c, 2, np.float32), cat(imgs_b, 2, np.float32), co, cat(pts, 3, np.float64), np.asarray(po, np.int64), pr,
            cat([s.tag_q for s in sets], 4, np.float64), cat([s.tag_t for s in sets], 3, np.float64))


def CamLaserCalibrationJointBatch(camera, problems: Sequence[dict], use_linefitting_data: bool = False, sigma_px: float = 0.3,
                                  sigma_laser: float = 0.01, solver: Optional[Solver] = None, options: Optional[Options] = None):
    """CamLaserCalibrationJoint for a list of problems in one call (one workgroup each): every problem a dict(corners_px, board_xy — one
    array per image —, obs, Tcl [4, 4], keep (optional)).  -> list of (Tcl, ObservationSet, report)."""
    sv = solver or _shared_solver()
    sets = [_as_set(p["obs"]) for p in problems]
    cp, bx, co, pts, po, pr, q0, t0 = _joint_arrays([p["corners_px"] for p in problems], [p["board_xy"] for p in problems], sets,
                                                    use_linefitting_data)
    keep = None
    if any(p.get("keep") is not None for p in problems):
        keep = np.concatenate([np.ones(s.n_poses, bool) if p.get("keep") is None else np.asarray(p["keep"], bool) for p, s in zip(problems, sets)])
    jo = _capi.default_joint_options(camera)
    jo.sigma_corner = sigma_px / float(np.sqrt(abs(camera.proj[0] * camera.proj[1])))
    jo.sigma_laser = sigma_laser
    cl0 = np.stack([simdata.pose7_from_T(np.asarray(p["Tcl"], np.float64)) for p in problems]) if problems else np.zeros((0, 7))
    r = sv.joint_refine(camera, cp, bx, co, pts, po, q0, t0, cl0, problem_offsets=pr, keep=keep, options=options, joint=jo)
    out = []
    for k, s in enumerate(sets):
        sl = slice(pr[k], pr[k + 1])
        H = r["H_cl"][k]
        report = dict(summary=r["summaries"][k], termination=_capi.TERMINATION.get(r["summaries"][k].termination, "?"), H_cl=H,
                      singular_values=np.linalg.svd(H, compute_uv=False) if np.all(np.isfinite(H)) else np.full(6, np.nan),
                      cost_corner=float(r["cost_parts"][k, 0]), cost_laser=float(r["cost_parts"][k, 1]), status=r["status"][sl].copy())
        refined = ObservationSet(r["q"][sl].copy(), r["t"][sl].copy(), s.pts_off, s.pts, s.ptl_off, s.ptl)
        out.append((simdata.T_from_pose7(r["poses_cl"][k]), refined, report))
    return out


def CamLaserCalibrationJoint(camera, corners_px: Sequence[np.ndarray], board_xy: Sequence[np.ndarray], obs: ObsLike, Tcl: np.ndarray,
                             use_linefitting_data: bool = False, keep=None, sigma_px: float = 0.3, sigma_laser: float = 0.01,
                             solver: Optional[Solver] = None, options: Optional[Options] = None):
    """Joint refinement of the board poses and T_cl (K18): image i belongs to pose i of `obs` — its start pose is that pose's tag pose,
    its laser points that pose's `points` (or `points_on_line`).  Minimises the corner reprojection error over sigma_px (pixels) plus
    the laser point-to-board-plane distance over sigma_laser (metres) over T_cl and every board pose.
    -> (Tcl [4, 4], the observation set with the refined tag poses, report: summary, termination, H_cl — the information on T_cl
    with the board poses marginalised —, its singular_values, cost_corner, cost_laser, status per image)."""
    return CamLaserCalibrationJointBatch(camera, [dict(corners_px=corners_px, board_xy=board_xy, obs=obs, Tcl=Tcl, keep=keep)],
                                         use_linefitting_data, sigma_px, sigma_laser, solver, options)[0]


def CamLaserCalibrationJointRobustBatch(camera, problems: Sequence[dict], use_linefitting_data: bool = False, sigma_px: float = 0.3,
                                        sigma_laser: float = 0.01, solver: Optional[Solver] = None, options: Optional[Options] = None,
                                        loss_px_sigmas: float = 3.0, loss_laser_m: float = 0.05):
    """CamLaserCalibrationJointRobust for a list of problems in one call (one workgroup each): the problems of
    CamLaserCalibrationJointBatch.  -> list of (Tcl, ObservationSet, report)."""
    sv = solver or _shared_solver()
    sets = [_as_set(p["obs"]) for p in problems]
    cp, bx, co, pts, po, pr, q0, t0 = _joint_arrays([p["corners_px"] for p in problems], [p["board_xy"] for p in problems], sets,
                                                    use_linefitting_data)
    keep = None
    if any(p.get("keep") is not None for p in problems):
        keep = np.concatenate([np.ones(s.n_poses, bool) if p.get("keep") is None else np.asarray(p["keep"], bool) for p, s in zip(problems, sets)])
    jo = _capi.default_joint_options(camera)
    jo.sigma_corner = sigma_px / float(np.sqrt(abs(camera.proj[0] * camera.proj[1])))
    jo.sigma_laser = sigma_laser
    lo = _capi.JointLossOptions(float(loss_px_sigmas), float(loss_laser_m) / float(sigma_laser))
    cl0 = np.stack([simdata.pose7_from_T(np.asarray(p["Tcl"], np.float64)) for p in problems]) if problems else np.zeros((0, 7))
    r = sv.joint_refine_robust(camera, cp, bx, co, pts, po, q0, t0, cl0, problem_offsets=pr, keep=keep, options=options, joint=jo, loss=lo)
    out = []
    for k, s in enumerate(sets):
        sl = slice(pr[k], pr[k + 1])
        H = r["H_cl"][k]
        w_corner = [r["w_corner"][co[i]:co[i + 1]].copy() for i in range(pr[k], pr[k + 1])]
        w_laser = [r["w_laser"][po[i]:po[i + 1]].copy() for i in range(pr[k], pr[k + 1])]
        report = dict(summary=r["summaries"][k], termination=_capi.TERMINATION.get(r["summaries"][k].termination, "?"), H_cl=H,
                      singular_values=np.linalg.svd(H, compute_uv=False) if np.all(np.isfinite(H)) else np.full(6, np.nan),
                      cost_corner=float(r["cost_parts"][k, 0]), cost_laser=float(r["cost_parts"][k, 1]), status=r["status"][sl].copy(),
                      w_corner=w_corner, w_laser=w_laser, inlier_corner=[w >= 0.5 for w in w_corner], inlier_laser=[w >= 0.5 for w in w_laser])
        refined = ObservationSet(r["q"][sl].copy(), r["t"][sl].copy(), s.pts_off, s.pts, s.ptl_off, s.ptl)
        out.append((simdata.T_from_pose7(r["poses_cl"][k]), refined, report))
    return out


def CamLaserCalibrationJointRobust(camera, corners_px: Sequence[np.ndarray], board_xy: Sequence[np.ndarray], obs: ObsLike, Tcl: np.ndarray,
                                   use_linefitting_data: bool = False, keep=None, sigma_px: float = 0.3, sigma_laser: float = 0.01,
                                   solver: Optional[Solver] = None, options: Optional[Options] = None, loss_px_sigmas: float = 3.0,
                                   loss_laser_m: float = 0.05):
    """CamLaserCalibrationJoint under a Cauchy loss per corner and per laser point (K22): a single bad laser point inside a board
    segment (a leg or a cable in front of the board, the mixed pixel at a board edge) or a single mis-refined corner is
    down-weighted instead of biasing T_cl.  loss_laser_m: the Cauchy scale of a laser residual in metres (0.05: the reference's
    CauchyLoss(0.05)); loss_px_sigmas: the scale of a corner's residual vector in units of sigma_px (3: a design value of this
    library, 0.9 px at 0.3 px); 0: no loss on that term.
    -> (Tcl [4, 4], the observation set with the refined tag poses, report: CamLaserCalibrationJoint's — cost_corner, cost_laser and
    the summary's costs are the robust ones — and per image w_corner, w_laser (rho' of every observation at the returned poses; NaN
    for an image that takes no part) and the masks inlier_corner, inlier_laser (w >= 0.5: |residual| within the loss scale))."""
    return CamLaserCalibrationJointRobustBatch(camera, [dict(corners_px=corners_px, board_xy=board_xy, obs=obs, Tcl=Tcl, keep=keep)],
                                               use_linefitting_data, sigma_px, sigma_laser, solver, options, loss_px_sigmas,
                                               loss_laser_m)[0]


def _range_hold_mask(hold) -> int:
    """hold: None, a mask 0..3, or names out of ("offset", "scale")."""
    if hold is None:
        return 0
    if isinstance(hold, (int, np.integer)):
        return int(hold)
    names = {"offset": 1, "scale": 2}
    return sum(names[str(h)] for h in set(hold))


def CamLaserCalibrationRangeBatch(camera, problems: Sequence[dict], use_linefitting_data: bool = False, hold=None,
                                  hold_board_poses: bool = False, hold_extrinsic: bool = False, sigma_px: float = 0.3,
                                  sigma_laser: float = 0.01, solver: Optional[Solver] = None, options: Optional[Options] = None):
    """CamLaserCalibrationRange for a list of problems in one call (one workgroup each): every problem a dict(corners_px, board_xy —
    one array per image; None with hold_board_poses —, obs, Tcl [4, 4], range0 (optional, (offset, scale)), keep (optional)).
    -> list of (Tcl, ObservationSet, report)."""
    sv = solver or _shared_solver()
    sets = [_as_set(p["obs"]) for p in problems]
    with_corners = not (hold_board_poses and all(p.get("corners_px") is None for p in problems))
    if with_corners:
        cp, bx, co, pts, po, pr, q0, t0 = _joint_arrays([p["corners_px"] for p in problems], [p["board_xy"] for p in problems], sets,
                                                        use_linefitting_data)
    else:
        empty = [[np.zeros((0, 2), np.float32)] * s.n_poses for s in sets]
        _, _, _, pts, po, pr, q0, t0 = _joint_arrays(empty, empty, sets, use_linefitting_data)
        cp = bx = co = None
    keep = None
    if any(p.get("keep") is not None for p in problems):
        keep = np.concatenate([np.ones(s.n_poses, bool) if p.get("keep") is None else np.asarray(p["keep"], bool) for p, s in zip(problems, sets)])
    ro = _capi.default_range_options(camera)
    if camera is not None:
        ro.sigma_corner = sigma_px / float(np.sqrt(abs(camera.proj[0] * camera.proj[1])))
    ro.sigma_laser = sigma_laser
    ro.hold_board_poses, ro.hold_extrinsic, ro.hold_range_mask = int(bool(hold_board_poses)), int(bool(hold_extrinsic)), _range_hold_mask(hold)
    cl0 = np.stack([simdata.pose7_from_T(np.asarray(p["Tcl"], np.float64)) for p in problems]) if problems else np.zeros((0, 7))
    r0 = np.array([(0.0, 0.0) if p.get("range0") is None else p["range0"] for p in problems], np.float64).reshape(len(problems), 2)
    r = sv.joint_refine_range(camera, cp, bx, co, pts, po, q0, t0, cl0, range0=r0, problem_offsets=pr, keep=keep, options=options,
                              range_options=ro)
    free = np.array([not hold_extrinsic] * 6 + [not (ro.hold_range_mask >> j) & 1 for j in range(2)])
    out = []
    for k, s in enumerate(sets):
        sl = slice(pr[k], pr[k + 1])
        H = r["H_cr"][k]
        sigma, corr = np.full(8, np.nan), np.full(3, np.nan)
        fi = np.flatnonzero(free)
        if np.all(np.isfinite(H)) and len(fi):
            try:
                cov = np.linalg.inv(H[np.ix_(fi, fi)])
                if np.all(np.diag(cov) > 0):
                    sigma[fi] = np.sqrt(np.diag(cov))
                    if free[6] and not hold_extrinsic:
                        full = np.zeros((8, 8))
                        full[np.ix_(fi, fi)] = cov
                        corr = full[6, :3] / (sigma[6] * sigma[:3])
            except np.linalg.LinAlgError:
                pass
        report = dict(summary=r["summaries"][k], termination=_capi.TERMINATION.get(r["summaries"][k].termination, "?"),
                      range_offset=float(r["range"][k, 0]), range_scale=float(r["range"][k, 1]), H_cr=H,
                      singular_values=np.linalg.svd(H, compute_uv=False) if np.all(np.isfinite(H)) else np.full(8, np.nan),
                      sigma=sigma, corr_offset_tcl=corr, cost_corner=float(r["cost_parts"][k, 0]), cost_laser=float(r["cost_parts"][k, 1]),
                      status=r["status"][sl].copy())
        refined = ObservationSet(r["q"][sl].copy(), r["t"][sl].copy(), s.pts_off, s.pts, s.ptl_off, s.ptl)
        out.append((simdata.T_from_pose7(r["poses_cl"][k]), refined, report))
    return out


def CamLaserCalibrationRange(camera, corners_px, board_xy, obs: ObsLike, Tcl: np.ndarray, range0=(0.0, 0.0), hold=None,
                             hold_board_poses: bool = False, hold_extrinsic: bool = False, use_linefitting_data: bool = False, keep=None,
                             sigma_px: float = 0.3, sigma_laser: float = 0.01, solver: Optional[Solver] = None,
                             options: Optional[Options] = None):
    """CamLaserCalibrationJoint with the scanner's range offset b (metres) and range scale kappa (K21): the laser points enter the
    cost corrected along their rays, p' = (1 + kappa + b / |p|) p, i.e. true range = (1 + kappa) measured + b.  range0: the start;
    hold: None, or out of ("offset", "scale") (or the mask: bit 0 offset, bit 1 scale) — a held parameter keeps range0's value and
    is still applied.  With hold_board_poses the tag poses of `obs` stay and camera, corners_px and board_xy may be None: T_cl and
    the range parameters from tag poses and points alone.
    -> (Tcl [4, 4], the observation set with the refined tag poses (the points as measured: ApplyRangeCorrection corrects them),
    report: summary, termination, range_offset, range_scale, H_cr — the information on [T_cl tangent, b, kappa] with the board poses
    marginalised —, its singular_values, sigma (1 sigma of the 8 parameters from the inverse of H_cr over the free ones, NaN for a
    held one), corr_offset_tcl (the correlation of b with t_cl), cost_corner, cost_laser, status per image).
    Observability: b and kappa separate only through a spread of ranges, b separates from t_cl only through a spread of plane
    normals and ray directions.  singular_values and sigma show when to hold one of them; a recording at a single range cannot have
    both free (the damping keeps the solve finite there, and sigma comes back NaN or huge)."""
    return CamLaserCalibrationRangeBatch(camera, [dict(corners_px=corners_px, board_xy=board_xy, obs=obs, Tcl=Tcl, range0=range0, keep=keep)],
                                         use_linefitting_data, hold, hold_board_poses, hold_extrinsic, sigma_px, sigma_laser, solver,
                                         options)[0]


def ApplyRangeCorrection(obs: ObsLike, offset: float, scale: float, solver: Optional[Solver] = None) -> ObservationSet:
    """The observation set with `points` and `points_on_line` corrected for the scanner's range offset and scale (clc_range_correct):
    upload, closed form, CamLaserCalibration, K18 and the pose guidance then run on corrected data."""
    sv = solver or _shared_solver()
    s = _as_set(obs)
    return ObservationSet(s.tag_q.copy(), s.tag_t.copy(), s.pts_off.copy(), sv.range_correct(s.pts, offset, scale), s.ptl_off.copy(),
                          sv.range_correct(s.ptl, offset, scale))


@dataclass
class GuidanceReport:
    """What SuggestBoardPoses returns; indices in the caller's numbering of the candidates."""
    chosen: np.ndarray        # [k] int64, in the order chosen, -1 padded
    sv_after: np.ndarray      # [k, 6] eigenvalues of H after each round (NaN in the padding)
    score_after: np.ndarray   # [k]
    n_hits: np.ndarray        # [n] int32: rays on the board per candidate (-1: non-finite; 0 for a candidate outside the image)
    in_image: np.ndarray      # [n] bool: every corner of the board rectangle projects inside the image (all True without a camera)
    H0: np.ndarray            # [6, 6] the information of the recording at Tcl
    sv0: np.ndarray           # [6] its eigenvalues, as the analysis pass prints them
    H_after: np.ndarray       # [6, 6] H0 plus the chosen poses' predicted information


def SuggestBoardPoses(obs: ObsLike, Tcl: np.ndarray, cand_q: np.ndarray, cand_t: np.ndarray, k: int = 5,
                      options: Optional[_capi.GuidanceOptions] = None, camera=None, use_linefitting_data: bool = False,
                      solver: Optional[Solver] = None) -> GuidanceReport:
    """Pose guidance (K20): where to hold the board next.  Uploads the recording `obs`, takes H0 from the analysis pass at Tcl (4x4,
    laser -> camera) and picks greedily k of the candidate board poses (cand_q [n, 4] w x y z, cand_t [n, 3], board in the camera
    frame) by the predicted information of clc_select_board_poses.  camera (with a width and a height): candidates whose four
    board-rectangle corners do not all project inside the image with P_z > 0 are dropped first.  H mixes metres and radians, and the
    prediction is taken at Tcl, which a degenerate recording leaves loose along its null directions."""
    sv = solver or _shared_solver()
    ses = Session(obs, sv)
    ses._ensure_stored()
    sv.select_observations(use_linefitting_data, False)
    pose = simdata.pose7_from_T(np.asarray(Tcl, dtype=np.float64))
    H0, _, _, sv0, _, _ = sv.information(pose)
    q = np.ascontiguousarray(cand_q, dtype=np.float64).reshape(-1, 4)
    t = np.ascontiguousarray(cand_t, dtype=np.float64).reshape(-1, 3)
    n = q.shape[0]
    o = options or _capi.default_guidance_options()
    in_image = np.ones(n, dtype=bool)
    if camera is not None and camera.width > 0 and camera.height > 0 and n > 0:
        R = simdata.quat_wxyz_to_rot(q).reshape(n, 3, 3)
        X = np.array([[o.board_min[0], o.board_min[1]], [o.board_max[0], o.board_min[1]], [o.board_max[0], o.board_max[1]],
                      [o.board_min[0], o.board_max[1]]])
        P = R[:, None, :, 0] * X[None, :, 0, None] + R[:, None, :, 1] * X[None, :, 1, None] + t[:, None, :]  # [n, 4, 3]
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(P).all(axis=(1, 2))
            px = sv.camera_project(camera, np.where(fin[:, None, None], P, 1.0).reshape(-1, 3)).reshape(n, 4, 2)
            ok = (P[:, :, 2] > 0) & (px[:, :, 0] >= 0) & (px[:, :, 0] < camera.width) & (px[:, :, 1] >= 0) & (px[:, :, 1] < camera.height)
        in_image = fin & ok.all(axis=1)
    idx = np.flatnonzero(in_image)
    n_hits = np.zeros(n, dtype=np.int32)
    kk = int(k)
    chosen = np.full(kk, -1, dtype=np.int64)
    if idx.size:
        qs, ts = np.ascontiguousarray(q[idx]), np.ascontiguousarray(t[idx])
        n_hits[idx] = sv.score_board_poses(pose, qs, ts, H0, o)["n_hits"]
        r = sv.select_board_poses(pose, qs, ts, kk, H0, o)
        got = r["chosen"] >= 0
        chosen[got] = idx[r["chosen"][got]]
        return GuidanceReport(chosen, r["sv_after"], r["score_after"], n_hits, in_image, H0, sv0, r["H_after"])
    return GuidanceReport(chosen, np.full((kk, 6), np.nan), np.full(kk, np.nan), n_hits, in_image, H0, sv0, H0.copy())


def CalibrateCamera(model: int, width: int, height: int, corners_px: Sequence[np.ndarray], board_xy: Sequence[np.ndarray], hold=None,
                    sigma_px: float = 0.3, camera0=None, solver: Optional[Solver] = None, options: Optional[Options] = None):
    """The camera's intrinsics from images of the board (K19): corners_px[i] [n_i, 2] pixels and board_xy[i] [n_i, 2] board-plane
    points of image i.  The start is `camera0` or the closed-form guess (clc_camera_guess: fx = fy from the images' homographies, the
    principal point at the image centre, zero distortion); the start poses are clc_board_poses' under that camera, images without
    one are dropped; then clc_camera_calibrate over the free intrinsics and every board pose.  hold: the intrinsics to hold — a bit
    mask or a sequence of indices into (proj[0..3], dist[0..3]); None = the model's default (Kannala-Brandt: k4, k5).
    -> (Camera, q_ca [n, 4] (w, x, y, z), t_ca [n, 3], report: summary, termination, cost, rms_px, iterations, H_cam [8, 8], sigma [8]
    (1 sigma of the free intrinsics from inv(H_cam restricted to the free set), NaN for a held one), hold_mask, camera0, status per
    image (CLC_CAMCAL_*), n_used)."""
    from .camera import Camera
    sv = solver or _shared_solver()
    cp = [np.asarray(c, dtype=np.float32).reshape(-1, 2) for c in corners_px]
    bx = [np.asarray(b, dtype=np.float32).reshape(-1, 2) for b in board_xy]
    if len(cp) != len(bx) or any(len(a) != len(b) for a, b in zip(cp, bx)):
        raise ValueError("CalibrateCamera: one board point per corner, image by image")
    off = np.zeros(len(cp) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in cp])
    C_ = np.concatenate(cp) if cp else np.zeros((0, 2), np.float32)
    B_ = np.concatenate(bx) if bx else np.zeros((0, 2), np.float32)
    co = _capi.default_camcal_options(model)
    co.sigma_px = float(sigma_px)
    if hold is not None:
        co.hold_mask = int(hold) if np.isscalar(hold) else int(sum(1 << int(j) for j in set(hold)))
    if camera0 is None:
        camera0, _ = sv.camera_guess(model, width, height, C_, B_, off)
    else:
        camera0 = Camera(camera0.model, tuple(camera0.proj), tuple(camera0.dist), int(width), int(height))
    q0, t0, _, st0, _ = sv.board_poses(camera0, C_, B_, off)
    keep = st0 == _capi.POSE_OK
    res = sv.camera_calibrate(camera0, C_, B_, off, q0, t0, keep=keep, options=options, camcal=co)
    sm = res["summaries"][0]
    H = res["H_cam"][0]
    free = [j for j in range(8) if not (co.hold_mask >> j) & 1]
    sigma = np.full(8, np.nan)
    if free and np.isfinite(H).all():
        try:
            sigma[free] = np.sqrt(np.diag(np.linalg.inv(H[np.ix_(free, free)])))
        except np.linalg.LinAlgError:
            pass
    report = dict(summary=sm, termination=_capi.TERMINATION.get(sm.termination, str(sm.termination)), cost=sm.final_cost,
                  rms_px=float(res["rms_px"][0]), iterations=sm.num_iterations, H_cam=H, sigma=sigma, hold_mask=int(co.hold_mask),
                  camera0=camera0, status=res["status"], n_used=int(np.count_nonzero(res["status"] == _capi.CAMCAL_OK)))
    return res["cameras"][0], res["q"], res["t"], report


FULL_NAMES = ("t_cl_x", "t_cl_y", "t_cl_z", "theta_cl_x", "theta_cl_y", "theta_cl_z", "offset", "scale", "proj0", "proj1", "proj2", "proj3",
              "dist0", "dist1", "dist2", "dist3")  # the order of H_full


def _full_hold(hold, model: int):
    """hold: None (the model's default: Kannala-Brandt's k4, k5), a dict(intrinsics=mask or indices, range=mask or names out of
    ("offset", "scale"), extrinsic=bool, board_poses=bool) or a sequence of names out of FULL_NAMES[6:] -> (intrinsics mask, range
    mask, hold_extrinsic, hold_board_poses)."""
    intr = int(_capi.default_full_options(model).hold_intrinsics_mask)
    if hold is None:
        return intr, 0, 0, 0
    if not isinstance(hold, dict):
        names = set(str(h) for h in hold)
        return (sum(1 << j for j in range(8) if FULL_NAMES[8 + j] in names), _range_hold_mask([h for h in names if h in ("offset", "scale")]),
                0, 0)
    if hold.get("intrinsics") is not None:
        h = hold["intrinsics"]
        intr = int(h) if np.isscalar(h) else int(sum(1 << int(j) for j in set(h)))
    return intr, _range_hold_mask(hold.get("range")), int(bool(hold.get("extrinsic"))), int(bool(hold.get("board_poses")))


def CalibrateFullBatch(problems: Sequence[dict], hold=None, use_linefitting_data: bool = False, sigma_px: float = 0.3,
                       sigma_laser: float = 0.01, loss_px_sigmas: float = 3.0, loss_laser_m: float = 0.05, solver: Optional[Solver] = None,
                       options: Optional[Options] = None):
    """CalibrateFull for a list of problems in one call (one workgroup each): every problem a dict(camera0, corners_px, board_xy — one
    array per image —, obs, Tcl [4, 4], range0 (optional, (offset, scale)), keep (optional)).  The problems share `hold` and the
    options, so their cameras share a model.  -> list of (Camera, Tcl, offset, scale, ObservationSet, report)."""
    sv = solver or _shared_solver()
    sets = [_as_set(p["obs"]) for p in problems]
    cp, bx, co, pts, po, pr, q0, t0 = _joint_arrays([p["corners_px"] for p in problems], [p["board_xy"] for p in problems], sets,
                                                    use_linefitting_data)
    cams0 = [p["camera0"] for p in problems]
    if len(set(c.model for c in cams0)) > 1:
        raise ValueError("CalibrateFullBatch: the problems of one call share a camera model")
    model = cams0[0].model if cams0 else 1
    fo = _capi.default_full_options(model)
    fo.sigma_px, fo.sigma_laser = float(sigma_px), float(sigma_laser)
    fo.loss_corner, fo.loss_laser = float(loss_px_sigmas), float(loss_laser_m) / float(sigma_laser)
    fo.hold_intrinsics_mask, fo.hold_range_mask, fo.hold_extrinsic, fo.hold_board_poses = _full_hold(hold, model)
    keep = None
    if any(p.get("keep") is not None for p in problems):
        keep = np.concatenate([np.ones(s.n_poses, bool) if p.get("keep") is None else np.asarray(p["keep"], bool) for p, s in zip(problems, sets)])
    cl0 = np.stack([simdata.pose7_from_T(np.asarray(p["Tcl"], np.float64)) for p in problems]) if problems else np.zeros((0, 7))
    r0 = np.array([(0.0, 0.0) if p.get("range0") is None else p["range0"] for p in problems], np.float64).reshape(len(problems), 2)
    r = sv.calibrate_full(cams0, cp, bx, co, pts, po, q0, t0, cl0, range0=r0, problem_offsets=pr, keep=keep, options=options, full=fo)
    held = np.array([bool(fo.hold_extrinsic)] * 6 + [bool((fo.hold_range_mask >> j) & 1) for j in range(2)] +
                    [bool((fo.hold_intrinsics_mask >> j) & 1) for j in range(8)])
    out = []
    for k, s in enumerate(sets):
        sl = slice(pr[k], pr[k + 1])
        H = r["H_full"][k]
        free = ~held
        if po[pr[k + 1]] == po[pr[k]]:  # no laser point: the problem holds T_cl, b and kappa by itself
            free[:8] = False
        fi = np.flatnonzero(free)
        sigma = np.full(16, np.nan)
        if np.all(np.isfinite(H)) and len(fi):
            try:
                cov = np.linalg.inv(H[np.ix_(fi, fi)])
                if np.all(np.diag(cov) > 0):
                    sigma[fi] = np.sqrt(np.diag(cov))
            except np.linalg.LinAlgError:
                pass
        w_corner = [r["w_corner"][co[i]:co[i + 1]].copy() for i in range(pr[k], pr[k + 1])]
        w_laser = [r["w_laser"][po[i]:po[i + 1]].copy() for i in range(pr[k], pr[k + 1])]
        sm = r["summaries"][k]
        report = dict(summary=sm, termination=_capi.TERMINATION.get(sm.termination, "?"), cost=sm.final_cost,
                      cost_corner=float(r["cost_parts"][k, 0]), cost_laser=float(r["cost_parts"][k, 1]), rms_px=float(r["rms_px"][k]),
                      iterations=sm.num_iterations, H_full=H, names=FULL_NAMES, sigma=sigma, free=free, status=r["status"][sl].copy(),
                      w_corner=w_corner, w_laser=w_laser, inlier_corner=[w >= 0.5 for w in w_corner],
                      inlier_laser=[w >= 0.5 for w in w_laser], camera0=cams0[k])
        refined = ObservationSet(r["q"][sl].copy(), r["t"][sl].copy(), s.pts_off, s.pts, s.ptl_off, s.ptl)
        out.append((r["cameras"][k], simdata.T_from_pose7(r["poses_cl"][k]), float(r["range"][k, 0]), float(r["range"][k, 1]), refined, report))
    return out


def CalibrateFull(camera0, corners_px: Sequence[np.ndarray], board_xy: Sequence[np.ndarray], obs: ObsLike, Tcl: np.ndarray,
                  range0=(0.0, 0.0), hold=None, use_linefitting_data: bool = False, keep=None, sigma_px: float = 0.3,
                  sigma_laser: float = 0.01, loss_px_sigmas: float = 3.0, loss_laser_m: float = 0.05, model: Optional[int] = None,
                  width: int = 0, height: int = 0, solver: Optional[Solver] = None, options: Optional[Options] = None):
    """The call at the end of the flow (K23): the camera's intrinsics, every board pose, T_cl and the scanner's range offset and scale
    refined under one robust cost — pixel reprojection of the corners (CalibrateCamera's residual), point-to-plane of the laser
    points corrected along their rays (CamLaserCalibrationRange's), a Cauchy loss per corner and per point
    (CamLaserCalibrationJointRobust's).  camera0: the start camera; None: CalibrateCamera's answer on these corners (model, width and
    height are then needed).  The tag poses of `obs` are the start poses.  hold: see _full_hold — None holds only what the model's
    default holds (Kannala-Brandt: k4, k5).
    -> (Camera, Tcl [4, 4], offset, scale, the observation set with the refined tag poses, report: summary, termination, cost,
    cost_corner, cost_laser, rms_px, iterations, H_full [16, 16] — the information on `names` = [T_cl tangent, offset, scale,
    proj[0..3], dist[0..3]] with the board poses marginalised —, sigma (1 sigma of the free shared parameters from the inverse of
    H_full over the free set, NaN for a held one: T_cl's now carries the intrinsics' uncertainty), free, status per image, and per
    image w_corner, w_laser, inlier_corner, inlier_laser (w >= 0.5)).
    Observability: the focal length, the boards' depth, the range scale and t_cl trade against each other along one weakly held
    direction; one-sided laser outliers (objects in front of the board) pull along it through the loss's tail.  Where `sigma` of the
    scale is large or the recording has little spread of ranges, hold "scale" (DESIGN.md K23)."""
    sv = solver or _shared_solver()
    if camera0 is None:
        if model is None:
            raise ValueError("CalibrateFull: camera0 None needs model, width and height for CalibrateCamera")
        camera0 = CalibrateCamera(model, width, height, corners_px, board_xy, sigma_px=sigma_px, solver=sv, options=options)[0]
    return CalibrateFullBatch([dict(camera0=camera0, corners_px=corners_px, board_xy=board_xy, obs=obs, Tcl=Tcl, range0=range0, keep=keep)],
                              hold, use_linefitting_data, sigma_px, sigma_laser, loss_px_sigmas, loss_laser_m, sv, options)[0]


def AutoGetLinePts(points: np.ndarray, debug: bool = True, solver: Optional[Solver] = None) -> np.ndarray:
    """The calibration board's segment in one scan — mirror of AutoGetLinePts(points, debug), src/selectScanPoints.cpp:17-190:
    points [n,3] -> the chosen segment's points [k,3] (empty when there is none).  Raises IndexError where the reference's
    points.at() raises std::out_of_range (an empty scan, or a segment widened past the scan's ends).  `debug` (the
    reference's drawing) is accepted and ignored.  Many scans at once: Solver.board_segments."""
    P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    sv = solver or _shared_solver()
    seg, status = sv.board_segments(P, np.array([0, P.shape[0]], dtype=np.int64))
    if status[0] == -1:
        raise IndexError("AutoGetLinePts: the reference raises std::out_of_range on this scan (selectScanPoints.cpp:47,110,121)")
    if status[0] == 0:
        return np.zeros((0, 3))
    return P[seg[0, 0]:seg[0, 1] + 1].copy()


def points_on_fitted_lines(obs_set: ObservationSet, solver: Optional[Solver] = None,
                           line0=(0.0, 0.0)) -> ObservationSet:
    """The scan front-end step of main/calibr_offline.cpp:121-142 for all scans at once: fit a line
    to every scan's `points` (batched on the GPU) and replace `points_on_line` by the two points of
    the fitted line at the first / last scan point's abscissa (or ordinate for near-vertical lines)."""
    S = obs_set.n_poses
    sv = solver or _shared_solver()
    lines, _ = sv.line_fit_batched(obs_set.pts[:, :2], obs_set.pts_off, np.tile(np.asarray(line0, dtype=np.float64), (S, 1)),
                                   want_summaries=False)

    # the two end points per scan, all scans at once (the per-scan arithmetic of :126-136, element for element)
    lo, hi = obs_set.pts_off[:-1], obs_set.pts_off[1:]
    keep = hi - lo >= 2
    first = np.where(keep, lo, 0)
    last = np.where(keep, hi - 1, 0)
    P = obs_set.pts if obs_set.pts.shape[0] else np.zeros((1, 3))
    xs, ys, xe, ye = P[first, 0].copy(), P[first, 1].copy(), P[last, 0].copy(), P[last, 1].copy()
    m0, m1 = lines[:, 0], lines[:, 1]
    horiz = np.abs(xe - xs) > np.abs(ye - ys)
    with np.errstate(divide="ignore", invalid="ignore"):
        ys = np.where(horiz, -(xs * m0 + 1) / m1, ys)   # :126-131
        ye = np.where(horiz, -(xe * m0 + 1) / m1, ye)
        xs = np.where(horiz, xs, -(ys * m1 + 1) / m0)   # :132-136
        xe = np.where(horiz, xe, -(ye * m1 + 1) / m0)
    ptl = np.zeros((2 * S, 3))
    ptl[0::2, 0], ptl[0::2, 1], ptl[1::2, 0], ptl[1::2, 1] = xs, ys, xe, ye
    ptl_off = np.zeros(S + 1, dtype=np.int64)
    ptl_off[1:] = np.cumsum(np.where(keep, 2, 0))
    ptl = ptl[np.repeat(keep, 2)]
    return ObservationSet(obs_set.tag_q, obs_set.tag_t, obs_set.pts_off, obs_set.pts, ptl_off, np.ascontiguousarray(ptl))
