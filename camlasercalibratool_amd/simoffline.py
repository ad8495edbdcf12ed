"""A seeded, consistent recording for the offline flow (main/calibr_offline.cpp:51-175): what apriltag_pose.txt and the laser
topic of a bag hold — stamped tag poses T_wc at camera rate and raw 1 081-ray laser scans — for a static camera + laser rig with
the ground truth simdata.GT_RLC / GT_TLC in front of which a finite square board is moved from station to station.

The board stands still at every station (the key-frame filter has poses to drop) and moves in between.  A scan is tied to one
camera frame: it sees the board where that frame saw it, and its stamp lies 1-8 ms from the frame's, so the only key frame that
can be within the 20 ms gate is that frame itself; scans tied to frames the filter drops have no pose, and in some scans the
board is missing.  The rays hit the segment where the board crosses the laser plane (simdata._ray_hits), in front of walls.

Integer decisions must not hinge on the last bit: recording() asserts that every key-frame test is at least 1e-6 from its
threshold, every |dt| at least 1e-6 s from the gate, and the nearest and second-nearest |dt| at least 1e-6 s apart."""
from __future__ import annotations

import numpy as np

from . import simdata as sd

DIST_MIN = 0.20
THETA_MIN = 3.1415926 * 10 / 180.0
MAX_DT = 0.02
MARGIN = 1e-6


def _board_pose(p: np.ndarray):
    """(R_ca, t_ca) of the board from (x, y, z, yaw, pitch, roll): the board's z axis looks back at the camera."""
    flip = np.diag([1.0, -1.0, -1.0])
    return flip @ sd.rot_zyx(p[3], p[4], p[5])[0], p[:3].copy()


def _board_chord(Rca, tca, side, Rlc, tlc):
    """The segment where the board square (|a|, |b| <= side / 2 in its own plane) crosses the laser plane z_l = 0 -> (A, B) in the
    laser frame's (x, y), or None."""
    Rla = Rlc @ Rca
    o = Rlc @ tca + tlc
    u, v = Rla[:, 0], Rla[:, 1]
    hs = side / 2
    # o_z + a u_z + b v_z = 0, clipped to the square: parametrise along the direction (v_z, -u_z)
    d = np.array([v[2], -u[2]])
    nn = u[2] * u[2] + v[2] * v[2]
    if nn < 1e-12:
        return None
    p0 = -o[2] * np.array([u[2], v[2]]) / nn
    lo, hi = -np.inf, np.inf
    for c in range(2):
        if abs(d[c]) < 1e-12:
            if abs(p0[c]) > hs:
                return None
            continue
        s1, s2 = (-hs - p0[c]) / d[c], (hs - p0[c]) / d[c]
        lo, hi = max(lo, min(s1, s2)), min(hi, max(s1, s2))
    if not lo < hi:
        return None
    ab1, ab2 = p0 + lo * d, p0 + hi * d
    A = o + ab1[0] * u + ab1[1] * v
    B = o + ab2[0] * u + ab2[1] * v
    return A[:2], B[:2]


def keyframe_walk(q_wc: np.ndarray, t_wc: np.ndarray, dist_min: float = DIST_MIN, theta_min: float = THETA_MIN):
    """The greedy filter of :62-78 -> (keep [n] bool, smallest distance of a finite dist / theta from its threshold)."""
    n = q_wc.shape[0]
    keep = np.zeros(n, dtype=bool)
    margin = np.inf
    if n == 0:
        return keep, margin
    keep[0] = True
    o = 0
    for j in range(1, n):
        d = t_wc[o] - t_wc[j]
        dist = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        qo, qn = q_wc[o], q_wc[j]
        w = (qo[0] * qn[0] + qo[1] * qn[1] + qo[2] * qn[2] + qo[3] * qn[3]) / (qo[0] * qo[0] + qo[1] * qo[1] + qo[2] * qo[2] + qo[3] * qo[3])
        with np.errstate(invalid="ignore"):
            theta = 2.0 * np.arccos(w)
        if np.isfinite(dist):
            margin = min(margin, abs(dist - dist_min))
        if np.isfinite(theta):
            margin = min(margin, abs(abs(theta) - theta_min))
        if dist > dist_min or abs(theta) > theta_min:
            keep[j] = True
            o = j
    return keep, margin


def recording(seed: int = 1, n_stations: int = 26, move_frames: int = 20, still_frames: int = 8, side: float = 1.2, n_rays: int = 1081,
              fov_deg: float = 270.0, range_sigma: float = 0.001, scan_prob: float = 0.85, board_prob: float = 0.9,
              Rlc: np.ndarray = sd.GT_RLC, tlc: np.ndarray = sd.GT_TLC) -> dict:
    """-> {pose_stamp [n], q_wc [n, 4] (w, x, y, z), t_wc [n, 3], scans (as simdata.sim_laser_scans), scan_stamp [S],
    scan_frame [S] (the camera frame every scan is tied to), has_board [S]}."""
    rng = np.random.default_rng(seed)
    lo = np.array([-0.35, 0.05, 1.0, -0.6, -0.6, -0.6])
    hi = np.array([0.35, 0.55, 1.55, 0.6, 0.6, 0.6])
    stations = rng.uniform(lo, hi, size=(n_stations, 6))
    params = []
    for i in range(n_stations):
        params += [stations[i]] * still_frames
        if i + 1 < n_stations:
            params += [stations[i] + (stations[i + 1] - stations[i]) * (k + 1) / (move_frames + 1) for k in range(move_frames)]
    params = np.array(params)
    n = params.shape[0]
    pose_stamp = 100.0 + np.arange(n) / 30.0
    Rca = np.empty((n, 3, 3)); tca = np.empty((n, 3))
    for j in range(n):
        Rca[j], tca[j] = _board_pose(params[j])
    # apriltag_pose.txt holds T_wc, the camera in the tag's frame: the inverse of T_ca
    Rwc = np.transpose(Rca, (0, 2, 1))
    t_wc = -np.einsum("nij,nj->ni", Rwc, tca)
    q_wc = sd.rot_to_quat_wxyz(Rwc)

    inc = np.deg2rad(fov_deg) / (n_rays - 1)
    a0 = -np.deg2rad(fov_deg) / 2
    th = a0 + np.arange(n_rays) * inc
    frames = np.nonzero(rng.random(n) < scan_prob)[0]
    S = frames.shape[0]
    ranges = np.empty((S, n_rays), dtype=np.float32)
    has_board = rng.random(S) < board_prob
    scan_stamp = pose_stamp[frames] + rng.choice([-1.0, 1.0], S) * rng.uniform(0.001, 0.008, S)
    for k, j in enumerate(frames):
        r = np.full(n_rays, np.inf)
        for _ in range(3):  # walls behind the board
            rho, phi = rng.uniform(3.0, 8.0), rng.uniform(-1.2, 1.2)
            c = np.cos(th - phi)
            r = np.minimum(r, np.where(c > 0.05, rho / np.maximum(c, 0.05), np.inf))
        r = np.minimum(r, 25.0)
        chord = _board_chord(Rca[j], tca[j], side, Rlc, tlc) if has_board[k] else None
        if chord is None:
            has_board[k] = False
        else:
            r = np.minimum(r, sd._ray_hits(th, chord[0], chord[1]))
        ranges[k] = (r + rng.normal(0.0, range_sigma, n_rays)).astype(np.float32)
    scans = {"ranges": ranges.ravel(), "offsets": np.arange(S + 1, dtype=np.int64) * n_rays,
             "angle_min": np.full(S, a0, dtype=np.float32), "angle_increment": np.full(S, inc, dtype=np.float32),
             "range_min": np.full(S, 0.05, dtype=np.float32)}
    rec = {"pose_stamp": pose_stamp, "q_wc": q_wc, "t_wc": t_wc, "scans": scans, "scan_stamp": scan_stamp, "scan_frame": frames,
           "has_board": has_board}
    check_margins(rec)
    return rec


def check_margins(rec: dict) -> dict:
    """Asserts the margin conditions of the module docstring -> {"keyframe": ..., "gate": ..., "tie": ...} (the smallest margins)."""
    keep, m_kf = keyframe_walk(rec["q_wc"], rec["t_wc"])
    assert m_kf >= MARGIN, f"a key-frame test is {m_kf:.3e} from its threshold"
    ks = rec["pose_stamp"][keep]
    dt = np.abs(ks[None, :] - rec["scan_stamp"][:, None])
    m_gate = float(np.abs(dt - MAX_DT).min()) if dt.size else np.inf
    assert m_gate >= MARGIN, f"a |dt| is {m_gate:.3e} s from the gate"
    m_tie = np.inf
    if dt.shape[1] >= 2 and dt.shape[0] > 0:
        two = np.sort(dt, axis=1)[:, :2]
        m_tie = float((two[:, 1] - two[:, 0]).min())
        assert m_tie >= MARGIN, f"nearest and second-nearest |dt| are {m_tie:.3e} s apart"
    return {"keyframe": m_kf, "gate": m_gate, "tie": m_tie}
