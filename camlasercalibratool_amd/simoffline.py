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
    rec = _record(seed, n_stations, move_frames, still_frames, side, n_rays, fov_deg, range_sigma, scan_prob, board_prob, Rlc, tlc)
    check_margins(rec)
    return rec


def _record(seed, n_stations, move_frames, still_frames, side, n_rays, fov_deg, range_sigma, scan_prob, board_prob, Rlc, tlc) -> dict:
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
    return {"pose_stamp": pose_stamp, "q_wc": q_wc, "t_wc": t_wc, "scans": scans, "scan_stamp": scan_stamp, "scan_frame": frames,
            "has_board": has_board}


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


# ---- static stations (GetStaticPose, src/utilities.cpp:86-155) --------------------------------------------------------------------
CENTER_DIST_MAX = 0.002
MIN_MEMBERS = 30


def station_walk(t_wc: np.ndarray, dist_max: float = CENTER_DIST_MAX, min_members: int = MIN_MEMBERS):
    """The walk of :96-124 -> (first [k], last [k], members [k], smallest distance of a finite membership distance from dist_max).
    A run starts at pose a (xy_sum = t_a, size = 1); candidate j = a, a + 1, ... is a member iff |t_j - xy_sum / size| < dist_max
    and then is added; the first non-member closes the run and is discarded; the run open at the end is dropped."""
    t = np.asarray(t_wc, dtype=np.float64).reshape(-1, 3)
    n = t.shape[0]
    first, last, members, margin = [], [], [], np.inf
    a = 0
    while a < n:
        xs, size, j = [float(v) for v in t[a]], 1, a
        while j < n:
            dx, dy, dz = float(t[j, 0]) - xs[0] / size, float(t[j, 1]) - xs[1] / size, float(t[j, 2]) - xs[2] / size
            d = np.sqrt(dx * dx + dy * dy + dz * dz)
            if np.isfinite(d):
                margin = min(margin, abs(d - dist_max))
            if not d < dist_max:
                break
            xs = [xs[c] + float(t[j, c]) for c in range(3)]
            size += 1
            j += 1
        if j >= n:
            break
        if size > min_members:
            first.append(a); last.append(max(j - 1, a)); members.append(size)
        a = j + 1
    return np.array(first, dtype=np.int64), np.array(last, dtype=np.int64), np.array(members, dtype=np.int64), float(margin)


def station_recording(seed: int = 1, n_stations: int = 12, move_frames: int = 20, still_frames: int = 40, pose_sigma_t: float = 2e-4,
                      pose_sigma_r: float = 1e-3, side: float = 1.2, n_rays: int = 1081, fov_deg: float = 270.0, range_sigma: float = 0.001,
                      scan_prob: float = 0.85, board_prob: float = 0.9, Rlc: np.ndarray = sd.GT_RLC, tlc: np.ndarray = sd.GT_TLC) -> dict:
    """recording() with stations long enough for GetStaticPose (more than 30 members) and seeded Gaussian jitter on the STAMPED tag
    poses: pose_sigma_t metres on t_wc, pose_sigma_r radians (a small rotation about a random axis) on q_wc.  The scans still see the
    board where it truly stood.  -> recording()'s dict, q_wc / t_wc the jittered poses, plus q_wc_true / t_wc_true and
    station_first / station_last / station_members (the CPU walk on the jittered translations).  Asserts that every finite
    membership distance is at least MARGIN from CENTER_DIST_MAX and every scan stamp at least MARGIN seconds from a station's ends."""
    rec = _record(seed, n_stations, move_frames, still_frames, side, n_rays, fov_deg, range_sigma, scan_prob, board_prob, Rlc, tlc)
    rng = np.random.default_rng([seed, 0x57A7])  # a stream of its own: the recording itself is recording()'s
    n = rec["pose_stamp"].shape[0]
    rec["q_wc_true"], rec["t_wc_true"] = rec["q_wc"], rec["t_wc"]
    rec["t_wc"] = rec["t_wc_true"] + rng.normal(0.0, pose_sigma_t, (n, 3))
    rv = rng.normal(0.0, pose_sigma_r, (n, 3))
    ang = np.linalg.norm(rv, axis=1)
    axis = rv / np.maximum(ang, 1e-300)[:, None]
    dq = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * axis], axis=1)
    w0, x0, y0, z0 = rec["q_wc_true"].T
    w1, x1, y1, z1 = dq.T
    q = np.stack([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1, w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1,
                  w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1], axis=1)
    rec["q_wc"] = q / np.linalg.norm(q, axis=1)[:, None]
    rec.update(check_station_margins(rec))
    return rec


def check_station_margins(rec: dict) -> dict:
    """Asserts the margin conditions of station_recording -> {"station_first", "station_last", "station_members", "station_margin",
    "stamp_margin"}."""
    first, last, members, m_walk = station_walk(rec["t_wc"])
    assert m_walk >= MARGIN, f"a membership distance is {m_walk:.3e} from its threshold"
    ends = np.concatenate([rec["pose_stamp"][first], rec["pose_stamp"][last]])
    m_stamp = float(np.abs(ends[None, :] - rec["scan_stamp"][:, None]).min()) if ends.size and rec["scan_stamp"].size else np.inf
    assert m_stamp >= MARGIN, f"a scan stamp is {m_stamp:.3e} s from a station's end"
    return {"station_first": first, "station_last": last, "station_members": members, "station_margin": m_walk, "stamp_margin": m_stamp}


# ---- a board that keeps moving: tag poses interpolated at the scans' stamps --------------------------------------------------------
MAX_GAP = 0.1


def moving_recording(seed: int = 1, n_stations: int = 26, move_frames: int = 20, still_frames: int = 8, clock_offset: float = 0.0,
                     side: float = 1.2, n_rays: int = 1081, fov_deg: float = 270.0, range_sigma: float = 0.001, board_prob: float = 0.9,
                     scan_rate: float = 40.0, offsets=(0.0,), Rlc: np.ndarray = sd.GT_RLC, tlc: np.ndarray = sd.GT_TLC) -> dict:
    """A continuous board path: piecewise linear in the six station parameters of recording(), still for still_frames camera periods
    at every station and moving for move_frames + 1 periods in between.  The camera samples the path at 30 Hz (stamps 100 + j / 30);
    the laser runs on a clock of its own, scan_rate Hz from a seeded phase, and a scan stamped tau sees the board where it is at
    path(tau + clock_offset) — clock_offset is what has to be ADDED to a scan's stamp to get camera time.  The scans cover the span in
    which tau + clock_offset +- 50 ms stays inside the camera's stamps.
    -> recording()'s dict without scan_frame, plus clock_offset and the margins of check_motion_margins(rec, offsets)."""
    rng = np.random.default_rng([seed, 0x1D7E])
    lo = np.array([-0.35, 0.05, 1.0, -0.6, -0.6, -0.6])
    hi = np.array([0.35, 0.55, 1.55, 0.6, 0.6, 0.6])
    stations = rng.uniform(lo, hi, size=(n_stations, 6))
    knots_t, knots_p, tk = [], [], 100.0
    for i in range(n_stations):
        knots_t += [tk, tk + (still_frames - 1) / 30.0]
        knots_p += [stations[i], stations[i]]
        tk += (still_frames - 1) / 30.0 + (move_frames + 1) / 30.0
    knots_t, knots_p = np.array(knots_t), np.array(knots_p)
    path = lambda tau: np.stack([np.interp(tau, knots_t, knots_p[:, c]) for c in range(6)], axis=-1)
    n = n_stations * still_frames + (n_stations - 1) * move_frames
    pose_stamp = 100.0 + np.arange(n) / 30.0
    params = path(pose_stamp)
    Rca = np.empty((n, 3, 3)); tca = np.empty((n, 3))
    for j in range(n):
        Rca[j], tca[j] = _board_pose(params[j])
    Rwc = np.transpose(Rca, (0, 2, 1))
    t_wc = -np.einsum("nij,nj->ni", Rwc, tca)
    q_wc = sd.rot_to_quat_wxyz(Rwc)

    inc = np.deg2rad(fov_deg) / (n_rays - 1)
    a0 = -np.deg2rad(fov_deg) / 2
    th = a0 + np.arange(n_rays) * inc
    first = pose_stamp[0] + 0.05 - min(clock_offset, 0.0) + rng.uniform(0.0, 1.0 / scan_rate)
    last = pose_stamp[-1] - 0.05 - max(clock_offset, 0.0)
    S = max(int(np.floor((last - first) * scan_rate)) + 1, 0)
    scan_stamp = first + np.arange(S) / scan_rate
    has_board = rng.random(S) < board_prob
    ranges = np.empty((S, n_rays), dtype=np.float32)
    seen = path(scan_stamp + clock_offset)
    for k in range(S):
        r = np.full(n_rays, np.inf)
        for _ in range(3):  # walls behind the board
            rho, phi = rng.uniform(3.0, 8.0), rng.uniform(-1.2, 1.2)
            c = np.cos(th - phi)
            r = np.minimum(r, np.where(c > 0.05, rho / np.maximum(c, 0.05), np.inf))
        r = np.minimum(r, 25.0)
        chord = _board_chord(*_board_pose(seen[k]), side, Rlc, tlc) if has_board[k] else None
        if chord is None:
            has_board[k] = False
        else:
            r = np.minimum(r, sd._ray_hits(th, chord[0], chord[1]))
        ranges[k] = (r + rng.normal(0.0, range_sigma, n_rays)).astype(np.float32)
    scans = {"ranges": ranges.ravel(), "offsets": np.arange(S + 1, dtype=np.int64) * n_rays,
             "angle_min": np.full(S, a0, dtype=np.float32), "angle_increment": np.full(S, inc, dtype=np.float32),
             "range_min": np.full(S, 0.05, dtype=np.float32)}
    rec = {"pose_stamp": pose_stamp, "q_wc": q_wc, "t_wc": t_wc, "scans": scans, "scan_stamp": scan_stamp, "has_board": has_board,
           "clock_offset": float(clock_offset)}
    rec.update(check_motion_margins(rec, offsets))
    return rec


def check_motion_margins(rec: dict, offsets=(0.0,), max_gap: float = MAX_GAP) -> dict:
    """Asserts that no bracket decision of the interpolated flow hinges on a last bit: every scan stamp + offset, for every offset the
    caller is going to use, is at least MARGIN seconds from every pose stamp, and every interval between consecutive pose stamps at
    least MARGIN seconds from max_gap -> {"stamp_margin", "gap_margin"} (the smallest margins)."""
    ps, ss = rec["pose_stamp"], rec["scan_stamp"]
    m_stamp = np.inf
    for d in offsets:
        if ps.size and ss.size:
            x = ss + d
            i = np.clip(np.searchsorted(ps, x), 1, len(ps) - 1)
            m_stamp = min(m_stamp, float(np.minimum(np.abs(x - ps[i - 1]), np.abs(x - ps[i])).min()))
    assert m_stamp >= MARGIN, f"a scan stamp + offset is {m_stamp:.3e} s from a pose stamp"
    m_gap = float(np.abs(np.diff(ps) - max_gap).min()) if ps.size >= 2 else np.inf
    assert m_gap >= MARGIN, f"an interval between pose stamps is {m_gap:.3e} s from max_gap"
    return {"stamp_margin": m_stamp, "gap_margin": m_gap}
