"""Plain-numpy restatement of main/calibr_offline.cpp:62-155 for the tests of clc_keyframes / clc_assemble_observations: the
reference's loops, walked sequentially as the reference walks them.  A test helper only — the package has no CPU path.
Uses the other restatements for the steps that have one: oracle.scan_to_points (TranScanToPoints), board_segment_ref
(AutoGetLinePts), oracle.line_fit (LineFittingCeres); the two points on the line are the arithmetic of
calib.points_on_fitted_lines (first and LAST segment point)."""
import math

import numpy as np

import board_segment_ref as BS
from camlasercalibratool_amd.simdata import ObservationSet, quat_wxyz_to_rot

DIST_MIN = 0.20
THETA_MIN = 3.1415926 * 10 / 180.0
MAX_DT = 0.02
NO_SEGMENT, REF_THROWS, NO_POSE = -1, -2, -3


def keyframes(q_wc, t_wc, dist_min=DIST_MIN, theta_min=THETA_MIN, margins=None):
    """:62-78 -> keep [n] bool.  margins (a list, optional) receives |dist - dist_min| and ||theta| - theta_min| of every test."""
    q = np.asarray(q_wc, dtype=np.float64).reshape(-1, 4)
    t = np.asarray(t_wc, dtype=np.float64).reshape(-1, 3)
    n = q.shape[0]
    keep = np.zeros(n, dtype=bool)
    if n == 0:
        return keep
    keep[0] = True
    qo, to = q[0], t[0]
    for j in range(1, n):
        dx, dy, dz = float(to[0] - t[j, 0]), float(to[1] - t[j, 1]), float(to[2] - t[j, 2])
        d2 = dx * dx + dy * dy + dz * dz
        dist = math.sqrt(d2) if d2 >= 0 else math.nan  # (NaN stays NaN)
        a, b = [float(v) for v in qo], [float(v) for v in q[j]]
        dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]
        n2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]
        try:
            w = dot / n2
        except ZeroDivisionError:
            w = math.nan
        theta = 2.0 * math.acos(w) if -1.0 <= w <= 1.0 else math.nan  # std::acos outside [-1, 1]: NaN
        if margins is not None:
            if math.isfinite(dist):
                margins.append(abs(dist - dist_min))
            if math.isfinite(theta):
                margins.append(abs(abs(theta) - theta_min))
        if (dist > dist_min) or (abs(theta) > theta_min):
            keep[j] = True
            qo, to = q[j], t[j]
    return keep


def closest_pose(kf_stamp, scan_stamp, max_dt=MAX_DT):
    """:102-116 for one scan -> position in the key-frame list, or -1.  Strict <, from 10000: the first of equal minima wins and
    a NaN never does."""
    min_dt, best = 10000.0, -1
    for i in range(len(kf_stamp)):
        t = abs(float(kf_stamp[i]) - float(scan_stamp))
        if t < min_dt:
            min_dt, best = t, i
    return best if (best >= 0 and min_dt < max_dt) else -1


def associate(pose_stamp, keep, status, scan_stamp, max_dt=MAX_DT):
    """-> scan_pose [S] int32: the original pose index of every scan with a segment and a pose, or the reason code."""
    kf = np.nonzero(keep)[0]
    ks = np.asarray(pose_stamp, dtype=np.float64)[kf]
    out = np.empty(len(status), dtype=np.int32)
    for s in range(len(status)):
        if status[s] != BS.FOUND:
            out[s] = REF_THROWS if status[s] == BS.THROWS else NO_SEGMENT
            continue
        b = closest_pose(ks, scan_stamp[s], max_dt)
        out[s] = kf[b] if b >= 0 else NO_POSE
    return out


def tag_pose(q_wc, t_wc):
    """:145-146: Qca = qwc.inverse() (conjugate / squared norm), tca = -R(Qca) twc."""
    q = np.asarray(q_wc, dtype=np.float64)
    qi = np.array([q[0], -q[1], -q[2], -q[3]]) / (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return qi, -(quat_wxyz_to_rot(qi) @ np.asarray(t_wc, dtype=np.float64))


def end_points(P, line):
    """:126-142 with the LAST point for points.end() -> [2, 3], or [0, 3] for fewer than 2 points."""
    if P.shape[0] < 2:
        return np.zeros((0, 3))
    xs, ys, xe, ye = P[0, 0], P[0, 1], P[-1, 0], P[-1, 1]
    m0, m1 = line
    with np.errstate(divide="ignore", invalid="ignore"):
        if abs(xe - xs) > abs(ye - ys):
            ys = -(xs * m0 + 1) / m1
            ye = -(xe * m0 + 1) / m1
        else:
            xs = -(ys * m1 + 1) / m0
            xe = -(ye * m1 + 1) / m0
    return np.array([[xs, ys, 0.0], [xe, ye, 0.0]])


def scan_points(scans, oracle):
    off = scans["offsets"]
    S = len(off) - 1
    parts = [oracle.scan_to_points(scans["ranges"][off[k]:off[k + 1]], float(scans["angle_min"][k]), float(scans["angle_increment"][k]),
                                   float(scans["range_min"][k])) for k in range(S)]
    return np.concatenate(parts) if parts else np.zeros((0, 3))


def assemble(pose_stamp, q_wc, t_wc, scans, scan_stamp, oracle=None, points=None, line_fit=True, dist_min=DIST_MIN, theta_min=THETA_MIN,
             max_dt=MAX_DT, line0=(0.0, 0.0)):
    """:62-155 -> (keep [n], scan_pose [S], ObservationSet, info dict).  points: the scans' points when the caller has them (the
    GPU's own TranScanToPoints output); line_fit False: points_on_line left empty (for tests that look at the rest only)."""
    keep = keyframes(q_wc, t_wc, dist_min, theta_min)
    off = np.asarray(scans["offsets"], dtype=np.int64)
    off = off - off[0]
    S = len(off) - 1
    P = scan_points(scans, oracle) if points is None else np.asarray(points, dtype=np.float64).reshape(-1, 3)
    seg, status = BS.board_segments(P, off)
    scan_pose = associate(pose_stamp, keep, status, scan_stamp, max_dt)
    tq, tt, pts, ptl = [], [], [], []
    for s in range(S):
        if scan_pose[s] < 0:
            continue
        pp = P[off[s] + seg[s, 0]: off[s] + seg[s, 1] + 1]
        qi, ti = tag_pose(q_wc[scan_pose[s]], t_wc[scan_pose[s]])
        tq.append(qi); tt.append(ti); pts.append(pp)
        if line_fit:
            ptl.append(end_points(pp, oracle.line_fit(pp[:, :2], line0).pose))
        else:
            ptl.append(np.zeros((0, 3)))
    n = len(pts)
    pts_off = np.zeros(n + 1, dtype=np.int64); ptl_off = np.zeros(n + 1, dtype=np.int64)
    if n:
        pts_off[1:] = np.cumsum([len(p) for p in pts]); ptl_off[1:] = np.cumsum([len(p) for p in ptl])
    obs = ObservationSet(np.array(tq).reshape(n, 4), np.array(tt).reshape(n, 3), pts_off,
                         np.ascontiguousarray(np.concatenate(pts)) if n else np.zeros((0, 3)), ptl_off,
                         np.ascontiguousarray(np.concatenate(ptl)) if n else np.zeros((0, 3)))
    info = {"n_keyframes": int(keep.sum()), "n_segments": int((status == BS.FOUND).sum()), "n_ref_throws": int((status == BS.THROWS).sum()),
            "n_unmatched": int((scan_pose == NO_POSE).sum()), "n_observations": n, "n_points": int(pts_off[n]), "n_line_points": int(ptl_off[n])}
    return keep, scan_pose, obs, info
