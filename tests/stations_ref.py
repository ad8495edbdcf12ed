"""Plain-numpy restatement of GetStaticPose (src/utilities.cpp:86-155) and getAvergeQwc (:156-166) for the tests of clc_static_poses /
clc_assemble_stations, walked sequentially as the reference walks them, plus this project's interval association of scans with
stations.  A test helper only — the package has no CPU path.  Checked against the reference's own compiled function on the frozen
fixture tests/golden/static_poses_ref.json (tests/test_stations_host.py)."""
import math

import numpy as np

import board_segment_ref as BS

DIST_MAX = 0.002
MIN_MEMBERS = 30
NO_SEGMENT, REF_THROWS, NO_POSE = -1, -2, -3
STATION_OK, STATION_NONFINITE = 1, -1


def _dist(t, xs, size):
    """|t - xs / size|: the centre a per-component division, norm() with every square and sum rounded."""
    dx, dy, dz = float(t[0]) - xs[0] / size, float(t[1]) - xs[1] / size, float(t[2]) - xs[2] / size
    d2 = dx * dx + dy * dy + dz * dz
    return math.sqrt(d2) if d2 >= 0 else math.nan


def walk_literal(t_wc, dist_max=DIST_MAX, min_members=MIN_MEMBERS):
    """The loop of :96-124 as written: new_center_flag, xy_sum, center, staticPose (a list of pose indices).
    -> list of member lists (the reference's staticPoses: the first pose of a run appears twice)."""
    t = np.asarray(t_wc, dtype=np.float64).reshape(-1, 3)
    new_center, xs, center, cur, out = True, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [], []
    for i in range(t.shape[0]):
        T = [float(v) for v in t[i]]
        if new_center:
            new_center = False
            xs = list(T)
            center = list(T)
            cur.append(i)
        if _dist(T, center, 1.0) < dist_max:
            xs = [xs[c] + T[c] for c in range(3)]
            cur.append(i)
            center = [xs[c] / len(cur) for c in range(3)]
        else:
            new_center = True
            xs = [0.0, 0.0, 0.0]
            if len(cur) > min_members:
                out.append(cur)
            cur = []
    return out


def walk(t_wc, dist_max=DIST_MAX, min_members=MIN_MEMBERS, close_last_run=False):
    """The uniform form: a run starts at pose a with xy_sum = t_a, size = 1; candidate j = a, a + 1, ... is a member iff
    |t_j - xy_sum / size| < dist_max and then does xy_sum += t_j, ++size; the first non-member closes the run [a, j - 1], is
    discarded, and the next run starts at j + 1.  -> dict: first, last, members [n_stations] int64 (members: the first pose
    counted twice), n_runs (every closed run), margin (the smallest |dist - dist_max| of a finite membership distance)."""
    t = np.asarray(t_wc, dtype=np.float64).reshape(-1, 3)
    n = t.shape[0]
    first, last, members, n_runs, margin = [], [], [], 0, math.inf

    def close(a, l, m):
        nonlocal n_runs
        n_runs += 1
        if m > min_members:
            first.append(a); last.append(l); members.append(m)

    a = 0
    while a < n:
        xs, size, j, closed = [float(v) for v in t[a]], 1, a, False
        while j < n:
            d = _dist(t[j], xs, size)
            if math.isfinite(d):
                margin = min(margin, abs(d - dist_max))
            if d < dist_max:
                xs = [xs[c] + float(t[j, c]) for c in range(3)]
                size += 1
                j += 1
                continue
            close(a, max(j - 1, a), size)
            a, closed = j + 1, True
            break
        if not closed:
            if close_last_run:
                close(a, n - 1, size)
            break
    return {"first": np.array(first, dtype=np.int64), "last": np.array(last, dtype=np.int64), "members": np.array(members, dtype=np.int64),
            "n_runs": n_runs, "margin": margin}


def member_list(first, members):
    """Pose indices of a station's members: the first pose, then poses first .. first + members - 2."""
    return [int(first)] + list(range(int(first), int(first) + int(members) - 1))


def fix_sign(q):
    q = np.asarray(q, dtype=np.float64)
    nz = np.nonzero(q)[0]
    return -q if len(nz) and q[nz[0]] < 0 else q


def mean_matrix(q_wc, idx):
    """A = sum q q^T / n over the members, q as (w, x, y, z), summed in the reference's order."""
    A = np.zeros((4, 4))
    for p in idx:
        v = np.asarray(q_wc[p], dtype=np.float64)
        A = A + np.outer(v, v)
    return A / len(idx)


def average(pose_stamp, q_wc, t_wc, w):
    """:129-152 for the stations of walk() -> dict: start_time, end_time [k], q [k, 4] (sign fixed: w > 0, or the first non-zero
    component positive), t [k, 3], status [k], gap [k] (largest minus second-largest eigenvalue of A)."""
    q_wc = np.asarray(q_wc, dtype=np.float64).reshape(-1, 4)
    t_wc = np.asarray(t_wc, dtype=np.float64).reshape(-1, 3)
    k = len(w["first"])
    out = {"start_time": np.zeros(k), "end_time": np.zeros(k), "q": np.zeros((k, 4)), "t": np.zeros((k, 3)),
           "status": np.full(k, STATION_OK, dtype=np.int32), "gap": np.full(k, np.nan)}
    for i in range(k):
        idx = member_list(w["first"][i], w["members"][i])
        if pose_stamp is not None:
            out["start_time"][i], out["end_time"][i] = pose_stamp[w["first"][i]], pose_stamp[w["last"][i]]
        ts = np.zeros(3)
        for p in idx:
            ts = ts + t_wc[p]
        tm = ts / len(idx)
        A = mean_matrix(q_wc, idx)
        if not (np.isfinite(A).all() and np.isfinite(tm).all()):
            out["status"][i] = STATION_NONFINITE
            out["q"][i] = [1.0, 0.0, 0.0, 0.0]
            continue
        ev, V = np.linalg.eigh(A)
        out["q"][i] = fix_sign(V[:, 3] / np.linalg.norm(V[:, 3]))
        out["t"][i] = tm
        out["gap"][i] = ev[3] - ev[2]
    return out


def associate(start_time, end_time, st_status, seg_status, scan_stamp):
    """-> scan_station [S] int32: the FIRST station in station order that is finite and has start_time <= stamp <= end_time, or
    the reason code."""
    out = np.empty(len(seg_status), dtype=np.int32)
    for s in range(len(seg_status)):
        if seg_status[s] != BS.FOUND:
            out[s] = REF_THROWS if seg_status[s] == BS.THROWS else NO_SEGMENT
            continue
        out[s] = NO_POSE
        ts = float(scan_stamp[s])
        for i in range(len(start_time)):
            if st_status[i] == STATION_OK and start_time[i] <= ts <= end_time[i]:
                out[s] = i
                break
    return out
