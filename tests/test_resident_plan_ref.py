"""The restatement of the batched lane planner (tests/resident_plan_ref.py) on hand-computed cases: the points per lane of a
problem, the 256 -> 512 lane fallback, the capacities 42 / 22, flags 4096 / 8192, records with z, empty problems, and the
scan identity — equal consecutive scans merge, a problem start always starts a scan."""
import numpy as np

import resident_plan_ref as R


def _records(scans, z=0.0):
    """scans: list of (plane id, points) -> records [n, 8]; equal plane ids give bitwise equal (n, d, scale)."""
    out = []
    for pid, c in scans:
        r = np.zeros((c, 8))
        r[:, 0:3] = (np.cos(0.1 * pid), np.sin(0.1 * pid), 0.0)
        r[:, 3] = -1.0 - 0.01 * pid
        r[:, 4] = np.arange(c) * 0.01
        r[:, 5] = 1.0
        r[:, 6] = z
        r[:, 7] = 1.0 + pid
        out.append(r)
    return np.concatenate(out) if out else np.zeros((0, 8))


def _batch(problems, z=0.0):
    """problems: lists of (plane id, points) -> (records, offsets)"""
    recs = [_records(p, z) for p in problems]
    off = np.zeros(len(problems) + 1, dtype=np.int64)
    off[1:] = np.cumsum([r.shape[0] for r in recs])
    return np.concatenate(recs) if recs else np.zeros((0, 8)), off


def _singles(first, m):
    return [(first + i, 1) for i in range(m)]


def test_points_per_lane_of_one_problem():
    assert R.problem_ppl([], 256, 42) == 0
    assert R.problem_ppl([1], 256, 42) == 1
    assert R.problem_ppl([1000], 256, 42) == 4            # ceil(1000 / 256) = 4 and 250 lanes
    assert R.problem_ppl([2] * 255 + [3], 256, 42) == 3   # lower bound ceil(513 / 256) = 3
    assert R.problem_ppl([42] + [1] * 255, 256, 42) == 42  # 41: 2 + 255 lanes
    assert R.problem_ppl([43] + [1] * 255, 256, 42) is None
    assert R.problem_ppl([43] + [1] * 255, 512, 22) == 1
    assert R.problem_ppl([1] * 257, 256, 42) is None       # more scans than lanes
    assert R.problem_ppl([22] + [1] * 511, 512, 22) == 22
    assert R.problem_ppl([23] + [1] * 511, 512, 22) is None
    assert R.problem_ppl([10] * 3, 256, 42) == 1


def test_forms_and_capacities():
    rec, off = _batch([[(0, 42)] + _singles(1, 255), [(300, 5)] * 1 + _singles(301, 9)])
    p = R.plan(rec, off)
    assert p.path_info() == (1, 256, 42, 43, 0) and p.ppl == [42, 1] and not p.uniform
    # one problem one point past 42: the whole batch moves to 512 lanes
    rec, off = _batch([[(0, 43)] + _singles(1, 255), [(300, 90)]])
    p = R.plan(rec, off)
    assert p.path_info() == (1, 512, 1, 2, 0) and p.uniform
    # a problem with 512 scans: 512 lanes; one point more than 512 x 22 allows: no lane layout
    rec, off = _batch([[(0, 22)] + _singles(1, 511)])
    assert R.plan(rec, off).path_info() == (1, 512, 22, 22, 0)
    rec, off = _batch([[(0, 23)] + _singles(1, 511)])
    assert R.plan(rec, off).path_info() == (0, 0, 0, 0, 0)
    # flags: 4096 no layout, 8192 straight to 512 lanes
    rec, off = _batch([[(0, 42)] + _singles(1, 255)])
    assert R.plan(rec, off, flags=R.FLAG_NO_RESIDENT).path_info() == (0, 0, 0, 0, 0)
    assert R.plan(rec, off, flags=R.FLAG_RESIDENT_WG512).path_info() == (1, 512, 1, 1, 0)
    # records with z: the 512-lane z form, capacity 22
    rec, off = _batch([[(0, 30)] * 1 + _singles(1, 20), [(50, 3)]], z=0.25)
    assert R.plan(rec, off).path_info() == (1, 512, 1, 2, 1)
    rec, off = _batch([[(0, 21)] + _singles(1, 511)], z=0.25)
    assert R.plan(rec, off).path_info() == (1, 512, 21, 21, 1) and R.plan(rec, off).form == "z"
    rec, off = _batch([[(0, 23)] + _singles(1, 511)], z=0.25)
    assert R.plan(rec, off).path_info() == (0, 0, 0, 0, 0)


def test_empty_problems():
    rec, off = _batch([[], [(0, 7)] * 1, []])
    p = R.plan(rec, off)
    assert p.path_info() == (1, 256, 1, 1, 0) and p.ppl == [0, 1, 0] and not p.uniform
    rec, off = _batch([[], [], []])
    assert rec.shape[0] == 0 and R.plan(rec, off).path_info() == (0, 0, 0, 0, 0)
    rec, off = _batch([[(0, 300)], [(1, 300)]])
    assert R.plan(rec, off).uniform and R.plan(rec, off).ppl == [2, 2]


def test_scan_identity():
    # two consecutive pieces of one board pose (bitwise equal (n, d, scale)) are ONE scan: 21 + 21 -> 42
    rec, off = _batch([[(0, 21), (0, 21)] + _singles(1, 255)])
    lens = R.scan_lengths(rec, off)
    assert len(lens[0]) == 256 and lens[0][0] == 42
    assert R.plan(rec, off).path_info() == (1, 256, 42, 42, 0)
    # ... kept apart (another plane between them) they are 257 scans: more than 256 lanes
    rec, off = _batch([[(0, 21), (1, 1), (0, 21)] + _singles(2, 254)])
    assert len(R.scan_lengths(rec, off)[0]) == 257
    assert R.plan(rec, off).path_info() == (1, 512, 1, 1, 0)
    # a problem start always starts a scan, even where the records on both sides are bitwise equal
    rec, off = _batch([[(5, 3), (0, 40)], [(0, 40), (6, 2)]])
    lens = R.scan_lengths(rec, off)
    assert [list(l) for l in lens] == [[3, 40], [40, 2]]
    # one whole scale differs in the last bit: a new scan
    rec, off = _batch([[(0, 4), (0, 4)]])
    rec[4:, 7] = np.nextafter(rec[4, 7], 2.0)
    assert list(R.scan_lengths(rec, off)[0]) == [4, 4]
    rec[4:, 7] = rec[0, 7]
    rec[4:, 4] += 1.0  # the points differ, the plane does not: one scan
    assert list(R.scan_lengths(rec, off)[0]) == [8]
