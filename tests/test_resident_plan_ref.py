"""The restatement of the batched lane planner (tests/resident_plan_ref.py) on hand-computed cases: the points per lane of a
problem, the 256 -> 512 lane fallback, the capacities 42 / 22, flags 4096 / 8192, records with z, empty problems, and the
scan identity — equal consecutive scans merge, a problem start always starts a scan; and the lane deal (lane_cuts)."""
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


def test_lane_cuts_by_hand():
    # 7 records at 3 per lane: 3 lanes of 3, 2, 2; then a scan of 3 in one lane, a scan of 1
    scan, first, cnt = R.lane_cuts([7, 3, 1], 8, 3)
    assert scan.tolist() == [0, 0, 0, 1, 2, -1, -1, -1]
    assert first.tolist() == [0, 3, 5, 7, 10, 11, 11, 11]
    assert cnt.tolist() == [3, 2, 2, 3, 1, 0, 0, 0]
    # 10 records at 4 per lane: ceil(10 / 4) = 3 lanes of 4, 3, 3 — not 4, 4, 2
    assert R.lane_cuts([10], 4, 4)[2].tolist() == [4, 3, 3, 0]
    assert R.lane_cuts([], 4, 1)[2].tolist() == [0, 0, 0, 0]


def test_lane_cuts_properties_on_seeded_problems():
    """Counts sum to n, every count of a used lane is in [1, ppl], at most nl lanes are used, a lane's first record is the sum of the
    counts before it, a lane holds records of one scan, and a scan's lanes differ by at most one record."""
    rng = np.random.default_rng(11)
    for case in range(300):
        nl = (256, 512)[case % 2]
        cap = R.CAP[nl]
        ns = int(rng.integers(1, nl + 1))
        lens = np.where(rng.random(ns) < 0.5, rng.integers(1, 4, size=ns), rng.integers(1, 3 * cap, size=ns)).astype(np.int64)
        ppl = R.problem_ppl(lens, nl, 10**6)
        scan, first, cnt = R.lane_cuts(lens, nl, ppl)
        n = int(lens.sum())
        used = cnt > 0
        assert scan.shape == first.shape == cnt.shape == (nl,)
        assert int(cnt.sum()) == n
        assert used.sum() <= nl and used.sum() == int((-(-lens // ppl)).sum())
        assert not used[int(used.sum()):].any() and np.all(scan[~used] == -1) and np.all(first[~used] == n)
        assert np.all((cnt[used] >= 1) & (cnt[used] <= ppl))
        assert np.array_equal(first[used], np.concatenate([[0], np.cumsum(cnt[used])[:-1]]))
        starts = np.concatenate([[0], np.cumsum(lens)])
        assert np.all(first[used] >= starts[scan[used]]) and np.all(first[used] + cnt[used] <= starts[scan[used] + 1])
        assert np.array_equal(np.bincount(scan[used], weights=cnt[used], minlength=ns).astype(np.int64), lens)
        for s in np.flatnonzero(lens > ppl)[:8]:
            c = cnt[scan == s]
            assert c.max() - c.min() <= 1 and np.all(np.diff(c) <= 0)
        if ppl > 1:   # one point per lane less would need more lanes than the workgroup has
            assert int((-(-lens // (ppl - 1))).sum()) > nl
