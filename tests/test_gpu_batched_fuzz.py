"""Seeded shape fuzz of clc_solve_batched and clc_solve_multistart against the oracle (DENSE_QR Ceres restatement), with batches
built to sit on the capacity edges of the on-chip resident kernel (csrc/clc_resident.hpp) and of its lane planner:

  form (lanes, PR + PL)        edges
  256 lanes, 23 + 19 = 42      ppl 1..3, 22 / 23 / 24 (last register slot / first LDS slot), 40 / 41 / 42 (groups of 3: every
                               residue), 43: the whole batch moves to 512 lanes
  512 lanes, 4 + 18 = 22       ppl 1, 2, 4 / 5, 21 / 22 (groups of 2); 23: no lane layout, the streaming paths take over
  512 lanes with z, 10 + 12    ppl 1, 10 / 11, 21 / 22; 23: no lane layout

A problem is a list of scan lengths, searched with the planner's restatement (tests/resident_plan_ref.py) so that its points per
lane are exactly the edge wanted: k long scans of q_i t - r_i points (0 <= r_i < q_i: q_i lanes at t points per lane, one more at
t - 1) and enough scans of 1-3 points that t - 1 points per lane would need one lane more than the workgroup has.  Batches:
uniform (row0 = problem x ppl) and mixed (res_row), with empty problems (problem 0 among them), 1-observation problems, two
consecutive pieces of one board pose (one scan), neighbouring problems whose boundary records are bitwise equal (two scans), and
P = 1, 2 CUs +- 1 (256 lanes: two problems per CU) or CUs +- 1 (512 lanes), the CU count read from the device.

Every batch: path_info() equals the restatement's prediction; every problem against the oracle (same termination and iteration
count, T_cl within 1e-6 and final cost within 1e-8 — without T_cl below 7 scans, which do not pin the pose); a second solve
bitwise equal; 16 sampled problems solved again as a batch of one, bitwise equal wherever the restatement gives them the same form
and points per lane.  Past capacity: the same gates on the default fallback and under flags 4096, 2048 and 2048 | 1024.
A difference in iteration count or termination passes only as a near tie of the oracle's own trace (tests/lm_near_tie.py).

Shared with tests/subsets_fuzz_cases.py and tests/test_gpu_subsets_fuzz.py, which import this module: Pool, edge_lens, EDGES, NL, K,
N_SCANS, _with_z, _options, _key and _path.  Change them with those callers in mind."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import camlasercalibratool_amd as clc
import lm_near_tie as NT
import resident_plan_ref as R
from camlasercalibratool_amd import simdata as sd

pytestmark = pytest.mark.gpu

T_TOL = 1e-6
COST_TOL = 1e-8
BASE = 2 | 16 | 32 | 128 | 256 | 512
FALLBACK_FLAGS = (-1, BASE | 4096, BASE | 2048, BASE | 2048 | 1024)
K = 1024          # points per pool scan
N_SCANS = 640     # pool scans
EDGES = {256: (1, 2, 3, 22, 23, 24, 40, 41, 42), 512: (1, 2, 4, 5, 21, 22), "z": (1, 10, 11, 21, 22)}
NL = {256: 256, 512: 512, "z": 512}
STATS = {}


@pytest.fixture(scope="module")
def sv():
    s = clc.Solver(0)
    yield s
    s.set_launch(0, -1)
    s.close()


@pytest.fixture(scope="module")
def pool():
    return Pool(20261015, N_SCANS, K, 0.01)


@pytest.fixture(scope="module")
def cus(sv):
    return sv.device_info()[1]


@pytest.fixture(scope="module")
def workers(oracle_mod):
    with ThreadPoolExecutor(max_workers=min(16, oracle_mod.max_threads())) as ex:
        yield ex


class Pool:
    """N scans of K points each around one ground truth; a problem = windows of some of them."""

    def __init__(self, seed, n_scans, K, noise):
        self.K, self.S = K, n_scans
        self.rec = clc.flatten_observations(sd.sim_fixed_count(seed, n_scans, K, noise_sigma=noise), False).reshape(n_scans, K, 8)
        self.gt = sd.pose7_from_T(sd.tlc_to_tcl(sd.GT_RLC, sd.GT_TLC))

    def pieces(self, lens, rng):
        """(scan, first, count) pieces: one window of a distinct pool scan per length."""
        lens = np.asarray(lens, dtype=np.int64)
        assert len(lens) <= self.S and (len(lens) == 0 or lens.max() <= self.K)
        scans = rng.permutation(self.S)[: len(lens)]
        return [(int(s), int(rng.integers(0, self.K - l + 1)), int(l)) for s, l in zip(scans, lens)]

    def build(self, pieces):
        if not pieces:
            return np.zeros((0, 8))
        return np.ascontiguousarray(np.concatenate([self.rec[s, a:a + l] for s, a, l in pieces]))


def edge_lens(nl, t, rng, style):
    """Scan lengths of a problem whose points per lane at nl lanes are exactly t (t - 1 needs one lane more than nl).
    style 'short': 1-4 scans of t points, the rest 1-3 points; 'split': up to 6 scans over 2-24 lanes each; 'dense': 8-16 long
    scans that fill the workgroup (few short scans: the row layout applies)."""
    if t == 1:
        return np.ones(int(rng.integers(max(7, nl // 4), nl + 1)), dtype=np.int64)
    qmax = max(1, min(K // t, 48))
    for _ in range(100):
        if style == "short":
            q = np.ones(int(rng.integers(1, 5)), dtype=np.int64)
        elif style == "split":
            q = rng.integers(min(2, qmax), min(24, qmax) + 1, size=int(rng.integers(1, 7)))
        else:
            k = int(rng.integers(8, 17))
            q = np.minimum(qmax, np.maximum(1, rng.multinomial(nl - k - int(rng.integers(0, 8)), np.ones(k) / k)))
        k = len(q)
        r = np.array([int(rng.integers(0, qi)) for qi in q], dtype=np.int64)
        long = q * t - r
        m = nl - int(q.sum()) - int(rng.integers(0, k))
        if m < 0:
            continue
        short = rng.integers(1, min(3, t - 1) + 1, size=m)
        lens = np.concatenate([long, short]).astype(np.int64)
        rng.shuffle(lens)
        assert R.problem_ppl(lens, nl, 10**6) == t, (nl, t, style)
        return lens
    raise AssertionError((nl, t, style))


def ragged_lens(rng):
    ns = int(rng.integers(7, 60))
    return np.where(rng.random(ns) < 0.3, rng.integers(1, 4, size=ns), rng.integers(4, 120, size=ns)).astype(np.int64)


class Batch:
    def __init__(self, label):
        self.label, self.pieces, self.kinds = label, [], []

    def add(self, pieces, kind=""):
        self.pieces.append(pieces)
        self.kinds.append(kind)


def _options(use_loss, oracle_mod):
    o, oo = clc.default_options(), oracle_mod.default_options()
    if not use_loss:
        o.use_loss = 0
        oo.use_loss = 0
    return o, oo


def _key(s):
    return (s.termination, s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps, s.num_evaluations, s.initial_cost, s.final_cost)


def _path(sv):
    pi = sv.path_info()
    return (pi.batched_resident, pi.batched_lanes, pi.batched_points_per_lane, pi.batched_lane_rows, pi.batched_points_carry_z)


def _stat(form):
    return STATS.setdefault(str(form), {"batches": 0, "problems": 0, "ppl": set(), "P": set(), "uniform": 0, "mixed": 0,
                                        "fallback": 0, "fallback_problems": 0, "multistart": [], "exempt": 0, "one": 0})


def _oracle_all(workers, oracle_mod, recs, x0, oo):
    def one(k):
        return None if recs[k].shape[0] == 0 else oracle_mod.solve(recs[k], x0[k], oo, linear_solver="qr")
    return list(workers.map(one, range(len(recs))))


def _gate(oracle_mod, rec, x0, oo, s, pose, ref, n_scans, label):
    """-> 1 for a near-tie exemption, 0 otherwise (asserts the gates)."""
    got = (s.termination, s.num_iterations, s.final_cost)
    want = (ref.summary.termination, ref.summary.num_iterations, ref.summary.final_cost)
    if NT.check_flip(oracle_mod, rec, x0, oo, got, want, label):
        return 1
    assert abs(s.final_cost - ref.summary.final_cost) <= COST_TOL, (label, s.final_cost, ref.summary.final_cost)
    if n_scans >= 7:
        dT = np.abs(sd.T_from_pose7(pose) - sd.T_from_pose7(ref.pose)).max()
        assert dT <= T_TOL, (label, dT)
    return 0


def _start_poses(sv, pool, lens_list, rng):
    x = np.empty((len(lens_list), 7))
    for k, lens in enumerate(lens_list):
        x[k] = sv.pose_plus(pool.gt[None, :], rng.normal(size=(1, 6)) * (0.03 if len(lens) > 2 else 0.005))[0]
    return x


def _with_z(recs, rng):
    for r in recs:
        if r.shape[0]:
            idx = np.arange(0, r.shape[0], int(rng.integers(1, 4)))
            r[idx, 6] = rng.normal(size=idx.shape[0]) * 0.02


def run_batch(sv, oracle_mod, workers, pool, batch, rng, form, z=False, fallback=False):
    """Upload, check the plan, solve, compare every problem with the oracle; -> the plan."""
    recs = [pool.build(p) for p in batch.pieces]
    if z:
        _with_z(recs, rng)
    P = len(recs)
    off = np.zeros(P + 1, dtype=np.int64)
    off[1:] = np.cumsum([r.shape[0] for r in recs])
    rec = np.concatenate(recs) if off[-1] else np.zeros((0, 8))
    lens = R.scan_lengths(rec, off)
    plan = R.plan_lens(lens, 0, bool(np.any(rec[:, 6] != 0.0)))
    label = f"{batch.label} P={P}"
    if fallback:
        assert not plan.resident or plan.form != form, (label, plan.path_info())
    else:
        assert plan.form == form, (label, plan.path_info())
    use_loss = bool(rng.random() < 0.8)
    o, oo = _options(use_loss, oracle_mod)
    x0 = _start_poses(sv, pool, lens, rng)
    sv.set_launch(0, -1)
    sv.upload_batched(rec, off)
    assert _path(sv) == plan.path_info(), (label, _path(sv), plan.path_info())
    refs = _oracle_all(workers, oracle_mod, recs, x0, oo)
    st = _stat(form)
    st["batches"] += 1
    st["problems"] += P
    st["P"].add(P)
    if plan.resident and plan.form == form:
        st["ppl"].update(c for c in plan.ppl if c > 0)
        st["uniform" if plan.uniform else "mixed"] += 1
    exempt = 0
    flag_sets = FALLBACK_FLAGS if not plan.resident or plan.form != form else (-1,)
    if len(flag_sets) > 1:
        st["fallback"] += 1
        st["fallback_problems"] += P
    first = None
    for flags in flag_sets:
        sv.set_launch(0, flags)
        pr, sr = sv.solve_batched(x0, o)
        for k in range(P):
            if recs[k].shape[0]:
                exempt += _gate(oracle_mod, recs[k], x0[k], oo, sr[k], pr[k], refs[k], len(lens[k]),
                                f"{label} flags={flags} problem {k} ({batch.kinds[k]}, ppl {plan.ppl[k] if plan.resident else '-'})")
        if first is None:
            first = (pr, [_key(s) for s in sr])
    sv.set_launch(0, -1)
    pr2, sr2 = sv.solve_batched(x0, o)  # bitwise repeatable
    assert np.array_equal(pr2, first[0], equal_nan=True) and [_key(s) for s in sr2] == first[1], label
    assert exempt <= max(1, P // 1000), (label, exempt)
    st["exempt"] += exempt
    if plan.resident:  # a problem alone, in the same form at the same points per lane: bitwise the same answer
        nonempty = [k for k in range(P) if recs[k].shape[0]]
        for k in rng.choice(nonempty, size=min(16, len(nonempty)), replace=False):
            flags = BASE | R.FLAG_RESIDENT_WG512 if plan.form == 512 else -1
            p1 = R.plan_lens([lens[k]], flags if flags > 0 else 0, bool(np.any(recs[k][:, 6] != 0.0)))
            if p1.form != plan.form or p1.ppl[0] != plan.ppl[k]:
                continue
            sv.set_launch(0, flags)
            sv.upload_batched(recs[k], np.array([0, recs[k].shape[0]]))
            assert _path(sv) == p1.path_info(), (label, k)
            p, s = sv.solve_batched(x0[k:k + 1], o)
            assert np.array_equal(p[0], first[0][k]) and _key(s[0]) == first[1][k], (label, "alone", k)
            st["one"] += 1
        sv.set_launch(0, -1)
    return plan


def _edge_problem(pool, form, t, rng, style):
    """Pieces of a problem at t points per lane in `form`; a 512-lane problem does not fit 256 lanes itself (it moves its batch)."""
    for i in range(50):
        lens = edge_lens(NL[form], t, rng, style if i < 25 else "short")
        if form != 512 or R.problem_ppl(lens, 256, R.CAP[256]) is None:
            return pool.pieces(lens, rng)
    raise AssertionError((form, t, style))


def _past_capacity_problem(pool, form, rng):
    """Pieces of a problem that needs 23 points per lane of 512 lanes (and does not fit 256 lanes either): no lane layout."""
    for _ in range(50):
        lens = edge_lens(512, 23, rng, "dense")
        if not R.plan_lens([lens], 0, form == "z").resident:
            return pool.pieces(lens, rng)
    raise AssertionError(form)


def _scan_identity_problems(pool, form, rng):
    """(pieces, kind): two consecutive pieces of one board pose, one scan of the form's capacity once merged, + nl - 1 scans of one
    point (unmerged: one scan more than the workgroup has lanes); and two neighbours whose boundary records are bitwise equal."""
    nl, t = NL[form], R.CAP[form]
    order = rng.permutation(pool.S)
    s, others = int(order[0]), order[1:nl]
    a = int(rng.integers(0, pool.K - t + 1))
    merged = [(s, a, t // 2), (s, a + t // 2, t - t // 2)] + [(int(c), int(rng.integers(0, pool.K)), 1) for c in others]
    s2 = int(order[nl])
    left = [p for p in pool.pieces(ragged_lens(rng), rng) if p[0] != s2] + [(s2, 0, 30)]
    right = [(s2, 30, 12)] + [p for p in pool.pieces(ragged_lens(rng), rng) if p[0] != s2]
    return [(merged, "merged scan"), (left, "boundary left"), (right, "boundary right")]


def _mixed_batch(pool, form, P, rng, label):
    b = Batch(label)
    edges = EDGES[form]
    ident = _scan_identity_problems(pool, form, rng)
    for k in range(P):
        u = rng.random()
        if P <= 2:
            t = R.CAP[form] if k == P - 1 else int(rng.choice(edges))
            b.add(_edge_problem(pool, form, t, rng, "short"), f"edge {t}")
        elif k == 0:
            b.add([], "empty")
        elif k in (1, 2, 3) and P > 8:
            b.add(*ident[k - 1])
        elif u < 0.05:
            b.add([], "empty")
        elif u < 0.12:
            b.add(pool.pieces([1], rng), "one observation")
        elif u < 0.2:
            b.add(pool.pieces(ragged_lens(rng), rng), "ragged")
        else:
            t = int(rng.choice(edges))
            b.add(_edge_problem(pool, form, t, rng, "short" if rng.random() < 0.85 else "split"), f"edge {t}")
    return b


def _summary(form):
    st = _stat(form)
    cap = R.GRP[form]
    print(f"batched fuzz [{form}]: {st['batches']} batches, {st['problems']} problems ({st['uniform']} uniform, {st['mixed']} mixed), "
          f"ppl hit {sorted(st['ppl'])} (residues mod {cap}: {sorted({c % cap for c in st['ppl']})}), P {sorted(st['P'])}, "
          f"{st['fallback']} fallback batches ({st['fallback_problems']} problems x {len(FALLBACK_FLAGS)} flag sets), multistart S "
          f"{st['multistart']}, {st['one']} problems alone bitwise, {st['exempt']} near-tie exemptions")


def _fuzz_form(sv, oracle_mod, workers, pool, cus, form, seed):
    rng = np.random.default_rng(seed)
    t0 = time.perf_counter()
    z = form == "z"
    styles = ("short", "split", "dense")
    # uniform batches: every edge, every problem at the same points per lane
    for i, t in enumerate(EDGES[form]):
        b = Batch(f"{form} uniform ppl={t}")
        for j in range(int(rng.integers(3, 7))):
            b.add(_edge_problem(pool, form, t, rng, styles[(i + j) % 3] if t > 1 else "short"), f"edge {t}")
        plan = run_batch(sv, oracle_mod, workers, pool, b, rng, form, z=z)
        assert plan.uniform and plan.max_ppl == t, (b.label, plan.ppl)
    # mixed batches at the problem counts where a second round of workgroups starts
    per_cu = 2 if form == 256 else 1
    for P in (1, per_cu * cus - 1, per_cu * cus, per_cu * cus + 1):
        run_batch(sv, oracle_mod, workers, pool, _mixed_batch(pool, form, P, rng, f"{form} mixed"), rng, form, z=z)
    st = _stat(form)
    assert set(EDGES[form]) <= st["ppl"], (form, sorted(st["ppl"]))
    assert {1, per_cu * cus - 1, per_cu * cus, per_cu * cus + 1} <= st["P"]
    return time.perf_counter() - t0


def test_batched_fuzz_256_lanes(sv, oracle_mod, workers, pool, cus):
    dt = _fuzz_form(sv, oracle_mod, workers, pool, cus, 256, 1)
    _summary(256)
    print(f"  {dt:.1f} s")


def test_batched_fuzz_512_lanes(sv, oracle_mod, workers, pool, cus):
    dt = _fuzz_form(sv, oracle_mod, workers, pool, cus, 512, 2)
    _summary(512)
    print(f"  {dt:.1f} s")


def test_batched_fuzz_512_lanes_with_z(sv, oracle_mod, workers, pool, cus):
    dt = _fuzz_form(sv, oracle_mod, workers, pool, cus, "z", 3)
    _summary("z")
    print(f"  {dt:.1f} s")


def test_batched_fuzz_one_past_capacity(sv, oracle_mod, workers, pool):
    """43 points per lane at 256 lanes: the whole batch on 512 lanes; 23 at 512 lanes (with and without z): no lane layout, and
    every problem meets the oracle gates on the default fallback and under flags 4096, 2048 and 2048 | 1024."""
    rng = np.random.default_rng(4)
    b = Batch("256 past capacity")
    for j in range(4):
        b.add(_edge_problem(pool, 256, 43, rng, ("short", "split")[j % 2]), "edge 43")
    b.add(_edge_problem(pool, 256, 42, rng, "short"), "edge 42")
    plan = run_batch(sv, oracle_mod, workers, pool, b, rng, 256, fallback=True)
    assert plan.form == 512, plan.path_info()
    for form in (512, "z"):
        b = Batch(f"{form} past capacity")
        b.add(_past_capacity_problem(pool, form, rng), "edge 23")
        for j in range(5):
            b.add(pool.pieces(ragged_lens(rng), rng) if j % 2 else _edge_problem(pool, form, 22, rng, "dense"), "fill")
        b.add(pool.pieces([1], rng), "one observation")
        plan = run_batch(sv, oracle_mod, workers, pool, b, rng, form, z=form == "z", fallback=True)
        assert not plan.resident
    print(f"batched fuzz past capacity: {[(f, _stat(f)['fallback'], _stat(f)['fallback_problems']) for f in (256, 512, 'z')]}")


def test_multistart_fuzz_at_the_edges(sv, oracle_mod, workers, pool, cus):
    """clc_solve_multistart on one problem at each form's largest points per lane: S = 1, a full round of workgroups, one more.
    Every start against the oracle; S = 1 bitwise equal to clc_solve_batched of the same problem."""
    rng = np.random.default_rng(5)
    for form in (256, 512, "z"):
        t = R.CAP[form]
        rec = pool.build(_edge_problem(pool, form, t, rng, "short"))
        if form == "z":
            _with_z([rec], rng)
        off = np.array([0, rec.shape[0]])
        lens = R.scan_lengths(rec, off)
        plan = R.plan_lens(lens, 0, form == "z")
        assert plan.form == form and plan.ppl == [t]
        use_loss = bool(rng.random() < 0.8)
        o, oo = _options(use_loss, oracle_mod)
        sv.set_launch(0, -1)
        sv.upload_batched(rec, off)
        assert _path(sv) == plan.path_info()
        per_cu = 2 if form == 256 else 1
        for S in (1, per_cu * cus, per_cu * cus + 1):
            x0 = _start_poses(sv, pool, lens * S, rng)
            pm, sm = sv.solve_multistart(x0, o)
            refs = _oracle_all(workers, oracle_mod, [rec] * S, x0, oo)
            exempt = sum(_gate(oracle_mod, rec, x0[k], oo, sm[k], pm[k], refs[k], len(lens[0]), f"{form} multistart S={S} start {k}")
                         for k in range(S))
            assert exempt <= max(1, S // 1000), (form, S, exempt)
            _stat(form)["exempt"] += exempt
            _stat(form)["multistart"].append(S)
            if S == 1:
                pb, sb = sv.solve_batched(x0, o)
                assert np.array_equal(pb, pm) and _key(sb[0]) == _key(sm[0]), form
    for form in (256, 512, "z"):
        _summary(form)
