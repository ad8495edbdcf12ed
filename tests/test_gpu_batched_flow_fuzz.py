"""Seeded shape and pose-branch fuzz of clc_closed_form_batched / clc_information_batched (K8 / K9, csrc/clc_batchflow.hpp) on the
constructed batches of tests/batched_flow_cases.py (checked without a GPU by tests/test_batched_flow_cases.py, where the oracle alone
meets the gates against an exact statement): chosen blocks_per_problem (1, 2, 7, 8, 9, 15, 16, 17; set by the longest problem and by
the batch size), problems with fewer rows than workgroups and than waves beside a long one, ragged scans, the row layout with z, the
tile layout at n = 1 .. 1025 with its odd tails, every branch of the start pose's quaternion, rank-deficient systems, four kinds of
analysis pose.

Per batch: the layout taken (path_info().batched_rows_layout, the number behind Solver.debug_rows(): 0 tiles, 1 rows, 2 rows with z) and
the blocks_per_problem reached (launch_paths_ref, on this device's CU count) are the ones meant — a batch that misses either fails;
every problem against the oracle and the single-problem calls with the helpers and gates of tests/test_gpu_batched_flow.py (unobservable
problems: finite and equal to clc_closed_form on the problem alone); H V = V sv to 1e-9 sv[0] and V^T V = I to 1e-12; no problem within
a factor of 10 of the 1e-10 / 1e-8 thresholds (0 excused, cap 5).
Bitwise: the same problems uploaded in three orders, and with one neighbour's records replaced by others of the same scan lengths, give
every problem the same bits in every output.  Empty problems first, last, two adjacent: CLC_ERR_NO_DATA, pose untouched, zero
information with n_null = 6, and their neighbours the same bits as beside a one-record problem in those slots.
The last test prints the worst differences against the oracle.  Measured on the MI355X (256 CUs): 32 batches, 1772 problems, 0 excused,
worst |dTlc| 5.1e-13, sv9 5.0e-15 of the largest, H 4.8e-15, b 2.0e-10 (the oracle's own cancellation: 1.7e-10 against exact sums),
chi2 4.3e-14."""
import numpy as np
import pytest

import batched_flow_cases as F
import camlasercalibratool_amd as clc
import test_gpu_batched_flow as GB    # _check_closed_form, _check_information, _upload (the module is imported, not its tests)
from camlasercalibratool_amd import simdata as sd

pytestmark = pytest.mark.gpu

STATS = {"batches": 0, "problems": 0, "excused": 0, "Tlc": 0.0, "sv9": 0.0, "H": 0.0, "b": 0.0, "chi2": 0.0, "bpp": set(), "branch": {}}
BITWISE_KINDS = ("cf", "far")


@pytest.fixture(scope="module")
def sv():
    with clc.Solver(0) as s:
        yield s


@pytest.fixture(scope="module")
def single():
    with clc.Solver(0) as s:
        yield s


@pytest.fixture(scope="module")
def cus(sv):
    return sv.device_info()[1]


def _upload(sv, b, cus):
    """Upload; the layout and the blocks_per_problem are the ones the batch was built to reach, or the test fails."""
    GB._upload(sv, b.recs)
    assert sv.path_info().batched_rows_layout == b.layout, (b.name, sv.path_info().batched_rows_layout, b.layout)
    if b.meant_bpp is not None:
        assert b.bpp(cus) == b.meant_bpp, (b.name, cus, b.bpp(cus), b.meant_bpp)
    return b.bpp(cus)


def _run(sv, b, cus, poses=None):
    """-> (closed form outputs, {kind: information outputs}, the poses used).  poses: dict kind -> [P, 7] (default: info_poses of
    this run's own closed form)."""
    _upload(sv, b, cus)
    cf = sv.closed_form_batched(np.full((b.P, 7), 7.0))
    if poses is None:
        poses = F.info_poses(b, cf[0], (cf[3] == 0) & ~cf[1])
    return cf, {kind: sv.information_batched(poses[kind]) for kind in poses}, poses


def _same_bits(a, i, b, j, what):
    """Problem i of run a = problem j of run b, in every output."""
    (cfa, infa, _), (cfb, infb, _) = a, b
    for x, y, nm in zip(cfa, cfb, ("Tlc", "unobservable", "sv9", "status", "pose")):
        assert np.array_equal(x[i], y[j], equal_nan=(nm in ("Tlc", "sv9"))), (what, i, j, nm)
    for kind in infa:
        for x, y, nm in zip(infa[kind], infb[kind], ("H", "b", "chi2", "sv", "V", "n_null")):
            assert np.array_equal(x[i], y[j]), (what, i, j, kind, nm)


def _eigen(H, s6, V):
    assert np.abs(H @ V - V * s6).max() <= 1e-9 * s6[0]
    assert np.abs(V.T @ V - np.eye(6)).max() <= 1e-12


@pytest.mark.parametrize("name", F.NAMES)
def test_batch_against_the_oracle_and_the_single_calls(sv, single, cus, oracle_mod, name):
    b = F.batch(name, cus)
    STATS["bpp"].add(_upload(sv, b, cus))
    T, un, sv9, st, poses = GB._check_closed_form(sv, single, oracle_mod, b.recs)
    usable = (st == 0) & ~un
    kinds = F.info_poses(b, T, usable)
    info = {kind: GB._check_information(sv, single, oracle_mod, b.recs, kinds[kind]) for kind in b.pose_kinds}
    for k, p in enumerate(b.problems):
        if p.n == 0:
            assert st[k] == GB.CLC_ERR_NO_DATA and np.all(poses[k] == 7.0) and np.isnan(T[k]).all()
            for H, bb, chi2, s6, V, nn in info.values():
                assert np.all(H[k] == 0.0) and np.all(bb[k] == 0.0) and chi2[k] == 0.0 and np.all(s6[k] == 0.0) and nn[k] == 6, (name, k)
            continue
        T0, un0, s90 = oracle_mod.closed_form(p.rec)
        s60 = []
        for kind, (H, bb, chi2, s6, V, nn) in info.items():
            _eigen(H[k], s6[k], V[k])
            H0, b0, c0, s6o, _, _ = oracle_mod.information(p.rec, kinds[kind][k])
            s60.append(s6o)
            STATS["H"] = max(STATS["H"], float(np.max(np.abs(H[k] - H0) / (np.abs(H0) + 1e-8 / 1e-11))))
            STATS["b"] = max(STATS["b"], float(np.max(np.abs(bb[k] - b0) / (np.abs(b0) + 1e-14 / 1e-9))))
            STATS["chi2"] = max(STATS["chi2"], abs(chi2[k] - c0) / (c0 + 1e-26 / 1e-11))
        near = F.near_threshold(s90, s60)
        STATS["excused"] += near
        assert not near, (name, k, p.tag)       # (no case of this module sits at a threshold: every flag above was compared)
        STATS["sv9"] = max(STATS["sv9"], float(np.abs(sv9[k] - s90).max() / s90[0]))
        if usable[k]:
            STATS["Tlc"] = max(STATS["Tlc"], float(np.abs(T[k] - T0).max()))
            q = sd.rot_to_quat_wxyz(T[k][:3, :3].T)
            assert np.array_equal(np.sign(poses[k][[6, 3, 4, 5]]), np.sign(q)), (name, k, poses[k], q)   # same branch, same sign
            br = F.quat_branch(T[k][:3, :3].T)
            STATS["branch"][br] = STATS["branch"].get(br, 0) + 1
            if p.truth is not None and p.kind == "fit" and p.tag != "sv9 threshold":
                assert np.abs(np.linalg.inv(T[k]) - p.truth).max() < 0.05, (name, k)    # the truth the records were built on (1 cm of noise)
        STATS["problems"] += 1
    STATS["batches"] += 1
    if name == "rot":
        want = {nm: br for nm, _, br in F.rotations()}
        got = {p.tag: F.quat_branch(T[k][:3, :3].T) for k, p in enumerate(b.problems)}
        assert got == want, got
    if name == "rank":
        tags = [p.tag for p in b.problems]
        assert not un[tags.index("sv9 threshold")] and not un[tags.index("d = 0")] and un[tags.index("parallel exact")]
        assert np.all(T[tags.index("d = 0")][:3, 3] == 0.0)


@pytest.mark.parametrize("name", F.NAMES)
def test_same_bits_in_any_order_and_beside_other_records(sv, cus, name):
    b = F.batch(name, cus)
    base = _run(sv, b, cus)
    poses = {kind: base[2][kind] for kind in BITWISE_KINDS}
    base = (base[0], {kind: base[1][kind] for kind in BITWISE_KINDS}, poses)
    for perm in F.permutations(b)[1:]:
        pb = b.with_problems(b.name, [b.problems[i] for i in perm])
        run = _run(sv, pb, cus, {kind: np.ascontiguousarray(poses[kind][perm]) for kind in poses})
        for i, j in enumerate(perm):
            _same_bits(run, i, base, int(j), (name, perm.tolist()))
    j, rb = F.replaced_neighbour(b)
    run = _run(sv, rb, cus, poses)
    for k in range(b.P):
        if k != j:
            _same_bits(run, k, base, k, (name, "replaced", j))
    assert not np.array_equal(run[0][2][j], base[0][2][j])      # (problem j itself did change)


@pytest.mark.parametrize("family", ["hetero", "hetero_z"])
def test_empty_problems_leave_their_neighbours_alone(sv, cus, family):
    for where in ("", "_first", "_last", "_adjacent"):
        e, o = F.batch(family + where, cus), F.batch(family + where + "_one", cus)
        slots = [k for k, p in enumerate(e.problems) if p.n == 0]
        assert slots and [k for k in range(e.P) if e.problems[k] is not o.problems[k]] == slots
        run_e = _run(sv, e, cus)
        poses = run_e[2]
        run_o = _run(sv, o, cus, poses)
        (T, un, sv9, st, p7), info, _ = run_e
        for k in range(e.P):
            if k in slots:
                assert st[k] == GB.CLC_ERR_NO_DATA and np.all(p7[k] == 7.0) and run_o[0][3][k] == 0
                for H, bb, chi2, s6, V, nn in info.values():
                    assert not H[k].any() and not bb[k].any() and chi2[k] == 0.0 and not s6[k].any() and nn[k] == 6
            else:
                assert st[k] == 0
                _same_bits(run_e, k, run_o, k, (family + where, "empty | one record"))


def test_prints_what_the_module_saw(cus):
    s = STATS
    print(f"batched-flow fuzz on {cus} CUs: {s['batches']} batches, {s['problems']} problems against the oracle, {s['excused']} excused "
          f"at a threshold (cap 5); blocks_per_problem reached {sorted(s['bpp'])}; start-pose branches {dict(sorted(s['branch'].items()))}; "
          f"worst |dTlc| {s['Tlc']:.2e} (gate 1e-9), sv9 {s['sv9']:.2e} of the largest (1e-9), H {s['H']:.2e} (1e-11), b {s['b']:.2e} (1e-9), "
          f"chi2 {s['chi2']:.2e} (1e-11)")
    if s["batches"] == len(F.NAMES):      # (the whole module ran)
        assert set(F.INTENDED_BPP) <= s["bpp"] and all(s["branch"].get(br, 0) >= 2 for br in ("t", "i0", "i1", "i2"))
        assert s["excused"] <= 5
