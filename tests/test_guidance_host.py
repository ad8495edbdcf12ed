"""K20 (csrc/clc_guidance.hpp) on the host: the cast, the score, the order of the argmax and the round's update compiled with g++
(tests/shim/guidance_shim.cpp) against the numpy restatement tests/guidance_ref.py on the cases of tests/guidance_cases.py: counts,
H_add, eigenvalues and scores; H_add against the oracle's analysis pass of the recording with the pose appended; the greedy order on
the two degenerate sets and what it buys; the edge semantics; the refusals of the C ABI (they need no device); a stand-alone
AddressSanitizer / UBSan program over the edge shapes."""
import ctypes as C
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import guidance_cases as cases  # noqa: E402
import guidance_ref as ref  # noqa: E402
from camlasercalibratool_amd import _capi, simdata  # noqa: E402

GXX = ["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off"]

# The ceiling set for H_add and the eigenvalues is 1e-12 of max|M|, M = H0 + H_add.  The bounds are one decade over the worst gaps
# measured on the 2 x 512 candidates of the degenerate sets and the shape cases (the figures: test_scores_match_restatement).
GATE = 1e-12
H_BOUND = 5e-16     # largest |H_add - restatement| / max|M| (measured 5.0e-17)
SV_BOUND = 3.0e-14  # largest |sv - eigvalsh| / max|M| (measured 2.4e-15 on the sets, 3.0e-15 on the 1 x 257 shape case)
# The score given the eigenvalues (ceiling: 1e-12 absolute per eigenvalue's log): on the host the gap is 0, the same libm.  The
# bound comes from the formats, for a device whose log is another library's: six logs of magnitude <= 18.5, each library within 1 ulp
# (3.6e-15), and five additions at |score| <= 111 (ulp 1.4e-14).
LOG_BOUND = 1.4e-13
assert H_BOUND < GATE and SV_BOUND < GATE and LOG_BOUND < 6e-12
KINDS = list(cases.DEGENERATE)


def V(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def build_shim(path):
    subprocess.check_call(GXX + ["-shared", os.path.join(HERE, "shim", "guidance_shim.cpp"), "-o", path])
    return C.CDLL(path)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(str(tmp_path_factory.mktemp("gd") / "libguidance_shim.so"))


def options_of(model, o=None):
    """A ref.Model as clc_guidance_options."""
    o = o or _capi.GuidanceOptions()
    o.n_rays, o.min_points, o.criterion, o.reserved = model.n_rays, model.min_points, model.criterion, 0
    o.angle_min, o.angle_increment, o.range_min, o.range_max = model.angle_min, model.angle_increment, model.range_min, model.range_max
    o.eig_floor = model.eig_floor
    for i in range(2):
        o.board_min[i], o.board_max[i] = model.board_min[i], model.board_max[i]
    return o


def shim_score(L, model, pose_cl, H0, q, t, table=True):
    """shim_score_board_poses -> dict, the keys of Solver.score_board_poses."""
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 4)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 3)
    n = q.shape[0]
    nh = np.full(n, -99, dtype=np.int32); Ha = np.full((n, 6, 6), np.nan); sv = np.full((n, 6), np.nan); sc = np.full(n, np.nan)
    o = options_of(model)
    H = None if H0 is None else np.ascontiguousarray(H0, dtype=np.float64)
    L.shim_score_board_poses(C.byref(o), V(np.ascontiguousarray(pose_cl)), V(H), C.c_longlong(n), V(q), V(t), C.c_int(int(table)), V(nh), V(Ha),
                             V(sv), V(sc))
    return dict(n_hits=nh, H_add=Ha, sv=sv, score=sc)


def shim_select(L, model, pose_cl, H0, q, t, k):
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 4)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 3)
    ch = np.full(k, -99, dtype=np.int64); sva = np.empty((k, 6)); sca = np.empty(k); Hf = np.empty((6, 6)); nc = C.c_int32(-1)
    o = options_of(model)
    H = None if H0 is None else np.ascontiguousarray(H0, dtype=np.float64)
    L.shim_select_board_poses(C.byref(o), V(np.ascontiguousarray(pose_cl)), V(H), C.c_longlong(q.shape[0]), V(q), V(t), C.c_longlong(k), V(ch),
                              V(sva), V(sca), V(Hf), C.byref(nc))
    return dict(chosen=ch, sv_after=sva, score_after=sca, H_after=Hf, n_chosen=nc.value)


def score_bound(model, sv, maxM):
    """What the eigenvalue bound allows the score to differ by, to first order: LOGDET sum_k SV_BOUND max|M| / max(sv_k, eig_floor) plus
    the logs' own bound; MIN_EIG the eigenvalue bound itself."""
    if model.criterion == ref.MIN_EIG:
        return SV_BOUND * maxM
    return float((SV_BOUND * maxM / np.maximum(sv, model.eig_floor)).sum()) + LOG_BOUND


def gaps(got, want, model, H0):
    """The gaps of a score call to the restatement's -> dict(H, sv: relative to max|M|; log: the score given the call's own
    eigenvalues; score: end to end; score_cond: the first-order bound of the end-to-end gap that SV_BOUND implies)."""
    M0 = np.zeros((6, 6)) if H0 is None else np.asarray(H0).reshape(6, 6)
    maxM = np.abs(M0[None] + want["H_add"]).max(axis=(1, 2))
    maxM = np.where(maxM > 0, maxM, 1.0)
    own = np.array([ref.score_of(model, s) for s in got["sv"]])
    cond = np.array([score_bound(model, want["sv"][i], maxM[i]) for i in range(len(maxM))])
    return dict(H=float((np.abs(got["H_add"] - want["H_add"]).max(axis=(1, 2)) / maxM).max()),
                sv=float((np.abs(got["sv"] - want["sv"]).max(axis=1) / maxM).max()),
                log=float(np.abs(got["score"] - own).max()),
                score=float(np.abs(got["score"] - want["score"]).max()),
                score_over_cond=float((np.abs(got["score"] - want["score"]) / cond).max()))


def assert_matches(got, want, model, H0, what=""):
    g = gaps(got, want, model, H0)
    print(what, "gaps", g)
    assert np.array_equal(got["n_hits"], want["n_hits"]), what
    assert g["H"] <= H_BOUND and g["sv"] <= SV_BOUND and g["log"] <= LOG_BOUND, (what, g)
    assert g["score_over_cond"] <= 1.0, (what, g)
    return g


def test_options_struct_and_defaults(shim):
    assert shim.shim_guidance_options_size() == C.sizeof(_capi.GuidanceOptions) == 88
    o = _capi.GuidanceOptions()
    shim.shim_guidance_options_default(C.byref(o))
    d = ref.Model()
    # the geometry of simdata.sim_laser_scans, bit for bit
    assert (o.n_rays, o.min_points, o.criterion) == (1081, 50, _capi.GUIDE_LOGDET)
    assert o.angle_min == d.angle_min == -np.deg2rad(270.0) / 2 and o.angle_increment == d.angle_increment
    assert (o.range_min, o.range_max, o.eig_floor) == (0.05, 30.0, 1e-8)
    assert list(o.board_min) == [-0.043, -0.043] and list(o.board_max) == [0.457, 0.457]


@pytest.mark.parametrize("kind", KINDS)
def test_scores_match_restatement(shim, kind):
    """n_hits equal; H_add, sv and the score against the restatement on the 512 candidates of each degenerate set.  Measured (both sets):
    H_add 5.0e-17 and sv 2.4e-15 of max|M| (bounds 5e-16, 3.0e-14, under the 1e-12 ceiling); the score given the eigenvalues 0
    (bound 1.4e-13 from the formats, under 6 x 1e-12).  FINDING: end to end the score differs from the restatement's by up to 5.4e-8 (only_pitch) and
    4.9e-10 (parallel_boards; 5.8e-7 on the 1 081 x 4 shape case), far over 1e-12 per log: a candidate can lift a null eigenvalue to just above eig_floor = 1e-8, where an
    absolute eigenvalue error of 1e-15 max|M| is 1e-6 of the eigenvalue and so of its log.  No implementation can do better than the
    conditioning: H_add itself differs by 5e-17 max|M|.  That gap is therefore held to the first-order bound the eigenvalue bound
    implies, sum_k SV_BOUND max|M| / max(sv_k, eig_floor), and the rounds' best scores lie 4e-5 relative apart at the least."""
    c = cases.degenerate(kind)
    got = shim_score(shim, c["model"], c["pose_cl"], c["H0"], c["q"], c["t"])
    g = assert_matches(got, c["ref"], c["model"], c["H0"], kind)
    seen = c["ref"]["n_hits"] >= 50
    print(kind, "seen", int(seen.sum()), "median hits", float(np.median(c["ref"]["n_hits"][seen])), "margin", c["margin"], "round gap", c["gap"], g)
    assert 0.4 < seen.mean() < 0.65
    # per-ray sincos instead of the table: the same code path of the directions on the host, the same bits
    again = shim_score(shim, c["model"], c["pose_cl"], c["H0"], c["q"][:32], c["t"][:32], table=False)
    for k in ("n_hits", "H_add", "sv", "score"):
        assert np.array_equal(again[k], got[k][:32]), k


@pytest.mark.parametrize("n_rays", cases.N_RAYS)
def test_shapes_match_restatement(shim, n_rays):
    for n in cases.N_CAND[:-1] if n_rays == 1081 else cases.N_CAND:
        c = cases.shape(n_rays, n)
        assert_matches(shim_score(shim, c["model"], c["pose_cl"], c["H0"], c["q"], c["t"]), c["ref"], c["model"], c["H0"], f"{n_rays}x{n}")
    c = cases.shape(n_rays, 5)
    m = replace(c["model"], criterion=ref.MIN_EIG)
    want = ref.score_all(m, c["pose_cl"], c["H0"], c["q"], c["t"])
    got = shim_score(shim, m, c["pose_cl"], c["H0"], c["q"], c["t"])
    assert_matches(got, want, m, c["H0"], "min_eig")
    assert np.array_equal(got["score"], got["sv"][:, 5])


# The oracle adds J^T J point by point, J = u / sqrt(c): its sum and the restatement's per-pose products differ by 6.4e-16 and 1.7e-14 of
# max|H| on the 2 400 points of the two sets, and the difference of two such sums from H_add by 7.1e-15; one decade over the largest.
ORACLE_BOUND = 1.7e-13
assert ORACLE_BOUND < GATE


def test_restated_information_is_the_oracles():
    import oracle
    for kind in KINDS:
        c = cases.degenerate(kind)
        H = oracle.information(oracle.flatten(c["obs"], False, False), c["pose_cl"])[0]
        gap = np.abs(H - c["H0"]).max() / np.abs(H).max()
        print(kind, "restated H0 against the oracle's, of max|H|:", gap)
        assert gap <= ORACLE_BOUND


@pytest.mark.parametrize("kind", KINDS)
def test_h_add_is_what_the_analysis_pass_gains(shim, kind):
    """For seen candidates: the oracle's analysis pass (its restatement of src/LaseCamCalCeres.cpp:316-381) of the recording with the
    restatement's hit points appended as one more observation, minus that of the recording, is H_add — within H_BOUND of max|M| plus
    what the oracle's own sums carry (ORACLE_BOUND)."""
    import oracle
    c = cases.degenerate(kind)
    obs = c["obs"]
    H_rec = oracle.information(oracle.flatten(obs, False, False), c["pose_cl"])[0]
    got = shim_score(shim, c["model"], c["pose_cl"], c["H0"], c["q"], c["t"])
    worst = 0.0
    for i in np.flatnonzero(c["ref"]["n_hits"] >= 50)[:24]:
        P = c["ref"]["pts"][i]
        ext = simdata.ObservationSet(np.vstack([obs.tag_q, c["q"][i]]), np.vstack([obs.tag_t, c["t"][i]]),
                                     np.append(obs.pts_off, obs.pts_off[-1] + len(P)), np.ascontiguousarray(np.vstack([obs.pts, P])),
                                     np.append(obs.ptl_off, obs.ptl_off[-1] + len(P)), np.ascontiguousarray(np.vstack([obs.ptl, P])))
        H_ext = oracle.information(oracle.flatten(ext, False, False), c["pose_cl"])[0]
        worst = max(worst, np.abs((H_ext - H_rec) - got["H_add"][i]).max() / np.abs(H_ext).max())
    print(kind, "identity gap / max|M|", worst)
    assert worst <= H_BOUND + ORACLE_BOUND


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_order_and_what_it_buys(shim, kind):
    """k = 6 of 512: chosen equal to the restatement's; sv_after, score_after, H_after within the bounds; lambda_min(H) after the six
    picks over lambda_min after the first six seen candidates: 6.9 (only_pitch: 0.474 / 0.0688), 7.6 (parallel_boards: 0.186 / 0.0245)."""
    c = cases.degenerate(kind)
    got = shim_select(shim, c["model"], c["pose_cl"], c["H0"], c["q"], c["t"], cases.K)
    want = c["greedy"]
    print(kind, "chosen", got["chosen"], "round gaps", want["gaps"])
    assert np.array_equal(got["chosen"], want["chosen"]) and got["n_chosen"] == cases.K
    maxM = np.abs(want["H_after"]).max()
    assert np.abs(got["H_after"] - want["H_after"]).max() <= cases.K * H_BOUND * maxM
    assert np.abs(got["sv_after"] - want["sv_after"]).max() <= SV_BOUND * maxM
    lam = float(np.linalg.eigvalsh(got["H_after"])[0])
    lam_first = cases.lambda_min_after(c, cases.first_seen(c))
    print(kind, "lambda_min after the picks", lam, "after the first six seen", lam_first, "ratio", lam / lam_first)
    assert lam > lam_first
    assert lam / lam_first > 5.0
    # the rounds are the score call's argmax, one after the other
    M = c["H0"].copy()
    for r in range(cases.K):
        s = shim_score(shim, c["model"], c["pose_cl"], M, c["q"], c["t"])
        ok = (s["n_hits"] >= 50) & ~np.isin(np.arange(512), got["chosen"][:r])
        best = int(np.flatnonzero(ok)[np.argmax(s["score"][ok])])
        assert best == got["chosen"][r]
        assert np.array_equal(s["sv"][best], got["sv_after"][r]) and s["score"][best] == got["score_after"][r]
        M = M + s["H_add"][best]
    assert np.array_equal(M, got["H_after"])


def test_greedy_runs_out_of_seen_candidates(shim):
    c = cases.degenerate("only_pitch")
    seen = np.flatnonzero(c["ref"]["n_hits"] >= 50)[:3]
    unseen = np.flatnonzero((c["ref"]["n_hits"] < 50))[:4]
    idx = np.sort(np.concatenate([seen, unseen]))
    got = shim_select(shim, c["model"], c["pose_cl"], c["H0"], c["q"][idx], c["t"][idx], 9)
    assert got["n_chosen"] == 3 and np.all(got["chosen"][3:] == -1) and np.all(np.isnan(got["score_after"][3:]))
    assert sorted(idx[got["chosen"][:3]]) == sorted(seen)
    want = ref.greedy(c["model"], c["H0"], c["ref"]["n_hits"][idx], c["ref"]["H_add"][idx], 9)
    assert np.array_equal(got["chosen"], want["chosen"])


def test_ties_go_to_the_lowest_index(shim):
    c = cases.degenerate("only_pitch")
    i = int(np.flatnonzero(c["ref"]["n_hits"] >= 50)[0])
    q, t = np.repeat(c["q"][i:i + 1], 3, 0), np.repeat(c["t"][i:i + 1], 3, 0)
    got = shim_select(shim, c["model"], c["pose_cl"], c["H0"], q, t, 3)
    assert list(got["chosen"]) == [0, 1, 2]


def test_edge_semantics(shim):
    e = cases.edge_candidates()
    model, pose, H0 = ref.Model(), cases.POSE_CL, cases.degenerate("only_pitch")["H0"]
    score_H0 = ref.score_of(model, ref.eig_desc(H0))

    def one(name, m=model, H=H0):
        q, t = e[name]
        return {k: v[0] for k, v in shim_score(shim, m, pose, H, q[None], t[None]).items()}

    def unseen(r, hits):
        assert r["n_hits"] == hits and not r["H_add"].any(), r
        assert abs(r["score"] - score_H0) <= score_bound(model, ref.eig_desc(H0), np.abs(H0).max()), r

    # seen at min_points, unseen at min_points - 1
    q, t = e["facing_1m"]
    cases.check_margin(model, pose, q[None], t[None])
    c = ref.cast(model, pose, q, t)["n_hits"]
    assert c > 100
    at = one("facing_1m", replace(model, min_points=c))
    below = one("facing_1m", replace(model, min_points=c + 1))
    assert at["n_hits"] == below["n_hits"] == c and at["H_add"].any()
    unseen(below, c)
    assert np.array_equal(below["sv"], one("coplanar_above")["sv"])  # an unseen candidate scores as H0 itself: the same bits
    want = ref.score_all(replace(model, min_points=c), pose, H0, q[None], t[None])
    assert_matches({k: v[None] for k, v in at.items()}, want, model, H0, "facing")
    # m . dir = 0 for every ray: 0 / 0 and d_l / 0
    unseen(one("coplanar_in_plane"), 0)
    unseen(one("coplanar_above"), 0)
    # behind the laser: the rays about the x axis meet the board's plane inside the rectangle, at rho < 0
    q, t = e["behind"]
    k = ref.cast(model, pose, q, t)
    inside = (np.abs(k["X"] - 0.207) <= 0.25).all(axis=1)
    assert (inside & (k["rho"] < 0)).sum() > 20 and k["n_hits"] == 0
    unseen(one("behind", replace(model, min_points=1)), 0)
    # range_max: the same board at 29 m is hit, at 31 m it is not
    m1 = replace(model, min_points=1)
    for name in ("within_range", "beyond_range"):
        cases.check_margin(m1, pose, e[name][0][None], e[name][1][None])
    assert one("within_range", m1)["n_hits"] == ref.cast(m1, pose, *e["within_range"])["n_hits"] >= 1
    assert one("beyond_range", m1)["n_hits"] == 0
    # a non-finite candidate: n_hits -1, unseen, and its neighbours in the batch untouched
    for name in ("nan_q", "inf_t"):
        unseen(one(name), -1)
    q = np.stack([e["facing_1m"][0], e["nan_q"][0], e["facing_1m"][0]])
    t = np.stack([e["facing_1m"][1], e["nan_q"][1], e["facing_1m"][1]])
    b = shim_score(shim, model, pose, H0, q, t)
    alone = shim_score(shim, model, pose, H0, q[:1], t[:1])
    assert list(b["n_hits"]) == [c, -1, c]
    for k2 in ("H_add", "sv", "score"):
        assert np.array_equal(b[k2][0], alone[k2][0]) and np.array_equal(b[k2][2], alone[k2][0])
    # H0 NULL: the bits of H0 = 0
    z = shim_score(shim, model, pose, np.zeros((6, 6)), q, t)
    nul = shim_score(shim, model, pose, None, q, t)
    for k2 in ("n_hits", "H_add", "sv", "score"):
        assert np.array_equal(z[k2], nul[k2], equal_nan=True)
    assert np.array_equal(shim_select(shim, model, pose, None, q, t, 2)["H_after"], shim_select(shim, model, pose, np.zeros((6, 6)), q, t, 2)["H_after"])


REFUSED = [
    (dict(n_rays=0), "n_rays"), (dict(n_rays=-5), "n_rays"), (dict(n_rays=2 ** 24 + 1), "n_rays"), (dict(min_points=0), "min_points"),
    (dict(range_min=30.0), "range_min"), (dict(range_min=31.0), "range_min"), (dict(range_min=float("nan")), "range_min"),
    (dict(range_max=float("nan")), "range_min"), (dict(board_min=(0.5, 0.0)), "empty board"), (dict(board_max=(0.4, -0.05)), "empty board"),
    (dict(board_min=(float("nan"), 0.0)), "empty board"), (dict(eig_floor=0.0), "eig_floor"), (dict(eig_floor=-1e-8), "eig_floor"),
    (dict(eig_floor=float("nan")), "eig_floor"), (dict(criterion=2), "criterion"), (dict(criterion=-1), "criterion"),
    (dict(angle_min=float("inf")), "angle"), (dict(angle_increment=float("nan")), "angle"),
]


@pytest.mark.parametrize("change,text", REFUSED)
def test_every_refused_option(change, text):
    """The refusals come before any device work: no handle is needed to see them (a NULL handle is itself refused, after them)."""
    L = _capi.lib()
    o = options_of(replace(ref.Model(), **change))
    pose = np.ascontiguousarray(cases.POSE_CL)
    q, t = (np.ascontiguousarray(a[None]) for a in cases.edge_candidates()["facing_1m"])
    ch = np.zeros(1, dtype=np.int64)
    calls = {
        "clc_score_board_poses": lambda f: f(None, C.byref(o), V(pose), None, 1, V(q), V(t), None, None, None, None),
        "clc_score_board_poses_device": lambda f: f(None, C.byref(o), V(pose), None, 1, V(q), V(t), None, None, None, None),
        "clc_select_board_poses": lambda f: f(None, C.byref(o), V(pose), None, 1, V(q), V(t), 1, V(ch), None, None, None, None),
        "clc_select_board_poses_device": lambda f: f(None, C.byref(o), V(pose), None, 1, V(q), V(t), 1, V(ch), None, None, None, None),
    }
    for name, call in calls.items():
        assert call(getattr(L, name)) == -1, name
        msg = L.clc_last_error().decode()
        assert msg.startswith(name + ":") and text in msg, msg


def test_refusals_of_arguments():
    L = _capi.lib()
    pose = np.ascontiguousarray(cases.POSE_CL)
    q, t = (np.ascontiguousarray(a[None]) for a in cases.edge_candidates()["facing_1m"])
    ch = np.zeros(1, dtype=np.int64)
    bad_pose = pose.copy(); bad_pose[4] = np.nan
    bad_H = np.zeros(36); bad_H[7] = np.inf
    assert L.clc_score_board_poses(None, None, V(bad_pose), None, 1, V(q), V(t), None, None, None, None) == -3
    assert "non-finite pose" in L.clc_last_error().decode()
    assert L.clc_select_board_poses(None, None, V(pose), V(bad_H), 1, V(q), V(t), 1, V(ch), None, None, None, None) == -3
    assert "non-finite H0" in L.clc_last_error().decode()
    assert L.clc_score_board_poses(None, None, None, None, 1, V(q), V(t), None, None, None, None) == -1
    assert L.clc_select_board_poses(None, None, V(pose), None, 1, V(q), V(t), 0, V(ch), None, None, None, None) == -1
    assert "k must be" in L.clc_last_error().decode()
    assert L.clc_select_board_poses_device(None, None, V(pose), None, 1, V(q), V(t), 0, V(ch), None, None, None, None) == -1
    assert "k must be" in L.clc_last_error().decode()
    assert L.clc_score_board_poses(None, None, V(pose), None, 1, V(q), V(t), None, None, None, None) == -1  # NULL handle
    assert "bad argument" in L.clc_last_error().decode()


def test_sanitized_standalone_program(tmp_path):
    """tests/shim/guidance_sanitize_main.cpp: the host functions on the edge shapes, every array of its exact size, built with
    -fsanitize=address,undefined and run as an ordinary process."""
    exe = str(tmp_path / "guidance_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "shim", "guidance_sanitize_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "shapes ok" in p.stdout, p.stdout
