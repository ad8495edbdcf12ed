"""K17 (csrc/clc_altpose.hpp) on the host: the mirror start, the LM stage from it, the costs and the classification compiled with g++
(tests/shim/altpose_shim.cpp) against the numpy / scipy restatement tests/altpose_ref.py on the seeded images of
tests/altpose_cases.py; the 32-start search for a second minimum; the alternate of the alternate; the swap to the better pose; the
host half of calib.BoardPosesChecked; the option refusals of the C ABI (they need no device); and a stand-alone AddressSanitizer /
UBSan program over the edge shapes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import altpose_cases as cases  # noqa: E402
import altpose_ref as ref  # noqa: E402
import campose_ref as cref  # noqa: E402
import robustpose_cases as rcases  # noqa: E402
import test_campose_host as H  # noqa: E402
import test_robustpose_host as RH  # noqa: E402
from camlasercalibratool_amd import _capi, calib  # noqa: E402

CAMS = ["radtan", "kb"]
# the largest relative gap of cost_alt / cost_in to the restatement on the seeded sets, 1.6e-13, is asserted one decade over what
# was measured (test_seeded_views_match_restatement's docstring)
COST_GAP_BOUND = 2e-12
d = H._d


def build_shim(path):
    subprocess.check_call(RH.GXX + ["-shared", os.path.join(HERE, "shim", "altpose_shim.cpp"), "-o", path])
    L = C.CDLL(path)
    L.shim_kb_theta.restype = C.c_double
    L.shim_kb_theta.argtypes = [C.c_void_p, C.c_double]
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(str(tmp_path_factory.mktemp("ap") / "libaltpose_shim.so"))


def shim_options(L, **kw):
    ao = _capi.AltPoseOptions()
    L.shim_alt_options_default(C.byref(ao))
    for k, v in kw.items():
        setattr(ao, k, v)
    return ao


def shim_alt(L, cam, corners, board, off, mask, q_in, t_in, st_in, ao=None):
    """shim_board_poses_alternate -> dict of arrays, the keys of Solver.board_poses_alternate."""
    corners = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 2)
    board = np.ascontiguousarray(board, dtype=np.float32).reshape(-1, 2)
    off = np.ascontiguousarray(off, dtype=np.int64)
    n = len(off) - 1
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
    qi, ti = np.ascontiguousarray(q_in, dtype=np.float64), np.ascontiguousarray(t_in, dtype=np.float64)
    si = np.ascontiguousarray(st_in, dtype=np.int32)
    ao = ao or shim_options(L)
    real = {k: np.empty(n) for k in ("rms", "cost_in", "cost_alt", "ratio", "rot_angle", "normal_angle")}
    q = np.empty((n, 4)); t = np.empty((n, 3)); kind = np.empty(n, dtype=np.int32)
    amb = np.zeros(max(n, 1), dtype=np.uint8); bet = np.zeros(max(n, 1), dtype=np.uint8)
    sm = (_capi.Summary * max(n, 1))()
    o = _capi.Options()
    L.shim_pose_options_default(C.byref(o))
    c = cam.to_c()
    L.shim_board_poses_alternate(C.byref(c), C.byref(o), C.byref(ao), d(corners), d(board), d(off), C.c_longlong(n),
                                 None if m is None else d(m), d(qi), d(ti), d(si), d(q), d(t), d(real["rms"]), d(real["cost_in"]),
                                 d(real["cost_alt"]), d(real["ratio"]), d(real["rot_angle"]), d(real["normal_angle"]), d(kind), d(amb),
                                 d(bet), sm)
    return dict(real, q=q, t=t, kind=kind, ambiguous=amb[:n].astype(bool), better=bet[:n].astype(bool), summaries=sm)


def input_poses(L, cam, px_pose, boards, masks):
    """The input poses of a batch: K10 (the shim's) on every image's set — the corners its mask keeps, all of them where it keeps
    fewer than 4.  -> q [n, 4], t [n, 3], status [n]"""
    seq = []
    for px, b, m in zip(px_pose, boards, masks):
        m = np.ones(len(px), bool) if (m is None or m.sum() < 4) else m
        seq.append((px[m], b[m]))
    corners, board, off = rcases.csr(seq) if seq else (np.zeros((0, 2), np.float32),) * 2 + (np.zeros(1, np.int64),)
    q, t, _, st, _ = H.shim_board_poses(L, cam, corners, board, off)
    return q, t, st


def restate(L, cam, corners, board, off, mask, q_in, t_in, st_in, ao):
    lifted = H.shim_lift(L, cam, corners).astype(np.float32).astype(np.float64)
    rs = []
    for k in range(len(off) - 1):
        sl = slice(off[k], off[k + 1])
        rs.append(ref.alt_pose(lifted[sl], board[sl], None if mask is None else mask[sl], cref.quat_wxyz_to_R(q_in[k]), t_in[k], st_in[k],
                               ao.same_angle, ao.ratio_gate))
    return lifted, rs


def assert_input_condition(rs, ao):
    """The issue's input condition on the restatement's own numbers, no image left out: every rot_angle a factor >= 10 away from
    same_angle, every DISTINCT ratio at least 1e-3 (relative) away from ratio_gate and from 1."""
    for k, r in enumerate(rs):
        if r["kind"] == ref.NONE:
            continue
        a = r["rot_angle"]
        assert a <= ao.same_angle / 10 or a >= ao.same_angle * 10, (k, a)
        if r["kind"] == ref.DISTINCT:
            for g in (ao.ratio_gate, 1.0):
                assert abs(r["ratio"] - g) >= 1e-3 * g, (k, r["ratio"])


def two_tier(R, t, cost, R2, t2, cost2, what):
    """test_campose_host's rule between an LM answer and scipy started from it: 1e-9, or else 1e-7 at a cost no higher than scipy's
    x (1 + 1e-12)."""
    dR, dt = np.abs(R2 - R).max(), np.abs(t2 - t).max()
    if not (dR <= 1e-9 and dt <= 1e-9):
        assert dR <= 1e-7 and dt <= 1e-7, (what, dR, dt)
        assert cost <= cost2 * (1 + 1e-12), (what, cost, cost2)


def assert_matches_restatement(s, rs, lifted, board, off, mask):
    """kind and the flags exactly; poses by the two-tier rule against scipy started from the answer; the costs against the
    restatement: -> the largest relative gap of cost_in / cost_alt, for the caller to print and to hold against COST_GAP_BOUND"""
    gap = 0.0
    for k, r in enumerate(rs):
        assert s["kind"][k] == r["kind"], (k, s["kind"][k], r["kind"], s["rot_angle"][k], r["rot_angle"])
        assert s["ambiguous"][k] == bool(r["ambiguous"]) and s["better"][k] == bool(r["better"]), (k, s["ratio"][k], r["ratio"])
        if r["kind"] == ref.NONE:
            assert np.array_equal(s["q"][k], [1, 0, 0, 0]) and np.array_equal(s["t"][k], [0, 0, 0])
            assert all(np.isnan(s[key][k]) for key in ("rms", "cost_in", "cost_alt", "ratio", "rot_angle", "normal_angle")), k
            continue
        sl = slice(off[k], off[k + 1])
        m = np.ones(off[k + 1] - off[k], bool) if mask is None else np.asarray(mask[sl], bool)
        R = cref.quat_wxyz_to_R(s["q"][k])
        assert s["q"][k][0] >= 0
        R2, t2, sol = cref.pnp_lsq(lifted[sl][m], board[sl][m], R, s["t"][k])
        two_tier(R, s["t"][k], s["cost_alt"][k], R2, t2, 0.5 * np.sum(sol.fun ** 2), k)
        assert s["cost_alt"][k] == s["summaries"][k].final_cost
        for key in ("cost_in", "cost_alt"):
            g = abs(s[key][k] - r[key]) / r[key]
            gap = max(gap, g)
        assert abs(s["rms"][k] - np.sqrt(2 * s["cost_alt"][k] / m.sum())) <= 1e-15 + 1e-14 * s["rms"][k], k
        # the angles are those of the answer's own pose (the restatement's pose is scipy's from the mirror start, whose stopping in a
        # shallow minimum leaves it up to ~1e-4 rad off: the kinds above are what it is held to)
        assert abs(s["rot_angle"][k] - ref.rotation_angle(r["R_in"], R)) <= 1e-12 and abs(s["normal_angle"][k] - ref.normal_angle(r["R_in"], R)) <= 1e-12, k
    return gap


def test_struct_layout(shim):
    assert shim.shim_alt_options_size() == 16 == C.sizeof(_capi.AltPoseOptions)
    assert (_capi.AltPoseOptions.same_angle.offset, _capi.AltPoseOptions.ratio_gate.offset) == (0, 8)
    ao = shim_options(shim)
    assert ao.same_angle == 0.01 and ao.ratio_gate == 2.0
    assert (_capi.ALT_NONE, _capi.ALT_SAME, _capi.ALT_DISTINCT) == (0, 1, 2) == (ref.NONE, ref.SAME, ref.DISTINCT)


VIEWS = [("near", 6), ("far", 10), ("block4", 10), ("tag1", 6)]


def seeded(L, name):
    """The seeded views of one camera as one batch (plus contaminated boards under K16's mask) -> dict."""
    cam = cases.CAMERAS[name]
    imgs, kinds = [], []
    for kind, n in VIEWS:
        v = cases.view(name, kind, n)
        imgs += v
        kinds += [kind] * n
    corners, board, off = rcases.csr([(i[0], i[1]) for i in imgs])
    q, t, _, st, _ = H.shim_board_poses(L, cam, corners, board, off)
    return dict(cam=cam, imgs=imgs, kinds=np.array(kinds), corners=corners, board=board, off=off, mask=None, q=q, t=t, st=st)


def contaminated(L, name, n=4):
    cam = cases.CAMERAS[name]
    imgs = cases.dirty(name, n)
    corners, board, off = rcases.csr([(i[0], i[1]) for i in imgs])
    s = RH.shim_robust(L, cam, corners, board, off)
    return dict(cam=cam, imgs=imgs, kinds=np.array(["dirty"] * n), corners=corners, board=board, off=off, mask=s["inlier"], q=s["q"],
                t=s["t"], st=s["status"])


def run_both(L, e, ao=None):
    ao = ao or shim_options(L)
    s = shim_alt(L, e["cam"], e["corners"], e["board"], e["off"], e["mask"], e["q"], e["t"], e["st"], ao)
    lifted, rs = restate(L, e["cam"], e["corners"], e["board"], e["off"], e["mask"], e["q"], e["t"], e["st"], ao)
    return s, lifted, rs


@pytest.fixture(scope="module")
def seeded_runs(shim):
    out = {}
    for name in CAMS:
        e = seeded(shim, name)
        out[name] = (e,) + run_both(shim, e)
    return out


@pytest.mark.parametrize("name", CAMS)
def test_seeded_views_match_restatement(shim, seeded_runs, name):
    """kind, ambiguous and better equal the restatement on every image; poses and costs within the rules of
    assert_matches_restatement.  Measured on these sets (both cameras, contaminated boards included): the largest relative gap of
    cost_in / cost_alt to the restatement 1.6e-13 (the edge shapes: 1.0e-13), asserted at COST_GAP_BOUND = 2e-12, one decade over it.
    (The restatement restarts scipy at its own answer until the cost stops falling: its first answer from the mirror start sits up to
    1e-4 rad off in a shallow minimum — a gap of 2.6e-7 that was scipy's, the shim's cost being the lower one.  The issue expected about
    1e-8 from a 1e-7 pose error; both fits end much nearer than that.)  The largest SAME rot_angle 1.5e-9 rad (edge shapes: 3.4e-9) and
    the smallest DISTINCT one 0.354 rad, against same_angle = 0.01."""
    e, s, lifted, rs = seeded_runs[name]
    ao = shim_options(shim)
    assert np.all(e["st"] == 1)
    assert_input_condition(rs, ao)
    gap = assert_matches_restatement(s, rs, lifted, e["board"], e["off"], None)
    c = contaminated(shim, name)
    assert np.all(c["st"] == 1) and all(np.array_equal(c["mask"][c["off"][k]:c["off"][k + 1]], c["imgs"][k][2]) for k in range(len(c["imgs"])))
    sc, lc, rc = run_both(shim, c)
    assert_input_condition(rc, ao)
    gap = max(gap, assert_matches_restatement(sc, rc, lc, c["board"], c["off"], c["mask"]))
    same, dist = s["kind"] == 1, s["kind"] == 2
    print("%s: largest relative cost gap %.2e; SAME %d (largest rot_angle %.2e), DISTINCT %d (smallest rot_angle %.3f), ambiguous %d, "
          "better %d" % (name, gap, same.sum(), s["rot_angle"][same].max() if same.any() else 0.0, dist.sum(),
                         s["rot_angle"][dist].min() if dist.any() else np.nan, s["ambiguous"].sum(), s["better"].sum()))
    assert gap <= COST_GAP_BOUND
    for kind, _ in VIEWS:
        sel = e["kinds"] == kind
        print("  %-7s kinds %s ratio min %.3g" % (kind, np.bincount(s["kind"][sel], minlength=3), np.nanmin(np.where(s["kind"][sel] == 2, s["ratio"][sel], np.nan)) if (s["kind"][sel] == 2).any() else np.nan))
    # the views do what they are for: near ones are unambiguous, the far and small ones hold ambiguous images
    assert not s["ambiguous"][e["kinds"] == "near"].any() and np.all(sc["kind"] != 0) and not sc["ambiguous"].any()
    assert s["ambiguous"][e["kinds"] == "far"].any() and s["ambiguous"][e["kinds"] == "block4"].any()
    assert np.all(s["kind"] != 0)


@pytest.mark.parametrize("name", CAMS)
def test_brute_force_search_agrees_on_well_conditioned_sets(shim, seeded_runs, name):
    """On the sets of >= 4 tags the 32-start search finds a second minimum exactly where the call says DISTINCT, and it is the call's
    one within 1e-3 rad; it finds no third."""
    e, s, lifted, _ = seeded_runs[name]
    for k in np.flatnonzero(e["kinds"] != "tag1"):
        sl = slice(e["off"][k], e["off"][k + 1])
        R_in = cref.quat_wxyz_to_R(e["q"][k])
        found = ref.brute_minima(lifted[sl], e["board"][sl], R_in, e["t"][k])
        others = [f for f in found if ref.rotation_angle(f[0], R_in) > np.deg2rad(0.5)]
        assert len(found) - len(others) == 1, (k, len(found))
        if s["kind"][k] == 2:
            assert len(others) == 1, (k, len(others))
            assert ref.rotation_angle(others[0][0], cref.quat_wxyz_to_R(s["q"][k])) <= 1e-3, k
        else:
            assert len(others) == 0, (k, len(others))


@pytest.mark.parametrize("name", CAMS)
def test_alternate_of_the_alternate_is_the_input(shim, seeded_runs, name):
    """The call on its own DISTINCT answers gives the input pose back, kind DISTINCT, within the two-tier rule against the input pose
    itself.  Measured: the largest gap in R or t 4.9e-9 (radtan) and 8.8e-9 (kb) — the second tier, the returned cost no higher than
    cost_in of the first call."""
    e, s, lifted, _ = seeded_runs[name]
    worst = 0.0
    dist = np.flatnonzero(s["kind"] == 2)
    assert len(dist) >= 8
    st2 = np.where(s["kind"] == 2, 1, 0).astype(np.int32)
    back = shim_alt(shim, e["cam"], e["corners"], e["board"], e["off"], None, s["q"], s["t"], st2)
    for k in dist:
        assert back["kind"][k] == 2, k
        sl = slice(e["off"][k], e["off"][k + 1])
        R = cref.quat_wxyz_to_R(back["q"][k])
        # both are answers of the project's LM: scipy from the one ...
        R2, t2, sol = cref.pnp_lsq(lifted[sl], e["board"][sl], R, back["t"][k])
        two_tier(R, back["t"][k], back["cost_alt"][k], R2, t2, 0.5 * np.sum(sol.fun ** 2), k)
        # ... and the input pose itself, by the same rule
        R_in = cref.quat_wxyz_to_R(e["q"][k])
        worst = max(worst, np.abs(R - R_in).max(), np.abs(back["t"][k] - e["t"][k]).max())
        two_tier(R, back["t"][k], back["cost_alt"][k], R_in, e["t"][k], s["cost_in"][k], k)
        assert abs(back["cost_alt"][k] - s["cost_in"][k]) <= COST_GAP_BOUND * s["cost_in"][k], k
    print("%s: alternate of the alternate against the input pose, largest gap in R or t %.2e" % (name, worst))
    assert np.all(back["kind"][s["kind"] != 2] == 0)


FAR_IMAGES, FAR_SEED = 100, 100


def far_images(name, ids, dist, tilt):
    cam = cases.CAMERAS[name]
    rng = np.random.default_rng(FAR_SEED)
    b = cases.board_of(ids)
    imgs = []
    for _ in range(FAR_IMAGES):
        R, t = cases.tilted_pose(rng, b, dist, tilt)
        imgs.append((rcases.project(cam, b, R, t, rng), b, R, t))
    return imgs


@pytest.mark.parametrize("name", CAMS)
def test_better_swaps_to_the_pose_nearer_the_truth(shim, name):
    """`better` on an image whose input pose is the higher-cost minimum while the true pose lies in the lower one: the swap of
    BoardPosesChecked takes a pose whose normal is nearer the true one than the input's.
    On 4 m images of this kind (36 tags, tilt 15 degrees, the board centred in the view) K10's own DLT start did not end in the higher
    minimum (measured: 0 of 1000 seeded images, either camera; the search went no further than this tilt and these centred views — on
    10^4 random tilts at 3.5-4.5 m it does, 7 and 5 times, profiles/board_poses_alternate.md), so here the input is made the higher minimum: the first call's alternate pose, fed back in, on the first seeded
    image whose true pose lies on K10's side (it exists, asserted).  On the 2 x 2 block of tags at 2.5 m K10 itself ends in the higher
    minimum now and then (measured: 7 and 9 of 400): the first such seeded image with the truth on the other side is picked (it exists,
    asserted).  A 4 m image of this kind whose TRUE pose is the higher-cost minimum was not found either: 0 of the same 1000 seeded
    images, either camera (the ratio there: 1.34-1.52 in the median, never below 1 for a DISTINCT image)."""
    cam = cases.CAMERAS[name]
    err = lambda qq, R_true: ref.normal_angle(cref.quat_wxyz_to_R(qq), R_true)
    # ---- 4 m ----
    imgs = far_images(name, np.arange(36), 4.0, 15.0)
    corners, board, off = rcases.csr([(i[0], i[1]) for i in imgs])
    q, t, _, st, _ = H.shim_board_poses(shim, cam, corners, board, off)
    assert np.all(st == 1)
    s = shim_alt(shim, cam, corners, board, off, None, q, t, st)
    dist = s["kind"] == 2
    truth_lower = [k for k in np.flatnonzero(dist) if not s["better"][k] and err(s["q"][k], imgs[k][2]) > err(q[k], imgs[k][2])]
    print("%s 4 m: DISTINCT %d of %d, ambiguous %d, better %d" % (name, dist.sum(), FAR_IMAGES, s["ambiguous"].sum(), s["better"].sum()))
    assert len(truth_lower) >= 1
    k = truth_lower[0]
    sl = slice(off[k], off[k + 1])
    one = np.array([0, sl.stop - sl.start])
    s2 = shim_alt(shim, cam, corners[sl], board[sl], one, None, s["q"][k:k + 1], s["t"][k:k + 1], st[k:k + 1])  # the input: the higher minimum
    assert s2["kind"][0] == 2 and s2["better"][0] and s2["cost_alt"][0] < s2["cost_in"][0]
    q2, t2, _ = calib.checked_poses(s["q"][k:k + 1], s["t"][k:k + 1], st[k:k + 1], s2)
    assert np.array_equal(q2[0], s2["q"][0]) and np.array_equal(t2[0], s2["t"][0])
    before, after = err(s["q"][k], imgs[k][2]), err(q2[0], imgs[k][2])
    print("  image %d: normal error %.2f -> %.2f degrees" % (k, np.degrees(before), np.degrees(after)))
    assert after < before
    # ---- the block of four tags at 2.5 m: K10's own pose is the higher minimum ----
    imgs = far_images(name, cases.BLOCK4, 2.5, 15.0)
    corners, board, off = rcases.csr([(i[0], i[1]) for i in imgs])
    q, t, _, st, _ = H.shim_board_poses(shim, cam, corners, board, off)
    assert np.all(st == 1)
    s = shim_alt(shim, cam, corners, board, off, None, q, t, st)
    q2, t2, keep = calib.checked_poses(q, t, st, s)
    picked = [k for k in np.flatnonzero(s["better"]) if err(s["q"][k], imgs[k][2]) < err(q[k], imgs[k][2])]
    print("%s 2.5 m, 4 tags: DISTINCT %d of %d, better %d, of those with the truth on the lower side %d"
          % (name, (s["kind"] == 2).sum(), FAR_IMAGES, s["better"].sum(), len(picked)))
    assert len(picked) >= 1
    k = picked[0]
    assert s["kind"][k] == 2 and np.array_equal(q2[k], s["q"][k]) and np.array_equal(t2[k], s["t"][k])
    print("  image %d: normal error %.2f -> %.2f degrees, ratio %.3f" % (k, np.degrees(err(q[k], imgs[k][2])), np.degrees(err(q2[k], imgs[k][2])), s["ratio"][k]))
    assert err(q2[k], imgs[k][2]) < err(q[k], imgs[k][2])
    keepers = ~s["better"]  # nothing else moves
    assert np.array_equal(q2[keepers], q[keepers]) and np.array_equal(t2[keepers], t[keepers])


def test_checked_poses_logic():
    q = np.tile([1.0, 0, 0, 0], (5, 1)); t = np.arange(15.0).reshape(5, 3)
    alt = dict(q=np.tile([0.0, 1, 0, 0], (5, 1)), t=-np.ones((5, 3)), better=np.array([0, 1, 0, 1, 0], bool),
               ambiguous=np.array([0, 1, 1, 0, 0], bool))
    st = np.array([1, 1, 1, 1, -3])
    q2, t2, keep = calib.checked_poses(q, t, st, alt)
    assert np.array_equal(keep, [True, False, False, True, False])
    assert np.array_equal(q2[[1, 3]], alt["q"][[1, 3]]) and np.array_equal(t2[[1, 3]], alt["t"][[1, 3]])
    assert np.array_equal(q2[[0, 2, 4]], q[[0, 2, 4]]) and np.array_equal(t2[[0, 2, 4]], t[[0, 2, 4]])
    assert q[1, 0] == 1.0  # the inputs are left as they are


def edge_batch(L, name):
    """altpose_cases.edge_shapes as the arrays of one call, the input poses by the shim's K10 -> dict."""
    cam = cases.CAMERAS[name]
    images, notes = cases.edge_shapes(name)
    corners, board, off = rcases.csr([(i["px"], i["board"]) for i in images])
    mask = np.concatenate([i["mask"] for i in images])
    q, t, st = input_poses(L, cam, [i["px_pose"] for i in images], [i["board_pose"] for i in images], [i["mask"] for i in images])
    st = st.copy()
    for k, i in enumerate(images):
        if len(i["px"]) >= 4:
            assert st[k] == 1, k
        if i["bad_status"]:
            st[k] = -1
    return dict(cam=cam, images=images, notes=notes, corners=corners, board=board, off=off, mask=mask, q=q, t=t, st=st)


def assert_edge_kinds(kind, notes):
    got = {k: kind[v] for k, v in notes.items()}
    assert got["mask3"] == got["bad_status"] == got["nan_inside"] == got["nan_board_inside"] == got["empty"] == 0, got
    assert all(got[k] != 0 for k in ("n4", "n5", "n63", "n64", "n65", "n144", "far144", "mask4", "mask65", "after_bad_status",
                                     "nan_outside", "tail")), got


@pytest.mark.parametrize("name", CAMS)
def test_edge_shapes_match_restatement(shim, name):
    e = edge_batch(shim, name)
    s, lifted, rs = run_both(shim, e)
    assert_input_condition(rs, shim_options(shim))
    gap = assert_matches_restatement(s, rs, lifted, e["board"], e["off"], e["mask"])
    print("%s edge shapes: largest relative cost gap %.2e, kinds %s" % (name, gap, s["kind"]))
    assert gap <= COST_GAP_BOUND
    assert_edge_kinds(s["kind"], e["notes"])
    # an image alone gives the bits it gives in the batch
    for nm in ("mask65", "after_bad_status", "n65"):
        k = e["notes"][nm]
        sl = slice(e["off"][k], e["off"][k + 1])
        a = shim_alt(shim, e["cam"], e["corners"][sl], e["board"][sl], np.array([0, sl.stop - sl.start]), e["mask"][sl], e["q"][k:k + 1],
                     e["t"][k:k + 1], e["st"][k:k + 1])
        for key in ("q", "t", "cost_in", "cost_alt", "rot_angle", "kind"):
            assert np.array_equal(a[key][0], s[key][k]), (nm, key)


def alt_call(L, ao, h=None):
    c = H.CAMERAS["pinhole"].to_c()
    return L.clc_board_poses_alternate(h, C.byref(c), None, C.byref(ao) if ao is not None else None, None, None, None, C.c_size_t(0),
                                       *([None] * 16))


def test_option_refusals_need_no_device():
    """The C ABI checks the options before it touches the handle."""
    L = _capi.lib()
    base = _capi.default_alt_pose_options()
    assert base.same_angle == 0.01 and base.ratio_gate == 2.0
    who = "clc_board_poses_alternate: "
    nan, inf = float("nan"), float("inf")
    rows = [(dict(same_angle=v), "same_angle must be finite and > 0") for v in (nan, inf, 0.0, -0.01)]
    rows += [(dict(ratio_gate=v), "ratio_gate must be finite and >= 1") for v in (nan, inf, 0.999, -2.0)]
    for kw, msg in rows:
        ao = _capi.AltPoseOptions(base.same_angle, base.ratio_gate)
        for k, v in kw.items():
            setattr(ao, k, v)
        assert alt_call(L, ao) == -1
        assert L.clc_last_error().decode() == who + msg
    for ao in (base, _capi.AltPoseOptions(1e-6, 1.0), None):  # good options: the call gets as far as the missing handle
        assert alt_call(L, ao) == -1
        assert L.clc_last_error().decode() == who + "bad argument"


def test_sanitized_standalone_program(tmp_path):
    """tests/shim/altpose_sanitize_main.cpp: the per-image host function on the edge shapes, every array of its exact size, built with
    -fsanitize=address,undefined and run as an ordinary process."""
    exe = str(tmp_path / "altpose_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "shim", "altpose_sanitize_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "shapes ok" in p.stdout, p.stdout
