"""Seeded cases of the pose guidance (K20) and the conditions that keep a comparison with the restatement honest.  The conditions are
checked on the restatement (tests/guidance_ref.py) alone; a case that violates one raises — it is a test error, never a skip.

  condition 1   every in-range intersection lies at least MARGIN = 1e-9 m from the rectangle's edge, and every finite range at least
                as far from both range limits: a last-bit difference of a direction's sin / cos cannot change a count
  condition 2   in every greedy round the best and the second-best score differ by at least GAP = 1e-6 relative: rounding cannot
                decide an order

Smallest figures of the cases here: margin 2.0e-6 m over the 2 x 512 candidates of the degenerate sets; the gaps are printed by
tests/test_guidance_host.py."""
import functools
import os
import sys
from dataclasses import replace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import guidance_ref as ref  # noqa: E402
from camlasercalibratool_amd import simdata  # noqa: E402

MARGIN, GAP = 1e-9, 1e-6
TCL = simdata.tlc_to_tcl(simdata.GT_RLC, simdata.GT_TLC)
POSE_CL = simdata.pose7_from_T(TCL)
BOARD_CENTRE = (0.207, 0.207)
DEGENERATE = {"only_pitch": 1, "parallel_boards": 2}  # kind -> seed of its 512 candidates
K = 6
N_RAYS = (1, 63, 64, 65, 1081)
N_CAND = (1, 3, 4, 5, 257)


def check_margin(model, pose_cl, q, t):
    """Condition 1 -> the smallest margin of the candidates."""
    g = min(ref.margin(model, pose_cl, q[i], t[i]) for i in range(len(q)))
    if not g >= MARGIN:
        raise AssertionError(f"case violates condition 1: margin {g:.3e} m < {MARGIN:.0e}")
    return g


def check_gaps(gaps):
    """Condition 2 -> the smallest gap of the rounds."""
    g = min(gaps) if gaps else np.inf
    if not g >= GAP:
        raise AssertionError(f"case violates condition 2: relative gap {g:.3e} < {GAP:.0e}")
    return g


@functools.lru_cache(maxsize=None)
def degenerate(kind):
    """One of simdata.sim_degenerate's sets with 512 seeded candidates: dict(obs, pose_cl, H0, model, q, t, ref (score_all), greedy,
    margin, gap).  The restatement's results are computed once and shared; treat them as read-only."""
    obs = simdata.sim_degenerate(kind)
    model = ref.Model()
    H0 = ref.information(obs, POSE_CL)
    q, t = simdata.candidate_board_poses(DEGENERATE[kind], 512, TCL)
    r = ref.score_all(model, POSE_CL, H0, q, t)
    g = ref.greedy(model, H0, r["n_hits"], r["H_add"], K)
    return dict(kind=kind, obs=obs, pose_cl=POSE_CL, H0=H0, model=model, q=q, t=t, ref=r, greedy=g,
                margin=check_margin(model, POSE_CL, q, t), gap=check_gaps(g["gaps"]))


def first_seen(case, k=K):
    """The first k seen candidates: what a user without guidance might record."""
    return [int(i) for i in np.flatnonzero(case["ref"]["n_hits"] >= case["model"].min_points)[:k]]


def lambda_min_after(case, idx):
    M = case["H0"].copy()
    for i in idx:
        M = M + case["ref"]["H_add"][i]
    return float(np.linalg.eigvalsh(M)[0])


def model_for(n_rays):
    """A scan of n_rays rays over 1.2 rad about the laser's x axis; a seen pose needs an eighth of them."""
    if n_rays == 1081:
        return ref.Model()
    inc = 1.2 / (n_rays - 1) if n_rays > 1 else 0.0
    return replace(ref.Model(), n_rays=n_rays, angle_min=-0.6 if n_rays > 1 else 0.01, angle_increment=inc, min_points=max(1, n_rays // 8))


@functools.lru_cache(maxsize=None)
def shape(n_rays, n_cand):
    """Seeded candidates close to the laser for the shape tests: dict(model, pose_cl, H0, q, t, ref)."""
    model = model_for(n_rays)
    q, t = simdata.candidate_board_poses(1000 + n_rays + n_cand, n_cand, TCL, dist=(0.8, 1.6), bearing=0.4)
    H0 = degenerate("only_pitch")["H0"]
    check_margin(model, POSE_CL, q, t)
    return dict(model=model, pose_cl=POSE_CL, H0=H0, q=q, t=t, ref=ref.score_all(model, POSE_CL, H0, q, t))


def board_in_laser(R_lb, centre_l):
    """T_ca of a board whose axes are the columns of R_lb and whose centre is centre_l, both in the laser frame -> (q_wxyz, t)."""
    Rca = TCL[:3, :3] @ np.asarray(R_lb, dtype=np.float64)
    c = TCL[:3, :3] @ np.asarray(centre_l, dtype=np.float64) + TCL[:3, 3]
    t = c - Rca[:, 0] * BOARD_CENTRE[0] - Rca[:, 1] * BOARD_CENTRE[1]
    return simdata.rot_to_quat_wxyz(Rca), t


FACING = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])  # board x = laser y, board y = laser z, normal = laser x


def edge_candidates():
    """name -> (q, t): the boards of the edge semantics."""
    nan_q, nan_t = board_in_laser(FACING, [1.0, 0.0, 0.0])
    inf_q, inf_t = board_in_laser(FACING, [1.0, 0.0, 0.0])
    nan_q = nan_q.copy(); nan_q[2] = np.nan
    inf_t = inf_t.copy(); inf_t[0] = np.inf
    return {
        "facing_1m": board_in_laser(FACING, [1.0, 0.02, 0.01]),
        "coplanar_in_plane": board_in_laser(np.eye(3), [1.5, 0.0, 0.0]),     # d_l = 0: rho = 0 / 0
        "coplanar_above": board_in_laser(np.eye(3), [1.5, 0.0, 0.1]),        # rho = -d_l / 0
        "behind": board_in_laser(FACING, [-1.5, 0.02, 0.01]),                # the rays about the x axis meet it at rho < 0
        "beyond_range": board_in_laser(FACING, [31.0, 0.02, 0.01]),
        "within_range": board_in_laser(FACING, [29.0, 0.02, 0.01]),
        "nan_q": (nan_q, nan_t),
        "inf_t": (inf_q, inf_t),
    }
