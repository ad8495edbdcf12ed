"""clc_score_blocks and the consensus rule without a GPU: the symbol is declared, exported and bound (version still 210); the hook that
counts lane -> block map builds exists in the hooks build only; resample.consensus_select on hand-made tables; the frozen oracle
result of the consensus scenario (tests/golden/consensus_oracle.json) is what its generator (tests/tools/consensus_scenario.py)
produces today, and satisfies the separation conditions it was frozen under."""
import ctypes as C
import importlib.util
import json
import os
import re

import numpy as np
import pytest

from camlasercalibratool_amd import _build, _capi, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scenario():
    spec = importlib.util.spec_from_file_location("consensus_scenario", os.path.join(ROOT, "tests", "tools", "consensus_scenario.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_score_blocks_is_declared_exported_and_refuses_a_null_handle():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clc.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+clc_score_blocks\s*\(\s*clc_handle\s*\*", hdr)
    assert "clc_score_blocks" in _capi.EXPORTED and "clc_debug_lane_map_builds" in _capi.HOOKS
    off = (C.c_int64 * 2)(0, 1)
    pose = (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1)
    out = (C.c_double * 1)(-5.0)
    for path in (_build.PRODUCT_LIB_PATH, _build.HOOKS_LIB_PATH):
        L = _capi.load(path)
        assert L.clc_version() == 210
        rc = L.clc_score_blocks(None, None, 1, off, 1, pose, 0.03, out, None, None)
        assert rc == -1 and _capi.ERRORS[rc] == "CLC_ERR_INVALID_ARG"
        assert L.clc_last_error().decode().startswith("clc_score_blocks")
        assert out[0] == -5.0
    assert not hasattr(_capi.load(_build.PRODUCT_LIB_PATH), "clc_debug_lane_map_builds")
    n = C.c_longlong(-1)
    assert _capi.load(_build.HOOKS_LIB_PATH).clc_debug_lane_map_builds(C.byref(n)) == 0 and n.value >= 0


def test_python_adapters_exist():
    import camlasercalibratool_amd as clc
    assert callable(clc.Solver.score_blocks) and callable(clc.CamLaserCalibrationConsensus)
    with pytest.raises(TypeError, match="rms_max"):
        clc.CamLaserCalibrationConsensus([], np.eye(4), False, False)   # required: no default can be derived


def test_consensus_select_largest_support_wins():
    #                 block 0   1      2      3
    ssq = np.array([[1e-4, 1e-4, 9e-2, 9e-2],     # support 2
                    [2e-4, 2e-4, 2e-4, 9e-2],     # support 3  <- winner
                    [9e-2, 9e-2, 9e-2, 1e-5]])    # support 1
    best, mask, sizes = resample.consensus_select(ssq, 0.03)
    assert best == 1 and mask.dtype == bool and mask.tolist() == [True, True, True, False] and sizes.tolist() == [2, 3, 1]
    # the threshold is on the root, and it is inclusive
    best, mask, sizes = resample.consensus_select(np.array([[0.25, 0.26]]), 0.5)
    assert best == 0 and sizes.tolist() == [1] and mask.tolist() == [True, False]


def test_consensus_select_ties():
    # same support: the smaller sum over the SUPPORTING blocks wins (the huge score of a block outside the support does not count)
    ssq = np.array([[3e-4, 3e-4, 1.0],
                    [2e-4, 3e-4, 50.0],
                    [2e-4, 3e-4, 70.0]])
    best, mask, sizes = resample.consensus_select(ssq, 0.03)
    assert sizes.tolist() == [2, 2, 2] and best == 1 and mask.tolist() == [True, True, False]   # rows 1 and 2 tie on the sum: lower index
    # ... also when the tied rows support DIFFERENT blocks
    ssq = np.array([[1.0, 2e-4, 2e-4],
                    [2e-4, 2e-4, 1.0]])
    best, mask, _ = resample.consensus_select(ssq, 0.03)
    assert best == 0 and mask.tolist() == [False, True, True]
    # a larger support beats any sum
    ssq = np.array([[1e-9, 1.0, 1.0], [8e-4, 8e-4, 1.0]])
    assert resample.consensus_select(ssq, 0.03)[0] == 1


def test_consensus_select_empty_support_and_nan_rows():
    best, mask, sizes = resample.consensus_select(np.full((3, 4), 1.0), 0.03)
    assert best == -1 and not mask.any() and mask.shape == (4,) and sizes.tolist() == [0, 0, 0]
    best, mask, sizes = resample.consensus_select(np.zeros((0, 4)), 0.03)
    assert best == -1 and mask.shape == (4,) and sizes.shape == (0,)
    # a NaN row (a non-finite candidate) never wins, wherever it stands; a NaN cell supports nothing
    nan = np.full(3, np.nan)
    ssq = np.stack([nan, np.array([1e-4, 1.0, 1.0]), nan])
    best, mask, sizes = resample.consensus_select(ssq, 0.03)
    assert best == 1 and sizes.tolist() == [0, 1, 0] and mask.tolist() == [True, False, False]
    assert resample.consensus_select(np.stack([nan, nan]), 0.03)[0] == -1
    best, mask, sizes = resample.consensus_select(np.array([[np.nan, 1e-4, 1e-4], [1e-4, 1e-4, 1.0]]), 0.03)
    assert best == 0 and mask.tolist() == [False, True, True]   # tie on support 2: sums 2e-4 both, lower index
    with pytest.raises(ValueError):
        resample.consensus_select(np.zeros(4), 0.03)


def test_frozen_oracle_result_is_what_the_generator_gives_and_separates(oracle_mod):
    sc = _scenario()
    want = json.load(open(sc.FIXTURE))
    got = sc.oracle_pipeline(oracle_mod, want["seed"])
    assert sc.separates(want) and sc.separates(got)
    assert got["best"] == want["best"] and got["inlier_mask"] == want["inlier_mask"] and got["bad_poses"] == want["bad_poses"]
    assert got["support"] == want["support"] == sc.N_POSES - sc.K_BAD
    assert want["support"] - want["support_of_best_other_mask"] >= 2 and want["tie_break_gap"] >= 1e-6
    # (another machine's libm may move the oracle's solves in the last bits: far inside the gates the GPU test applies)
    assert np.abs(np.array(got["refit_pose"]) - np.array(want["refit_pose"])).max() <= 1e-9
    assert abs(got["refit_cost"] - want["refit_cost"]) <= 1e-10
    print("plain solve |dT| vs ground truth", want["plain_max_abs_dT_vs_ground_truth"], "consensus refit",
          want["consensus_max_abs_dT_vs_ground_truth"])
