"""Interpolated tag poses and the clock sweep (K15) without a GPU: the C-ABI's new structs and symbols, the restatement
tests/interp_ref.py against scipy's Slerp, the margins of simoffline.moving_recording, and clc_clock_offset_best (host code) on
hand-made cost tables."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import interp_ref as IR
from camlasercalibratool_amd import _capi, simoffline as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("clc_interp_options_default", "clc_interpolate_poses", "clc_assemble_interpolated", "clc_assemble_interpolated_device",
       "clc_clock_offset_options_default", "clc_clock_offset_best", "clc_clock_offset_sweep", "clc_clock_offset_sweep_device")


def _struct_fields(name):
    hdr = open(os.path.join(ROOT, "include", "clc.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [m.group(2) for m in re.finditer(r"(double|int32_t|int64_t|clc_options|clc_interp_options)\s+(\w+)(?:\[\d+\])?;", body)]


def test_struct_layouts_match_header():
    assert _struct_fields("clc_interp_options") == [f[0] for f in _capi.InterpOptions._fields_]
    assert _struct_fields("clc_clock_offset_options") == [f[0] for f in _capi.TimeOffsetOptions._fields_]
    assert _struct_fields("clc_clock_offset_result") == [f[0] for f in _capi.TimeOffsetResult._fields_]
    assert C.sizeof(_capi.InterpOptions) == 4 * 8 + C.sizeof(_capi.Options) and _capi.InterpOptions.line.offset == 32
    assert C.sizeof(_capi.TimeOffsetOptions) == 2 * 8 + 2 * 4 + C.sizeof(_capi.InterpOptions) + C.sizeof(_capi.Options)
    assert _capi.TimeOffsetOptions.interp.offset == 24
    assert C.sizeof(_capi.TimeOffsetResult) == 2 * 8 + 2 * 4 + 8
    # the other modes' structs keep their layout
    assert C.sizeof(_capi.AssembleOptions) == 5 * 8 + C.sizeof(_capi.Options) and C.sizeof(_capi.AssembleInfo) == 7 * 8
    assert C.sizeof(_capi.StationOptions) == 8 + 8 + 4 + 4 + 16 + C.sizeof(_capi.Options)


def test_new_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clc.h")).read(), flags=re.S)
    L = _capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _capi.EXPORTED and hasattr(L, name)
    assert _capi.EXPORTED[-len(NEW):] == list(NEW)  # appended, nothing moved
    assert "clc_debug_sweep_records" in _capi.HOOKS and "clc_debug_sweep_records" not in _capi.EXPORTED
    assert L.clc_version() == 210
    from camlasercalibratool_amd import Solver
    for m in ("interpolate_poses", "assemble_interpolated", "assemble_interpolated_device", "time_offset_sweep", "time_offset_sweep_device"):
        assert callable(getattr(Solver, m))
    import camlasercalibratool_amd as clc
    assert callable(clc.CalibrateOfflineInterpolated)


def test_option_defaults():
    o = _capi.default_interp_options()  # host code: needs no GPU
    assert (o.time_offset, o.max_gap, o.line0[0], o.line0[1]) == (0.0, 0.1, 0.0, 0.0)
    assert o.line.max_num_iterations == 10 and o.line.loss_scale_factor == 0.05
    s = _capi.default_time_offset_options()
    assert (s.offset_min, s.offset_max, s.n_offsets, s.points_per_scan) == (-0.02, 0.02, 41, 16)
    assert (s.interp.time_offset, s.interp.max_gap) == (0.0, 0.1)
    d = _capi.default_options()
    assert bytes(s.solve) == bytes(d)


def test_restatement_matches_scipy_slerp():
    worst_q, worst_t = IR.self_check(seed=0, n=800)
    print(f"interp_ref vs scipy Slerp: |dq| <= {worst_q:.2e}, |dt| <= {worst_t:.2e}")
    assert worst_q <= 1e-12 and worst_t <= 4 * 2.0 ** -53 * 2.0


def test_restated_bracket_rule():
    st = [0.0, 1.0, 1.0, 2.0, 5.0, 5.5]
    f = lambda x, g=2.0: IR.find_bracket(st, x, g)
    assert [f(-0.1), f(0.0), f(0.5), f(1.0), f(1.5), f(2.0), f(3.0), f(5.0), f(5.5), f(5.6), f(math.nan)] == [-1, 0, 0, 0, 2, 2, -1, 4, 4, -1, -1]
    assert f(3.0, 3.0) == 3 and f(2.0, 0.5) == -1 and f(5.25, 0.5) == 4
    assert IR.find_bracket([0.0, math.nan, 1.0, 2.0], 0.5, 2.0) == -1 and IR.find_bracket([0.0, math.nan, 1.0, 2.0], 1.5, 2.0) == 2
    assert IR.find_bracket([3.0, 4.0, 0.0, 1.0], 0.5, 2.0) == 2  # unsorted: the first in file order
    assert IR.find_bracket([0.0, 2.0, 1.0, 3.0], 1.5, 2.0) == 0 and IR.n_pairs([0.0, 2.0, 1.0, 3.0], 2.0) == 2
    assert IR.decimate(5, 16) == [0, 1, 2, 3, 4] and IR.decimate(5, 0) == [0, 1, 2, 3, 4] and IR.decimate(40, 1) == [20]
    assert IR.decimate(40, 2) == [10, 30] and IR.decimate(17, 16)[:3] == [0, 1, 2] and len(set(IR.decimate(17, 16))) == 16
    assert max(IR.decimate(17, 16)) <= 16


OFFSETS9 = [-0.02 + 0.005 * j for j in range(9)]


@pytest.mark.parametrize("seed", [1, 2])
def test_moving_recording_margins(seed):
    rec = so.moving_recording(seed, n_stations=6, move_frames=10, still_frames=4, clock_offset=0.007, offsets=OFFSETS9 + [0.007])
    assert rec["stamp_margin"] >= so.MARGIN and rec["gap_margin"] >= so.MARGIN
    m = so.check_motion_margins(rec, OFFSETS9)
    assert m["stamp_margin"] >= rec["stamp_margin"]
    n = len(rec["pose_stamp"])
    assert n == 6 * 4 + 5 * 10 and np.allclose(np.diff(rec["pose_stamp"]), 1 / 30.0) and np.allclose(np.diff(rec["scan_stamp"]), 1 / 40.0)
    assert rec["has_board"].sum() >= 0.7 * len(rec["scan_stamp"]) and np.abs(np.linalg.norm(rec["q_wc"], axis=1) - 1).max() < 1e-15
    # every stamp + offset the tests use lies inside the camera's stamps
    assert rec["scan_stamp"].min() - 0.02 > rec["pose_stamp"][0] and rec["scan_stamp"].max() + 0.02 < rec["pose_stamp"][-1]
    with pytest.raises(AssertionError):
        so.check_motion_margins(rec, [float(rec["pose_stamp"][5] - rec["scan_stamp"][3])])  # a stamp ON a pose stamp
    # the existing generators draw what they drew
    import hashlib
    r = so.recording(1)
    h = hashlib.sha256(b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("pose_stamp", "q_wc", "t_wc", "scan_stamp", "scan_frame", "has_board")) +
                       r["scans"]["ranges"].tobytes()).hexdigest()
    assert h == "e02a22bcd953be067a31155e6cc0f0f21f5201045aabe5d22b9c7f383d3caaa0"


def test_best_offset_rule_on_hand_made_tables():
    x = np.array([-0.02, -0.01, 0.0, 0.01, 0.02])
    par = lambda v, h=0.1: 3.0 * (x - v) ** 2 + h
    bi, bo, ae = _capi.time_offset_best(x, par(0.003))          # interior: the vertex of an exact parabola
    assert (bi, ae) == (2, 0) and abs(bo - 0.003) <= 1e-12
    bi, bo, ae = _capi.time_offset_best(x, par(-0.0149))
    assert (bi, ae) == (1, 0) and abs(bo + 0.0149) <= 1e-12
    assert _capi.time_offset_best(x, par(-0.03)) == (0, -0.02, 1)   # the edges
    assert _capi.time_offset_best(x, par(0.05)) == (4, 0.02, 1)
    assert _capi.time_offset_best(x, [5.0, 1.0, 3.0, 1.0, 5.0])[0] == 1  # ties: the first of equal minima
    assert _capi.time_offset_best(x, [1.0, 1.0, 1.0, 1.0, 1.0]) == (0, -0.02, 1)
    assert _capi.time_offset_best(x, [2.0, 1.0, 1.0, 1.0, 2.0]) == (1, -0.01, 0)  # no minimum of its own: the candidate itself
    F, okc = 6, 1
    c = par(0.003)
    bi, bo, ae = _capi.time_offset_best(x, c, [okc, okc, F, okc, okc])  # the smallest cost failed: the next one, its neighbour failed
    assert (bi, bo, ae) == (3, 0.01, 0)
    bi, bo, ae = _capi.time_offset_best(x, c, [F, okc, okc, okc, okc])
    assert (bi, ae) == (2, 0) and abs(bo - 0.003) <= 1e-12
    bi, bo, ae = _capi.time_offset_best(x, c, [F] * 5)
    assert bi == -1 and math.isnan(bo) and ae == 0
    bi, bo, ae = _capi.time_offset_best(x, [math.nan, 2.0, math.nan, 1.0, 3.0])  # a NaN is never chosen, and no parabola through one
    assert (bi, bo, ae) == (3, 0.01, 0)
    assert _capi.time_offset_best([], [])[0] == -1
    # unequal spacing: still the exact vertex
    xs = np.array([-0.02, -0.004, 0.0, 0.013, 0.02])
    bi, bo, ae = _capi.time_offset_best(xs, 2.0 * (xs - 0.002) ** 2 + 1.0)
    assert bi == 2 and abs(bo - 0.002) <= 1e-12
    # the restatement the GPU tests compare with says the same
    for tab, tm in ((par(0.003), None), (par(-0.03), None), ([5.0, 1.0, 3.0, 1.0, 5.0], None), (c, [okc, okc, F, okc, okc]), ([2.0, 1.0, 1.0, 1.0, 2.0], None)):
        a, b = _capi.time_offset_best(x, tab, tm), IR.best(x, tab, tm)
        assert a[0] == b[0] and a[2] == b[2] and abs(a[1] - b[1]) <= 1e-12
    L = _capi.lib()
    assert L.clc_clock_offset_best(3, None, None, None, None, None, None) == -1
