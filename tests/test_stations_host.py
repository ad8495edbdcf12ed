"""Static stations (K14) without a GPU: the C-ABI's new structs and symbols, the restatement tests/stations_ref.py against the frozen
output of the reference's own GetStaticPose (tests/golden/static_poses_ref.json, made by tests/golden/make_static_poses_golden.py),
the two forms of the walk against each other, and the margins of simoffline.station_recording for the seeds the GPU tests use."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import stations_ref as SR
from camlasercalibratool_amd import _capi, simoffline as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "static_poses_ref.json")) as f:
        G = json.load(f)
    return {"pose_stamp": np.array(G["pose_stamp"]), "q_wc": np.array(G["q_wc"]), "t_wc": np.array(G["t_wc"]),
            "ref": {k: np.array(v) for k, v in G["ref"].items()}}


def _struct_fields(name):
    hdr = open(os.path.join(ROOT, "include", "clc.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [m.group(2) for m in re.finditer(r"(double|int32_t|int64_t|clc_options)\s+(\w+)(?:\[\d+\])?;", body)]


def test_struct_layouts_match_header():
    assert _struct_fields("clc_station_options") == [f[0] for f in _capi.StationOptions._fields_]
    assert _struct_fields("clc_station_info") == [f[0] for f in _capi.StationInfo._fields_]
    assert C.sizeof(_capi.StationOptions) == 8 + 8 + 4 + 4 + 16 + C.sizeof(_capi.Options)
    assert C.sizeof(_capi.StationInfo) == 9 * 8
    assert _capi.StationOptions.line0.offset == 24 and _capi.StationOptions.line.offset == 40
    # the key-frame mode's structs keep their layout
    assert C.sizeof(_capi.AssembleOptions) == 5 * 8 + C.sizeof(_capi.Options) and C.sizeof(_capi.AssembleInfo) == 7 * 8


def test_new_symbols_are_exported():
    for name in ("clc_station_options_default", "clc_static_poses", "clc_assemble_stations", "clc_assemble_stations_device"):
        assert name in _capi.EXPORTED
    assert "clc_debug_station_walk" in _capi.HOOKS and "clc_debug_station_walk" not in _capi.EXPORTED
    o = _capi.default_station_options()  # host code: needs no GPU
    assert (o.center_dist_max, o.min_members, o.close_last_run, o.reserved, o.line0[0], o.line0[1]) == (0.002, 30, 0, 0, 0.0, 0.0)
    assert o.line.max_num_iterations == 10 and o.line.loss_scale_factor == 0.05
    assert _capi.lib().clc_version() == 210


def test_restatement_matches_the_references_function(golden):
    ref = golden["ref"]
    w = SR.walk(golden["t_wc"])
    assert w["margin"] >= 1e-6
    assert w["members"].tolist() == ref["members"].tolist() == [31, 32, 34, 38]  # runs of 30, 31, 33 and 37 distinct poses
    assert np.array_equal(w["first"], ref["first"]) and np.array_equal(w["last"], ref["last"])
    a = SR.average(golden["pose_stamp"], golden["q_wc"], golden["t_wc"], w)
    assert np.array_equal(a["start_time"], ref["start_time"]) and np.array_equal(a["end_time"], ref["end_time"])
    assert np.array_equal(a["start_time"], golden["pose_stamp"][ref["first"]]) and np.array_equal(a["end_time"], golden["pose_stamp"][ref["last"]])
    assert np.array_equal(a["t"], ref["t"])  # the same sums in the same order
    for k in range(len(ref["q"])):
        d = min(np.abs(a["q"][k] - ref["q"][k]).max(), np.abs(a["q"][k] + ref["q"][k]).max())
        assert d <= 1e-12, (k, d)
        assert a["q"][k][0] > 0 and a["gap"][k] >= 0.5
    assert (a["status"] == SR.STATION_OK).all()


def test_fixture_holds_the_odd_cases(golden):
    t, q = golden["t_wc"], golden["q_wc"]
    runs = SR.walk(t, min_members=0)  # every closed run
    m = runs["members"].tolist()
    assert 30 in m and 31 in m and 32 in m                # 29, 30 and 31 distinct poses
    assert 1 in m                                         # a NaN at a run's start: a run of one member
    assert np.isnan(t).any(axis=1).sum() == 2
    assert SR.walk(t)["n_runs"] == runs["n_runs"] == len(m)
    assert len(SR.walk(t, close_last_run=True)["first"]) == len(SR.walk(t)["first"]) + 1   # the open run at the end
    two = [i for i in range(len(m) - 1) if m[i] > 30 and m[i + 1] == 2]                    # two breakers in a row behind a station
    assert two
    k = 1  # the station with mixed signs
    idx = SR.member_list(SR.walk(t)["first"][k], SR.walk(t)["members"][k])
    assert (q[idx, 0] > 0).any() and (q[idx, 0] < 0).any()


def test_uniform_walk_equals_literal_walk(golden):
    for t in (golden["t_wc"], so.station_recording(1)["t_wc"]):
        for dist_max, min_members in ((0.002, 30), (0.002, 0), (0.0005, 3), (0.0, 0)):
            lit = SR.walk_literal(t, dist_max, min_members)
            w = SR.walk(t, dist_max, min_members)
            assert len(lit) == len(w["first"])
            for k, members in enumerate(lit):
                assert members == SR.member_list(w["first"][k], w["members"][k])
                assert members[-1] == w["last"][k]


def fixed_centre_walk(t, dist_max=SR.DIST_MAX, min_members=SR.MIN_MEMBERS):
    """NOT the reference: every candidate is tested against the run's FIRST pose instead of the running centre."""
    first, members, a, n = [], [], 0, len(t)
    while a < n:
        j = a
        while j < n and np.sqrt(((t[j] - t[a]) ** 2).sum()) < dist_max:
            j += 1
        if j >= n:
            break
        if 1 + j - a > min_members:
            first.append(a); members.append(1 + j - a)
        a = j + 1
    return first, members


def drift(n=400, step=0.000053):
    """A constant drift of 0.053 mm per pose along x: the running centre follows at half the speed."""
    t = np.zeros((n, 3))
    t[:, 0] = step * np.arange(n)
    return t


def test_constant_drift_tells_running_centre_from_fixed_centre():
    t = drift()
    w = SR.walk(t)
    f, m = fixed_centre_walk(t)
    assert w["margin"] >= 1e-6
    assert len(w["first"]) >= 2 and (w["first"].tolist(), w["members"].tolist()) != (f, m)
    assert w["members"][0] > m[0]  # the centre follows the drift: the run is about twice as long


@pytest.mark.parametrize("seed", [1, 2])
def test_station_recording_margins(seed):
    rec = so.station_recording(seed)
    assert rec["station_margin"] >= so.MARGIN and rec["stamp_margin"] >= so.MARGIN
    w = SR.walk(rec["t_wc"])
    assert np.array_equal(w["first"], rec["station_first"]) and np.array_equal(w["last"], rec["station_last"])
    assert np.array_equal(w["members"], rec["station_members"]) and len(w["first"]) >= 10 and w["margin"] == rec["station_margin"]
    # the scans are those of recording() with the same arguments: the jitter has a stream of its own
    base = so.recording(seed, n_stations=12, still_frames=40)
    assert rec["scans"]["ranges"].tobytes() == base["scans"]["ranges"].tobytes() and np.array_equal(rec["scan_stamp"], base["scan_stamp"])
    assert np.array_equal(rec["t_wc_true"], base["t_wc"]) and not np.array_equal(rec["t_wc"], base["t_wc"])
    assert np.abs(rec["t_wc"] - rec["t_wc_true"]).max() < 2e-3 and np.abs(np.linalg.norm(rec["q_wc"], axis=1) - 1).max() < 1e-15


def test_recording_is_what_it_was():
    """recording() draws what it drew before station_recording existed (sha256 of its arrays, seed 1)."""
    import hashlib
    r = so.recording(1)
    h = hashlib.sha256(b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("pose_stamp", "q_wc", "t_wc", "scan_stamp", "scan_frame", "has_board")) +
                       r["scans"]["ranges"].tobytes()).hexdigest()
    assert h == "e02a22bcd953be067a31155e6cc0f0f21f5201045aabe5d22b9c7f383d3caaa0"
