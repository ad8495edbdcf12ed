"""Board-segment detection (AutoGetLinePts, src/selectScanPoints.cpp:17-190) without a GPU: the C-ABI declares and exports
clc_board_segments[_device], the test restatement (tests/board_segment_ref.py) equals the reference's own outputs frozen
in tests/golden/segment_vectors.npz, the scan generator behind that fixture has not drifted, and the K7 kernel builds for
gfx950 without scratch."""
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import board_segment_ref as R
from camlasercalibratool_amd import _build, _capi, simdata as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "segment_vectors.npz")
NEW = ("clc_board_segments", "clc_board_segments_device")


def test_header_declares_and_product_library_exports_board_segments():
    hdr = open(os.path.join(ROOT, "include", "clc.h")).read()
    for name in NEW:
        assert re.search(rf"\bint {name}\(", hdr), name
        assert name in _capi.EXPORTED
    for macro, v in (("CLC_SEG_FOUND", "1"), ("CLC_SEG_NONE", "0"), ("CLC_SEG_REF_THROWS", "(-1)")):
        assert re.search(rf"#define {macro} {re.escape(v)}(?!\S)", hdr), macro
    out = subprocess.run(["nm", "-D", "--defined-only", _build.PRODUCT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if len(l.split()) >= 3 and l.split()[-2] == "T"}
    assert set(NEW) <= syms


def test_restatement_equals_reference_on_hand_made_cases():
    G = np.load(GOLDEN)
    seg, st = R.board_segments(G["hand_points"], G["hand_offsets"])
    for k, name in enumerate(G["hand_names"]):
        assert (tuple(seg[k]), st[k]) == (tuple(G["hand_seg"][k]), G["hand_status"][k]), name
    # every status occurs, and the quirks the cases are named after hold
    assert set(G["hand_status"].tolist()) == {-1, 0, 1}
    res = dict(zip(G["hand_names"].tolist(), zip(G["hand_status"].tolist(), G["hand_seg"].tolist())))
    assert res["n0"][0] == -1 and res["left_bound_n537"][0] == -1 and res["left_bound_n538"][0] == 1
    assert res["d_eq_100_current"][0] == 0 and res["nan_current"][0] == 0 and res["d_above_100_current"][0] == 1
    assert res["length_48"][0] == 0 and res["length_51"][0] == 1
    assert res["dist_exactly_0p2"][0] == 0 and res["dist_above_0p2"][0] == 1
    assert res["end_norm_exactly_2"][0] == 0 and res["end_norm_below_2"][0] == 1
    assert res["open_final_segment"][0] == 0 and res["throws_not_best"][0] == -1
    assert res["nonmonotone_widening"][1][0] == 271 and res["equal_length_tie"][1] == [360, 429]


def test_restatement_equals_reference_on_simulated_scans():
    G = np.load(GOLDEN)
    S = int(G["sim_n_scans"])
    for i, seed in enumerate(G["sim_seeds"]):
        P = sd.scan_points_host(sd.sim_laser_scans(int(seed), S))
        assert hashlib.sha256(P.tobytes()).hexdigest() == G["sim_sha256"][i], "simdata.sim_laser_scans drifted from the fixture"
        seg, st = R.board_segments(P, np.arange(S + 1, dtype=np.int64) * 1081)
        assert np.array_equal(seg, G["sim_seg"][i]) and np.array_equal(st, G["sim_status"][i])
        assert 0.4 < (st == 1).mean() < 0.95  # the generator yields both outcomes


def test_board_segment_kernel_has_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + ["--cuda-device-only", "-c", os.path.join(csrc, "abi_frontend.hip"), "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = re.split(r"Function Name: ", p.stderr)
    blk = [b for b in blocks if b.startswith("_ZN3clc20board_segment_kernel")]
    assert len(blk) == 1
    vals = {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", blk[0])}
    assert vals["ScratchSize"] == 0 and vals["VGPRs Spill"] == 0 and vals["SGPRs Spill"] == 0, vals
    assert vals["LDS Size"] <= 8192, vals
