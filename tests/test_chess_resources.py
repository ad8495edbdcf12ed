"""Build-time guard of the kernels of the chessboard-corner detection (K25, csrc/clc_chess.hpp), without a GPU: hipcc's
kernel-resource-usage remarks for gfx950 over abi_chess.hip only, product and hooks builds.  Both kernels use no scratch memory and spill
nothing; the figures, the LDS bytes among them, are printed (DESIGN.md K25 records them).  The unit and its header are wired into the build
where the identity of the measured kernels (csrc_sha16) does not see them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")


def test_build_wiring():
    from camlasercalibratool_amd import _build
    assert "abi_chess.hip" in _build.UNITS
    assert "clc_chess.hpp" in _build.SIDE_HEADERS and "clc_chess.hpp" not in _build.HEADERS
    assert "clc_chessorder.hpp" in _build.SOURCES and "clc_chessorder.hpp" not in _build.HEADERS
    for unit in _build.UNITS:  # no other unit includes the kernels' header
        if unit != "abi_chess.hip":
            assert "clc_chess" not in open(os.path.join(CSRC, unit)).read(), unit


@pytest.fixture(scope="module", params=[(), ("-DCLC_TEST_HOOKS",)], ids=["product", "hooks"])
def usage(request, tmp_path_factory):
    from camlasercalibratool_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("res")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + list(request.param) + ["-c", os.path.join(CSRC, "abi_chess.hip"), "-o",
                        str(tmp / "abi_chess.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    res, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            res[cur][m.group(1).strip()] = int(m.group(2))
    return {k: v for k, v in res.items() if "chess_" in k}


def test_kernels_use_no_scratch_and_spill_nothing(usage):
    """As built (product and hooks builds alike): chess_response_nms_kernel 46 VGPRs, 54 SGPRs, 8 200 bytes of LDS (the 40 x 88 byte
    image, the 30 x 78 int16 responses); chess_select_kernel 25 VGPRs, 58 SGPRs, no LDS; no AGPR, no scratch, no spill: 8 waves per
    SIMD by registers."""
    assert len(usage) == 2 and all(sum(k in name for name in usage) == 1 for k in ("chess_response_nms_kernel", "chess_select_kernel")), sorted(usage)
    for name, r in usage.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (name, r)
        assert r["LDS Size"] <= 40 * 88 + 30 * 78 * 2 + 64, (name, r)
