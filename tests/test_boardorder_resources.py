"""Build-time guard of the kernels of the chessboard ordering on the device (K26, csrc/clc_boardorder.hpp), without a GPU: hipcc's
kernel-resource-usage remarks for gfx950 over abi_chess.hip only, product and hooks builds.  Both kernels use no scratch memory and spill
nothing; the figures are printed (DESIGN.md K26 records them).  The header is wired into the build where the identity of the measured
kernels (csrc_sha16) does not see it, and its kernels live in abi_chess.hip under names the K25 guard does not count."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")


def test_build_wiring():
    from camlasercalibratool_amd import _build
    assert "clc_boardorder.hpp" in _build.SIDE_HEADERS and "clc_boardorder.hpp" in _build.SOURCES
    assert "clc_boardorder.hpp" not in _build.HEADERS and "clc_boardorder.hpp" not in _build.HOST_HEADERS
    for unit in _build.UNITS:  # abi_chess.hip alone includes the kernels' header
        assert ("clc_boardorder" in open(os.path.join(CSRC, unit)).read()) == (unit == "abi_chess.hip"), unit
    text = open(os.path.join(CSRC, "clc_boardorder.hpp")).read()
    assert "namespace boardorder" in text and "asm" not in re.sub(r"//.*", "", text)
    for name in re.findall(r"__global__[^(]*\bvoid (\w+)\(", text):
        assert "chess_" not in name and "board_" in name, name


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
    return {k: v for k, v in res.items() if "board_" in k}


def test_kernels_use_no_scratch_and_spill_nothing(usage):
    """As built (product and hooks builds alike): board_order_kernel 64 VGPRs, 95 SGPRs, no static LDS (its LDS is dynamic:
    56 cols rows + 2 784 bytes); board_gather_kernel 15 VGPRs, 43 SGPRs, no LDS; no AGPR, no scratch, no spill: 8 waves per SIMD by
    registers."""
    assert len(usage) == 2 and all(sum(k in name for name in usage) == 1 for k in ("board_order_kernel", "board_gather_kernel")), sorted(usage)
    for name, r in usage.items():
        print(name, r)
        assert "chess_" not in name
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (name, r)
        assert r["LDS Size"] == 0, (name, r)  # (static; the ordering's is dynamic)
