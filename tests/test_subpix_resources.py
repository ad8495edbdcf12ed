"""Build-time guard of the kernel of the sub-pixel corner refinement (K24, csrc/clc_subpix.hpp), without a GPU: hipcc's
kernel-resource-usage remarks for gfx950 over abi_subpix.hip only, product and hooks builds.  The kernel uses no scratch memory, spills no
VGPR and stays within 128 VGPRs + AGPRs; the figures, the LDS bytes among them, are printed.  The unit and its header are wired into the
build where the identity of the measured kernels (csrc_sha16) does not see them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")


def test_build_wiring():
    from camlasercalibratool_amd import _build
    assert "abi_subpix.hip" in _build.UNITS
    assert "clc_subpix.hpp" in _build.SIDE_HEADERS and "clc_subpix.hpp" not in _build.HEADERS
    for unit in ("abi_frontend.hip", "abi_campose.hip"):  # their resource tests count kernels
        assert "clc_subpix.hpp" not in open(os.path.join(CSRC, unit)).read(), unit


@pytest.fixture(scope="module", params=[(), ("-DCLC_TEST_HOOKS",)], ids=["product", "hooks"])
def usage(request, tmp_path_factory):
    from camlasercalibratool_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("res")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + list(request.param) + ["-c", os.path.join(CSRC, "abi_subpix.hip"), "-o",
                        str(tmp / "abi_subpix.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
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
    return {k: v for k, v in res.items() if "corner_subpix_kernel" in k}


def test_kernel_uses_no_scratch_spills_nothing_and_fits_128_registers(usage):
    """As built (product and hooks builds alike): 58 VGPRs, 0 AGPRs, 75 SGPRs, no scratch, no spill, 4 872 bytes of LDS (the 34 x 34
    neighbourhood and the two mask tables): 8 waves per SIMD by registers, and 32 one-wave workgroups per CU by LDS."""
    assert len(usage) == 1, sorted(usage)
    for name, r in usage.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (name, r)
        assert r["LDS Size"] <= 34 * 34 * 4 + 2 * 31 * 4, (name, r)
