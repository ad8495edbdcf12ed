"""Build-time guard of the kernels of the intrinsic calibration (K19, csrc/clc_camcal.hpp, clc_arrow.hpp), without a GPU: hipcc's
kernel-resource-usage remarks for gfx950 over abi_camcal.hip only.  camcal_kernel — the evaluation waves, the per-lane Schur step and
the controller in one kernel — and homography_kernel use no scratch memory and spill no VGPR.  The register and LDS figures they are
built with are printed and recorded in DESIGN.md (K19), not fixed here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    from camlasercalibratool_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert "abi_camcal.hip" in _build.UNITS and "clc_camcal.hpp" in _build.SIDE_HEADERS
    tmp = tmp_path_factory.mktemp("res")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + ["-c", os.path.join(CSRC, "abi_camcal.hip"), "-o", str(tmp / "abi_camcal.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
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
    return res


def one(usage, kernel):
    found = {k: v for k, v in usage.items() if re.search(r"\d+%sE" % kernel, k)}
    assert len(found) == 1, (kernel, sorted(usage)[-12:])
    (name, r), = found.items()
    print(name, r)
    return r


@pytest.mark.parametrize("kernel", ["camcal_kernel", "homography_kernel"])
def test_kernels_use_no_scratch_and_spill_no_vgpr(usage, kernel):
    r = one(usage, kernel)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
    assert r["LDS Size"] <= 65536, r
