"""Build-time guard of the kernels of the pose guidance (K20, csrc/clc_guidance.hpp), without a GPU: hipcc's kernel-resource-usage
remarks for gfx950 over abi_guidance.hip only.  No K20 kernel uses scratch memory or spills a VGPR; the figures are printed.  The
unit and its header are wired into the build where the identity of the measured kernels (csrc_sha16) does not see them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")
KERNELS = ["guidance_dirs_kernel", "guidance_cast_kernel", "guidance_score_kernel", "guidance_pick_kernel"]


def test_build_wiring():
    from camlasercalibratool_amd import _build
    assert "abi_guidance.hip" in _build.UNITS
    assert "clc_guidance.hpp" in _build.SIDE_HEADERS and "clc_guidance.hpp" not in _build.HEADERS


@pytest.fixture(scope="module", params=[(), ("-DCLC_TEST_HOOKS",)], ids=["product", "hooks"])
def usage(request, tmp_path_factory):
    from camlasercalibratool_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("res")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + list(request.param) + ["-c", os.path.join(CSRC, "abi_guidance.hip"), "-o",
                        str(tmp / "abi_guidance.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
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
    return {k: v for k, v in res.items() if "guidance_" in k}, bool(request.param)


def test_no_kernel_uses_scratch_or_spills_vgprs(usage):
    """As built: dirs 32 VGPRs; cast (table) 98 VGPRs, (a sincos per ray, hooks build only) 120; score 118 / 119 VGPRs, the selection
    round's form parks 8 SGPRs in VGPR lanes (M's 36 doubles are wave-uniform: 72 SGPRs), 64 B of LDS; pick 18 VGPRs, 72 B of LDS; the hooks build's row-per-lane score form 55 VGPRs."""
    res, hooks = usage
    for kernel in KERNELS:
        assert any(re.search(r"\d+%s[IE]" % kernel, k) for k in res), (kernel, sorted(res))
    for name, r in res.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (name, r)  # four waves per SIMD at the least
    # dirs, cast, score x 2, pick; the hooks build adds the two forms kept for their measurements (a sincos per ray, a row per lane)
    assert len(res) == (7 if hooks else 5), sorted(res)
