"""Build-time guard of the kernels of the tag-grid corners (K27, csrc/clc_tags.hpp), without a GPU: hipcc's kernel-resource-usage remarks
for gfx950 over abi_tags.hip only, product and hooks builds.  The four kernels use no scratch memory and spill nothing; the figures, the
LDS bytes among them, are printed (DESIGN.md K27 records them).  The unit and its header are wired into the build where the identity of
the measured kernels (csrc_sha16) does not see them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")
KERNELS = ("tag_edges_kernel", "tag_decode_kernel", "tag_scan_kernel", "tag_points_kernel")


def test_build_wiring():
    from camlasercalibratool_amd import _build
    assert "abi_tags.hip" in _build.UNITS and len(_build.UNITS) == 18
    assert "clc_tags.hpp" in _build.SIDE_HEADERS and "clc_tags.hpp" in _build.SOURCES
    assert "clc_tags.hpp" not in _build.HEADERS and "clc_tags.hpp" not in _build.HOST_HEADERS
    for unit in _build.UNITS:  # abi_tags.hip alone includes the kernels' header
        assert ("clc_tags" in open(os.path.join(CSRC, unit)).read()) == (unit == "abi_tags.hip"), unit
    text = open(os.path.join(CSRC, "clc_tags.hpp")).read()
    assert "namespace tags" in text and "asm" not in re.sub(r"//.*", "", text) and "atomic" not in re.sub(r"//.*", "", text)
    assert sorted(re.findall(r"__global__.*\bvoid (\w+)\(", text)) == sorted(KERNELS)


@pytest.fixture(scope="module", params=[(), ("-DCLC_TEST_HOOKS",)], ids=["product", "hooks"])
def usage(request, tmp_path_factory):
    from camlasercalibratool_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("res")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + list(request.param) + ["-c", os.path.join(CSRC, "abi_tags.hip"), "-o",
                        str(tmp / "abi_tags.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
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
    return {k: v for k, v in res.items() if "tag_" in k}


def test_kernels_use_no_scratch_and_spill_nothing(usage):
    """As built (product and hooks builds alike): tag_edges_kernel 58 VGPRs, 76 SGPRs, 9 216 bytes of LDS (the candidates as two int32
    arrays, the 256 partial counts); tag_decode_kernel 62 VGPRs, 100 SGPRs, 24 784 bytes of LDS (K26's system, the candidates, the quad
    list, the per-id keys); tag_scan_kernel 44 VGPRs, 25 SGPRs, 2 056 bytes; tag_points_kernel 114 VGPRs, 46 SGPRs, 256 bytes; no
    AGPR, no scratch, no spill."""
    assert len(usage) == 4 and all(sum(k in name for name in usage) == 1 for k in KERNELS), sorted(usage)
    limits = {"tag_edges_kernel": 2 * 4 * 1024 + 4 * 256, "tag_decode_kernel": 32 * 1024, "tag_scan_kernel": 8 * 256 + 8, "tag_points_kernel": 4 * 64}
    for name, r in usage.items():
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (name, r)
        assert r["LDS Size"] <= [v for k, v in limits.items() if k in name][0], (name, r)
