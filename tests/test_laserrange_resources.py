"""Build-time guard of the kernels of K21 (csrc/clc_laserrange.hpp on clc_jointterms.hpp and clc_arrow.hpp), without a GPU: the build wiring, and hipcc's
kernel-resource-usage remarks for gfx950 over abi_laserrange.hip only.  range_refine_kernel — the evaluation waves with the 48-wide
and 44-wide passes, the per-lane Schur step and the controller in one kernel — uses no scratch memory, spills no VGPR and stays within
the figures it was built with; the point correction and the kernel that reads the ranges of a device-array call stay small."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")


def test_build_wiring():
    from camlasercalibratool_amd import _build
    assert "abi_laserrange.hip" in _build.UNITS
    assert "clc_laserrange.hpp" in _build.SIDE_HEADERS and "clc_laserrange.hpp" not in _build.HEADERS
    src = open(os.path.join(CSRC, "clc_laserrange.hpp")).read()
    assert re.findall(r'#include\s+["<]([^">]+)[">]', src) == ["clc_jointterms.hpp"]  # the leaf of the joint problems (over clc_arrow.hpp)
    others = [u for u in _build.UNITS + _build.HEADERS + _build.HOST_HEADERS + _build.SIDE_HEADERS if u not in ("abi_laserrange.hip", "clc_laserrange.hpp")]
    for u in others:  # the unit alone includes the header
        assert "clc_laserrange.hpp" not in re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, u)).read()), u


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    from camlasercalibratool_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("res")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + ["-c", os.path.join(CSRC, "abi_laserrange.hip"), "-o", str(tmp / "abi_laserrange.o"),
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


# range_refine_kernel as built (256 threads, one wave per SIMD: the 512-register file of a lane is its own; the 48 sums of J_i J_c^T
# are the widest pass); the SGPRs that do not fit are parked in VGPR lanes, as in joint_refine_kernel
RANGE_KERNEL = {"VGPRs": 256, "AGPRs": 80, "SGPRs Spill": 28, "LDS Size": 4032}


def test_range_kernel_no_scratch_within_its_figures(usage):
    r = one(usage, "range_refine_kernel")
    print("bounds:", RANGE_KERNEL)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
    assert all(r[k] <= v for k, v in RANGE_KERNEL.items()), (r, RANGE_KERNEL)


def test_correct_kernel_is_small(usage):
    r = one(usage, "range_correct_kernel")
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, r
    assert r["VGPRs"] + r["AGPRs"] <= 32, r


def test_ends_kernel_is_small(usage):
    r = one(usage, "joint_ends_kernelILi0E")  # clc_jointterms.hpp's (a template), the one under K18, K21 and K22
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, r
    assert r["VGPRs"] + r["AGPRs"] <= 16, r
