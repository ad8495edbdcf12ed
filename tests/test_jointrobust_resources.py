"""Build-time guard of the kernels of K22 (csrc/clc_jointrobust.hpp on clc_jointterms.hpp and clc_arrow.hpp), without a GPU: the build wiring, and hipcc's
kernel-resource-usage remarks for gfx950 over abi_jointrobust.hip only.  joint_robust_kernel — the evaluation waves with the
per-corner row and its weight, the three weighted laser passes, the per-lane Schur step and the controller in one kernel — uses no
scratch memory, spills no VGPR and stays within the figures it was built with; the weights kernel and the kernel that reads the
ranges of a device-array call stay small.  K18's own figures (tests/test_joint_resources.py) are untouched: its unit does not
include this header."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")


def test_build_wiring():
    from camlasercalibratool_amd import _build
    assert "abi_jointrobust.hip" in _build.UNITS
    assert "clc_jointrobust.hpp" in _build.SIDE_HEADERS and "clc_jointrobust.hpp" not in _build.HEADERS
    src = open(os.path.join(CSRC, "clc_jointrobust.hpp")).read()
    assert re.findall(r'#include\s+["<]([^">]+)[">]', src) == ["clc_jointterms.hpp"]  # the leaf of the joint problems (over clc_arrow.hpp)
    others = [u for u in _build.UNITS + _build.HEADERS + _build.HOST_HEADERS + _build.SIDE_HEADERS if u not in ("abi_jointrobust.hip", "clc_jointrobust.hpp")]
    for u in others:  # the unit alone includes the header
        assert "clc_jointrobust.hpp" not in re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, u)).read()), u


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    from camlasercalibratool_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("res")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + ["-c", os.path.join(CSRC, "abi_jointrobust.hip"), "-o", str(tmp / "abi_jointrobust.o"),
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


# joint_robust_kernel as built (256 threads, one wave per SIMD: the 512-register file of a lane is its own; K18's kernel has 256 + 32,
# the corner pass here keeps a 28-entry row beside the 28 accumulators); the SGPRs that do not fit are parked in VGPR lanes, as in
# joint_refine_kernel; the LDS is K18's JointShared
ROBUST_KERNEL = {"VGPRs": 256, "AGPRs": 50, "SGPRs Spill": 42, "LDS Size": 2192}


def test_robust_kernel_no_scratch_within_its_figures(usage):
    r = one(usage, "joint_robust_kernel")
    print("bounds:", ROBUST_KERNEL)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
    assert all(r[k] <= v for k, v in ROBUST_KERNEL.items()), (r, ROBUST_KERNEL)


def test_weights_kernel_is_small(usage):
    """One corner row (28) and two rotations per lane: 108 VGPRs as built, four waves per SIMD."""
    r = one(usage, "joint_weights_kernel")
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, r
    assert r["VGPRs"] + r["AGPRs"] <= 128, r


def test_ends_kernel_is_small(usage):
    r = one(usage, "joint_ends_kernelILi0E")  # clc_jointterms.hpp's (a template), the one under K18, K21 and K22
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, r
    assert r["VGPRs"] + r["AGPRs"] <= 16, r


def test_other_units_do_not_name_the_new_kernels():
    """K18's header and unit and the headers under them know nothing of K22: what the two share they take from clc_jointterms.hpp and
    abi_jointcall.hpp (which may name every unit), never from one another."""
    for u in ("clc_arrow.hpp", "clc_joint.hpp", "abi_joint.hip", "clc_campose.hpp", "clc_math.hpp"):
        assert "jointrobust" not in open(os.path.join(CSRC, u)).read() and "joint_robust" not in open(os.path.join(CSRC, u)).read(), u
