"""Build-time guard of the kernel of the joint refinement (K18, csrc/clc_joint.hpp, clc_arrow.hpp), without a GPU: hipcc's kernel-resource-usage
remarks for gfx950 over abi_joint.hip only.  joint_refine_kernel — the evaluation waves, the per-lane Schur step and the controller
in one kernel — uses no scratch memory, spills no VGPR and stays within the figures it was built with; the small kernel that reads
the ranges of a device-array call stays small."""
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
    assert "abi_joint.hip" in _build.UNITS and "clc_joint.hpp" in _build.SIDE_HEADERS
    tmp = tmp_path_factory.mktemp("res")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + ["-c", os.path.join(CSRC, "abi_joint.hip"), "-o", str(tmp / "abi_joint.o"),
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


# joint_refine_kernel as built (256 threads, one wave per SIMD: the 512-register file of a lane is its own); the SGPRs that do not fit
# are parked in VGPR lanes, as in board_pose_kernel
JOINT_KERNEL = {"VGPRs": 256, "AGPRs": 32, "SGPRs Spill": 12, "LDS Size": 2192}


def test_joint_kernel_no_scratch_within_its_figures(usage):
    r = one(usage, "joint_refine_kernel")
    print("bounds:", JOINT_KERNEL)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
    assert all(r[k] <= v for k, v in JOINT_KERNEL.items()), (r, JOINT_KERNEL)


def test_ends_kernel_is_small(usage):
    r = one(usage, "joint_ends_kernelILi0E")  # clc_jointterms.hpp's (a template), the one under K18, K21 and K22
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, r
    assert r["VGPRs"] + r["AGPRs"] <= 16, r
