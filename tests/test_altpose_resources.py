"""Build-time guard of the kernels of the planar fit's second minimum (K17, csrc/clc_altpose.hpp), without a GPU: hipcc's
kernel-resource-usage remarks for gfx950 over abi_campose.hip.  alt_start_kernel uses no scratch memory, at most 64 VGPRs and leaves
room for eight waves per SIMD; board_pose_from_start_kernel — cost_in and K10's LM stage with the controller inlined, which is what
fills board_pose_kernel's budget too — uses no scratch and stays within the figures it was built with.  (board_pose_kernel and
board_pose_subset_kernel, which share the translation unit, are held to their figures by tests/test_robustpose_resources.py.)"""
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
    tmp = tmp_path_factory.mktemp("res")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + ["-c", os.path.join(CSRC, "abi_campose.hip"), "-o", str(tmp / "abi_campose.o"),
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


def test_start_kernel_no_scratch_64_vgprs_eight_waves(usage):
    r = one(usage, "alt_start_kernel")
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["VGPRs"] + r["AGPRs"] <= 64 and r["Occupancy"] >= 8, r


# board_pose_from_start_kernel as built: the SGPRs that do not fit are parked in VGPR lanes, as in board_pose_kernel (26 there)
FIT_KERNEL = {"VGPRs": 256, "AGPRs": 46, "SGPRs Spill": 48, "LDS Size": 2584}


def test_fit_kernel_no_scratch_within_its_figures(usage):
    r = one(usage, "board_pose_from_start_kernel")
    print("bounds:", FIT_KERNEL)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
    assert all(r[k] <= v for k, v in FIT_KERNEL.items()), (r, FIT_KERNEL)
