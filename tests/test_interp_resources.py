"""Build-time guard of the kernels of the interpolated flow (K15, csrc/clc_interp.hpp), without a GPU: hipcc's kernel-resource-usage
remarks for gfx950.  None of them uses scratch memory (the issue's requirement for sweep_records_kernel: FP64, no atomics, no
scratch), none holds dynamic LDS, and each leaves room for at least four waves per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")
KERNELS = ("interp_stamps_kernel", "interp_kernel", "sweep_member_kernel", "sweep_offsets_kernel", "sweep_records_kernel")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    from camlasercalibratool_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("res")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + ["-c", os.path.join(CSRC, "abi_frontend.hip"), "-o", str(tmp / "abi_frontend.o"),
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


@pytest.mark.parametrize("kernel", KERNELS)
def test_interp_kernels_use_no_scratch(usage, kernel):
    found = {k: v for k, v in usage.items() if re.search(r"\d+%sE" % kernel, k)}
    assert len(found) == 1, (kernel, sorted(usage)[:40])
    (name, r), = found.items()
    print(name, r)
    assert r["ScratchSize"] == 0, (name, r)
    assert r["Occupancy"] >= 4 and r["VGPRs"] <= 128, (name, r)


def test_the_kernels_beside_them_are_still_there(usage):
    """K13's and K14's kernels come out of the same translation unit."""
    for k in ("keyframe_kernel", "associate_kernel", "compact_kernel", "gather_kernel", "endpoints_kernel", "station_walk_kernel",
              "station_average_kernel", "station_associate_kernel"):
        assert any(re.search(r"\d+%sE" % k, name) for name in usage), k
