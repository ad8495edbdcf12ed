"""Build-time guard of the kernels of K23 (csrc/clc_fullcal.hpp on clc_jointterms.hpp, clc_arrow.hpp and clc_camcal.hpp), without a GPU: the build wiring,
and hipcc's kernel-resource-usage remarks for gfx950 over abi_fullcal.hip only.  fullcal_kernel — the evaluation waves with the four
weighted corner passes and the four weighted laser passes, the per-lane Schur step over a 6 x 16 coupling block and the controller
with its run-time-n Cholesky in one kernel — uses no scratch memory, spills no VGPR and stays within the figures it was built with;
the weights kernel stays within its own.  The call needs no kernel that reads ranges back: the workspace is sized from n_images.  The
figures of K19, K21 and K22 (their own resource tests) are untouched: their units do not include this header."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")


def test_build_wiring():
    from camlasercalibratool_amd import _build
    assert "abi_fullcal.hip" in _build.UNITS
    assert "clc_fullcal.hpp" in _build.SIDE_HEADERS and "clc_fullcal.hpp" not in _build.HEADERS
    src = open(os.path.join(CSRC, "clc_fullcal.hpp")).read()
    # the leaf of the joint problems (over clc_arrow.hpp) and K19's corner terms; neither K21's nor K22's header (their own units alone
    # include them)
    assert re.findall(r'#include\s+["<]([^">]+)[">]', src) == ["clc_jointterms.hpp", "clc_camcal.hpp"]
    others = [u for u in _build.UNITS + _build.HEADERS + _build.HOST_HEADERS + _build.SIDE_HEADERS if u not in ("abi_fullcal.hip", "clc_fullcal.hpp")]
    for u in others:  # the unit alone includes the header
        assert "clc_fullcal.hpp" not in re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, u)).read()), u
    unit = re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, "abi_fullcal.hip")).read())
    assert "clc_fullcal.hpp" in unit and "clc_laserrange.hpp" not in unit and "clc_jointrobust.hpp" not in unit
    # the kernels whose measured constants csrc_sha16 guards are built from the same bytes
    with open(os.path.join(ROOT, "profiles", "valu_counts.json")) as f:
        assert _build.csrc_sha16() == json.load(f)["csrc_sha16"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    from camlasercalibratool_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("res")
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + ["-c", os.path.join(CSRC, "abi_fullcal.hip"), "-o", str(tmp / "abi_fullcal.o"),
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


# fullcal_kernel as built (256 threads, one wave per SIMD: the 512-register file of a lane is its own; K19's kernel has 256 + 90, the
# corner passes here carry the weight beside K19's rows); the SGPRs that do not fit are parked in VGPR lanes, as in camcal_kernel; the
# LDS is FullShared: the controller, the totals of two records of 154, the 16 x 16 reduced system three times and its compact copy
FULL_KERNEL = {"VGPRs": 256, "AGPRs": 192, "SGPRs Spill": 122, "LDS Size": 13512}


def test_full_kernel_no_scratch_within_its_figures(usage):
    r = one(usage, "fullcal_kernel")
    print("bounds:", FULL_KERNEL)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
    assert all(r[k] <= v for k, v in FULL_KERNEL.items()), (r, FULL_KERNEL)


def test_weights_kernel_within_its_figures(usage):
    """One corner's rows (2 x 6 and 2 x 8) and two rotations per lane: 229 VGPRs and 24 parked SGPRs as built, two waves per SIMD, no
    LDS."""
    r = one(usage, "fullcal_weights_kernel")
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["LDS Size"] == 0, r
    assert r["VGPRs"] + r["AGPRs"] <= 232 and r["SGPRs Spill"] <= 24, r


def test_no_kernel_reads_ranges_back(usage):
    """The device form sizes its workspace from n_images alone (K19's way): the unit holds no ends kernel."""
    assert not [k for k in usage if "ends_kernel" in k]
    src = open(os.path.join(CSRC, "abi_fullcal.hip")).read()
    assert src.count("hipLaunchKernelGGL") == 2


def test_other_units_do_not_name_the_new_kernels():
    """The headers and units of K19, K21 and K22 and the headers under them know nothing of K23: what they share they take from
    clc_arrow.hpp, clc_jointterms.hpp and abi_jointcall.hpp (the last two may name every unit), never from one another."""
    for u in ("clc_arrow.hpp", "clc_camcal.hpp", "abi_camcal.hip", "clc_laserrange.hpp", "abi_laserrange.hip", "clc_jointrobust.hpp",
              "abi_jointrobust.hip", "clc_campose.hpp", "clc_math.hpp"):
        assert "fullcal" not in open(os.path.join(CSRC, u)).read(), u
