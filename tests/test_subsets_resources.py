"""Build-time guard of the weighted resident kernel (clc_solve_subsets), without a GPU: hipcc's kernel-resource-usage remarks for
gfx950.  The weighted instantiations of resident_solve_kernel are bounded like their unweighted twins (tests/test_build_resources.py):
at most 256 VGPRs, two waves per SIMD, and no more scratch than the twin's bound — 128 bytes, 160 for the form whose points carry z."""
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
    p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + ["-c", os.path.join(CSRC, "abi_batched.hip"), "-o", str(tmp / "abi_batched.o"),
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


def _split(usage):
    """resident_solve_kernel<LOSS, NT, NW, PR, PL, CTRL, Z, WEIGHTED>: -> {(loss, nt, nw, pr, pl, ctrl, z): {weighted: remarks}}."""
    out = {}
    for k, v in usage.items():
        m = re.search(r"21resident_solve_kernelILb(\d)ELb(\d)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELb(\d)EE", k)
        if m:
            out.setdefault(tuple(int(g) for g in m.groups()[:7]), {})[int(m.group(8))] = v
    return out


def test_weighted_resident_kernels_are_bounded_like_their_twins(usage):
    forms = _split(usage)
    weighted = {f: v for f, v in forms.items() if 1 in v}
    # the forms multi-start covers: 256 lanes, 512 lanes, 512 lanes with z — each with and without the robust loss
    assert {(f[2], f[3], f[4], f[6]) for f in weighted} == {(4, 23, 19, 0), (8, 4, 18, 0), (8, 10, 12, 1)}
    assert {f[0] for f in weighted} == {0, 1}
    for f, v in sorted(weighted.items()):
        assert 0 in v, ("no unweighted twin", f)
        w, twin = v[1], v[0]
        bound = 160 if f[6] else 128   # tests/test_build_resources.py's bound of the twin
        print(f, "weighted", w, "twin", twin)
        assert w["VGPRs"] <= 256 and w["Occupancy"] >= 2, (f, w)
        assert w["ScratchSize"] <= bound and twin["ScratchSize"] <= bound, (f, w, twin)
