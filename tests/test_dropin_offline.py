"""The offline flow through the C++ drop-in header: tests/dropin/offline_main.cpp — a ROS-free port of main/calibr_offline.cpp:51-175
on clc_adapter::AssembleObservations and the adopting Session — compiled as C++11 against the Eigen stub and linked to the C-ABI
library.  CPU: it compiles and links.  GPU: on the simoffline recording it builds the restatement's observations, reaches the Python
path's Tcl, and its adopting Session refuses scans that were replaced."""
import os
import re
import subprocess

import numpy as np
import pytest

from camlasercalibratool_amd import _build, simdata as sd, simoffline as so

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(HERE, "dropin", "offline_main")


def _build_exe():
    src = os.path.join(HERE, "dropin", "offline_main.cpp")
    deps = [src, os.path.join(ROOT, "include", "LaseCamCalCeres.h"), os.path.join(ROOT, "include", "clc.h"), _build.LIB_PATH]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        lib_dir = os.path.dirname(_build.LIB_PATH)
        subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
                               "-I", os.path.join(HERE, "dropin", "eigen_stub"), src, "-o", EXE,
                               "-L", lib_dir, "-lclc_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return EXE


def test_offline_main_compiles_as_cxx11_and_links():
    assert os.path.exists(_build_exe())


def _write(rec, path):
    sc = rec["scans"]
    with open(path, "w") as f:
        n = len(rec["pose_stamp"])
        f.write(f"{n}\n")
        for i in range(n):
            f.write(" ".join("%.17g" % v for v in [rec["pose_stamp"][i], *rec["q_wc"][i], *rec["t_wc"][i]]) + "\n")
        S = len(rec["scan_stamp"])
        f.write(f"{S}\n")
        for k in range(S):
            r = sc["ranges"][sc["offsets"][k]:sc["offsets"][k + 1]]
            f.write("%.17g %.9g %.9g %.9g %d\n" % (rec["scan_stamp"][k], sc["angle_min"][k], sc["angle_increment"][k], sc["range_min"][k], len(r)))
            f.write(" ".join("%.9g" % v for v in r) + "\n")


@pytest.mark.gpu
def test_offline_main_on_the_recording(tmp_path):
    import camlasercalibratool_amd as clc
    rec = so.recording(1)
    path = str(tmp_path / "recording.txt")
    _write(rec, path)
    p = subprocess.run([_build_exe(), path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-800:]
    with clc.Solver(0) as sv:
        out = clc.CalibrateOffline(rec["pose_stamp"], rec["q_wc"], rec["t_wc"], rec["scans"], rec["scan_stamp"], solver=sv, verbose=False)
    info = out["info"]
    got = [int(v) for v in re.search(r"INFO (.*)", p.stdout).group(1).split()]
    assert got == [getattr(info, f[0]) for f in info._fields_]  # the same library on the same numbers
    assert [int(v) for v in re.search(r"OBS (.*)", p.stdout).group(1).split()] == [info.n_observations, info.n_points, info.n_line_points]
    Tcl = np.array([float(v) for v in re.search(r"TCL (.*)", p.stdout).group(1).split()]).reshape(4, 4)
    # the same calls on the same stored scans; the start differs in the last bits (rigid inverse here, numpy's general inverse there),
    # so the two solves agree as two solves of one problem do: the project's gate on T_cl
    assert np.abs(Tcl - out["Tcl"]).max() <= 1e-6
    Tlc = np.linalg.inv(Tcl)
    assert np.abs(Tlc[:3, :3] - sd.GT_RLC).max() <= 2e-3 and np.abs(Tlc[:3, 3] - sd.GT_TLC).max() <= 2e-3
    assert "HOSTONLY -1 0 0 0" in p.stdout and "holds no observations" in p.stderr
    assert re.search(r"FROMSTARTS [01] 1", p.stdout) and "AFTERFULL 0" in p.stdout
    assert "REPLACED 1" in p.stdout and "adopted were replaced" in p.stderr
