#!/usr/bin/env python3
"""Generates tests/golden/segment_vectors.npz: the reference's own AutoGetLinePts (src/selectScanPoints.cpp:17-190) on
hand-made scans that pin each of its quirks and on seeded simdata.sim_laser_scans scans, for clc_board_segments.

A small driver is compiled with g++ into a temporary directory.  It #includes the reference's selectScanPoints.cpp where it
lies (nothing is copied) against oracle/ref_shim's Eigen stand-in and tests/golden/cv_stub's OpenCV stand-in, and calls
AutoGetLinePts(points, false) on every scan, with z replaced by the point's index (z is never read by the detection) so
that the returned points name the chosen index range; std::out_of_range is caught and reported as a status.

    python tests/golden/make_segment_golden.py [REFERENCE_ROOT]     # rewrite the fixture

Keys: hand_points [M,3], hand_offsets [S+1], hand_names [S], hand_seg [S,2], hand_status [S]; sim_seeds, sim_n_scans,
sim_sha256 (of the generated points), sim_seg, sim_status.  GPU tests read this file only."""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from camlasercalibratool_amd import simdata as sd  # noqa: E402

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include "selectScanPoints.cpp"
int main(int argc, char** argv) {
  FILE* f = std::fopen(argv[1], "rb");
  int64_t S;
  if (std::fread(&S, 8, 1, f) != 1) return 1;
  std::vector<int64_t> off(S + 1);
  if (std::fread(off.data(), 8, S + 1, f) != (size_t)(S + 1)) return 1;
  std::vector<double> P(3 * off[S]);
  if (off[S] && std::fread(P.data(), 8, P.size(), f) != P.size()) return 1;
  std::fclose(f);
  FILE* g = std::fopen(argv[2], "wb");
  for (int64_t k = 0; k < S; ++k) {
    std::vector<Eigen::Vector3d> pts;
    for (int64_t i = off[k]; i < off[k + 1]; ++i) pts.push_back(Eigen::Vector3d(P[3 * i], P[3 * i + 1], (double)(i - off[k])));
    int64_t r[3] = {-1, -1, 0};
    try {
      std::vector<Eigen::Vector3d> line = AutoGetLinePts(pts, false);
      if (!line.empty()) { r[0] = (int64_t)line.front().z(); r[1] = (int64_t)line.back().z(); r[2] = 1; }
    } catch (const std::out_of_range&) { r[2] = -1; }
    std::fwrite(r, 8, 3, g);
  }
  std::fclose(g);
  return 0;
}
"""


def build_driver(ref_root, tmp):
    src = os.path.join(tmp, "seg_driver.cpp")
    open(src, "w").write(DRIVER)
    exe = os.path.join(tmp, "seg_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-w", "-I", os.path.join(HERE, "cv_stub"),
                           "-I", os.path.join(ROOT, "oracle", "ref_shim"), "-I", os.path.join(ref_root, "include"),
                           "-I", os.path.join(ref_root, "src"), src, "-o", exe])
    return exe


def run_driver(exe, tmp, points, offsets):
    fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fi, "wb") as f:
        f.write(np.int64(len(offsets) - 1).tobytes() + np.asarray(offsets, np.int64).tobytes() + np.ascontiguousarray(points, np.float64).tobytes())
    subprocess.check_call([exe, fi, fo])
    r = np.fromfile(fo, dtype=np.int64).reshape(-1, 3)
    return r[:, :2].copy(), r[:, 2].astype(np.int32)


# ---- hand-made scans: each pins one behaviour of the reference ----
def _board(n, lo, hi, x=1.0, half=0.4, bg=5.0):
    """n points on the x axis at range bg, and points lo..hi-1 on the line x = `x`, y from -half to +half."""
    P = np.zeros((n, 3))
    P[:, 0] = bg
    P[lo:hi, 0] = x
    P[lo:hi, 1] = np.linspace(-half, half, hi - lo)
    return P


def hand_cases():
    C = []
    C.append(("basic", _board(1081, 420, 620)))
    C.append(("open_final_segment", _board(1081, 420, 1081)))  # the board runs past the window's end: never closed
    P = _board(1081, 420, 620)
    P[623:660, :2] = 1000.0  # invalid run right after the close: the next segment's id_end is preset on an invalid point
    P[660:760, 0], P[660:760, 1] = 1.2, np.linspace(-0.3, 0.3, 100)
    C.append(("invalid_run_after_close", P))
    P = _board(1081, 420, 620)
    P[500:530, :2] = 1000.0  # a hole of invalid returns inside the board: the current point waits, the segment goes on
    C.append(("hole_in_board", P))
    # the current point lands on a point only through an invalid one before it (d1 > 100 moves it on, :96-99)
    for tag, v in (("d_eq_100_current", 100.0), ("nan_current", np.nan), ("d_above_100_current", np.nextafter(100.0, 200.0))):
        P = _board(1081, 420, 620)
        P[274, :2] = 1000.0  # id_right
        P[277, :2] = (v, 0.0)
        C.append((tag, P))
    P = _board(1081, 274, 500)  # the board starts at id_right = 274: widening to the left is free, non-monotone
    P[271:274, 0] = (1.001, 1.2, 1.2)  # 273, 272 fail the 0.05 test against 274, 271 passes
    P[271:274, 1] = -0.4
    C.append(("nonmonotone_widening", P))
    P = _board(1081, 360, 430)
    P[460:530, 0], P[460:530, 1] = 1.0, np.linspace(-0.4, 0.4, 70)
    C.append(("equal_length_tie", P))
    for L in (48, 51, 54):  # id_end - id_start before widening is a multiple of 3: 50 itself cannot occur
        P = np.zeros((1081, 3))
        P[:, 0] = 5.0
        a = 400  # a grid point (id_right = 274, 400 - 274 = 126)
        P[a:a + L + 1, 0], P[a:a + L + 1, 1] = 1.0, np.linspace(-0.4, 0.4, L + 1)
        C.append((f"length_{L}", P))
    P = np.zeros((1081, 3))
    P[:, 0] = 5.0
    P[400:460, 0], P[400:460, 1] = 1.0, np.linspace(-0.1, 0.1, 60)  # first and last grid point of the run: y = -/+0.1
    P[400 + 57, 1], P[400, 1] = 0.1, -0.1
    P[458:460, :2] = 5.0
    C.append(("dist_exactly_0p2", P))
    P = P.copy()
    P[457, 1] = 0.1 + 1e-9
    C.append(("dist_above_0p2", P))
    for tag, end in (("end_norm_exactly_2", (2.0, 0.0)), ("end_norm_below_2", (np.nextafter(2.0, 0.0), 0.0))):
        P = np.zeros((1081, 3))
        P[:, 0] = 5.0
        P[400:458, 0], P[400:458, 1] = np.linspace(1.5, 2.0, 58), np.linspace(-0.6, 0.0, 58)
        P[457, :2] = end
        C.append((tag, P))
    P = _board(300, 0, 120)  # the first segment starts at index 0: widening to the left raises (:121)
    C.append(("throws_left_n300", P))
    P = _board(300, 120, 200)
    C.append(("short_scan_no_throw", P))
    for n in (537, 538):  # id_right = 2 / 3: a segment starting there raises / does not
        C.append((f"left_bound_n{n}", _board(n, max(n // 2 - 266, 0), n // 2)))
    C.append(("throws_not_best", np.concatenate([_board(300, 0, 80)[:150], _board(300, 150, 260)[150:]])))
    C.append(("n0", np.zeros((0, 3))))
    C.append(("n1", np.array([[1.0, 0.0, 0.0]])))
    C.append(("n7", _board(7, 0, 7)))
    return C


SIM_SEEDS = [11, 12, 13]
SIM_N_SCANS = 200


def sim_points(seed):
    return sd.scan_points_host(sd.sim_laser_scans(seed, SIM_N_SCANS))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    from oracle.ref import REF_ROOT  # the reference checkout oracle/ builds from (CLC_REF_ROOT)
    ref_root = sys.argv[1] if len(sys.argv) > 1 else REF_ROOT
    G = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(ref_root, tmp)
        C = hand_cases()
        P = np.concatenate([c[1] for c in C]) if C else np.zeros((0, 3))
        off = np.r_[0, np.cumsum([c[1].shape[0] for c in C])].astype(np.int64)
        seg, st = run_driver(exe, tmp, P, off)
        G.update(hand_points=P, hand_offsets=off, hand_names=np.array([c[0] for c in C]), hand_seg=seg, hand_status=st)
        segs, sts, shas = [], [], []
        for s in SIM_SEEDS:
            Q = sim_points(s)
            sg, stt = run_driver(exe, tmp, Q, np.arange(SIM_N_SCANS + 1, dtype=np.int64) * 1081)
            segs.append(sg), sts.append(stt), shas.append(sha(Q))
        G.update(sim_seeds=np.array(SIM_SEEDS), sim_n_scans=np.int64(SIM_N_SCANS), sim_sha256=np.array(shas),
                 sim_seg=np.stack(segs), sim_status=np.stack(sts))
    np.savez_compressed(os.path.join(HERE, "segment_vectors.npz"), **G)
    for name, s, t in zip(G["hand_names"], G["hand_seg"], G["hand_status"]):
        print(f"{name:24s} {t:3d} {s}")
    for s, t in zip(SIM_SEEDS, G["sim_status"]):
        print("sim", s, np.unique(t, return_counts=True))


if __name__ == "__main__":
    main()
