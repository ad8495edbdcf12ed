#!/usr/bin/env python3
"""Generates tests/golden/static_poses_ref.json: inputs and outputs of the REFERENCE'S OWN GetStaticPose (src/utilities.cpp:86-155,
compiled into oracle/_ref/libref.so by `make -C oracle ref`) on about 200 stamped poses, so that tests/stations_ref.py and the GPU
kernels are checked against the reference's code wherever the suite runs.  The driver below is this project's: it fills a
std::vector<CamPose>, calls GetStaticPose and prints what came back; it is compiled against oracle/ref_shim and linked with
libref.so in a temporary directory, and only the JSON is kept.

The poses: runs of 29, 30 and 31 distinct poses (members 30, 31, 32: the first is no station), a single breaker and two breakers in
a row, a NaN translation inside a run and at a run's start, mixed quaternion signs, a slow drift, an open run at the end.

    python tests/golden/make_static_poses_golden.py        # rewrite the fixture (needs the reference sources, see oracle/ref.py)
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle.ref as ref  # noqa: E402
import stations_ref as SR  # noqa: E402
from camlasercalibratool_amd import simdata as sd  # noqa: E402

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "utilities.h"
int main() {
  int n = 0;
  if (std::scanf("%d", &n) != 1) return 1;
  std::vector<CamPose> poses(n);
  for (int i = 0; i < n; ++i) {
    double s, w, x, y, z, a, b, c;
    if (std::scanf("%lf %lf %lf %lf %lf %lf %lf %lf", &s, &w, &x, &y, &z, &a, &b, &c) != 8) return 1;
    poses[i].timestamp = s;
    poses[i].start_time = poses[i].end_time = 0.0;
    poses[i].qwc = Eigen::Quaterniond(w, x, y, z);
    poses[i].twc = Eigen::Vector3d(a, b, c);
  }
  std::vector<CamPose> avg;
  std::vector<std::vector<CamPose> > runs = GetStaticPose(poses, avg);
  std::printf("%zu\n", avg.size());
  for (size_t k = 0; k < avg.size(); ++k)
    std::printf("%zu %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", runs[k].size(), runs[k].front().timestamp,
                runs[k].back().timestamp, avg[k].start_time, avg[k].end_time, avg[k].qwc.w(), avg[k].qwc.x(), avg[k].qwc.y(), avg[k].qwc.z(),
                avg[k].twc(0), avg[k].twc(1), avg[k].twc(2));
  return 0;
}
"""


def make_poses(seed):
    rng = np.random.default_rng(seed)
    t, q = [], []

    def station(k, nan_at=None, flip=False, drift=0.0):
        c = rng.uniform(-1.0, 1.0, 3)
        ang = rng.uniform(-0.6, 0.6, 3)
        for i in range(k):
            a = ang + rng.normal(0, 0.002, 3)
            qq = sd.rot_to_quat_wxyz(sd.rot_zyx(a[0], a[1], a[2])[0]).reshape(4)
            q.append(-qq if (flip and i % 2) else qq)
            p = c + rng.normal(0, 0.0002, 3) + drift * i * np.array([1.0, 0.0, 0.0])
            if nan_at is not None and i == nan_at:
                p = np.array([p[0], np.nan, p[2]])
            t.append(p)

    def breaker():
        t.append(rng.uniform(3.0, 4.0, 3)); q.append(np.array([1.0, 0.0, 0.0, 0.0]))

    station(29); breaker()                       # members 30: no station
    station(30); breaker(); breaker()            # members 31: a station; two breakers (the second is a run of its own, closed by the
    station(32, flip=True); breaker()            # ... first pose of this run, which is discarded: 31 distinct poses remain)
    station(40, nan_at=33); breaker()            # closed by the NaN after 33 poses; the rest too short
    station(3, nan_at=0)                         # a NaN at a run's start: a run of one member
    station(38, drift=0.00002); breaker()        # a drift the running centre follows
    station(35)                                  # open at the end: dropped
    n = len(t)
    return 100.0 + np.arange(n) / 30.0, np.array(q), np.array(t)


def run_reference(stamp, q, t):
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        lib = ref.build()
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-w", "-I", os.path.join(ROOT, "oracle", "ref_shim"),
                               "-I", os.path.join(ref.REF_ROOT, "include"), src, lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
        text = "%d\n" % len(stamp) + "".join(" ".join("%.17g" % v for v in [stamp[i], *q[i], *t[i]]) + "\n" for i in range(len(stamp)))
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    k = int(out[0])
    rows = np.array([[float(v) for v in out[1 + i].split()] for i in range(k)]).reshape(k, 12)
    index = {float(s): i for i, s in enumerate(stamp)}
    return {"members": [int(v) for v in rows[:, 0]], "first": [index[v] for v in rows[:, 1]], "last": [index[v] for v in rows[:, 2]],
            "start_time": rows[:, 3].tolist(), "end_time": rows[:, 4].tolist(), "q": rows[:, 5:9].tolist(), "t": rows[:, 9:12].tolist()}


if __name__ == "__main__":
    stamp, q, t = make_poses(20261018)
    w = SR.walk(t)
    assert w["margin"] >= 1e-6, w["margin"]
    got = run_reference(stamp, q, t)
    G = {"pose_stamp": stamp.tolist(), "q_wc": q.tolist(), "t_wc": t.tolist(), "ref": got}
    out = os.path.join(HERE, "static_poses_ref.json")
    with open(out, "w") as f:
        json.dump(G, f)
    print(out, os.path.getsize(out), "bytes;", len(stamp), "poses,", len(got["first"]), "stations: members", got["members"], "margin", w["margin"])
