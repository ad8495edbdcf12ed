#!/usr/bin/env python3
"""The bits of the cooperative solve (csrc/clc_coop.hpp) on the inputs of tests/test_gpu_coop_gather_wave.py, recorded on ONE build:
pose and final cost as hex, the summary key (termination, iterations, evaluations, successful / unsuccessful steps), the workgroup
count the launch ran on.  A change of the kernel that claims "the same arithmetic in the same order" is held to them bit for bit.

cases() is the one definition of those inputs: the test imports it from here.  The seeds were fixed on the CPU: for every one of them
the oracle's DENSE_QR and normal-equation solves agree on termination and iteration count (--check-seeds repeats that; no GPU needed),
so no case sits on a rounding knife edge.

usage (GPU box, on the build to record):  python scripts/coop_golden_bits.py --head <commit> [--out tests/golden/coop_gather_wave_parent.json]
                                          python scripts/coop_golden_bits.py --check-seeds"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np

GOLDEN = os.path.join(ROOT, "tests", "golden", "coop_gather_wave_parent.json")
TWO_HOP_ABOVE = 32 * 256 * 13  # observations above which the solve runs on 256 workgroups with two hops (abi_layouts.hip, kCoopSmallMaxPpl)


def cases():
    """name -> (records, workgroups, points carry z)"""
    import camlasercalibratool_amd as clc
    from camlasercalibratool_amd import simdata as sd
    out = {}
    rec = clc.flatten_observations(sd.sim_fixed_count(41, 214, 500, noise_sigma=0.01), False)  # 107 000: 2 points per lane
    out["two_hop_smallest"] = (rec, 256, 0)
    recz = rec.copy()
    recz[7, 6] = 1e-3  # one point off the lidar plane: the 24-byte-slot form
    out["z_form"] = (recz, 256, 1)
    rag = clc.flatten_observations(sd.GenerateSimData(43, n_poses=1400, noise_sigma=0.02), False)
    assert rag.shape[0] > 107000
    out["ragged_scans"] = (np.ascontiguousarray(rag[:107000]), 256, 0)  # scans of 0..180 points: chunks cut scans, lanes are short
    out["block_boundary"] = (clc.flatten_observations(sd.sim_fixed_count(45, 1060, 500, noise_sigma=0.01), False), 256, 0)  # 9 points per lane
    out["one_hop"] = (clc.flatten_observations(sd.sim_fixed_count(49, 48, 500, noise_sigma=0.01), False), 32, 0)  # 24 000 observations
    for name, (r, wgs, z) in out.items():
        assert (r.shape[0] > TWO_HOP_ABOVE) == (wgs == 256), name
    return out


def key(s):
    return [int(s.termination), int(s.num_iterations), int(s.num_evaluations), int(s.num_successful_steps), int(s.num_unsuccessful_steps)]


def bits(res):
    return {"pose": [float(v).hex() for v in res.pose], "final_cost": float(res.summary.final_cost).hex(), "key": key(res.summary)}


def check_seeds():
    import oracle
    from camlasercalibratool_amd import simdata as sd
    oracle.build()
    x0 = sd.pose7_from_T(np.eye(4))
    ok = True
    for name, (rec, _, _) in cases().items():
        a, b = (oracle.solve(rec, x0, linear_solver=ls).summary for ls in ("qr", "ne"))
        same = a.termination == b.termination and a.num_iterations == b.num_iterations
        ok = ok and same
        print(f"{name}: n = {rec.shape[0]}, qr {a.termination}/{a.num_iterations}, ne {b.termination}/{b.num_iterations}: {'agree' if same else 'KNIFE EDGE'}")
    return ok


def main():
    if "--check-seeds" in sys.argv:
        sys.exit(0 if check_seeds() else 1)
    import camlasercalibratool_amd as clc
    from camlasercalibratool_amd import simdata as sd
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    head = sys.argv[sys.argv.index("--head") + 1] if "--head" in sys.argv else None
    x0 = sd.pose7_from_T(np.eye(4))
    doc = {"recorded_on_commit": head, "device": None, "cases": {}}
    with clc.Solver(0) as sv:
        doc["device"] = sv.device_info()[0]
        for name, (rec, wgs, z) in cases().items():
            sv.set_launch(0, -1)
            sv.upload(rec)
            pi = sv.path_info()
            assert pi.coop_resident == 1 and pi.coop_workgroups == wgs and pi.coop_points_carry_z == z, name
            n0, t0 = pi.coop_solves, pi.coop_timeouts
            r, r2 = sv.solve(x0), sv.solve(x0)
            pi = sv.path_info()
            assert pi.coop_solves == n0 + 2 and pi.coop_timeouts == t0, name  # both ran as the one launch
            assert np.array_equal(r.pose, r2.pose) and r.summary.final_cost == r2.summary.final_cost, name
            doc["cases"][name] = dict(bits(r), observations=int(rec.shape[0]), workgroups=wgs, points_per_lane=int(pi.coop_points_per_lane))
            print(name, json.dumps(doc["cases"][name]))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
