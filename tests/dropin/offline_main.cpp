// tests/dropin/offline_main.cpp — TEST ONLY.  A ROS-free port of main/calibr_offline.cpp:51-175 on the drop-in header: reads the
// stamped tag poses and the laser scans from a text file the test writes (%.17g: both sides hold the same numbers), builds the
// observations on the device (clc_adapter::AssembleObservations), then closed form, Tcl = inv(Tlc) and CamLaserCalibration(obs, Tcl,
// false) on the scans the shared context already holds (Session::AdoptStored), and prints what the test compares.
//   file: n_poses, then per pose: stamp qw qx qy qz tx ty tz; n_scans, then per scan: stamp angle_min angle_increment range_min n, n ranges
//   usage: offline_main FILE
#include <cstdio>
#include <cstdlib>

#include "LaseCamCalCeres.h"

// inverse of a rigid transform (the Eigen stub of the tests has no general inverse())
static Eigen::Matrix4d invert(const Eigen::Matrix4d& T) {
    Eigen::Matrix4d I = Eigen::Matrix4d::Identity();
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) I(i, j) = T(j, i);
    for (int i = 0; i < 3; ++i) { double s = 0; for (int k = 0; k < 3; ++k) s += T(k, i) * T(k, 3); I(i, 3) = -s; }
    return I;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: offline_main FILE\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int n = 0, S = 0;
    if (std::fscanf(f, "%d", &n) != 1 || n < 0) return 2;
    std::vector<double> pose_stamp;
    std::vector<Eigen::Quaterniond> qwc;
    std::vector<Eigen::Vector3d> twc;
    for (int i = 0; i < n; ++i) {
        double v[8];
        for (int k = 0; k < 8; ++k) if (std::fscanf(f, "%lf", &v[k]) != 1) return 2;
        pose_stamp.push_back(v[0]);
        qwc.push_back(Eigen::Quaterniond(v[1], v[2], v[3], v[4]));
        twc.push_back(Eigen::Vector3d(v[5], v[6], v[7]));
    }
    if (std::fscanf(f, "%d", &S) != 1 || S < 0) return 2;
    std::vector<float> ranges, am, ai, rm;
    std::vector<int64_t> offsets(1, 0);
    std::vector<double> scan_stamp;
    for (int k = 0; k < S; ++k) {
        double st; float a, b, c; int m = 0;
        if (std::fscanf(f, "%lf %f %f %f %d", &st, &a, &b, &c, &m) != 5) return 2;
        scan_stamp.push_back(st); am.push_back(a); ai.push_back(b); rm.push_back(c);
        for (int j = 0; j < m; ++j) { float r; if (std::fscanf(f, "%f", &r) != 1) return 2; ranges.push_back(r); }
        offsets.push_back((int64_t)ranges.size());
    }
    std::fclose(f);
    if (pose_stamp.size() < 10) { std::cout << "apriltag pose less than 10." << std::endl; return 0; }  // :56
    clc_assemble_info info;
    bool ok = false;
    const std::vector<Oberserve> obs = clc_adapter::AssembleObservations(pose_stamp, qwc, twc, ranges, offsets, am, ai, rm, scan_stamp, &info, &ok);
    if (!ok) return 1;
    std::printf("INFO %lld %lld %lld %lld %lld %lld %lld\n", (long long)info.n_keyframes, (long long)info.n_segments, (long long)info.n_ref_throws,
                (long long)info.n_unmatched, (long long)info.n_observations, (long long)info.n_points, (long long)info.n_line_points);
    if (obs.size() < 5) { std::cout << "Valid Calibra Data Less" << std::endl; return 0; }  // :158
    size_t pts = 0, ptl = 0;
    for (size_t i = 0; i < obs.size(); ++i) { pts += obs[i].points.size(); ptl += obs[i].points_on_line.size(); }
    std::printf("OBS %zu %zu %zu\n", obs.size(), pts, ptl);
    clc_adapter::Session run((clc_adapter::Session::AdoptStored()));
    if (!run.ok()) return 1;
    Eigen::Matrix4d Tlc_initial = Eigen::Matrix4d::Identity();
    run.ClosedSolution(Tlc_initial);                       // :167
    if (!run.ok()) return 1;
    Eigen::Matrix4d Tcl = invert(Tlc_initial);             // :169
    run.Calibration(Tcl, false);                           // :170
    if (!run.ok()) return 1;
    std::printf("TCL");
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) std::printf(" %.17g", Tcl(i, j));
    std::printf("\n");
    // the calls that need the observations on the host refuse on an adopting session (and do not crash)
    {
        Eigen::Matrix4d starts[2] = {Tcl, Tcl};
        std::vector<uint8_t> w(obs.size(), 1), inl;
        const int best = run.CalibrationFromStarts(starts, 2, false);
        const bool a = run.ok();
        const bool sub = run.CalibrationSubsets(&w[0], 1, starts, false);
        Eigen::Matrix4d Tc = Tcl;
        const bool con = run.CalibrationConsensus(Tc, 0.01, inl);
        std::printf("HOSTONLY %d %d %d %d\n", best, a ? 1 : 0, sub ? 1 : 0, con ? 1 : 0);
        // ... and work on a Session that has the vector AssembleObservations returned
        clc_adapter::Session full(obs);
        const int b2 = full.CalibrationFromStarts(starts, 2, false);
        std::printf("FROMSTARTS %d %d\n", b2, full.ok() ? 1 : 0);
        run.ClosedSolution(Tlc_initial);  // `full` replaced the stored scans with the same observations: the adopting session refuses
        std::printf("AFTERFULL %d\n", run.ok() ? 1 : 0);
    }
    // another caller replaces the stored scans: the adopting session must refuse, not solve them
    std::vector<Oberserve> other(obs.begin(), obs.begin() + 5);
    Eigen::Matrix4d T2 = Eigen::Matrix4d::Identity();
    CamLaserCalClosedSolution(other, T2);
    run.ClosedSolution(T2);
    std::printf("REPLACED %d\n", run.ok() ? 0 : 1);
    return 0;
}
