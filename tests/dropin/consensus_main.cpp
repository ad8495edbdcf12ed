// tests/dropin/consensus_main.cpp — TEST ONLY.  The consensus calibration through the drop-in header, as a C++11 caller of the
// reference's interface would use it: reads a std::vector<Oberserve>, a start Tcl and the candidate rows from a text file the test
// writes (so that both sides hold the same observations and the same rows, to the bit: %.17g), runs
// clc_adapter::Session::CalibrationConsensus, and prints the winning row, the inlier mask, the support sizes and the refined Tcl for
// the test to compare with the Python path and the oracle.
//   file: P, rms_max, n_rows, then 16 numbers of the start Tcl (row-major), then n_rows rows of P weights (0 / 1), then per
//         observation: qw qx qy qz tx ty tz n, n points (x y z)
//   usage: consensus_main FILE [use_linefitting_data use_boundary_constraint]
#include <cstdio>
#include <cstdlib>
#include <string>

#include "LaseCamCalCeres.h"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: consensus_main FILE [linefit boundary]\n"); return 2; }
    const bool linefit = argc > 2 && std::atoi(argv[2]) != 0, boundary = argc > 3 && std::atoi(argv[3]) != 0;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int P = 0, n_rows = 0;
    double rms_max = 0.0;
    if (std::fscanf(f, "%d %lf %d", &P, &rms_max, &n_rows) != 3 || P <= 0 || n_rows <= 0) return 2;
    Eigen::Matrix4d T = Eigen::Matrix4d::Identity();
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { double v; if (std::fscanf(f, "%lf", &v) != 1) return 2; T(i, j) = v; }
    std::vector<uint8_t> rows((size_t)n_rows * (size_t)P);
    for (size_t i = 0; i < rows.size(); ++i) { int w; if (std::fscanf(f, "%d", &w) != 1) return 2; rows[i] = (uint8_t)w; }
    std::vector<Oberserve> obs;
    for (int i = 0; i < P; ++i) {
        double q[4], t[3];
        int n = 0;
        if (std::fscanf(f, "%lf %lf %lf %lf %lf %lf %lf %d", &q[0], &q[1], &q[2], &q[3], &t[0], &t[1], &t[2], &n) != 8) return 2;
        Oberserve ob;
        ob.tagPose_Qca = Eigen::Quaterniond(q[0], q[1], q[2], q[3]);
        ob.tagPose_tca = Eigen::Vector3d(t[0], t[1], t[2]);
        for (int j = 0; j < n; ++j) {
            double x, y, z;
            if (std::fscanf(f, "%lf %lf %lf", &x, &y, &z) != 3) return 2;
            ob.points.push_back(Eigen::Vector3d(x, y, z));
        }
        ob.points_on_line = ob.points;
        obs.push_back(ob);
    }
    std::fclose(f);
    std::vector<uint8_t> inliers;
    std::vector<double> rms;
    std::vector<int> sizes;
    int best = -1;
    double cost = 0.0;
    clc_adapter::Session run(obs);
    if (!run.CalibrationConsensus(T, rms_max, inliers, (size_t)n_rows, 5, 0, linefit, boundary, rows.data(), &rms, &sizes, &best, &cost) ||
        !run.ok()) {
        std::printf("CONSENSUS failed best=%d\n", best);
        return 1;
    }
    std::printf("BEST %d cost=%.17g\nMASK", best, cost);
    for (size_t i = 0; i < inliers.size(); ++i) std::printf(" %d", (int)inliers[i]);
    std::printf("\nSIZES");
    for (size_t i = 0; i < sizes.size(); ++i) std::printf(" %d", sizes[i]);
    std::printf("\nRMS");
    for (size_t i = 0; i < rms.size(); ++i) std::printf(" %.17g", rms[i]);
    std::printf("\nTCL");
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) std::printf(" %.17g", T(i, j));
    std::printf("\n");
    // the same call drawing its own rows (std::mt19937): must run and find a support of its own
    Eigen::Matrix4d T2 = Eigen::Matrix4d::Identity();
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) T2(i, j) = T(i, j);
    std::vector<uint8_t> in2;
    int best2 = -1;
    const bool ok2 = run.CalibrationConsensus(T2, rms_max, in2, 64, 5, 1, linefit, boundary, NULL, NULL, NULL, &best2);
    int n2 = 0;
    for (size_t i = 0; i < in2.size(); ++i) n2 += in2[i];
    std::printf("DRAWN ok=%d best=%d support=%d\n", ok2 ? 1 : 0, best2, n2);
    return 0;
}
