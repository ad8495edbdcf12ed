// tests/dropin/subsets_main.cpp — TEST ONLY.  Resampled calibrations through the drop-in header, as a C++11 caller of the reference's
// interface would use them: reads a std::vector<Oberserve> and a start Tcl from a text file the test writes (so that both sides
// hold the same observations, to the bit: %.17g), runs the leave-one-out rows plus one all-zero row through
// clc_adapter::Session::CalibrationSubsets, and prints every refined Tcl for the test to compare with the Python path.
//   file: P, then 16 numbers of the start Tcl (row-major), then per observation: qw qx qy qz tx ty tz n, n points (x y z)
//   usage: subsets_main FILE [use_linefitting_data use_boundary_constraint]
#include <cstdio>
#include <cstdlib>
#include <string>

#include "LaseCamCalCeres.h"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: subsets_main FILE [linefit boundary]\n"); return 2; }
    const bool linefit = argc > 2 && std::atoi(argv[2]) != 0, boundary = argc > 3 && std::atoi(argv[3]) != 0;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int P = 0;
    if (std::fscanf(f, "%d", &P) != 1 || P <= 0) return 2;
    Eigen::Matrix4d T0 = Eigen::Matrix4d::Identity();
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) { double v; if (std::fscanf(f, "%lf", &v) != 1) return 2; T0(i, j) = v; }
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
    const size_t S = (size_t)P + 1;  // leave-one-out rows, then a row with nothing in it
    std::vector<uint8_t> w(S * (size_t)P, 1);
    for (int k = 0; k < P; ++k) w[(size_t)k * (size_t)P + (size_t)k] = 0;
    for (int b = 0; b < P; ++b) w[(size_t)P * (size_t)P + (size_t)b] = 0;
    std::vector<Eigen::Matrix4d> T(S, T0);
    std::vector<double> cost(S);
    std::vector<int> term(S);
    clc_adapter::Session run(obs);
    if (!run.CalibrationSubsets(w.data(), S, T.data(), linefit, boundary, cost.data(), term.data()) || !run.ok()) {
        std::printf("SUBSETS failed\n");
        return 1;
    }
    for (size_t k = 0; k < S; ++k) {
        std::printf("SUBSET %zu term=%d cost=%.17g T=", k, term[k], cost[k]);
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) std::printf("%.17g ", T[k](i, j));
        std::printf("\n");
    }
    return 0;
}
