// tests/shim/guidance_sanitize_main.cpp — TEST ONLY.  A stand-alone program over the edge shapes of K20's host functions
// (guidance_shim.cpp), every array of its exact size: built with -fsanitize=address,undefined and run as an ordinary process by
// tests/test_guidance_host.py.  Not loaded into Python, not run on a GPU.
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "guidance_shim.cpp"

namespace {

// A board facing the laser squarely, its centre `dist` ahead on the laser's x axis, under T_cl = the reference simulation's truth.
void facing(double dist, double lateral, double* q, double* t) {
  // R_ca = R_cl [y z x]: with R_cl = [[0,-1,0],[0,0,-1],[1,0,0]] this is diag(-1, -1, 1)
  q[0] = 0.0; q[1] = 0.0; q[2] = 0.0; q[3] = 1.0;
  const double centre_l[3] = {dist, lateral, 0.01};
  const double Rcl[9] = {0, -1, 0, 0, 0, -1, 1, 0, 0}, tcl[3] = {0.2, 0.3, -0.1};
  double c[3];
  for (int i = 0; i < 3; ++i) c[i] = Rcl[3 * i] * centre_l[0] + Rcl[3 * i + 1] * centre_l[1] + Rcl[3 * i + 2] * centre_l[2] + tcl[i];
  t[0] = c[0] + 0.207; t[1] = c[1] + 0.207; t[2] = c[2];
}

int check(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); std::exit(1); }
  return 0;
}

}  // namespace

int main() {
  const double pose_cl[7] = {0.2, 0.3, -0.1, 0.5, -0.5, 0.5, 0.5};  // the quaternion (w 0.5; x 0.5, y -0.5, z 0.5) of R_cl above
  const int rays[] = {1, 63, 64, 65, 1081};
  const long long cands[] = {1, 3, 4, 5, 9};
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  long long total_hits = 0;
  for (int nr : rays)
    for (long long n : cands)
      for (int crit = 0; crit < 2; ++crit) {
        clc_guidance_options o;
        shim_guidance_options_default(&o);
        o.criterion = crit;
        if (nr != 1081) {
          o.n_rays = nr;
          o.angle_min = nr > 1 ? -0.6 : 0.0;
          o.angle_increment = nr > 1 ? 1.2 / (nr - 1) : 0.0;
          o.min_points = nr / 8 > 1 ? nr / 8 : 1;
        }
        std::vector<double> q((size_t)(4 * n)), t((size_t)(3 * n)), Ha((size_t)(36 * n)), sv((size_t)(6 * n)), sc((size_t)n), H0(36, 0.0);
        std::vector<int32_t> nh((size_t)n);
        for (long long i = 0; i < n; ++i) facing(0.8 + 0.3 * (double)i, 0.02 * (double)i, &q[(size_t)(4 * i)], &t[(size_t)(3 * i)]);
        if (n >= 3) q[4 * 1 + 2] = nan;              // a non-finite candidate in the batch
        if (n >= 4) t[3 * 3 + 0] = inf;
        if (n >= 5) { q[4 * 4] = 1.0; q[4 * 4 + 3] = 0.0; }  // R_ca = I: the board's normal is the camera's z = the laser's x ... a facing board too
        for (int i = 0; i < 6; ++i) H0[(size_t)(7 * i)] = i < 3 ? 2.0 : 0.0;
        for (int table = 0; table < 2; ++table) {
          shim_score_board_poses(&o, pose_cl, table ? H0.data() : nullptr, n, q.data(), t.data(), table, nh.data(), Ha.data(), sv.data(),
                                 sc.data());
          shim_score_board_poses(&o, pose_cl, H0.data(), n, q.data(), t.data(), table, nullptr, nullptr, nullptr, sc.data());
          shim_score_board_poses(&o, pose_cl, H0.data(), n, q.data(), t.data(), table, nh.data(), nullptr, nullptr, nullptr);
        }
        check(nh[0] >= 1, "the first board is hit");
        if (n >= 3) check(nh[1] == -1, "non-finite candidate");
        for (long long i = 0; i < n; ++i) total_hits += nh[(size_t)i] > 0 ? nh[(size_t)i] : 0;
        const long long ks[] = {1, n, n + 3};
        for (long long k : ks) {
          std::vector<long long> ch((size_t)k);
          std::vector<double> sva((size_t)(6 * k)), sca((size_t)k), Hf(36);
          int32_t nc = -1;
          shim_select_board_poses(&o, pose_cl, H0.data(), n, q.data(), t.data(), k, ch.data(), sva.data(), sca.data(), Hf.data(), &nc);
          check(nc >= 1 && nc <= n && ch[0] >= 0 && ch[0] < n, "a first choice");
          for (long long r = nc; r < k; ++r) check(ch[(size_t)r] == -1, "padding");
          shim_select_board_poses(&o, pose_cl, nullptr, n, q.data(), t.data(), k, ch.data(), nullptr, nullptr, nullptr, nullptr);
        }
      }
  // every ray hits: a rectangle far larger than the scan's footprint; no ray hits: the board in the scan plane
  {
    clc_guidance_options o;
    shim_guidance_options_default(&o);
    o.n_rays = 65; o.angle_min = -0.6; o.angle_increment = 1.2 / 64; o.min_points = 65;
    o.board_min[0] = o.board_min[1] = -100.0; o.board_max[0] = o.board_max[1] = 100.0;
    double q[4], t[3], Ha[36], sv[6], sc;
    int32_t nh;
    facing(1.0, 0.0, q, t);
    shim_score_board_poses(&o, pose_cl, nullptr, 1, q, t, 1, &nh, Ha, sv, &sc);
    check(nh == 65 && Ha[0] + Ha[7] + Ha[14] > 0.99, "every ray hits");
    const double qi[4] = {0.5, 0.5, -0.5, 0.5};  // R_ca = R_cl: the board lies in the scan plane
    shim_score_board_poses(&o, pose_cl, nullptr, 1, qi, pose_cl, 1, &nh, Ha, sv, &sc);
    check(nh == 0 && Ha[0] == 0.0, "coplanar board");
  }
  std::printf("hits %lld\nshapes ok\n", total_hits);
  return 0;
}
