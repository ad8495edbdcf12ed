// tests/shim/guidance_shim.cpp — TEST ONLY.  Compiles K20 (camlasercalibratool_amd/csrc/clc_guidance.hpp: the cast of a candidate, the
// score of a candidate, the order of the argmax and the round's update) for the host with g++.  The lanes of a candidate's wave are
// a loop and the wave all-reduce a butterfly in the device's order; the candidates of a launch are a loop.  The tests compare it
// with the numpy restatement tests/guidance_ref.py, and the GPU tests compare the device against it.
#include <cmath>
#include <vector>

#include "../../camlasercalibratool_amd/csrc/clc_guidance.hpp"

namespace {

namespace gd = clc::gd;

// guidance_model of abi_guidance.hip, without its checks
gd::GuideModel model_of(const clc_guidance_options* o, const double* pose_cl) {
  gd::GuideModel g{};
  g.n_rays = o->n_rays; g.min_points = o->min_points; g.criterion = o->criterion;
  g.angle_min = o->angle_min; g.angle_increment = o->angle_increment; g.range_min = o->range_min; g.range_max = o->range_max;
  for (int i = 0; i < 2; ++i) { g.board_min[i] = o->board_min[i]; g.board_max[i] = o->board_max[i]; }
  g.eig_floor = o->eig_floor;
  clc::quat_to_rot(pose_cl + 3, g.Rcl);
  for (int i = 0; i < 3; ++i) g.tcl[i] = pose_cl[i];
  return g;
}

void cast_all(const gd::GuideModel& g, bool table, long long n, const double* q, const double* t, int32_t* n_hits, double* H_add) {
  std::vector<double> dirs((size_t)(2 * g.n_rays));
  for (int i = 0; i < g.n_rays; ++i) gd::ray_dir(g, i, &dirs[(size_t)(2 * i)], &dirs[(size_t)(2 * i + 1)]);
  gd::CastArgs a{};
  a.g = g; a.dirs = dirs.data(); a.q = q; a.t = t; a.n_cand = n; a.n_hits = n_hits; a.H_add = H_add;
  for (long long c = 0; c < n; ++c) {
    if (table) gd::cast_candidate<true>(a, c);
    else gd::cast_candidate<false>(a, c);
  }
}

gd::ScoreArgs score_args(const gd::GuideModel& g, const double* M, const double* H_add, const int32_t* n_hits, long long n) {
  gd::ScoreArgs s{};
  s.criterion = g.criterion; s.min_points = g.min_points; s.eig_floor = g.eig_floor; s.M = M; s.H_add = H_add; s.n_hits = n_hits; s.n_cand = n;
  return s;
}

}  // namespace

extern "C" {

int shim_guidance_options_size() { return (int)sizeof(clc_guidance_options); }

// clc_guidance_options_default (abi_guidance.hip)
void shim_guidance_options_default(clc_guidance_options* o) {
  const double fov = 270.0 * (3.14159265358979323846 / 180.0);
  o->n_rays = 1081;
  o->min_points = 50;
  o->angle_min = -fov / 2;
  o->angle_increment = fov / 1080;
  o->range_min = 0.05;
  o->range_max = 30.0;
  o->board_min[0] = o->board_min[1] = -0.043;
  o->board_max[0] = o->board_max[1] = 0.457;
  o->eig_floor = 1e-8;
  o->criterion = CLC_GUIDE_LOGDET;
  o->reserved = 0;
}

// clc_score_board_poses on the host; every output nullable; table = 0: a sincos per ray.
void shim_score_board_poses(const clc_guidance_options* o, const double* pose_cl, const double* H0, long long n, const double* q,
                            const double* t, int table, int32_t* n_hits, double* H_add, double* sv, double* score) {
  if (n <= 0) return;
  const gd::GuideModel g = model_of(o, pose_cl);
  std::vector<int32_t> nh((size_t)n);
  std::vector<double> Ha((size_t)(36 * n));
  cast_all(g, table != 0, n, q, t, nh.data(), Ha.data());
  double M[36];
  for (int i = 0; i < 36; ++i) M[i] = H0 ? H0[i] : 0.0;
  const gd::ScoreArgs s = score_args(g, M, Ha.data(), nh.data(), n);
  for (long long c = 0; c < n; ++c) {
    if (n_hits) n_hits[c] = nh[(size_t)c];
    if (H_add) for (int i = 0; i < 36; ++i) H_add[36 * c + i] = Ha[(size_t)(36 * c + i)];
    if (!sv && !score) continue;
    double w[6];
    const double sc = gd::score_candidate(s, c, w);
    if (sv) for (int i = 0; i < 6; ++i) sv[6 * c + i] = w[i];
    if (score) score[c] = sc;
  }
}

// clc_select_board_poses on the host: the rounds of select_device (abi_guidance.hip), the two kernels of a round as loops.
void shim_select_board_poses(const clc_guidance_options* o, const double* pose_cl, const double* H0, long long n, const double* q,
                             const double* t, long long k, long long* chosen, double* sv_after, double* score_after, double* H_after,
                             int32_t* n_chosen) {
  if (n <= 0) return;
  const gd::GuideModel g = model_of(o, pose_cl);
  std::vector<int32_t> nh((size_t)n);
  std::vector<double> Ha((size_t)(36 * n)), sv((size_t)(6 * n)), score((size_t)n), sva((size_t)(6 * k)), sca((size_t)k);
  std::vector<unsigned char> taken((size_t)n, 0);
  cast_all(g, true, n, q, t, nh.data(), Ha.data());
  double M[36];
  for (int i = 0; i < 36; ++i) M[i] = H0 ? H0[i] : 0.0;
  gd::ScoreArgs s = score_args(g, M, Ha.data(), nh.data(), n);
  s.taken = taken.data();
  gd::PickArgs p{};
  p.H_add = Ha.data(); p.sv = sv.data(); p.score = score.data(); p.M = M; p.taken = taken.data(); p.chosen = chosen;
  p.sv_after = sva.data(); p.score_after = sca.data();
  const long long rounds = k < n ? k : n;
  const double nan = std::nan("");
  int32_t nc = 0;
  for (long long r = 0; r < k; ++r) {
    if (r < rounds) {
      double bs = 0.0;
      long long bi = -1;
      for (long long c = 0; c < n; ++c) {
        score[(size_t)c] = gd::score_candidate(s, c, &sv[(size_t)(6 * c)]);
        const long long idx = gd::selectable(s, c, score[(size_t)c]) ? c : -1;
        if (gd::better(score[(size_t)c], idx, bs, bi)) { bs = score[(size_t)c]; bi = idx; }
      }
      p.round = (int)r;
      gd::pick_apply(p, bi, 0, 1);
    } else {
      chosen[r] = -1;
      sca[(size_t)r] = nan;
      for (int i = 0; i < 6; ++i) sva[(size_t)(6 * r + i)] = nan;
    }
    if (chosen[r] >= 0) ++nc;
    if (score_after) score_after[r] = sca[(size_t)r];
    if (sv_after) for (int i = 0; i < 6; ++i) sv_after[6 * r + i] = sva[(size_t)(6 * r + i)];
  }
  if (H_after) for (int i = 0; i < 36; ++i) H_after[i] = M[i];
  if (n_chosen) *n_chosen = nc;
}

}  // extern "C"
