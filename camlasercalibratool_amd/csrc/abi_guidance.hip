// abi_guidance.hip — clc_guidance_options_default, clc_score_board_poses(_device), clc_select_board_poses(_device): pose guidance
// (K20 in clc_guidance.hpp).  A unit of its own, held to its own register figures (tests/test_guidance_resources.py).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "abi_staging.hpp"
#include "clc_guidance.hpp"

using namespace clc_abi;

namespace {

namespace gd = clc::gd;

#ifdef CLC_TEST_HOOKS
std::atomic<int> g_dir_table{1};  // clc_debug_guidance_dirs: 0 = a sincos per ray instead of the table (scripts/guidance.py measures both)
std::atomic<int> g_score_rows{0};  // clc_debug_guidance_score_rows: 1 = clc_score_board_poses scores with one wave per candidate
#endif

// The options (the caller's or the defaults), T_cl and H0, checked: everything that can be refused without the device.
int guidance_model(const clc_guidance_options* in, const double* pose_cl, const double* H0, const char* who, gd::GuideModel* g, double* M0) {
  const std::string w(who);
  clc_guidance_options o;
  if (in) o = *in; else clc_guidance_options_default(&o);
  if (o.n_rays <= 0 || o.n_rays > (1 << 24)) return fail(CLC_ERR_INVALID_ARG, (w + ": n_rays must be in [1, 2^24]").c_str());
  if (o.min_points < 1) return fail(CLC_ERR_INVALID_ARG, (w + ": min_points must be >= 1").c_str());
  if (!(o.range_min < o.range_max)) return fail(CLC_ERR_INVALID_ARG, (w + ": range_min must be < range_max").c_str());
  if (!(std::isfinite(o.angle_min) && std::isfinite(o.angle_increment))) return fail(CLC_ERR_INVALID_ARG, (w + ": non-finite scan angle").c_str());
  if (!(o.board_min[0] <= o.board_max[0] && o.board_min[1] <= o.board_max[1]))
    return fail(CLC_ERR_INVALID_ARG, (w + ": empty board rectangle").c_str());
  if (!(o.eig_floor > 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": eig_floor must be > 0").c_str());
  if (o.criterion != CLC_GUIDE_LOGDET && o.criterion != CLC_GUIDE_MIN_EIG) return fail(CLC_ERR_INVALID_ARG, (w + ": unknown criterion").c_str());
  if (!pose_cl) return fail(CLC_ERR_INVALID_ARG, (w + ": bad argument").c_str());
  if (!all_finite(pose_cl, 7)) return fail(CLC_ERR_NONFINITE, (w + ": non-finite pose").c_str());
  if (H0 && !all_finite(H0, 36)) return fail(CLC_ERR_NONFINITE, (w + ": non-finite H0").c_str());
  g->n_rays = o.n_rays; g->min_points = o.min_points; g->criterion = o.criterion; g->reserved = 0;
  g->angle_min = o.angle_min; g->angle_increment = o.angle_increment; g->range_min = o.range_min; g->range_max = o.range_max;
  for (int i = 0; i < 2; ++i) { g->board_min[i] = o.board_min[i]; g->board_max[i] = o.board_max[i]; }
  g->eig_floor = o.eig_floor;
  clc::quat_to_rot(pose_cl + 3, g->Rcl);
  for (int i = 0; i < 3; ++i) g->tcl[i] = pose_cl[i];
  for (int i = 0; i < 36; ++i) M0[i] = H0 ? H0[i] : 0.0;
  return CLC_OK;
}

// The direction table and the cast of every candidate, on the handle's stream.
void enqueue_cast(Staging& st, const gd::GuideModel& g, const double* q, const double* t, size_t n, int32_t* n_hits, double* H_add) {
  double* dirs = st.scratch<double>(2 * (size_t)g.n_rays);
  gd::CastArgs a{};
  a.g = g; a.dirs = dirs; a.q = q; a.t = t; a.n_cand = (long long)n; a.n_hits = n_hits; a.H_add = H_add;
  if (!st.ok()) return;
  const unsigned blocks = (unsigned)((n + gd::CAST_WAVES - 1) / gd::CAST_WAVES);
#ifdef CLC_TEST_HOOKS
  if (!g_dir_table.load(std::memory_order_relaxed)) {
    hipLaunchKernelGGL(gd::guidance_cast_kernel<false>, dim3(blocks), dim3(gd::CAST_THREADS), 0, st.stream(), a);
    st.launched();
    return;
  }
#endif
  hipLaunchKernelGGL(gd::guidance_dirs_kernel, dim3((unsigned)((g.n_rays + 255) / 256)), dim3(256), 0, st.stream(), g, dirs);
  st.launched();
  if (!st.ok()) return;
  hipLaunchKernelGGL(gd::guidance_cast_kernel<true>, dim3(blocks), dim3(gd::CAST_THREADS), 0, st.stream(), a);
  st.launched();
}

unsigned score_blocks(size_t n) { return (unsigned)((n + gd::SCORE_THREADS - 1) / gd::SCORE_THREADS); }

// What the score kernels read and write, every array on the device (the fields of the greedy rounds left NULL).
gd::ScoreArgs score_args(const gd::GuideModel& g, const double* M, const double* H_add, const int32_t* n_hits, size_t n, double* sv,
                         double* score) {
  gd::ScoreArgs s{};
  s.criterion = g.criterion; s.min_points = g.min_points; s.eig_floor = g.eig_floor;
  s.M = M; s.H_add = H_add; s.n_hits = n_hits; s.n_cand = (long long)n; s.sv = sv; s.score = score;
  return s;
}

// Cast and score with the candidates and the outputs (every one nullable) in device memory, under both forms of
// clc_score_board_poses.  The cast's outputs are needed whether or not the caller takes them: NULL -> scratch.
void enqueue_score(Staging& st, const gd::GuideModel& g, const double* M0, size_t n, const double* q, const double* t, int32_t* n_hits,
                   double* H_add, double* sv, double* score) {
  if (!n_hits) n_hits = st.scratch<int32_t>(n);
  if (!H_add) H_add = st.scratch<double>(36 * n);
  enqueue_cast(st, g, q, t, n, n_hits, H_add);
  if (!sv && !score) return;
  const gd::ScoreArgs s = score_args(g, st.in(M0, 36), H_add, n_hits, n, sv, score);
  if (!st.ok()) return;
#ifdef CLC_TEST_HOOKS
  if (g_score_rows.load(std::memory_order_relaxed)) {
    hipLaunchKernelGGL(gd::guidance_score_rows_kernel, dim3((unsigned)((n + gd::CAST_WAVES - 1) / gd::CAST_WAVES)), dim3(gd::CAST_THREADS), 0,
                       st.stream(), s);
    st.launched();
    return;
  }
#endif
  hipLaunchKernelGGL(gd::guidance_score_kernel<false>, dim3(score_blocks(n)), dim3(gd::SCORE_THREADS), 0, st.stream(), s);
  st.launched();
}

// The greedy choice with the candidates in device memory, under both forms of clc_select_board_poses: the cast once, `rounds` rounds
// back to back, the small results to the host arrays, one synchronisation.
int select_on_device(Staging& st, const char* who, const gd::GuideModel& g, const double* M0, size_t n, const double* q, const double* t,
                     size_t k, int64_t* chosen, double* sv_after, double* score_after, double* H_after, int32_t* n_chosen) {
  static_assert(sizeof(long long) == sizeof(int64_t), "index type");
  const size_t rounds = std::min(k, n);
  const unsigned blocks = score_blocks(n);
  double* M = H_after ? st.inout(H_after, 36, M0) : st.in(M0, 36);  // the running information matrix
  double* H_add = st.scratch<double>(36 * n);
  double* sv = st.scratch<double>(6 * n);
  double* score = st.scratch<double>(n);
  double* best_s = st.scratch<double>(blocks);
  long long* best_i = st.scratch<long long>(blocks);
  int32_t* n_hits = st.scratch<int32_t>(n);
  unsigned char* taken = st.scratch<unsigned char>(n);
  long long* ch = st.out(reinterpret_cast<long long*>(chosen), rounds);
  double* sva = sv_after ? st.out(sv_after, 6 * rounds) : st.scratch<double>(6 * rounds);
  double* sca = score_after ? st.out(score_after, rounds) : st.scratch<double>(rounds);
  if (st.ok()) st.check(hipMemsetAsync(taken, 0, n, st.stream()));
  enqueue_cast(st, g, q, t, n, n_hits, H_add);
  gd::ScoreArgs s = score_args(g, M, H_add, n_hits, n, sv, score);
  s.taken = taken; s.best_score = best_s; s.best_index = best_i;
  gd::PickArgs p{};
  p.n_blocks = (long long)blocks; p.best_score = best_s; p.best_index = best_i; p.H_add = H_add; p.sv = sv; p.score = score;
  p.M = M; p.taken = taken; p.chosen = ch; p.sv_after = sva; p.score_after = sca;
  for (size_t r = 0; r < rounds && st.ok(); ++r) {
    hipLaunchKernelGGL(gd::guidance_score_kernel<true>, dim3(blocks), dim3(gd::SCORE_THREADS), 0, st.stream(), s);
    st.launched();
    if (!st.ok()) break;
    p.round = (int)r;
    hipLaunchKernelGGL(gd::guidance_pick_kernel, dim3(1), dim3(gd::PICK_THREADS), 0, st.stream(), p);
    st.launched();
  }
  CLC_TRY(st.finish(who));
  const double nan = std::nan("");
  int32_t nc = 0;
  for (size_t r = 0; r < k; ++r) {
    if (r >= rounds) {
      chosen[r] = -1;
      if (score_after) score_after[r] = nan;
      if (sv_after) for (int i = 0; i < 6; ++i) sv_after[6 * r + i] = nan;
    }
    if (chosen[r] >= 0) ++nc;
  }
  if (n_chosen) *n_chosen = nc;
  return CLC_OK;
}

int count_check(const char* who, size_t n, const void* q, const void* t) {
  if (n > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": too many candidates").c_str());
  if (n > 0 && (!q || !t)) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": bad argument").c_str());
  return CLC_OK;
}

}  // namespace

extern "C" {

void clc_guidance_options_default(clc_guidance_options* o) {
  if (!o) return;
  const double fov = 270.0 * (3.14159265358979323846 / 180.0);  // the geometry of the project's simulated scans: 1 081 rays over 270 degrees
  o->n_rays = 1081;
  o->min_points = 50;  // the shortest segment AutoGetLinePts accepts
  o->angle_min = -fov / 2;
  o->angle_increment = fov / 1080;
  o->range_min = 0.05;
  o->range_max = 30.0;  // src/utilities.cpp:201
  o->board_min[0] = o->board_min[1] = -0.043;  // src/LaseCamCalCeres.cpp:262-268
  o->board_max[0] = o->board_max[1] = 0.457;
  o->eig_floor = 1e-8;  // :371
  o->criterion = CLC_GUIDE_LOGDET;
  o->reserved = 0;
}

int clc_score_board_poses_device(clc_handle* h, const clc_guidance_options* gopt, const double pose_cl[7], const double* H0, size_t n_cand,
                                 const double* q_ca_wxyz_dev, const double* t_ca_dev, int32_t* n_hits_dev, double* H_add_dev,
                                 double* sv_dev, double* score_dev) {
  const char* who = "clc_score_board_poses_device";
  gd::GuideModel g;
  double M0[36];
  CLC_TRY(guidance_model(gopt, pose_cl, H0, who, &g, M0));
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_score_board_poses_device: bad argument");
  CLC_TRY(count_check(who, n_cand, q_ca_wxyz_dev, t_ca_dev));
  if (n_cand == 0 || (!n_hits_dev && !H_add_dev && !sv_dev && !score_dev)) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  enqueue_score(st, g, M0, n_cand, q_ca_wxyz_dev, t_ca_dev, n_hits_dev, H_add_dev, sv_dev, score_dev);
  return st.finish(who);
}

int clc_score_board_poses(clc_handle* h, const clc_guidance_options* gopt, const double pose_cl[7], const double* H0, size_t n_cand,
                          const double* q_ca_wxyz, const double* t_ca, int32_t* n_hits, double* H_add, double* sv, double* score) {
  const char* who = "clc_score_board_poses";
  gd::GuideModel g;
  double M0[36];
  CLC_TRY(guidance_model(gopt, pose_cl, H0, who, &g, M0));
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_score_board_poses: bad argument");
  CLC_TRY(count_check(who, n_cand, q_ca_wxyz, t_ca));
  if (n_cand == 0 || (!n_hits && !H_add && !sv && !score)) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const size_t n = n_cand;
  Staging st(h);
  const double* q_dev = st.in(q_ca_wxyz, 4 * n);
  const double* t_dev = st.in(t_ca, 3 * n);
  int32_t* n_hits_dev = st.out_opt(n_hits, n);
  double* H_add_dev = st.out_opt(H_add, 36 * n);
  double* sv_dev = st.out_opt(sv, 6 * n);
  enqueue_score(st, g, M0, n, q_dev, t_dev, n_hits_dev, H_add_dev, sv_dev, st.out_opt(score, n));
  return st.finish(who);
}

int clc_select_board_poses_device(clc_handle* h, const clc_guidance_options* gopt, const double pose_cl[7], const double* H0,
                                  size_t n_cand, const double* q_ca_wxyz_dev, const double* t_ca_dev, size_t k, int64_t* chosen,
                                  double* sv_after, double* score_after, double* H_after, int32_t* n_chosen) {
  const char* who = "clc_select_board_poses_device";
  gd::GuideModel g;
  double M0[36];
  CLC_TRY(guidance_model(gopt, pose_cl, H0, who, &g, M0));
  if (k < 1 || k > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_select_board_poses_device: k must be in [1, 2^31)");
  if (!h || !chosen) return fail(CLC_ERR_INVALID_ARG, "clc_select_board_poses_device: bad argument");
  CLC_TRY(count_check(who, n_cand, q_ca_wxyz_dev, t_ca_dev));
  if (n_cand == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  return select_on_device(st, who, g, M0, n_cand, q_ca_wxyz_dev, t_ca_dev, k, chosen, sv_after, score_after, H_after, n_chosen);
}

int clc_select_board_poses(clc_handle* h, const clc_guidance_options* gopt, const double pose_cl[7], const double* H0, size_t n_cand,
                           const double* q_ca_wxyz, const double* t_ca, size_t k, int64_t* chosen, double* sv_after,
                           double* score_after, double* H_after, int32_t* n_chosen) {
  const char* who = "clc_select_board_poses";
  gd::GuideModel g;
  double M0[36];
  CLC_TRY(guidance_model(gopt, pose_cl, H0, who, &g, M0));
  if (k < 1 || k > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_select_board_poses: k must be in [1, 2^31)");
  if (!h || !chosen) return fail(CLC_ERR_INVALID_ARG, "clc_select_board_poses: bad argument");
  CLC_TRY(count_check(who, n_cand, q_ca_wxyz, t_ca));
  if (n_cand == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  const double* q_dev = st.in(q_ca_wxyz, 4 * n_cand);
  const double* t_dev = st.in(t_ca, 3 * n_cand);
  return select_on_device(st, who, g, M0, n_cand, q_dev, t_dev, k, chosen, sv_after, score_after, H_after, n_chosen);
}

}  // extern "C"

#ifdef CLC_TEST_HOOKS
// Test / profiling hooks, process-wide.  1 = the ray directions from the table (the product's path), 0 = a sincos per ray.
#pragma GCC visibility push(default)
extern "C" int clc_debug_guidance_dirs(int table) {
  g_dir_table.store(table ? 1 : 0, std::memory_order_relaxed);
  return CLC_OK;
}
// 1 = clc_score_board_poses(_device) scores with one wave per candidate and one matrix row per lane (the mapping not chosen).
extern "C" int clc_debug_guidance_score_rows(int rows) {
  g_score_rows.store(rows ? 1 : 0, std::memory_order_relaxed);
  return CLC_OK;
}
#pragma GCC visibility pop
#endif
