// abi_guidance.hip — clc_guidance_options_default, clc_score_board_poses(_device), clc_select_board_poses(_device): pose guidance
// (K20 in clc_guidance.hpp).  A unit of its own, held to its own register figures (tests/test_guidance_resources.py).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
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
hipError_t enqueue_cast(clc_handle* h, const gd::GuideModel& g, double* dirs, const double* q, const double* t, size_t n, int32_t* n_hits,
                        double* H_add) {
  gd::CastArgs a{};
  a.g = g; a.dirs = dirs; a.q = q; a.t = t; a.n_cand = (long long)n; a.n_hits = n_hits; a.H_add = H_add;
  const unsigned blocks = (unsigned)((n + gd::CAST_WAVES - 1) / gd::CAST_WAVES);
#ifdef CLC_TEST_HOOKS
  if (!g_dir_table.load(std::memory_order_relaxed)) {
    hipLaunchKernelGGL(gd::guidance_cast_kernel<false>, dim3(blocks), dim3(gd::CAST_THREADS), 0, h->stream, a);
    return hipGetLastError();
  }
#endif
  hipLaunchKernelGGL(gd::guidance_dirs_kernel, dim3((unsigned)((g.n_rays + 255) / 256)), dim3(256), 0, h->stream, g, dirs);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gd::guidance_cast_kernel<true>, dim3(blocks), dim3(gd::CAST_THREADS), 0, h->stream, a);
  return hipGetLastError();
}

unsigned score_blocks(size_t n) { return (unsigned)((n + gd::SCORE_THREADS - 1) / gd::SCORE_THREADS); }

// Cast and score with the candidates and the outputs (every one nullable) in device memory; no synchronisation.  The buffers of the
// outputs the caller does not take live until the caller's synchronisation: ws owns them.
struct ScoreScratch {
  DevBuf<double> dirs, M, H_add;
  DevBuf<int32_t> n_hits;
  explicit ScoreScratch(DevPool* p) : dirs(p), M(p), H_add(p), n_hits(p) {}
};
int enqueue_score(clc_handle* h, const gd::GuideModel& g, const double* M0, size_t n, const double* q, const double* t, int32_t* n_hits,
                  double* H_add, double* sv, double* score, ScoreScratch& ws) {
  CLC_HIP(ws.dirs.alloc(2 * (size_t)g.n_rays));
  if (!n_hits) { CLC_HIP(ws.n_hits.alloc(n)); n_hits = ws.n_hits.p; }
  if (!H_add) { CLC_HIP(ws.H_add.alloc(36 * n)); H_add = ws.H_add.p; }
  CLC_HIP(enqueue_cast(h, g, ws.dirs.p, q, t, n, n_hits, H_add));
  if (!sv && !score) return CLC_OK;
  CLC_HIP(ws.M.alloc(36));
  CLC_HIP(hipMemcpyAsync(ws.M.p, M0, 36 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  gd::ScoreArgs s{};
  s.criterion = g.criterion; s.min_points = g.min_points; s.eig_floor = g.eig_floor;
  s.M = ws.M.p; s.H_add = H_add; s.n_hits = n_hits; s.n_cand = (long long)n; s.sv = sv; s.score = score;
#ifdef CLC_TEST_HOOKS
  if (g_score_rows.load(std::memory_order_relaxed)) {
    hipLaunchKernelGGL(gd::guidance_score_rows_kernel, dim3((unsigned)((n + gd::CAST_WAVES - 1) / gd::CAST_WAVES)), dim3(gd::CAST_THREADS), 0,
                       h->stream, s);
    CLC_HIP(hipGetLastError());
    return CLC_OK;
  }
#endif
  hipLaunchKernelGGL(gd::guidance_score_kernel<false>, dim3(score_blocks(n)), dim3(gd::SCORE_THREADS), 0, h->stream, s);
  CLC_HIP(hipGetLastError());
  return CLC_OK;
}

// The greedy choice with the candidates in device memory: the cast once, `rounds` rounds back to back, the small results to the host
// arrays, one synchronisation.
int select_device(clc_handle* h, const gd::GuideModel& g, const double* M0, size_t n, const double* q, const double* t, size_t k,
                  int64_t* chosen, double* sv_after, double* score_after, double* H_after, int32_t* n_chosen) {
  const size_t rounds = std::min(k, n);
  const unsigned blocks = score_blocks(n);
  DevBuf<double> dirs(&h->pool), M(&h->pool), H_add(&h->pool), sv(&h->pool), score(&h->pool), best_s(&h->pool), sva(&h->pool), sca(&h->pool);
  DevBuf<int32_t> n_hits(&h->pool);
  DevBuf<unsigned char> taken(&h->pool);
  DevBuf<long long> best_i(&h->pool), ch(&h->pool);
  CLC_HIP(dirs.alloc(2 * (size_t)g.n_rays)); CLC_HIP(M.alloc(36)); CLC_HIP(H_add.alloc(36 * n)); CLC_HIP(sv.alloc(6 * n));
  CLC_HIP(score.alloc(n)); CLC_HIP(best_s.alloc(blocks)); CLC_HIP(best_i.alloc(blocks)); CLC_HIP(n_hits.alloc(n)); CLC_HIP(taken.alloc(n));
  CLC_HIP(ch.alloc(rounds)); CLC_HIP(sva.alloc(6 * rounds)); CLC_HIP(sca.alloc(rounds));
  CLC_HIP(hipMemcpyAsync(M.p, M0, 36 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemsetAsync(taken.p, 0, n, h->stream));
  CLC_HIP(enqueue_cast(h, g, dirs.p, q, t, n, n_hits.p, H_add.p));
  gd::ScoreArgs s{};
  s.criterion = g.criterion; s.min_points = g.min_points; s.eig_floor = g.eig_floor;
  s.M = M.p; s.H_add = H_add.p; s.n_hits = n_hits.p; s.n_cand = (long long)n; s.sv = sv.p; s.score = score.p;
  s.taken = taken.p; s.best_score = best_s.p; s.best_index = best_i.p;
  gd::PickArgs p{};
  p.n_blocks = (long long)blocks; p.best_score = best_s.p; p.best_index = best_i.p; p.H_add = H_add.p; p.sv = sv.p; p.score = score.p;
  p.M = M.p; p.taken = taken.p; p.chosen = ch.p; p.sv_after = sva.p; p.score_after = sca.p;
  for (size_t r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(gd::guidance_score_kernel<true>, dim3(blocks), dim3(gd::SCORE_THREADS), 0, h->stream, s);
    CLC_HIP(hipGetLastError());
    p.round = (int)r;
    hipLaunchKernelGGL(gd::guidance_pick_kernel, dim3(1), dim3(gd::PICK_THREADS), 0, h->stream, p);
    CLC_HIP(hipGetLastError());
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "index type");
  CLC_HIP(hipMemcpyAsync(chosen, ch.p, rounds * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  if (sv_after) CLC_HIP(hipMemcpyAsync(sv_after, sva.p, 6 * rounds * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (score_after) CLC_HIP(hipMemcpyAsync(score_after, sca.p, rounds * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (H_after) CLC_HIP(hipMemcpyAsync(H_after, M.p, 36 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
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
  ScoreScratch ws(&h->pool);
  CLC_TRY(enqueue_score(h, g, M0, n_cand, q_ca_wxyz_dev, t_ca_dev, n_hits_dev, H_add_dev, sv_dev, score_dev, ws));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
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
  DevBuf<double> bq(&h->pool), bt(&h->pool), bH(&h->pool), bsv(&h->pool), bsc(&h->pool);
  DevBuf<int32_t> bn(&h->pool);
  CLC_HIP(bq.alloc(4 * n)); CLC_HIP(bt.alloc(3 * n));
  if (n_hits) CLC_HIP(bn.alloc(n));
  if (H_add) CLC_HIP(bH.alloc(36 * n));
  if (sv) CLC_HIP(bsv.alloc(6 * n));
  if (score) CLC_HIP(bsc.alloc(n));
  CLC_HIP(hipMemcpyAsync(bq.p, q_ca_wxyz, 4 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(bt.p, t_ca, 3 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  ScoreScratch ws(&h->pool);
  CLC_TRY(enqueue_score(h, g, M0, n, bq.p, bt.p, n_hits ? bn.p : nullptr, H_add ? bH.p : nullptr, sv ? bsv.p : nullptr,
                        score ? bsc.p : nullptr, ws));
  if (n_hits) CLC_HIP(hipMemcpyAsync(n_hits, bn.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (H_add) CLC_HIP(hipMemcpyAsync(H_add, bH.p, 36 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (sv) CLC_HIP(hipMemcpyAsync(sv, bsv.p, 6 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (score) CLC_HIP(hipMemcpyAsync(score, bsc.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
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
  return select_device(h, g, M0, n_cand, q_ca_wxyz_dev, t_ca_dev, k, chosen, sv_after, score_after, H_after, n_chosen);
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
  DevBuf<double> bq(&h->pool), bt(&h->pool);
  CLC_HIP(bq.alloc(4 * n_cand)); CLC_HIP(bt.alloc(3 * n_cand));
  CLC_HIP(hipMemcpyAsync(bq.p, q_ca_wxyz, 4 * n_cand * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(bt.p, t_ca, 3 * n_cand * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return select_device(h, g, M0, n_cand, bq.p, bt.p, k, chosen, sv_after, score_after, H_after, n_chosen);
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
