// abi_jointrobust.hip — clc_joint_loss_options_default, clc_joint_refine_robust(_device): the joint refinement of the board poses and
// the camera-laser extrinsic under a Cauchy loss per corner and per laser point, with the per-observation weights (K22 in
// clc_jointrobust.hpp).  A unit of its own: joint_robust_kernel is held to its own register figures
// (tests/test_jointrobust_resources.py), and abi_joint.hip keeps K18's.
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include <limits>

#include "abi_drive.hpp"
#include "abi_lift.hpp"
#include "clc_jointrobust.hpp"

using namespace clc_abi;

namespace {

namespace jr = clc::jr;

// The call's options: the caller's or the defaults; checked with clc_joint_refine's rules and messages.
int robust_options(const clc_joint_options* in, const clc_joint_loss_options* lin, const clc_camera* cam, clc_joint_options* o,
                   clc_joint_loss_options* lo, const char* who) {
  if (in) *o = *in; else clc_joint_options_default(o, cam);
  const std::string w(who);
  if (!(std::isfinite(o->sigma_corner) && o->sigma_corner > 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": sigma_corner must be finite and > 0").c_str());
  if (!(std::isfinite(o->sigma_laser) && o->sigma_laser > 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": sigma_laser must be finite and > 0").c_str());
  if (o->hold_board_poses && o->hold_extrinsic) return fail(CLC_ERR_INVALID_ARG, (w + ": both hold flags set").c_str());
  if (lin) *lo = *lin; else clc_joint_loss_options_default(lo, o);
  if (!(std::isfinite(lo->loss_corner) && lo->loss_corner >= 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": loss_corner must be finite and >= 0").c_str());
  if (!(std::isfinite(lo->loss_laser) && lo->loss_laser >= 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": loss_laser must be finite and >= 0").c_str());
  return CLC_OK;
}

// The refusals both forms make first, in clc_joint_refine's order: the camera, the solve options, the joint and loss options.
int robust_checks(const char* who, const clc_camera* cam, const clc_options* opt_in, const clc_joint_options* jopt_in,
                  const clc_joint_loss_options* lopt_in, clc_options* opt, clc_joint_options* jo, clc_joint_loss_options* lo) {
  CLC_TRY(camera_check(cam, who));
  CLC_TRY(pose_options(opt_in, opt, who));
  return robust_options(jopt_in, lopt_in, cam, jo, lo, who);
}

// K22 on device arrays, the one function under both forms (as enqueue_joint of abi_joint.hip): the lift, one workgroup per problem
// for the solve, then — where the caller asked for weights — one workgroup per problem for the weights, on the handle's stream.
void enqueue_robust(Staging& st, const clc_camera& cam, const clc_options& opt, const clc_joint_options& jo, const clc_joint_loss_options& lo,
                    const float* corners_dev, jr::RobustArgs a, size_t n_problems) {
  a.opt = opt;
  a.sigma_corner = jo.sigma_corner;
  a.sigma_laser = jo.sigma_laser;
  a.loss_corner = lo.loss_corner;
  a.loss_laser = lo.loss_laser;
  a.hold_board_poses = jo.hold_board_poses ? 1 : 0;
  a.hold_extrinsic = jo.hold_extrinsic ? 1 : 0;
  a.lifted = enqueue_lift(st, cam, corners_dev, a.first_corner, (size_t)a.n_corners);
  a.ws = st.scratch<jr::RobustImage>((size_t)a.n_images);
  if (!st.ok()) return;
  hipLaunchKernelGGL(jr::joint_robust_kernel, dim3((unsigned)n_problems), dim3(jr::ROBUST_THREADS), 0, st.stream(), a);
  st.launched();
  if (!st.ok() || (!a.w_corner && !a.w_laser)) return;
  hipLaunchKernelGGL(jr::joint_weights_kernel, dim3((unsigned)n_problems), dim3(jr::ROBUST_THREADS), 0, st.stream(), a);
  st.launched();
}

}  // namespace

extern "C" {

void clc_joint_loss_options_default(clc_joint_loss_options* lo, const clc_joint_options* jopt) {
  if (!lo) return;
  // corners: a design value, 3 sigma (0.9 px at the default 0.3 px).  laser: the reference's CauchyLoss(0.05) in metres
  // (src/LaseCamCalCeres.cpp:249,286) over sigma_laser: 5 at the default 0.01 m.
  lo->loss_corner = 3.0;
  lo->loss_laser = (jopt && std::isfinite(jopt->sigma_laser) && jopt->sigma_laser > 0.0) ? 0.05 / jopt->sigma_laser : 5.0;
}

int clc_joint_refine_robust(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_joint_options* jopt_in,
                            const clc_joint_loss_options* lopt_in, const float* corners_px, const float* board_xy,
                            const int64_t* corner_offsets, const double* pts, const int64_t* pts_offsets, const uint8_t* keep,
                            size_t n_images, const int64_t* problem_offsets, size_t n_problems, double* q_ca_wxyz, double* t_ca,
                            double* poses_cl, clc_summary* summaries, double* H_cl, double* cost_parts, int32_t* image_status,
                            double* w_corner, double* w_laser) {
  const char* who = "clc_joint_refine_robust";
  // everything that can be refused without the device first
  clc_options opt;
  clc_joint_options jo;
  clc_joint_loss_options lo;
  CLC_TRY(robust_checks(who, cam, opt_in, jopt_in, lopt_in, &opt, &jo, &lo));
  if ((n_images > 0 && (!corner_offsets || !pts_offsets || !q_ca_wxyz || !t_ca || !image_status)) ||
      (n_problems > 0 && (!poses_cl || !summaries)))
    return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_robust: bad argument");
  CLC_TRY(problem_count_checks(who, n_images, problem_offsets != nullptr, n_problems));
  std::vector<long long> crel, prel;
  size_t M = 0, N = 0;
  CLC_TRY(host_offsets(who, corner_offsets, n_images, true, nullptr, &crel, &M));
  CLC_TRY(host_offsets(who, pts_offsets, n_images, true, nullptr, &prel, &N));
  CLC_TRY(host_problem_offsets(who, problem_offsets, n_problems, n_images));
  if (!h || (M > 0 && (!corners_px || !board_xy)) || (N > 0 && !pts)) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_robust: bad argument");
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = Clock::now();
  const size_t n = n_images, np = n_problems;
  const size_t n_off = n > 0 ? n + 1 : 0;  // a call without images sends no offsets
  const std::vector<int32_t> not_kept(n, CLC_JOINT_NOT_KEPT);  // the status of the images outside every problem
  // ... and their weights: NaN, as for every image that takes no part
  const std::vector<double> no_weight(std::max((w_corner && M > 0) ? M : 0, (w_laser && N > 0) ? N : 0), std::numeric_limits<double>::quiet_NaN());
  Staging st(h);
  const float* corners_dev = st.in(M > 0 ? corners_px + 2 * corner_offsets[0] : nullptr, 2 * M);
  jr::RobustArgs a{};  // the host arrays start at image 0 and, rebased, at corner 0 and point 0
  a.board = st.in(M > 0 ? board_xy + 2 * corner_offsets[0] : nullptr, 2 * M);
  a.coff = st.in(crel.data(), n_off);
  a.n_corners = (long long)M;
  a.pts = st.in(N > 0 ? pts + 3 * pts_offsets[0] : nullptr, 3 * N);
  a.poff = st.in(prel.data(), n_off);
  a.keep = st.in_opt(keep, n);
  a.prob_off = st.in_opt(reinterpret_cast<const long long*>(problem_offsets), np + 1);
  a.n_images = (long long)n;
  a.q = st.inout(q_ca_wxyz, 4 * n);
  a.t = st.inout(t_ca, 3 * n);
  a.status = st.inout(image_status, n, not_kept.data());
  a.poses_cl = st.inout(poses_cl, 7 * np);
  a.summaries = st.out(summaries, np);
  a.H_cl = st.out_opt(H_cl, 36 * np);
  a.cost_parts = st.out_opt(cost_parts, 2 * np);
  a.w_corner = (w_corner && M > 0) ? st.inout(w_corner + corner_offsets[0], M, no_weight.data()) : nullptr;
  a.w_laser = (w_laser && N > 0) ? st.inout(w_laser + pts_offsets[0], N, no_weight.data()) : nullptr;
  enqueue_robust(st, *cam, opt, jo, lo, corners_dev, a, np);
  CLC_TRY(st.finish(who));
  stamp_solve_ms(summaries, np, t0);
  return CLC_OK;
}

int clc_joint_refine_robust_device(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_joint_options* jopt_in,
                                   const clc_joint_loss_options* lopt_in, const float* corners_px_dev, const float* board_xy_dev,
                                   const int64_t* corner_offsets_dev, const double* pts_dev, const int64_t* pts_offsets_dev,
                                   const uint8_t* keep_dev, size_t n_images, const int64_t* problem_offsets_dev, size_t n_problems,
                                   double* q_ca_wxyz_dev, double* t_ca_dev, double* poses_cl_dev, clc_summary* summaries_dev,
                                   double* H_cl_dev, double* cost_parts_dev, int32_t* image_status_dev, double* w_corner_dev,
                                   double* w_laser_dev) {
  const char* who = "clc_joint_refine_robust_device";
  clc_options opt;
  clc_joint_options jo;
  clc_joint_loss_options lo;
  CLC_TRY(robust_checks(who, cam, opt_in, jopt_in, lopt_in, &opt, &jo, &lo));
  if (!h || (n_images > 0 && (!corner_offsets_dev || !pts_offsets_dev || !q_ca_wxyz_dev || !t_ca_dev || !image_status_dev)) ||
      (n_problems > 0 && (!poses_cl_dev || !summaries_dev)))
    return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_robust_device: bad argument");
  CLC_TRY(problem_count_checks(who, n_images, problem_offsets_dev != nullptr, n_problems));
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  jr::RobustArgs a{};
  a.board = board_xy_dev;
  a.coff = reinterpret_cast<const long long*>(corner_offsets_dev);
  a.pts = pts_dev;
  a.poff = reinterpret_cast<const long long*>(pts_offsets_dev);
  a.keep = keep_dev;
  a.prob_off = reinterpret_cast<const long long*>(problem_offsets_dev);
  a.n_images = (long long)n_images;
  a.q = q_ca_wxyz_dev;
  a.t = t_ca_dev;
  a.status = image_status_dev;
  a.poses_cl = poses_cl_dev;
  a.summaries = summaries_dev;
  a.H_cl = H_cl_dev;
  a.cost_parts = cost_parts_dev;
  a.w_corner = w_corner_dev;
  a.w_laser = w_laser_dev;
  // the image and corner ranges, to size the lifted corners and the workspace: one small read ahead of the enqueue (as
  // clc_joint_refine_device)
  long long ends[3] = {0, 0, 0};
  if (n_images > 0) {
    Staging read(h);
    long long* ends_dev = read.out(ends, 3);
    if (read.ok()) {
      hipLaunchKernelGGL(jr::robust_ends_kernel, dim3(1), dim3(64), 0, read.stream(), a.prob_off, a.coff, (long long)n_images, ends_dev);
      read.launched();
    }
    CLC_TRY(read.finish(who));
  }
  if (ends[0] < 0 || ends[1] < 0 || ends[2] < ends[1]) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_robust_device: offsets not monotone");
  a.first_image = ends[0];
  a.first_corner = ends[1];
  a.n_corners = ends[2] - ends[1];
  if (a.n_corners > 0 && (!corners_px_dev || !board_xy_dev)) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_robust_device: bad argument");
  Staging st(h);
  enqueue_robust(st, *cam, opt, jo, lo, corners_px_dev, a, n_problems);
  return st.finish(who);
}

}  // extern "C"
