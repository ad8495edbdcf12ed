// abi_jointrobust.hip — clc_joint_loss_options_default, clc_joint_refine_robust(_device): the joint refinement of the board poses and
// the camera-laser extrinsic under a Cauchy loss per corner and per laser point, with the per-observation weights (K22 in
// clc_jointrobust.hpp).  A unit of its own: joint_robust_kernel is held to its own register figures
// (tests/test_jointrobust_resources.py), and abi_joint.hip keeps K18's.
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include <limits>

#include "abi_jointcall.hpp"
#include "abi_lift.hpp"
#include "clc_jointrobust.hpp"

using namespace clc_abi;

namespace {

namespace jr = clc::jr;

// The refusals both forms make first, in clc_joint_refine's order and with its messages: the camera, the solve options, the joint
// options, then the loss options (the caller's or the defaults).
int robust_checks(const char* who, const clc_camera* cam, const clc_options* opt_in, const clc_joint_options* jopt_in,
                  const clc_joint_loss_options* lopt_in, clc_options* opt, clc_joint_options* jo, clc_joint_loss_options* lo) {
  CLC_TRY(camera_check(cam, who));
  CLC_TRY(pose_options(opt_in, opt, who));
  if (jopt_in) *jo = *jopt_in; else clc_joint_options_default(jo, cam);
  CLC_TRY(check_sigmas_and_holds(who, true, jo->sigma_corner, jo->sigma_laser, jo->hold_board_poses, jo->hold_extrinsic));
  if (lopt_in) *lo = *lopt_in; else clc_joint_loss_options_default(lo, jo);
  return check_loss_scales(who, lo->loss_corner, lo->loss_laser);
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
  const JointArrays c{corners_px, board_xy, corner_offsets, pts, pts_offsets, keep, n_images, problem_offsets, n_problems, q_ca_wxyz, t_ca,
                      poses_cl, summaries, H_cl, cost_parts, image_status};
  std::vector<long long> crel, prel;
  size_t M = 0, N = 0;
  CLC_TRY(joint_host_checks(who, h, c, &crel, &prel, &M, &N));
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = Clock::now();
  const std::vector<int32_t> not_kept(n_images, CLC_JOINT_NOT_KEPT);  // the status of the images outside every problem
  // ... and their weights: NaN, as for every image that takes no part
  const std::vector<double> no_weight(std::max((w_corner && M > 0) ? M : 0, (w_laser && N > 0) ? N : 0), std::numeric_limits<double>::quiet_NaN());
  Staging st(h);
  jr::RobustArgs a{};
  const float* corners_dev = stage_joint_arrays(st, c, crel, prel, M, N, not_kept.data(), a);
  a.w_corner = (w_corner && M > 0) ? st.inout(w_corner + corner_offsets[0], M, no_weight.data()) : nullptr;
  a.w_laser = (w_laser && N > 0) ? st.inout(w_laser + pts_offsets[0], N, no_weight.data()) : nullptr;
  enqueue_robust(st, *cam, opt, jo, lo, corners_dev, a, n_problems);
  CLC_TRY(st.finish(who));
  stamp_solve_ms(summaries, n_problems, t0);
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
  const JointArrays c{corners_px_dev, board_xy_dev, corner_offsets_dev, pts_dev, pts_offsets_dev, keep_dev, n_images, problem_offsets_dev,
                      n_problems, q_ca_wxyz_dev, t_ca_dev, poses_cl_dev, summaries_dev, H_cl_dev, cost_parts_dev, image_status_dev};
  CLC_TRY(joint_device_checks(who, h, c));
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  jr::RobustArgs a{};
  name_joint_arrays(c, a);
  a.w_corner = w_corner_dev;
  a.w_laser = w_laser_dev;
  // the image and corner ranges, to size the lifted corners and the workspace
  CLC_TRY(read_joint_ends(h, who, jr::joint_ends_kernel<>, n_images > 0, n_images, corners_px_dev, a));
  Staging st(h);
  enqueue_robust(st, *cam, opt, jo, lo, corners_px_dev, a, n_problems);
  return st.finish(who);
}

}  // extern "C"
