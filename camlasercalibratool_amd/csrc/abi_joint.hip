// abi_joint.hip — clc_joint_options_default, clc_joint_refine(_device): the joint refinement of the board poses and the camera-laser
// extrinsic (K18 in clc_joint.hpp).  A unit of its own: the kernels of abi_campose.hip are held to their register figures, and this
// one is held to its own (tests/test_joint_resources.py).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_jointcall.hpp"
#include "abi_lift.hpp"
#include "clc_joint.hpp"

using namespace clc_abi;

namespace {

namespace jt = clc::jt;

// The refusals both forms make first, in the same order: the camera, the solve options, then the joint call's options (the caller's or
// the defaults).
int joint_checks(const char* who, const clc_camera* cam, const clc_options* opt_in, const clc_joint_options* jopt_in, clc_options* opt,
                 clc_joint_options* jo) {
  CLC_TRY(camera_check(cam, who));
  CLC_TRY(pose_options(opt_in, opt, who));
  if (jopt_in) *jo = *jopt_in; else clc_joint_options_default(jo, cam);
  return check_sigmas_and_holds(who, true, jo->sigma_corner, jo->sigma_laser, jo->hold_board_poses, jo->hold_extrinsic);
}

// K18 on device arrays, the one function under both forms.  `a` arrives with the call's arrays and ranges named by the form (the
// per-image arrays indexed by the absolute image index; the call covers a.n_images images from a.first_image on and a.n_corners
// corners from a.first_corner on); here it gets the options, the lifted corners and the per-image workspace, both scratch of the
// call.  The lift, then one workgroup per problem, on the handle's stream.
void enqueue_joint(Staging& st, const clc_camera& cam, const clc_options& opt, const clc_joint_options& jo, const float* corners_dev,
                   jt::JointArgs a, size_t n_problems) {
  a.opt = opt;
  a.sigma_corner = jo.sigma_corner;
  a.sigma_laser = jo.sigma_laser;
  a.hold_board_poses = jo.hold_board_poses ? 1 : 0;
  a.hold_extrinsic = jo.hold_extrinsic ? 1 : 0;
  a.lifted = enqueue_lift(st, cam, corners_dev, a.first_corner, (size_t)a.n_corners);
  a.ws = st.scratch<jt::JointImage>((size_t)a.n_images);
  if (!st.ok()) return;
  hipLaunchKernelGGL(jt::joint_refine_kernel, dim3((unsigned)n_problems), dim3(jt::JOINT_THREADS), 0, st.stream(), a);
  st.launched();
}

}  // namespace

extern "C" {

void clc_joint_options_default(clc_joint_options* o, const clc_camera* cam) {
  if (!o) return;
  // 0.3 px and 0.01 m: the noise levels of the project's simulations (simdata, tests/robustpose_cases.py)
  const double f = cam ? std::sqrt(std::fabs(cam->proj[0] * cam->proj[1])) : 0.0;
  o->sigma_corner = f > 0.0 ? 0.3 / f : 0.0;
  o->sigma_laser = 0.01;
  o->hold_board_poses = 0;
  o->hold_extrinsic = 0;
}

int clc_joint_refine(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_joint_options* jopt_in,
                     const float* corners_px, const float* board_xy, const int64_t* corner_offsets, const double* pts,
                     const int64_t* pts_offsets, const uint8_t* keep, size_t n_images, const int64_t* problem_offsets, size_t n_problems,
                     double* q_ca_wxyz, double* t_ca, double* poses_cl, clc_summary* summaries, double* H_cl, double* cost_parts,
                     int32_t* image_status) {
  const char* who = "clc_joint_refine";
  // everything that can be refused without the device first
  clc_options opt;
  clc_joint_options jo;
  CLC_TRY(joint_checks(who, cam, opt_in, jopt_in, &opt, &jo));
  const JointArrays c{corners_px, board_xy, corner_offsets, pts, pts_offsets, keep, n_images, problem_offsets, n_problems, q_ca_wxyz, t_ca,
                      poses_cl, summaries, H_cl, cost_parts, image_status};
  std::vector<long long> crel, prel;
  size_t M = 0, N = 0;
  CLC_TRY(joint_host_checks(who, h, c, &crel, &prel, &M, &N));
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = Clock::now();
  const std::vector<int32_t> not_kept(n_images, CLC_JOINT_NOT_KEPT);  // the status of the images outside every problem
  Staging st(h);
  jt::JointArgs a{};
  const float* corners_dev = stage_joint_arrays(st, c, crel, prel, M, N, not_kept.data(), a);
  enqueue_joint(st, *cam, opt, jo, corners_dev, a, n_problems);
  CLC_TRY(st.finish(who));
  stamp_solve_ms(summaries, n_problems, t0);
  return CLC_OK;
}

int clc_joint_refine_device(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_joint_options* jopt_in,
                            const float* corners_px_dev, const float* board_xy_dev, const int64_t* corner_offsets_dev,
                            const double* pts_dev, const int64_t* pts_offsets_dev, const uint8_t* keep_dev, size_t n_images,
                            const int64_t* problem_offsets_dev, size_t n_problems, double* q_ca_wxyz_dev, double* t_ca_dev,
                            double* poses_cl_dev, clc_summary* summaries_dev, double* H_cl_dev, double* cost_parts_dev,
                            int32_t* image_status_dev) {
  const char* who = "clc_joint_refine_device";
  clc_options opt;
  clc_joint_options jo;
  CLC_TRY(joint_checks(who, cam, opt_in, jopt_in, &opt, &jo));
  const JointArrays c{corners_px_dev, board_xy_dev, corner_offsets_dev, pts_dev, pts_offsets_dev, keep_dev, n_images, problem_offsets_dev,
                      n_problems, q_ca_wxyz_dev, t_ca_dev, poses_cl_dev, summaries_dev, H_cl_dev, cost_parts_dev, image_status_dev};
  CLC_TRY(joint_device_checks(who, h, c));
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  jt::JointArgs a{};
  name_joint_arrays(c, a);
  // the image and corner ranges, to size the lifted corners and the workspace
  CLC_TRY(read_joint_ends(h, who, jt::joint_ends_kernel<>, n_images > 0, n_images, corners_px_dev, a));
  Staging st(h);
  enqueue_joint(st, *cam, opt, jo, corners_px_dev, a, n_problems);
  return st.finish(who);
}

}  // extern "C"
