// abi_joint.hip — clc_joint_options_default, clc_joint_refine(_device): the joint refinement of the board poses and the camera-laser
// extrinsic (K18 in clc_joint.hpp).  A unit of its own: the kernels of abi_campose.hip are held to their register figures, and this
// one is held to its own (tests/test_joint_resources.py).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "abi_lift.hpp"
#include "clc_joint.hpp"

using namespace clc_abi;

namespace {

namespace jt = clc::jt;

// The joint call's options: the caller's or the defaults; checked.
int joint_options(const clc_joint_options* in, const clc_camera* cam, clc_joint_options* o, const char* who) {
  if (in) *o = *in; else clc_joint_options_default(o, cam);
  const std::string w(who);
  if (!(std::isfinite(o->sigma_corner) && o->sigma_corner > 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": sigma_corner must be finite and > 0").c_str());
  if (!(std::isfinite(o->sigma_laser) && o->sigma_laser > 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": sigma_laser must be finite and > 0").c_str());
  if (o->hold_board_poses && o->hold_extrinsic) return fail(CLC_ERR_INVALID_ARG, (w + ": both hold flags set").c_str());
  return CLC_OK;
}

// The refusals both forms make first, in the same order: the camera and the options.
int joint_checks(const char* who, const clc_camera* cam, const clc_options* opt_in, const clc_joint_options* jopt_in, clc_options* opt,
                 clc_joint_options* jo) {
  CLC_TRY(camera_check(cam, who));
  CLC_TRY(pose_options(opt_in, opt, who));
  return joint_options(jopt_in, cam, jo, who);
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
  if ((n_images > 0 && (!corner_offsets || !pts_offsets || !q_ca_wxyz || !t_ca || !image_status)) ||
      (n_problems > 0 && (!poses_cl || !summaries)))
    return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine: bad argument");
  CLC_TRY(problem_count_checks(who, n_images, problem_offsets != nullptr, n_problems));
  std::vector<long long> crel, prel;
  size_t M = 0, N = 0;
  CLC_TRY(host_offsets(who, corner_offsets, n_images, true, nullptr, &crel, &M));
  CLC_TRY(host_offsets(who, pts_offsets, n_images, true, nullptr, &prel, &N));
  CLC_TRY(host_problem_offsets(who, problem_offsets, n_problems, n_images));
  if (!h || (M > 0 && (!corners_px || !board_xy)) || (N > 0 && !pts)) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine: bad argument");
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = Clock::now();
  const size_t n = n_images, np = n_problems;
  const size_t n_off = n > 0 ? n + 1 : 0;  // a call without images sends no offsets
  const std::vector<int32_t> not_kept(n, CLC_JOINT_NOT_KEPT);  // the status of the images outside every problem
  Staging st(h);
  const float* corners_dev = st.in(M > 0 ? corners_px + 2 * corner_offsets[0] : nullptr, 2 * M);
  jt::JointArgs a{};  // the host arrays start at image 0 and, rebased, at corner 0 and point 0
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
  enqueue_joint(st, *cam, opt, jo, corners_dev, a, np);
  CLC_TRY(st.finish(who));
  stamp_solve_ms(summaries, np, t0);
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
  if (!h || (n_images > 0 && (!corner_offsets_dev || !pts_offsets_dev || !q_ca_wxyz_dev || !t_ca_dev || !image_status_dev)) ||
      (n_problems > 0 && (!poses_cl_dev || !summaries_dev)))
    return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_device: bad argument");
  CLC_TRY(problem_count_checks(who, n_images, problem_offsets_dev != nullptr, n_problems));
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  jt::JointArgs a{};
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
  // the image and corner ranges, to size the lifted corners and the workspace: one small read ahead of the enqueue (as
  // clc_board_poses_device reads the ends of its offsets)
  long long ends[3] = {0, 0, 0};
  if (n_images > 0) {
    Staging read(h);
    long long* ends_dev = read.out(ends, 3);
    if (read.ok()) {
      hipLaunchKernelGGL(jt::joint_ends_kernel, dim3(1), dim3(64), 0, read.stream(), a.prob_off, a.coff, (long long)n_images, ends_dev);
      read.launched();
    }
    CLC_TRY(read.finish(who));
  }
  if (ends[0] < 0 || ends[1] < 0 || ends[2] < ends[1]) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_device: offsets not monotone");
  a.first_image = ends[0];
  a.first_corner = ends[1];
  a.n_corners = ends[2] - ends[1];
  if (a.n_corners > 0 && (!corners_px_dev || !board_xy_dev)) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_device: bad argument");
  Staging st(h);
  enqueue_joint(st, *cam, opt, jo, corners_px_dev, a, n_problems);
  return st.finish(who);
}

}  // extern "C"
