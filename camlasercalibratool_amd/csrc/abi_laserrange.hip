// abi_laserrange.hip — clc_range_options_default, clc_joint_refine_range(_device), clc_range_correct(_device): the joint refinement
// with the scanner's range offset and scale (K21 in clc_laserrange.hpp).  A unit of its own: range_refine_kernel is held to its own
// register figures (tests/test_laserrange_resources.py).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_jointcall.hpp"
#include "abi_lift.hpp"
#include "clc_laserrange.hpp"

using namespace clc_abi;

namespace {

namespace lr = clc::lr;

// The call's options: the caller's or the defaults; checked.
int range_options(const clc_range_options* in, const clc_camera* cam, clc_range_options* o, const char* who) {
  if (in) *o = *in; else clc_range_options_default(o, cam);
  // (with the board poses held the corners take no part and their sigma goes unchecked)
  CLC_TRY(check_sigmas_and_holds(who, !o->hold_board_poses, o->sigma_corner, o->sigma_laser, o->hold_board_poses, o->hold_extrinsic));
  CLC_TRY(check_range_mask(who, o->hold_range_mask));
  if (o->reserved != 0) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": reserved must be 0").c_str());
  return CLC_OK;
}

// The refusals both forms make first, in the same order: the options, then the camera where the corners are read.
int range_checks(const char* who, const clc_camera* cam, const clc_options* opt_in, const clc_range_options* ropt_in, clc_options* opt,
                 clc_range_options* ro) {
  CLC_TRY(pose_options(opt_in, opt, who));
  CLC_TRY(range_options(ropt_in, cam, ro, who));
  if (!ro->hold_board_poses) CLC_TRY(camera_check(cam, who));
  return CLC_OK;
}

// K21 on device arrays, the one function under both forms (as enqueue_joint of abi_joint.hip).  With the board poses held no corner
// is read: no lift, and the corner arrays of `a` are NULL.
void enqueue_range(Staging& st, const clc_camera* cam, const clc_options& opt, const clc_range_options& ro, const float* corners_dev,
                   lr::RangeArgs a, size_t n_problems) {
  a.opt = opt;
  a.sigma_corner = ro.hold_board_poses ? 1.0 : ro.sigma_corner;
  a.sigma_laser = ro.sigma_laser;
  a.hold_board_poses = ro.hold_board_poses ? 1 : 0;
  a.hold_extrinsic = ro.hold_extrinsic ? 1 : 0;
  a.hold_range_mask = ro.hold_range_mask;
  if (a.hold_board_poses) {
    a.lifted = a.board = nullptr;
    a.coff = nullptr;
    a.first_corner = a.n_corners = 0;
  } else {
    a.lifted = enqueue_lift(st, *cam, corners_dev, a.first_corner, (size_t)a.n_corners);
  }
  a.ws = st.scratch<lr::RangeImage>((size_t)a.n_images);
  if (!st.ok()) return;
  hipLaunchKernelGGL(lr::range_refine_kernel, dim3((unsigned)n_problems), dim3(lr::RANGE_THREADS), 0, st.stream(), a);
  st.launched();
}

// The point correction on device arrays.
void enqueue_correct(Staging& st, const double range[2], const double* pts_dev, size_t n, double* out_dev) {
  if (!st.ok() || n == 0) return;
  const size_t blocks = (n + lr::CORRECT_THREADS - 1) / lr::CORRECT_THREADS;
  hipLaunchKernelGGL(lr::range_correct_kernel, dim3((unsigned)std::min<size_t>(blocks, 65536)), dim3(lr::CORRECT_THREADS), 0, st.stream(),
                     pts_dev, (long long)n, range[0], range[1], out_dev);
  st.launched();
}

int correct_checks(const char* who, clc_handle* h, const double* range, const double* pts, size_t n, double* out) {
  const std::string w(who);
  if (!h || !range || (n > 0 && (!pts || !out)) || n > (size_t)0x7FFFFFFFFFFFFFFFll / 24) return fail(CLC_ERR_INVALID_ARG, (w + ": bad argument").c_str());
  if (!std::isfinite(range[0]) || !std::isfinite(range[1])) return fail(CLC_ERR_NONFINITE, (w + ": non-finite range parameter").c_str());
  return CLC_OK;
}

}  // namespace

extern "C" {

void clc_range_options_default(clc_range_options* o, const clc_camera* cam) {
  if (!o) return;
  clc_joint_options jo;
  clc_joint_options_default(&jo, cam);
  o->sigma_corner = jo.sigma_corner;
  o->sigma_laser = jo.sigma_laser;
  o->hold_board_poses = 0;
  o->hold_extrinsic = 0;
  o->hold_range_mask = 0;
  o->reserved = 0;
}

int clc_joint_refine_range(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_range_options* ropt_in,
                           const float* corners_px, const float* board_xy, const int64_t* corner_offsets, const double* pts,
                           const int64_t* pts_offsets, const uint8_t* keep, size_t n_images, const int64_t* problem_offsets,
                           size_t n_problems, double* q_ca_wxyz, double* t_ca, double* poses_cl, double* range, clc_summary* summaries,
                           double* H_cr, double* cost_parts, int32_t* image_status) {
  const char* who = "clc_joint_refine_range";
  // everything that can be refused without the device first
  clc_options opt;
  clc_range_options ro;
  CLC_TRY(range_checks(who, cam, opt_in, ropt_in, &opt, &ro));
  const bool corners = !ro.hold_board_poses;
  if ((n_images > 0 && ((corners && !corner_offsets) || !pts_offsets || !q_ca_wxyz || !t_ca || !image_status)) ||
      (n_problems > 0 && (!poses_cl || !range || !summaries)))
    return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_range: bad argument");
  CLC_TRY(problem_count_checks(who, n_images, problem_offsets != nullptr, n_problems));
  std::vector<long long> crel, prel;
  size_t M = 0, N = 0;
  if (corners) CLC_TRY(host_offsets(who, corner_offsets, n_images, true, nullptr, &crel, &M));
  CLC_TRY(host_offsets(who, pts_offsets, n_images, true, nullptr, &prel, &N));
  CLC_TRY(host_problem_offsets(who, problem_offsets, n_problems, n_images));
  if (!h || (M > 0 && (!corners_px || !board_xy)) || (N > 0 && !pts)) return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_range: bad argument");
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = Clock::now();
  const size_t n = n_images, np = n_problems;
  const size_t n_off = n > 0 ? n + 1 : 0;  // a call without images sends no offsets
  const std::vector<int32_t> not_kept(n, CLC_JOINT_NOT_KEPT);  // the status of the images outside every problem
  Staging st(h);
  lr::RangeArgs a{};  // the host arrays start at image 0 and, rebased, at corner 0 and point 0
  const float* corners_dev = nullptr;
  if (corners) {
    corners_dev = st.in(M > 0 ? corners_px + 2 * corner_offsets[0] : nullptr, 2 * M);
    a.board = st.in(M > 0 ? board_xy + 2 * corner_offsets[0] : nullptr, 2 * M);
    a.coff = st.in(crel.data(), n_off);
    a.n_corners = (long long)M;
  }
  a.pts = st.in(N > 0 ? pts + 3 * pts_offsets[0] : nullptr, 3 * N);
  a.poff = st.in(prel.data(), n_off);
  a.keep = st.in_opt(keep, n);
  a.prob_off = st.in_opt(reinterpret_cast<const long long*>(problem_offsets), np + 1);
  a.n_images = (long long)n;
  a.q = st.inout(q_ca_wxyz, 4 * n);
  a.t = st.inout(t_ca, 3 * n);
  a.status = st.inout(image_status, n, not_kept.data());
  a.poses_cl = st.inout(poses_cl, 7 * np);
  a.range = st.inout(range, 2 * np);
  a.summaries = st.out(summaries, np);
  a.H_cr = st.out_opt(H_cr, 64 * np);
  a.cost_parts = st.out_opt(cost_parts, 2 * np);
  enqueue_range(st, cam, opt, ro, corners_dev, a, np);
  CLC_TRY(st.finish(who));
  stamp_solve_ms(summaries, np, t0);
  return CLC_OK;
}

int clc_joint_refine_range_device(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_range_options* ropt_in,
                                  const float* corners_px_dev, const float* board_xy_dev, const int64_t* corner_offsets_dev,
                                  const double* pts_dev, const int64_t* pts_offsets_dev, const uint8_t* keep_dev, size_t n_images,
                                  const int64_t* problem_offsets_dev, size_t n_problems, double* q_ca_wxyz_dev, double* t_ca_dev,
                                  double* poses_cl_dev, double* range_dev, clc_summary* summaries_dev, double* H_cr_dev,
                                  double* cost_parts_dev, int32_t* image_status_dev) {
  const char* who = "clc_joint_refine_range_device";
  clc_options opt;
  clc_range_options ro;
  CLC_TRY(range_checks(who, cam, opt_in, ropt_in, &opt, &ro));
  const bool corners = !ro.hold_board_poses;
  if (!h || (n_images > 0 && ((corners && !corner_offsets_dev) || !pts_offsets_dev || !q_ca_wxyz_dev || !t_ca_dev || !image_status_dev)) ||
      (n_problems > 0 && (!poses_cl_dev || !range_dev || !summaries_dev)))
    return fail(CLC_ERR_INVALID_ARG, "clc_joint_refine_range_device: bad argument");
  CLC_TRY(problem_count_checks(who, n_images, problem_offsets_dev != nullptr, n_problems));
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  lr::RangeArgs a{};
  a.board = board_xy_dev;
  a.coff = corners ? reinterpret_cast<const long long*>(corner_offsets_dev) : nullptr;
  a.pts = pts_dev;
  a.poff = reinterpret_cast<const long long*>(pts_offsets_dev);
  a.keep = keep_dev;
  a.prob_off = reinterpret_cast<const long long*>(problem_offsets_dev);
  a.n_images = (long long)n_images;
  a.q = q_ca_wxyz_dev;
  a.t = t_ca_dev;
  a.status = image_status_dev;
  a.poses_cl = poses_cl_dev;
  a.range = range_dev;
  a.summaries = summaries_dev;
  a.H_cr = H_cr_dev;
  a.cost_parts = cost_parts_dev;
  // the image and corner ranges, to size the lifted corners and the workspace (nothing to read without corners and problem offsets)
  CLC_TRY(read_joint_ends(h, who, lr::joint_ends_kernel<>, n_images > 0 && (corners || a.prob_off), n_images, corners_px_dev, a));
  Staging st(h);
  enqueue_range(st, cam, opt, ro, corners_px_dev, a, n_problems);
  return st.finish(who);
}

int clc_range_correct(clc_handle* h, const double range[2], const double* pts, size_t n, double* out) {
  const char* who = "clc_range_correct";
  CLC_TRY(correct_checks(who, h, range, pts, n, out));
  if (n == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  const double* pts_dev = st.in(pts, 3 * n);
  double* out_dev = st.out(out, 3 * n);
  enqueue_correct(st, range, pts_dev, n, out_dev);
  return st.finish(who);
}

int clc_range_correct_device(clc_handle* h, const double range[2], const double* pts_dev, size_t n, double* out_dev) {
  const char* who = "clc_range_correct_device";
  CLC_TRY(correct_checks(who, h, range, pts_dev, n, out_dev));
  if (n == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  enqueue_correct(st, range, pts_dev, n, out_dev);
  return st.finish(who);
}

}  // extern "C"
