// abi_fullcal.hip — clc_full_options_default, clc_calibrate_full(_device): one robust cost over the camera's intrinsics, every board
// pose, T_cl and the scanner's range offset and scale, with the per-observation weights (K23 in clc_fullcal.hpp).  A unit of its
// own: fullcal_kernel is held to its own register figures (tests/test_fullcal_resources.py), and the units of K19, K21 and K22 keep
// theirs.
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include <limits>

#include "abi_jointcall.hpp"
#include "clc_fullcal.hpp"

using namespace clc_abi;

namespace {

namespace fc = clc::fc;

// Whether the corner terms take part: with the board poses and all 8 intrinsics held they are constant.
bool corners_take_part(const clc_full_options& o) { return !(o.hold_board_poses && o.hold_intrinsics_mask == 0xFFu); }

// The call's options: the caller's or the defaults for `model`; checked with the messages of K19, K21 and K22 for their share.
int full_options(const clc_full_options* in, int32_t model, clc_full_options* o, const char* who) {
  if (in) *o = *in; else clc_full_options_default(o, model);
  const std::string w(who);
  if (o->hold_intrinsics_mask > 0xFFu) return fail(CLC_ERR_INVALID_ARG, (w + ": hold_intrinsics_mask has bits beyond the 8 intrinsics").c_str());
  CLC_TRY(check_range_mask(who, o->hold_range_mask));
  if (corners_take_part(*o)) CLC_TRY(check_sigma(who, "sigma_px", o->sigma_px));  // (unchecked where the corners take no part)
  CLC_TRY(check_sigma(who, "sigma_laser", o->sigma_laser));
  CLC_TRY(check_loss_scales(who, o->loss_corner, o->loss_laser));
  if (o->hold_board_poses && o->hold_extrinsic && o->hold_range_mask == 3 && o->hold_intrinsics_mask == 0xFFu)
    return fail(CLC_ERR_INVALID_ARG, (w + ": everything is held").c_str());
  return CLC_OK;
}

// K23 on device arrays, the one function under both forms.  `a` arrives with the call's arrays named by the form and a.n_images, the
// images from the first problem's first image on; here it gets the options and the per-image workspace of n_images rows, scratch of
// the call.  One workgroup per problem for the solve, then — where the caller asked for weights — one per problem for the weights,
// on the handle's stream.
void enqueue_full(Staging& st, const clc_options& opt, const clc_full_options& fo, fc::FullArgs a, size_t n_images, size_t n_problems) {
  a.opt = opt;
  a.use_corners = corners_take_part(fo) ? 1 : 0;
  a.sigma_px = a.use_corners ? fo.sigma_px : 1.0;
  a.sigma_laser = fo.sigma_laser;
  a.loss_corner = fo.loss_corner;
  a.loss_laser = fo.loss_laser;
  a.hold_intrinsics_mask = fo.hold_intrinsics_mask;
  a.hold_range_mask = fo.hold_range_mask;
  a.hold_board_poses = fo.hold_board_poses ? 1 : 0;
  a.hold_extrinsic = fo.hold_extrinsic ? 1 : 0;
  if (!a.use_corners) {
    a.corners = a.board = nullptr;
    a.coff = nullptr;
    a.w_corner = nullptr;
  }
  a.ws = st.scratch<fc::FullImage>(n_images);
  if (!st.ok()) return;
  hipLaunchKernelGGL(fc::fullcal_kernel, dim3((unsigned)n_problems), dim3(fc::FULL_THREADS), 0, st.stream(), a);
  st.launched();
  if (!st.ok() || (!a.w_corner && !a.w_laser)) return;
  hipLaunchKernelGGL(fc::fullcal_weights_kernel, dim3((unsigned)n_problems), dim3(fc::FULL_THREADS), 0, st.stream(), a);
  st.launched();
}

}  // namespace

extern "C" {

void clc_full_options_default(clc_full_options* o, int32_t model) {
  if (!o) return;
  o->sigma_px = 0.3;  // the noise levels of the project's simulations
  o->sigma_laser = 0.01;
  o->loss_corner = 3.0;  // clc_joint_loss_options_default's at those sigmas
  o->loss_laser = 5.0;
  o->hold_intrinsics_mask = model == CLC_CAMERA_KANNALA_BRANDT ? (1u << 6) | (1u << 7) : 0u;
  o->hold_range_mask = 0;
  o->hold_board_poses = 0;
  o->hold_extrinsic = 0;
}

int clc_calibrate_full(clc_handle* h, clc_camera* cams, const clc_options* opt_in, const clc_full_options* fopt_in, const float* corners_px,
                       const float* board_xy, const int64_t* corner_offsets, const double* pts, const int64_t* pts_offsets,
                       const uint8_t* keep, size_t n_images, const int64_t* problem_offsets, size_t n_problems, double* q_ca_wxyz,
                       double* t_ca, double* poses_cl, double* range, clc_summary* summaries, double* H_full, double* cost_parts,
                       double* rms_px, int32_t* image_status, double* w_corner, double* w_laser) {
  const char* who = "clc_calibrate_full";
  // everything that can be refused without the device first
  clc_options opt;
  CLC_TRY(pose_options(opt_in, &opt, who));
  if (n_problems > 0 && !cams) return fail(CLC_ERR_INVALID_ARG, "clc_calibrate_full: bad argument");
  for (size_t k = 0; k < n_problems; ++k)
    if (!known_model(cams[k].model)) return fail(CLC_ERR_INVALID_ARG, "clc_calibrate_full: unknown camera model");
  clc_full_options fo;
  CLC_TRY(full_options(fopt_in, n_problems > 0 ? cams[0].model : CLC_CAMERA_PINHOLE, &fo, who));
  const bool corners = corners_take_part(fo);
  if ((n_images > 0 && ((corners && !corner_offsets) || !pts_offsets || !q_ca_wxyz || !t_ca || !image_status)) ||
      (n_problems > 0 && (!poses_cl || !range || !summaries)))
    return fail(CLC_ERR_INVALID_ARG, "clc_calibrate_full: bad argument");
  CLC_TRY(problem_count_checks(who, n_images, problem_offsets != nullptr, n_problems));
  std::vector<long long> crel, prel;
  size_t M = 0, N = 0;
  if (corners) CLC_TRY(host_offsets(who, corner_offsets, n_images, true, nullptr, &crel, &M));
  CLC_TRY(host_offsets(who, pts_offsets, n_images, true, nullptr, &prel, &N));
  CLC_TRY(host_problem_offsets(who, problem_offsets, n_problems, n_images));
  if (!h || (M > 0 && (!corners_px || !board_xy)) || (N > 0 && !pts)) return fail(CLC_ERR_INVALID_ARG, "clc_calibrate_full: bad argument");
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = Clock::now();
  const size_t n = n_images, np = n_problems;
  const size_t n_off = n > 0 ? n + 1 : 0;  // a call without images sends no offsets
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  const std::vector<int32_t> not_kept(n, CLC_JOINT_NOT_KEPT);  // the status of the images outside every problem
  // ... and their weights: NaN, as for every image that takes no part
  const std::vector<double> no_weight(std::max((w_corner && M > 0) ? M : 0, (w_laser && N > 0) ? N : 0), std::numeric_limits<double>::quiet_NaN());
  Staging st(h);
  fc::FullArgs a{};  // the host arrays start at image 0 and, rebased, at corner 0 and point 0
  if (corners) {
    a.corners = st.in(M > 0 ? corners_px + 2 * corner_offsets[0] : nullptr, 2 * M);
    a.board = st.in(M > 0 ? board_xy + 2 * corner_offsets[0] : nullptr, 2 * M);
    a.coff = st.in(crel.data(), n_off);
  }
  a.pts = st.in(N > 0 ? pts + 3 * pts_offsets[0] : nullptr, 3 * N);
  a.poff = st.in(prel.data(), n_off);
  a.keep = st.in_opt(keep, n);
  // the device indexes the per-image arrays by the absolute image index and the workspace from the first problem's first image:
  // the host arrays start at image 0, so the offsets go down as they are and the call covers [problem_offsets[0], n)
  a.prob_off = st.in_opt(reinterpret_cast<const long long*>(problem_offsets), np + 1);
  a.n_images = (long long)n - (problem_offsets ? (long long)problem_offsets[0] : 0);
  a.q = st.inout(q_ca_wxyz, 4 * n);
  a.t = st.inout(t_ca, 3 * n);
  a.status = st.inout(image_status, n, not_kept.data());
  a.cams = st.inout(cams, np);
  a.poses_cl = st.inout(poses_cl, 7 * np);
  a.range = st.inout(range, 2 * np);
  a.summaries = st.out(summaries, np);
  a.H_full = st.out_opt(H_full, 256 * np);
  a.cost_parts = st.out_opt(cost_parts, 2 * np);
  a.rms = st.out_opt(rms_px, np);
  a.w_corner = (corners && w_corner && M > 0) ? st.inout(w_corner + corner_offsets[0], M, no_weight.data()) : nullptr;
  a.w_laser = (w_laser && N > 0) ? st.inout(w_laser + pts_offsets[0], N, no_weight.data()) : nullptr;
  enqueue_full(st, opt, fo, a, n, np);
  CLC_TRY(st.finish(who));
  stamp_solve_ms(summaries, np, t0);
  return CLC_OK;
}

int clc_calibrate_full_device(clc_handle* h, clc_camera* cams_dev, const clc_options* opt_in, const clc_full_options* fopt_in,
                              const float* corners_px_dev, const float* board_xy_dev, const int64_t* corner_offsets_dev,
                              const double* pts_dev, const int64_t* pts_offsets_dev, const uint8_t* keep_dev, size_t n_images,
                              const int64_t* problem_offsets_dev, size_t n_problems, double* q_ca_wxyz_dev, double* t_ca_dev,
                              double* poses_cl_dev, double* range_dev, clc_summary* summaries_dev, double* H_full_dev,
                              double* cost_parts_dev, double* rms_px_dev, int32_t* image_status_dev, double* w_corner_dev,
                              double* w_laser_dev) {
  const char* who = "clc_calibrate_full_device";
  clc_options opt;
  CLC_TRY(pose_options(opt_in, &opt, who));
  clc_full_options fo;
  CLC_TRY(full_options(fopt_in, CLC_CAMERA_PINHOLE, &fo, who));
  const bool corners = corners_take_part(fo);
  if (!h || (n_images > 0 && ((corners && (!corner_offsets_dev || !corners_px_dev || !board_xy_dev)) || !pts_offsets_dev ||
                              !q_ca_wxyz_dev || !t_ca_dev || !image_status_dev)) ||
      (n_problems > 0 && (!cams_dev || !poses_cl_dev || !range_dev || !summaries_dev)))
    return fail(CLC_ERR_INVALID_ARG, "clc_calibrate_full_device: bad argument");
  CLC_TRY(problem_count_checks(who, n_images, problem_offsets_dev != nullptr, n_problems));
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  Staging st(h);
  fc::FullArgs a{};
  a.corners = corners_px_dev;
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
  a.cams = cams_dev;
  a.poses_cl = poses_cl_dev;
  a.range = range_dev;
  a.summaries = summaries_dev;
  a.H_full = H_full_dev;
  a.cost_parts = cost_parts_dev;
  a.rms = rms_px_dev;
  a.w_corner = w_corner_dev;
  a.w_laser = w_laser_dev;
  enqueue_full(st, opt, fo, a, n_images, n_problems);
  return st.finish(who);
}

}  // extern "C"
