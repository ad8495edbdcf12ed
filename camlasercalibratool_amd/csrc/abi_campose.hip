// abi_campose.hip — clc_camera_lift, clc_camera_project, clc_board_poses(_device): the camera models and the batched planar PnP
// (K10 in clc_campose.hpp); clc_board_poses_robust(_device): the per-tag consensus ahead of it (K16 in clc_robustpose.hpp);
// clc_board_poses_alternate(_device): the planar fit's second minimum (K17 in clc_altpose.hpp).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "abi_lift.hpp"
#include "clc_campose.hpp"
#include "clc_robustpose.hpp"
#include "clc_altpose.hpp"

using namespace clc_abi;

namespace {

// What every board-pose call works on, in device memory: the images' corner ranges off[n_images + 1] inside px / board, of which
// the call covers the corners [first, first + n_corners).
struct Corners {
  const float *px, *board;
  const long long* off;
  long long first;
  size_t n_corners, n_images;
};

// The host arrays of a call up: the corners and board points from offsets[0] on and the rebased offsets (host_offsets), so first = 0.
Corners upload_corners(Staging& st, const float* corners_px, const float* board_xy, const int64_t* offsets, const std::vector<long long>& rel,
                       size_t n_corners) {
  const long long first = n_corners > 0 ? (long long)offsets[0] : 0;  // (the arrays may be NULL when there is no corner)
  const float* px = st.in(n_corners > 0 ? corners_px + 2 * first : nullptr, 2 * n_corners);
  const float* board = st.in(n_corners > 0 ? board_xy + 2 * first : nullptr, 2 * n_corners);
  return {px, board, st.in(rel.data(), rel.size()), 0, n_corners, rel.size() - 1};
}

// (the corner range of a _device call: device_offset_ends of abi_drive.hpp; the lifted corners go to a scratch array of that size)
Corners device_corners(const float* corners_px_dev, const float* board_xy_dev, const int64_t* offsets_dev, const long long ends[2], size_t n_images) {
  return {corners_px_dev, board_xy_dev, reinterpret_cast<const long long*>(offsets_dev), ends[0], (size_t)(ends[1] - ends[0]), n_images};
}

// K10 on device arrays: the lift, then one wave per image.
void enqueue_board_poses(Staging& st, const clc_camera& cam, const clc_options& opt, const Corners& c, double* q_dev, double* t_dev,
                         double* rms_dev, int32_t* status_dev, clc_summary* sum_dev) {
  const float* lifted = enqueue_lift(st, cam, c.px, c.first, c.n_corners);
  if (!st.ok()) return;
  hipLaunchKernelGGL(clc::cp::board_pose_kernel, dim3((unsigned)c.n_images), dim3(64), 0, st.stream(), opt, lifted, c.board, c.off, c.first,
                     q_dev, t_dev, rms_dev, status_dev, sum_dev);
  st.launched();
}

// The checks that clc_board_poses and its _device form make in the same order, up to the empty call.
int board_pose_checks(const char* who, const clc_handle* h, bool required, const clc_camera* cam, const clc_options* opt_in, size_t n_images,
                      clc_options* opt) {
  const std::string w(who);
  if (!h || (n_images > 0 && !required)) return fail(CLC_ERR_INVALID_ARG, (w + ": bad argument").c_str());
  CLC_TRY(camera_check(cam, who));
  CLC_TRY(pose_options(opt_in, opt, who));
  if (n_images > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, (w + ": too many images").c_str());
  return CLC_OK;
}
// The robust and the alternate calls check their options first (those refusals need no device), then the handle and the counts.
int count_checks(const char* who, const clc_handle* h, bool required, size_t n_images) {
  const std::string w(who);
  if (!h || (n_images > 0 && !required)) return fail(CLC_ERR_INVALID_ARG, (w + ": bad argument").c_str());
  if (n_images > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, (w + ": too many images").c_str());
  return CLC_OK;
}

// The robust call's options: the caller's or the defaults; checked.
int robust_options(const clc_robust_pose_options* in, const clc_camera* cam, clc_robust_pose_options* o, const char* who) {
  if (in) *o = *in; else clc_robust_pose_options_default(o, cam);
  const std::string w(who);
  if (!(std::isfinite(o->hyp_threshold) && o->hyp_threshold > 0.0 && std::isfinite(o->threshold) && o->threshold > 0.0))
    return fail(CLC_ERR_INVALID_ARG, (w + ": the gates must be finite and > 0").c_str());
  if (o->hyp_threshold < o->threshold) return fail(CLC_ERR_INVALID_ARG, (w + ": hyp_threshold < threshold").c_str());
  if (o->min_inliers < 4) return fail(CLC_ERR_INVALID_ARG, (w + ": min_inliers < 4").c_str());
  if (o->max_fits < 1 || o->max_fits > 8) return fail(CLC_ERR_INVALID_ARG, (w + ": max_fits outside 1..8").c_str());
  return CLC_OK;
}

// Every refusal of clc_board_poses_robust and its _device form up to the empty call: the options first (they need no device).
int robust_checks(const char* who, const clc_handle* h, bool required, const clc_camera* cam, const clc_options* opt_in,
                  const clc_robust_pose_options* ropt_in, size_t n_images, clc_options* opt, clc_robust_pose_options* ro) {
  CLC_TRY(camera_check(cam, who));
  CLC_TRY(pose_options(opt_in, opt, who));
  CLC_TRY(robust_options(ropt_in, cam, ro, who));
  return count_checks(who, h, required, n_images);
}

// What the robust call leaves per image, every array on the device (mask indexed by the absolute offsets; rms, summaries, best_group
// nullable).
struct RobustOut {
  double *q, *t, *rms;
  int32_t* status;
  clc_summary* summaries;
  unsigned char* mask;
  int32_t *n_inliers, *best_group, *n_fits;
};

// K16 on device arrays: lift -> consensus -> (fit -> re-gate) x max_fits on the handle's stream, every launch sized by n_images, no
// read-back in between.  The counts are needed whether or not the caller takes them: o.n_inliers / o.n_fits NULL -> scratch.
void enqueue_board_poses_robust(Staging& st, const clc_camera& cam, const clc_options& opt, const clc_robust_pose_options& ro,
                                const Corners& c, RobustOut o) {
  namespace rp = clc::rp;
  const float* lifted = enqueue_lift(st, cam, c.px, c.first, c.n_corners);
  float* sub_l = st.scratch<float>(2 * c.n_corners);  // indexed like lifted: corner `first` first
  float* sub_b = st.scratch<float>(2 * c.n_corners);
  int32_t* flag = st.scratch<int32_t>(c.n_images);
  if (!o.n_inliers) o.n_inliers = st.scratch<int32_t>(c.n_images);
  if (!o.n_fits) o.n_fits = st.scratch<int32_t>(c.n_images);
  if (!st.ok()) return;
  const dim3 grid((unsigned)c.n_images), block(64);
  hipLaunchKernelGGL(rp::tag_consensus_kernel, grid, block, 0, st.stream(), lifted, c.board, c.off, c.first, ro.hyp_threshold,
                     (int)ro.min_inliers, o.mask, sub_l, sub_b, o.n_inliers, flag, o.n_fits, o.best_group, o.q, o.t, o.rms, o.status,
                     o.summaries);
  st.launched();
  for (int round = 0; round < ro.max_fits && st.ok(); ++round) {
    hipLaunchKernelGGL(rp::board_pose_subset_kernel, grid, block, 0, st.stream(), opt, sub_l, sub_b, c.off, c.first, flag, o.n_inliers,
                       o.n_fits, o.q, o.t, o.rms, o.status, o.summaries);
    st.launched();
    if (!st.ok()) return;
    hipLaunchKernelGGL(rp::pose_rescore_kernel, grid, block, 0, st.stream(), lifted, c.board, c.off, c.first, ro.threshold,
                       (int)ro.min_inliers, (int)ro.max_fits, o.mask, sub_l, sub_b, o.n_inliers, flag, o.n_fits, o.q, o.t, o.rms,
                       o.status, o.summaries);
    st.launched();
  }
}

// The alternate call's options: the caller's or the defaults; checked.
int alt_options(const clc_alt_pose_options* in, clc_alt_pose_options* o, const char* who) {
  if (in) *o = *in; else clc_alt_pose_options_default(o);
  const std::string w(who);
  if (!(std::isfinite(o->same_angle) && o->same_angle > 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": same_angle must be finite and > 0").c_str());
  if (!(std::isfinite(o->ratio_gate) && o->ratio_gate >= 1.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": ratio_gate must be finite and >= 1").c_str());
  return CLC_OK;
}

// Every refusal of clc_board_poses_alternate and its _device form up to the empty call: the options first.
int alt_checks(const char* who, const clc_handle* h, bool required, const clc_camera* cam, const clc_options* opt_in,
               const clc_alt_pose_options* aopt_in, size_t n_images, clc_options* opt, clc_alt_pose_options* ao) {
  CLC_TRY(camera_check(cam, who));
  CLC_TRY(pose_options(opt_in, opt, who));
  CLC_TRY(alt_options(aopt_in, ao, who));
  return count_checks(who, h, required, n_images);
}

// What the alternate call reads per image, every array on the device (inlier nullable, indexed by the absolute offsets).
struct AltIn {
  const unsigned char* inlier;
  const double *q, *t;
  const int32_t* status;
};

// K17 on device arrays: lift -> start -> fit on the handle's stream, every launch sized by n_images, no read-back in between.
void enqueue_board_poses_alternate(Staging& st, const clc_camera& cam, const clc_options& opt, const clc_alt_pose_options& ao,
                                   const Corners& c, const AltIn& in, const clc::ap::AltOut& o) {
  namespace ap = clc::ap;
  const float* lifted = enqueue_lift(st, cam, c.px, c.first, c.n_corners);
  float* sub_l = st.scratch<float>(2 * c.n_corners);  // indexed like lifted: corner `first` first
  float* sub_b = st.scratch<float>(2 * c.n_corners);
  int32_t* cnt = st.scratch<int32_t>(c.n_images);
  int32_t* flag = st.scratch<int32_t>(c.n_images);
  double* start7 = st.scratch<double>(7 * c.n_images);
  if (!st.ok()) return;
  const dim3 grid((unsigned)c.n_images), block(64);
  hipLaunchKernelGGL(ap::alt_start_kernel, grid, block, 0, st.stream(), lifted, c.board, c.off, c.first, in.inlier, in.q, in.t, in.status,
                     sub_l, sub_b, cnt, flag, start7, o);
  st.launched();
  if (!st.ok()) return;
  hipLaunchKernelGGL(ap::board_pose_from_start_kernel, grid, block, 0, st.stream(), opt, ao, sub_l, sub_b, c.off, c.first, flag, cnt, start7,
                     in.q, in.t, o);
  st.launched();
}

}  // namespace

extern "C" {

void clc_pose_options_default(clc_options* o) {
  clc_options_default(o);
  if (!o) return;
  o->use_loss = 0;
  o->max_num_iterations = 50;
  o->function_tolerance = 1e-15;
  o->parameter_tolerance = 1e-14;
  o->gradient_tolerance = 1e-16;
}

int clc_camera_lift(clc_handle* h, const clc_camera* cam, const float* px, size_t n, double* xy_norm) {
  if (!h || (n > 0 && (!px || !xy_norm))) return fail(CLC_ERR_INVALID_ARG, "clc_camera_lift: bad argument");
  CLC_TRY(camera_check(cam, "clc_camera_lift"));
  if (n == 0) return CLC_OK;
  if (n > 0x3FFFFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_camera_lift: too many points");
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  const float* px_dev = st.in(px, 2 * n);
  double* out_dev = st.out(xy_norm, 2 * n);
  if (st.ok()) {
    hipLaunchKernelGGL((clc::cp::campose_lift_kernel<false>), dim3(lift_blocks(n)), dim3(clc::cp::LIFT_THREADS), 0, st.stream(), *cam, px_dev,
                       (long long)n, out_dev, nullptr);
    st.launched();
  }
  return st.finish("clc_camera_lift");
}

int clc_camera_project(clc_handle* h, const clc_camera* cam, const double pose7[7], const double* pts, size_t n, double* px) {
  if (!h || (n > 0 && (!pts || !px))) return fail(CLC_ERR_INVALID_ARG, "clc_camera_project: bad argument");
  CLC_TRY(camera_check(cam, "clc_camera_project"));
  clc::cp::Pose7Arg pose{};
  if (pose7) {
    for (int i = 0; i < 7; ++i) {
      if (!std::isfinite(pose7[i])) return fail(CLC_ERR_NONFINITE, "clc_camera_project: non-finite pose");
      pose.v[i] = pose7[i];
    }
  }
  if (n == 0) return CLC_OK;
  if (n > 0x3FFFFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_camera_project: too many points");
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  const double* pts_dev = st.in(pts, 3 * n);
  double* px_dev = st.out(px, 2 * n);
  if (st.ok()) {
    hipLaunchKernelGGL(clc::cp::campose_project_kernel, dim3(lift_blocks(n)), dim3(clc::cp::LIFT_THREADS), 0, st.stream(), *cam, pose,
                       pose7 ? 1 : 0, pts_dev, (long long)n, px_dev);
    st.launched();
  }
  return st.finish("clc_camera_project");
}

int clc_board_poses(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const float* corners_px, const float* board_xy,
                    const int64_t* offsets, size_t n_images, double* q_ca_wxyz, double* t_ca, double* rms, int32_t* status,
                    clc_summary* summaries) {
  const char* who = "clc_board_poses";
  clc_options opt;
  CLC_TRY(board_pose_checks(who, h, offsets && q_ca_wxyz && t_ca && status, cam, opt_in, n_images, &opt));
  if (n_images == 0) return CLC_OK;
  std::vector<long long> rel;
  size_t M;
  CLC_TRY(host_offsets(who, offsets, n_images, true, nullptr, &rel, &M));
  if (M > 0 && (!corners_px || !board_xy)) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses: bad argument");
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = Clock::now();
  Staging st(h);
  const Corners c = upload_corners(st, corners_px, board_xy, offsets, rel, M);
  double* q_dev = st.out(q_ca_wxyz, 4 * n_images);
  double* t_dev = st.out(t_ca, 3 * n_images);
  double* rms_dev = st.out_opt(rms, n_images);
  int32_t* status_dev = st.out(status, n_images);
  enqueue_board_poses(st, *cam, opt, c, q_dev, t_dev, rms_dev, status_dev, st.out_opt(summaries, n_images));
  CLC_TRY(st.finish(who));
  stamp_solve_ms(summaries, n_images, t0);
  return CLC_OK;
}

int clc_board_poses_device(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const float* corners_px_dev,
                           const float* board_xy_dev, const int64_t* offsets_dev, size_t n_images, double* q_ca_wxyz_dev,
                           double* t_ca_dev, double* rms_dev, int32_t* status_dev, clc_summary* summaries_dev) {
  const char* who = "clc_board_poses_device";
  clc_options opt;
  CLC_TRY(board_pose_checks(who, h, offsets_dev && q_ca_wxyz_dev && t_ca_dev && status_dev, cam, opt_in, n_images, &opt));
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  long long ends[2];
  CLC_TRY(device_offset_ends(h, who, offsets_dev, n_images, ends));
  const Corners c = device_corners(corners_px_dev, board_xy_dev, offsets_dev, ends, n_images);
  if (c.n_corners > 0 && (!corners_px_dev || !board_xy_dev)) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_device: bad argument");
  Staging st(h);
  enqueue_board_poses(st, *cam, opt, c, q_ca_wxyz_dev, t_ca_dev, rms_dev, status_dev, summaries_dev);
  return st.finish(who);
}

void clc_robust_pose_options_default(clc_robust_pose_options* o, const clc_camera* cam) {
  if (!o) return;
  // 8 px and 2 px: design values from the numpy experiment recorded in DESIGN.md K16, in units of the focal length
  const double f = cam ? std::sqrt(std::fabs(cam->proj[0] * cam->proj[1])) : 0.0;
  o->hyp_threshold = f > 0.0 ? 8.0 / f : 0.0;
  o->threshold = f > 0.0 ? 2.0 / f : 0.0;
  o->min_inliers = 4;
  o->max_fits = 4;
}

int clc_board_poses_robust(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_robust_pose_options* ropt_in,
                           const float* corners_px, const float* board_xy, const int64_t* offsets, size_t n_images, double* q_ca_wxyz,
                           double* t_ca, double* rms, int32_t* status, clc_summary* summaries, uint8_t* inlier, int32_t* n_inliers,
                           int32_t* best_group, int32_t* n_fits) {
  const char* who = "clc_board_poses_robust";
  clc_options opt;
  clc_robust_pose_options ro;
  CLC_TRY(robust_checks(who, h, offsets && q_ca_wxyz && t_ca && status, cam, opt_in, ropt_in, n_images, &opt, &ro));
  if (n_images == 0) return CLC_OK;
  std::vector<long long> rel;
  size_t M;
  CLC_TRY(host_offsets(who, offsets, n_images, true, nullptr, &rel, &M));
  if (M > 0 && (!corners_px || !board_xy || !inlier)) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_robust: bad argument");
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = Clock::now();
  Staging st(h);
  const Corners c = upload_corners(st, corners_px, board_xy, offsets, rel, M);
  const size_t n = n_images;
  RobustOut out{};
  out.q = st.out(q_ca_wxyz, 4 * n);
  out.t = st.out(t_ca, 3 * n);
  out.rms = st.out_opt(rms, n);
  out.status = st.out(status, n);
  out.summaries = st.out_opt(summaries, n);
  out.mask = st.out(M > 0 ? inlier + offsets[0] : nullptr, M);  // indexed by the absolute offsets
  out.n_inliers = st.out_opt(n_inliers, n);
  out.best_group = st.out_opt(best_group, n);
  out.n_fits = st.out_opt(n_fits, n);
  enqueue_board_poses_robust(st, *cam, opt, ro, c, out);
  CLC_TRY(st.finish(who));
  stamp_solve_ms(summaries, n, t0);
  return CLC_OK;
}

int clc_board_poses_robust_device(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_robust_pose_options* ropt_in,
                                  const float* corners_px_dev, const float* board_xy_dev, const int64_t* offsets_dev, size_t n_images,
                                  double* q_ca_wxyz_dev, double* t_ca_dev, double* rms_dev, int32_t* status_dev,
                                  clc_summary* summaries_dev, uint8_t* inlier_dev, int32_t* n_inliers_dev, int32_t* best_group_dev,
                                  int32_t* n_fits_dev) {
  const char* who = "clc_board_poses_robust_device";
  clc_options opt;
  clc_robust_pose_options ro;
  CLC_TRY(robust_checks(who, h, offsets_dev && q_ca_wxyz_dev && t_ca_dev && status_dev, cam, opt_in, ropt_in, n_images, &opt, &ro));
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  long long ends[2];
  CLC_TRY(device_offset_ends(h, who, offsets_dev, n_images, ends));
  const Corners c = device_corners(corners_px_dev, board_xy_dev, offsets_dev, ends, n_images);
  if (c.n_corners > 0 && (!corners_px_dev || !board_xy_dev || !inlier_dev))
    return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_robust_device: bad argument");
  Staging st(h);
  enqueue_board_poses_robust(st, *cam, opt, ro, c, RobustOut{q_ca_wxyz_dev, t_ca_dev, rms_dev, status_dev, summaries_dev, inlier_dev,
                                                            n_inliers_dev, best_group_dev, n_fits_dev});
  return st.finish(who);
}

void clc_alt_pose_options_default(clc_alt_pose_options* o) {
  if (!o) return;
  // design values (include/clc.h): between the two clusters of rot_angle; a mirror within a factor two of the cost
  o->same_angle = 0.01;
  o->ratio_gate = 2.0;
}

int clc_board_poses_alternate(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_alt_pose_options* aopt_in,
                              const float* corners_px, const float* board_xy, const int64_t* offsets, size_t n_images,
                              const uint8_t* inlier, const double* q_in_wxyz, const double* t_in, const int32_t* status_in,
                              double* q_alt_wxyz, double* t_alt, double* rms_alt, double* cost_in, double* cost_alt, double* ratio,
                              double* rot_angle, double* normal_angle, int32_t* kind, uint8_t* ambiguous, uint8_t* better,
                              clc_summary* summaries_alt) {
  const char* who = "clc_board_poses_alternate";
  clc_options opt;
  clc_alt_pose_options ao;
  CLC_TRY(alt_checks(who, h, offsets && q_in_wxyz && t_in && status_in && kind, cam, opt_in, aopt_in, n_images, &opt, &ao));
  if (n_images == 0) return CLC_OK;
  std::vector<long long> rel;
  size_t M;
  CLC_TRY(host_offsets(who, offsets, n_images, true, nullptr, &rel, &M));
  if (M > 0 && (!corners_px || !board_xy)) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_alternate: bad argument");
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = Clock::now();
  Staging st(h);
  const Corners c = upload_corners(st, corners_px, board_xy, offsets, rel, M);
  const size_t n = n_images;
  AltIn in{};
  in.inlier = st.in_opt(inlier && M > 0 ? inlier + offsets[0] : nullptr, M);  // indexed by the absolute offsets; none without corners
  in.q = st.in(q_in_wxyz, 4 * n);
  in.t = st.in(t_in, 3 * n);
  in.status = st.in(status_in, n);
  clc::ap::AltOut out{};
  out.q = st.out_opt(q_alt_wxyz, 4 * n);
  out.t = st.out_opt(t_alt, 3 * n);
  out.rms = st.out_opt(rms_alt, n);
  out.cost_in = st.out_opt(cost_in, n);
  out.cost_alt = st.out_opt(cost_alt, n);
  out.ratio = st.out_opt(ratio, n);
  out.rot_angle = st.out_opt(rot_angle, n);
  out.normal_angle = st.out_opt(normal_angle, n);
  out.kind = st.out(kind, n);
  out.ambiguous = st.out_opt(ambiguous, n);
  out.better = st.out_opt(better, n);
  out.summaries = st.out_opt(summaries_alt, n);
  enqueue_board_poses_alternate(st, *cam, opt, ao, c, in, out);
  CLC_TRY(st.finish(who));
  stamp_solve_ms(summaries_alt, n, t0);
  return CLC_OK;
}

int clc_board_poses_alternate_device(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_alt_pose_options* aopt_in,
                                     const float* corners_px_dev, const float* board_xy_dev, const int64_t* offsets_dev,
                                     size_t n_images, const uint8_t* inlier_dev, const double* q_in_wxyz_dev, const double* t_in_dev,
                                     const int32_t* status_in_dev, double* q_alt_wxyz_dev, double* t_alt_dev, double* rms_alt_dev,
                                     double* cost_in_dev, double* cost_alt_dev, double* ratio_dev, double* rot_angle_dev,
                                     double* normal_angle_dev, int32_t* kind_dev, uint8_t* ambiguous_dev, uint8_t* better_dev,
                                     clc_summary* summaries_alt_dev) {
  const char* who = "clc_board_poses_alternate_device";
  clc_options opt;
  clc_alt_pose_options ao;
  CLC_TRY(alt_checks(who, h, offsets_dev && q_in_wxyz_dev && t_in_dev && status_in_dev && kind_dev, cam, opt_in, aopt_in, n_images, &opt,
                     &ao));
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  long long ends[2];
  CLC_TRY(device_offset_ends(h, who, offsets_dev, n_images, ends));
  const Corners c = device_corners(corners_px_dev, board_xy_dev, offsets_dev, ends, n_images);
  if (c.n_corners > 0 && (!corners_px_dev || !board_xy_dev)) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_alternate_device: bad argument");
  Staging st(h);
  const AltIn in{inlier_dev, q_in_wxyz_dev, t_in_dev, status_in_dev};
  const clc::ap::AltOut out{q_alt_wxyz_dev, t_alt_dev, rms_alt_dev, cost_in_dev, cost_alt_dev, ratio_dev, rot_angle_dev, normal_angle_dev,
                            kind_dev, ambiguous_dev, better_dev, summaries_alt_dev};
  enqueue_board_poses_alternate(st, *cam, opt, ao, c, in, out);
  return st.finish(who);
}

}  // extern "C"
