// abi_campose.hip — clc_camera_lift, clc_camera_project, clc_board_poses(_device): the camera models and the batched planar PnP
// (K10 in clc_campose.hpp); clc_board_poses_robust(_device): the per-tag consensus ahead of it (K16 in clc_robustpose.hpp);
// clc_board_poses_alternate(_device): the planar fit's second minimum (K17 in clc_altpose.hpp).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "clc_campose.hpp"
#include "clc_robustpose.hpp"
#include "clc_altpose.hpp"

using namespace clc_abi;

namespace {

unsigned lift_blocks(size_t n) { return (unsigned)((n + clc::cp::LIFT_THREADS - 1) / clc::cp::LIFT_THREADS); }

// lift (rounded) into lifted_dev[2 * n_corners] (corner `first` first), then one wave per image; every array on the device, offsets
// absolute
hipError_t launch_board_poses(clc_handle* h, const clc_camera& cam, const clc_options& opt, const float* corners_dev, const float* board_dev,
                              const long long* off_dev, long long first, size_t n_corners, size_t n_images, float* lifted_dev,
                              double* q_dev, double* t_dev, double* rms_dev, int32_t* status_dev, clc_summary* sum_dev) {
  if (n_corners > 0) {
    hipLaunchKernelGGL((clc::cp::campose_lift_kernel<true>), dim3(lift_blocks(n_corners)), dim3(clc::cp::LIFT_THREADS), 0, h->stream, cam,
                       corners_dev + 2 * first, (long long)n_corners, nullptr, lifted_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(clc::cp::board_pose_kernel, dim3((unsigned)n_images), dim3(64), 0, h->stream, opt, lifted_dev, board_dev, off_dev,
                     first, q_dev, t_dev, rms_dev, status_dev, sum_dev);
  return hipGetLastError();
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

// What the robust call leaves per image, every array on the device (mask indexed by the absolute offsets; rms, summaries, best_group
// nullable).
struct RobustOut {
  double *q, *t, *rms;
  int32_t* status;
  clc_summary* summaries;
  unsigned char* mask;
  int32_t *n_inliers, *best_group, *n_fits;
};

// lift -> consensus -> (fit -> re-gate) x max_fits on the handle's stream, every launch sized by n_images, no read-back in between.
// Scratch of the caller (indexed like lifted_dev, corner `first` first): lifted_dev, sub_l, sub_b [2 * n_corners]; flag [n_images].
hipError_t launch_board_poses_robust(clc_handle* h, const clc_camera& cam, const clc_options& opt, const clc_robust_pose_options& ro,
                                     const float* corners_dev, const float* board_dev, const long long* off_dev, long long first,
                                     size_t n_corners, size_t n_images, float* lifted_dev, float* sub_l, float* sub_b, int32_t* flag,
                                     const RobustOut& o) {
  namespace rp = clc::rp;
  if (n_corners > 0) {
    hipLaunchKernelGGL((clc::cp::campose_lift_kernel<true>), dim3(lift_blocks(n_corners)), dim3(clc::cp::LIFT_THREADS), 0, h->stream, cam,
                       corners_dev + 2 * first, (long long)n_corners, nullptr, lifted_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)n_images), block(64);
  hipLaunchKernelGGL(rp::tag_consensus_kernel, grid, block, 0, h->stream, lifted_dev, board_dev, off_dev, first, ro.hyp_threshold,
                     (int)ro.min_inliers, o.mask, sub_l, sub_b, o.n_inliers, flag, o.n_fits, o.best_group, o.q, o.t, o.rms, o.status,
                     o.summaries);
  hipError_t e = hipGetLastError();
  for (int round = 0; round < ro.max_fits && e == hipSuccess; ++round) {
    hipLaunchKernelGGL(rp::board_pose_subset_kernel, grid, block, 0, h->stream, opt, sub_l, sub_b, off_dev, first, flag, o.n_inliers,
                       o.n_fits, o.q, o.t, o.rms, o.status, o.summaries);
    e = hipGetLastError();
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(rp::pose_rescore_kernel, grid, block, 0, h->stream, lifted_dev, board_dev, off_dev, first, ro.threshold,
                       (int)ro.min_inliers, (int)ro.max_fits, o.mask, sub_l, sub_b, o.n_inliers, flag, o.n_fits, o.q, o.t, o.rms,
                       o.status, o.summaries);
    e = hipGetLastError();
  }
  return e;
}

// The alternate call's options: the caller's or the defaults; checked.
int alt_options(const clc_alt_pose_options* in, clc_alt_pose_options* o, const char* who) {
  if (in) *o = *in; else clc_alt_pose_options_default(o);
  const std::string w(who);
  if (!(std::isfinite(o->same_angle) && o->same_angle > 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": same_angle must be finite and > 0").c_str());
  if (!(std::isfinite(o->ratio_gate) && o->ratio_gate >= 1.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": ratio_gate must be finite and >= 1").c_str());
  return CLC_OK;
}

// What the alternate call reads per image, every array on the device (inlier nullable, indexed by the absolute offsets).
struct AltIn {
  const unsigned char* inlier;
  const double *q, *t;
  const int32_t* status;
};

// lift -> start -> fit on the handle's stream, every launch sized by n_images, no read-back in between.  Scratch of the caller
// (indexed like lifted_dev, corner `first` first): lifted_dev, sub_l, sub_b [2 * n_corners]; cnt, flag [n_images]; start7 [7 * n_images].
hipError_t launch_board_poses_alternate(clc_handle* h, const clc_camera& cam, const clc_options& opt, const clc_alt_pose_options& ao,
                                        const float* corners_dev, const float* board_dev, const long long* off_dev, long long first,
                                        size_t n_corners, size_t n_images, const AltIn& in, float* lifted_dev, float* sub_l, float* sub_b,
                                        int32_t* cnt, int32_t* flag, double* start7, const clc::ap::AltOut& o) {
  namespace ap = clc::ap;
  if (n_corners > 0) {
    hipLaunchKernelGGL((clc::cp::campose_lift_kernel<true>), dim3(lift_blocks(n_corners)), dim3(clc::cp::LIFT_THREADS), 0, h->stream, cam,
                       corners_dev + 2 * first, (long long)n_corners, nullptr, lifted_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)n_images), block(64);
  hipLaunchKernelGGL(ap::alt_start_kernel, grid, block, 0, h->stream, lifted_dev, board_dev, off_dev, first, in.inlier, in.q, in.t,
                     in.status, sub_l, sub_b, cnt, flag, start7, o);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ap::board_pose_from_start_kernel, grid, block, 0, h->stream, opt, ao, sub_l, sub_b, off_dev, first, flag, cnt, start7,
                     in.q, in.t, o);
  return hipGetLastError();
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
  DevBuf<float> bp(&h->pool);
  DevBuf<double> bo(&h->pool);
  CLC_HIP(bp.alloc(2 * n));
  CLC_HIP(bo.alloc(2 * n));
  CLC_HIP(hipMemcpyAsync(bp.p, px, 2 * n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL((clc::cp::campose_lift_kernel<false>), dim3(lift_blocks(n)), dim3(clc::cp::LIFT_THREADS), 0, h->stream, *cam, bp.p,
                     (long long)n, bo.p, nullptr);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipMemcpyAsync(xy_norm, bo.p, 2 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
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
  DevBuf<double> bp(&h->pool), bo(&h->pool);
  CLC_HIP(bp.alloc(3 * n));
  CLC_HIP(bo.alloc(2 * n));
  CLC_HIP(hipMemcpyAsync(bp.p, pts, 3 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(clc::cp::campose_project_kernel, dim3(lift_blocks(n)), dim3(clc::cp::LIFT_THREADS), 0, h->stream, *cam, pose,
                     pose7 ? 1 : 0, bp.p, (long long)n, bo.p);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipMemcpyAsync(px, bo.p, 2 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
}

int clc_board_poses(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const float* corners_px, const float* board_xy,
                    const int64_t* offsets, size_t n_images, double* q_ca_wxyz, double* t_ca, double* rms, int32_t* status,
                    clc_summary* summaries) {
  if (!h || (n_images > 0 && (!offsets || !q_ca_wxyz || !t_ca || !status)))
    return fail(CLC_ERR_INVALID_ARG, "clc_board_poses: bad argument");
  CLC_TRY(camera_check(cam, "clc_board_poses"));
  clc_options opt;
  CLC_TRY(pose_options(opt_in, &opt, "clc_board_poses"));
  if (n_images == 0) return CLC_OK;
  if (n_images > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses: too many images");
  std::vector<long long> rel;
  size_t M;
  CLC_TRY(host_offsets("clc_board_poses", offsets, n_images, true, nullptr, &rel, &M));
  if (M > 0 && (!corners_px || !board_xy)) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses: bad argument");
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  DevBuf<float> bc(&h->pool), bb(&h->pool), bl(&h->pool);
  DevBuf<long long> boff(&h->pool);
  DevBuf<double> bq(&h->pool), bt(&h->pool), br(&h->pool);
  DevBuf<int32_t> bs(&h->pool);
  DevBuf<clc_summary> bsum(&h->pool);
  CLC_HIP(bc.alloc(2 * M)); CLC_HIP(bb.alloc(2 * M)); CLC_HIP(bl.alloc(2 * M)); CLC_HIP(boff.alloc(n_images + 1));
  CLC_HIP(bq.alloc(4 * n_images)); CLC_HIP(bt.alloc(3 * n_images)); CLC_HIP(bs.alloc(n_images));
  if (rms) CLC_HIP(br.alloc(n_images));
  if (summaries) CLC_HIP(bsum.alloc(n_images));
  if (M > 0) {
    CLC_HIP(hipMemcpyAsync(bc.p, corners_px + 2 * offsets[0], 2 * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bb.p, board_xy + 2 * offsets[0], 2 * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
  }
  CLC_HIP(hipMemcpyAsync(boff.p, rel.data(), (n_images + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(launch_board_poses(h, *cam, opt, bc.p, bb.p, boff.p, 0, M, n_images, bl.p, bq.p, bt.p, rms ? br.p : nullptr, bs.p,
                             summaries ? bsum.p : nullptr));
  CLC_HIP(hipMemcpyAsync(q_ca_wxyz, bq.p, 4 * n_images * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(t_ca, bt.p, 3 * n_images * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(status, bs.p, n_images * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (rms) CLC_HIP(hipMemcpyAsync(rms, br.p, n_images * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (summaries) CLC_HIP(hipMemcpyAsync(summaries, bsum.p, n_images * sizeof(clc_summary), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  if (summaries) {
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (size_t k = 0; k < n_images; ++k) summaries[k].solve_ms = ms;
  }
  return CLC_OK;
}

int clc_board_poses_device(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const float* corners_px_dev,
                           const float* board_xy_dev, const int64_t* offsets_dev, size_t n_images, double* q_ca_wxyz_dev,
                           double* t_ca_dev, double* rms_dev, int32_t* status_dev, clc_summary* summaries_dev) {
  if (!h || (n_images > 0 && (!offsets_dev || !q_ca_wxyz_dev || !t_ca_dev || !status_dev)))
    return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_device: bad argument");
  CLC_TRY(camera_check(cam, "clc_board_poses_device"));
  clc_options opt;
  CLC_TRY(pose_options(opt_in, &opt, "clc_board_poses_device"));
  if (n_images == 0) return CLC_OK;
  if (n_images > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_device: too many images");
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  CLC_HIP(hipSetDevice(h->device));
  // the corner range: the two ends of the offsets (a small read; the lifted corners go to a scratch array of the same indexing)
  long long ends[2];
  CLC_HIP(hipMemcpyAsync(&ends[0], offsets_dev, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(&ends[1], offsets_dev + n_images, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  if (ends[1] < ends[0] || ends[0] < 0) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_device: offsets not monotone");
  const size_t M = (size_t)(ends[1] - ends[0]);
  if (M > 0 && (!corners_px_dev || !board_xy_dev)) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_device: bad argument");
  DevBuf<float> bl(&h->pool);
  CLC_HIP(bl.alloc(2 * M));
  CLC_HIP(launch_board_poses(h, *cam, opt, corners_px_dev, board_xy_dev, reinterpret_cast<const long long*>(offsets_dev), ends[0], M,
                             n_images, bl.p, q_ca_wxyz_dev, t_ca_dev, rms_dev, status_dev, summaries_dev));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
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
  // the options first: their refusals need no device
  CLC_TRY(camera_check(cam, who));
  clc_options opt;
  CLC_TRY(pose_options(opt_in, &opt, who));
  clc_robust_pose_options ro;
  CLC_TRY(robust_options(ropt_in, cam, &ro, who));
  if (!h || (n_images > 0 && (!offsets || !q_ca_wxyz || !t_ca || !status)))
    return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_robust: bad argument");
  if (n_images == 0) return CLC_OK;
  if (n_images > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_robust: too many images");
  std::vector<long long> rel;
  size_t M;
  CLC_TRY(host_offsets(who, offsets, n_images, true, nullptr, &rel, &M));
  if (M > 0 && (!corners_px || !board_xy || !inlier)) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_robust: bad argument");
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  DevBuf<float> bc(&h->pool), bb(&h->pool), bl(&h->pool), bsl(&h->pool), bsb(&h->pool);
  DevBuf<long long> boff(&h->pool);
  DevBuf<double> bq(&h->pool), bt(&h->pool), br(&h->pool);
  DevBuf<int32_t> bs(&h->pool), bflag(&h->pool), bni(&h->pool), bnf(&h->pool), bbg(&h->pool);
  DevBuf<clc_summary> bsum(&h->pool);
  DevBuf<unsigned char> bm(&h->pool);
  CLC_HIP(bc.alloc(2 * M)); CLC_HIP(bb.alloc(2 * M)); CLC_HIP(bl.alloc(2 * M)); CLC_HIP(bsl.alloc(2 * M)); CLC_HIP(bsb.alloc(2 * M));
  CLC_HIP(bm.alloc(M)); CLC_HIP(boff.alloc(n_images + 1));
  CLC_HIP(bq.alloc(4 * n_images)); CLC_HIP(bt.alloc(3 * n_images)); CLC_HIP(bs.alloc(n_images));
  CLC_HIP(bflag.alloc(n_images)); CLC_HIP(bni.alloc(n_images)); CLC_HIP(bnf.alloc(n_images));
  if (rms) CLC_HIP(br.alloc(n_images));
  if (summaries) CLC_HIP(bsum.alloc(n_images));
  if (best_group) CLC_HIP(bbg.alloc(n_images));
  if (M > 0) {
    CLC_HIP(hipMemcpyAsync(bc.p, corners_px + 2 * offsets[0], 2 * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bb.p, board_xy + 2 * offsets[0], 2 * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
  }
  CLC_HIP(hipMemcpyAsync(boff.p, rel.data(), (n_images + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  const RobustOut out{bq.p, bt.p, rms ? br.p : nullptr, bs.p, summaries ? bsum.p : nullptr, bm.p, bni.p, best_group ? bbg.p : nullptr,
                      bnf.p};
  CLC_HIP(launch_board_poses_robust(h, *cam, opt, ro, bc.p, bb.p, boff.p, 0, M, n_images, bl.p, bsl.p, bsb.p, bflag.p, out));
  CLC_HIP(hipMemcpyAsync(q_ca_wxyz, bq.p, 4 * n_images * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(t_ca, bt.p, 3 * n_images * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(status, bs.p, n_images * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (M > 0) CLC_HIP(hipMemcpyAsync(inlier + offsets[0], bm.p, M, hipMemcpyDeviceToHost, h->stream));
  if (rms) CLC_HIP(hipMemcpyAsync(rms, br.p, n_images * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (summaries) CLC_HIP(hipMemcpyAsync(summaries, bsum.p, n_images * sizeof(clc_summary), hipMemcpyDeviceToHost, h->stream));
  if (n_inliers) CLC_HIP(hipMemcpyAsync(n_inliers, bni.p, n_images * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (best_group) CLC_HIP(hipMemcpyAsync(best_group, bbg.p, n_images * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (n_fits) CLC_HIP(hipMemcpyAsync(n_fits, bnf.p, n_images * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  if (summaries) {
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (size_t k = 0; k < n_images; ++k) summaries[k].solve_ms = ms;
  }
  return CLC_OK;
}

int clc_board_poses_robust_device(clc_handle* h, const clc_camera* cam, const clc_options* opt_in, const clc_robust_pose_options* ropt_in,
                                  const float* corners_px_dev, const float* board_xy_dev, const int64_t* offsets_dev, size_t n_images,
                                  double* q_ca_wxyz_dev, double* t_ca_dev, double* rms_dev, int32_t* status_dev,
                                  clc_summary* summaries_dev, uint8_t* inlier_dev, int32_t* n_inliers_dev, int32_t* best_group_dev,
                                  int32_t* n_fits_dev) {
  const char* who = "clc_board_poses_robust_device";
  // the options first: their refusals need no device
  CLC_TRY(camera_check(cam, who));
  clc_options opt;
  CLC_TRY(pose_options(opt_in, &opt, who));
  clc_robust_pose_options ro;
  CLC_TRY(robust_options(ropt_in, cam, &ro, who));
  if (!h || (n_images > 0 && (!offsets_dev || !q_ca_wxyz_dev || !t_ca_dev || !status_dev)))
    return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_robust_device: bad argument");
  if (n_images == 0) return CLC_OK;
  if (n_images > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_robust_device: too many images");
  CLC_HIP(hipSetDevice(h->device));
  long long ends[2];  // the corner range, as clc_board_poses_device reads it
  CLC_HIP(hipMemcpyAsync(&ends[0], offsets_dev, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(&ends[1], offsets_dev + n_images, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  if (ends[1] < ends[0] || ends[0] < 0) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_robust_device: offsets not monotone");
  const size_t M = (size_t)(ends[1] - ends[0]);
  if (M > 0 && (!corners_px_dev || !board_xy_dev || !inlier_dev))
    return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_robust_device: bad argument");
  DevBuf<float> bl(&h->pool), bsl(&h->pool), bsb(&h->pool);
  DevBuf<int32_t> bflag(&h->pool), bni(&h->pool), bnf(&h->pool);
  CLC_HIP(bl.alloc(2 * M)); CLC_HIP(bsl.alloc(2 * M)); CLC_HIP(bsb.alloc(2 * M)); CLC_HIP(bflag.alloc(n_images));
  if (!n_inliers_dev) CLC_HIP(bni.alloc(n_images));
  if (!n_fits_dev) CLC_HIP(bnf.alloc(n_images));
  const RobustOut out{q_ca_wxyz_dev, t_ca_dev, rms_dev, status_dev, summaries_dev, inlier_dev, n_inliers_dev ? n_inliers_dev : bni.p,
                      best_group_dev, n_fits_dev ? n_fits_dev : bnf.p};
  CLC_HIP(launch_board_poses_robust(h, *cam, opt, ro, corners_px_dev, board_xy_dev, reinterpret_cast<const long long*>(offsets_dev),
                                    ends[0], M, n_images, bl.p, bsl.p, bsb.p, bflag.p, out));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
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
  // the options first: their refusals need no device
  CLC_TRY(camera_check(cam, who));
  clc_options opt;
  CLC_TRY(pose_options(opt_in, &opt, who));
  clc_alt_pose_options ao;
  CLC_TRY(alt_options(aopt_in, &ao, who));
  if (!h || (n_images > 0 && (!offsets || !q_in_wxyz || !t_in || !status_in || !kind)))
    return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_alternate: bad argument");
  if (n_images == 0) return CLC_OK;
  if (n_images > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_alternate: too many images");
  std::vector<long long> rel;
  size_t M;
  CLC_TRY(host_offsets(who, offsets, n_images, true, nullptr, &rel, &M));
  if (M > 0 && (!corners_px || !board_xy)) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_alternate: bad argument");
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  const size_t n = n_images;
  DevBuf<float> bc(&h->pool), bb(&h->pool), bl(&h->pool), bsl(&h->pool), bsb(&h->pool);
  DevBuf<long long> boff(&h->pool);
  DevBuf<unsigned char> bm(&h->pool), bamb(&h->pool), bbet(&h->pool);
  DevBuf<double> bqi(&h->pool), bti(&h->pool), bq(&h->pool), bt(&h->pool), bst7(&h->pool);
  DevBuf<double> breal(&h->pool);  // rms, cost_in, cost_alt, ratio, rot_angle, normal_angle: n each
  DevBuf<int32_t> bsi(&h->pool), bkind(&h->pool), bcnt(&h->pool), bflag(&h->pool);
  DevBuf<clc_summary> bsum(&h->pool);
  CLC_HIP(bc.alloc(2 * M)); CLC_HIP(bb.alloc(2 * M)); CLC_HIP(bl.alloc(2 * M)); CLC_HIP(bsl.alloc(2 * M)); CLC_HIP(bsb.alloc(2 * M));
  CLC_HIP(boff.alloc(n + 1));
  if (inlier) CLC_HIP(bm.alloc(M));
  CLC_HIP(bqi.alloc(4 * n)); CLC_HIP(bti.alloc(3 * n)); CLC_HIP(bsi.alloc(n)); CLC_HIP(bkind.alloc(n)); CLC_HIP(bcnt.alloc(n));
  CLC_HIP(bflag.alloc(n)); CLC_HIP(bst7.alloc(7 * n)); CLC_HIP(breal.alloc(6 * n));
  if (q_alt_wxyz) CLC_HIP(bq.alloc(4 * n));
  if (t_alt) CLC_HIP(bt.alloc(3 * n));
  if (ambiguous) CLC_HIP(bamb.alloc(n));
  if (better) CLC_HIP(bbet.alloc(n));
  if (summaries_alt) CLC_HIP(bsum.alloc(n));
  if (M > 0) {
    CLC_HIP(hipMemcpyAsync(bc.p, corners_px + 2 * offsets[0], 2 * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bb.p, board_xy + 2 * offsets[0], 2 * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (inlier) CLC_HIP(hipMemcpyAsync(bm.p, inlier + offsets[0], M, hipMemcpyHostToDevice, h->stream));
  }
  CLC_HIP(hipMemcpyAsync(boff.p, rel.data(), (n + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(bqi.p, q_in_wxyz, 4 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(bti.p, t_in, 3 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(bsi.p, status_in, n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  double* const host_real[6] = {rms_alt, cost_in, cost_alt, ratio, rot_angle, normal_angle};
  double* dev_real[6];
  for (int i = 0; i < 6; ++i) dev_real[i] = host_real[i] ? breal.p + (size_t)i * n : nullptr;
  const AltIn in{(inlier && M > 0) ? bm.p : nullptr, bqi.p, bti.p, bsi.p};
  const clc::ap::AltOut out{q_alt_wxyz ? bq.p : nullptr, t_alt ? bt.p : nullptr, dev_real[0], dev_real[1], dev_real[2],
                            dev_real[3], dev_real[4], dev_real[5], bkind.p, ambiguous ? bamb.p : nullptr, better ? bbet.p : nullptr,
                            summaries_alt ? bsum.p : nullptr};
  CLC_HIP(launch_board_poses_alternate(h, *cam, opt, ao, bc.p, bb.p, boff.p, 0, M, n, in, bl.p, bsl.p, bsb.p, bcnt.p, bflag.p, bst7.p,
                                       out));
  CLC_HIP(hipMemcpyAsync(kind, bkind.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (q_alt_wxyz) CLC_HIP(hipMemcpyAsync(q_alt_wxyz, bq.p, 4 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (t_alt) CLC_HIP(hipMemcpyAsync(t_alt, bt.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  for (int i = 0; i < 6; ++i)
    if (host_real[i]) CLC_HIP(hipMemcpyAsync(host_real[i], dev_real[i], n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (ambiguous) CLC_HIP(hipMemcpyAsync(ambiguous, bamb.p, n, hipMemcpyDeviceToHost, h->stream));
  if (better) CLC_HIP(hipMemcpyAsync(better, bbet.p, n, hipMemcpyDeviceToHost, h->stream));
  if (summaries_alt) CLC_HIP(hipMemcpyAsync(summaries_alt, bsum.p, n * sizeof(clc_summary), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  if (summaries_alt) {
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (size_t k = 0; k < n; ++k) summaries_alt[k].solve_ms = ms;
  }
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
  // the options first: their refusals need no device
  CLC_TRY(camera_check(cam, who));
  clc_options opt;
  CLC_TRY(pose_options(opt_in, &opt, who));
  clc_alt_pose_options ao;
  CLC_TRY(alt_options(aopt_in, &ao, who));
  if (!h || (n_images > 0 && (!offsets_dev || !q_in_wxyz_dev || !t_in_dev || !status_in_dev || !kind_dev)))
    return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_alternate_device: bad argument");
  if (n_images == 0) return CLC_OK;
  if (n_images > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_alternate_device: too many images");
  CLC_HIP(hipSetDevice(h->device));
  long long ends[2];  // the corner range, as clc_board_poses_device reads it
  CLC_HIP(hipMemcpyAsync(&ends[0], offsets_dev, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(&ends[1], offsets_dev + n_images, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  if (ends[1] < ends[0] || ends[0] < 0) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_alternate_device: offsets not monotone");
  const size_t M = (size_t)(ends[1] - ends[0]);
  if (M > 0 && (!corners_px_dev || !board_xy_dev)) return fail(CLC_ERR_INVALID_ARG, "clc_board_poses_alternate_device: bad argument");
  DevBuf<float> bl(&h->pool), bsl(&h->pool), bsb(&h->pool);
  DevBuf<int32_t> bcnt(&h->pool), bflag(&h->pool);
  DevBuf<double> bst7(&h->pool);
  CLC_HIP(bl.alloc(2 * M)); CLC_HIP(bsl.alloc(2 * M)); CLC_HIP(bsb.alloc(2 * M)); CLC_HIP(bcnt.alloc(n_images));
  CLC_HIP(bflag.alloc(n_images)); CLC_HIP(bst7.alloc(7 * n_images));
  const AltIn in{inlier_dev, q_in_wxyz_dev, t_in_dev, status_in_dev};
  const clc::ap::AltOut out{q_alt_wxyz_dev, t_alt_dev, rms_alt_dev, cost_in_dev, cost_alt_dev, ratio_dev, rot_angle_dev, normal_angle_dev,
                            kind_dev, ambiguous_dev, better_dev, summaries_alt_dev};
  CLC_HIP(launch_board_poses_alternate(h, *cam, opt, ao, corners_px_dev, board_xy_dev, reinterpret_cast<const long long*>(offsets_dev),
                                       ends[0], M, n_images, in, bl.p, bsl.p, bsb.p, bcnt.p, bflag.p, bst7.p, out));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
}

}  // extern "C"
