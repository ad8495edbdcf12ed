// abi_camcal.hip — clc_camcal_options_default, clc_camera_guess(_device), clc_camera_calibrate(_device): the camera's intrinsics from
// the board images (K19 in clc_camcal.hpp).  A unit of its own: the kernels of abi_campose.hip and abi_joint.hip are held to their
// register figures, and these are held to their own (tests/test_camcal_resources.py).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "clc_camcal.hpp"

using namespace clc_abi;

namespace {

namespace cc = clc::cc;

// The calibration's options: the caller's or the defaults for `model`; checked.
int camcal_options(const clc_camcal_options* in, int32_t model, clc_camcal_options* o, const char* who) {
  if (in) *o = *in; else clc_camcal_options_default(o, model);
  const std::string w(who);
  if (!(std::isfinite(o->sigma_px) && o->sigma_px > 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": sigma_px must be finite and > 0").c_str());
  if (o->hold_mask > 0xFFu) return fail(CLC_ERR_INVALID_ARG, (w + ": hold_mask has bits beyond the 8 intrinsics").c_str());
  if (o->hold_mask == 0xFFu && o->hold_board_poses) return fail(CLC_ERR_INVALID_ARG, (w + ": everything is held").c_str());
  return CLC_OK;
}

cc::CalArgs base_args(const clc_options& opt, const clc_camcal_options& co) {
  cc::CalArgs a{};
  a.opt = opt;
  a.sigma_px = co.sigma_px;
  a.hold_mask = co.hold_mask;
  a.hold_board_poses = co.hold_board_poses ? 1 : 0;
  return a;
}

hipError_t launch_camcal(clc_handle* h, const cc::CalArgs& a, size_t n_problems) {
  hipLaunchKernelGGL(cc::camcal_kernel, dim3((unsigned)n_problems), dim3(cc::CAL_THREADS), 0, h->stream, a);
  return hipGetLastError();
}

// The device half of the closed-form start on device arrays (off absolute, image 0 of the call first), then the host's half.
int guess_on_device(clc_handle* h, const char* who, int32_t model, int32_t width, int32_t height, const float* px_dev,
                    const float* board_dev, const long long* off_dev, size_t n, clc_camera* cam_out, int32_t* n_used) {
  DevBuf<double> bH(&h->pool);
  DevBuf<int32_t> bs(&h->pool);
  CLC_HIP(bH.alloc(9 * n));
  CLC_HIP(bs.alloc(n));
  const double cx0 = 0.5 * (double)width, cy0 = 0.5 * (double)height;
  hipLaunchKernelGGL(cc::homography_kernel, dim3((unsigned)n), dim3(64), 0, h->stream, px_dev, board_dev, off_dev, cx0, cy0, bH.p, bs.p);
  CLC_HIP(hipGetLastError());
  std::vector<double> H(9 * n);
  std::vector<int32_t> st(n);
  CLC_HIP(hipMemcpyAsync(H.data(), bH.p, 9 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(st.data(), bs.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  int32_t used = 0;
  const double f = cc::guess_focal(H.data(), st.data(), (long long)n, &used);
  if (n_used) *n_used = used;
  if (!(f == f)) return fail(CLC_ERR_LINALG, (std::string(who) + ": no focal length from these images (fewer than 2 usable, or 1/f^2 not positive)").c_str());
  cam_out->model = model;
  cam_out->reserved = 0;
  cam_out->proj[0] = cam_out->proj[1] = f;
  cam_out->proj[2] = cx0;
  cam_out->proj[3] = cy0;
  for (int i = 0; i < 4; ++i) cam_out->dist[i] = 0.0;
  return CLC_OK;
}

int guess_check(const char* who, clc_handle* h, int32_t model, int32_t width, int32_t height, const void* off, size_t n, clc_camera* cam_out) {
  if (!known_model(model)) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": unknown camera model").c_str());
  if (width <= 0 || height <= 0) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": width and height must be > 0").c_str());
  if (!h || !cam_out || (n > 0 && !off) || n > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": bad argument").c_str());
  return CLC_OK;
}

}  // namespace

extern "C" {

void clc_camcal_options_default(clc_camcal_options* o, int32_t model) {
  if (!o) return;
  o->sigma_px = 0.3;  // the corner noise of the project's simulations
  o->hold_mask = model == CLC_CAMERA_KANNALA_BRANDT ? (1u << 6) | (1u << 7) : 0u;
  o->hold_board_poses = 0;
}

int clc_camera_guess(clc_handle* h, int32_t model, int32_t width, int32_t height, const float* corners_px, const float* board_xy,
                     const int64_t* offsets, size_t n_images, clc_camera* cam_out, int32_t* n_used) {
  const char* who = "clc_camera_guess";
  CLC_TRY(guess_check(who, h, model, width, height, offsets, n_images, cam_out));
  std::vector<long long> rel;
  size_t M = 0;
  CLC_TRY(host_offsets(who, offsets, n_images, true, nullptr, &rel, &M));
  if (M > 0 && (!corners_px || !board_xy)) return fail(CLC_ERR_INVALID_ARG, "clc_camera_guess: bad argument");
  if (n_used) *n_used = 0;
  if (n_images < 2) return fail(CLC_ERR_LINALG, "clc_camera_guess: fewer than 2 images");
  CLC_HIP(hipSetDevice(h->device));
  DevBuf<float> bc(&h->pool), bb(&h->pool);
  DevBuf<long long> bo(&h->pool);
  CLC_HIP(bc.alloc(2 * M)); CLC_HIP(bb.alloc(2 * M)); CLC_HIP(bo.alloc(n_images + 1));
  if (M > 0) {
    CLC_HIP(hipMemcpyAsync(bc.p, corners_px + 2 * offsets[0], 2 * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bb.p, board_xy + 2 * offsets[0], 2 * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
  }
  CLC_HIP(hipMemcpyAsync(bo.p, rel.data(), (n_images + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  return guess_on_device(h, who, model, width, height, bc.p, bb.p, bo.p, n_images, cam_out, n_used);
}

int clc_camera_guess_device(clc_handle* h, int32_t model, int32_t width, int32_t height, const float* corners_px_dev,
                            const float* board_xy_dev, const int64_t* offsets_dev, size_t n_images, clc_camera* cam_out,
                            int32_t* n_used) {
  const char* who = "clc_camera_guess_device";
  CLC_TRY(guess_check(who, h, model, width, height, offsets_dev, n_images, cam_out));
  if (n_images > 0 && (!corners_px_dev || !board_xy_dev)) return fail(CLC_ERR_INVALID_ARG, "clc_camera_guess_device: bad argument");
  if (n_used) *n_used = 0;
  if (n_images < 2) return fail(CLC_ERR_LINALG, "clc_camera_guess_device: fewer than 2 images");
  CLC_HIP(hipSetDevice(h->device));
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  return guess_on_device(h, who, model, width, height, corners_px_dev, board_xy_dev, reinterpret_cast<const long long*>(offsets_dev), n_images,
                         cam_out, n_used);
}

int clc_camera_calibrate(clc_handle* h, const clc_options* opt_in, const clc_camcal_options* copt_in, const float* corners_px,
                         const float* board_xy, const int64_t* corner_offsets, const uint8_t* keep, size_t n_images,
                         const int64_t* problem_offsets, size_t n_problems, clc_camera* cams, double* q_ca_wxyz, double* t_ca,
                         clc_summary* summaries, double* H_cam, double* rms_px, int32_t* image_status) {
  const char* who = "clc_camera_calibrate";
  // everything that can be refused without the device first
  clc_options opt;
  CLC_TRY(pose_options(opt_in, &opt, who));
  if ((n_images > 0 && (!corner_offsets || !q_ca_wxyz || !t_ca || !image_status)) || (n_problems > 0 && (!cams || !summaries)))
    return fail(CLC_ERR_INVALID_ARG, "clc_camera_calibrate: bad argument");
  for (size_t k = 0; k < n_problems; ++k)
    if (!known_model(cams[k].model)) return fail(CLC_ERR_INVALID_ARG, "clc_camera_calibrate: unknown camera model");
  clc_camcal_options co;
  CLC_TRY(camcal_options(copt_in, n_problems > 0 ? cams[0].model : CLC_CAMERA_PINHOLE, &co, who));
  if (n_images > 0x7FFFFFFFull || n_problems > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_camera_calibrate: too many images");
  if (!problem_offsets && n_problems > 1) return fail(CLC_ERR_INVALID_ARG, "clc_camera_calibrate: bad argument");
  std::vector<long long> crel, orel;
  size_t M = 0, span = 0;
  CLC_TRY(host_offsets(who, corner_offsets, n_images, true, nullptr, &crel, &M));
  if (problem_offsets) {
    CLC_TRY(host_offsets(who, problem_offsets, n_problems, true, nullptr, &orel, &span));
    if (n_problems > 0 && (size_t)problem_offsets[n_problems] > n_images)
      return fail(CLC_ERR_INVALID_ARG, "clc_camera_calibrate: problem_offsets beyond n_images");
  }
  if (!h || (M > 0 && (!corners_px || !board_xy))) return fail(CLC_ERR_INVALID_ARG, "clc_camera_calibrate: bad argument");
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  const size_t n = n_images, np = n_problems;
  DevBuf<float> bc(&h->pool), bb(&h->pool);
  DevBuf<long long> bco(&h->pool), bpr(&h->pool);
  DevBuf<double> bq(&h->pool), bt(&h->pool), bH(&h->pool), brms(&h->pool);
  DevBuf<unsigned char> bk(&h->pool);
  DevBuf<int32_t> bs(&h->pool);
  DevBuf<clc_summary> bsum(&h->pool);
  DevBuf<clc_camera> bcam(&h->pool);
  DevBuf<cc::CalImage> bws(&h->pool);
  CLC_HIP(bc.alloc(2 * M)); CLC_HIP(bb.alloc(2 * M)); CLC_HIP(bco.alloc(n + 1)); CLC_HIP(bq.alloc(4 * n)); CLC_HIP(bt.alloc(3 * n));
  CLC_HIP(bs.alloc(n)); CLC_HIP(bcam.alloc(np)); CLC_HIP(bsum.alloc(np)); CLC_HIP(bws.alloc(n));
  if (keep) CLC_HIP(bk.alloc(n));
  if (problem_offsets) CLC_HIP(bpr.alloc(np + 1));
  if (H_cam) CLC_HIP(bH.alloc(64 * np));
  if (rms_px) CLC_HIP(brms.alloc(np));
  if (M > 0) {
    CLC_HIP(hipMemcpyAsync(bc.p, corners_px + 2 * corner_offsets[0], 2 * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bb.p, board_xy + 2 * corner_offsets[0], 2 * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
  }
  std::vector<int32_t> st0(n, CLC_CAMCAL_NOT_KEPT);  // images outside every problem
  if (n > 0) {
    CLC_HIP(hipMemcpyAsync(bco.p, crel.data(), (n + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bq.p, q_ca_wxyz, 4 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bt.p, t_ca, 3 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bs.p, st0.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (keep) CLC_HIP(hipMemcpyAsync(bk.p, keep, n, hipMemcpyHostToDevice, h->stream));
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  // the device indexes the per-image arrays by the absolute image index and the workspace from the first problem's first image:
  // the host arrays start at image 0, so the offsets go down as they are and the workspace covers [problem_offsets[0], n)
  if (problem_offsets)
    CLC_HIP(hipMemcpyAsync(bpr.p, problem_offsets, (np + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(bcam.p, cams, np * sizeof(clc_camera), hipMemcpyHostToDevice, h->stream));
  cc::CalArgs a = base_args(opt, co);
  a.corners = bc.p; a.board = bb.p; a.coff = bco.p; a.keep = keep ? bk.p : nullptr; a.prob_off = problem_offsets ? bpr.p : nullptr;
  a.n_images = (long long)n - (problem_offsets ? (long long)problem_offsets[0] : 0);
  a.q = bq.p; a.t = bt.p; a.cams = bcam.p; a.summaries = bsum.p; a.H_cam = H_cam ? bH.p : nullptr; a.rms = rms_px ? brms.p : nullptr;
  a.status = bs.p; a.ws = bws.p;
  CLC_HIP(launch_camcal(h, a, np));
  if (n > 0) {
    CLC_HIP(hipMemcpyAsync(q_ca_wxyz, bq.p, 4 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CLC_HIP(hipMemcpyAsync(t_ca, bt.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CLC_HIP(hipMemcpyAsync(image_status, bs.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  }
  CLC_HIP(hipMemcpyAsync(cams, bcam.p, np * sizeof(clc_camera), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(summaries, bsum.p, np * sizeof(clc_summary), hipMemcpyDeviceToHost, h->stream));
  if (H_cam) CLC_HIP(hipMemcpyAsync(H_cam, bH.p, 64 * np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (rms_px) CLC_HIP(hipMemcpyAsync(rms_px, brms.p, np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (size_t k = 0; k < np; ++k) summaries[k].solve_ms = ms;
  return CLC_OK;
}

int clc_camera_calibrate_device(clc_handle* h, const clc_options* opt_in, const clc_camcal_options* copt_in, const float* corners_px_dev,
                                const float* board_xy_dev, const int64_t* corner_offsets_dev, const uint8_t* keep_dev, size_t n_images,
                                const int64_t* problem_offsets_dev, size_t n_problems, clc_camera* cams_dev, double* q_ca_wxyz_dev,
                                double* t_ca_dev, clc_summary* summaries_dev, double* H_cam_dev, double* rms_px_dev,
                                int32_t* image_status_dev) {
  const char* who = "clc_camera_calibrate_device";
  clc_options opt;
  CLC_TRY(pose_options(opt_in, &opt, who));
  clc_camcal_options co;
  CLC_TRY(camcal_options(copt_in, CLC_CAMERA_PINHOLE, &co, who));
  if (!h || (n_images > 0 && (!corner_offsets_dev || !q_ca_wxyz_dev || !t_ca_dev || !image_status_dev || !corners_px_dev || !board_xy_dev)) ||
      (n_problems > 0 && (!cams_dev || !summaries_dev)))
    return fail(CLC_ERR_INVALID_ARG, "clc_camera_calibrate_device: bad argument");
  if (n_images > 0x7FFFFFFFull || n_problems > 0x7FFFFFFFull)
    return fail(CLC_ERR_INVALID_ARG, "clc_camera_calibrate_device: too many images");
  if (!problem_offsets_dev && n_problems > 1) return fail(CLC_ERR_INVALID_ARG, "clc_camera_calibrate_device: bad argument");
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  DevBuf<cc::CalImage> bws(&h->pool);
  CLC_HIP(bws.alloc(n_images));
  cc::CalArgs a = base_args(opt, co);
  a.corners = corners_px_dev; a.board = board_xy_dev; a.coff = reinterpret_cast<const long long*>(corner_offsets_dev);
  a.keep = keep_dev; a.prob_off = reinterpret_cast<const long long*>(problem_offsets_dev); a.n_images = (long long)n_images;
  a.q = q_ca_wxyz_dev; a.t = t_ca_dev; a.cams = cams_dev; a.summaries = summaries_dev; a.H_cam = H_cam_dev; a.rms = rms_px_dev;
  a.status = image_status_dev; a.ws = bws.p;
  CLC_HIP(launch_camcal(h, a, n_problems));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
}

}  // extern "C"
