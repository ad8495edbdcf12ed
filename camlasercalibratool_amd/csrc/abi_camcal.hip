// abi_camcal.hip — clc_camcal_options_default, clc_camera_guess(_device), clc_camera_calibrate(_device): the camera's intrinsics from
// the board images (K19 in clc_camcal.hpp).  A unit of its own: the kernels of abi_campose.hip and abi_joint.hip are held to their
// register figures, and these are held to their own (tests/test_camcal_resources.py).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "abi_staging.hpp"
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

// K19 on device arrays, the one function under both forms.  `a` arrives with the call's arrays named by the form and a.n_images, the
// images from the first problem's first image on; here it gets the options and the per-image workspace of n_images rows, scratch of
// the call.  One workgroup per problem on the handle's stream.
void enqueue_camcal(Staging& st, const clc_options& opt, const clc_camcal_options& co, cc::CalArgs a, size_t n_images, size_t n_problems) {
  a.opt = opt;
  a.sigma_px = co.sigma_px;
  a.hold_mask = co.hold_mask;
  a.hold_board_poses = co.hold_board_poses ? 1 : 0;
  a.ws = st.scratch<cc::CalImage>(n_images);
  if (!st.ok()) return;
  hipLaunchKernelGGL(cc::camcal_kernel, dim3((unsigned)n_problems), dim3(cc::CAL_THREADS), 0, st.stream(), a);
  st.launched();
}

// The device half of the closed-form start on device arrays (off absolute, image 0 of the call first), then the host's half.
int guess_on_device(Staging& st, const char* who, int32_t model, int32_t width, int32_t height, const float* px_dev, const float* board_dev,
                    const long long* off_dev, size_t n, clc_camera* cam_out, int32_t* n_used) {
  std::vector<double> H(9 * n);
  std::vector<int32_t> status(n);
  double* H_dev = st.out(H.data(), 9 * n);
  int32_t* status_dev = st.out(status.data(), n);
  const double cx0 = 0.5 * (double)width, cy0 = 0.5 * (double)height;
  if (st.ok()) {
    hipLaunchKernelGGL(cc::homography_kernel, dim3((unsigned)n), dim3(64), 0, st.stream(), px_dev, board_dev, off_dev, cx0, cy0, H_dev,
                       status_dev);
    st.launched();
  }
  CLC_TRY(st.finish(who));
  int32_t used = 0;
  const double f = cc::guess_focal(H.data(), status.data(), (long long)n, &used);
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
  Staging st(h);
  const float* corners_dev = st.in(M > 0 ? corners_px + 2 * offsets[0] : nullptr, 2 * M);
  const float* board_dev = st.in(M > 0 ? board_xy + 2 * offsets[0] : nullptr, 2 * M);
  const long long* off_dev = st.in(rel.data(), n_images + 1);
  return guess_on_device(st, who, model, width, height, corners_dev, board_dev, off_dev, n_images, cam_out, n_used);
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
  Staging st(h);
  return guess_on_device(st, who, model, width, height, corners_px_dev, board_xy_dev, reinterpret_cast<const long long*>(offsets_dev),
                         n_images, cam_out, n_used);
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
  CLC_TRY(problem_count_checks(who, n_images, problem_offsets != nullptr, n_problems));
  std::vector<long long> crel;
  size_t M = 0;
  CLC_TRY(host_offsets(who, corner_offsets, n_images, true, nullptr, &crel, &M));
  CLC_TRY(host_problem_offsets(who, problem_offsets, n_problems, n_images));
  if (!h || (M > 0 && (!corners_px || !board_xy))) return fail(CLC_ERR_INVALID_ARG, "clc_camera_calibrate: bad argument");
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = Clock::now();
  const size_t n = n_images, np = n_problems;
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  const std::vector<int32_t> not_kept(n, CLC_CAMCAL_NOT_KEPT);  // the status of the images outside every problem
  Staging st(h);
  cc::CalArgs a{};
  a.corners = st.in(M > 0 ? corners_px + 2 * corner_offsets[0] : nullptr, 2 * M);
  a.board = st.in(M > 0 ? board_xy + 2 * corner_offsets[0] : nullptr, 2 * M);
  a.coff = st.in(crel.data(), n > 0 ? n + 1 : 0);  // (a call without images sends no offsets)
  a.keep = st.in_opt(keep, n);
  // the device indexes the per-image arrays by the absolute image index and the workspace from the first problem's first image:
  // the host arrays start at image 0, so the offsets go down as they are and the call covers [problem_offsets[0], n)
  a.prob_off = st.in_opt(reinterpret_cast<const long long*>(problem_offsets), np + 1);
  a.n_images = (long long)n - (problem_offsets ? (long long)problem_offsets[0] : 0);
  a.q = st.inout(q_ca_wxyz, 4 * n);
  a.t = st.inout(t_ca, 3 * n);
  a.status = st.inout(image_status, n, not_kept.data());
  a.cams = st.inout(cams, np);
  a.summaries = st.out(summaries, np);
  a.H_cam = st.out_opt(H_cam, 64 * np);
  a.rms = st.out_opt(rms_px, np);
  enqueue_camcal(st, opt, co, a, n, np);
  CLC_TRY(st.finish(who));
  stamp_solve_ms(summaries, np, t0);
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
  CLC_TRY(problem_count_checks(who, n_images, problem_offsets_dev != nullptr, n_problems));
  if (n_problems == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  cc::CalArgs a{};
  a.corners = corners_px_dev;
  a.board = board_xy_dev;
  a.coff = reinterpret_cast<const long long*>(corner_offsets_dev);
  a.keep = keep_dev;
  a.prob_off = reinterpret_cast<const long long*>(problem_offsets_dev);
  a.n_images = (long long)n_images;
  a.q = q_ca_wxyz_dev;
  a.t = t_ca_dev;
  a.status = image_status_dev;
  a.cams = cams_dev;
  a.summaries = summaries_dev;
  a.H_cam = H_cam_dev;
  a.rms = rms_px_dev;
  enqueue_camcal(st, opt, co, a, n_images, n_problems);
  return st.finish(who);
}

}  // extern "C"
