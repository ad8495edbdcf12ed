// abi_subpix.hip — clc_subpix_options_default, clc_corner_subpix(_device): sub-pixel corner refinement (K24 in clc_subpix.hpp).
// A unit of its own, held to its own register figures (tests/test_subpix_resources.py).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "abi_staging.hpp"
#include "clc_subpix.hpp"

using namespace clc_abi;

namespace {

namespace sp = clc::sp;

// What both forms refuse alike ahead of the handle and the offsets, in one order; then the options as the kernel takes them.
int subpix_checks(const char* who, bool required, const clc_subpix_options* in, int32_t width, int32_t height,
                  int64_t pitch, size_t n_images, sp::SubpixModel* m) {
  const std::string w(who);
  clc_subpix_options o;
  if (in) o = *in; else clc_subpix_options_default(&o, 0);
  if (o.win_x < 1 || o.win_x > CLC_SUBPIX_MAX_WIN || o.win_y < 1 || o.win_y > CLC_SUBPIX_MAX_WIN)
    return fail(CLC_ERR_INVALID_ARG, (w + ": the half-window must be in [1, 15]").c_str());
  if (o.max_iter < 1 || o.max_iter > 100) return fail(CLC_ERR_INVALID_ARG, (w + ": max_iter must be in [1, 100]").c_str());
  if (!(std::isfinite(o.eps) && o.eps >= 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": eps must be finite and >= 0").c_str());
  if (o.reserved != 0) return fail(CLC_ERR_INVALID_ARG, (w + ": reserved must be 0").c_str());
  if (width < 1 || height < 1) return fail(CLC_ERR_INVALID_ARG, (w + ": width and height must be >= 1").c_str());
  if (pitch < (int64_t)width) return fail(CLC_ERR_INVALID_ARG, (w + ": pitch must be >= width").c_str());
  if (n_images > 0x7FFFFFFFull || (n_images > 0 && pitch > (int64_t)(0x7FFFFFFFFFFFFFFFull / n_images / (uint64_t)height)))
    return fail(CLC_ERR_INVALID_ARG, (w + ": too many images").c_str());
  if (!required) return fail(CLC_ERR_INVALID_ARG, (w + ": bad argument").c_str());
  *m = sp::subpix_model(o);
  return CLC_OK;
}

// K24 on device arrays: the mask tables up, then one wave per corner.
void enqueue_subpix(Staging& st, const sp::SubpixModel& m, const uint8_t* images, int32_t width, int32_t height, int64_t pitch,
                    size_t n_images, const float* in, const int64_t* off, long long first, size_t n_corners, float* out, int32_t* status,
                    int32_t* iterations, double* strength) {
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  sp::SubpixArgs a{};
  a.wx = m.wx; a.wy = m.wy; a.zx = m.zx; a.zy = m.zy; a.max_iter = m.max_iter; a.width = width; a.height = height;
  a.eps2 = m.eps2; a.mask_sum = m.mask_sum; a.pitch = (long long)pitch; a.images = images;
  a.vx = st.in(m.vx, (size_t)(2 * m.wx + 1));
  a.vy = st.in(m.vy, (size_t)(2 * m.wy + 1));
  a.in = in; a.off = reinterpret_cast<const long long*>(off); a.first = first; a.n_corners = (long long)n_corners;
  a.n_images = (long long)n_images; a.out = out; a.status = status; a.iterations = iterations; a.strength = strength;
  if (!st.ok()) return;
  hipLaunchKernelGGL(sp::corner_subpix_kernel, dim3((unsigned)n_corners), dim3(64), 0, st.stream(), a);
  st.launched();
}

int count_check(const char* who, size_t n_corners) {
  if (n_corners > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": too many corners").c_str());
  return CLC_OK;
}

}  // namespace

extern "C" {

void clc_subpix_options_default(clc_subpix_options* o, int32_t win) {
  if (!o) return;
  o->win_x = o->win_y = win > 0 ? win : 3;  // src/calcCamPose.cpp:87: the Kalibr call; :21: 11 on the chessboard
  o->zero_x = o->zero_y = -1;
  o->max_iter = 30;  // TermCriteria(EPS + MAX_ITER, 30, 0.1)
  o->reserved = 0;
  o->eps = 0.1;
}

int clc_corner_subpix(clc_handle* h, const clc_subpix_options* sopt, const uint8_t* images, int32_t width, int32_t height, int64_t pitch,
                      size_t n_images, const float* corners_in, const int64_t* offsets, float* corners_out, int32_t* status,
                      int32_t* iterations, double* strength) {
  const char* who = "clc_corner_subpix";
  sp::SubpixModel m;
  CLC_TRY(subpix_checks(who, n_images == 0 || (images && corners_in && offsets && corners_out), sopt, width, height, pitch, n_images, &m));
  std::vector<long long> rel;
  size_t M = 0;
  CLC_TRY(host_offsets(who, offsets, n_images, true, nullptr, &rel, &M));
  CLC_TRY(count_check(who, M));
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_corner_subpix: bad argument");
  if (n_images == 0 || M == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const long long first = (long long)offsets[0];
  Staging st(h);
  const uint8_t* img_dev = st.in(images, n_images * (size_t)height * (size_t)pitch);
  const float* in_dev = st.in(corners_in + 2 * first, 2 * M);
  const long long* off_dev = st.in(rel.data(), rel.size());
  float* out_dev = st.out(corners_out + 2 * first, 2 * M);
  int32_t* status_dev = st.out_opt(status ? status + first : nullptr, M);
  int32_t* iter_dev = st.out_opt(iterations ? iterations + first : nullptr, M);
  double* strength_dev = st.out_opt(strength ? strength + first : nullptr, M);
  enqueue_subpix(st, m, img_dev, width, height, pitch, n_images, in_dev, reinterpret_cast<const int64_t*>(off_dev), 0, M, out_dev, status_dev,
                 iter_dev, strength_dev);
  return st.finish(who);
}

int clc_corner_subpix_device(clc_handle* h, const clc_subpix_options* sopt, const uint8_t* images_dev, int32_t width, int32_t height,
                             int64_t pitch, size_t n_images, const float* corners_in_dev, const int64_t* offsets_dev,
                             float* corners_out_dev, int32_t* status_dev, int32_t* iterations_dev, double* strength_dev) {
  const char* who = "clc_corner_subpix_device";
  sp::SubpixModel m;
  CLC_TRY(subpix_checks(who, n_images == 0 || (images_dev && corners_in_dev && offsets_dev && corners_out_dev), sopt, width, height, pitch,
                        n_images, &m));
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_corner_subpix_device: bad argument");
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  long long ends[2];
  CLC_TRY(device_offset_ends(h, who, offsets_dev, n_images, ends));
  const size_t M = (size_t)(ends[1] - ends[0]);
  CLC_TRY(count_check(who, M));
  if (M == 0) return CLC_OK;
  Staging st(h);
  enqueue_subpix(st, m, images_dev, width, height, pitch, n_images, corners_in_dev, offsets_dev, ends[0], M, corners_out_dev, status_dev,
                 iterations_dev, strength_dev);
  return st.finish(who);
}

}  // extern "C"
