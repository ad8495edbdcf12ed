// abi_subpix.hip — clc_subpix_options_default, clc_corner_subpix(_device): sub-pixel corner refinement (K24 in clc_subpix.hpp).
// A unit of its own, held to its own register figures (tests/test_subpix_resources.py).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "abi_imagecall.hpp"
#include "clc_subpix.hpp"

using namespace clc_abi;

namespace {

// What both forms refuse alike ahead of the handle and the offsets, in one order; then the options with the defaults filled in.
int subpix_checks(const char* who, bool required, const clc_subpix_options* in, int32_t width, int32_t height, int64_t pitch, size_t n_images,
                  clc_subpix_options* o) {
  if (in) *o = *in; else clc_subpix_options_default(o, 0);
  if (const char* fault = subpix_options_fault(*o)) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": " + fault).c_str());
  CLC_TRY(image_geometry_check(who, width, height, pitch, n_images));
  if (!required) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": bad argument").c_str());
  return CLC_OK;
}

}  // namespace

// K24 on device arrays, for this unit's two forms and for the calls of other units that end in it (declared in abi_imagecall.hpp).
void clc_abi::enqueue_subpix_refinement(Staging& st, const clc_subpix_options& o, const uint8_t* images, int32_t width, int32_t height,
                                        int64_t pitch, size_t n_images, const float* in, const int64_t* off, long long first, size_t n_corners,
                                        float* out, int32_t* status, int32_t* iterations, double* strength) {
  namespace sp = clc::sp;
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  const sp::SubpixModel m = sp::subpix_model(o);
  sp::SubpixArgs a{};
  a.wx = m.wx; a.wy = m.wy; a.zx = m.zx; a.zy = m.zy; a.max_iter = m.max_iter; a.width = width; a.height = height;
  a.eps2 = m.eps2; a.mask_sum = m.mask_sum; a.pitch = (long long)pitch; a.images = images;
  a.vx = st.in_owned(std::vector<float>(m.vx, m.vx + 2 * m.wx + 1));
  a.vy = st.in_owned(std::vector<float>(m.vy, m.vy + 2 * m.wy + 1));
  a.in = in; a.off = reinterpret_cast<const long long*>(off); a.first = first; a.n_corners = (long long)n_corners;
  a.n_images = (long long)n_images; a.out = out; a.status = status; a.iterations = iterations; a.strength = strength;
  if (!st.ok()) return;
  hipLaunchKernelGGL(sp::corner_subpix_kernel, dim3((unsigned)n_corners), dim3(64), 0, st.stream(), a);
  st.launched();
}

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
  clc_subpix_options o;
  CLC_TRY(subpix_checks(who, n_images == 0 || (images && corners_in && offsets && corners_out), sopt, width, height, pitch, n_images, &o));
  std::vector<long long> rel;
  size_t M = 0;
  CLC_TRY(host_offsets(who, offsets, n_images, true, nullptr, &rel, &M));
  CLC_TRY(corner_count_check(who, M));
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
  enqueue_subpix_refinement(st, o, img_dev, width, height, pitch, n_images, in_dev, reinterpret_cast<const int64_t*>(off_dev), 0, M, out_dev,
                            status_dev, iter_dev, strength_dev);
  return st.finish(who);
}

int clc_corner_subpix_device(clc_handle* h, const clc_subpix_options* sopt, const uint8_t* images_dev, int32_t width, int32_t height,
                             int64_t pitch, size_t n_images, const float* corners_in_dev, const int64_t* offsets_dev,
                             float* corners_out_dev, int32_t* status_dev, int32_t* iterations_dev, double* strength_dev) {
  const char* who = "clc_corner_subpix_device";
  clc_subpix_options o;
  CLC_TRY(subpix_checks(who, n_images == 0 || (images_dev && corners_in_dev && offsets_dev && corners_out_dev), sopt, width, height, pitch,
                        n_images, &o));
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_corner_subpix_device: bad argument");
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  long long ends[2];
  CLC_TRY(device_offset_ends(h, who, offsets_dev, n_images, ends));
  const size_t M = (size_t)(ends[1] - ends[0]);
  CLC_TRY(corner_count_check(who, M));
  if (M == 0) return CLC_OK;
  Staging st(h);
  enqueue_subpix_refinement(st, o, images_dev, width, height, pitch, n_images, corners_in_dev, offsets_dev, ends[0], M, corners_out_dev,
                            status_dev, iterations_dev, strength_dev);
  return st.finish(who);
}

}  // extern "C"
