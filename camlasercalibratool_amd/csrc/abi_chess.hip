// abi_chess.hip — clc_chess_options_default, clc_chess_corners(_device), clc_chessorder_options_default, clc_chessboard_order,
// clc_find_chessboard: chessboard corners from images (K25: the kernels in clc_chess.hpp, the host ordering in clc_chessorder.hpp);
// clc_chessboard_order_device, clc_find_chessboard_device, clc_find_chessboard_gpu: the ordering on the device (K26: clc_boardorder.hpp).
// A unit of its own, held to its own register figures (tests/test_chess_resources.py).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "abi_imagecall.hpp"
#include "clc_chess.hpp"
#include "clc_chessorder.hpp"
#include "clc_boardorder.hpp"

using namespace clc_abi;

namespace ch = clc::chess;

// K25's checks and enqueue, for this unit and for the unit that builds on its candidates (abi_tags.hip; declared in abi_imagecall.hpp).
// What both detection forms refuse alike ahead of the handle, in one order; then the options with the defaults filled in.
int clc_abi::chess_checks(const char* who, bool required, const clc_chess_options* in, int32_t width, int32_t height, int64_t pitch,
                          size_t n_images, clc_chess_options* o) {
  const std::string w(who);
  if (in) *o = *in; else clc_chess_options_default(o);
  if (o->threshold < 1) return fail(CLC_ERR_INVALID_ARG, (w + ": threshold must be >= 1").c_str());
  if (o->nms_radius < 1 || o->nms_radius > ch::MAX_R) return fail(CLC_ERR_INVALID_ARG, (w + ": nms_radius must be in [1, 7]").c_str());
  if (o->rel_permille < 0 || o->rel_permille > 1000) return fail(CLC_ERR_INVALID_ARG, (w + ": rel_permille must be in [0, 1000]").c_str());
  if (o->max_per_image < 1 || o->max_per_image > CLC_CHESS_MAX_CANDIDATES)
    return fail(CLC_ERR_INVALID_ARG, (w + ": max_per_image must be in [1, 1024]").c_str());
  if (o->reserved != 0) return fail(CLC_ERR_INVALID_ARG, (w + ": reserved must be 0").c_str());
  CLC_TRY(image_geometry_check(who, width, height, pitch, n_images));
  const uint64_t tiles = (((uint64_t)width + ch::TILE_W - 1) / ch::TILE_W) * (((uint64_t)height + ch::TILE_H - 1) / ch::TILE_H);
  if (tiles > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, (w + ": the image is too large").c_str());
  if (!required) return fail(CLC_ERR_INVALID_ARG, (w + ": bad argument").c_str());
  return CLC_OK;
}

// K25 on device arrays: per chunk of images the counters to zero, one workgroup per tile, one wave per image.
void clc_abi::enqueue_chess(Staging& st, const clc_chess_options& o, const uint8_t* images, int32_t width, int32_t height, int64_t pitch,
                            size_t n_images, float* cand_xy, int32_t* cand_r5, int32_t* count, int32_t* count_raw, int32_t* status) {
  static_assert(ch::RAW_CAP == CLC_CHESS_RAW_CAP, "kChessChunkImages is sized by the raw list");
  const size_t chunk = std::min(n_images, kChessChunkImages);
  ch::ChessArgs a{};
  a.width = width; a.height = height; a.threshold = o.threshold; a.nms_radius = o.nms_radius; a.rel_permille = o.rel_permille;
  a.max_per_image = o.max_per_image; a.pitch = (long long)pitch; a.n_images = (long long)n_images; a.images = images;
  a.tiles_x = ((long long)width + ch::TILE_W - 1) / ch::TILE_W;
  const long long tiles = a.tiles_x * (((long long)height + ch::TILE_H - 1) / ch::TILE_H);
  a.raw_count = st.scratch<unsigned int>(chunk);
  a.raw = st.scratch<int32_t>(chunk * (size_t)ch::RAW_CAP * 3);
  a.cand_xy = cand_xy; a.cand_r5 = cand_r5; a.count = count; a.count_raw = count_raw; a.status = status;
  const bool any_domain = width >= 2 * ch::RING + 1 && height >= 2 * ch::RING + 1;
  for (size_t first = 0; first < n_images && st.ok(); first += chunk) {
    const size_t n = std::min(chunk, n_images - first);
    a.first = (long long)first;
    st.check(hipMemsetAsync(a.raw_count, 0, n * sizeof(unsigned int), st.stream()));
    if (!st.ok()) return;
    if (any_domain) {
      hipLaunchKernelGGL(ch::chess_response_nms_kernel, dim3((unsigned)tiles, (unsigned)n), dim3(ch::THREADS), 0, st.stream(), a);
      st.launched();
      if (!st.ok()) return;
    }
    hipLaunchKernelGGL(ch::chess_select_kernel, dim3((unsigned)n), dim3(64), 0, st.stream(), a);
    st.launched();
  }
}

namespace {

int order_checks(const char* who, bool required, const clc_chessorder_options* in, int32_t cols, int32_t rows, size_t n_images, double* tol) {
  const std::string w(who);
  clc_chessorder_options o;
  if (in) o = *in; else clc_chessorder_options_default(&o);
  if (!(std::isfinite(o.tol) && o.tol > 0.0 && o.tol <= 0.5)) return fail(CLC_ERR_INVALID_ARG, (w + ": tol must be in (0, 0.5]").c_str());
  if (o.reserved != 0 || o.reserved2 != 0) return fail(CLC_ERR_INVALID_ARG, (w + ": reserved must be 0").c_str());
  if (cols < 2 || rows < 2 || (int64_t)cols * rows > CLC_CHESS_MAX_CANDIDATES)
    return fail(CLC_ERR_INVALID_ARG, (w + ": cols and rows must be >= 2 and cols x rows <= 1024").c_str());
  if (n_images > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, (w + ": too many images").c_str());
  if (!required) return fail(CLC_ERR_INVALID_ARG, (w + ": bad argument").c_str());
  *tol = o.tol;
  return CLC_OK;
}

namespace bo = clc::boardorder;

// Images per launch of the K26 kernels (the grid of one launch stays far below 2^32 threads).
constexpr size_t kOrderLaunchImages = (size_t)1 << 20;

// K26 on device arrays: one wave per image.
void enqueue_order(Staging& st, const float* cand_xy, const int32_t* count, int64_t stride, size_t n_images, int32_t cols, int32_t rows, double tol,
                   int32_t* index, int32_t* status, int32_t* n_labelings, double* worst) {
  bo::OrderArgs a{};
  a.cand_xy = cand_xy; a.count = count; a.stride = (long long)stride; a.cols = cols; a.rows = rows; a.tol = tol;
  a.index = index; a.status = status; a.n_labelings = n_labelings; a.worst = worst;
  const size_t lds = bo::lds_bytes(cols * rows);
  for (size_t first = 0; first < n_images && st.ok(); first += kOrderLaunchImages) {
    a.first = (long long)first;
    hipLaunchKernelGGL(bo::board_order_kernel, dim3((unsigned)std::min(kOrderLaunchImages, n_images - first)), dim3(bo::LANES), lds, st.stream(), a);
    st.launched();
  }
}

// The ordered candidate pixels as the refinement's starts (NaN where no board was found), found, and where asked the offsets and a
// NaN strength.
void enqueue_gather(Staging& st, const float* cand_xy, const int32_t* index, const int32_t* status, int64_t stride, size_t n_images, int32_t n,
                    float* starts, int32_t* found, int64_t* offsets, double* strength) {
  bo::GatherArgs g{};
  g.cand_xy = cand_xy; g.index = index; g.status = status; g.stride = (long long)stride; g.n_images = (long long)n_images; g.n = n;
  g.starts = starts; g.found = found; g.offsets = offsets; g.strength = strength;
  for (size_t first = 0; first < n_images && st.ok(); first += kOrderLaunchImages) {
    hipLaunchKernelGGL(bo::board_gather_kernel, dim3((unsigned)std::min(kOrderLaunchImages, n_images - first)), dim3(bo::LANES), 0, st.stream(), g,
                       (long long)first);
    st.launched();
  }
}

// What the three forms of clc_find_chessboard refuse ahead of the handle, in one order; then the options.
int find_checks(const char* who, bool required, const clc_chess_options* copt, const clc_chessorder_options* oopt, const clc_subpix_options* sopt,
                int32_t width, int32_t height, int64_t pitch, size_t n_images, int32_t cols, int32_t rows, clc_chess_options* o, double* tol) {
  const std::string w(who);
  CLC_TRY(chess_checks(who, required, copt, width, height, pitch, n_images, o));
  CLC_TRY(order_checks(who, required, oopt, cols, rows, n_images, tol));
  if ((size_t)o->max_per_image < (size_t)cols * (size_t)rows) return fail(CLC_ERR_INVALID_ARG, (w + ": max_per_image must be >= cols x rows").c_str());
  return refinement_checks(who, sopt, (uint64_t)n_images * (uint64_t)cols * (uint64_t)rows);
}

// Detection, ordering, gather and with sopt the refinement on device arrays, all enqueued on the caller's st: nothing is read back in
// between and nothing is waited for here.
void find_on_device(Staging& st, const clc_chess_options& o, double tol, const clc_subpix_options* sopt, const uint8_t* img_dev, int32_t width,
                    int32_t height, int64_t pitch, size_t n_images, int32_t cols, int32_t rows, float* corners_dev, int32_t* found_dev,
                    double* strength_dev) {
  const size_t stride = (size_t)o.max_per_image, per = (size_t)cols * (size_t)rows, M = n_images * per;
  float* xy_dev = st.scratch<float>(2 * n_images * stride);
  int32_t* count_dev = st.scratch<int32_t>(n_images);
  int32_t* status_dev = st.scratch<int32_t>(n_images);
  int32_t* index_dev = st.scratch<int32_t>(M);
  float* starts_dev = sopt ? st.scratch<float>(2 * M) : corners_dev;
  int64_t* off_dev = sopt ? st.scratch<int64_t>(n_images + 1) : nullptr;  // the gather writes them: i per
  if (st.ok()) enqueue_chess(st, o, img_dev, width, height, pitch, n_images, xy_dev, nullptr, count_dev, nullptr, status_dev);
  if (st.ok()) enqueue_order(st, xy_dev, count_dev, (int64_t)stride, n_images, cols, rows, tol, index_dev, status_dev, nullptr, nullptr);
  if (st.ok())
    enqueue_gather(st, xy_dev, index_dev, status_dev, (int64_t)stride, n_images, (int32_t)per, starts_dev, found_dev, off_dev,
                   sopt ? nullptr : strength_dev);
  // (a NaN start comes back as it is: an image without a board keeps its NaN corners)
  if (sopt && st.ok())
    enqueue_subpix_refinement(st, *sopt, img_dev, width, height, pitch, n_images, starts_dev, off_dev, 0, M, corners_dev, nullptr, nullptr,
                              strength_dev);
}

}  // namespace

extern "C" {

void clc_chess_options_default(clc_chess_options* o) {
  if (!o) return;
  o->threshold = 500;
  o->nms_radius = 3;
  o->rel_permille = 250;
  o->max_per_image = 256;
  o->reserved = 0;
}

void clc_chessorder_options_default(clc_chessorder_options* o) {
  if (!o) return;
  o->tol = 0.3;
  o->reserved = o->reserved2 = 0;
}

int clc_chess_corners(clc_handle* h, const clc_chess_options* copt, const uint8_t* images, int32_t width, int32_t height, int64_t pitch,
                      size_t n_images, float* cand_xy, int32_t* cand_r5, int32_t* count, int32_t* count_raw, int32_t* status) {
  const char* who = "clc_chess_corners";
  clc_chess_options o;
  CLC_TRY(chess_checks(who, n_images == 0 || (images && cand_xy && count && status), copt, width, height, pitch, n_images, &o));
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_chess_corners: bad argument");
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  const size_t slots = n_images * (size_t)o.max_per_image;
  const uint8_t* img_dev = st.in(images, n_images * (size_t)height * (size_t)pitch);
  float* xy_dev = st.out(cand_xy, 2 * slots);
  int32_t* r5_dev = st.out_opt(cand_r5, slots);
  int32_t* count_dev = st.out(count, n_images);
  int32_t* raw_dev = st.out_opt(count_raw, n_images);
  int32_t* status_dev = st.out(status, n_images);
  if (st.ok()) enqueue_chess(st, o, img_dev, width, height, pitch, n_images, xy_dev, r5_dev, count_dev, raw_dev, status_dev);
  return st.finish(who);
}

int clc_chess_corners_device(clc_handle* h, const clc_chess_options* copt, const uint8_t* images_dev, int32_t width, int32_t height,
                             int64_t pitch, size_t n_images, float* cand_xy_dev, int32_t* cand_r5_dev, int32_t* count_dev,
                             int32_t* count_raw_dev, int32_t* status_dev) {
  const char* who = "clc_chess_corners_device";
  clc_chess_options o;
  CLC_TRY(chess_checks(who, n_images == 0 || (images_dev && cand_xy_dev && count_dev && status_dev), copt, width, height, pitch, n_images, &o));
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_chess_corners_device: bad argument");
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  enqueue_chess(st, o, images_dev, width, height, pitch, n_images, cand_xy_dev, cand_r5_dev, count_dev, count_raw_dev, status_dev);
  return st.finish(who);
}

int clc_chessboard_order(const float* cand_xy, const int32_t* count, int64_t stride, size_t n_images, int32_t cols, int32_t rows,
                         const clc_chessorder_options* oopt, int32_t* index, int32_t* status, int32_t* n_labelings, double* worst) {
  const char* who = "clc_chessboard_order";
  double tol = 0.0;
  CLC_TRY(order_checks(who, n_images == 0 || (cand_xy && count && index && status), oopt, cols, rows, n_images, &tol));
  if (n_images > 0 && stride < (int64_t)cols * rows) return fail(CLC_ERR_INVALID_ARG, "clc_chessboard_order: stride must be >= cols x rows");
  clc::chessorder::order_images(cand_xy, count, (long long)stride, (long long)n_images, cols, rows, tol, index, status, n_labelings, worst);
  return CLC_OK;
}

int clc_find_chessboard(clc_handle* h, const clc_chess_options* copt, const clc_chessorder_options* oopt, const clc_subpix_options* sopt,
                        const uint8_t* images, int32_t width, int32_t height, int64_t pitch, size_t n_images, int32_t cols, int32_t rows,
                        float* corners, int32_t* found, double* strength) {
  const char* who = "clc_find_chessboard";
  clc_chess_options o;
  double tol = 0.0;
  CLC_TRY(find_checks(who, n_images == 0 || (images && corners && found), copt, oopt, sopt, width, height, pitch, n_images, cols, rows, &o, &tol));
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_find_chessboard: bad argument");
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const size_t stride = (size_t)o.max_per_image, per = (size_t)cols * (size_t)rows, M = n_images * per;
  std::vector<float> cand(2 * n_images * stride), starts(2 * M, std::nanf(""));
  std::vector<int32_t> count(n_images), status(n_images), index(M);
  Staging st(h);  // the images stay on the device for both stages
  const uint8_t* img_dev = st.in(images, n_images * (size_t)height * (size_t)pitch);
  float* xy_dev = st.scratch<float>(cand.size());
  int32_t* count_dev = st.scratch<int32_t>(n_images);
  int32_t* status_dev = st.scratch<int32_t>(n_images);
  if (st.ok()) enqueue_chess(st, o, img_dev, width, height, pitch, n_images, xy_dev, nullptr, count_dev, nullptr, status_dev);
  CLC_TRY(st.status(who));
  st.check(hipMemcpyAsync(cand.data(), xy_dev, cand.size() * sizeof(float), hipMemcpyDeviceToHost, st.stream()));
  st.check(hipMemcpyAsync(count.data(), count_dev, n_images * sizeof(int32_t), hipMemcpyDeviceToHost, st.stream()));
  st.check(hipMemcpyAsync(status.data(), status_dev, n_images * sizeof(int32_t), hipMemcpyDeviceToHost, st.stream()));
  st.check(hipStreamSynchronize(st.stream()));
  CLC_TRY(st.status(who));
  clc::chessorder::order_images(cand.data(), count.data(), (long long)stride, (long long)n_images, cols, rows, tol, index.data(), status.data(),
                                nullptr, nullptr);
  for (size_t i = 0; i < n_images; ++i) {
    found[i] = status[i] == CLC_CHESS_FOUND ? 1 : 0;
    if (!found[i]) continue;
    for (size_t m = 0; m < per; ++m) {
      const size_t slot = i * stride + (size_t)index[i * per + m];
      starts[2 * (i * per + m)] = cand[2 * slot];
      starts[2 * (i * per + m) + 1] = cand[2 * slot + 1];
    }
  }
  if (!sopt) {  // the integer pixels as they are
    std::copy(starts.begin(), starts.end(), corners);
    if (strength) std::fill(strength, strength + M, (double)NAN);
    return CLC_OK;
  }
  std::vector<int64_t> offsets(n_images + 1);
  for (size_t i = 0; i <= n_images; ++i) offsets[i] = (int64_t)(i * per);
  const float* starts_dev = st.in(starts.data(), starts.size());
  const int64_t* off_dev = st.in(offsets.data(), offsets.size());
  float* out_dev = st.out(corners, 2 * M);
  double* strength_dev = st.out_opt(strength, M);
  // (a NaN start comes back as it is: an image without a board keeps its NaN corners)
  enqueue_subpix_refinement(st, *sopt, img_dev, width, height, pitch, n_images, starts_dev, off_dev, 0, M, out_dev, nullptr, nullptr, strength_dev);
  return st.finish(who);
}

int clc_chessboard_order_device(clc_handle* h, const float* cand_xy_dev, const int32_t* count_dev, int64_t stride, size_t n_images, int32_t cols,
                                int32_t rows, const clc_chessorder_options* oopt, int32_t* index_dev, int32_t* status_dev,
                                int32_t* n_labelings_dev, double* worst_dev) {
  const char* who = "clc_chessboard_order_device";
  double tol = 0.0;
  CLC_TRY(order_checks(who, n_images == 0 || (cand_xy_dev && count_dev && index_dev && status_dev), oopt, cols, rows, n_images, &tol));
  if (n_images > 0 && stride < (int64_t)cols * rows) return fail(CLC_ERR_INVALID_ARG, "clc_chessboard_order_device: stride must be >= cols x rows");
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_chessboard_order_device: bad argument");
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  enqueue_order(st, cand_xy_dev, count_dev, stride, n_images, cols, rows, tol, index_dev, status_dev, n_labelings_dev, worst_dev);
  return st.finish(who);
}

int clc_find_chessboard_device(clc_handle* h, const clc_chess_options* copt, const clc_chessorder_options* oopt, const clc_subpix_options* sopt,
                               const uint8_t* images_dev, int32_t width, int32_t height, int64_t pitch, size_t n_images, int32_t cols,
                               int32_t rows, float* corners_dev, int32_t* found_dev, double* strength_dev) {
  const char* who = "clc_find_chessboard_device";
  clc_chess_options o;
  double tol = 0.0;
  CLC_TRY(find_checks(who, n_images == 0 || (images_dev && corners_dev && found_dev), copt, oopt, sopt, width, height, pitch, n_images, cols, rows,
                      &o, &tol));
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_find_chessboard_device: bad argument");
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  find_on_device(st, o, tol, sopt, images_dev, width, height, pitch, n_images, cols, rows, corners_dev, found_dev, strength_dev);
  return st.finish(who);
}

int clc_find_chessboard_gpu(clc_handle* h, const clc_chess_options* copt, const clc_chessorder_options* oopt, const clc_subpix_options* sopt,
                            const uint8_t* images, int32_t width, int32_t height, int64_t pitch, size_t n_images, int32_t cols, int32_t rows,
                            float* corners, int32_t* found, double* strength) {
  const char* who = "clc_find_chessboard_gpu";
  clc_chess_options o;
  double tol = 0.0;
  CLC_TRY(find_checks(who, n_images == 0 || (images && corners && found), copt, oopt, sopt, width, height, pitch, n_images, cols, rows, &o, &tol));
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_find_chessboard_gpu: bad argument");
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const size_t M = n_images * (size_t)cols * (size_t)rows;
  Staging st(h);  // the images go up once
  const uint8_t* img_dev = st.in(images, n_images * (size_t)height * (size_t)pitch);
  float* corners_dev = st.out(corners, 2 * M);
  int32_t* found_dev = st.out(found, n_images);
  double* strength_dev = st.out_opt(strength, M);
  find_on_device(st, o, tol, sopt, img_dev, width, height, pitch, n_images, cols, rows, corners_dev, found_dev, strength_dev);
  return st.finish(who);
}

}  // extern "C"
