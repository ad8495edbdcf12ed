// abi_tags.hip — clc_tag_options_default, clc_tag_grid(_device), clc_tag_grid_points_device: the corners of a Kalibr-style tag grid
// from images (K27: the kernels in clc_tags.hpp, on K25's candidates and K26's 4-point solve; the refinement is K24's).
// A unit of its own, held to its own register figures (tests/test_tags_resources.py).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "abi_imagecall.hpp"
#include "clc_tags.hpp"

using namespace clc_abi;

namespace {

namespace tg = clc::tags;

// (images per launch of the edge and decode kernels: kChessChunkImages, as K25 chunks its own; the edge lists of one launch stay
// below 10 MiB)
constexpr size_t kPointLaunchImages = (size_t)1 << 20;

struct Checked {
  clc_tag_options t;
  tg::DetectOptions c;
};

// What both forms refuse alike ahead of the handle, in one order; then the options with the defaults filled in.
int tag_checks(const char* who, bool required, const clc_tag_family* f, const clc_tag_options* topt, const tg::DetectOptions* copt,
               const clc_subpix_options* sopt, int32_t width, int32_t height, int64_t pitch, size_t n_images, int32_t cols, int32_t rows,
               Checked* out) {
  const std::string w(who);
  if (!f) return fail(CLC_ERR_INVALID_ARG, (w + ": the family is required").c_str());
  if (f->side < 3 || f->side > 7) return fail(CLC_ERR_INVALID_ARG, (w + ": family.side must be in [3, 7]").c_str());
  if (f->border < 1 || f->border > 2) return fail(CLC_ERR_INVALID_ARG, (w + ": family.border must be 1 or 2").c_str());
  if (f->n_codes < 1 || f->n_codes > CLC_TAG_MAX_CODES) return fail(CLC_ERR_INVALID_ARG, (w + ": family.n_codes must be in [1, 4096]").c_str());
  const int bits = f->side * f->side;
  if (f->max_hamming < 0 || f->max_hamming > bits / 2) return fail(CLC_ERR_INVALID_ARG, (w + ": family.max_hamming must be in [0, d d / 2]").c_str());
  if (!f->codes) return fail(CLC_ERR_INVALID_ARG, (w + ": family.codes is required").c_str());
  for (int32_t i = 0; i < f->n_codes; ++i)
    if (f->codes[i] >> bits) return fail(CLC_ERR_INVALID_ARG, (w + ": a code has bits above d d").c_str());
  if (topt) out->t = *topt; else clc_tag_options_default(&out->t);
  const clc_tag_options& t = out->t;
  if (t.min_side_px < 8) return fail(CLC_ERR_INVALID_ARG, (w + ": min_side_px must be >= 8").c_str());
  if (t.max_side_px != 0 && t.max_side_px < t.min_side_px) return fail(CLC_ERR_INVALID_ARG, (w + ": max_side_px must be 0 or >= min_side_px").c_str());
  if (t.contrast < 1 || t.contrast > 255) return fail(CLC_ERR_INVALID_ARG, (w + ": contrast must be in [1, 255]").c_str());
  if (t.max_border_errors < 0 || t.max_border_errors > 8) return fail(CLC_ERR_INVALID_ARG, (w + ": max_border_errors must be in [0, 8]").c_str());
  if (t.max_quads < 1 || t.max_quads > CLC_TAG_MAX_QUADS) return fail(CLC_ERR_INVALID_ARG, (w + ": max_quads must be in [1, 1024]").c_str());
  if (t.reserved != 0) return fail(CLC_ERR_INVALID_ARG, (w + ": reserved must be 0").c_str());
  if (cols < 1 || rows < 1 || (int64_t)cols * rows > CLC_TAG_MAX_TAGS)
    return fail(CLC_ERR_INVALID_ARG, (w + ": cols and rows must be >= 1 and cols x rows <= 1024").c_str());
  tg::DetectOptions dflt;
  if (!copt) {  // K25's defaults with every slot of an image
    tg::detect_options_default(&dflt);
    dflt.max_per_image = tg::MAX_CAND;
    copt = &dflt;
  }
  CLC_TRY(chess_checks(who, true, copt, width, height, pitch, n_images, &out->c));
  CLC_TRY(refinement_checks(who, sopt, (uint64_t)n_images * 4 * (uint64_t)cols * (uint64_t)rows));
  if (!required) return fail(CLC_ERR_INVALID_ARG, (w + ": bad argument").c_str());
  return CLC_OK;
}

// Detection, edges, quads and decode, and with sopt the refinement, on device arrays, all enqueued on the caller's st: nothing is read
// back in between and nothing is waited for here.
void tags_on_device(Staging& st, const Checked& o, const clc_tag_family& f, const clc_subpix_options* sopt, const uint8_t* img_dev,
                    int32_t width, int32_t height, int64_t pitch, size_t n_images, int32_t cols, int32_t rows, float* corners_dev,
                    int32_t* hamming_dev, int32_t* count_dev, int32_t* status_dev, int32_t* n_quads_dev, int32_t* n_foreign_dev,
                    int32_t* n_dropped_dev, double* strength_dev) {
  const size_t stride = (size_t)o.c.max_per_image, T = (size_t)cols * (size_t)rows, chunk = std::min(n_images, kChessChunkImages);
  const uint64_t* codes_dev = st.in(f.codes, (size_t)f.n_codes);
  float* xy_dev = st.scratch<float>(2 * n_images * stride);
  int32_t* cnt_dev = st.scratch<int32_t>(n_images);
  int32_t* cst_dev = st.scratch<int32_t>(n_images);
  int32_t* edges_dev = st.scratch<int32_t>(chunk * stride * (size_t)tg::EDGE_INTS);
  const int64_t* off_dev = nullptr;
  if (sopt) {  // every image has 4 T corners
    std::vector<int64_t> offsets(n_images + 1);
    for (size_t i = 0; i <= n_images; ++i) offsets[i] = (int64_t)(i * 4 * T);
    off_dev = st.in_owned(std::move(offsets));
  }
  if (st.ok()) enqueue_chess(st, o.c, img_dev, width, height, pitch, n_images, xy_dev, nullptr, cnt_dev, nullptr, cst_dev);
  tg::TagArgs a{};
  a.width = width; a.height = height; a.stride = (int32_t)stride; a.d = f.side; a.b = f.border; a.n_codes = f.n_codes;
  a.max_hamming = f.max_hamming; a.min_side = o.t.min_side_px; a.max_side = o.t.max_side_px ? o.t.max_side_px : std::min(width, height);
  a.contrast = o.t.contrast; a.max_border_errors = o.t.max_border_errors; a.max_quads = o.t.max_quads; a.n_tags = (int32_t)T;
  a.pitch = (long long)pitch; a.codes = codes_dev; a.edges = edges_dev;
  for (size_t first = 0; first < n_images && st.ok(); first += chunk) {
    const size_t n = std::min(chunk, n_images - first);
    a.images = img_dev + first * (size_t)height * (size_t)pitch;
    a.cand_xy = xy_dev + 2 * first * stride; a.cand_count = cnt_dev + first; a.cand_status = cst_dev + first;
    a.corners = corners_dev + first * T * 8; a.hamming = hamming_dev + first * T; a.count = count_dev + first; a.status = status_dev + first;
    a.n_quads = n_quads_dev ? n_quads_dev + first : nullptr;
    a.n_foreign = n_foreign_dev ? n_foreign_dev + first : nullptr;
    a.n_edges_dropped = n_dropped_dev ? n_dropped_dev + first : nullptr;
    a.strength = (!sopt && strength_dev) ? strength_dev + first * T * 4 : nullptr;
    hipLaunchKernelGGL(tg::tag_edges_kernel, dim3((unsigned)n), dim3(tg::EDGE_THREADS), 0, st.stream(), a);
    st.launched();
    if (!st.ok()) break;
    hipLaunchKernelGGL(tg::tag_decode_kernel, dim3((unsigned)n), dim3(tg::LANES), 0, st.stream(), a);
    st.launched();
  }
  // (a NaN start comes back as it is: a tag not seen keeps its NaN corners)
  if (sopt && st.ok())
    enqueue_subpix_refinement(st, *sopt, img_dev, width, height, pitch, n_images, corners_dev, off_dev, 0, n_images * 4 * T, corners_dev, nullptr,
                              nullptr, strength_dev);
}

}  // namespace

extern "C" {

void clc_tag_options_default(clc_tag_options* o) {
  if (!o) return;
  o->min_side_px = 16;
  o->max_side_px = 0;
  o->contrast = 40;
  o->max_border_errors = 0;
  o->max_quads = 256;
  o->reserved = 0;
}

int clc_tag_grid(clc_handle* h, const clc_tag_family* family, const clc_tag_options* topt, const tg::DetectOptions* copt,
                 const clc_subpix_options* sopt, const uint8_t* images, int32_t width, int32_t height, int64_t pitch, size_t n_images,
                 int32_t cols, int32_t rows, float* corners, int32_t* hamming, int32_t* count, int32_t* status, int32_t* n_quads,
                 int32_t* n_foreign, int32_t* n_edges_dropped, double* strength) {
  const char* who = "clc_tag_grid";
  Checked o;
  CLC_TRY(tag_checks(who, n_images == 0 || (images && corners && hamming && count && status), family, topt, copt, sopt, width, height, pitch,
                     n_images, cols, rows, &o));
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_tag_grid: bad argument");
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const size_t T = (size_t)cols * (size_t)rows;
  Staging st(h);  // the images go up once
  const uint8_t* img_dev = st.in(images, n_images * (size_t)height * (size_t)pitch);
  float* corners_dev = st.out(corners, n_images * T * 8);
  int32_t* hamming_dev = st.out(hamming, n_images * T);
  int32_t* count_dev = st.out(count, n_images);
  int32_t* status_dev = st.out(status, n_images);
  int32_t* quads_dev = st.out_opt(n_quads, n_images);
  int32_t* foreign_dev = st.out_opt(n_foreign, n_images);
  int32_t* dropped_dev = st.out_opt(n_edges_dropped, n_images);
  double* strength_dev = st.out_opt(strength, n_images * T * 4);
  tags_on_device(st, o, *family, sopt, img_dev, width, height, pitch, n_images, cols, rows, corners_dev, hamming_dev, count_dev, status_dev,
                 quads_dev, foreign_dev, dropped_dev, strength_dev);
  return st.finish(who);
}

int clc_tag_grid_device(clc_handle* h, const clc_tag_family* family, const clc_tag_options* topt, const tg::DetectOptions* copt,
                        const clc_subpix_options* sopt, const uint8_t* images_dev, int32_t width, int32_t height, int64_t pitch,
                        size_t n_images, int32_t cols, int32_t rows, float* corners_dev, int32_t* hamming_dev, int32_t* count_dev,
                        int32_t* status_dev, int32_t* n_quads_dev, int32_t* n_foreign_dev, int32_t* n_edges_dropped_dev,
                        double* strength_dev) {
  const char* who = "clc_tag_grid_device";
  Checked o;
  CLC_TRY(tag_checks(who, n_images == 0 || (images_dev && corners_dev && hamming_dev && count_dev && status_dev), family, topt, copt, sopt, width,
                     height, pitch, n_images, cols, rows, &o));
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_tag_grid_device: bad argument");
  if (n_images == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  tags_on_device(st, o, *family, sopt, images_dev, width, height, pitch, n_images, cols, rows, corners_dev, hamming_dev, count_dev, status_dev,
                 n_quads_dev, n_foreign_dev, n_edges_dropped_dev, strength_dev);
  return st.finish(who);
}

int clc_tag_grid_points_device(clc_handle* h, const float* corners_dev, const int32_t* hamming_dev, size_t n_images, int32_t cols,
                               int32_t rows, double tag_size, double tag_spacing, float* corners_px_dev, float* board_xy_dev,
                               int64_t* offsets_dev) {
  const char* who = "clc_tag_grid_points_device";
  if (cols < 1 || rows < 1 || (int64_t)cols * rows > CLC_TAG_MAX_TAGS)
    return fail(CLC_ERR_INVALID_ARG, "clc_tag_grid_points_device: cols and rows must be >= 1 and cols x rows <= 1024");
  if (!(std::isfinite(tag_size) && tag_size > 0.0)) return fail(CLC_ERR_INVALID_ARG, "clc_tag_grid_points_device: tag_size must be > 0");
  if (!(std::isfinite(tag_spacing) && tag_spacing >= 0.0)) return fail(CLC_ERR_INVALID_ARG, "clc_tag_grid_points_device: tag_spacing must be >= 0");
  if (n_images > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_tag_grid_points_device: too many images");
  if (!offsets_dev || (n_images > 0 && !(corners_dev && hamming_dev && corners_px_dev && board_xy_dev)) || !h)
    return fail(CLC_ERR_INVALID_ARG, "clc_tag_grid_points_device: bad argument");
  CLC_HIP(hipSetDevice(h->device));
  Staging st(h);
  tg::PointArgs g{};
  g.corners = corners_dev; g.hamming = hamming_dev; g.n_images = (long long)n_images; g.cols = cols; g.n_tags = cols * rows;
  g.tag_size = tag_size; g.tag_spacing = tag_spacing; g.corners_px = corners_px_dev; g.board_xy = board_xy_dev;
  g.offsets = reinterpret_cast<long long*>(offsets_dev);
  hipLaunchKernelGGL(tg::tag_scan_kernel, dim3(1), dim3(tg::SCAN_THREADS), 0, st.stream(), g);
  st.launched();
  for (size_t first = 0; first < n_images && st.ok(); first += kPointLaunchImages) {
    hipLaunchKernelGGL(tg::tag_points_kernel, dim3((unsigned)std::min(kPointLaunchImages, n_images - first)), dim3(tg::LANES), 0, st.stream(), g,
                       (long long)first);
    st.launched();
  }
  return st.finish(who);
}

}  // extern "C"
