// abi_imagecall.hpp — host code the units of the image front end share (abi_subpix.hip: K24, abi_chess.hip: K25 and K26, abi_tags.hip:
// K27): the rules on the images and on the refinement options with their messages, once, and what one unit needs of another,
// through public types only.  No kernel lives here and no kernel header is included: clc_subpix.hpp stays in abi_subpix.hip alone and
// clc_chess.hpp in abi_chess.hip alone, so each unit's code object holds its own kernels (tests/test_*_resources.py).
#pragma once
#include <cmath>
#include <string>

#include "abi_staging.hpp"

namespace clc_abi {

// ---- the rules; the order in which a unit applies them is its own ----
// n_images images of height rows of pitch bytes, width of them pixels.
inline int image_geometry_check(const char* who, int32_t width, int32_t height, int64_t pitch, size_t n_images) {
  const std::string w(who);
  if (width < 1 || height < 1) return fail(CLC_ERR_INVALID_ARG, (w + ": width and height must be >= 1").c_str());
  if (pitch < (int64_t)width) return fail(CLC_ERR_INVALID_ARG, (w + ": pitch must be >= width").c_str());
  if (n_images > 0x7FFFFFFFull || (n_images > 0 && pitch > (int64_t)(0x7FFFFFFFFFFFFFFFull / n_images / (uint64_t)height)))
    return fail(CLC_ERR_INVALID_ARG, (w + ": too many images").c_str());
  return CLC_OK;
}
// What is wrong with the first field of the refinement options that is out of range; nullptr: nothing is.
inline const char* subpix_options_fault(const clc_subpix_options& o) {
  if (o.win_x < 1 || o.win_x > CLC_SUBPIX_MAX_WIN || o.win_y < 1 || o.win_y > CLC_SUBPIX_MAX_WIN) return "the half-window must be in [1, 15]";
  if (o.max_iter < 1 || o.max_iter > 100) return "max_iter must be in [1, 100]";
  if (!(std::isfinite(o.eps) && o.eps >= 0.0)) return "eps must be finite and >= 0";
  if (o.reserved != 0) return "reserved must be 0";
  return nullptr;
}
// One launch of K24 takes one workgroup per corner.
inline int corner_count_check(const char* who, uint64_t n_corners) {
  if (n_corners > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": too many corners").c_str());
  return CLC_OK;
}
// The refinement as a composite call (detection, then K24 on what it found) sees it: nothing to refuse without sopt; with it the
// options as a whole, then the n_corners the call will hand to K24.
inline int refinement_checks(const char* who, const clc_subpix_options* sopt, uint64_t n_corners) {
  if (!sopt) return CLC_OK;
  if (subpix_options_fault(*sopt))
    return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": the refinement options are not valid (clc_corner_subpix)").c_str());
  return corner_count_check(who, n_corners);
}

// ---- K25's detection on device arrays (abi_chess.hip), for the units that build on its candidates ----
// Images per enqueue of its kernels: the raw lists of one chunk (CLC_CHESS_RAW_CAP entries of 3 int32 per image: 48 KiB) stay
// within 8 MiB; images beyond go in further chunks on the same stream.  K27 chunks its edge lists alike.
constexpr size_t kChessChunkImages = ((size_t)8 << 20) / ((size_t)CLC_CHESS_RAW_CAP * 3 * sizeof(int32_t));
// What the detection refuses ahead of the handle, in one order (`required`: the call's arrays are there); then the options with
// the defaults filled in.
int chess_checks(const char* who, bool required, const clc_chess_options* in, int32_t width, int32_t height, int64_t pitch, size_t n_images,
                 clc_chess_options* o);
// Per chunk of images the counters to zero, one workgroup per tile, one wave per image.
void enqueue_chess(Staging& st, const clc_chess_options& o, const uint8_t* images, int32_t width, int32_t height, int64_t pitch, size_t n_images,
                   float* cand_xy, int32_t* cand_r5, int32_t* count, int32_t* count_raw, int32_t* status);

// ---- K24's refinement on device arrays (abi_subpix.hip), for the calls that end in it ----
// The mask tables of the (checked) options up, owned by st, then one wave per corner: corners [first, first + n_corners) of in, the
// image of each from off[n_images + 1]; n_corners in [1, 2^31).
void enqueue_subpix_refinement(Staging& st, const clc_subpix_options& o, const uint8_t* images, int32_t width, int32_t height, int64_t pitch,
                               size_t n_images, const float* in, const int64_t* off, long long first, size_t n_corners, float* out,
                               int32_t* status, int32_t* iterations, double* strength);

}  // namespace clc_abi
