// tests/shim/subpix_shim.cpp — TEST ONLY.  Compiles K24 (camlasercalibratool_amd/csrc/clc_subpix.hpp: the refinement of one corner,
// the options as the kernel takes them, the image of a corner) for the host with g++.  The lanes of a corner's wave are a loop and the
// wave all-reduce a butterfly in the device's order; the corners of a launch are a loop.  The tests compare it with the numpy
// restatement tests/subpix_ref.py, and the GPU tests compare the device against it bit for bit.
#include <cmath>
#include <vector>

#include "../../camlasercalibratool_amd/csrc/clc_subpix.hpp"

extern "C" {

int shim_subpix_options_size() { return (int)sizeof(clc_subpix_options); }

// clc_subpix_options_default (abi_subpix.hip)
void shim_subpix_options_default(clc_subpix_options* o, int32_t win) {
  o->win_x = o->win_y = win > 0 ? win : 3;
  o->zero_x = o->zero_y = -1;
  o->max_iter = 30;
  o->reserved = 0;
  o->eps = 0.1;
}

// The mask tables and what else the kernel takes of the options: vx[2 win_x + 1], vy[2 win_y + 1], zone[2] (-1: off), mask_sum.
void shim_subpix_model(const clc_subpix_options* o, float* vx, float* vy, int32_t* zone, double* mask_sum) {
  const clc::sp::SubpixModel m = clc::sp::subpix_model(*o);
  for (int j = 0; j <= 2 * m.wx; ++j) vx[j] = m.vx[j];
  for (int i = 0; i <= 2 * m.wy; ++i) vy[i] = m.vy[i];
  zone[0] = m.zx; zone[1] = m.zy;
  *mask_sum = m.mask_sum;
}

// clc_corner_subpix on the host (valid options, monotone offsets); corners_out may be corners_in; status, iterations, strength nullable.
void shim_corner_subpix(const clc_subpix_options* o, const uint8_t* images, int32_t width, int32_t height, long long pitch,
                        long long n_images, const float* corners_in, const long long* offsets, float* corners_out, int32_t* status,
                        int32_t* iterations, double* strength) {
  namespace sp = clc::sp;
  if (n_images <= 0 || offsets[n_images] == offsets[0]) return;
  const sp::SubpixModel m = sp::subpix_model(*o);
  sp::SubpixArgs a{};
  a.wx = m.wx; a.wy = m.wy; a.zx = m.zx; a.zy = m.zy; a.max_iter = m.max_iter; a.width = width; a.height = height;
  a.eps2 = m.eps2; a.mask_sum = m.mask_sum; a.pitch = pitch; a.images = images;
  // the tables at their exact sizes, as the device's copies are
  const std::vector<float> vx(m.vx, m.vx + 2 * m.wx + 1), vy(m.vy, m.vy + 2 * m.wy + 1);
  a.vx = vx.data(); a.vy = vy.data();
  a.in = corners_in; a.off = offsets; a.first = offsets[0]; a.n_corners = offsets[n_images] - offsets[0]; a.n_images = n_images;
  a.out = corners_out; a.status = status; a.iterations = iterations; a.strength = strength;
  static thread_local sp::Patch L;
  for (long long c = a.first; c < a.first + a.n_corners; ++c) sp::refine_corner(a, c, sp::image_of(a, c), L);
}

}  // extern "C"
