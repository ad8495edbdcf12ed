// tests/shim/boardorder_shim.cpp — TEST ONLY.  Compiles K26 (camlasercalibratool_amd/csrc/clc_boardorder.hpp: the ordering of one image
// per wave, the gather of the ordered pixels) for the host with g++ -ffp-contract=off.  The lanes of a wave are a loop, the barrier
// between two passes is the end of the loop, an image's LDS is a heap block of exactly lds_bytes(cols rows); the images of a launch
// are a loop.  The tests compare it with the product library's clc_chessboard_order, and its hull and quadrilateral with
// tests/chess_ref.py.
#include <cstdlib>

#include "../../camlasercalibratool_amd/csrc/clc_boardorder.hpp"

extern "C" {

long long shim_board_lds_bytes(int n) { return (long long)clc::boardorder::lds_bytes(n); }

// clc_chessboard_order_device on the host (valid arguments); n_labelings and worst nullable.  nh [n_images], hull [n_images][cols rows]
// (the candidate slots of the hull's vertices) and quad [n_images][4] (hull positions), all nullable: 0 and untouched where the image
// did not get that far.
void shim_board_order(const float* cand_xy, const int32_t* count, long long stride, long long n_images, int32_t cols, int32_t rows, double tol,
                      int32_t* index, int32_t* status, int32_t* n_labelings, double* worst, int32_t* nh, int32_t* hull, int32_t* quad) {
  namespace bo = clc::boardorder;
  const int n = cols * rows;
  bo::OrderArgs a{};
  a.cand_xy = cand_xy; a.count = count; a.stride = stride; a.first = 0; a.cols = cols; a.rows = rows; a.tol = tol;
  a.index = index; a.status = status; a.n_labelings = n_labelings; a.worst = worst;
  void* lds = std::malloc(bo::lds_bytes(n));  // exactly the launch's dynamic LDS
  for (long long i = 0; i < n_images; ++i) {
    int32_t h = 0;
    bo::order_one(a, i, lds, &h, hull ? hull + i * n : nullptr, quad ? quad + i * 4 : nullptr);
    if (nh) nh[i] = h;
  }
  std::free(lds);
}

// The gather on the host; offsets and strength nullable.
void shim_board_gather(const float* cand_xy, const int32_t* index, const int32_t* status, long long stride, long long n_images, int32_t n,
                       float* starts, int32_t* found, int64_t* offsets, double* strength) {
  namespace bo = clc::boardorder;
  bo::GatherArgs g{};
  g.cand_xy = cand_xy; g.index = index; g.status = status; g.stride = stride; g.n_images = n_images; g.n = n;
  g.starts = starts; g.found = found; g.offsets = offsets; g.strength = strength;
  for (long long i = 0; i < n_images; ++i) bo::gather_one(g, i);
}

}  // extern "C"
