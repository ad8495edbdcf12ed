// tests/shim/chessorder_main.cpp — TEST ONLY.  A stand-alone program over the host ordering of K25
// (camlasercalibratool_amd/csrc/clc_chessorder.hpp): two boards under a homography and the refusals, every array of its exact size:
// built with -fsanitize=address,undefined and run as an ordinary process by tests/test_chess_host.py.  Not loaded into Python, not
// run on a GPU.
#include <cstdio>
#include <cstdlib>

#include "../../camlasercalibratool_amd/csrc/clc_chessorder.hpp"

namespace {

int check(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); std::exit(1); }
  return 0;
}

// The nodes of a cols x rows grid under a perspective map, rounded to pixels, in a scrambled slot order; slot_of[i cols + j] = the slot.
void board(int cols, int rows, double angle, double px, double py, std::vector<float>& xy, std::vector<int>& slot_of) {
  const int n = cols * rows;
  xy.assign((size_t)(2 * n), 0.0f);
  slot_of.assign((size_t)n, 0);
  for (int m = 0; m < n; ++m) slot_of[(size_t)m] = (m * 7 + 3) % n;  // a bijection where gcd(7, n) = 1
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) {
      const double X = 22.0 * (j - 0.5 * (cols - 1)), Y = 22.0 * (i - 0.5 * (rows - 1));
      const double u = std::cos(angle) * X - std::sin(angle) * Y, v = std::sin(angle) * X + std::cos(angle) * Y;
      const double w = 1.0 + px * u + py * v;
      const int s = slot_of[(size_t)(i * cols + j)];
      xy[(size_t)(2 * s)] = (float)std::llround(160.0 + u / w);
      xy[(size_t)(2 * s + 1)] = (float)std::llround(120.0 + v / w);
    }
}

}  // namespace

int main() {
  namespace co = clc::chessorder;
  long long found = 0;
  const int shapes[][2] = {{5, 4}, {9, 6}, {6, 6}, {2, 2}, {3, 2}};
  for (const auto& sh : shapes)
    for (int k = 0; k < 6; ++k) {
      const int cols = sh[0], rows = sh[1], n = cols * rows;
      if (n % 7 == 0) continue;
      std::vector<float> xy;
      std::vector<int> slot_of;
      board(cols, rows, 0.3 + 1.1 * k, 4e-4 * (k - 2), -3e-4 * (k % 3), xy, slot_of);
      std::vector<int32_t> count(1, n), status(1, CLC_CHESS_OK), index((size_t)n, -5), lab(1, -5);
      std::vector<double> worst(1, -5.0);
      co::order_images(xy.data(), count.data(), n, 1, cols, rows, 0.3, index.data(), status.data(), lab.data(), worst.data());
      check(status[0] == CLC_CHESS_FOUND, "a board under a homography is found");
      check(lab[0] == (cols == rows ? 4 : 2), "the labelings of a front view");
      check(worst[0] >= 0.0 && worst[0] < 0.1, "the worst ratio");
      // the labeling is the truth's or the truth turned by a half turn (a square grid: by a quarter turn as well)
      bool same = true, half = true;
      for (int m = 0; m < n; ++m) {
        same = same && index[(size_t)m] == slot_of[(size_t)m];
        half = half && index[(size_t)m] == slot_of[(size_t)(n - 1 - m)];
      }
      check(same || half || cols == rows, "the grid's order");
      std::vector<char> used((size_t)n, 0);
      for (int m = 0; m < n; ++m) {
        check(index[(size_t)m] >= 0 && index[(size_t)m] < n && !used[(size_t)index[(size_t)m]], "a bijection");
        used[(size_t)index[(size_t)m]] = 1;
      }
      // node (0, 0) comes first in raster order among the four corner nodes
      const int corner[4] = {0, cols - 1, n - 1, n - cols};
      for (int c = 1; c < 4; ++c) {
        const float y0 = xy[(size_t)(2 * index[0] + 1)], x0 = xy[(size_t)(2 * index[0])];
        const float y1 = xy[(size_t)(2 * index[(size_t)corner[c]] + 1)], x1 = xy[(size_t)(2 * index[(size_t)corner[c]])];
        if (cols == rows || c == 2) check(y0 < y1 || (y0 == y1 && x0 < x1), "node (0, 0) first in raster order");
      }
      ++found;
      // the refusals on the same board: one candidate short; a corner moved by a spacing; every candidate on one line; overflow
      std::vector<int32_t> st2(1, CLC_CHESS_OK), cnt2(1, n - 1);
      co::order_images(xy.data(), cnt2.data(), n, 1, cols, rows, 0.3, index.data(), st2.data(), nullptr, nullptr);
      check(st2[0] == CLC_CHESS_TOO_FEW && index[0] == -1, "too few");
      if (n >= 12) {
        std::vector<float> moved(xy);
        const int s = slot_of[(size_t)(n - 1)], t = slot_of[(size_t)(n - 2)];
        moved[(size_t)(2 * s)] += moved[(size_t)(2 * s)] - moved[(size_t)(2 * t)];
        moved[(size_t)(2 * s + 1)] += moved[(size_t)(2 * s + 1)] - moved[(size_t)(2 * t + 1)];
        st2[0] = CLC_CHESS_OK;
        co::order_images(moved.data(), count.data(), n, 1, cols, rows, 0.3, index.data(), st2.data(), lab.data(), worst.data());
        check(st2[0] == CLC_CHESS_NO_GRID && lab[0] == 0 && worst[0] != worst[0] && index[(size_t)(n - 1)] == -1, "a corner moved by a spacing");
      }
      std::vector<float> line((size_t)(2 * n));
      for (int m = 0; m < n; ++m) { line[(size_t)(2 * m)] = (float)(10 + 3 * m); line[(size_t)(2 * m + 1)] = (float)(20 + 2 * m); }
      st2[0] = CLC_CHESS_OK;
      co::order_images(line.data(), count.data(), n, 1, cols, rows, 0.3, index.data(), st2.data(), nullptr, nullptr);
      check(st2[0] == CLC_CHESS_NO_GRID, "collinear candidates");
      st2[0] = CLC_CHESS_OVERFLOW;
      co::order_images(xy.data(), count.data(), n, 1, cols, rows, 0.3, index.data(), st2.data(), nullptr, nullptr);
      check(st2[0] == CLC_CHESS_OVERFLOW && index[0] == -1, "overflow passes through");
      // NaN and coincident candidates
      std::vector<float> bad(xy);
      bad[1] = std::nanf("");
      st2[0] = CLC_CHESS_OK;
      co::order_images(bad.data(), count.data(), n, 1, cols, rows, 0.3, index.data(), st2.data(), nullptr, nullptr);
      check(st2[0] == CLC_CHESS_NO_GRID, "a NaN candidate");
      std::vector<float> dup((size_t)(2 * n), 7.0f);
      st2[0] = CLC_CHESS_OK;
      co::order_images(dup.data(), count.data(), n, 1, cols, rows, 0.3, index.data(), st2.data(), nullptr, nullptr);
      check(st2[0] == CLC_CHESS_NO_GRID, "coincident candidates");
    }
  // no image
  co::order_images(nullptr, nullptr, 4, 0, 2, 2, 0.3, nullptr, nullptr, nullptr, nullptr);
  std::printf("boards found %lld\nshapes ok\n", found);
  return 0;
}
