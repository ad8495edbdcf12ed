// tests/shim/boardorder_main.cpp — TEST ONLY.  A stand-alone program (g++ -fsanitize=address,undefined -ffp-contract=off) that runs K26's
// host build (camlasercalibratool_amd/csrc/clc_boardorder.hpp, the lanes a loop) beside the host ordering it restates
// (clc_chessorder.hpp) with every array allocated exactly: the candidate sets of tests/boardorder_cases.py from the file named on the
// command line (int32 n_cases; per case int32 cols, rows, stride, k, then count[k], status[k], float xy[k stride 2]), then grids from
// 2 x 2 to 32 x 32 under a homography with integer jitter.  index, status and n_labelings must be equal, worst within 16 eps; the
// gather's starts must be the indexed candidates.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../camlasercalibratool_amd/csrc/clc_boardorder.hpp"
#include "../../camlasercalibratool_amd/csrc/clc_chessorder.hpp"

namespace bo = clc::boardorder;

static int failures = 0;

template <class T>
struct Exact {  // a heap block of exactly n elements (at least one byte), so that one element past it is caught
  T* p;
  explicit Exact(size_t n) : p(static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1))) {}
  ~Exact() { std::free(p); }
  Exact(const Exact&) = delete;
};

static int run_case(const char* what, const float* xy, const int32_t* count, const int32_t* status_in, int cols, int rows, long long stride,
                    long long k, int* found_out) {
  const int n = cols * rows;
  Exact<int32_t> ia((size_t)k * n), ib((size_t)k * n), sa((size_t)k), sb((size_t)k), la((size_t)k), lb((size_t)k), found((size_t)k);
  Exact<double> wa((size_t)k), wb((size_t)k), strength((size_t)k * n);
  Exact<float> starts((size_t)k * n * 2);
  Exact<int64_t> offsets((size_t)k + 1);
  std::memcpy(sa.p, status_in, (size_t)k * sizeof(int32_t));
  std::memcpy(sb.p, status_in, (size_t)k * sizeof(int32_t));
  clc::chessorder::order_images(xy, count, stride, k, cols, rows, 0.3, ia.p, sa.p, la.p, wa.p);
  bo::OrderArgs a{};
  a.cand_xy = xy; a.count = count; a.stride = stride; a.cols = cols; a.rows = rows; a.tol = 0.3;
  a.index = ib.p; a.status = sb.p; a.n_labelings = lb.p; a.worst = wb.p;
  Exact<char> lds(bo::lds_bytes(n));
  for (long long i = 0; i < k; ++i) bo::order_one(a, i, lds.p);
  bo::GatherArgs g{};
  g.cand_xy = xy; g.index = ib.p; g.status = sb.p; g.stride = stride; g.n_images = k; g.n = n;
  g.starts = starts.p; g.found = found.p; g.offsets = offsets.p; g.strength = strength.p;
  for (long long i = 0; i < k; ++i) bo::gather_one(g, i);
  int bad = 0;
  for (long long i = 0; i < k; ++i) {
    bad += sa.p[i] != sb.p[i] || la.p[i] != lb.p[i];
    for (int m = 0; m < n; ++m) bad += ia.p[i * n + m] != ib.p[i * n + m];
    if (std::isnan(wa.p[i]) != std::isnan(wb.p[i])) ++bad;
    else if (!std::isnan(wa.p[i]) && std::fabs(wa.p[i] - wb.p[i]) > 16 * 2.220446049250313e-16 * std::fabs(wa.p[i])) ++bad;
    const bool f = sb.p[i] == CLC_CHESS_FOUND;
    bad += found.p[i] != (f ? 1 : 0) || offsets.p[i] != i * n;
    for (int m = 0; m < n; ++m) {
      const float x = starts.p[2 * (i * n + m)], y = starts.p[2 * (i * n + m) + 1];
      if (f) bad += x != xy[(i * stride + ib.p[i * n + m]) * 2] || y != xy[(i * stride + ib.p[i * n + m]) * 2 + 1];
      else bad += !(std::isnan(x) && std::isnan(y));
      bad += !std::isnan(strength.p[i * n + m]);
    }
    if (f) ++*found_out;
  }
  if (k > 0) bad += offsets.p[k] != k * n;
  if (bad) { std::printf("MISMATCH %s %dx%d: %d\n", what, cols, rows, bad); ++failures; }
  return bad;
}

int main(int argc, char** argv) {
  int n_cases = 0, found = 0;
  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int32_t total = 0;
    if (std::fread(&total, 4, 1, f) != 1) return 2;
    for (int c = 0; c < total; ++c) {
      int32_t h[4];
      if (std::fread(h, 4, 4, f) != 4) return 2;
      const int cols = h[0], rows = h[1];
      const long long stride = h[2], k = h[3];
      Exact<int32_t> count((size_t)k), status((size_t)k);
      Exact<float> xy((size_t)(k * stride * 2));
      if (std::fread(count.p, 4, (size_t)k, f) != (size_t)k || std::fread(status.p, 4, (size_t)k, f) != (size_t)k ||
          std::fread(xy.p, 4, (size_t)(k * stride * 2), f) != (size_t)(k * stride * 2))
        return 2;
      run_case("case", xy.p, count.p, status.p, cols, rows, stride, k, &found);
      ++n_cases;
    }
    std::fclose(f);
  }
  // grids from 2 x 2 to 32 x 32: a lattice at 14 px under a homography, integer jitter in {-1, 0, 1}^2, the slots in a scrambled order
  unsigned long long s = 2601;
  auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); };
  int grids = 0, grids_found = 0;
  const int sizes[][2] = {{2, 2}, {2, 3}, {3, 2}, {3, 3}, {4, 3}, {5, 4}, {7, 2}, {8, 8}, {9, 6}, {11, 7}, {13, 13}, {16, 9}, {21, 17}, {31, 33}, {32, 32}};
  for (const auto& sz : sizes) {
    const int cols = sz[0], rows = sz[1], n = cols * rows;
    const long long k = 3;
    Exact<float> xy((size_t)(k * n * 2));
    Exact<int32_t> count((size_t)k), status((size_t)k);
    for (long long i = 0; i < k; ++i) {
      count.p[i] = n; status.p[i] = CLC_CHESS_OK;
      const double th = 0.3 * (double)i + 0.1 * (double)(rnd() % 7), c = std::cos(th), sn = std::sin(th);
      std::vector<int> perm((size_t)n);
      for (int m = 0; m < n; ++m) perm[(size_t)m] = m;
      for (int m = n - 1; m > 0; --m) std::swap(perm[(size_t)m], perm[(size_t)(rnd() % (unsigned)(m + 1))]);
      for (int m = 0; m < n; ++m) {
        const double X = 14.0 * (m % cols) - 7.0 * (cols - 1), Y = 14.0 * (m / cols) - 7.0 * (rows - 1);
        const double w = 1.0 + 1e-4 * X - 5e-5 * Y;
        const double x = (c * X - sn * Y) / w + 600.0, y = (sn * X + c * Y) / w + 600.0;
        float* o = xy.p + (i * n + perm[(size_t)m]) * 2;
        o[0] = (float)(std::llround(x) + (long long)(rnd() % 3) - 1);
        o[1] = (float)(std::llround(y) + (long long)(rnd() % 3) - 1);
      }
    }
    run_case("grid", xy.p, count.p, status.p, cols, rows, n, k, &grids_found);
    grids += (int)k;
  }
  std::printf("cases %d boards found %d grids %d found %d\n", n_cases, found, grids, grids_found);
  if (failures) { std::printf("FAILED %d\n", failures); return 1; }
  std::printf("shapes ok\n");
  return 0;
}
