// clc_chessorder.hpp — K25, host side: the strongest cols x rows chessboard candidates of an image ordered into the board's grid
// (DESIGN.md K25, §4 of its contract).  Plain C++ without a device: clc_chessboard_order (abi_chess.hip) and the stand-alone
// sanitizer program tests/shim/chessorder_main.cpp both run this code.
//
//   hull        monotone chain on the integer pixels (exact, int64), from the vertex smallest in (x, y), every turn a positive cross
//               product (bx - ax)(cy - by) - (by - ay)(cx - bx) in image coordinates; collinear points are no vertices
//   quad        the 4 hull vertices a < b < c < d (hull order) of the largest shoelace area; the first such tuple on ties
//   labelings   per rotation k of the quad as the images of the nodes (0, 0), (cols - 1, 0), (cols - 1, rows - 1), (0, rows - 1):
//               the 4-point homography (8 x 8 elimination, partial pivoting), every node's nearest candidate, valid iff a bijection
//               with every distance <= tol x the smallest distance of two predicted 4-neighbours; then the least-squares homography
//               of all matches (normal equations, the same elimination) and the matching once more; both passes must be valid
//   choice      of the valid labelings the one whose node (0, 0) comes first in raster order (y, then x)
// The pixels and the grid are brought to [-1, 1] ahead of the fits (the ratios tested are free of scale).
#pragma once
#include "../../include/clc.h"

#include <cmath>
#include <cstdint>
#include <algorithm>
#include <vector>

namespace clc {
namespace chessorder {

struct P2 { double x, y; };

inline long long cross3(const long long* a, const long long* b, const long long* c) {
  return (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0]);
}

// Solves the 8 x 8 system A h = b in place (partial pivoting); false where a pivot vanishes.
inline bool solve8(double A[8][8], double b[8], double h[8]) {
  for (int c = 0; c < 8; ++c) {
    int p = c;
    for (int r = c + 1; r < 8; ++r)
      if (std::fabs(A[r][c]) > std::fabs(A[p][c])) p = r;
    if (!(std::fabs(A[p][c]) > 1e-13)) return false;
    if (p != c) {
      for (int k = 0; k < 8; ++k) std::swap(A[p][k], A[c][k]);
      std::swap(b[p], b[c]);
    }
    for (int r = c + 1; r < 8; ++r) {
      const double f = A[r][c] / A[c][c];
      for (int k = c; k < 8; ++k) A[r][k] -= f * A[c][k];
      b[r] -= f * b[c];
    }
  }
  for (int c = 7; c >= 0; --c) {
    double s = b[c];
    for (int k = c + 1; k < 8; ++k) s -= A[c][k] * h[k];
    h[c] = s / A[c][c];
  }
  for (int c = 0; c < 8; ++c)
    if (!std::isfinite(h[c])) return false;
  return true;
}

// The two rows of the match (X, Y) -> (u, v) with h33 = 1.
inline void match_rows(double X, double Y, double u, double v, double r0[8], double r1[8]) {
  const double a[8] = {X, Y, 1.0, 0.0, 0.0, 0.0, -u * X, -u * Y};
  const double b[8] = {0.0, 0.0, 0.0, X, Y, 1.0, -v * X, -v * Y};
  for (int k = 0; k < 8; ++k) { r0[k] = a[k]; r1[k] = b[k]; }
}

// H through 4 matches (the system itself), or the least-squares H of more (the normal equations).
inline bool fit_homography(const std::vector<P2>& grid, const std::vector<P2>& px, double h[8]) {
  double A[8][8] = {}, b[8] = {};
  const size_t n = grid.size();
  for (size_t m = 0; m < n; ++m) {
    double r0[8], r1[8];
    match_rows(grid[m].x, grid[m].y, px[m].x, px[m].y, r0, r1);
    if (n == 4) {
      for (int k = 0; k < 8; ++k) { A[2 * m][k] = r0[k]; A[2 * m + 1][k] = r1[k]; }
      b[2 * m] = px[m].x; b[2 * m + 1] = px[m].y;
    } else {
      for (int i = 0; i < 8; ++i) {
        for (int k = 0; k < 8; ++k) A[i][k] += r0[i] * r0[k] + r1[i] * r1[k];
        b[i] += r0[i] * px[m].x + r1[i] * px[m].y;
      }
    }
  }
  return solve8(A, b, h);
}

// One pass: the nodes under h, every node's nearest candidate (the first on ties) -> valid?, the matches and the worst distance /
// spacing ratio.
inline bool match_pass(const double h[8], const std::vector<P2>& nodes, const std::vector<P2>& cand, int cols, int rows, double tol,
                       std::vector<int>& match, double* worst) {
  const size_t n = nodes.size();
  std::vector<P2> pred(n);
  for (size_t m = 0; m < n; ++m) {
    const double X = nodes[m].x, Y = nodes[m].y;
    const double w = h[6] * X + h[7] * Y + 1.0;
    if (!(std::fabs(w) > 1e-12)) return false;
    pred[m].x = (h[0] * X + h[1] * Y + h[2]) / w;
    pred[m].y = (h[3] * X + h[4] * Y + h[5]) / w;
    if (!(std::isfinite(pred[m].x) && std::isfinite(pred[m].y))) return false;
  }
  double spacing = INFINITY;
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) {
      const P2& p = pred[(size_t)(i * cols + j)];
      if (j + 1 < cols) spacing = std::min(spacing, std::hypot(pred[(size_t)(i * cols + j + 1)].x - p.x, pred[(size_t)(i * cols + j + 1)].y - p.y));
      if (i + 1 < rows) spacing = std::min(spacing, std::hypot(pred[(size_t)((i + 1) * cols + j)].x - p.x, pred[(size_t)((i + 1) * cols + j)].y - p.y));
    }
  if (!(spacing > 0.0)) return false;
  std::vector<char> used(n, 0);
  double far = 0.0;
  bool bijection = true;
  for (size_t m = 0; m < n; ++m) {
    int best = 0;
    double bd = INFINITY;  // (the squared distance in the search, its root once)
    for (size_t c = 0; c < n; ++c) {
      const double dx = cand[c].x - pred[m].x, dy = cand[c].y - pred[m].y, d = dx * dx + dy * dy;
      if (d < bd) { bd = d; best = (int)c; }
    }
    bd = std::sqrt(bd);
    if (used[(size_t)best]) bijection = false;
    used[(size_t)best] = 1;
    match[m] = best;
    far = std::max(far, bd);
  }
  *worst = far / spacing;
  return bijection && far <= tol * spacing;
}

// One image: xy[2 n] the n = cols rows strongest candidates (integer pixels).  -> CLC_CHESS_FOUND / CLC_CHESS_NO_GRID; index[n].
inline int order_image(const float* xy, int cols, int rows, double tol, int32_t* index, int32_t* n_labelings, double* worst_out) {
  const int n = cols * rows;
  *n_labelings = 0;
  *worst_out = NAN;
  std::vector<long long> ip((size_t)(2 * n));
  for (int k = 0; k < 2 * n; ++k) {
    const float v = xy[k];
    if (!(std::fabs(v) <= 16777216.0f)) return CLC_CHESS_NO_GRID;  // (a NaN among them too)
    ip[(size_t)k] = std::llround((double)v);
  }
  // the hull
  std::vector<int> idx((size_t)n);
  for (int k = 0; k < n; ++k) idx[(size_t)k] = k;
  std::sort(idx.begin(), idx.end(), [&](int a, int b) {
    if (ip[(size_t)(2 * a)] != ip[(size_t)(2 * b)]) return ip[(size_t)(2 * a)] < ip[(size_t)(2 * b)];
    if (ip[(size_t)(2 * a + 1)] != ip[(size_t)(2 * b + 1)]) return ip[(size_t)(2 * a + 1)] < ip[(size_t)(2 * b + 1)];
    return a < b;
  });
  idx.erase(std::unique(idx.begin(), idx.end(), [&](int a, int b) {
    return ip[(size_t)(2 * a)] == ip[(size_t)(2 * b)] && ip[(size_t)(2 * a + 1)] == ip[(size_t)(2 * b + 1)];
  }), idx.end());
  std::vector<int> hull;
  auto push = [&](int k, size_t base) {
    while (hull.size() >= base + 2 && cross3(&ip[(size_t)(2 * hull[hull.size() - 2])], &ip[(size_t)(2 * hull.back())], &ip[(size_t)(2 * k)]) <= 0)
      hull.pop_back();
    hull.push_back(k);
  };
  for (size_t k = 0; k < idx.size(); ++k) push(idx[k], 0);
  const size_t lower = hull.size();
  for (size_t k = idx.size() - 1; k-- > 0;) push(idx[k], lower - 1);
  if (hull.size() > 1) hull.pop_back();  // the first vertex again
  const int nh = (int)hull.size();
  if (nh < 4) return CLC_CHESS_NO_GRID;
  // the quadrilateral of the largest area (twice the area, exact)
  auto X = [&](int v) { return ip[(size_t)(2 * hull[(size_t)v])]; };
  auto Y = [&](int v) { return ip[(size_t)(2 * hull[(size_t)v] + 1)]; };
  long long best_area = -1;
  int q[4] = {0, 1, 2, 3};
  for (int a = 0; a < nh - 3; ++a)
    for (int b = a + 1; b < nh - 2; ++b)
      for (int c = b + 1; c < nh - 1; ++c)
        for (int d = c + 1; d < nh; ++d) {
          const long long area = (X(a) * Y(b) - X(b) * Y(a)) + (X(b) * Y(c) - X(c) * Y(b)) + (X(c) * Y(d) - X(d) * Y(c)) + (X(d) * Y(a) - X(a) * Y(d));
          if (area > best_area) { best_area = area; q[0] = a; q[1] = b; q[2] = c; q[3] = d; }
        }
  // everything to [-1, 1]
  double cx = 0.0, cy = 0.0;
  for (int k = 0; k < n; ++k) { cx += (double)ip[(size_t)(2 * k)]; cy += (double)ip[(size_t)(2 * k + 1)]; }
  cx /= n; cy /= n;
  double scale = 1.0;
  for (int k = 0; k < n; ++k) scale = std::max(scale, std::max(std::fabs((double)ip[(size_t)(2 * k)] - cx), std::fabs((double)ip[(size_t)(2 * k + 1)] - cy)));
  std::vector<P2> cand((size_t)n), nodes((size_t)n);
  for (int k = 0; k < n; ++k) cand[(size_t)k] = P2{((double)ip[(size_t)(2 * k)] - cx) / scale, ((double)ip[(size_t)(2 * k + 1)] - cy) / scale};
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) nodes[(size_t)(i * cols + j)] = P2{2.0 * j / (cols - 1) - 1.0, 2.0 * i / (rows - 1) - 1.0};
  const std::vector<P2> corner_nodes = {nodes[0], nodes[(size_t)(cols - 1)], nodes[(size_t)(n - 1)], nodes[(size_t)(n - cols)]};
  int chosen = -1;
  std::vector<int> match((size_t)n), best_match;
  for (int k = 0; k < 4; ++k) {
    std::vector<P2> quad(4);
    for (int m = 0; m < 4; ++m) quad[(size_t)m] = cand[(size_t)hull[(size_t)q[(k + m) & 3]]];
    double h[8], worst = 0.0;
    if (!fit_homography(corner_nodes, quad, h)) continue;
    if (!match_pass(h, nodes, cand, cols, rows, tol, match, &worst)) continue;
    std::vector<P2> matched((size_t)n);
    for (int m = 0; m < n; ++m) matched[(size_t)m] = cand[(size_t)match[(size_t)m]];
    if (!fit_homography(nodes, matched, h)) continue;
    if (!match_pass(h, nodes, cand, cols, rows, tol, match, &worst)) continue;
    ++*n_labelings;
    const int o = match[0];
    const bool first = chosen < 0 || ip[(size_t)(2 * o + 1)] < ip[(size_t)(2 * chosen + 1)] ||
                       (ip[(size_t)(2 * o + 1)] == ip[(size_t)(2 * chosen + 1)] && ip[(size_t)(2 * o)] < ip[(size_t)(2 * chosen)]);
    if (first) { chosen = o; best_match = match; *worst_out = worst; }
  }
  if (chosen < 0) return CLC_CHESS_NO_GRID;
  for (int m = 0; m < n; ++m) index[m] = best_match[(size_t)m];
  return CLC_CHESS_FOUND;
}

// clc_chessboard_order behind its argument checks.
inline void order_images(const float* cand_xy, const int32_t* count, long long stride, long long n_images, int cols, int rows, double tol,
                         int32_t* index, int32_t* status, int32_t* n_labelings, double* worst) {
  const int n = cols * rows;
  for (long long i = 0; i < n_images; ++i) {
    int32_t* ix = index + i * n;
    for (int m = 0; m < n; ++m) ix[m] = -1;
    int32_t labelings = 0;
    double w = NAN;
    int st;
    if (status[i] == CLC_CHESS_OVERFLOW) st = CLC_CHESS_OVERFLOW;
    else if (count[i] < n) st = CLC_CHESS_TOO_FEW;
    else {
      st = order_image(cand_xy + i * stride * 2, cols, rows, tol, ix, &labelings, &w);
      if (st != CLC_CHESS_FOUND)
        for (int m = 0; m < n; ++m) ix[m] = -1;
    }
    status[i] = st;
    if (n_labelings) n_labelings[i] = labelings;
    if (worst) worst[i] = st == CLC_CHESS_FOUND ? w : NAN;
  }
}

}  // namespace chessorder
}  // namespace clc
