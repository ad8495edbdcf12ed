// clc_boardorder.hpp — K26: the ordering of clc_chessorder.hpp ("Ordering into the board's grid", steps 1-6) on the
// device, one image per 64-lane workgroup (one wave), rule for rule.
//
//   exact int64      the rounded pixels, the order under (x, y, slot) by counting, the duplicates onto their smallest slot, the monotone
//                    chain (one lane), the quadrilateral of the largest shoelace area: per diagonal (a, c) twice the area is
//                    tri(a, b, c) + tri(a, c, d) with b and d independent; the hull is strictly convex, so each triangle's area rises,
//                    stays at most once and falls along its chain, and the FIRST largest b and d come from a bisection on the sign of
//                    the step: nh^2 / 2 diagonals over the lanes, 2 log2 nh steps each; the first tuple (a, b, c, d) of the largest
//                    area under the lexicographic order, as the host's four nested loops find it
//   double           every add, mul, div and sqrt rounded on its own and in the host code's order (no contraction, no libm): the
//                    4-point systems and the normal equations (entry (i, k) of the 8 x 8 matrix on lane 8 i + k and the right-hand
//                    side on lanes 0-7, each summed over the matches in order, four matches' rows at a time through LDS), the
//                    elimination with partial pivoting (a row operation per lane, from one LDS copy of the system into the other),
//                    the predicted nodes, the squared distances, the nearest candidate (the first on ties), far.  The spacing is sqrt(dx dx + dy dy) where the host
//                    calls std::hypot: the one difference, in `worst` alone.
//
// Per-image state lives in dynamic LDS sized by n = cols rows (lds_bytes(n): 56 n + 2 784 bytes, 60 128 at n = 1024).  Every loop has a
// bound known on entry; the workgroups share nothing.  tests/shim/boardorder_shim.cpp compiles this header for the host with g++, the
// lanes a loop, and the tests hold it to clc_chessboard_order.
#pragma once
#include "../../include/clc.h"
#include "clc_math.hpp"

#include <stddef.h>
#include <stdint.h>

#if defined(__clang__)
#define CLC_BO_NO_CONTRACT _Pragma("clang fp contract(off)")
#define CLC_BO_ROLLED _Pragma("unroll 1")
#else
#define CLC_BO_NO_CONTRACT
#define CLC_BO_ROLLED
#endif

namespace clc {
namespace boardorder {

constexpr int LANES = 64;

struct OrderArgs {
  const float* cand_xy;  // [n_images][stride][2]
  const int32_t* count;  // [n_images]
  long long stride;
  long long first;       // the first image of this launch
  int32_t cols, rows;
  double tol;
  int32_t* index;        // [n_images][cols rows]
  int32_t* status;       // [n_images], read and written
  int32_t* n_labelings;  // [n_images], nullable
  double* worst;         // [n_images], nullable
};

struct GatherArgs {
  const float* cand_xy;
  const int32_t* index;
  const int32_t* status;
  long long stride, n_images;
  int32_t n;             // cols rows
  float* starts;         // [n_images][n][2]
  int32_t* found;        // [n_images]
  int64_t* offsets;      // [n_images + 1], nullable
  double* strength;      // [n_images][n], nullable: filled with NaN
};

// One image's LDS behind its base: 344 doubles and 8 flags of fixed state, then per candidate 4 doubles and 6 ints.  `sorted` shares
// `owner` (the order is needed for the hull alone), the chain's stack of 2 n slots shares `px`.
constexpr int FIXED_DOUBLES = 64 + 64 + 8 + 8 + 8 + 64 + 64 + 64;
constexpr int FIXED_BYTES = FIXED_DOUBLES * 8 + 8 * 4;

CLC_HD size_t lds_bytes(int n) { return (size_t)FIXED_BYTES + (size_t)n * (4 * 8 + 6 * 4); }

struct Lds {
  double* base;
  int n;
  CLC_HD double* A0() const { return base; }            // 64: the system, and its other copy
  CLC_HD double* A1() const { return base + 64; }
  CLC_HD double* b0() const { return base + 128; }      // 8, 8
  CLC_HD double* b1() const { return base + 136; }
  CLC_HD double* h() const { return base + 144; }       // 8
  CLC_HD double* red() const { return base + 152; }     // 64: a value per lane
  CLC_HD long long* qarea() const { return reinterpret_cast<long long*>(base + 216); }  // 64, 64
  CLC_HD long long* qkey() const { return reinterpret_cast<long long*>(base + 280); }
  CLC_HD double* cx() const { return base + FIXED_DOUBLES; }           // n each: the normalised candidates, the predicted nodes
  CLC_HD double* cy() const { return base + FIXED_DOUBLES + n; }
  CLC_HD double* px() const { return base + FIXED_DOUBLES + 2 * n; }
  CLC_HD double* py() const { return base + FIXED_DOUBLES + 3 * n; }
  CLC_HD int32_t* ints() const { return reinterpret_cast<int32_t*>(base + FIXED_DOUBLES + 4 * n); }
  CLC_HD int32_t* ipx() const { return ints(); }         // n each
  CLC_HD int32_t* ipy() const { return ints() + n; }
  CLC_HD int32_t* match() const { return ints() + 2 * n; }
  CLC_HD int32_t* best() const { return ints() + 3 * n; }
  CLC_HD int32_t* owner() const { return ints() + 4 * n; }
  CLC_HD int32_t* hull() const { return ints() + 5 * n; }
  CLC_HD int32_t* flag() const { return ints() + 6 * n; }  // 8: [0] a lane's refusal, [1] nh, [4..7] the quadrilateral's candidates
};

CLC_HD Lds carve(void* base, int n) { return Lds{static_cast<double*>(base), n}; }

// f(lane) on every lane of the image's wave (host: a loop), and the barrier between two such passes.
template <class F>
CLC_HD void lanes(F f) {
#if defined(__HIP_DEVICE_COMPILE__)
  f((int)threadIdx.x);
#else
  for (int l = 0; l < LANES; ++l) f(l);
#endif
}
CLC_HD void wave_sync() {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}

CLC_HD double dabs(double v) { return v < 0.0 ? -v : v; }
CLC_HD bool finite(double v) { return dabs(v) <= 1.7976931348623157e308; }  // (false for a NaN)

// v[0] = the smallest (op 0) or the largest (op 1) of v[0 .. 63], by halves across the lanes.
CLC_HD void fold64(double* v, int op) {
  for (int w = LANES / 2; w >= 1; w >>= 1) {
    lanes([&](int lane) {
      if (lane >= w) return;
      const double a = v[lane], b = v[lane + w];
      v[lane] = op ? (a < b ? b : a) : (b < a ? b : a);
    });
    wave_sync();
  }
}

// Twice the signed area of the hull vertices at positions p, q, r: (q - p) x (r - p), exact.
CLC_HD long long tri(const Lds& L, int p, int q, int r) {
  const int vp = L.hull()[p], vq = L.hull()[q], vr = L.hull()[r];
  const long long xp = L.ipx()[vp], yp = L.ipy()[vp];
  return ((long long)L.ipx()[vq] - xp) * ((long long)L.ipy()[vr] - yp) - ((long long)L.ipy()[vq] - yp) * ((long long)L.ipx()[vr] - xp);
}

// The first position t of [lo, hi] with the largest area(t), for an area that rises, stays at most once and falls over [lo, hi] (or a
// leading part of such a run): the first t with area(t + 1) <= area(t), hi where there is none.  At most 10 steps (hi - lo < 1024).
template <class F>
CLC_HD int first_largest(int lo, int hi, F area) {
  for (int it = 0; it < 11 && lo < hi; ++it) {
    const int mid = (lo + hi) >> 1;
    if (area(mid + 1) <= area(mid)) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Node m of the grid in [-1, 1]^2.
CLC_HD void node(int m, int cols, int rows, double* X, double* Y) {
  CLC_BO_NO_CONTRACT
  const int i = m / cols, j = m - i * cols;
  *X = 2.0 * (double)j / (double)(cols - 1) - 1.0;
  *Y = 2.0 * (double)i / (double)(rows - 1) - 1.0;
}

// Entry k of the match's row `which` (0: the u row, 1: the v row) with h33 = 1.
CLC_HD double row_entry(int which, int k, double X, double Y, double u, double v) {
  CLC_BO_NO_CONTRACT
  const double s = which ? v : u;
  if (k == 6) return -s * X;
  if (k == 7) return -s * Y;
  const int kk = which ? k - 3 : k;  // 0 1 2 of the row's own block
  return kk == 0 ? X : kk == 1 ? Y : kk == 2 ? 1.0 : 0.0;
}

// The 8 x 8 system in (A0, b0), solved into h as chessorder::solve8 does: the same pivots, the same operations.  -> false where a pivot
// vanishes or h is not finite.  Each elimination step goes from one copy of the system into the other, entry (r, k) on lane 8 r + k.
CLC_HD bool solve8(const Lds& L) {
  CLC_BO_NO_CONTRACT
  double *src = L.A0(), *dst = L.A1(), *bs = L.b0(), *bd = L.b1();
  CLC_BO_ROLLED
  for (int c = 0; c < 8; ++c) {
    int p = c;
    for (int r = c + 1; r < 8; ++r)
      if (dabs(src[r * 8 + c]) > dabs(src[p * 8 + c])) p = r;
    if (!(dabs(src[p * 8 + c]) > 1e-13)) return false;
    lanes([&](int lane) {
      CLC_BO_NO_CONTRACT
      const int r = lane >> 3, k = lane & 7;
      const int rs = r == c ? p : (r == p ? c : r);  // the row after the swap
      double v = src[rs * 8 + k], f = 0.0;
      if (r > c) {
        f = src[rs * 8 + c] / src[p * 8 + c];
        if (k >= c) { const double t = f * src[p * 8 + k]; v = v - t; }
      }
      dst[lane] = v;
      if (k == 7) {
        double w = bs[rs];
        if (r > c) { const double t = f * bs[p]; w = w - t; }
        bd[r] = w;
      }
    });
    wave_sync();
    double* t = src; src = dst; dst = t;
    t = bs; bs = bd; bd = t;
  }
  lanes([&](int lane) {
    CLC_BO_NO_CONTRACT
    if (lane != 0) return;
    for (int c = 7; c >= 0; --c) {
      double s = bs[c];
      for (int k = c + 1; k < 8; ++k) { const double t = src[c * 8 + k] * L.h()[k]; s = s - t; }
      L.h()[c] = s / src[c * 8 + c];
    }
  });
  wave_sync();
  bool ok = true;
  for (int c = 0; c < 8; ++c) ok = ok && finite(L.h()[c]);
  return ok;
}

// The rows of the matches m0 .. m0 + 3 (those below npts): entry k of row `which` of match m0 + mm on lane 16 mm + 8 which + k of
// rows[64], the match's pixel in uv[2 mm], uv[2 mm + 1].  pt(m, &X, &Y, &u, &v): match m.
template <class P>
CLC_HD void match_rows4(int m0, int npts, P pt, double* rows, double* uv) {
  lanes([&](int lane) {
    CLC_BO_NO_CONTRACT
    const int mm = lane >> 4, m = m0 + mm;
    if (m >= npts) return;
    double X, Y, u, v;
    pt(m, &X, &Y, &u, &v);
    rows[lane] = row_entry((lane >> 3) & 1, lane & 7, X, Y, u, v);
    if ((lane & 15) == 0) { uv[2 * mm] = u; uv[2 * mm + 1] = v; }
  });
}

// H through 4 matches (the system itself) or the least-squares H of more (the normal equations), as chessorder::fit_homography: entry
// (i, k) of the normal matrix on lane 8 i + k, the right-hand side on lanes 0-7, both summed over the matches in order, four matches'
// rows at a time through the system's other copy.
template <class P>
CLC_HD bool fit(const Lds& L, int npts, P pt) {
  CLC_BO_NO_CONTRACT
  if (npts == 4) {
    match_rows4(0, 4, pt, L.A0(), L.b0());  // rows 2 m and 2 m + 1 are lanes 16 m .. 16 m + 15; b[2 m] = u, b[2 m + 1] = v
  } else {
    lanes([&](int lane) {
      L.A0()[lane] = 0.0;
      if (lane < 8) L.b0()[lane] = 0.0;
    });
    CLC_BO_ROLLED
    for (int m0 = 0; m0 < npts; m0 += 4) {
      wave_sync();
      match_rows4(m0, npts, pt, L.A1(), L.b1());
      wave_sync();
      const int cnt = npts - m0 < 4 ? npts - m0 : 4;
      lanes([&](int lane) {
        CLC_BO_NO_CONTRACT
        const int i = lane >> 3, k = lane & 7;
        const double* rw = L.A1();
        double acc = L.A0()[lane];
        for (int mm = 0; mm < cnt; ++mm) {
          const double t0 = rw[16 * mm + i] * rw[16 * mm + k];
          const double t1 = rw[16 * mm + 8 + i] * rw[16 * mm + 8 + k];
          const double t = t0 + t1;
          acc = acc + t;
        }
        L.A0()[lane] = acc;
        if (lane < 8) {
          double bacc = L.b0()[lane];
          for (int mm = 0; mm < cnt; ++mm) {
            const double t0 = rw[16 * mm + lane] * L.b1()[2 * mm];
            const double t1 = rw[16 * mm + 8 + lane] * L.b1()[2 * mm + 1];
            const double t = t0 + t1;
            bacc = bacc + t;
          }
          L.b0()[lane] = bacc;
        }
      });
    }
  }
  wave_sync();
  return solve8(L);
}

// One pass, as chessorder::match_pass: the nodes under h, every node's nearest candidate, valid?  match[] and *worst.
CLC_HD bool match_pass(const Lds& L, int n, int cols, int rows, double tol, double* worst) {
  CLC_BO_NO_CONTRACT
  L.flag()[0] = 0;
  wave_sync();
  lanes([&](int lane) {
    CLC_BO_NO_CONTRACT
    for (int m = lane; m < n; m += LANES) {
      double X, Y;
      node(m, cols, rows, &X, &Y);
      const double w6 = L.h()[6] * X, w7 = L.h()[7] * Y;
      const double w = (w6 + w7) + 1.0;
      if (!(dabs(w) > 1e-12)) { L.flag()[0] = 1; continue; }
      const double a0 = L.h()[0] * X, a1 = L.h()[1] * Y, b0 = L.h()[3] * X, b1 = L.h()[4] * Y;
      const double x = ((a0 + a1) + L.h()[2]) / w, y = ((b0 + b1) + L.h()[5]) / w;
      L.px()[m] = x; L.py()[m] = y;
      if (!(finite(x) && finite(y))) L.flag()[0] = 1;
    }
  });
  wave_sync();
  if (L.flag()[0]) return false;
  lanes([&](int lane) {
    CLC_BO_NO_CONTRACT
    double part = __builtin_inf();
    for (int m = lane; m < n; m += LANES) {
      const int i = m / cols, j = m - i * cols;
      if (j + 1 < cols) {
        const double dx = L.px()[m + 1] - L.px()[m], dy = L.py()[m + 1] - L.py()[m];
        const double xx = dx * dx, yy = dy * dy;
        const double s = __builtin_sqrt(xx + yy);
        part = s < part ? s : part;
      }
      if (i + 1 < rows) {
        const double dx = L.px()[m + cols] - L.px()[m], dy = L.py()[m + cols] - L.py()[m];
        const double xx = dx * dx, yy = dy * dy;
        const double s = __builtin_sqrt(xx + yy);
        part = s < part ? s : part;
      }
    }
    L.red()[lane] = part;
  });
  wave_sync();
  fold64(L.red(), 0);  // (min and max of finite values do not depend on the order)
  const double spacing = L.red()[0];
  wave_sync();
  if (!(spacing > 0.0)) return false;
  lanes([&](int lane) {
    CLC_BO_NO_CONTRACT
    double part = 0.0;
    for (int m = lane; m < n; m += LANES) {
      const double x = L.px()[m], y = L.py()[m];
      int best = 0;
      double bd = __builtin_inf();
      for (int c = 0; c < n; ++c) {
        const double dx = L.cx()[c] - x, dy = L.cy()[c] - y;
        const double xx = dx * dx, yy = dy * dy;
        const double d = xx + yy;
        if (d < bd) { bd = d; best = c; }
      }
      bd = __builtin_sqrt(bd);
      L.match()[m] = best;
      L.owner()[best] = m;  // (of several nodes on one candidate one stays: the others find another's mark below)
      part = part < bd ? bd : part;
    }
    L.red()[lane] = part;
  });
  wave_sync();
  lanes([&](int lane) {
    for (int m = lane; m < n; m += LANES)
      if (L.owner()[L.match()[m]] != m) L.flag()[0] = 1;
  });
  wave_sync();
  fold64(L.red(), 1);
  const double far = L.red()[0];
  const bool bijection = L.flag()[0] == 0;
  *worst = far / spacing;
  const double gate = tol * spacing;
  return bijection && far <= gate;
}

// One image behind the count and status rules, as chessorder::order_image: -> CLC_CHESS_FOUND (the labeling in L.best()) or
// CLC_CHESS_NO_GRID.  hull_out [n] and quad_out [4] (hull positions), both nullable, are for the host tests.
CLC_HD int order_image(const Lds& L, const float* xy, int cols, int rows, double tol, int32_t* n_labelings, double* worst_out, int32_t* nh_out,
                       int32_t* hull_out, int32_t* quad_out) {
  CLC_BO_NO_CONTRACT
  const int n = cols * rows;
  *n_labelings = 0;
  *worst_out = __builtin_nan("");
  if (nh_out) *nh_out = 0;
  L.flag()[0] = 0;
  wave_sync();
  lanes([&](int lane) {
    for (int k = lane; k < n; k += LANES) {
      const float fx = xy[2 * k], fy = xy[2 * k + 1];
      const bool ok = (fx < 0.0f ? -fx : fx) <= 16777216.0f && (fy < 0.0f ? -fy : fy) <= 16777216.0f;  // (false for a NaN)
      if (!ok) L.flag()[0] = 1;
      const double dx = ok ? (double)fx : 0.0, dy = ok ? (double)fy : 0.0;
      L.ipx()[k] = (int32_t)(dx + (dx < 0.0 ? -0.5 : 0.5));  // half away from zero: the sum is exact, the conversion truncates
      L.ipy()[k] = (int32_t)(dy + (dy < 0.0 ? -0.5 : 0.5));
    }
  });
  wave_sync();
  if (L.flag()[0]) return CLC_CHESS_NO_GRID;
  // the order under (x, y, slot) by counting; a duplicate (match[k] = 1) falls onto its smallest slot
  int32_t* sorted = L.owner();
  lanes([&](int lane) {
    for (int k = lane; k < n; k += LANES) {
      const int x = L.ipx()[k], y = L.ipy()[k];
      int dup = 0;
      for (int j = 0; j < k; ++j) dup |= (L.ipx()[j] == x && L.ipy()[j] == y) ? 1 : 0;
      L.match()[k] = dup;
    }
  });
  wave_sync();
  lanes([&](int lane) {
    for (int k = lane; k < n; k += LANES) {
      if (L.match()[k]) continue;
      const int x = L.ipx()[k], y = L.ipy()[k];
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        const int xj = L.ipx()[j], yj = L.ipy()[j];
        rank += (!L.match()[j] && (xj < x || (xj == x && yj < y))) ? 1 : 0;
      }
      sorted[rank] = k;
    }
  });
  wave_sync();
  // the monotone chain on one lane; at most 2 n - 1 pushes, so the stack of 2 n slots holds it
  lanes([&](int lane) {
    if (lane != 0) return;
    int nu = 0;
    for (int k = 0; k < n; ++k) nu += L.match()[k] ? 0 : 1;
    int32_t* S = reinterpret_cast<int32_t*>(L.px());
    int sz = 0;
    auto push = [&](int k, int base) {
      while (sz >= base + 2) {
        const int a = S[sz - 2], b = S[sz - 1];
        const long long cr = ((long long)L.ipx()[b] - L.ipx()[a]) * ((long long)L.ipy()[k] - L.ipy()[b]) -
                             ((long long)L.ipy()[b] - L.ipy()[a]) * ((long long)L.ipx()[k] - L.ipx()[b]);
        if (cr > 0) break;
        --sz;
      }
      if (sz < 2 * n) S[sz++] = k;
    };
    for (int k = 0; k < nu; ++k) push(sorted[k], 0);
    const int lower = sz;
    for (int k = nu - 1; k-- > 0;) push(sorted[k], lower - 1);
    if (sz > 1) --sz;  // the first vertex again
    const int nh = sz < n ? sz : n;
    for (int k = 0; k < nh; ++k) L.hull()[k] = S[k];
    L.flag()[1] = nh;
  });
  wave_sync();
  const int nh = L.flag()[1];
  if (nh_out) *nh_out = nh;
  if (hull_out)
    for (int k = 0; k < nh; ++k) hull_out[k] = L.hull()[k];
  if (nh < 4) return CLC_CHESS_NO_GRID;
  // the quadrilateral of the largest area: the diagonals (a, c) over the lanes
  lanes([&](int lane) {
    long long best_area = -1, best_key = 0;
    for (int a = 0; a + 3 < nh; ++a)
      for (int c = a + 2 + lane; c + 1 < nh; c += LANES) {
        const int b = first_largest(a + 1, c - 1, [&](int t) { return tri(L, a, t, c); });
        const int d = first_largest(c + 1, nh - 1, [&](int t) { return tri(L, a, c, t); });
        const long long area = tri(L, a, b, c) + tri(L, a, c, d);
        const long long key = ((long long)a << 30) | ((long long)b << 20) | ((long long)c << 10) | (long long)d;
        if (area > best_area || (area == best_area && key < best_key)) { best_area = area; best_key = key; }
      }
    L.qarea()[lane] = best_area;
    L.qkey()[lane] = best_key;
  });
  wave_sync();
  for (int w = LANES / 2; w >= 1; w >>= 1) {  // (a total order: the fold does not depend on the order)
    lanes([&](int lane) {
      if (lane >= w) return;
      const long long ar = L.qarea()[lane + w], ky = L.qkey()[lane + w];
      if (ar > L.qarea()[lane] || (ar == L.qarea()[lane] && ky < L.qkey()[lane])) { L.qarea()[lane] = ar; L.qkey()[lane] = ky; }
    });
    wave_sync();
  }
  const long long best_key = L.qkey()[0];
  if (quad_out)
    for (int m = 0; m < 4; ++m) quad_out[m] = (int32_t)((best_key >> (30 - 10 * m)) & 1023);
  wave_sync();
  // everything to [-1, 1]: the sums are sums of integers below 2^53, exact in any order
  lanes([&](int lane) {
    CLC_BO_NO_CONTRACT
    if (lane != 0) return;
    for (int m = 0; m < 4; ++m) L.flag()[4 + m] = L.hull()[(int)((best_key >> (30 - 10 * m)) & 1023)];
    long long sx = 0, sy = 0;
    for (int k = 0; k < n; ++k) { sx += L.ipx()[k]; sy += L.ipy()[k]; }
    const double mx = (double)sx / (double)n, my = (double)sy / (double)n;
    double scale = 1.0;
    for (int k = 0; k < n; ++k) {
      const double ax = dabs((double)L.ipx()[k] - mx), ay = dabs((double)L.ipy()[k] - my);
      const double m2 = ax < ay ? ay : ax;
      scale = scale < m2 ? m2 : scale;
    }
    L.red()[0] = mx; L.red()[1] = my; L.red()[2] = scale;
  });
  wave_sync();
  lanes([&](int lane) {
    CLC_BO_NO_CONTRACT
    const double mx = L.red()[0], my = L.red()[1], scale = L.red()[2];
    for (int k = lane; k < n; k += LANES) {
      L.cx()[k] = ((double)L.ipx()[k] - mx) / scale;
      L.cy()[k] = ((double)L.ipy()[k] - my) / scale;
    }
  });
  wave_sync();
  int chosen = -1;
  CLC_BO_ROLLED
  for (int k = 0; k < 4; ++k) {
    double worst = 0.0;
    bool valid = true;
    // pass 0: the 4-point fit of the quadrilateral's rotation k; pass 1: the fit of all the matches of pass 0
    CLC_BO_ROLLED
    for (int pass = 0; pass < 2 && valid; ++pass) {
      valid = fit(L, pass ? n : 4, [&](int m, double* X, double* Y, double* u, double* v) {
        const int g = pass ? m : (m == 0 ? 0 : m == 1 ? cols - 1 : m == 2 ? n - 1 : n - cols);
        node(g, cols, rows, X, Y);
        const int c = pass ? L.match()[m] : L.flag()[4 + ((k + m) & 3)];
        *u = L.cx()[c]; *v = L.cy()[c];
      });
      valid = valid && match_pass(L, n, cols, rows, tol, &worst);
    }
    if (!valid) continue;
    ++*n_labelings;
    const int o = L.match()[0];
    const bool first = chosen < 0 || L.ipy()[o] < L.ipy()[chosen] || (L.ipy()[o] == L.ipy()[chosen] && L.ipx()[o] < L.ipx()[chosen]);
    if (first) {
      chosen = o;
      *worst_out = worst;
      lanes([&](int lane) {
        for (int m = lane; m < n; m += LANES) L.best()[m] = L.match()[m];
      });
      wave_sync();
    }
  }
  return chosen < 0 ? CLC_CHESS_NO_GRID : CLC_CHESS_FOUND;
}

// Image `img` of the arrays, as chessorder::order_images treats it: every lane of its wave calls this (host: once).
CLC_HD void order_one(const OrderArgs& a, long long img, void* lds, int32_t* nh_out = nullptr, int32_t* hull_out = nullptr,
                      int32_t* quad_out = nullptr) {
  const int n = a.cols * a.rows;
  const Lds L = carve(lds, n);
  const int st_in = a.status[img], cnt = a.count[img];
  int32_t labelings = 0;
  double w = __builtin_nan("");
  int st;
  if (nh_out) *nh_out = 0;
  if (st_in == CLC_CHESS_OVERFLOW) st = CLC_CHESS_OVERFLOW;
  else if (cnt < n) st = CLC_CHESS_TOO_FEW;
  else st = order_image(L, a.cand_xy + img * a.stride * 2, a.cols, a.rows, a.tol, &labelings, &w, nh_out, hull_out, quad_out);
  wave_sync();
  int32_t* ix = a.index + img * n;
  lanes([&](int lane) {
    for (int m = lane; m < n; m += LANES) ix[m] = st == CLC_CHESS_FOUND ? L.best()[m] : -1;
    if (lane == 0) {
      a.status[img] = st;
      if (a.n_labelings) a.n_labelings[img] = labelings;
      if (a.worst) a.worst[img] = st == CLC_CHESS_FOUND ? w : __builtin_nan("");
    }
  });
}

// The ordered candidate pixels of image `img` (NaN where no board was found), found and the offsets of clc_corner_subpix.
CLC_HD void gather_one(const GatherArgs& g, long long img) {
  const bool found = g.status[img] == CLC_CHESS_FOUND;
  const long long base = img * (long long)g.n;
  lanes([&](int lane) {
    for (int m = lane; m < g.n; m += LANES) {
      float x = __builtin_nanf(""), y = __builtin_nanf("");
      if (found) {
        const int32_t s = g.index[base + m];
        if (s >= 0 && (long long)s < g.stride) {
          x = g.cand_xy[(img * g.stride + s) * 2];
          y = g.cand_xy[(img * g.stride + s) * 2 + 1];
        }
      }
      g.starts[2 * (base + m)] = x;
      g.starts[2 * (base + m) + 1] = y;
      if (g.strength) g.strength[base + m] = __builtin_nan("");
    }
    if (lane == 0) {
      g.found[img] = found ? 1 : 0;
      if (g.offsets) {
        g.offsets[img] = (int64_t)base;
        if (img + 1 == g.n_images) g.offsets[img + 1] = (int64_t)(base + g.n);
      }
    }
  });
}

#if defined(__HIPCC__)

// K26: one wave per image of the launch; dynamic LDS lds_bytes(cols rows).
static __global__ __launch_bounds__(LANES) void board_order_kernel(const OrderArgs a) {
  extern __shared__ double board_lds[];
  order_one(a, a.first + (long long)blockIdx.x, board_lds);
}

// K26: the ordered starts of the refinement; `first`: the first image of the launch.
static __global__ __launch_bounds__(LANES) void board_gather_kernel(const GatherArgs g, long long first) {
  gather_one(g, first + (long long)blockIdx.x);
}

#endif  // __HIPCC__

}  // namespace boardorder
}  // namespace clc
