// clc_subpix.hpp — K24: sub-pixel corner refinement, cv::cornerSubPix (src/calcCamPose.cpp:20-22, :86-89) restated from its
// published algorithm for many corners of many images at once (DESIGN.md K24 states every rounding step).
//
//   per corner   cT = cI = the start (float32).  Per iteration:
//                  the integer neighbourhood (2 wx + 4) x (2 wy + 4) about cI into LDS, border replicated; the getRectSubPix patch
//                  S (2 wx + 3) x (2 wy + 3) is its bilinear blend with ONE fractional pair (patch_sample: four float32 products,
//                  added in a fixed order);
//                  per window pixel (i, j): tgx = S[i+1][j+2] - S[i+1][j], tgy = S[i+2][j+1] - S[i][j+1] (float32), the mask
//                  m = vy[i] vx[j] (float32, 0 in the zero zone), and in double a += tgx^2 m, b += tgx tgy m, c += tgy^2 m,
//                  bb1 += gxx px + gxy py, bb2 += gxy px + gyy py;
//                  the 2 x 2 solve, the shift, the four ways out (converged, max_iter, singular, left the image).
//                at the end a result farther than the half-window from cT is given up for cT.
//
//   corner_subpix_kernel   one wave (= one 64-thread workgroup) per corner.  The lanes stride over the neighbourhood to load it
//                          and over the window pixels in row-major index order (k = lane, lane + 64, ...) to sum them: five double
//                          sums per lane, wave_sum of clc_campose.hpp (a butterfly in a fixed order: every lane ends with the
//                          same bits), then every lane computes the solve and the decisions from them: they are wave-uniform
//                          without a broadcast.  LDS: the neighbourhood (at most 34 x 34 floats) and the two mask tables, 4 872 bytes.
//                          No atomics, no cross-workgroup traffic: the same bits on every run, for a corner alone or in a batch.
//
// The arithmetic is IEEE add, mul, div, sqrt and floor, without FMA contraction, and no transcendental runs on the device (the mask
// tables exp(-x^2) come from the host: subpix_model): tests/shim/subpix_shim.cpp compiles this header for the host with g++ and runs
// the same per-corner code with the lanes as loops, and the device is compared with it bit for bit.
#pragma once
#include "clc_campose.hpp"

namespace clc {
namespace sp {

constexpr int MAX_WIN = CLC_SUBPIX_MAX_WIN;
constexpr int MAX_SIDE = 2 * MAX_WIN + 4;  // the integer neighbourhood of the (2 w + 3) patch: one more row and column for the blend
constexpr int MAX_TABLE = 2 * MAX_WIN + 1;

// What the kernel takes of clc_subpix_options (checked and resolved by subpix_model).
struct SubpixModel {
  int32_t wx, wy;
  int32_t zx, zy;  // -1, -1: no zero zone
  int32_t max_iter, reserved;
  double eps2;      // eps^2: the stopping test is err > eps2
  double mask_sum;  // sum of the mask over the window, in double in row-major order
  float vx[MAX_TABLE], vy[MAX_TABLE];
};

struct SubpixArgs {
  int32_t wx, wy, zx, zy, max_iter, width, height, reserved;
  double eps2, mask_sum;
  long long pitch;  // bytes per image row
  const uint8_t* images;
  const float* vx;  // [2 wx + 1]
  const float* vy;  // [2 wy + 1]
  const float* in;  // [2 M'] (x, y), indexed by the absolute offsets
  const long long* off;  // [n_images + 1]
  long long first, n_corners, n_images;  // the call covers corners [first, first + n_corners)
  float* out;            // may be `in`
  int32_t* status;       // nullable
  int32_t* iterations;   // nullable
  double* strength;      // nullable
};

// What one corner's wave keeps in LDS (host: an ordinary object).
struct Patch {
  float nb[MAX_SIDE * MAX_SIDE];
  float vx[MAX_TABLE], vy[MAX_TABLE];
};

// The options as the kernel takes them: the zero zone resolved, eps squared, the mask tables vx[j] = expf(-x^2),
// x = (float)(j - wx) / wx (float32 throughout, the host's expf) and the mask's sum.  Host code, and the one place they are
// computed: the ABI unit and the host shim both call it.
inline SubpixModel subpix_model(const clc_subpix_options& o) {
  SubpixModel m{};
  m.wx = o.win_x; m.wy = o.win_y; m.max_iter = o.max_iter;
  const bool zone = o.zero_x >= 0 && o.zero_y >= 0 && 2 * o.zero_x + 1 < 2 * o.win_x + 1 && 2 * o.zero_y + 1 < 2 * o.win_y + 1;
  m.zx = zone ? o.zero_x : -1;
  m.zy = zone ? o.zero_y : -1;
  m.eps2 = o.eps * o.eps;
  for (int j = 0; j <= 2 * m.wx; ++j) {
    const float x = (float)(j - m.wx) / (float)m.wx;
    m.vx[j] = expf(-(x * x));
  }
  for (int i = 0; i <= 2 * m.wy; ++i) {
    const float y = (float)(i - m.wy) / (float)m.wy;
    m.vy[i] = expf(-(y * y));
  }
  double s = 0.0;
  for (int i = 0; i <= 2 * m.wy; ++i)
    for (int j = 0; j <= 2 * m.wx; ++j) {
      const bool in_zone = zone && i >= m.wy - m.zy && i <= m.wy + m.zy && j >= m.wx - m.zx && j <= m.wx + m.zx;
      const float v = m.vy[i] * m.vx[j];
      s += in_zone ? 0.0 : (double)v;
    }
  m.mask_sum = s;
  return m;
}

// f(lane) on every lane of the corner's wave (host: a loop over the 64 lanes).
template <class F>
CLC_HD void each_lane(F f) {
#if defined(__HIP_DEVICE_COMPILE__)
  f((int)(threadIdx.x & 63));
#else
  for (int l = 0; l < cp::POSE_LANES; ++l) f(l);
#endif
}

CLC_HD bool finite_f(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

CLC_HD bool inside_image(const SubpixArgs& a, float x, float y) {
  return x >= 0.0f && x < (float)a.width && y >= 0.0f && y < (float)a.height;  // false for a NaN
}

// Sample (r, c) of the getRectSubPix patch from the neighbourhood (row stride nx): the four products added in this order.
CLC_HD float patch_sample(const float* nb, int nx, int r, int c, float w00, float w01, float w10, float w11) {
  CLC_BF_NO_CONTRACT
  const float* p = nb + r * nx + c;
  return ((p[0] * w00 + p[1] * w01) + p[nx] * w10) + p[nx + 1] * w11;
}

// One corner (absolute index) of image `image`: every lane of its wave calls it (host: once).
CLC_HD void refine_corner(const SubpixArgs& a, long long corner, long long image, Patch& L) {
  CLC_BF_NO_CONTRACT
  const int W = 2 * a.wx + 1, H = 2 * a.wy + 1;  // the window
  const int NX = W + 3, NY = H + 3;              // the neighbourhood: NX * NY <= MAX_SIDE^2
  const float sx = a.in[2 * corner], sy = a.in[2 * corner + 1];
  float cx = sx, cy = sy;
  int32_t status = CLC_SUBPIX_MAX_ITER, iter = 0;
  double strength = __builtin_nan("");
  if (!(finite_f(sx) && finite_f(sy))) {
    status = CLC_SUBPIX_NONFINITE;
  } else if (!inside_image(a, sx, sy)) {
    status = CLC_SUBPIX_LEFT_IMAGE;
  } else {  // (every branch here is wave-uniform)
    each_lane([&](int lane) {
      if (lane < W) L.vx[lane] = a.vx[lane];
      if (lane < H) L.vy[lane] = a.vy[lane];
    });
    const uint8_t* img = a.images + image * ((long long)a.height * a.pitch);
    for (;;) {
      // the patch's top-left sample: cI - (P - 1) / 2 = cI - (w + 1); cI is inside the image, so the floors fit an int
      const float tlx = cx - (float)(a.wx + 1), tly = cy - (float)(a.wy + 1);
      const float fx = floorf(tlx), fy = floorf(tly);
      const float fa = tlx - fx, fb = tly - fy;
      const float w00 = (1.0f - fa) * (1.0f - fb), w01 = fa * (1.0f - fb), w10 = (1.0f - fa) * fb, w11 = fa * fb;
      const long long ipx = (long long)fx, ipy = (long long)fy;
      cp::wave_barrier();  // the last iteration's reads are done
      each_lane([&](int lane) {
        int r = lane / NX, c = lane - r * NX;
        const int dr = 64 / NX, dc = 64 - dr * NX;
        for (int k = lane; k < NX * NY; k += 64) {
          long long x = ipx + c, y = ipy + r;
          x = x < 0 ? 0 : (x > a.width - 1 ? a.width - 1 : x);
          y = y < 0 ? 0 : (y > a.height - 1 ? a.height - 1 : y);
          L.nb[k] = (float)img[y * a.pitch + x];
          r += dr; c += dc;
          if (c >= NX) { c -= NX; ++r; }
        }
      });
      cp::wave_barrier();
      double s[5];
      cp::wave_sum<5>([&](int lane, double* acc) {
        CLC_BF_NO_CONTRACT
        int i = lane / W, j = lane - i * W;
        const int di = 64 / W, dj = 64 - di * W;
        for (int k = lane; k < W * H; k += 64) {
          const bool in_zone = a.zx >= 0 && i >= a.wy - a.zy && i <= a.wy + a.zy && j >= a.wx - a.zx && j <= a.wx + a.zx;
          const float m = in_zone ? 0.0f : L.vy[i] * L.vx[j];
          const float tgx = patch_sample(L.nb, NX, i + 1, j + 2, w00, w01, w10, w11) - patch_sample(L.nb, NX, i + 1, j, w00, w01, w10, w11);
          const float tgy = patch_sample(L.nb, NX, i + 2, j + 1, w00, w01, w10, w11) - patch_sample(L.nb, NX, i, j + 1, w00, w01, w10, w11);
          const double gx = (double)tgx, gy = (double)tgy, dm = (double)m;
          const double gxx = (gx * gx) * dm, gxy = (gx * gy) * dm, gyy = (gy * gy) * dm;
          const double px = (double)(j - a.wx), py = (double)(i - a.wy);
          acc[0] = acc[0] + gxx;
          acc[1] = acc[1] + gxy;
          acc[2] = acc[2] + gyy;
          acc[3] = acc[3] + (gxx * px + gxy * py);
          acc[4] = acc[4] + (gxy * px + gyy * py);
          i += di; j += dj;
          if (j >= W) { j -= W; ++i; }
        }
      }, s);
      const double A = s[0], B = s[1], C = s[2], bb1 = s[3], bb2 = s[4];
      const double dac = A - C;
      strength = (((A + C) - sqrt(dac * dac + (4.0 * B) * B)) / 2.0) / a.mask_sum;
      const double det = A * C - B * B;
      if (fabs(det) <= 2.220446049250313e-16 * 2.220446049250313e-16) { status = CLC_SUBPIX_SINGULAR; break; }
      const double scale = 1.0 / det;
      const float nx = (float)(((double)cx + (C * scale) * bb1) - (B * scale) * bb2);
      const float ny = (float)(((double)cy - (B * scale) * bb1) + (A * scale) * bb2);
      const double ex = (double)nx - (double)cx, ey = (double)ny - (double)cy;
      const double err = ex * ex + ey * ey;
      cx = nx; cy = ny;
      if (!inside_image(a, cx, cy)) { status = CLC_SUBPIX_LEFT_IMAGE; break; }
      ++iter;
      if (!(err > a.eps2)) { status = CLC_SUBPIX_CONVERGED; break; }
      if (iter >= a.max_iter) break;  // CLC_SUBPIX_MAX_ITER
    }
    if (fabsf(cx - sx) > (float)a.wx || fabsf(cy - sy) > (float)a.wy) { cx = sx; cy = sy; status = CLC_SUBPIX_REVERTED; }
  }
  if (!bf::lead_lane()) return;
  a.out[2 * corner] = cx;
  a.out[2 * corner + 1] = cy;
  if (a.status) a.status[corner] = status;
  if (a.iterations) a.iterations[corner] = iter;
  if (a.strength) a.strength[corner] = strength;
}

// The image of a corner: the i with off[i] <= corner < off[i + 1] (empty images are stepped over), inside [0, n_images) whatever
// the offsets hold.
CLC_HD long long image_of(const SubpixArgs& a, long long corner) {
  long long lo = 0, hi = a.n_images;
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (a.off[mid + 1] <= corner) lo = mid + 1; else hi = mid;
  }
  return lo < a.n_images ? lo : a.n_images - 1;
}

#if defined(__HIPCC__)

// K24: one wave per corner.
static __global__ __launch_bounds__(64) void corner_subpix_kernel(const SubpixArgs a) {
  __shared__ Patch L;
  const long long corner = a.first + (long long)blockIdx.x;
  if ((long long)blockIdx.x >= a.n_corners) return;
  refine_corner(a, corner, image_of(a, corner), L);
}

#endif  // __HIPCC__

}  // namespace sp
}  // namespace clc
