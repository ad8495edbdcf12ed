// clc_campose.hpp — K10: board poses from tag corners, the numeric half of CamPoseEst::calcCamPose (src/calcCamPose.cpp:270-303)
// for many images at once:
//
//   camera models   cam_lift / cam_project: camodocal's PinholeCamera and EquidistantCamera (Kannala-Brandt), the two models the
//                   reference's nodes select (main/kalibratag_detector_node.cpp:90-105)
//   campose_lift_kernel    one thread per corner: lift, x/z and y/z rounded to float32 (calcCamPose.cpp:284-286)
//   board_pose_kernel      one wave (= one 64-thread workgroup) per image: normalized DLT homography (45 accumulators, wave
//                          all-reduce, 9x9 Jacobi on one matrix row per lane), decomposition with the board in front, then the project's
//                          Ceres-semantics LM controller (clc_lm.hpp, Se3Manifold, no loss) on the K = I reprojection error;
//                          the lanes stride over the corners and all-reduce {H(21), g(6), cost} per evaluation, the controller
//                          runs on lane 0 with its state in LDS.  Registers: 256 VGPRs + 36 AGPRs, no scratch, SGPRs parked in VGPR lanes
//                          (the inlined controller step is what fills the budget; as a call it needs a 120-byte stack).
//
// Everything numeric is CLC_HD: tests/shim/campose_shim.cpp compiles this header for the host with g++ and runs the same
// per-image code with the 64 lanes as a loop (LaneRows of clc_batchflow.hpp: rows as an array), in the same summation order.
// The camera models and the DLT run without FMA contraction, so the pinhole lift / project are bit for bit the host's.
#pragma once
#include "../../include/clc.h"
#include "clc_math.hpp"
#include "clc_lm.hpp"
#include "clc_batchflow.hpp"

namespace clc {
namespace cp {

// ---------------------------------------------------------------------------------------
// Camera models
// ---------------------------------------------------------------------------------------

// PinholeCamera::distortion, PinholeCamera.cc:554-571.
CLC_HD void pinhole_distortion(const double* dist, double mx, double my, double* du) {
  CLC_BF_NO_CONTRACT
  const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3];
  const double mx2_u = mx * mx, my2_u = my * my, mxy_u = mx * my;
  const double rho2_u = mx2_u + my2_u;
  const double rad_dist_u = k1 * rho2_u + k2 * rho2_u * rho2_u;
  du[0] = mx * rad_dist_u + 2.0 * p1 * mxy_u + p2 * (rho2_u + 2.0 * mx2_u);
  du[1] = my * rad_dist_u + 2.0 * p2 * mxy_u + p1 * (rho2_u + 2.0 * my2_u);
}

CLC_HD bool pinhole_no_distortion(const clc_camera& c) {
  return c.dist[0] == 0.0 && c.dist[1] == 0.0 && c.dist[2] == 0.0 && c.dist[3] == 0.0;  // :196-205
}

// The odd polynomial of backprojectSymmetric (EquidistantCamera.cc:647-680): c[0..4] = coefficients of theta^1,3,5,7,9 and its
// degree npow, the degree dropping by 2 for every zero k (:647-663) — the coefficient slots stay where they are, so a zero inner
// k truncates the outer ones, as in the reference.
struct KbPoly {
  double c[5];
  int npow;
};

CLC_HD KbPoly kb_poly(const double* k) {
  KbPoly P;
  int npow = 9;
  if (k[3] == 0.0) npow -= 2;
  if (k[2] == 0.0) npow -= 2;
  if (k[1] == 0.0) npow -= 2;
  if (k[0] == 0.0) npow -= 2;
  P.npow = npow;
  P.c[0] = 1.0;
  P.c[1] = npow >= 3 ? k[0] : 0.0;
  P.c[2] = npow >= 5 ? k[1] : 0.0;
  P.c[3] = npow >= 7 ? k[2] : 0.0;
  P.c[4] = npow >= 9 ? k[3] : 0.0;
  // a zero leading slot (an inner k zero, an outer one not) leaves a polynomial of lower degree; the companion matrix of the
  // reference is then not defined — take the degree of the highest nonzero slot, as numpy's roots() does (constant indices only:
  // a dynamically indexed register array goes to scratch)
  int top = 0;
#pragma unroll
  for (int i = 1; i < 5; ++i)
    if (2 * i + 1 <= npow && P.c[i] != 0.0) top = i;
  P.npow = 2 * top + 1;
  return P;
}

// f(theta) = theta + c3 theta^3 + ... - p (Horner in theta^2)
CLC_HD double kb_f(const KbPoly& P, double p, double th, double* df) {
  CLC_BF_NO_CONTRACT
  const double t2 = th * th;
  double a = P.c[4], d = 9.0 * P.c[4];
  a = a * t2 + P.c[3]; d = d * t2 + 7.0 * P.c[3];
  a = a * t2 + P.c[2]; d = d * t2 + 5.0 * P.c[2];
  a = a * t2 + P.c[1]; d = d * t2 + 3.0 * P.c[1];
  a = a * t2 + 1.0;    d = d * t2 + 1.0;
  *df = d;
  return a * th - p;
}

// Safeguarded Newton / bisection on a bracket [a, b], fa = the sign of f at a (f(b) has the other sign): a Newton step is taken when
// it stays strictly inside the bracket, a bisection otherwise (f may report d = 0: bisection only); stops when the Newton step is
// below an ulp or the bracket cannot shrink any further.
template <class F>
CLC_HD double polish_root(F f, double a, double b, double fa) {
  CLC_BF_NO_CONTRACT
  double x = 0.5 * (a + b);
  for (int it = 0; it < 200; ++it) {
    double d;
    const double fx = f(x, &d);
    if (fx == 0.0) return x;
    if ((fx < 0.0) == (fa < 0.0)) a = x; else b = x;
    const double lo = a < b ? a : b, hi = a < b ? b : a;
    const double m = 0.5 * (a + b);
    if (!(m > lo && m < hi)) return x;
    const double xn = x - fx / d;
    if (xn > lo && xn < hi) {
      if (fabs(xn - x) <= 2.220446049250313e-16 * fabs(x)) return xn;
      x = xn;
    } else {
      x = m;
    }
  }
  return x;
}

// A polynomial of degree <= 4 in u, coefficients a[0..4] (low to high; constant indices only — a dynamically indexed register array
// goes to scratch).
CLC_HD double poly4(const double* a, double u) {
  CLC_BF_NO_CONTRACT
  return (((a[4] * u + a[3]) * u + a[2]) * u + a[1]) * u + a[0];
}

// The root of a polynomial that changes sign on [a, b] (fa: its value at a), by bisection to adjacent doubles.
CLC_HD double bisect4(const double* e, double a, double b, double fa) {
  CLC_BF_NO_CONTRACT
  for (int it = 0; it < 200; ++it) {
    const double m = 0.5 * (a + b);
    if (!(m > a && m < b)) break;
    const double fm = poly4(e, m);
    if (fm == 0.0) return m;
    if ((fm < 0.0) == (fa < 0.0)) { a = m; fa = fm; } else { b = m; }
  }
  return b;
}

// The critical points of f on (0, inf): f'(theta) = 1 + 3 c3 u + 5 c5 u^2 + 7 c7 u^3 + 9 c9 u^4 with u = theta^2.  Its positive roots
// in u are found level by level down the chain of its u-derivatives: the roots of the (j+1)-th derivative split (0, hi) into
// pieces on which the j-th is monotone, so each piece holds at most one root of it (a sign change, bisected).  hi: Cauchy's bound
// on the roots of f'.  Out: crit[4] ascending theta values, unused slots = inf.
CLC_HD void kb_critical(const KbPoly& P, double* crit) {
  CLC_BF_NO_CONTRACT
  const int top = (P.npow - 1) / 2;  // degree of f' in u, >= 1 here
  double E[5][5];                    // E[j]: the j-th u-derivative of f'
#pragma unroll
  for (int i = 0; i < 5; ++i) E[0][i] = (i <= top) ? (2.0 * i + 1.0) * P.c[i] : 0.0;
#pragma unroll
  for (int j = 1; j < 5; ++j) {
#pragma unroll
    for (int i = 0; i < 4; ++i) E[j][i] = (i + 1.0) * E[j - 1][i + 1];
    E[j][4] = 0.0;
  }
  double lead = 0.0, big = 0.0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    if (i == top) lead = fabs(E[0][i]);
    if (i < top) big = fmax(big, fabs(E[0][i]));
  }
  const double hi = 1.0 + big / lead;
  double r[4] = {hi, hi, hi, hi};  // roots of the level below, ascending; hi = none
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    if (top - j < 1) continue;  // a constant: no roots
    double nr[4] = {hi, hi, hi, hi};
    int cnt = 0;
    double a = 0.0, fa = poly4(E[j], 0.0);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double b = k < 4 ? r[k] : hi;
      if (b > a) {
        const double fb = poly4(E[j], b);
        if ((fa < 0.0 && fb >= 0.0) || (fa > 0.0 && fb <= 0.0)) {
          const double x = bisect4(E[j], a, b, fa);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (cnt == i) nr[i] = x;
          ++cnt;
        }
        a = b;
        fa = fb;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = nr[i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) crit[i] = r[i] < hi ? sqrt(r[i]) : __builtin_inf();
}

// theta of backprojectSymmetric for |p_u| = p: the smallest real root >= -1e-10 (clamped to 0) of f, or p when there is none.
// f(0) = -p < 0, so the root is the first sign change of f on [0, inf).  Between consecutive critical points (kb_critical) f is
// monotone: each piece [0, t1], [t1, t2], ..., [tm, B] holds at most one root, and the first piece whose right end is >= 0 holds the
// first one, which is then polished there.  B: Cauchy's bound on the roots of f (f(B) has the sign of the leading coefficient).
// A pair of roots as close as the local maximum between them is still found (a fixed grid steps over such pairs); only a tangent
// root that f touches without crossing, which the reference's 1e-10 imaginary-part test accepts as real, is not.
CLC_HD double kb_theta(const KbPoly& P, double p) {
  CLC_BF_NO_CONTRACT
  if (!(p > 0.0)) return p == 0.0 ? 0.0 : p;  // the centre (0 is a root); NaN stays NaN
  if (P.npow == 1) return p;
  const int top = (P.npow - 1) / 2;
  double lead = 0.0, big = fmax(1.0, p);
#pragma unroll
  for (int i = 1; i < 5; ++i) {
    if (i == top) lead = fabs(P.c[i]);
    if (i < top) big = fmax(big, fabs(P.c[i]));
  }
  const double B = 1.0 + big / lead;
  double crit[4];
  kb_critical(P, crit);
  auto f = [&](double th, double* d) { return kb_f(P, p, th, d); };
  double d;
  double a = 0.0, fa = -p;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double b = k < 4 ? fmin(crit[k], B) : B;
    if (b > a) {
      const double fb = kb_f(P, p, b, &d);
      if (fb == 0.0) return b;
      if (fb > 0.0) return polish_root(f, a, b, fa);
      a = b;
      fa = fb;
    }
  }
  return p;  // no admissible root (:721-724)
}

// liftProjective -> (x/z, y/z), unrounded.
CLC_HD void cam_lift(const clc_camera& c, double u, double v, double* xy) {
  CLC_BF_NO_CONTRACT
  if (c.model == CLC_CAMERA_PINHOLE) {
    const double inv_K11 = 1.0 / c.proj[0], inv_K13 = -c.proj[2] / c.proj[0];  // :208-211
    const double inv_K22 = 1.0 / c.proj[1], inv_K23 = -c.proj[3] / c.proj[1];
    const double mx_d = inv_K11 * u + inv_K13, my_d = inv_K22 * v + inv_K23;  // :365-366
    double mx_u = mx_d, my_u = my_d;
    if (!pinhole_no_distortion(c)) {  // recursive distortion model, :401-415
      double du[2];
      pinhole_distortion(c.dist, mx_d, my_d, du);
      mx_u = mx_d - du[0];
      my_u = my_d - du[1];
      for (int i = 1; i < 8; ++i) {
        pinhole_distortion(c.dist, mx_u, my_u, du);
        mx_u = mx_d - du[0];
        my_u = my_d - du[1];
      }
    }
    xy[0] = mx_u / 1.0;  // P = (mx_u, my_u, 1): x/z, y/z
    xy[1] = my_u / 1.0;
  } else {
    const double inv_K11 = 1.0 / c.proj[0], inv_K13 = -c.proj[2] / c.proj[0];
    const double inv_K22 = 1.0 / c.proj[1], inv_K23 = -c.proj[3] / c.proj[1];
    const double pux = inv_K11 * u + inv_K13, puy = inv_K22 * v + inv_K23;  // :345-346
    const double pn = sqrt(pux * pux + puy * puy);
    const double phi = pn < 1e-10 ? 0.0 : atan2(puy, pux);  // :637-645
    const double theta = kb_theta(kb_poly(c.dist), pn);
    const double st = sin(theta), ct = cos(theta);  // :351-355
    xy[0] = (st * cos(phi)) / ct;
    xy[1] = (st * sin(phi)) / ct;
  }
}

// spaceToPlane of the camera-frame point P.
CLC_HD void cam_project(const clc_camera& c, const double* P, double* px) {
  CLC_BF_NO_CONTRACT
  if (c.model == CLC_CAMERA_PINHOLE) {  // PinholeCamera.cc:428-453
    double pd0 = P[0] / P[2], pd1 = P[1] / P[2];
    if (!pinhole_no_distortion(c)) {
      double du[2];
      pinhole_distortion(c.dist, pd0, pd1, du);
      pd0 = pd0 + du[0];
      pd1 = pd1 + du[1];
    }
    px[0] = c.proj[0] * pd0 + c.proj[2];
    px[1] = c.proj[1] * pd1 + c.proj[3];
  } else {  // EquidistantCamera.cc:364-377, r() of EquidistantCamera.h:153-161
    const double nrm = sqrt(P[0] * P[0] + P[1] * P[1] + P[2] * P[2]);
    const double theta = acos(P[2] / nrm);
    const double phi = atan2(P[1], P[0]);
    const double k2 = c.dist[0], k3 = c.dist[1], k4 = c.dist[2], k5 = c.dist[3], t = theta;
    const double r = t + k2 * t * t * t + k3 * t * t * t * t * t + k4 * t * t * t * t * t * t * t +
                     k5 * t * t * t * t * t * t * t * t * t;
    px[0] = c.proj[0] * (r * cos(phi)) + c.proj[2];
    px[1] = c.proj[1] * (r * sin(phi)) + c.proj[3];
  }
}

// The transform of clc_camera_project: p_c = R(q) p + t, pose7 = [t, qx, qy, qz, qw] (showscan_node.cpp:86-89).
CLC_HD void pose_apply(const double* pose7, const double* p, double* out) {
  CLC_BF_NO_CONTRACT
  double R[9];
  quat_to_rot(pose7 + 3, R);
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = ((R[3 * i] * p[0] + R[3 * i + 1] * p[1]) + R[3 * i + 2] * p[2]) + pose7[i];
}

// ---------------------------------------------------------------------------------------
// The wave of one image: 64 lanes, all-reduce by butterfly (each stage adds a value and its partner's: every lane ends with the
// same bits).  On the host the lanes are a loop and the butterfly is spelled out in the same order.
// ---------------------------------------------------------------------------------------
constexpr int POSE_LANES = 64;

struct Pose7Arg {  // a pose passed to a kernel by value
  double v[7];
};

// f(lane, acc) accumulates lane `lane`'s share into acc[K] (zeroed); out[K] = the sum over the 64 lanes, on every lane.
template <int K, class F>
CLC_HD void wave_sum(F f, double* out) {
  CLC_BF_NO_CONTRACT
#if defined(__HIP_DEVICE_COMPILE__)
  double acc[K];
#pragma unroll
  for (int i = 0; i < K; ++i) acc[i] = 0.0;
  f((int)(threadIdx.x & 63), acc);
#pragma unroll
  for (int i = 0; i < K; ++i) {
    double v = acc[i];
    v = v + dpp_read<0xB1>(v);   // xor 1
    v = v + dpp_read<0x4E>(v);   // xor 2
    v = v + dpp_read<0x141>(v);  // row_half_mirror: the other quad's (equal) sums
    v = v + dpp_read<0x140>(v);  // row_mirror: the other half-row's sums
    v = v + __shfl_xor(v, 16, 64);
    v = v + __shfl_xor(v, 32, 64);
    out[i] = v;
  }
#else
  static thread_local double acc[POSE_LANES][K > 0 ? K : 1];
  for (int l = 0; l < POSE_LANES; ++l) {
    for (int i = 0; i < K; ++i) acc[l][i] = 0.0;
    f(l, acc[l]);
  }
  for (int o = 1; o < POSE_LANES; o <<= 1)
    for (int l = 0; l < POSE_LANES; ++l)
      if (!(l & o))
        for (int i = 0; i < K; ++i) {
          const double v = acc[l][i] + acc[l ^ o][i];
          acc[l][i] = v;
          acc[l ^ o][i] = v;
        }
  for (int i = 0; i < K; ++i) out[i] = acc[0][i];
#endif
}

CLC_HD void wave_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();  // the workgroup is the one wave
#endif
}

// What one image keeps in LDS: the 45 DLT accumulators (rows are read from here by lane), the controller's state and temporaries.
struct PoseShared {
  double acc45[45];
  double e[28];  // the all-reduced {H, g, sum r^2} the controller reads
  double x0[7];  // the start pose
  double R0[9];  // its rotation
  LmStateT<Se3Manifold> st;
  LmScratchT<Se3Manifold> w;
  clc_summary sm;
  int32_t status;
};

constexpr double POSE_DEGENERATE_RATIO = 1e-10;  // second-smallest / largest eigenvalue of the normalized DLT normal matrix

// The DLT row pair of one correspondence (normalized image x, y; normalized board X, Y) into the 45 upper-triangle entries of A^T A.
CLC_HD void dlt_accumulate(double x, double y, double X, double Y, double* acc) {
  CLC_BF_NO_CONTRACT
  const double a1[9] = {X, Y, 1.0, 0.0, 0.0, 0.0, -x * X, -x * Y, -x};
  const double a2[9] = {0.0, 0.0, 0.0, X, Y, 1.0, -y * X, -y * Y, -y};
  int k = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int j = i; j < 9; ++j) {
      acc[k] = fma(a1[i], a1[j], acc[k]);
      acc[k] = fma(a2[i], a2[j], acc[k]);
      ++k;
    }
}

CLC_HD int tri9(int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo * 9 - (lo * (lo - 1)) / 2 + (hi - lo);
}

// Reprojection residual (K = I) of board point (X, Y, 0) against the lifted x at pose [t, q(xyzw)] and its Jacobian in the
// PoseLocalParameterization tangent [dt, dtheta] (R+ = R Exp(dtheta): dP/dtheta = -R [X]x).  Accumulates H (21, tri<6> order),
// g (6) and sum r^2 (infinite when a point lies behind the camera) into acc[28].
CLC_HD void reproj_accumulate(const double* R, const double* t, double X, double Y, double u, double v, double* acc) {
  CLC_BF_NO_CONTRACT
  const double P0 = (R[0] * X + R[1] * Y) + t[0];
  const double P1 = (R[3] * X + R[4] * Y) + t[1];
  const double P2 = (R[6] * X + R[7] * Y) + t[2];
  const double iz = 1.0 / P2;
  const double xn = P0 * iz, yn = P1 * iz;
  const double r[2] = {xn - u, yn - v};
  // dr/dP = [[iz, 0, -xn iz], [0, iz, -yn iz]]; B = dr/dP R
  double J[2][6];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double a0 = i == 0 ? iz : 0.0, a1 = i == 0 ? 0.0 : iz, a2 = -(i == 0 ? xn : yn) * iz;
    const double B0 = (a0 * R[0] + a1 * R[3]) + a2 * R[6];
    const double B1 = (a0 * R[1] + a1 * R[4]) + a2 * R[7];
    const double B2 = (a0 * R[2] + a1 * R[5]) + a2 * R[8];
    J[i][0] = a0; J[i][1] = a1; J[i][2] = a2;
    J[i][3] = B2 * Y;
    J[i][4] = -(B2 * X);
    J[i][5] = B1 * X - B0 * Y;
  }
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) {
      acc[k] = fma(J[0][a], J[0][b], acc[k]);
      acc[k] = fma(J[1][a], J[1][b], acc[k]);
      ++k;
    }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    acc[21 + a] = fma(J[0][a], r[0], acc[21 + a]);
    acc[21 + a] = fma(J[1][a], r[1], acc[21 + a]);
  }
  acc[27] = fma(r[0], r[0], acc[27]);
  acc[27] = fma(r[1], r[1], acc[27]);
  // (R X + t)/z is the same for -(R X + t): a point behind the camera fits exactly as well as one in front.  Such a pose is an invalid
  // evaluation (Ceres: the cost function returns false): an infinite sum, so the controller rejects it as a candidate (a failure at
  // the start).  Without it a large step can land on the mirror image of the board behind the camera.
  if (!(P2 > 0.0)) acc[27] += __builtin_inf();
}

// One image: lifted[2n] (the float32-rounded x/z, y/z), board[2n].  Every lane calls it (device: the image's wave; host: once).
// Returns the CLC_POSE_* status (wave-uniform); on CLC_POSE_OK pose7 = [t, qx, qy, qz, qw], *rms and sh.sm are set.
CLC_HD int board_pose_image(const clc_options& o, const float* __restrict__ lifted, const float* __restrict__ board, long long n,
                            PoseShared& sh, double* pose7, double* rms) {
  CLC_BF_NO_CONTRACT
  if (n < 4) return CLC_POSE_TOO_FEW;  // EstimatePose, :217
  // ---- pass 1: centroids and spreads of both point sets (Hartley normalization), non-finite count ----
  double m[9];
  wave_sum<9>([&](int lane, double* a) {
    for (long long k = lane; k < n; k += POSE_LANES) {
      const double x = lifted[2 * k], y = lifted[2 * k + 1], X = board[2 * k], Y = board[2 * k + 1];
      if (!(isfinite(x) && isfinite(y) && isfinite(X) && isfinite(Y))) { a[8] += 1.0; continue; }
      a[0] += x; a[1] += y; a[2] = fma(x, x, a[2]); a[3] = fma(y, y, a[3]);
      a[4] += X; a[5] += Y; a[6] = fma(X, X, a[6]); a[7] = fma(Y, Y, a[7]);
    }
  }, m);
  if (m[8] != 0.0) return CLC_POSE_NONFINITE;
  const double inv_n = 1.0 / (double)n;
  const double cx = m[0] * inv_n, cy = m[1] * inv_n, cX = m[4] * inv_n, cY = m[5] * inv_n;
  const double var_i = (m[2] + m[3]) * inv_n - (cx * cx + cy * cy), var_b = (m[6] + m[7]) * inv_n - (cX * cX + cY * cY);
  if (!(var_i > 0.0 && var_b > 0.0)) return CLC_POSE_DEGENERATE;
  const double si = sqrt(2.0 / var_i), sb = sqrt(2.0 / var_b);  // RMS distance sqrt(2) after scaling
  // ---- pass 2: A^T A of the normalized DLT ----
  double acc[45];
  wave_sum<45>([&](int lane, double* a) {
    for (long long k = lane; k < n; k += POSE_LANES)
      dlt_accumulate((lifted[2 * k] - cx) * si, (lifted[2 * k + 1] - cy) * si, (board[2 * k] - cX) * sb, (board[2 * k + 1] - cY) * sb, a);
  }, acc);
  if (bf::lead_lane())
    for (int i = 0; i < 45; ++i) sh.acc45[i] = acc[i];
  wave_barrier();
  bf::LaneRows<9> A, V;
  A.each([&](int k, double* row) {
#pragma unroll
    for (int j = 0; j < 9; ++j) row[j] = sh.acc45[tri9(k, j)];
  });
  double w[9];
  bf::jacobi_rows<9, true>(A, V, w);  // descending; the null vector is column 8
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) finite = finite && isfinite(w[i]);
  if (!finite) return CLC_POSE_NONFINITE;
  if (!(w[7] > POSE_DEGENERATE_RATIO * w[0])) return CLC_POSE_DEGENERATE;
  double hn[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) hn[i] = V.at(i, 8);
  // H = Ti^-1 Hn Tb, Ti = [si 0 -si cx; 0 si -si cy; 0 0 1], Tb likewise
  double Hb[9];  // Hn Tb
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    Hb[3 * r] = hn[3 * r] * sb;
    Hb[3 * r + 1] = hn[3 * r + 1] * sb;
    Hb[3 * r + 2] = (hn[3 * r + 2] - hn[3 * r] * sb * cX) - hn[3 * r + 1] * sb * cY;
  }
  double H[9];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    H[j] = Hb[j] / si + cx * Hb[6 + j];
    H[3 + j] = Hb[3 + j] / si + cy * Hb[6 + j];
    H[6 + j] = Hb[6 + j];
  }
  // H ~ [r1 r2 t]: scale by the mean column norm
  const double n1 = sqrt((H[0] * H[0] + H[3] * H[3]) + H[6] * H[6]), n2 = sqrt((H[1] * H[1] + H[4] * H[4]) + H[7] * H[7]);
  double lam = 2.0 / (n1 + n2);
  // the sign that puts the board in front: the projective depth at the corners' centroid (the board origin can lie on the far side
  // of the homography's line at infinity when only a tag far from it is seen — its depth, t_z, then has the wrong sign)
  if ((H[6] * cX + H[7] * cY) + H[8] < 0.0) lam = -lam;
  const double r1[3] = {lam * H[0], lam * H[3], lam * H[6]}, r2[3] = {lam * H[1], lam * H[4], lam * H[7]};
  double r3[3];
  bf::cross3(r1, r2, r3);
  const double M[9] = {r1[0], r2[0], r3[0], r1[1], r2[1], r3[1], r1[2], r2[2], r3[2]};
  // the start pose and the controller's initialisation on lane 0, through LDS (rot_to_quat_xyzw indexes its matrix at run time)
  if (bf::lead_lane()) {
    bf::nearest_orthogonal3(M, sh.R0);
    sh.x0[0] = lam * H[2]; sh.x0[1] = lam * H[5]; sh.x0[2] = lam * H[8];
    bf::rot_to_quat_xyzw(sh.R0, sh.x0 + 3);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 7; ++i) ok = ok && isfinite(sh.x0[i]);
    sh.status = ok ? CLC_POSE_OK : CLC_POSE_NONFINITE;
    if (ok) lm_init(sh.st, o, sh.x0);
  }
  wave_barrier();
  if (sh.status != CLC_POSE_OK) return CLC_POSE_NONFINITE;
  // ---- LM on the reprojection error: lane 0 runs the controller, every lane evaluates ----
  while (sh.st.status == CLC_RUNNING) {
    double xe[7], R[9];
#pragma unroll
    for (int i = 0; i < 7; ++i) xe[i] = sh.st.x_eval[i];
    quat_to_rot(xe + 3, R);
    double e[28];
    wave_sum<28>([&](int lane, double* a) {
      for (long long k = lane; k < n; k += POSE_LANES)
        reproj_accumulate(R, xe, board[2 * k], board[2 * k + 1], lifted[2 * k], lifted[2 * k + 1], a);
    }, e);
    wave_barrier();
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 28; ++i) sh.e[i] = e[i];
      lm_advance(sh.st, sh.w, o, nullptr, 0, 0.5 * sh.e[27], sh.e + 21, sh.e);
    }
    wave_barrier();
  }
  if (bf::lead_lane()) lm_fill_summary(sh.st, sh.sm);
  wave_barrier();
#pragma unroll
  for (int i = 0; i < 7; ++i) pose7[i] = sh.st.x_out[i];
  const double fc = sh.sm.final_cost;
  finite = isfinite(fc) && sh.st.status != CLC_FAILURE;
#pragma unroll
  for (int i = 0; i < 7; ++i) finite = finite && isfinite(pose7[i]);
  if (!finite) return CLC_POSE_NONFINITE;
  *rms = sqrt(2.0 * fc / (double)n);
  return CLC_POSE_OK;
}

// The outputs of one image (lead lane / host): q as w, x, y, z with w >= 0.
CLC_HD void board_pose_store(int st, const double* pose7, double rms, long long img, double* q_wxyz, double* t, double* rms_out,
                             int32_t* status) {
  status[img] = st;
  if (st == CLC_POSE_OK) {
    const double sgn = pose7[6] < 0.0 ? -1.0 : 1.0;
    q_wxyz[4 * img] = sgn * pose7[6];
    q_wxyz[4 * img + 1] = sgn * pose7[3];
    q_wxyz[4 * img + 2] = sgn * pose7[4];
    q_wxyz[4 * img + 3] = sgn * pose7[5];
    for (int i = 0; i < 3; ++i) t[3 * img + i] = pose7[i];
    if (rms_out) rms_out[img] = rms;
  } else {
    q_wxyz[4 * img] = 1.0;
    q_wxyz[4 * img + 1] = 0.0;
    q_wxyz[4 * img + 2] = 0.0;
    q_wxyz[4 * img + 3] = 0.0;
    for (int i = 0; i < 3; ++i) t[3 * img + i] = 0.0;
    if (rms_out) rms_out[img] = __builtin_nan("");
  }
}

CLC_HD void summary_empty(clc_summary& s) {
  s.termination = 0; s.num_iterations = 0; s.num_successful_steps = 0; s.num_unsuccessful_steps = 0;
  s.num_evaluations = 0; s.initial_cost = 0.0; s.final_cost = 0.0; s.solve_ms = 0.0; s.eval_kernel_ms = 0.0;
  s.eval_kernel_launches = 0;
}

#if defined(__HIPCC__)

constexpr int LIFT_THREADS = 256;

// clc_camera_lift (ROUND = false: doubles out) and the first step of clc_board_poses (ROUND: float32 x/z, y/z, :284-286).
template <bool ROUND>
__global__ __launch_bounds__(LIFT_THREADS) void campose_lift_kernel(const clc_camera cam, const float* __restrict__ px, const long long n,
                                                                    double* __restrict__ out_d, float* __restrict__ out_f) {
  const long long i = (long long)blockIdx.x * LIFT_THREADS + threadIdx.x;
  if (i >= n) return;
  double xy[2];
  cam_lift(cam, (double)px[2 * i], (double)px[2 * i + 1], xy);
  if (ROUND) {
    out_f[2 * i] = (float)xy[0];
    out_f[2 * i + 1] = (float)xy[1];
  } else {
    out_d[2 * i] = xy[0];
    out_d[2 * i + 1] = xy[1];
  }
}

// clc_camera_project: one thread per point.
static __global__ __launch_bounds__(LIFT_THREADS) void campose_project_kernel(const clc_camera cam, const Pose7Arg pose, const int has_pose,
                                                                              const double* __restrict__ pts, const long long n,
                                                                              double* __restrict__ px) {
  const long long i = (long long)blockIdx.x * LIFT_THREADS + threadIdx.x;
  if (i >= n) return;
  double P[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
  if (has_pose) {
    double Q[3];
    pose_apply(pose.v, P, Q);
    P[0] = Q[0]; P[1] = Q[1]; P[2] = Q[2];
  }
  double o[2];
  cam_project(cam, P, o);
  px[2 * i] = o[0];
  px[2 * i + 1] = o[1];
}

// K10: one 64-thread workgroup (one wave) per image.  lifted: the rounded x/z, y/z of campose_lift_kernel<true> for the corners
// [first, off[n_images]) (lifted[0] is corner `first`); board indexed by the absolute offsets.
static __global__ __launch_bounds__(64) void board_pose_kernel(const clc_options opt, const float* __restrict__ lifted,
                                                               const float* __restrict__ board, const long long* __restrict__ off,
                                                               const long long first, double* __restrict__ q_wxyz,
                                                               double* __restrict__ t, double* __restrict__ rms,
                                                               int32_t* __restrict__ status, clc_summary* __restrict__ summaries) {
  __shared__ PoseShared sh;
  const long long img = blockIdx.x;
  const long long b = off[img], n = off[img + 1] - b;
  double pose7[7], r = 0.0;
  const int st = board_pose_image(opt, lifted + 2 * (b - first), board + 2 * b, n, sh, pose7, &r);
  if (threadIdx.x == 0) {
    board_pose_store(st, pose7, r, img, q_wxyz, t, rms, status);
    if (summaries) {
      if (st == CLC_POSE_OK) summaries[img] = sh.sm;
      else summary_empty(summaries[img]);
    }
  }
}

#endif  // __HIPCC__

}  // namespace cp
}  // namespace clc
