// clc_fullcal.hpp — K23: one robust cost over the camera's intrinsics, every board pose, T_cl and the scanner's range offset and scale.
//
//   corner j of image i   e_j = (project(cam, R_i X_j + t_i) - u_j) / sigma_px                      K19's residual: pixels, no lift
//   laser point k         r_k = e3^T R_i^T (R_cl p'_k + t_cl - t_i) / sigma_laser,  p' = (1 + kappa + b / |p|) p            (K21)
//   cost = 1/2 sum rho_ac(|e_j|^2) + 1/2 sum rho_al(r_k^2)        rho_a(z) = a^2 log1p(z / a^2), rho_a'(z) = 1 / (1 + z / a^2); a = 0: z
//
// The loss is K22's: one loss on a corner's residual 2-vector, Ceres' corrector for rho'' <= 0 (rows and residual scaled by
// sqrt(rho')), so the Gauss-Newton blocks take w J^T J and w J^T r with w = rho'(z).  The fifth arrow problem of clc_arrow.hpp, with
// a 16-wide shared block
//
//   [dt_cl(3), dtheta_cl(3), b, kappa, proj[0..3], dist[0..3]]       the leading 8 as K21's H_cr, the trailing 8 in clc_camera order
//
// T_cl moves on its tangent, b, kappa and the intrinsics additively.  The laser rows do not depend on the intrinsics and the corner
// rows not on T_cl, b, kappa: the [T_cl, range] x intrinsics block of C is exactly zero, it is written as zeros and never summed; the
// two groups couple only through the board poses in the Schur complement.  The range correction (clc_laserrange.hpp) and the Cauchy
// weight (clc_jointrobust.hpp) are restated here in their few lines: those headers belong to their own units.
//
//   fullcal_kernel   one 256-thread workgroup (4 waves) per problem, the whole Levenberg-Marquardt solve in one launch.
//     evaluation   per image a wave all-reduces K19's four corner passes with each corner's rows weighted by rho' — {A_i, g_i, sum rho}
//                  (28), {B_i[:, 8:12], g_c[8:16]} (32), B_i[:, 12:16] (24), C[8:16, 8:16] (36) — and four weighted passes over the laser
//                  points — {A_i, g_i, sum rho} (28), B_i[:, 0:6] (36), {B_i[:, 6:8], g_c[0:8]} (20), C[0:8, 0:8] (36) —, the residual
//                  recomputed in each: 240 sums, never more than 36 live.
//     reduced system   thread 0 compacts it to the free shared parameters (up to 16) and solves it with a rolled run-time-n Cholesky
//                  on its LDS copy.  A held parameter has scale 0 and keeps its bits; a problem without a laser point holds T_cl, b and
//                  kappa by itself.
//   fullcal_weights_kernel   one workgroup per problem, one wave per image: rho' of every observation at the returned point.
//   Per-image state: FullImage, 8.3 KB.  With the board poses and all 8 intrinsics held the corner terms are constant: they are left
//   out and no corner is read (K21's rule).
//
// Everything numeric is CLC_HD: tests/shim/fullcal_shim.cpp compiles this header for the host with g++ and runs the same code with
// the threads as loops, in the same summation order (log1p is the platform's: the device and the host build agree to rounding where
// a loss is on).
#pragma once
#include "clc_arrow.hpp"
#include "clc_camcal.hpp"

namespace clc {
namespace fc {

using aw::finite_d;

constexpr int FULL_THREADS = aw::ARROW_THREADS;
constexpr int NF = 16;  // the shared block
constexpr int NX = 8;   // its leading part: T_cl's tangent (6), b, kappa
constexpr int NK = 8;   // its trailing part: the intrinsics

// offsets into an evaluation record E[EVAL_DOUBLES] of one image (aw::ArrowRecord<16> and the two cost parts)
using Rec = aw::ArrowRecord<NF>;
constexpr int E_A = Rec::E_A, E_B = Rec::E_B, E_G = Rec::E_G, E_C = Rec::E_C, E_GC = Rec::E_GC, E_COST_CORNER = Rec::E_COST,
              E_COST_LASER = E_COST_CORNER + 1, EVAL_DOUBLES = E_COST_LASER + 1;
static_assert(E_B == 21 && E_G == 117 && E_C == 123 && E_GC == 259 && EVAL_DOUBLES == 277, "the record of K23");
static_assert(EVAL_DOUBLES - E_C <= FULL_THREADS && Rec::SS <= FULL_THREADS, "one total per lane");

using FullImage = aw::ArrowImage<NF, EVAL_DOUBLES>;

struct FullShared : aw::ArrowShared<NF, EVAL_DOUBLES> {
  double xc[7], xce[7];                // T_cl accepted / to evaluate
  double rg[2], rge[2];                // b, kappa
  double kc[NK], kce[NK];              // the intrinsics
  double Af[NF * NF], rf[NF], yf[NF];  // the reduced system of the free parameters, compact
  long long n_laser;
  int32_t model, n_free, hold_pose, pad_;
  int32_t free_idx[NF], is_free[NF];
};

struct FullArgs {
  clc_options opt;
  double sigma_px, sigma_laser;
  double loss_corner, loss_laser;  // Cauchy scales in units of sigma; 0: no loss
  uint32_t hold_intrinsics_mask;
  int32_t hold_range_mask, hold_board_poses, hold_extrinsic;
  int32_t use_corners, pad_;       // 0: the board poses and all 8 intrinsics are held, the corner terms are left out
  const float* corners;            // pixels, indexed by the absolute corner offsets; not read without use_corners
  const float* board;
  const long long* coff;           // [image] absolute; not read without use_corners
  const double* pts;               // indexed by the absolute point offsets
  const long long* poff;           // [image] absolute
  const unsigned char* keep;       // nullable
  const long long* prob_off;       // nullable: one problem over every image
  long long n_images;              // images from prob_off[0] (0 without it) on
  double *q, *t, *poses_cl, *range;
  clc_camera* cams;
  clc_summary* summaries;
  double *H_full, *cost_parts, *rms;  // nullable
  int32_t* status;
  double *w_corner, *w_laser;      // nullable; indexed by the absolute corner / point offsets
  FullImage* ws;                   // [n_images], the call's first image first
};

// rho_a and rho_a' at z, with a2 = a^2 and inv_a2 = 1 / a^2 (K22's definitions).
CLC_HD double cauchy_weight(double z, double inv_a2) { return 1.0 / (1.0 + z * inv_a2); }
CLC_HD double cauchy_rho(double z, double a2, double inv_a2) { return a2 * log1p(z * inv_a2); }

// |p|, and a point the model takes: finite with a range that is finite and > 0 (K21's rule).
CLC_HD double point_range(const double* p) {
  CLC_BF_NO_CONTRACT
  return sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
}
CLC_HD bool point_usable(const double* p) {
  const double rho = point_range(p);
  return finite_d(p[0]) && finite_d(p[1]) && finite_d(p[2]) && finite_d(rho) && rho > 0.0;
}

// The laser residual of the measured point p and its Jacobians (K21's range_point): p' = (1 + kappa + b / |p|) p,
// r = e3^T R^T (R_cl p' + t_cl - t) / sigma; Ji over [dt_i, dtheta_i], Jc over [dt_cl, dtheta_cl, b, kappa].
CLC_HD void range_point(const double* R, const double* t, const double* Rcl, const double* tcl, double b, double kappa, const double* p,
                        double inv_s, double* Ji, double* Jc, double* r) {
  CLC_BF_NO_CONTRACT
  const double rho = point_range(p), inv = 1.0 / rho;
  const double s = (1.0 + kappa) + b / rho;
  double pc[3], uh[3], d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    uh[i] = p[i] * inv;
    pc[i] = s * p[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = (((Rcl[3 * i] * pc[0] + Rcl[3 * i + 1] * pc[1]) + Rcl[3 * i + 2] * pc[2]) + tcl[i]) - t[i];
  const double m0 = (R[0] * d[0] + R[3] * d[1]) + R[6] * d[2];
  const double m1 = (R[1] * d[0] + R[4] * d[1]) + R[7] * d[2];
  const double m2 = (R[2] * d[0] + R[5] * d[1]) + R[8] * d[2];
  const double n0 = R[2], n1 = R[5], n2 = R[8];
  *r = m2 * inv_s;
  Ji[0] = -n0 * inv_s; Ji[1] = -n1 * inv_s; Ji[2] = -n2 * inv_s;
  Ji[3] = -m1 * inv_s; Ji[4] = m0 * inv_s; Ji[5] = 0.0;
  // u = R_cl^T n; d r / d theta_cl = (p' x u) / sigma
  const double u0 = (Rcl[0] * n0 + Rcl[3] * n1) + Rcl[6] * n2;
  const double u1 = (Rcl[1] * n0 + Rcl[4] * n1) + Rcl[7] * n2;
  const double u2 = (Rcl[2] * n0 + Rcl[5] * n1) + Rcl[8] * n2;
  Jc[0] = n0 * inv_s; Jc[1] = n1 * inv_s; Jc[2] = n2 * inv_s;
  Jc[3] = (pc[1] * u2 - pc[2] * u1) * inv_s;
  Jc[4] = (pc[2] * u0 - pc[0] * u2) * inv_s;
  Jc[5] = (pc[0] * u1 - pc[1] * u0) * inv_s;
  Jc[6] = ((u0 * uh[0] + u1 * uh[1]) + u2 * uh[2]) * inv_s;
  Jc[7] = ((u0 * p[0] + u1 * p[1]) + u2 * p[2]) * inv_s;
}

// What an evaluation sees of the shared block at its candidate.
struct FullCtx {
  clc_camera cam;
  double Rcl[9], tcl[3], b, kappa;
};

// The loss scales of a call, prepared once per evaluation.
struct Loss {
  bool corner, laser;
  double ac2, inv_ac2, al2, inv_al2;
};
CLC_HD Loss loss_of(const FullArgs& a) {
  Loss l;
  l.corner = a.loss_corner != 0.0;
  l.laser = a.loss_laser != 0.0;
  l.ac2 = a.loss_corner * a.loss_corner;
  l.al2 = a.loss_laser * a.loss_laser;
  l.inv_ac2 = l.corner ? 1.0 / l.ac2 : 0.0;
  l.inv_al2 = l.laser ? 1.0 / l.al2 : 0.0;
  return l;
}

// One image's evaluation record at pose7 / ctx: every lane of the image's wave calls it (host: once); the lead lane stores.
CLC_HD void eval_image(const FullArgs& a, const FullCtx& c, long long img, const double* pose7, double* E) {
  CLC_BF_NO_CONTRACT
  double xe[7], R[9];
#pragma unroll
  for (int i = 0; i < 7; ++i) xe[i] = pose7[i];
  quat_to_rot(xe + 3, R);
  const Loss ls = loss_of(a);
  // the cross block of C: the laser rows carry no intrinsics, the corner rows nothing of [T_cl, b, kappa]
  if (bf::lead_lane())
    CLC_AW_ROLLED for (int p = 0; p < NX; ++p)
      CLC_AW_ROLLED for (int q = NX; q < NF; ++q) E[E_C + tri<NF>(p, q)] = 0.0;
  if (a.use_corners) {  // (uniform over the call)
    const long long cb = a.coff[img], n = a.coff[img + 1] - cb;
    const float* __restrict__ px = a.corners + 2 * cb;
    const float* __restrict__ board = a.board + 2 * cb;
    const double inv_s = 1.0 / a.sigma_px;
    {  // w J J^T, w J r, sum rho
      double s[28];
      cp::wave_sum<28>([&](int lane, double* acc) {
        for (long long k = lane; k < n; k += cp::POSE_LANES) {
          double r[2], J[12], JK[16], wJ[12];
          const bool front = cc::corner_terms(c.cam, R, xe, board[2 * k], board[2 * k + 1], px[2 * k], px[2 * k + 1], inv_s, r, J, JK);
          const double z = r[0] * r[0] + r[1] * r[1];
          const double w = ls.corner ? cauchy_weight(z, ls.inv_ac2) : 1.0;
#pragma unroll
          for (int p = 0; p < 12; ++p) wJ[p] = w * J[p];
          int idx = 0;
#pragma unroll
          for (int p = 0; p < 6; ++p)
#pragma unroll
            for (int q = p; q < 6; ++q) {
              acc[idx] = fma(wJ[p], J[q], acc[idx]);
              acc[idx] = fma(wJ[6 + p], J[6 + q], acc[idx]);
              ++idx;
            }
#pragma unroll
          for (int p = 0; p < 6; ++p) {
            acc[21 + p] = fma(wJ[p], r[0], acc[21 + p]);
            acc[21 + p] = fma(wJ[6 + p], r[1], acc[21 + p]);
          }
          if (ls.corner) {
            acc[27] += cauchy_rho(z, ls.ac2, ls.inv_ac2);
          } else {
            acc[27] = fma(r[0], r[0], acc[27]);
            acc[27] = fma(r[1], r[1], acc[27]);
          }
          if (!front) acc[27] += __builtin_inf();  // an invalid evaluation, as K19's
        }
      }, s);
      if (bf::lead_lane()) {
#pragma unroll
        for (int i = 0; i < 21; ++i) E[E_A + i] = s[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) E[E_G + i] = s[21 + i];
        E[E_COST_CORNER] = 0.5 * s[27];
      }
    }
    {  // w J JK^T[:, 0:4], w JK r
      double s[32];
      cp::wave_sum<32>([&](int lane, double* acc) {
        for (long long k = lane; k < n; k += cp::POSE_LANES) {
          double r[2], J[12], JK[16];
          cc::corner_terms(c.cam, R, xe, board[2 * k], board[2 * k + 1], px[2 * k], px[2 * k + 1], inv_s, r, J, JK);
          const double w = ls.corner ? cauchy_weight(r[0] * r[0] + r[1] * r[1], ls.inv_ac2) : 1.0;
#pragma unroll
          for (int p = 0; p < 6; ++p) {
            const double w0 = w * J[p], w1 = w * J[6 + p];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              acc[4 * p + q] = fma(w0, JK[q], acc[4 * p + q]);
              acc[4 * p + q] = fma(w1, JK[8 + q], acc[4 * p + q]);
            }
          }
          const double wr0 = w * r[0], wr1 = w * r[1];
#pragma unroll
          for (int q = 0; q < NK; ++q) {
            acc[24 + q] = fma(JK[q], wr0, acc[24 + q]);
            acc[24 + q] = fma(JK[8 + q], wr1, acc[24 + q]);
          }
        }
      }, s);
      if (bf::lead_lane()) {
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) E[E_B + NF * p + NX + q] = s[4 * p + q];
#pragma unroll
        for (int q = 0; q < NK; ++q) E[E_GC + NX + q] = s[24 + q];
      }
    }
    {  // w J JK^T[:, 4:8]
      double s[24];
      cp::wave_sum<24>([&](int lane, double* acc) {
        for (long long k = lane; k < n; k += cp::POSE_LANES) {
          double r[2], J[12], JK[16];
          cc::corner_terms(c.cam, R, xe, board[2 * k], board[2 * k + 1], px[2 * k], px[2 * k + 1], inv_s, r, J, JK);
          const double w = ls.corner ? cauchy_weight(r[0] * r[0] + r[1] * r[1], ls.inv_ac2) : 1.0;
#pragma unroll
          for (int p = 0; p < 6; ++p) {
            const double w0 = w * J[p], w1 = w * J[6 + p];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              acc[4 * p + q] = fma(w0, JK[4 + q], acc[4 * p + q]);
              acc[4 * p + q] = fma(w1, JK[12 + q], acc[4 * p + q]);
            }
          }
        }
      }, s);
      if (bf::lead_lane()) {
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) E[E_B + NF * p + NX + 4 + q] = s[4 * p + q];
      }
    }
    {  // w JK JK^T: the intrinsics' block of C
      double s[36];
      cp::wave_sum<36>([&](int lane, double* acc) {
        for (long long k = lane; k < n; k += cp::POSE_LANES) {
          double r[2], J[12], JK[16];
          cc::corner_terms(c.cam, R, xe, board[2 * k], board[2 * k + 1], px[2 * k], px[2 * k + 1], inv_s, r, J, JK);
          const double w = ls.corner ? cauchy_weight(r[0] * r[0] + r[1] * r[1], ls.inv_ac2) : 1.0;
          int idx = 0;
#pragma unroll
          for (int p = 0; p < NK; ++p) {
            const double w0 = w * JK[p], w1 = w * JK[8 + p];
#pragma unroll
            for (int q = p; q < NK; ++q) {
              acc[idx] = fma(w0, JK[q], acc[idx]);
              acc[idx] = fma(w1, JK[8 + q], acc[idx]);
              ++idx;
            }
          }
        }
      }, s);
      if (bf::lead_lane()) {
        int idx = 0;
#pragma unroll
        for (int p = 0; p < NK; ++p)
#pragma unroll
          for (int q = p; q < NK; ++q) E[E_C + tri<NF>(NX + p, NX + q)] = s[idx++];
      }
    }
  } else if (bf::lead_lane()) {
    CLC_AW_ROLLED for (int i = 0; i < 21; ++i) E[E_A + i] = 0.0;
    CLC_AW_ROLLED for (int i = 0; i < 6; ++i) E[E_G + i] = 0.0;
    CLC_AW_ROLLED for (int p = 0; p < 6; ++p)
      CLC_AW_ROLLED for (int q = NX; q < NF; ++q) E[E_B + NF * p + q] = 0.0;
    CLC_AW_ROLLED for (int p = NX; p < NF; ++p) {
      CLC_AW_ROLLED for (int q = p; q < NF; ++q) E[E_C + tri<NF>(p, q)] = 0.0;
      E[E_GC + p] = 0.0;
    }
    E[E_COST_CORNER] = 0.0;
  }
  const double inv_s = 1.0 / a.sigma_laser;
  const long long pb = a.poff[img], np = a.poff[img + 1] - pb;
  const double* __restrict__ pts = a.pts + 3 * pb;
  if (np <= 0) {  // (wave-uniform)
    if (bf::lead_lane()) {
      CLC_AW_ROLLED for (int p = 0; p < 6; ++p)
        CLC_AW_ROLLED for (int q = 0; q < NX; ++q) E[E_B + NF * p + q] = 0.0;
      CLC_AW_ROLLED for (int p = 0; p < NX; ++p) {
        CLC_AW_ROLLED for (int q = p; q < NX; ++q) E[E_C + tri<NF>(p, q)] = 0.0;
        E[E_GC + p] = 0.0;
      }
      E[E_COST_LASER] = 0.0;
    }
    return;
  }
  // The laser passes, K21's split so that no pass holds more than 36 sums; each recomputes r and w = rho'(r^2).
  {  // w J_i J_i^T, w J_i r, sum rho
    double s[28];
    cp::wave_sum<28>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[NX], wJ[6], r;
        range_point(R, xe, c.Rcl, c.tcl, c.b, c.kappa, pts + 3 * k, inv_s, Ji, Jc, &r);
        const double w = ls.laser ? cauchy_weight(r * r, ls.inv_al2) : 1.0;
#pragma unroll
        for (int p = 0; p < 6; ++p) wJ[p] = w * Ji[p];
        int idx = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = p; q < 6; ++q) { acc[idx] = fma(wJ[p], Ji[q], acc[idx]); ++idx; }
#pragma unroll
        for (int p = 0; p < 6; ++p) acc[21 + p] = fma(wJ[p], r, acc[21 + p]);
        acc[27] = ls.laser ? acc[27] + cauchy_rho(r * r, ls.al2, ls.inv_al2) : fma(r, r, acc[27]);
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 21; ++i) E[E_A + i] += s[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) E[E_G + i] += s[21 + i];
      E[E_COST_LASER] = 0.5 * s[27];
    }
  }
  {  // w J_i J_c^T over T_cl's six columns
    double s[36];
    cp::wave_sum<36>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[NX], r;
        range_point(R, xe, c.Rcl, c.tcl, c.b, c.kappa, pts + 3 * k, inv_s, Ji, Jc, &r);
        const double w = ls.laser ? cauchy_weight(r * r, ls.inv_al2) : 1.0;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
          const double wj = w * Ji[p];
#pragma unroll
          for (int q = 0; q < 6; ++q) acc[6 * p + q] = fma(wj, Jc[q], acc[6 * p + q]);
        }
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = 0; q < 6; ++q) E[E_B + NF * p + q] = s[6 * p + q];
    }
  }
  {  // w J_i J_c^T over b, kappa; w J_c r
    double s[20];
    cp::wave_sum<20>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[NX], r;
        range_point(R, xe, c.Rcl, c.tcl, c.b, c.kappa, pts + 3 * k, inv_s, Ji, Jc, &r);
        const double w = ls.laser ? cauchy_weight(r * r, ls.inv_al2) : 1.0;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
          const double wj = w * Ji[p];
          acc[2 * p] = fma(wj, Jc[6], acc[2 * p]);
          acc[2 * p + 1] = fma(wj, Jc[7], acc[2 * p + 1]);
        }
        const double wr = w * r;
#pragma unroll
        for (int q = 0; q < NX; ++q) acc[12 + q] = fma(Jc[q], wr, acc[12 + q]);
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        E[E_B + NF * p + 6] = s[2 * p];
        E[E_B + NF * p + 7] = s[2 * p + 1];
      }
#pragma unroll
      for (int q = 0; q < NX; ++q) E[E_GC + q] = s[12 + q];
    }
  }
  {  // w J_c J_c^T: the [T_cl, b, kappa] block of C
    double s[36];
    cp::wave_sum<36>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[NX], r;
        range_point(R, xe, c.Rcl, c.tcl, c.b, c.kappa, pts + 3 * k, inv_s, Ji, Jc, &r);
        const double w = ls.laser ? cauchy_weight(r * r, ls.inv_al2) : 1.0;
        int idx = 0;
#pragma unroll
        for (int p = 0; p < NX; ++p) {
          const double wj = w * Jc[p];
#pragma unroll
          for (int q = p; q < NX; ++q) { acc[idx] = fma(wj, Jc[q], acc[idx]); ++idx; }
        }
      }
    }, s);
    if (bf::lead_lane()) {
      int idx = 0;
#pragma unroll
      for (int p = 0; p < NX; ++p)
#pragma unroll
        for (int q = p; q < NX; ++q) E[E_C + tri<NF>(p, q)] = s[idx++];
    }
  }
}

// Why an image takes no part (wave-uniform; every lane of the image's wave calls it): K19's rule for the corners (where they take
// part), K21's for the points.
CLC_HD int image_status(const FullArgs& a, long long img) {
  if (a.keep && !a.keep[img]) return CLC_JOINT_NOT_KEPT;
  const long long pb = a.poff[img], np = a.poff[img + 1] - pb;
  long long n = 0;
  const float *px = nullptr, *board = nullptr;
  if (a.use_corners) {
    const long long cb = a.coff[img];
    n = a.coff[img + 1] - cb;
    if (n < 4) return CLC_JOINT_TOO_FEW;
    if (cb < 0) return CLC_JOINT_NONFINITE;
    px = a.corners + 2 * cb;
    board = a.board + 2 * cb;
  }
  if (np < 0 || pb < 0) return CLC_JOINT_NONFINITE;
  const double* pts = a.pts + 3 * pb;
  double bad[1];
  cp::wave_sum<1>([&](int lane, double* acc) {
    for (long long k = lane; k < n; k += cp::POSE_LANES)
      if (!(isfinite(px[2 * k]) && isfinite(px[2 * k + 1]) && isfinite(board[2 * k]) && isfinite(board[2 * k + 1]))) acc[0] += 1.0;
    for (long long k = lane; k < np; k += cp::POSE_LANES)
      if (!point_usable(pts + 3 * k)) acc[0] += 1.0;
    if (lane < 4 && !finite_d(a.q[4 * img + lane])) acc[0] += 1.0;
    if (lane < 3 && !finite_d(a.t[3 * img + lane])) acc[0] += 1.0;
  }, bad);
  if (bad[0] != 0.0) return CLC_JOINT_NONFINITE;
  const double w = a.q[4 * img], x = a.q[4 * img + 1], y = a.q[4 * img + 2], z = a.q[4 * img + 3];
  if (!((w * w + x * x) + (y * y + z * z) > 0.0)) return CLC_JOINT_NONFINITE;
  return CLC_JOINT_OK;
}

// Solve A y = b for the symmetric positive definite n x n A (row-major, n at run time): chol_solve of clc_math.hpp, rolled.
// L (n * n), z (n) scratch; false if a pivot is not positive.
CLC_HD bool chol_solve_n(int n, const double* A, const double* b, double* y, double* L, double* z) {
  CLC_AW_ROLLED for (int j = 0; j < n; ++j) {
    double d = A[n * j + j];
    CLC_AW_ROLLED for (int k = 0; k < j; ++k) d -= L[n * j + k] * L[n * j + k];
    if (!(d > 0.0)) return false;
    const double inv = rsqrt_pos(d);
    L[n * j + j] = inv;
    CLC_AW_ROLLED for (int i = j + 1; i < n; ++i) {
      double s = A[n * i + j];
      CLC_AW_ROLLED for (int k = 0; k < j; ++k) s -= L[n * i + k] * L[n * j + k];
      L[n * i + j] = s * inv;
    }
  }
  CLC_AW_ROLLED for (int i = 0; i < n; ++i) {
    double s = b[i];
    CLC_AW_ROLLED for (int k = 0; k < i; ++k) s -= L[n * i + k] * z[k];
    z[i] = s * L[n * i + i];
  }
  CLC_AW_ROLLED for (int i = n - 1; i >= 0; --i) {
    double s = z[i];
    CLC_AW_ROLLED for (int k = i + 1; k < n; ++k) s -= L[n * k + i] * y[k];
    y[i] = s * L[n * i + i];
  }
  return true;
}

// [first image, images) of problem pb and its first image's place in the workspace, clamped to the call's images: n_images from
// prob_off[0] on (K19's convention: nothing is read back to size the workspace).
CLC_HD void problem_range(const FullArgs& a, long long pb, long long* i0, long long* P, long long* w0) {
  const long long first = a.prob_off ? a.prob_off[0] : 0;
  long long b = a.prob_off ? a.prob_off[pb] : 0, e = a.prob_off ? a.prob_off[pb + 1] : a.n_images;
  if (b < first) b = first;
  if (e > first + a.n_images) e = first + a.n_images;
  *i0 = b;
  *P = e > b ? e - b : 0;
  *w0 = b - first;
}

// What K23 gives the arrow solve (clc_arrow.hpp): the 16-wide shared block.
struct FullTraits {
  static constexpr int NC = NF, EVAL_DOUBLES = fc::EVAL_DOUBLES;
  using Args = FullArgs;
  using Image = FullImage;
  using Shared = FullShared;
  using Ctx = FullCtx;

  static CLC_HD aw::Problem<Image> problem(const Args& a, long long pb) {
    long long i0, P, w0;
    problem_range(a, pb, &i0, &P, &w0);
    return {i0, P, a.ws + w0};
  }
  static CLC_HD int image_status(const Args& a, long long img) { return fc::image_status(a, img); }
  static CLC_HD long long observations(const Args& a, long long img) { return a.poff[img + 1] - a.poff[img]; }
  static CLC_HD void context(const Shared& sh, Ctx& c) {
    double q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = sh.xce[3 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) c.tcl[i] = sh.xce[i];
    quat_to_rot(q, c.Rcl);
    c.b = sh.rge[0];
    c.kappa = sh.rge[1];
    c.cam.model = sh.model;
    c.cam.reserved = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { c.cam.proj[i] = sh.kce[i]; c.cam.dist[i] = sh.kce[4 + i]; }
  }
  static CLC_HD void eval_image(const Args& a, const Ctx& c, long long img, const double* pose7, double* E) {
    fc::eval_image(a, c, img, pose7, E);
  }
  // held over the whole call: T_cl by hold_extrinsic, b and kappa and the intrinsics bit by bit
  static CLC_HD bool held(const Args& a, int p) {
    if (p < 6) return a.hold_extrinsic != 0;
    if (p < NX) return ((a.hold_range_mask >> (p - 6)) & 1) != 0;
    return ((a.hold_intrinsics_mask >> (p - NX)) & 1u) != 0;
  }
  static CLC_HD bool init_block(const Args& a, long long pb, long long n_laser, Shared& sh, double& xn) {
    const clc_camera& cam = a.cams[pb];
    bool ok = cam.model == CLC_CAMERA_PINHOLE || cam.model == CLC_CAMERA_KANNALA_BRANDT;
    CLC_AW_ROLLED for (int i = 0; i < 7; ++i) {
      const double v = a.poses_cl[7 * pb + i];
      sh.xc[i] = sh.xce[i] = v;
      ok = ok && finite_d(v);
    }
    CLC_AW_ROLLED for (int i = 0; i < 2; ++i) {
      const double v = a.range[2 * pb + i];
      sh.rg[i] = sh.rge[i] = v;
      ok = ok && finite_d(v);
    }
    CLC_AW_ROLLED for (int i = 0; i < 4; ++i) {
      sh.kc[i] = sh.kce[i] = cam.proj[i];
      sh.kc[4 + i] = sh.kce[4 + i] = cam.dist[i];
      ok = ok && finite_d(cam.proj[i]) && finite_d(cam.dist[i]);
    }
    sh.model = cam.model;
    // without a laser point nothing constrains T_cl, b, kappa: the problem holds them by itself
    int nf = 0;
    CLC_AW_ROLLED for (int i = 0; i < NF; ++i) {
      sh.free_idx[i] = 0;
      const bool fr = !held(a, i) && !(i < NX && n_laser == 0);
      sh.is_free[i] = fr ? 1 : 0;
      if (fr) sh.free_idx[nf++] = i;
    }
    sh.n_free = nf;
    sh.hold_pose = (a.hold_extrinsic || n_laser == 0) ? 1 : 0;
    sh.n_laser = n_laser;
    sh.move_c = nf > 0 ? 1 : 0;
    if (sh.move_c) {
      CLC_AW_ROLLED for (int i = 0; i < 7; ++i) xn += sh.xc[i] * sh.xc[i];
      CLC_AW_ROLLED for (int i = 0; i < 2; ++i) xn += sh.rg[i] * sh.rg[i];
      CLC_AW_ROLLED for (int i = 0; i < NK; ++i) xn += sh.kc[i] * sh.kc[i];
    }
    return ok;
  }
  static CLC_HD double cost(const double* tot) { return tot[E_COST_CORNER - E_C] + tot[E_COST_LASER - E_C]; }
  static CLC_HD double block_gradient(const Shared& sh, double m) {
    if (!sh.move_c) return m;
    if (!sh.hold_pose) m = fmax(m, aw::block_gradient_norm(sh.xc, sh.tot[sh.cur] + (E_GC - E_C)));
    CLC_AW_ROLLED for (int f = 0; f < sh.n_free; ++f)
      if (sh.free_idx[f] >= 6) m = fmax(m, fabs(sh.tot[sh.cur][(E_GC - E_C) + sh.free_idx[f]]));
    return m;
  }
  // held parameters lose their rows and columns: the Cholesky runs at the number of free ones
  static CLC_HD bool solve_block(Shared& sh) {
    const int n = sh.n_free;
    CLC_AW_ROLLED for (int p = 0; p < n; ++p) {
      CLC_AW_ROLLED for (int q = 0; q < n; ++q) sh.Af[n * p + q] = sh.A[NF * sh.free_idx[p] + sh.free_idx[q]];
      sh.rf[p] = sh.rhs[sh.free_idx[p]];
    }
    bool ok = chol_solve_n(n, sh.Af, sh.rf, sh.yf, sh.L, sh.z);
    CLC_AW_ROLLED for (int f = 0; f < n; ++f) {
      sh.step_c[sh.free_idx[f]] = -sh.yf[f];
      if (!finite_d(sh.yf[f])) ok = false;
    }
    return ok;
  }
  static CLC_HD void block_candidate(Shared& sh, double& sn, double& xn) {
    double n2 = 0.0;
    if (!sh.hold_pose) {
      sn += aw::block_candidate(sh.xc, sh.step_c, sh.scale_c, sh.xce, &n2);
    } else {  // a held T_cl keeps its bits
      CLC_AW_ROLLED for (int i = 0; i < 7; ++i) {
        sh.xce[i] = sh.xc[i];
        n2 += sh.xc[i] * sh.xc[i];
      }
    }
    xn += n2;
    CLC_AW_ROLLED for (int p = 6; p < NF; ++p) {
      // a held parameter keeps its bits
      const double x0 = p < NX ? sh.rg[p - 6] : sh.kc[p - NX];
      const double v = sh.is_free[p] ? x0 + sh.step_c[p] * sh.scale_c[p] : x0;
      if (p < NX) sh.rge[p - 6] = v; else sh.kce[p - NX] = v;
      sn += (x0 - v) * (x0 - v);
      xn += v * v;
    }
  }
  static CLC_HD void accept_block(Shared& sh) {
    CLC_AW_ROLLED for (int i = 0; i < 7; ++i) sh.xc[i] = sh.xce[i];
    CLC_AW_ROLLED for (int i = 0; i < 2; ++i) sh.rg[i] = sh.rge[i];
    CLC_AW_ROLLED for (int i = 0; i < NK; ++i) sh.kc[i] = sh.kce[i];
  }
  static CLC_HD double* information(const Args& a) { return a.H_full; }
  static CLC_HD void write_outputs(const Args& a, long long pb, const Shared& sh, bool failed) {
    if (!failed && sh.move_c) {
      if (!sh.hold_pose) CLC_AW_ROLLED for (int i = 0; i < 7; ++i) a.poses_cl[7 * pb + i] = sh.xc[i];
      CLC_AW_ROLLED for (int i = 0; i < 2; ++i)
        if (sh.is_free[6 + i]) a.range[2 * pb + i] = sh.rg[i];
      CLC_AW_ROLLED for (int i = 0; i < NK; ++i)
        if (sh.is_free[NX + i]) {
          if (i < 4) a.cams[pb].proj[i] = sh.kc[i]; else a.cams[pb].dist[i - 4] = sh.kc[i];
        }
    }
    const bool have = sh.n_evals > 0 && !failed;
    if (a.cost_parts) {
      a.cost_parts[2 * pb] = have ? sh.tot[sh.cur][E_COST_CORNER - E_C] : __builtin_nan("");
      a.cost_parts[2 * pb + 1] = have ? sh.tot[sh.cur][E_COST_LASER - E_C] : __builtin_nan("");
    }
    if (a.rms) {
      // sigma_px sqrt(2 cost_corner / corners) over the participating images: K19's RMS where the corners carry no loss
      long long n_corners = 0;
      if (a.use_corners) {
        const aw::Problem<Image> pr = problem(a, pb);
        for (long long j = 0; j < pr.P; ++j)
          if (pr.ws[j].st == aw::IMAGE_OK) n_corners += a.coff[pr.i0 + j + 1] - a.coff[pr.i0 + j];
      }
      a.rms[pb] = (have && n_corners > 0) ? a.sigma_px * sqrt(2.0 * sh.tot[sh.cur][E_COST_CORNER - E_C] / (double)n_corners) : __builtin_nan("");
    }
  }
};

// One problem: every thread of its workgroup calls it (host: once).
CLC_HD void full_problem(const FullArgs& a, long long pb, FullShared& sh) { aw::arrow_problem<FullTraits>(a, pb, sh); }

// f(lane) on the 64 lanes of a wave (host: a loop).
template <class F>
CLC_HD void each_wave_lane(F f) {
#if defined(__HIP_DEVICE_COMPILE__)
  f((int)(threadIdx.x & 63));
#else
  for (int l = 0; l < cp::POSE_LANES; ++l) f(l);
#endif
}

// The weights of one image at the returned point, after the solve: every lane of the image's wave calls it (host: once).  `failed`:
// the image's problem ended CLC_FAILURE.  An image that takes no part gets NaN over the ranges its offsets name (K22's convention);
// without use_corners no corner weight is written.
CLC_HD void weights_image(const FullArgs& a, long long img, bool failed, const clc_camera& cam, const double* pose_cl, double b, double kappa) {
  CLC_BF_NO_CONTRACT
  const long long pb = a.poff[img], np = a.poff[img + 1] - pb;
  long long cb = 0, n = 0;
  if (a.use_corners) {
    cb = a.coff[img];
    n = a.coff[img + 1] - cb;
  }
  const bool corners_in = a.use_corners && cb >= 0 && n >= 0, points_in = pb >= 0 && np >= 0;
  const bool part = a.status[img] == CLC_JOINT_OK && !failed;
  if (!part) {
    each_wave_lane([&](int lane) {
      if (a.w_corner && corners_in)
        for (long long k = lane; k < n; k += cp::POSE_LANES) a.w_corner[cb + k] = __builtin_nan("");
      if (a.w_laser && points_in)
        for (long long k = lane; k < np; k += cp::POSE_LANES) a.w_laser[pb + k] = __builtin_nan("");
    });
    return;
  }
  // the pose as the solve reads it: [t, q(xyzw)] normalised
  const double qw = a.q[4 * img], qx = a.q[4 * img + 1], qy = a.q[4 * img + 2], qz = a.q[4 * img + 3];
  const double inv = 1.0 / sqrt((qw * qw + qx * qx) + (qy * qy + qz * qz));
  const double xe[7] = {a.t[3 * img], a.t[3 * img + 1], a.t[3 * img + 2], qx * inv, qy * inv, qz * inv, qw * inv};
  double R[9], Rcl[9], qcl[4];
  quat_to_rot(xe + 3, R);
#pragma unroll
  for (int i = 0; i < 4; ++i) qcl[i] = pose_cl[3 + i];
  quat_to_rot(qcl, Rcl);
  const Loss ls = loss_of(a);
  const double inv_px = 1.0 / a.sigma_px, inv_s = 1.0 / a.sigma_laser;
  const float* __restrict__ px = a.use_corners ? a.corners + 2 * cb : nullptr;
  const float* __restrict__ board = a.use_corners ? a.board + 2 * cb : nullptr;
  const double* __restrict__ pts = a.pts + 3 * pb;
  each_wave_lane([&](int lane) {
    if (a.w_corner)
      for (long long k = lane; k < n; k += cp::POSE_LANES) {
        double w = 1.0;
        if (ls.corner) {
          double r[2], J[12], JK[16];
          cc::corner_terms(cam, R, xe, board[2 * k], board[2 * k + 1], px[2 * k], px[2 * k + 1], inv_px, r, J, JK);
          w = cauchy_weight(r[0] * r[0] + r[1] * r[1], ls.inv_ac2);
        }
        a.w_corner[cb + k] = w;
      }
    if (a.w_laser)
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double w = 1.0;
        if (ls.laser) {
          double Ji[6], Jc[NX], r;
          range_point(R, xe, Rcl, pose_cl, b, kappa, pts + 3 * k, inv_s, Ji, Jc, &r);
          w = cauchy_weight(r * r, ls.inv_al2);
        }
        a.w_laser[pb + k] = w;
      }
  });
}

// The weights of one problem: the waves take its images round-robin (host: a loop).
CLC_HD void weights_problem(const FullArgs& a, long long pb) {
  long long i0, P, w0;
  problem_range(a, pb, &i0, &P, &w0);
  const bool failed = a.summaries[pb].termination == CLC_FAILURE;
  const clc_camera cam = a.cams[pb];
  double pose_cl[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) pose_cl[i] = a.poses_cl[7 * pb + i];
  const double b = a.range[2 * pb], kappa = a.range[2 * pb + 1];
  aw::each_image_wave(P, [&](long long j) { weights_image(a, i0 + j, failed, cam, pose_cl, b, kappa); });
}

#if defined(__HIPCC__)

// K23: one 256-thread workgroup per problem.
static __global__ __launch_bounds__(FULL_THREADS) void fullcal_kernel(const FullArgs a) {
  __shared__ FullShared sh;
  full_problem(a, (long long)blockIdx.x, sh);
}

// The weights at the returned point: one workgroup per problem, one wave per image.  Runs after fullcal_kernel on its stream.
static __global__ __launch_bounds__(FULL_THREADS) void fullcal_weights_kernel(const FullArgs a) {
  weights_problem(a, (long long)blockIdx.x);
}

#endif  // __HIPCC__

}  // namespace fc
}  // namespace clc
