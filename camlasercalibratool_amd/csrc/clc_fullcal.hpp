// clc_fullcal.hpp — K23: one robust cost over the camera's intrinsics, every board pose, T_cl and the scanner's range offset and scale.
//
//   corner j of image i   e_j = (project(cam, R_i X_j + t_i) - u_j) / sigma_px                      K19's residual: pixels, no lift
//   laser point k         r_k = e3^T R_i^T (R_cl p'_k + t_cl - t_i) / sigma_laser,  p' = (1 + kappa + b / |p|) p            (K21)
//   cost = 1/2 sum rho_ac(|e_j|^2) + 1/2 sum rho_al(r_k^2)        rho_a(z) = a^2 log1p(z / a^2), rho_a'(z) = 1 / (1 + z / a^2); a = 0: z
//
// The loss is K22's: one loss on a corner's residual 2-vector, Ceres' corrector for rho'' <= 0 (rows and residual scaled by
// sqrt(rho')), so the Gauss-Newton blocks take w J^T J and w J^T r with w = rho'(z).  An arrow problem of clc_arrow.hpp, with
// a 16-wide shared block
//
//   [dt_cl(3), dtheta_cl(3), b, kappa, proj[0..3], dist[0..3]]       the leading 8 as K21's H_cr, the trailing 8 in clc_camera order
//
// T_cl moves on its tangent, b, kappa and the intrinsics additively.  The laser rows do not depend on the intrinsics and the corner
// rows not on T_cl, b, kappa: the [T_cl, range] x intrinsics block of C is exactly zero, it is written as zeros and never summed; the
// two groups couple only through the board poses in the Schur complement.  The laser row under the range correction, the point rules, the
// Cauchy loss and the skeleton of the weights are clc_jointterms.hpp's, the same that K21 and K22 take, and the corner rows
// clc_camcal.hpp's; this file holds K23's arguments, its evaluation with the eight passes written out, and what is its shared block's
// own.
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
#include "clc_jointterms.hpp"
#include "clc_camcal.hpp"

namespace clc {
namespace fc {

using namespace jtm;

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

// What an evaluation sees of the shared block at its candidate.
struct FullCtx {
  clc_camera cam;
  double Rcl[9], tcl[3], b, kappa;
};

// One image's evaluation record at pose7 / ctx: every lane of the image's wave calls it (host: once); the lead lane stores.  The
// eight passes are written out: grouped from the shared accumulate helpers fullcal_kernel computed the same sums in another
// instruction order and its batch measured 0.3 % slower (profiles/joint_terms_refactor.md).
CLC_HD void eval_image(const FullArgs& a, const FullCtx& c, long long img, const double* pose7, double* E) {
  CLC_BF_NO_CONTRACT
  double xe[7], R[9];
#pragma unroll
  for (int i = 0; i < 7; ++i) xe[i] = pose7[i];
  quat_to_rot(xe + 3, R);
  const Loss ls = loss_of(a.loss_corner, a.loss_laser);
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

// What the weights read of a call: the corners (where they take part) are pixels indexed by the absolute offsets, no end named.
CLC_HD ImageView view_of(const FullArgs& a) {
  return {a.corners, a.board, a.use_corners ? a.coff : nullptr, 0, 0, NO_CORNER_END, a.pts, a.poff, a.keep, a.q, a.t, a.status,
          a.w_corner, a.w_laser};
}

// Why an image takes no part (wave-uniform; every lane of the image's wave calls it): K19's rule for the corners (where they take
// part), K21's for the points.  The rule of jtm::image_status, written out: through jtm's view fullcal_kernel's batch measured
// 1.3 % slower (profiles/joint_terms_refactor.md).  A change to the rule has to be made in both places.
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

// What K23 gives the arrow solve (clc_arrow.hpp): the 16-wide shared block.
struct FullTraits {
  static constexpr int NC = NF, EVAL_DOUBLES = fc::EVAL_DOUBLES;
  using Args = FullArgs;
  using Image = FullImage;
  using Shared = FullShared;
  using Ctx = FullCtx;

  // the call's images: n_images from prob_off[0] on (K19's convention: nothing is read back to size the workspace)
  static CLC_HD aw::Problem<Image> problem(const Args& a, long long pb) {
    return aw::problem_range(a.prob_off, pb, a.prob_off ? a.prob_off[0] : 0, a.n_images, a.ws);
  }
  static CLC_HD int image_status(const Args& a, long long img) {
    return fc::image_status(a, img);
  }
  static CLC_HD long long observations(const Args& a, long long img) { return a.poff[img + 1] - a.poff[img]; }
  static CLC_HD void context(const Shared& sh, Ctx& c) {
    aw::tcl_context(sh, c);
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
    ok = aw::tcl_init(a.poses_cl + 7 * pb, sh) && ok;
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
    sh.n_free = aw::free_parameters<NF>(sh.free_idx, [&](int i) {  // (the predicate also records sh.is_free[i])
      const bool fr = !held(a, i) && !(i < NX && n_laser == 0);
      sh.is_free[i] = fr ? 1 : 0;
      return fr;
    });
    sh.hold_pose = (a.hold_extrinsic || n_laser == 0) ? 1 : 0;
    sh.n_laser = n_laser;
    sh.move_c = sh.n_free > 0 ? 1 : 0;
    if (sh.move_c) {
      CLC_AW_ROLLED for (int i = 0; i < 7; ++i) xn += sh.xc[i] * sh.xc[i];
      CLC_AW_ROLLED for (int i = 0; i < 2; ++i) xn += sh.rg[i] * sh.rg[i];
      CLC_AW_ROLLED for (int i = 0; i < NK; ++i) xn += sh.kc[i] * sh.kc[i];
    }
    return ok;
  }
  static CLC_HD double cost(const double* tot) { return aw::cost_of_parts<NF>(tot); }
  static CLC_HD double block_gradient(const Shared& sh, double m) {
    if (!sh.move_c) return m;
    if (!sh.hold_pose) m = aw::tcl_gradient<NF>(sh, m);
    return aw::free_gradient<NF>(sh, 6, m);
  }
  // held parameters lose their rows and columns: the rolled Cholesky runs at the number of free ones
  static CLC_HD bool solve_block(Shared& sh) {
    aw::compact_free<NF>(sh, sh.n_free);
    return aw::scatter_free(sh, aw::chol_solve_n(sh.n_free, sh.Af, sh.rf, sh.yf, sh.L, sh.z));
  }
  static CLC_HD void block_candidate(Shared& sh, double& sn, double& xn) {
    aw::tcl_candidate(sh, sh.hold_pose != 0, sn, xn);
    CLC_AW_ROLLED for (int p = 6; p < NF; ++p) {
      // a held parameter keeps its bits
      const double x0 = p < NX ? sh.rg[p - 6] : sh.kc[p - NX];
      const double v = aw::additive_candidate(x0, sh.is_free[p] ? x0 + sh.step_c[p] * sh.scale_c[p] : x0, sn, xn);
      if (p < NX) sh.rge[p - 6] = v; else sh.kce[p - NX] = v;
    }
  }
  static CLC_HD void accept_block(Shared& sh) {
    aw::tcl_accept(sh);
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
    aw::write_cost_parts<NF>(a.cost_parts, pb, sh, failed);
    if (a.rms) {
      // sigma_px sqrt(2 cost_corner / corners) over the participating images: K19's RMS where the corners carry no loss
      const bool have = sh.n_evals > 0 && !failed;
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

// The weights of one problem at the returned point: the waves take its images round-robin (host: a loop).  Without use_corners no
// corner weight is written.
CLC_HD void weights_problem(const FullArgs& a, long long pb) {
  CLC_BF_NO_CONTRACT
  const aw::Problem<FullImage> pr = FullTraits::problem(a, pb);
  const bool failed = a.summaries[pb].termination == CLC_FAILURE;
  const clc_camera cam = a.cams[pb];
  double pose_cl[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) pose_cl[i] = a.poses_cl[7 * pb + i];
  const double b = a.range[2 * pb], kappa = a.range[2 * pb + 1];
  const ImageView v = view_of(a);
  const Loss ls = loss_of(a.loss_corner, a.loss_laser);
  const double inv_px = 1.0 / a.sigma_px, inv_s = 1.0 / a.sigma_laser;
  aw::each_image_wave(pr.P, [&](long long j) {
    double Rcl[9];
    quat_to_rot(pose_cl + 3, Rcl);
    weights_image(v, ls, pr.i0 + j, failed,
                  [&](const double* R, const double* xe, const float* px, const float* board, long long k) {
                    double r[2], J[12], JK[16];
                    cc::corner_terms(cam, R, xe, board[2 * k], board[2 * k + 1], px[2 * k], px[2 * k + 1], inv_px, r, J, JK);
                    return cauchy_weight(r[0] * r[0] + r[1] * r[1], ls.inv_ac2);
                  },
                  [&](const double* R, const double* xe, const double* pts, long long k) {
                    double Ji[6], Jc[NX], r;
                    range_point(R, xe, Rcl, pose_cl, b, kappa, pts + 3 * k, inv_s, Ji, Jc, &r);
                    return cauchy_weight(r * r, ls.inv_al2);
                  });
  });
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
