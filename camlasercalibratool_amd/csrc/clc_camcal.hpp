// clc_camcal.hpp — K19: the camera's intrinsics from the board images.  One problem = one camera seen in P images of the board; the cost
//
//   1/2 sum |(project(cam, R_i X + t_i) - u) / sigma_px|^2          project: cam_project of clc_campose.hpp, pixels, no lift
//
// is minimised over the 8 intrinsics (clc_camera order: proj[0..3], dist[0..3]; moved additively) and the tangent [dt, dtheta] of every
// board pose.  The arrow of clc_arrow.hpp with the intrinsics as its 8-wide shared block: the solve (step, controller, outputs) is
// aw::arrow_problem; this file holds the cost, what is the intrinsics' own and the closed-form start.
//
//   camcal_kernel   one 256-thread workgroup (4 waves) per problem, the whole Levenberg-Marquardt solve in one launch.
//     evaluation   per image a wave all-reduces, in four passes over the corners (the cheap residual recomputed), {A_i, g_i, sum r^2}
//                  (28), {B_i[:, 0:4], g_c} (32), B_i[:, 4:8] (24) and the image's share of C (36): 120 sums, never more than 36 live.
//                  An evaluation with a corner at P_z <= 0 is invalid (a rejected candidate).
//     reduced 8x8  thread 0 compacts it to the free intrinsics and solves it with chol_solve<n_free>.  A held intrinsic has scale 0
//                  (Jacobi scaling matters here: focal lengths and k-coefficients differ by five orders of magnitude).
//   homography_kernel   one wave per image: the pixel-space homography of the image's corners about the image centre (K10's normalized
//                       DLT and jacobi_rows, the same degeneracy ratio), scaled to unit Frobenius norm: the closed-form focal start's
//                       per-image half (guess_focal is the host's half).
//   Per-image state: CalImage, 4.4 KB.
//
// Everything numeric is CLC_HD: tests/shim/camcal_shim.cpp compiles this header for the host with g++ and runs the same code with the
// threads as loops, in the same summation order.
#pragma once
#include "clc_arrow.hpp"

namespace clc {
namespace cc {

using aw::finite_d;

constexpr int CAL_THREADS = aw::ARROW_THREADS;
constexpr int NK = 8;  // intrinsics

// offsets into an evaluation record E[EVAL_DOUBLES] of one image (aw::ArrowRecord<8> and the cost)
constexpr int E_A = 0, E_B = 21, E_G = 69, E_C = 75, E_GC = 111, E_COST = 119, EVAL_DOUBLES = 120;
static_assert(E_G == aw::ArrowRecord<NK>::E_G && E_C == aw::ArrowRecord<NK>::E_C && E_GC == aw::ArrowRecord<NK>::E_GC &&
                  E_COST == aw::ArrowRecord<NK>::E_COST, "the record of K19 is the arrow's");

using CalImage = aw::ArrowImage<NK, EVAL_DOUBLES>;

struct CalShared : aw::ArrowShared<NK, EVAL_DOUBLES> {
  double kc[NK], kce[NK];         // intrinsics accepted / to evaluate
  double Af[64], rf[NK], yf[NK];  // the reduced system of the free intrinsics, compact
  long long n_corners;
  int32_t model, n_free;
  int32_t free_idx[NK];
};

struct CalArgs {
  clc_options opt;
  double sigma_px;
  uint32_t hold_mask;
  int32_t hold_board_poses;
  const float* corners;       // pixels, indexed by the absolute corner offsets
  const float* board;
  const long long* coff;      // [image] absolute
  const unsigned char* keep;  // nullable
  const long long* prob_off;  // nullable: one problem over every image
  long long n_images;         // images from prob_off[0] (0 without it) on
  double *q, *t;
  clc_camera* cams;
  clc_summary* summaries;
  double *H_cam, *rms;        // nullable
  int32_t* status;
  CalImage* ws;               // [n_images], the call's first image first
};

// ---- the projection's derivatives -----------------------------------------------------------------------------------------
// JP[3 i + j] = d px_i / d P_j, JK[8 i + q] = d px_i / d intrinsic q (proj[0..3], dist[0..3]) of cam_project at the camera-frame
// point P.  PINHOLE: radial-tangential distortion of x = P_x / P_z, y = P_y / P_z.  KANNALA_BRANDT: through theta = acos(P_z / |P|)
// and phi; on the optical axis (rho = 0) phi is undefined and the limit d px / d P_xy = f / P_z is taken.
CLC_HD void project_jacobian(const clc_camera& c, const double* P, double* JP, double* JK) {
  CLC_BF_NO_CONTRACT
  const double fx = c.proj[0], fy = c.proj[1];
  if (c.model == CLC_CAMERA_PINHOLE) {
    const double k1 = c.dist[0], k2 = c.dist[1], p1 = c.dist[2], p2 = c.dist[3];
    const double iz = 1.0 / P[2];
    const double x = P[0] * iz, y = P[1] * iz;
    const double x2 = x * x, y2 = y * y, xy = x * y, r2 = x2 + y2;
    const double rad = k1 * r2 + k2 * r2 * r2, drad = 2.0 * (k1 + 2.0 * k2 * r2);  // d rad / d r2, doubled
    const double xd = x + (x * rad + 2.0 * p1 * xy + p2 * (r2 + 2.0 * x2));
    const double yd = y + (y * rad + 2.0 * p2 * xy + p1 * (r2 + 2.0 * y2));
    const double xd_x = 1.0 + rad + x2 * drad + 2.0 * p1 * y + 6.0 * p2 * x;
    const double xd_y = xy * drad + 2.0 * p1 * x + 2.0 * p2 * y;
    const double yd_x = xy * drad + 2.0 * p2 * y + 2.0 * p1 * x;
    const double yd_y = 1.0 + rad + y2 * drad + 2.0 * p2 * x + 6.0 * p1 * y;
    JP[0] = fx * xd_x * iz; JP[1] = fx * xd_y * iz; JP[2] = -fx * (xd_x * x + xd_y * y) * iz;
    JP[3] = fy * yd_x * iz; JP[4] = fy * yd_y * iz; JP[5] = -fy * (yd_x * x + yd_y * y) * iz;
    JK[0] = xd; JK[1] = 0.0; JK[2] = 1.0; JK[3] = 0.0;
    JK[4] = fx * x * r2; JK[5] = fx * x * r2 * r2; JK[6] = fx * 2.0 * xy; JK[7] = fx * (r2 + 2.0 * x2);
    JK[8] = 0.0; JK[9] = yd; JK[10] = 0.0; JK[11] = 1.0;
    JK[12] = fy * y * r2; JK[13] = fy * y * r2 * r2; JK[14] = fy * (r2 + 2.0 * y2); JK[15] = fy * 2.0 * xy;
  } else {
    const double rho2 = P[0] * P[0] + P[1] * P[1];
    const double n2 = rho2 + P[2] * P[2];
    const double nrm = sqrt(n2), rho = sqrt(rho2);
    const double th = acos(P[2] / nrm), t2 = th * th;
    const double t3 = t2 * th, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
    const double r = th + c.dist[0] * t3 + c.dist[1] * t5 + c.dist[2] * t7 + c.dist[3] * t9;
    const double dr = 1.0 + t2 * (3.0 * c.dist[0] + t2 * (5.0 * c.dist[1] + t2 * (7.0 * c.dist[2] + t2 * 9.0 * c.dist[3])));
    if (rho > 1e-12 * nrm) {
      const double cph = P[0] / rho, sph = P[1] / rho;
      // d theta / d P = (x z, y z, -rho^2) / (|P|^2 rho); d phi / d P = (-y, x, 0) / rho^2
      const double a = P[2] / (n2 * rho);
      const double th0 = P[0] * a, th1 = P[1] * a, th2 = -rho / n2;
      const double ph0 = -P[1] / rho2, ph1 = P[0] / rho2;
      JP[0] = fx * (dr * cph * th0 - r * sph * ph0); JP[1] = fx * (dr * cph * th1 - r * sph * ph1); JP[2] = fx * (dr * cph * th2);
      JP[3] = fy * (dr * sph * th0 + r * cph * ph0); JP[4] = fy * (dr * sph * th1 + r * cph * ph1); JP[5] = fy * (dr * sph * th2);
      JK[0] = r * cph; JK[1] = 0.0; JK[2] = 1.0; JK[3] = 0.0;
      JK[4] = fx * t3 * cph; JK[5] = fx * t5 * cph; JK[6] = fx * t7 * cph; JK[7] = fx * t9 * cph;
      JK[8] = 0.0; JK[9] = r * sph; JK[10] = 0.0; JK[11] = 1.0;
      JK[12] = fy * t3 * sph; JK[13] = fy * t5 * sph; JK[14] = fy * t7 * sph; JK[15] = fy * t9 * sph;
    } else {
      const double iz = 1.0 / P[2];
      JP[0] = fx * iz; JP[1] = 0.0; JP[2] = 0.0;
      JP[3] = 0.0; JP[4] = fy * iz; JP[5] = 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) JK[i] = 0.0;
      JK[2] = 1.0;
      JK[11] = 1.0;
    }
  }
}

// The two residuals of board point (X, Y, 0) against pixel (u, v) at (R, t), scaled by inv_s, their Jacobians over the image's
// tangent (J[6 i + a]) and over the intrinsics (JK[8 i + q]); false when the point is not in front of the camera.
CLC_HD bool corner_terms(const clc_camera& c, const double* R, const double* t, double X, double Y, double u, double v, double inv_s,
                         double* r, double* J, double* JK) {
  CLC_BF_NO_CONTRACT
  const double P[3] = {(R[0] * X + R[1] * Y) + t[0], (R[3] * X + R[4] * Y) + t[1], (R[6] * X + R[7] * Y) + t[2]};
  double px[2], JP[6];
  cp::cam_project(c, P, px);
  project_jacobian(c, P, JP, JK);
  r[0] = (px[0] - u) * inv_s;
  r[1] = (px[1] - v) * inv_s;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double a0 = JP[3 * i] * inv_s, a1 = JP[3 * i + 1] * inv_s, a2 = JP[3 * i + 2] * inv_s;
    // dP/dt = I, dP/dtheta = -R [X]x
    const double B0 = (a0 * R[0] + a1 * R[3]) + a2 * R[6];
    const double B1 = (a0 * R[1] + a1 * R[4]) + a2 * R[7];
    const double B2 = (a0 * R[2] + a1 * R[5]) + a2 * R[8];
    J[6 * i] = a0; J[6 * i + 1] = a1; J[6 * i + 2] = a2;
    J[6 * i + 3] = B2 * Y;
    J[6 * i + 4] = -(B2 * X);
    J[6 * i + 5] = B1 * X - B0 * Y;
#pragma unroll
    for (int q = 0; q < NK; ++q) JK[8 * i + q] *= inv_s;
  }
  return P[2] > 0.0;
}

// One image's evaluation record at pose7 under camera c: every lane of the image's wave calls it (host: once); the lead lane stores.
CLC_HD void eval_image(const CalArgs& a, const clc_camera& c, long long img, const double* pose7, double* E) {
  CLC_BF_NO_CONTRACT
  double xe[7], R[9];
#pragma unroll
  for (int i = 0; i < 7; ++i) xe[i] = pose7[i];
  quat_to_rot(xe + 3, R);
  const long long cb = a.coff[img], n = a.coff[img + 1] - cb;
  const float* __restrict__ px = a.corners + 2 * cb;
  const float* __restrict__ board = a.board + 2 * cb;
  const double inv_s = 1.0 / a.sigma_px;
  {  // A_i, g_i, sum r^2
    double s[28];
    cp::wave_sum<28>([&](int lane, double* acc) {
      for (long long k = lane; k < n; k += cp::POSE_LANES) {
        double r[2], J[12], JK[16];
        const bool front = corner_terms(c, R, xe, board[2 * k], board[2 * k + 1], px[2 * k], px[2 * k + 1], inv_s, r, J, JK);
        int idx = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = p; q < 6; ++q) {
            acc[idx] = fma(J[p], J[q], acc[idx]);
            acc[idx] = fma(J[6 + p], J[6 + q], acc[idx]);
            ++idx;
          }
#pragma unroll
        for (int p = 0; p < 6; ++p) {
          acc[21 + p] = fma(J[p], r[0], acc[21 + p]);
          acc[21 + p] = fma(J[6 + p], r[1], acc[21 + p]);
        }
        acc[27] = fma(r[0], r[0], acc[27]);
        acc[27] = fma(r[1], r[1], acc[27]);
        if (!front) acc[27] += __builtin_inf();  // an invalid evaluation, as reproj_accumulate's
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 21; ++i) E[E_A + i] = s[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) E[E_G + i] = s[21 + i];
      E[E_COST] = 0.5 * s[27];
    }
  }
  {  // B_i[:, 0:4], g_c
    double s[32];
    cp::wave_sum<32>([&](int lane, double* acc) {
      for (long long k = lane; k < n; k += cp::POSE_LANES) {
        double r[2], J[12], JK[16];
        corner_terms(c, R, xe, board[2 * k], board[2 * k + 1], px[2 * k], px[2 * k + 1], inv_s, r, J, JK);
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            acc[4 * p + q] = fma(J[p], JK[q], acc[4 * p + q]);
            acc[4 * p + q] = fma(J[6 + p], JK[8 + q], acc[4 * p + q]);
          }
#pragma unroll
        for (int q = 0; q < NK; ++q) {
          acc[24 + q] = fma(JK[q], r[0], acc[24 + q]);
          acc[24 + q] = fma(JK[8 + q], r[1], acc[24 + q]);
        }
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) E[E_B + 8 * p + q] = s[4 * p + q];
#pragma unroll
      for (int q = 0; q < NK; ++q) E[E_GC + q] = s[24 + q];
    }
  }
  {  // B_i[:, 4:8]
    double s[24];
    cp::wave_sum<24>([&](int lane, double* acc) {
      for (long long k = lane; k < n; k += cp::POSE_LANES) {
        double r[2], J[12], JK[16];
        corner_terms(c, R, xe, board[2 * k], board[2 * k + 1], px[2 * k], px[2 * k + 1], inv_s, r, J, JK);
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            acc[4 * p + q] = fma(J[p], JK[4 + q], acc[4 * p + q]);
            acc[4 * p + q] = fma(J[6 + p], JK[12 + q], acc[4 * p + q]);
          }
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) E[E_B + 8 * p + 4 + q] = s[4 * p + q];
    }
  }
  {  // the image's share of C
    double s[36];
    cp::wave_sum<36>([&](int lane, double* acc) {
      for (long long k = lane; k < n; k += cp::POSE_LANES) {
        double r[2], J[12], JK[16];
        corner_terms(c, R, xe, board[2 * k], board[2 * k + 1], px[2 * k], px[2 * k + 1], inv_s, r, J, JK);
        int idx = 0;
#pragma unroll
        for (int p = 0; p < NK; ++p)
#pragma unroll
          for (int q = p; q < NK; ++q) {
            acc[idx] = fma(JK[p], JK[q], acc[idx]);
            acc[idx] = fma(JK[8 + p], JK[8 + q], acc[idx]);
            ++idx;
          }
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 36; ++i) E[E_C + i] = s[i];
    }
  }
}

CLC_HD void camera_of(const CalShared& sh, const double* k, clc_camera& c) {
  c.model = sh.model;
  c.reserved = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) { c.proj[i] = k[i]; c.dist[i] = k[4 + i]; }
}

// Why an image takes no part (wave-uniform; every lane of the image's wave calls it).
CLC_HD int image_status(const CalArgs& a, long long img) {
  if (a.keep && !a.keep[img]) return CLC_CAMCAL_NOT_KEPT;
  const long long cb = a.coff[img], n = a.coff[img + 1] - cb;
  if (n < 4) return CLC_CAMCAL_TOO_FEW;
  if (cb < 0) return CLC_CAMCAL_NONFINITE;
  const float* px = a.corners + 2 * cb;
  const float* board = a.board + 2 * cb;
  double bad[1];
  cp::wave_sum<1>([&](int lane, double* acc) {
    for (long long k = lane; k < n; k += cp::POSE_LANES)
      if (!(isfinite(px[2 * k]) && isfinite(px[2 * k + 1]) && isfinite(board[2 * k]) && isfinite(board[2 * k + 1]))) acc[0] += 1.0;
    if (lane < 4 && !finite_d(a.q[4 * img + lane])) acc[0] += 1.0;
    if (lane < 3 && !finite_d(a.t[3 * img + lane])) acc[0] += 1.0;
  }, bad);
  if (bad[0] != 0.0) return CLC_CAMCAL_NONFINITE;
  const double w = a.q[4 * img], x = a.q[4 * img + 1], y = a.q[4 * img + 2], z = a.q[4 * img + 3];
  if (!((w * w + x * x) + (y * y + z * z) > 0.0)) return CLC_CAMCAL_NONFINITE;
  return CLC_CAMCAL_OK;
}

// What K19 gives the arrow solve (clc_arrow.hpp): the shared block is the 8 intrinsics, moved additively, those of hold_mask held.
struct CalTraits {
  static constexpr int NC = NK, EVAL_DOUBLES = cc::EVAL_DOUBLES;
  using Args = CalArgs;
  using Image = CalImage;
  using Shared = CalShared;
  using Ctx = clc_camera;

  // clamped to the call's images: n_images from prob_off[0] on
  static CLC_HD aw::Problem<Image> problem(const Args& a, long long pb) {
    return aw::problem_range(a.prob_off, pb, a.prob_off ? a.prob_off[0] : 0, a.n_images, a.ws);
  }
  static CLC_HD int image_status(const Args& a, long long img) { return cc::image_status(a, img); }
  static CLC_HD long long observations(const Args& a, long long img) { return a.coff[img + 1] - a.coff[img]; }
  static CLC_HD void context(const Shared& sh, Ctx& c) { camera_of(sh, sh.kce, c); }
  static CLC_HD void eval_image(const Args& a, const Ctx& c, long long img, const double* pose7, double* E) {
    cc::eval_image(a, c, img, pose7, E);
  }
  static CLC_HD bool init_block(const Args& a, long long pb, long long n_corners, Shared& sh, double& xn) {
    const clc_camera& cam = a.cams[pb];
    bool ok = cam.model == CLC_CAMERA_PINHOLE || cam.model == CLC_CAMERA_KANNALA_BRANDT;
    CLC_AW_ROLLED for (int i = 0; i < 4; ++i) {
      sh.kc[i] = sh.kce[i] = cam.proj[i];
      sh.kc[4 + i] = sh.kce[4 + i] = cam.dist[i];
      ok = ok && finite_d(cam.proj[i]) && finite_d(cam.dist[i]);
    }
    sh.model = cam.model;
    sh.n_free = aw::free_parameters<NK>(sh.free_idx, [&](int i) { return !held(a, i); });
    sh.n_corners = n_corners;
    sh.move_c = sh.n_free > 0 ? 1 : 0;
    if (sh.move_c) CLC_AW_ROLLED for (int i = 0; i < NK; ++i) xn += sh.kc[i] * sh.kc[i];
    return ok;
  }
  static CLC_HD bool held(const Args& a, int p) { return (a.hold_mask >> p) & 1u; }
  static CLC_HD double cost(const double* tot) { return tot[E_COST - E_C]; }
  static CLC_HD double block_gradient(const Shared& sh, double m) { return aw::free_gradient<NK>(sh, 0, m); }
  // held intrinsics lose their rows and columns: chol_solve at the number of free ones
  static CLC_HD bool solve_block(Shared& sh) {
    bool ok;
    switch (sh.n_free) {
      case 1: ok = aw::solve_free<NK, 1>(sh); break;
      case 2: ok = aw::solve_free<NK, 2>(sh); break;
      case 3: ok = aw::solve_free<NK, 3>(sh); break;
      case 4: ok = aw::solve_free<NK, 4>(sh); break;
      case 5: ok = aw::solve_free<NK, 5>(sh); break;
      case 6: ok = aw::solve_free<NK, 6>(sh); break;
      case 7: ok = aw::solve_free<NK, 7>(sh); break;
      default: ok = aw::solve_free<NK, 8>(sh); break;
    }
    return aw::scatter_free(sh, ok);
  }
  static CLC_HD void block_candidate(Shared& sh, double& sn, double& xn) {
    CLC_AW_ROLLED for (int p = 0; p < NK; ++p) {
      // a held intrinsic (scale 0, step 0) keeps its bits
      const double d = sh.step_c[p] * sh.scale_c[p];
      sh.kce[p] = aw::additive_candidate(sh.kc[p], sh.scale_c[p] != 0.0 ? sh.kc[p] + d : sh.kc[p], sn, xn);
    }
  }
  static CLC_HD void accept_block(Shared& sh) {
    CLC_AW_ROLLED for (int i = 0; i < NK; ++i) sh.kc[i] = sh.kce[i];
  }
  static CLC_HD double* information(const Args& a) { return a.H_cam; }
  static CLC_HD void write_outputs(const Args& a, long long pb, const Shared& sh, bool failed) {
    if (!failed && sh.move_c)
      CLC_AW_ROLLED for (int f = 0; f < sh.n_free; ++f) {
        const int i = sh.free_idx[f];
        if (i < 4) a.cams[pb].proj[i] = sh.kc[i]; else a.cams[pb].dist[i - 4] = sh.kc[i];
      }
    if (a.rms) {
      const bool have = sh.n_evals > 0 && !failed && sh.n_corners > 0;
      a.rms[pb] = have ? a.sigma_px * sqrt(2.0 * sh.x_cost / (double)sh.n_corners) : __builtin_nan("");
    }
  }
};

// One problem: every thread of its workgroup calls it (host: once).
CLC_HD void camcal_problem(const CalArgs& a, long long pb, CalShared& sh) { aw::arrow_problem<CalTraits>(a, pb, sh); }

// ---- the closed-form focal start ---------------------------------------------------------------------------------------------
struct GuessShared {
  double acc45[45];
};

// The homography board (X, Y, 1) -> pixel - (cx0, cy0) of one image, unit Frobenius norm: H[9] row-major.  Every lane calls it
// (device: the image's wave; host: once).  Returns a CLC_POSE_* status (wave-uniform).  board_pose_image's DLT on pixels.
CLC_HD int homography_image(const float* __restrict__ px, const float* __restrict__ board, long long n, double cx0, double cy0,
                            GuessShared& sh, double* H) {
  CLC_BF_NO_CONTRACT
  if (n < 4) return CLC_POSE_TOO_FEW;
  double m[9];
  cp::wave_sum<9>([&](int lane, double* a) {
    for (long long k = lane; k < n; k += cp::POSE_LANES) {
      const double x = (double)px[2 * k] - cx0, y = (double)px[2 * k + 1] - cy0, X = board[2 * k], Y = board[2 * k + 1];
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
  const double si = sqrt(2.0 / var_i), sb = sqrt(2.0 / var_b);
  double acc[45];
  cp::wave_sum<45>([&](int lane, double* a) {
    for (long long k = lane; k < n; k += cp::POSE_LANES)
      cp::dlt_accumulate((((double)px[2 * k] - cx0) - cx) * si, (((double)px[2 * k + 1] - cy0) - cy) * si, (board[2 * k] - cX) * sb,
                         (board[2 * k + 1] - cY) * sb, a);
  }, acc);
  if (bf::lead_lane())
    for (int i = 0; i < 45; ++i) sh.acc45[i] = acc[i];
  cp::wave_barrier();
  bf::LaneRows<9> A, V;
  A.each([&](int k, double* row) {
#pragma unroll
    for (int j = 0; j < 9; ++j) row[j] = sh.acc45[cp::tri9(k, j)];
  });
  double w[9];
  bf::jacobi_rows<9, true>(A, V, w);
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) finite = finite && isfinite(w[i]);
  if (!finite) return CLC_POSE_NONFINITE;
  if (!(w[7] > cp::POSE_DEGENERATE_RATIO * w[0])) return CLC_POSE_DEGENERATE;
  double hn[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) hn[i] = V.at(i, 8);
  double Hb[9];  // Hn Tb
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    Hb[3 * r] = hn[3 * r] * sb;
    Hb[3 * r + 1] = hn[3 * r + 1] * sb;
    Hb[3 * r + 2] = (hn[3 * r + 2] - hn[3 * r] * sb * cX) - hn[3 * r + 1] * sb * cY;
  }
  double f2 = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    H[j] = Hb[j] / si + cx * Hb[6 + j];
    H[3 + j] = Hb[3 + j] / si + cy * Hb[6 + j];
    H[6 + j] = Hb[6 + j];
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) f2 += H[i] * H[i];
  if (!(f2 > 0.0) || !finite_d(f2)) return CLC_POSE_NONFINITE;
  const double inv = 1.0 / sqrt(f2);
#pragma unroll
  for (int i = 0; i < 9; ++i) H[i] *= inv;
  return CLC_POSE_OK;
}

// The host's half: the one-unknown least squares for u = 1 / f^2 over the usable images' homographies, in image order (Zhang's two
// constraints h1^T w h2 = 0, h1^T w h1 = h2^T w h2 with w = diag(u, u, 1)).  Returns the focal length, NaN when u is not positive and
// finite or fewer than 2 images are usable; *n_used = the usable images.
inline double guess_focal(const double* H, const int32_t* status, long long n_images, int32_t* n_used) {
  double sab = 0.0, saa = 0.0;
  int32_t used = 0;
  for (long long k = 0; k < n_images; ++k) {
    if (status[k] != CLC_POSE_OK) continue;
    const double* h = H + 9 * k;
    const double h1x = h[0], h1y = h[3], h1z = h[6], h2x = h[1], h2y = h[4], h2z = h[7];
    const double a1 = h1x * h2x + h1y * h2y, b1 = h1z * h2z;
    const double a2 = (h1x * h1x + h1y * h1y) - (h2x * h2x + h2y * h2y), b2 = h1z * h1z - h2z * h2z;
    sab += a1 * b1;
    sab += a2 * b2;
    saa += a1 * a1;
    saa += a2 * a2;
    ++used;
  }
  if (n_used) *n_used = used;
  if (used < 2) return __builtin_nan("");
  const double u = -sab / saa;
  if (!(u > 0.0) || !finite_d(u)) return __builtin_nan("");
  const double f = 1.0 / sqrt(u);
  return finite_d(f) ? f : __builtin_nan("");
}

#if defined(__HIPCC__)

// K19: one 256-thread workgroup per problem.
static __global__ __launch_bounds__(CAL_THREADS) void camcal_kernel(const CalArgs a) {
  __shared__ CalShared sh;
  camcal_problem(a, (long long)blockIdx.x, sh);
}

// The closed-form start's per-image half: one 64-thread workgroup (one wave) per image; off absolute, image `first` first in H / status.
static __global__ __launch_bounds__(64) void homography_kernel(const float* __restrict__ px, const float* __restrict__ board,
                                                               const long long* __restrict__ off, const double cx0, const double cy0,
                                                               double* __restrict__ H, int32_t* __restrict__ status) {
  __shared__ GuessShared sh;
  const long long img = blockIdx.x;
  const long long b = off[img], n = off[img + 1] - b;
  double h[9];
  const int st = (b >= 0 && n >= 0) ? homography_image(px + 2 * b, board + 2 * b, n, cx0, cy0, sh, h) : CLC_POSE_NONFINITE;
  if (threadIdx.x == 0) {
    status[img] = st;
    for (int i = 0; i < 9; ++i) H[9 * img + i] = st == CLC_POSE_OK ? h[i] : __builtin_nan("");
  }
}

#endif  // __HIPCC__

}  // namespace cc
}  // namespace clc
