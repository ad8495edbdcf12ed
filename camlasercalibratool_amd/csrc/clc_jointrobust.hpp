// clc_jointrobust.hpp — K22: K18's joint refinement with a Cauchy loss on every corner and on every laser point,
//
//   1/2 sum rho_ac(|e_j|^2) + 1/2 sum rho_al(r_k^2)        rho_a(z) = a^2 log1p(z / a^2),  rho_a'(z) = 1 / (1 + z / a^2)
//
//   e_j = ((R_i X + t_i)_xy / (R_i X + t_i)_z - x_lifted) / sigma_corner   (one loss on the squared norm of the corner's 2-vector)
//   r_k = e3^T R_i^T (R_cl p + t_cl - t_i) / sigma_laser
//
// The scales a are in units of sigma (loss_corner, loss_laser); a = 0: no loss on that term, rho(z) = z, and that term's sums are
// K18's expressions, bit for bit.  The Gauss-Newton blocks follow Ceres' corrector for rho'' <= 0: every row of an observation and
// its residual are scaled by sqrt(rho'), so A_i, B_i, C take w J^T J and the gradients w J^T r with w = rho'(z).  The fourth arrow
// problem of clc_arrow.hpp (NC = 6, K18's record): the solve (step, controller, outputs) is aw::arrow_problem; this file holds the
// cost.  The residual and Jacobian expressions of the laser term are clc_joint.hpp's laser_point, restated.
//
//   joint_robust_kernel    one 256-thread workgroup (4 waves) per problem, the whole Levenberg-Marquardt solve in one launch.
//     evaluation   per image a wave all-reduces the corners' 28 sums — per corner one reproj_accumulate into a zeroed local row
//                  gives z (its sum r^2 entry / sigma^2), and the row is added scaled by w — and makes K18's three passes over the
//                  laser points, each recomputing the residual and its weight; the cost entries sum rho.
//   joint_weights_kernel   one workgroup per problem, one wave per image, lanes stride over its corners and points at the
//                  returned poses: w_corner, w_laser = rho'(z); 1 where the term has no loss, NaN for an image that takes no part
//                  or a problem that ended CLC_FAILURE.
//   Per-image state: RobustImage = K18's JointImage, 3.5 KB.
//
// Everything numeric is CLC_HD: tests/shim/jointrobust_shim.cpp compiles this header for the host with g++ and runs the same code
// with the threads as loops, in the same summation order (log1p is the platform's: the device and the host build agree to rounding,
// not bit for bit, where a loss is on).
#pragma once
#include "clc_arrow.hpp"

namespace clc {
namespace jr {

using aw::finite_d;

constexpr int ROBUST_THREADS = aw::ARROW_THREADS;

// offsets into an evaluation record E[EVAL_DOUBLES] of one image (aw::ArrowRecord<6> and the two cost parts): K18's
constexpr int E_A = 0, E_B = 21, E_G = 57, E_C = 63, E_GC = 84, E_COST_CORNER = 90, E_COST_LASER = 91, EVAL_DOUBLES = 92;
static_assert(E_G == aw::ArrowRecord<6>::E_G && E_C == aw::ArrowRecord<6>::E_C && E_GC == aw::ArrowRecord<6>::E_GC &&
                  E_COST_CORNER == aw::ArrowRecord<6>::E_COST, "the record of K22 is the arrow's");

using RobustImage = aw::ArrowImage<6, EVAL_DOUBLES>;

struct RobustShared : aw::ArrowShared<6, EVAL_DOUBLES> {
  double xc[7], xce[7];  // T_cl accepted / to evaluate
  double y[6];
  long long n_laser;
};

struct RobustArgs {
  clc_options opt;
  double sigma_corner, sigma_laser;
  double loss_corner, loss_laser;  // Cauchy scales in units of sigma; 0: no loss
  int32_t hold_board_poses, hold_extrinsic;
  const float* lifted;   // rounded x/z, y/z, corner `first_corner` first, n_corners of them
  const float* board;    // indexed by the absolute corner offsets
  const long long* coff; // [image] absolute
  long long first_corner, n_corners;
  const double* pts;
  const long long* poff;
  const unsigned char* keep;      // nullable
  const long long* prob_off;      // nullable: one problem over [first_image, first_image + n_images)
  long long first_image, n_images;
  double *q, *t, *poses_cl;
  clc_summary* summaries;
  double *H_cl, *cost_parts;      // nullable
  int32_t* status;
  double *w_corner, *w_laser;     // nullable; indexed by the absolute corner / point offsets
  RobustImage* ws;                // [n_images], image first_image first
};

// rho_a and rho_a' at z, with a2 = a^2 and inv_a2 = 1 / a^2.  z = inf (a corner behind the camera): weight 0, rho inf.
CLC_HD double cauchy_weight(double z, double inv_a2) { return 1.0 / (1.0 + z * inv_a2); }
CLC_HD double cauchy_rho(double z, double a2, double inv_a2) { return a2 * log1p(z * inv_a2); }

// The laser residual of point p and its Jacobians (clc_joint.hpp's laser_point): r = e3^T R^T (R_cl p + t_cl - t) / sigma; Ji over
// [dt_i, dtheta_i], Jc over [dt_cl, dtheta_cl].
CLC_HD void laser_point(const double* R, const double* t, const double* Rcl, const double* tcl, const double* p, double inv_s, double* Ji,
                        double* Jc, double* r) {
  CLC_BF_NO_CONTRACT
  double d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = (((Rcl[3 * i] * p[0] + Rcl[3 * i + 1] * p[1]) + Rcl[3 * i + 2] * p[2]) + tcl[i]) - t[i];
  const double m0 = (R[0] * d[0] + R[3] * d[1]) + R[6] * d[2];
  const double m1 = (R[1] * d[0] + R[4] * d[1]) + R[7] * d[2];
  const double m2 = (R[2] * d[0] + R[5] * d[1]) + R[8] * d[2];
  const double n0 = R[2], n1 = R[5], n2 = R[8];
  *r = m2 * inv_s;
  Ji[0] = -n0 * inv_s; Ji[1] = -n1 * inv_s; Ji[2] = -n2 * inv_s;
  Ji[3] = -m1 * inv_s; Ji[4] = m0 * inv_s; Ji[5] = 0.0;
  // u = R_cl^T n; d r / d theta_cl = (p x u) / sigma
  const double u0 = (Rcl[0] * n0 + Rcl[3] * n1) + Rcl[6] * n2;
  const double u1 = (Rcl[1] * n0 + Rcl[4] * n1) + Rcl[7] * n2;
  const double u2 = (Rcl[2] * n0 + Rcl[5] * n1) + Rcl[8] * n2;
  Jc[0] = n0 * inv_s; Jc[1] = n1 * inv_s; Jc[2] = n2 * inv_s;
  Jc[3] = (p[1] * u2 - p[2] * u1) * inv_s;
  Jc[4] = (p[2] * u0 - p[0] * u2) * inv_s;
  Jc[5] = (p[0] * u1 - p[1] * u0) * inv_s;
}

// The laser residual alone (the m2 of laser_point, the same expression).
CLC_HD double laser_residual(const double* R, const double* t, const double* Rcl, const double* tcl, const double* p, double inv_s) {
  CLC_BF_NO_CONTRACT
  double d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = (((Rcl[3 * i] * p[0] + Rcl[3 * i + 1] * p[1]) + Rcl[3 * i + 2] * p[2]) + tcl[i]) - t[i];
  return ((R[2] * d[0] + R[5] * d[1]) + R[8] * d[2]) * inv_s;
}

// z = |e|^2 of one corner: reproj_accumulate's sum r^2 entry over sigma^2, from a zeroed row (infinite behind the camera).
CLC_HD double corner_z(const double* R, const double* t, double X, double Y, double u, double v, double wc, double* row) {
#pragma unroll
  for (int i = 0; i < 28; ++i) row[i] = 0.0;
  cp::reproj_accumulate(R, t, X, Y, u, v, row);
  return row[27] * wc;
}

// One image's evaluation record at pose7 / (Rcl, tcl): every lane of the image's wave calls it (host: once); the lead lane stores.
CLC_HD void eval_image(const RobustArgs& a, long long img, const double* pose7, const double* Rcl, const double* tcl, double* E) {
  CLC_BF_NO_CONTRACT
  double xe[7], R[9];
#pragma unroll
  for (int i = 0; i < 7; ++i) xe[i] = pose7[i];
  quat_to_rot(xe + 3, R);
  const long long cb = a.coff[img], n = a.coff[img + 1] - cb;
  const float* __restrict__ lifted = a.lifted + 2 * (cb - a.first_corner);
  const float* __restrict__ board = a.board + 2 * cb;
  const double wc = 1.0 / (a.sigma_corner * a.sigma_corner), inv_s = 1.0 / a.sigma_laser;
  const bool corner_loss = a.loss_corner != 0.0, laser_loss = a.loss_laser != 0.0;  // (uniform over the call)
  const double ac2 = a.loss_corner * a.loss_corner, inv_ac2 = corner_loss ? 1.0 / ac2 : 0.0;
  const double al2 = a.loss_laser * a.loss_laser, inv_al2 = laser_loss ? 1.0 / al2 : 0.0;
  double e[28];
  if (!corner_loss) {  // K18's sums
    cp::wave_sum<28>([&](int lane, double* acc) {
      for (long long k = lane; k < n; k += cp::POSE_LANES)
        cp::reproj_accumulate(R, xe, board[2 * k], board[2 * k + 1], lifted[2 * k], lifted[2 * k + 1], acc);
    }, e);
  } else {
    cp::wave_sum<28>([&](int lane, double* acc) {
      for (long long k = lane; k < n; k += cp::POSE_LANES) {
        double row[28];
        const double z = corner_z(R, xe, board[2 * k], board[2 * k + 1], lifted[2 * k], lifted[2 * k + 1], wc, row);
        const double w = cauchy_weight(z, inv_ac2);
#pragma unroll
        for (int i = 0; i < 27; ++i) acc[i] = fma(w, row[i], acc[i]);
        acc[27] += cauchy_rho(z, ac2, inv_ac2);
      }
    }, e);
  }
  const long long pb = a.poff[img], np = a.poff[img + 1] - pb;
  const double* __restrict__ pts = a.pts + 3 * pb;
  if (bf::lead_lane()) {
#pragma unroll
    for (int i = 0; i < 21; ++i) E[E_A + i] = e[i] * wc;
#pragma unroll
    for (int i = 0; i < 6; ++i) E[E_G + i] = e[21 + i] * wc;
    E[E_COST_CORNER] = corner_loss ? 0.5 * e[27] : 0.5 * e[27] * wc;  // (with the loss e[27] is sum rho, in units of sigma already)
  }
  if (np <= 0) {  // (wave-uniform)
    if (bf::lead_lane()) {
      CLC_AW_ROLLED for (int i = 0; i < 36; ++i) E[E_B + i] = 0.0;
      CLC_AW_ROLLED for (int i = E_C; i < E_COST_CORNER; ++i) E[i] = 0.0;
      E[E_COST_LASER] = 0.0;
    }
    return;
  }
  // The three passes of K18; each recomputes r and w = rho'(r^2).  Without the loss w is exactly 1 and w J has J's bits.
  {  // w J_i J_i^T, w J_i r, sum rho
    double s[28];
    cp::wave_sum<28>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[6], wJ[6], r;
        laser_point(R, xe, Rcl, tcl, pts + 3 * k, inv_s, Ji, Jc, &r);
        const double w = laser_loss ? cauchy_weight(r * r, inv_al2) : 1.0;
#pragma unroll
        for (int p = 0; p < 6; ++p) wJ[p] = w * Ji[p];
        int idx = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = p; q < 6; ++q) { acc[idx] = fma(wJ[p], Ji[q], acc[idx]); ++idx; }
#pragma unroll
        for (int p = 0; p < 6; ++p) acc[21 + p] = fma(wJ[p], r, acc[21 + p]);
        acc[27] = laser_loss ? acc[27] + cauchy_rho(r * r, al2, inv_al2) : fma(r, r, acc[27]);
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
  {  // w J_i J_c^T
    double s[36];
    cp::wave_sum<36>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[6], wJ[6], r;
        laser_point(R, xe, Rcl, tcl, pts + 3 * k, inv_s, Ji, Jc, &r);
        const double w = laser_loss ? cauchy_weight(r * r, inv_al2) : 1.0;
#pragma unroll
        for (int p = 0; p < 6; ++p) wJ[p] = w * Ji[p];
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = 0; q < 6; ++q) acc[6 * p + q] = fma(wJ[p], Jc[q], acc[6 * p + q]);
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 36; ++i) E[E_B + i] = s[i];
    }
  }
  {  // w J_c J_c^T, w J_c r
    double s[27];
    cp::wave_sum<27>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[6], wJ[6], r;
        laser_point(R, xe, Rcl, tcl, pts + 3 * k, inv_s, Ji, Jc, &r);
        const double w = laser_loss ? cauchy_weight(r * r, inv_al2) : 1.0;
#pragma unroll
        for (int p = 0; p < 6; ++p) wJ[p] = w * Jc[p];
        int idx = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = p; q < 6; ++q) { acc[idx] = fma(wJ[p], Jc[q], acc[idx]); ++idx; }
#pragma unroll
        for (int p = 0; p < 6; ++p) acc[21 + p] = fma(wJ[p], r, acc[21 + p]);
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 27; ++i) E[E_C + i] = s[i];
    }
  }
}

// Why an image takes no part (wave-uniform; every lane of the image's wave calls it): K18's rule.
CLC_HD int image_status(const RobustArgs& a, long long img) {
  if (a.keep && !a.keep[img]) return CLC_JOINT_NOT_KEPT;
  const long long cb = a.coff[img], n = a.coff[img + 1] - cb, pb = a.poff[img], np = a.poff[img + 1] - pb;
  if (n < 4) return CLC_JOINT_TOO_FEW;
  if (cb < a.first_corner || cb + n > a.first_corner + a.n_corners || np < 0 || pb < 0) return CLC_JOINT_NONFINITE;
  const float* lifted = a.lifted + 2 * (cb - a.first_corner);
  const float* board = a.board + 2 * cb;
  const double* pts = a.pts + 3 * pb;
  double bad[1];
  cp::wave_sum<1>([&](int lane, double* acc) {
    for (long long k = lane; k < n; k += cp::POSE_LANES)
      if (!(isfinite(lifted[2 * k]) && isfinite(lifted[2 * k + 1]) && isfinite(board[2 * k]) && isfinite(board[2 * k + 1]))) acc[0] += 1.0;
    for (long long k = lane; k < np; k += cp::POSE_LANES)
      if (!(finite_d(pts[3 * k]) && finite_d(pts[3 * k + 1]) && finite_d(pts[3 * k + 2]))) acc[0] += 1.0;
    if (lane < 4 && !finite_d(a.q[4 * img + lane])) acc[0] += 1.0;
    if (lane < 3 && !finite_d(a.t[3 * img + lane])) acc[0] += 1.0;
  }, bad);
  if (bad[0] != 0.0) return CLC_JOINT_NONFINITE;
  const double w = a.q[4 * img], x = a.q[4 * img + 1], y = a.q[4 * img + 2], z = a.q[4 * img + 3];
  if (!((w * w + x * x) + (y * y + z * z) > 0.0)) return CLC_JOINT_NONFINITE;
  return CLC_JOINT_OK;
}

// [first image, images) of problem pb, clamped to [first_image, first_image + n_images)
CLC_HD void problem_range(const RobustArgs& a, long long pb, long long* i0, long long* P) {
  long long b = a.prob_off ? a.prob_off[pb] : a.first_image, e = a.prob_off ? a.prob_off[pb + 1] : a.first_image + a.n_images;
  if (b < a.first_image) b = a.first_image;
  if (e > a.first_image + a.n_images) e = a.first_image + a.n_images;
  *i0 = b;
  *P = e > b ? e - b : 0;
}

// What K22 gives the arrow solve (clc_arrow.hpp): the shared block is the pose T_cl, 6 tangent parameters, none of them held — K18's
// traits over the robust evaluation.
struct JointRobustTraits {
  static constexpr int NC = 6, EVAL_DOUBLES = jr::EVAL_DOUBLES;
  using Args = RobustArgs;
  using Image = RobustImage;
  using Shared = RobustShared;
  struct Ctx { double Rcl[9], tcl[3]; };

  static CLC_HD aw::Problem<Image> problem(const Args& a, long long pb) {
    long long i0, P;
    problem_range(a, pb, &i0, &P);
    return {i0, P, a.ws + (i0 - a.first_image)};
  }
  static CLC_HD int image_status(const Args& a, long long img) { return jr::image_status(a, img); }
  static CLC_HD long long observations(const Args& a, long long img) { return a.poff[img + 1] - a.poff[img]; }
  static CLC_HD void context(const Shared& sh, Ctx& c) {
    double q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = sh.xce[3 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) c.tcl[i] = sh.xce[i];
    quat_to_rot(q, c.Rcl);
  }
  static CLC_HD void eval_image(const Args& a, const Ctx& c, long long img, const double* pose7, double* E) {
    jr::eval_image(a, img, pose7, c.Rcl, c.tcl, E);
  }
  static CLC_HD bool init_block(const Args& a, long long pb, long long n_laser, Shared& sh, double& xn) {
    bool ok = true;
    CLC_AW_ROLLED for (int i = 0; i < 7; ++i) {
      const double v = a.poses_cl[7 * pb + i];
      sh.xc[i] = sh.xce[i] = v;
      ok = ok && finite_d(v);
    }
    sh.n_laser = n_laser;
    sh.move_c = (a.hold_extrinsic || n_laser == 0) ? 0 : 1;
    if (sh.move_c) CLC_AW_ROLLED for (int i = 0; i < 7; ++i) xn += sh.xc[i] * sh.xc[i];
    return ok;
  }
  static CLC_HD bool held(const Args&, int) { return false; }
  static CLC_HD double cost(const double* tot) { return tot[E_COST_CORNER - E_C] + tot[E_COST_LASER - E_C]; }
  static CLC_HD double block_gradient(const Shared& sh, double m) {
    return sh.move_c ? fmax(m, aw::block_gradient_norm(sh.xc, sh.tot[sh.cur] + (E_GC - E_C))) : m;
  }
  static CLC_HD bool solve_block(Shared& sh) {
    bool ok = chol_solve<6>(sh.A, sh.rhs, sh.y, sh.L, sh.z);
    CLC_AW_ROLLED for (int p = 0; p < 6; ++p) {
      sh.step_c[p] = -sh.y[p];
      if (!finite_d(sh.y[p])) ok = false;
    }
    return ok;
  }
  static CLC_HD void block_candidate(Shared& sh, double& sn, double& xn) {
    double n2;
    sn += aw::block_candidate(sh.xc, sh.step_c, sh.scale_c, sh.xce, &n2);
    xn += n2;
  }
  static CLC_HD void accept_block(Shared& sh) {
    CLC_AW_ROLLED for (int i = 0; i < 7; ++i) sh.xc[i] = sh.xce[i];
  }
  static CLC_HD double* information(const Args& a) { return a.H_cl; }
  static CLC_HD void write_outputs(const Args& a, long long pb, const Shared& sh, bool failed) {
    if (!failed && sh.move_c) CLC_AW_ROLLED for (int i = 0; i < 7; ++i) a.poses_cl[7 * pb + i] = sh.xc[i];
    if (a.cost_parts) {
      const bool have = sh.n_evals > 0 && !failed;
      a.cost_parts[2 * pb] = have ? sh.tot[sh.cur][E_COST_CORNER - E_C] : __builtin_nan("");
      a.cost_parts[2 * pb + 1] = have ? sh.tot[sh.cur][E_COST_LASER - E_C] : __builtin_nan("");
    }
  }
};

// One problem: every thread of its workgroup calls it (host: once).
CLC_HD void robust_problem(const RobustArgs& a, long long pb, RobustShared& sh) { aw::arrow_problem<JointRobustTraits>(a, pb, sh); }

// f(lane) on the 64 lanes of a wave (host: a loop).
template <class F>
CLC_HD void each_wave_lane(F f) {
#if defined(__HIP_DEVICE_COMPILE__)
  f((int)(threadIdx.x & 63));
#else
  for (int l = 0; l < cp::POSE_LANES; ++l) f(l);
#endif
}

// The weights of one image at the returned poses, after the solve: every lane of the image's wave calls it (host: once).  `failed`:
// the image's problem ended CLC_FAILURE.  An image that takes no part gets NaN over the ranges its offsets name, where these lie
// inside the call's arrays (an image whose offsets leave them has status CLC_JOINT_NONFINITE and nothing is written for it).
CLC_HD void weights_image(const RobustArgs& a, long long img, bool failed, const double* pose_cl) {
  CLC_BF_NO_CONTRACT
  const long long cb = a.coff[img], n = a.coff[img + 1] - cb, pb = a.poff[img], np = a.poff[img + 1] - pb;
  const bool corners_in = cb >= a.first_corner && n >= 0 && cb + n <= a.first_corner + a.n_corners, points_in = pb >= 0 && np >= 0;
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
  const double wc = 1.0 / (a.sigma_corner * a.sigma_corner), inv_s = 1.0 / a.sigma_laser;
  const bool corner_loss = a.loss_corner != 0.0, laser_loss = a.loss_laser != 0.0;
  const double inv_ac2 = corner_loss ? 1.0 / (a.loss_corner * a.loss_corner) : 0.0;
  const double inv_al2 = laser_loss ? 1.0 / (a.loss_laser * a.loss_laser) : 0.0;
  const float* __restrict__ lifted = a.lifted + 2 * (cb - a.first_corner);
  const float* __restrict__ board = a.board + 2 * cb;
  const double* __restrict__ pts = a.pts + 3 * pb;
  each_wave_lane([&](int lane) {
    if (a.w_corner)
      for (long long k = lane; k < n; k += cp::POSE_LANES) {
        double w = 1.0;
        if (corner_loss) {
          double row[28];
          w = cauchy_weight(corner_z(R, xe, board[2 * k], board[2 * k + 1], lifted[2 * k], lifted[2 * k + 1], wc, row), inv_ac2);
        }
        a.w_corner[cb + k] = w;
      }
    if (a.w_laser)
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double w = 1.0;
        if (laser_loss) {
          const double r = laser_residual(R, xe, Rcl, pose_cl, pts + 3 * k, inv_s);
          w = cauchy_weight(r * r, inv_al2);
        }
        a.w_laser[pb + k] = w;
      }
  });
}

// The weights of one problem: the waves take its images round-robin (host: a loop).
CLC_HD void weights_problem(const RobustArgs& a, long long pb) {
  long long i0, P;
  problem_range(a, pb, &i0, &P);
  const bool failed = a.summaries[pb].termination == CLC_FAILURE;
  double pose_cl[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) pose_cl[i] = a.poses_cl[7 * pb + i];
  aw::each_image_wave(P, [&](long long j) { weights_image(a, i0 + j, failed, pose_cl); });
}

#if defined(__HIPCC__)

// K22: one 256-thread workgroup per problem.
static __global__ __launch_bounds__(ROBUST_THREADS) void joint_robust_kernel(const RobustArgs a) {
  __shared__ RobustShared sh;
  robust_problem(a, (long long)blockIdx.x, sh);
}

// The weights at the returned poses: one workgroup per problem, one wave per image.  Runs after joint_robust_kernel on its stream.
static __global__ __launch_bounds__(ROBUST_THREADS) void joint_weights_kernel(const RobustArgs a) {
  weights_problem(a, (long long)blockIdx.x);
}

// The ranges a device-array call needs on the host to size its scratch: {first image, first corner, end of the corners}.
static __global__ void robust_ends_kernel(const long long* __restrict__ prob_off, const long long* __restrict__ coff, const long long n_images,
                                          long long* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const long long first = prob_off ? prob_off[0] : 0;
  out[0] = first;
  const bool ok = first >= 0;
  out[1] = ok ? coff[first] : 0;
  out[2] = ok ? coff[first + n_images] : -1;
}

#endif  // __HIPCC__

}  // namespace jr
}  // namespace clc
