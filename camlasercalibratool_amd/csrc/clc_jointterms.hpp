// clc_jointterms.hpp — the terms the joint problems K18, K21, K22 and K23 are built from (clc_joint.hpp, clc_laserrange.hpp,
// clc_jointrobust.hpp, clc_fullcal.hpp): the laser residual with its Jacobians, the range correction and the point rules, the Cauchy
// loss, the rule by which an image takes part (K18, K21, K22; K23's solve kernel keeps a copy), the skeleton of the weights, and the
// evaluation passes of K18 and K22.  A leaf over clc_arrow.hpp: inline functions and one single-thread kernel, no solve
// kernel.  A unit still includes one kernel header only and is held to its own register figures (tests/test_*_resources.py); what the
// kernels share is what they include from here, so that a change to a term reaches every problem that the tests hold equal bit for bit
// (K22 without loss against K18, K21 with the range held against K18, K23 reduced onto K19 and K21).
//
// The passes over the laser points sum w J^T J and w J^T r in groups that a kernel chooses (its register figures depend on the
// grouping, its bits do not: an accumulator sums the same terms in the same lane order whatever else its pass holds).  K18 and K22
// take the three passes of laser_passes.  K21 and K23 keep theirs written out in their headers: through the shared bodies their
// kernels summed the same terms in another instruction order and measured slower (profiles/joint_terms_refactor.md).
//
// Everything numeric is CLC_HD: the shims of tests/shim compile it for the host with g++ through the kernel headers.
#pragma once
#include "clc_arrow.hpp"

namespace clc {
namespace jtm {

using aw::finite_d;

// ---- point rules ------------------------------------------------------------------------------------------------------------
// |p|, summed as everywhere in this file.
CLC_HD double point_range(const double* p) {
  CLC_BF_NO_CONTRACT
  return sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
}

// A point K18 and K22 take: finite.
CLC_HD bool point_finite(const double* p) { return finite_d(p[0]) && finite_d(p[1]) && finite_d(p[2]); }

// A point the range model takes: finite with a range that is finite and > 0 (a zero range is the scanner's "no return").
CLC_HD bool point_usable(const double* p) {
  const double rho = point_range(p);
  return finite_d(p[0]) && finite_d(p[1]) && finite_d(p[2]) && finite_d(rho) && rho > 0.0;
}

// p' = (1 + kappa + b / |p|) p; uh = p / |p|.  (b, kappa) = (0, 0) gives p itself, bit for bit.
CLC_HD void correct_point(const double* p, double b, double kappa, double* pc, double* uh) {
  CLC_BF_NO_CONTRACT
  const double rho = point_range(p), inv = 1.0 / rho;
  const double s = (1.0 + kappa) + b / rho;  // (the model's own expression, not b * inv: one rounding fewer)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    uh[i] = p[i] * inv;
    pc[i] = s * p[i];
  }
}

// ---- the laser residual -----------------------------------------------------------------------------------------------------
// d = R_cl p + t_cl - t: the point from the board's origin, camera frame.
CLC_HD void laser_offset(const double* t, const double* Rcl, const double* tcl, const double* p, double* d) {
  CLC_BF_NO_CONTRACT
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = (((Rcl[3 * i] * p[0] + Rcl[3 * i + 1] * p[1]) + Rcl[3 * i + 2] * p[2]) + tcl[i]) - t[i];
}

// The laser row of point p, and u = R_cl^T n (n = R e3) for range_point's two more columns: laser_point's body.
CLC_HD void laser_row(const double* R, const double* t, const double* Rcl, const double* tcl, const double* p, double inv_s, double* Ji,
                      double* Jc, double* r, double* u) {
  CLC_BF_NO_CONTRACT
  double d[3];
  laser_offset(t, Rcl, tcl, p, d);
  const double m0 = (R[0] * d[0] + R[3] * d[1]) + R[6] * d[2];
  const double m1 = (R[1] * d[0] + R[4] * d[1]) + R[7] * d[2];
  const double m2 = (R[2] * d[0] + R[5] * d[1]) + R[8] * d[2];
  const double n0 = R[2], n1 = R[5], n2 = R[8];
  *r = m2 * inv_s;
  Ji[0] = -n0 * inv_s; Ji[1] = -n1 * inv_s; Ji[2] = -n2 * inv_s;
  Ji[3] = -m1 * inv_s; Ji[4] = m0 * inv_s; Ji[5] = 0.0;
  // d r / d theta_cl = (p x u) / sigma
  const double u0 = (Rcl[0] * n0 + Rcl[3] * n1) + Rcl[6] * n2;
  const double u1 = (Rcl[1] * n0 + Rcl[4] * n1) + Rcl[7] * n2;
  const double u2 = (Rcl[2] * n0 + Rcl[5] * n1) + Rcl[8] * n2;
  Jc[0] = n0 * inv_s; Jc[1] = n1 * inv_s; Jc[2] = n2 * inv_s;
  Jc[3] = (p[1] * u2 - p[2] * u1) * inv_s;
  Jc[4] = (p[2] * u0 - p[0] * u2) * inv_s;
  Jc[5] = (p[0] * u1 - p[1] * u0) * inv_s;
  u[0] = u0; u[1] = u1; u[2] = u2;
}
// The laser residual of point p and its Jacobians: r = e3^T R^T (R_cl p + t_cl - t) / sigma; Ji over [dt_i, dtheta_i], Jc over
// [dt_cl, dtheta_cl].
CLC_HD void laser_point(const double* R, const double* t, const double* Rcl, const double* tcl, const double* p, double inv_s, double* Ji,
                        double* Jc, double* r) {
  double u[3];
  laser_row(R, t, Rcl, tcl, p, inv_s, Ji, Jc, r, u);
}

// The laser residual alone (the m2 of laser_point, the same expression).
CLC_HD double laser_residual(const double* R, const double* t, const double* Rcl, const double* tcl, const double* p, double inv_s) {
  CLC_BF_NO_CONTRACT
  double d[3];
  laser_offset(t, Rcl, tcl, p, d);
  return ((R[2] * d[0] + R[5] * d[1]) + R[8] * d[2]) * inv_s;
}

// The laser residual of the measured point p under the range correction and its Jacobians: laser_point at p', and Jc's two more
// columns over [b, kappa]: d r / d b = (u . p / |p|) / sigma, d r / d kappa = (u . p) / sigma.
CLC_HD void range_point(const double* R, const double* t, const double* Rcl, const double* tcl, double b, double kappa, const double* p,
                        double inv_s, double* Ji, double* Jc, double* r) {
  CLC_BF_NO_CONTRACT
  double pc[3], uh[3], u[3];
  correct_point(p, b, kappa, pc, uh);
  laser_row(R, t, Rcl, tcl, pc, inv_s, Ji, Jc, r, u);
  Jc[6] = ((u[0] * uh[0] + u[1] * uh[1]) + u[2] * uh[2]) * inv_s;
  Jc[7] = ((u[0] * p[0] + u[1] * p[1]) + u[2] * p[2]) * inv_s;
}

// ---- the Cauchy loss --------------------------------------------------------------------------------------------------------
// rho_a and rho_a' at z, with a2 = a^2 and inv_a2 = 1 / a^2.  z = inf (a corner behind the camera): weight 0, rho inf.
CLC_HD double cauchy_weight(double z, double inv_a2) { return 1.0 / (1.0 + z * inv_a2); }
CLC_HD double cauchy_rho(double z, double a2, double inv_a2) { return a2 * log1p(z * inv_a2); }

// The loss scales of a call (in units of sigma; 0: no loss on that term), prepared once per evaluation.
struct Loss {
  bool corner, laser;
  double ac2, inv_ac2, al2, inv_al2;
};
CLC_HD Loss loss_of(double loss_corner, double loss_laser) {
  Loss l;
  l.corner = loss_corner != 0.0;
  l.laser = loss_laser != 0.0;
  l.ac2 = loss_corner * loss_corner;
  l.al2 = loss_laser * loss_laser;
  l.inv_ac2 = l.corner ? 1.0 / l.ac2 : 0.0;
  l.inv_al2 = l.laser ? 1.0 / l.al2 : 0.0;
  return l;
}
// The weight of a laser row with residual r (exactly 1 without the loss: w J then has J's bits), and its term of the cost sum.
CLC_HD double laser_weight(const Loss& ls, double r) { return ls.laser ? cauchy_weight(r * r, ls.inv_al2) : 1.0; }
CLC_HD double laser_cost(const Loss& ls, double r, double acc) {
  return ls.laser ? acc + cauchy_rho(r * r, ls.al2, ls.inv_al2) : fma(r, r, acc);
}

// f(lane) on the 64 lanes of a wave (host: a loop).
template <class F>
CLC_HD void each_wave_lane(F f) {
#if defined(__HIP_DEVICE_COMPILE__)
  f((int)(threadIdx.x & 63));
#else
  for (int l = 0; l < cp::POSE_LANES; ++l) f(l);
#endif
}

// ---- the passes of K18 and K22: the shared block is T_cl's six columns (aw::ArrowRecord<6>, Jc[6]) --------------------------
// Every lane of the image's wave calls them (host: once), the lead lane stores.  K21 and K23 keep their passes written out in their
// headers: through these bodies their kernels summed the same terms in another instruction order and measured slower.
using Rec6 = aw::ArrowRecord<6>;

// Per-point accumulations over six columns; wl is the left factor, weighted by the caller.
// acc[tri<6>(p, q)] += wl[p] x[q], p <= q
CLC_HD void acc_sym(const double* wl, const double* x, double* acc) {
  int idx = 0;
#pragma unroll
  for (int p = 0; p < 6; ++p)
#pragma unroll
    for (int q = p; q < 6; ++q) { acc[idx] = fma(wl[p], x[q], acc[idx]); ++idx; }
}
// acc[6 p + q] += wl[p] x[q]
CLC_HD void acc_outer(const double* wl, const double* x, double* acc) {
#pragma unroll
  for (int p = 0; p < 6; ++p)
#pragma unroll
    for (int q = 0; q < 6; ++q) acc[6 * p + q] = fma(wl[p], x[q], acc[6 * p + q]);
}
// acc[p] += wl[p] r
CLC_HD void acc_vec(const double* wl, double r, double* acc) {
#pragma unroll
  for (int p = 0; p < 6; ++p) acc[p] = fma(wl[p], r, acc[p]);
}
// The left factor of a laser row's products and its term of the cost sum: under a loss (W) w x in wx and rho, without one x itself
// and r^2 (not 1 x: K18 then keeps the registers of the unweighted sums).
template <bool W>
CLC_HD const double* left_factor(const Loss& ls, double r, const double* x, double* wx) {
  if (!W) return x;
  const double w = laser_weight(ls, r);
#pragma unroll
  for (int p = 0; p < 6; ++p) wx[p] = w * x[p];
  return wx;
}
template <bool W>
CLC_HD double cost_term(const Loss& ls, double r, double acc) { return W ? laser_cost(ls, r, acc) : fma(r, r, acc); }

// The corner part of a record from the 28 sums e of a corner pass in units of the lift: A_i and g_i scaled by wc = 1 / sigma^2.
CLC_HD void store_corner_sums(const double* e, double wc, double cost, double* E) {
  if (!bf::lead_lane()) return;
#pragma unroll
  for (int i = 0; i < 21; ++i) E[Rec6::E_A + i] = e[i] * wc;
#pragma unroll
  for (int i = 0; i < 6; ++i) E[Rec6::E_G + i] = e[21 + i] * wc;
  E[Rec6::E_COST] = cost;
}
// The unweighted pass over n lifted corners (reproj_accumulate, as it is).
CLC_HD void lifted_corner_pass(const float* __restrict__ lifted, const float* __restrict__ board, long long n, const double* R,
                               const double* xe, double wc, double* E) {
  double e[28];
  cp::wave_sum<28>([&](int lane, double* acc) {
    for (long long k = lane; k < n; k += cp::POSE_LANES)
      cp::reproj_accumulate(R, xe, board[2 * k], board[2 * k + 1], lifted[2 * k], lifted[2 * k + 1], acc);
  }, e);
  store_corner_sums(e, wc, 0.5 * e[27] * wc, E);
}
// The laser part of a record of an image without a laser point.
CLC_HD void zero_laser_part(double* E) {
  if (!bf::lead_lane()) return;
  CLC_AW_ROLLED for (int i = 0; i < 36; ++i) E[Rec6::E_B + i] = 0.0;
  CLC_AW_ROLLED for (int i = Rec6::E_C; i < Rec6::E_COST; ++i) E[i] = 0.0;
  E[Rec6::E_COST + 1] = 0.0;
}

// The three passes over the np laser points, each recomputing the row and, under the loss ls (W), its weight: {w J_i J_i^T, w J_i r,
// cost} (28 sums, added to the corners' A_i and g_i), w J_i J_c^T (36) and {w J_c J_c^T, w J_c r} (27).  point(k, Ji, Jc, &r) gives
// row k.
template <bool W, class P>
CLC_HD void laser_passes(long long np, const Loss& ls, P point, double* E) {
  {
    double s[28];
    cp::wave_sum<28>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[6], wx[6], r;
        point(k, Ji, Jc, &r);
        const double* wJ = left_factor<W>(ls, r, Ji, wx);
        acc_sym(wJ, Ji, acc);
        acc_vec(wJ, r, acc + 21);
        acc[27] = cost_term<W>(ls, r, acc[27]);
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 21; ++i) E[Rec6::E_A + i] += s[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) E[Rec6::E_G + i] += s[21 + i];
      E[Rec6::E_COST + 1] = 0.5 * s[27];
    }
  }
  {
    double s[36];
    cp::wave_sum<36>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[6], wx[6], r;
        point(k, Ji, Jc, &r);
        acc_outer(left_factor<W>(ls, r, Ji, wx), Jc, acc);
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 36; ++i) E[Rec6::E_B + i] = s[i];
    }
  }
  {
    double s[Rec6::SS];
    cp::wave_sum<Rec6::SS>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[6], wx[6], r;
        point(k, Ji, Jc, &r);
        const double* wJ = left_factor<W>(ls, r, Jc, wx);
        acc_sym(wJ, Jc, acc);
        acc_vec(wJ, r, acc + Rec6::TRI);
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < Rec6::SS; ++i) E[Rec6::E_C + i] = s[i];
    }
  }
}
// ... without a loss (K18; the loss is never read without W)
template <class P>
CLC_HD void laser_passes(long long np, P point, double* E) {
  laser_passes<false>(np, Loss(), point, E);
}

// ---- which images take part -------------------------------------------------------------------------------------------------
// What the rule and the weights read of a call.  The corner observations `obs` (lifted or pixels) start at corner obs_first, the
// board, w_corner and w_laser are indexed by the absolute offsets; coff NULL: the corners take no part and none is read; an image's
// corners must lie in [c_first, c_end).
struct ImageView {
  const float *obs, *board;
  const long long* coff;
  long long obs_first, c_first, c_end;
  const double* pts;
  const long long* poff;
  const unsigned char* keep;  // nullable
  const double *q, *t;
  const int32_t* status;
  double *w_corner, *w_laser;  // nullable
};
constexpr long long NO_CORNER_END = 0x7FFFFFFFFFFFFFFFll;  // c_end of a call that names no end

// Why an image takes no part (wave-uniform; every lane of the image's wave calls it); point_ok(p): a point the problem takes.
template <class Pt>
CLC_HD int image_status(const ImageView& v, long long img, Pt point_ok) {
  if (v.keep && !v.keep[img]) return CLC_JOINT_NOT_KEPT;
  const long long pb = v.poff[img], np = v.poff[img + 1] - pb;
  long long n = 0;
  const float *obs = nullptr, *board = nullptr;
  if (v.coff) {
    const long long cb = v.coff[img];
    n = v.coff[img + 1] - cb;
    if (n < 4) return CLC_JOINT_TOO_FEW;
    if (cb < v.c_first || cb + n > v.c_end) return CLC_JOINT_NONFINITE;
    obs = v.obs + 2 * (cb - v.obs_first);
    board = v.board + 2 * cb;
  }
  if (np < 0 || pb < 0) return CLC_JOINT_NONFINITE;
  const double* pts = v.pts + 3 * pb;
  double bad[1];
  cp::wave_sum<1>([&](int lane, double* acc) {
    for (long long k = lane; k < n; k += cp::POSE_LANES)
      if (!(isfinite(obs[2 * k]) && isfinite(obs[2 * k + 1]) && isfinite(board[2 * k]) && isfinite(board[2 * k + 1]))) acc[0] += 1.0;
    for (long long k = lane; k < np; k += cp::POSE_LANES)
      if (!point_ok(pts + 3 * k)) acc[0] += 1.0;
    if (lane < 4 && !finite_d(v.q[4 * img + lane])) acc[0] += 1.0;
    if (lane < 3 && !finite_d(v.t[3 * img + lane])) acc[0] += 1.0;
  }, bad);
  if (bad[0] != 0.0) return CLC_JOINT_NONFINITE;
  const double w = v.q[4 * img], x = v.q[4 * img + 1], y = v.q[4 * img + 2], z = v.q[4 * img + 3];
  if (!((w * w + x * x) + (y * y + z * z) > 0.0)) return CLC_JOINT_NONFINITE;
  return CLC_JOINT_OK;
}

// ---- the traits of K18 and K22 ------------------------------------------------------------------------------------------------
// What a problem whose shared block is the pose T_cl alone (6 tangent parameters, none of them held one by one) gives the arrow
// solve, but for its image_status and eval_image.  A: its arguments (prob_off, first_image, n_images, ws, poff, hold_extrinsic,
// poses_cl, H_cl, cost_parts), S: its shared state (xc, xce, y, n_laser).
template <class A, class I, class S>
struct TclTraits {
  static constexpr int NC = 6, EVAL_DOUBLES = aw::ArrowRecord<6>::E_COST + 2;
  using Args = A;
  using Image = I;
  using Shared = S;
  struct Ctx { double Rcl[9], tcl[3]; };

  static CLC_HD aw::Problem<Image> problem(const Args& a, long long pb) {
    return aw::problem_range(a.prob_off, pb, a.first_image, a.n_images, a.ws);
  }
  static CLC_HD long long observations(const Args& a, long long img) { return a.poff[img + 1] - a.poff[img]; }
  static CLC_HD void context(const Shared& sh, Ctx& c) { aw::tcl_context(sh, c); }
  static CLC_HD bool init_block(const Args& a, long long pb, long long n_laser, Shared& sh, double& xn) {
    const bool ok = aw::tcl_init(a.poses_cl + 7 * pb, sh);
    sh.n_laser = n_laser;
    sh.move_c = (a.hold_extrinsic || n_laser == 0) ? 0 : 1;
    if (sh.move_c) CLC_AW_ROLLED for (int i = 0; i < 7; ++i) xn += sh.xc[i] * sh.xc[i];
    return ok;
  }
  static CLC_HD bool held(const Args&, int) { return false; }
  static CLC_HD double cost(const double* tot) { return aw::cost_of_parts<6>(tot); }
  static CLC_HD double block_gradient(const Shared& sh, double m) { return sh.move_c ? aw::tcl_gradient<6>(sh, m) : m; }
  static CLC_HD bool solve_block(Shared& sh) {
    bool ok = chol_solve<6>(sh.A, sh.rhs, sh.y, sh.L, sh.z);
    CLC_AW_ROLLED for (int p = 0; p < 6; ++p) {
      sh.step_c[p] = -sh.y[p];
      if (!finite_d(sh.y[p])) ok = false;
    }
    return ok;
  }
  static CLC_HD void block_candidate(Shared& sh, double& sn, double& xn) { aw::tcl_candidate(sh, false, sn, xn); }
  static CLC_HD void accept_block(Shared& sh) { aw::tcl_accept(sh); }
  static CLC_HD double* information(const Args& a) { return a.H_cl; }
  static CLC_HD void write_outputs(const Args& a, long long pb, const Shared& sh, bool failed) {
    if (!failed && sh.move_c) CLC_AW_ROLLED for (int i = 0; i < 7; ++i) a.poses_cl[7 * pb + i] = sh.xc[i];
    aw::write_cost_parts<6>(a.cost_parts, pb, sh, failed);
  }
};

// ---- the weights ------------------------------------------------------------------------------------------------------------
// The weights of one image at the returned point, after the solve: every lane of the image's wave calls it (host: once).  `failed`:
// the image's problem ended CLC_FAILURE.  An image that takes no part gets NaN over the ranges its offsets name, where these lie
// inside the call's arrays (an image whose offsets leave them has status CLC_JOINT_NONFINITE and nothing is written for it).  A term
// without loss has weight 1; corner_weight(R, xe, obs, board, k) and laser_weight(R, xe, pts, k) give rho' of observation k of the
// image at its pose xe = [t, q(xyzw)], R its rotation.
template <class CW, class LW>
CLC_HD void weights_image(const ImageView& v, const Loss& ls, long long img, bool failed, CW corner_weight, LW laser_weight) {
  CLC_BF_NO_CONTRACT
  const long long pb = v.poff[img], np = v.poff[img + 1] - pb;
  long long cb = 0, n = 0;
  if (v.coff) {
    cb = v.coff[img];
    n = v.coff[img + 1] - cb;
  }
  const bool corners_in = v.coff && cb >= v.c_first && n >= 0 && cb + n <= v.c_end, points_in = pb >= 0 && np >= 0;
  const bool part = v.status[img] == CLC_JOINT_OK && !failed;
  if (!part) {
    each_wave_lane([&](int lane) {
      if (v.w_corner && corners_in)
        for (long long k = lane; k < n; k += cp::POSE_LANES) v.w_corner[cb + k] = __builtin_nan("");
      if (v.w_laser && points_in)
        for (long long k = lane; k < np; k += cp::POSE_LANES) v.w_laser[pb + k] = __builtin_nan("");
    });
    return;
  }
  // the pose as the solve reads it: [t, q(xyzw)] normalised
  const double qw = v.q[4 * img], qx = v.q[4 * img + 1], qy = v.q[4 * img + 2], qz = v.q[4 * img + 3];
  const double inv = 1.0 / sqrt((qw * qw + qx * qx) + (qy * qy + qz * qz));
  const double xe[7] = {v.t[3 * img], v.t[3 * img + 1], v.t[3 * img + 2], qx * inv, qy * inv, qz * inv, qw * inv};
  double R[9];
  quat_to_rot(xe + 3, R);
  const float* __restrict__ obs = v.coff ? v.obs + 2 * (cb - v.obs_first) : nullptr;
  const float* __restrict__ board = v.coff ? v.board + 2 * cb : nullptr;
  const double* __restrict__ pts = v.pts + 3 * pb;
  each_wave_lane([&](int lane) {
    if (v.w_corner)
      for (long long k = lane; k < n; k += cp::POSE_LANES) v.w_corner[cb + k] = ls.corner ? corner_weight(R, xe, obs, board, k) : 1.0;
    if (v.w_laser)
      for (long long k = lane; k < np; k += cp::POSE_LANES) v.w_laser[pb + k] = ls.laser ? laser_weight(R, xe, pts, k) : 1.0;
  });
}

#if defined(__HIPCC__)

// The ranges a device-array call needs on the host to size its scratch: {first image, first corner, end of the corners}; coff NULL
// (the corners take no part): no corners.  A template, so that a unit which never launches it (K23's sizes its workspace from n_images)
// holds no such kernel.
template <int = 0>
static __global__ void joint_ends_kernel(const long long* __restrict__ prob_off, const long long* __restrict__ coff, const long long n_images,
                                         long long* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const long long first = prob_off ? prob_off[0] : 0;
  out[0] = first;
  const bool ok = first >= 0 && coff != nullptr;
  out[1] = ok ? coff[first] : 0;
  out[2] = ok ? coff[first + n_images] : (first >= 0 ? 0 : -1);
}

#endif  // __HIPCC__

}  // namespace jtm
}  // namespace clc
