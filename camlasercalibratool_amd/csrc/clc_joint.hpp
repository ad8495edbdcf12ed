// clc_joint.hpp — K18: joint refinement of the board poses T_ca,i and the camera-laser extrinsic T_cl of one problem, one cost
//
//   1/2 sum |((R_i X + t_i)_xy / (R_i X + t_i)_z - x_lifted) / sigma_corner|^2  +  1/2 sum (e3^T R_i^T (R_cl p + t_cl - t_i) / sigma_laser)^2
//
// over the tangent [dt, dtheta] of every pose.  The arrow of clc_arrow.hpp with the 6 tangent parameters of T_cl as its shared block:
// the solve (step, controller, outputs) is aw::arrow_problem; this file holds the cost and what is T_cl's own.
//
//   joint_refine_kernel   one 256-thread workgroup (4 waves) per problem, the whole Levenberg-Marquardt solve in one launch.
//     evaluation   per image a wave all-reduces (wave_sum of clc_campose.hpp) the corners' {H, g, sum r^2} (reproj_accumulate, as it
//                  is) and, in three passes over the laser points, {J_i J_i^T, J_i r, r^2}, J_i J_c^T and {J_c J_c^T, J_c r}; the lead
//                  lane stores A_i, B_i, g_i and the image's share of C, g_c and of the two cost parts.
//     reduced 6x6  chol_solve of clc_math.hpp, in place: the system the project's controllers solve.
//   Per-image state: JointImage, 3.5 KB.
//
// Everything numeric is CLC_HD: tests/shim/joint_shim.cpp compiles this header for the host with g++ and runs the same code with
// the threads as loops, in the same summation order.
#pragma once
#include "clc_arrow.hpp"

namespace clc {
namespace jt {

using aw::finite_d;

constexpr int JOINT_THREADS = aw::ARROW_THREADS;

// offsets into an evaluation record E[EVAL_DOUBLES] of one image (aw::ArrowRecord<6> and the two cost parts)
constexpr int E_A = 0, E_B = 21, E_G = 57, E_C = 63, E_GC = 84, E_COST_CORNER = 90, E_COST_LASER = 91, EVAL_DOUBLES = 92;
static_assert(E_G == aw::ArrowRecord<6>::E_G && E_C == aw::ArrowRecord<6>::E_C && E_GC == aw::ArrowRecord<6>::E_GC &&
                  E_COST_CORNER == aw::ArrowRecord<6>::E_COST, "the record of K18 is the arrow's");

using JointImage = aw::ArrowImage<6, EVAL_DOUBLES>;

struct JointShared : aw::ArrowShared<6, EVAL_DOUBLES> {
  double xc[7], xce[7];  // T_cl accepted / to evaluate
  double y[6];
  long long n_laser;
};

struct JointArgs {
  clc_options opt;
  double sigma_corner, sigma_laser;
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
  JointImage* ws;                 // [n_images], image first_image first
};

// The laser residual of point p and its Jacobians: r = e3^T R^T (R_cl p + t_cl - t) / sigma; Ji over [dt_i, dtheta_i], Jc over
// [dt_cl, dtheta_cl].
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

// One image's evaluation record at pose7 / (Rcl, tcl): every lane of the image's wave calls it (host: once); the lead lane stores.
CLC_HD void eval_image(const JointArgs& a, long long img, const double* pose7, const double* Rcl, const double* tcl, double* E) {
  CLC_BF_NO_CONTRACT
  double xe[7], R[9];
#pragma unroll
  for (int i = 0; i < 7; ++i) xe[i] = pose7[i];
  quat_to_rot(xe + 3, R);
  const long long cb = a.coff[img], n = a.coff[img + 1] - cb;
  const float* __restrict__ lifted = a.lifted + 2 * (cb - a.first_corner);
  const float* __restrict__ board = a.board + 2 * cb;
  double e[28];
  cp::wave_sum<28>([&](int lane, double* acc) {
    for (long long k = lane; k < n; k += cp::POSE_LANES)
      cp::reproj_accumulate(R, xe, board[2 * k], board[2 * k + 1], lifted[2 * k], lifted[2 * k + 1], acc);
  }, e);
  const double wc = 1.0 / (a.sigma_corner * a.sigma_corner), inv_s = 1.0 / a.sigma_laser;
  const long long pb = a.poff[img], np = a.poff[img + 1] - pb;
  const double* __restrict__ pts = a.pts + 3 * pb;
  if (bf::lead_lane()) {
#pragma unroll
    for (int i = 0; i < 21; ++i) E[E_A + i] = e[i] * wc;
#pragma unroll
    for (int i = 0; i < 6; ++i) E[E_G + i] = e[21 + i] * wc;
    E[E_COST_CORNER] = 0.5 * e[27] * wc;
  }
  if (np <= 0) {  // (wave-uniform)
    if (bf::lead_lane()) {
      CLC_AW_ROLLED for (int i = 0; i < 36; ++i) E[E_B + i] = 0.0;
      CLC_AW_ROLLED for (int i = E_C; i < E_COST_CORNER; ++i) E[i] = 0.0;
      E[E_COST_LASER] = 0.0;
    }
    return;
  }
  {  // J_i J_i^T, J_i r, r^2
    double s[28];
    cp::wave_sum<28>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[6], r;
        laser_point(R, xe, Rcl, tcl, pts + 3 * k, inv_s, Ji, Jc, &r);
        int idx = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = p; q < 6; ++q) { acc[idx] = fma(Ji[p], Ji[q], acc[idx]); ++idx; }
#pragma unroll
        for (int p = 0; p < 6; ++p) acc[21 + p] = fma(Ji[p], r, acc[21 + p]);
        acc[27] = fma(r, r, acc[27]);
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
  {  // J_i J_c^T
    double s[36];
    cp::wave_sum<36>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[6], r;
        laser_point(R, xe, Rcl, tcl, pts + 3 * k, inv_s, Ji, Jc, &r);
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = 0; q < 6; ++q) acc[6 * p + q] = fma(Ji[p], Jc[q], acc[6 * p + q]);
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 36; ++i) E[E_B + i] = s[i];
    }
  }
  {  // J_c J_c^T, J_c r
    double s[27];
    cp::wave_sum<27>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[6], r;
        laser_point(R, xe, Rcl, tcl, pts + 3 * k, inv_s, Ji, Jc, &r);
        int idx = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = p; q < 6; ++q) { acc[idx] = fma(Jc[p], Jc[q], acc[idx]); ++idx; }
#pragma unroll
        for (int p = 0; p < 6; ++p) acc[21 + p] = fma(Jc[p], r, acc[21 + p]);
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 27; ++i) E[E_C + i] = s[i];
    }
  }
}

// Why an image takes no part (wave-uniform; every lane of the image's wave calls it).
CLC_HD int image_status(const JointArgs& a, long long img) {
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

// What K18 gives the arrow solve (clc_arrow.hpp): the shared block is the pose T_cl, 6 tangent parameters, none of them held.
struct JointTraits {
  static constexpr int NC = 6, EVAL_DOUBLES = jt::EVAL_DOUBLES;
  using Args = JointArgs;
  using Image = JointImage;
  using Shared = JointShared;
  struct Ctx { double Rcl[9], tcl[3]; };

  // clamped to [first_image, first_image + n_images)
  static CLC_HD aw::Problem<Image> problem(const Args& a, long long pb) {
    long long i0 = a.prob_off ? a.prob_off[pb] : a.first_image, i1 = a.prob_off ? a.prob_off[pb + 1] : a.first_image + a.n_images;
    if (i0 < a.first_image) i0 = a.first_image;
    if (i1 > a.first_image + a.n_images) i1 = a.first_image + a.n_images;
    return {i0, i1 > i0 ? i1 - i0 : 0, a.ws + (i0 - a.first_image)};
  }
  static CLC_HD int image_status(const Args& a, long long img) { return jt::image_status(a, img); }
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
    jt::eval_image(a, img, pose7, c.Rcl, c.tcl, E);
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
CLC_HD void joint_problem(const JointArgs& a, long long pb, JointShared& sh) { aw::arrow_problem<JointTraits>(a, pb, sh); }

#if defined(__HIPCC__)

// K18: one 256-thread workgroup per problem.
static __global__ __launch_bounds__(JOINT_THREADS) void joint_refine_kernel(const JointArgs a) {
  __shared__ JointShared sh;
  joint_problem(a, (long long)blockIdx.x, sh);
}

// The ranges a device-array call needs on the host to size its scratch: {first image, first corner, end of the corners}.
static __global__ void joint_ends_kernel(const long long* __restrict__ prob_off, const long long* __restrict__ coff, const long long n_images,
                                         long long* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const long long first = prob_off ? prob_off[0] : 0;
  out[0] = first;
  const bool ok = first >= 0;
  out[1] = ok ? coff[first] : 0;
  out[2] = ok ? coff[first + n_images] : -1;
}

#endif  // __HIPCC__

}  // namespace jt
}  // namespace clc
