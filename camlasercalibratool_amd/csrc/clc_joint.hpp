// clc_joint.hpp — K18: joint refinement of the board poses T_ca,i and the camera-laser extrinsic T_cl of one problem, one cost
//
//   1/2 sum |((R_i X + t_i)_xy / (R_i X + t_i)_z - x_lifted) / sigma_corner|^2  +  1/2 sum (e3^T R_i^T (R_cl p + t_cl - t_i) / sigma_laser)^2
//
// over the tangent [dt, dtheta] of every pose (Se3Manifold: t += dt, R <- R Exp(dtheta)).  The normal matrix is an arrow: a 6x6
// block A_i per image, coupled through B_i (6x6) only to the 6x6 block C of T_cl; the Schur complement over the images leaves the
// 6x6 system the project's controllers solve.
//
//   joint_refine_kernel   one 256-thread workgroup (4 waves) per problem, the whole Levenberg-Marquardt solve in one launch.
//     evaluation   the waves take the images round-robin; per image a wave all-reduces (wave_sum of clc_campose.hpp) the corners'
//                  {H, g, sum r^2} (reproj_accumulate, as it is) and, in three passes over the laser points, {J_i J_i^T, J_i r, r^2},
//                  J_i J_c^T and {J_c J_c^T, J_c r}; the lead lane stores A_i, B_i, g_i and the image's share of C, g_c and of the two
//                  cost parts.  The shares are then added over the images in image order, one entry per lane.
//     step         one image per lane: the scaled, damped A_i + D_i factored, Y_i = (A_i + D_i)^-1 B_i, S_i = B_i^T Y_i,
//                  s_i = B_i^T (A_i + D_i)^-1 g_i; S and s added over the images in image order; thread 0 solves the reduced 6x6
//                  (chol_solve of clc_math.hpp) for delta_c; the lanes back-substitute delta_i = -(A_i + D_i)^-1 (g_i + B_i delta_c).
//                  A rejected step repeats only this with the new radius: the blocks of the accepted point are kept.
//     controller   thread 0, state in LDS: the semantics of clc_lm.hpp (Jacobi scaling fixed at the first evaluation over all 6 + 6P
//                  columns, the diagonal clamp, the radius rule, the three tolerances, the iteration cap), written over the arrow.
//   Per-image state (the blocks of the accepted and of the candidate point, poses, scaling, factor: JointImage, 3.5 KB) lives in a
//   workspace in device memory indexed by image: any number of images fits, and every access goes through pointers, so the
//   per-lane 6x6 algebra needs no private arrays (no scratch).  Every sum has a fixed shape (butterflies within a wave, image
//   order across images): no atomics, the same bits on every run, and a problem never reads another problem's state.
//
// Everything numeric is CLC_HD: tests/shim/joint_shim.cpp compiles this header for the host with g++ and runs the same code with
// the threads as loops, in the same summation order.
#pragma once
#include "clc_campose.hpp"

namespace clc {
namespace jt {

constexpr int JOINT_THREADS = 256;
constexpr int JOINT_WAVES = JOINT_THREADS / 64;

#if defined(__HIP_DEVICE_COMPILE__)
#define CLC_JT_ROLLED _Pragma("nounroll")
#else
#define CLC_JT_ROLLED
#endif

// offsets into an evaluation record E[EVAL_DOUBLES] of one image
constexpr int E_A = 0, E_B = 21, E_G = 57, E_C = 63, E_GC = 84, E_COST_CORNER = 90, E_COST_LASER = 91, EVAL_DOUBLES = 92;
constexpr int TOTAL_DOUBLES = EVAL_DOUBLES - E_C;  // C, g_c, the two cost parts

struct JointImage {
  double x[7], xe[7];           // accepted pose, pose the next evaluation uses: [t, qx, qy, qz, qw]
  double E[2][EVAL_DOUBLES];    // the blocks at the accepted point (sh.cur) and at the candidate
  double scale[6], diag[6];     // Jacobi scaling, clamped diagonal of the scaled A
  double As[36], Md[36], L[36]; // scaled A, scaled damped A, its Cholesky factor (inverse diagonal)
  double Bs[36], Y[36];         // scaled B, (A + D)^-1 B
  double gs[6], yg[6], z[6];    // scaled g, (A + D)^-1 g, substitution scratch
  double Ss[27];                // S_i (21, tri<6> order) and s_i (6)
  double step[6];               // delta_i in the scaled space
  double red[6];                // shares: step.g, step^T H step, |x - xe|^2, |xe|^2, gradient max norm, bad-step flag
  int32_t st;                   // CLC_JOINT_*
  int32_t pad_;
};

struct JointShared {
  double xc[7], xce[7];  // T_cl accepted / to evaluate
  double tot[2][TOTAL_DOUBLES];
  double scale_c[6], diag_c[6], step_c[6], gs_c[6], rhs[6];
  double Ss[27], red[6];
  double Hs[36], A[36], L[36], y[6], z[6];
  double x_cost, x_norm, initial_cost, min_iter_cost, radius, decrease_factor, model_cost_change, gmax;
  double it_cost, it_gmax;
  long long n_evals, n_laser;
  int32_t status, n_invalid, reuse_diagonal, num_successful, num_unsuccessful, n_trace, cur, step_ok, move_c, move_i, n_part;
  int32_t it_iteration, it_successful;
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

// ---- the workgroup of one problem; on the host the threads are loops ----
template <class F>
CLC_HD void each_image(long long P, F f) {  // one image per thread
#if defined(__HIP_DEVICE_COMPILE__)
  for (long long j = threadIdx.x; j < P; j += JOINT_THREADS) f(j);
#else
  for (long long j = 0; j < P; ++j) f(j);
#endif
}
template <class F>
CLC_HD void each_image_wave(long long P, F f) {  // the waves take the images round-robin
#if defined(__HIP_DEVICE_COMPILE__)
  for (long long j = threadIdx.x >> 6; j < P; j += JOINT_WAVES) f(j);
#else
  for (long long j = 0; j < P; ++j) f(j);
#endif
}
template <class F>
CLC_HD void each_lane(int K, F f) {  // K <= JOINT_THREADS entries, one per thread
#if defined(__HIP_DEVICE_COMPILE__)
  if ((int)threadIdx.x < K) f((int)threadIdx.x);
#else
  for (int k = 0; k < K; ++k) f(k);
#endif
}
CLC_HD void wg_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}
CLC_HD bool wg_lead() {
#if defined(__HIP_DEVICE_COMPILE__)
  return threadIdx.x == 0;
#else
  return true;
#endif
}

CLC_HD bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }

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
      CLC_JT_ROLLED for (int i = 0; i < 36; ++i) E[E_B + i] = 0.0;
      CLC_JT_ROLLED for (int i = E_C; i < E_COST_CORNER; ++i) E[i] = 0.0;
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

// The factor of chol_solve (clc_math.hpp): L with the inverse diagonal.  false if a pivot is not positive.
CLC_HD bool chol_factor6(const double* A, double* L) {
  CLC_JT_ROLLED for (int j = 0; j < 6; ++j) {
    double d = A[6 * j + j];
    CLC_JT_ROLLED for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k];
    if (!(d > 0.0)) return false;
    const double inv = rsqrt_pos(d);
    L[6 * j + j] = inv;
    CLC_JT_ROLLED for (int i = j + 1; i < 6; ++i) {
      double s = A[6 * i + j];
      CLC_JT_ROLLED for (int k = 0; k < j; ++k) s -= L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = s * inv;
    }
  }
  return true;
}

// y = (L L^T)^-1 b, b and y strided; z[6] scratch.
CLC_HD void chol_apply6(const double* L, const double* b, int bs, double* y, int ys, double* z) {
  CLC_JT_ROLLED for (int i = 0; i < 6; ++i) {
    double s = b[bs * i];
    CLC_JT_ROLLED for (int k = 0; k < i; ++k) s -= L[6 * i + k] * z[k];
    z[i] = s * L[6 * i + i];
  }
  CLC_JT_ROLLED for (int i = 5; i >= 0; --i) {
    double s = z[i];
    CLC_JT_ROLLED for (int k = i + 1; k < 6; ++k) s -= L[6 * k + i] * y[ys * k];
    y[ys * i] = s * L[6 * i + i];
  }
}

// Y = M^-1 B and S = B^T Y (tri<6> order) of one image, from im.L.
CLC_HD void schur_share(JointImage& im, const double* B) {
  CLC_JT_ROLLED for (int b = 0; b < 6; ++b) chol_apply6(im.L, B + b, 6, im.Y + b, 6, im.z);
  int idx = 0;
  CLC_JT_ROLLED for (int p = 0; p < 6; ++p)
    CLC_JT_ROLLED for (int q = p; q < 6; ++q) {
      double s = 0.0;
      CLC_JT_ROLLED for (int k = 0; k < 6; ++k) s += B[6 * k + p] * im.Y[6 * k + q];
      im.Ss[idx++] = s;
    }
}

// ||x - Plus(x, -g)||_inf of one pose block.
CLC_HD double block_gradient_norm(const double* x, const double* g) {
  double xx[7], ng[6], pr[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) xx[i] = x[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) ng[i] = -g[i];
  pose_plus_rcp(xx, ng, pr);
  double m = 0.0;
#pragma unroll
  for (int i = 0; i < 7; ++i) m = fmax(m, fabs(xx[i] - pr[i]));
  return m;
}

// out = Plus(x, step * scale); returns |x - out|^2, *n2 = |out|^2
CLC_HD double block_candidate(const double* x, const double* step, const double* scale, double* out, double* n2) {
  double xx[7], dl[6], pr[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) xx[i] = x[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) dl[i] = step[i] * scale[i];
  pose_plus_rcp(xx, dl, pr);
  double s = 0.0, nn = 0.0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    out[i] = pr[i];
    s += (xx[i] - pr[i]) * (xx[i] - pr[i]);
    nn += pr[i] * pr[i];
  }
  *n2 = nn;
  return s;
}

struct Problem {
  long long i0, P;   // first image (absolute), images
  JointImage* ws;    // image i0 first
};

// Adds the images' shares in image order: sh.red (sums of 0..3, maxima of 4..5).
CLC_HD void reduce_red(const Problem& pr, JointShared& sh) {
  each_lane(6, [&](int k) {
    double s = 0.0;
    for (long long j = 0; j < pr.P; ++j) {
      const JointImage& im = pr.ws[j];
      if (im.st != CLC_JOINT_OK) continue;
      s = k < 4 ? s + im.red[k] : fmax(s, im.red[k]);
    }
    sh.red[k] = s;
  });
}

// Evaluates every participating image at its xe and T_cl at sh.xce into record `set`; the totals into sh.tot[set].
CLC_HD void evaluate(const JointArgs& a, const Problem& pr, JointShared& sh, int set) {
  double Rcl[9], tcl[3];
  {
    double q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = sh.xce[3 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tcl[i] = sh.xce[i];
    quat_to_rot(q, Rcl);
  }
  each_image_wave(pr.P, [&](long long j) {
    JointImage& im = pr.ws[j];
    if (im.st != CLC_JOINT_OK) return;
    eval_image(a, pr.i0 + j, im.xe, Rcl, tcl, im.E[set]);
  });
  wg_barrier();
  each_lane(TOTAL_DOUBLES, [&](int k) {
    double s = 0.0;
    for (long long j = 0; j < pr.P; ++j) {
      const JointImage& im = pr.ws[j];
      if (im.st != CLC_JOINT_OK) continue;
      s += im.E[set][E_C + k];
    }
    sh.tot[set][k] = s;
  });
  wg_barrier();
}

// The gradient max norm over the moving blocks at the accepted point (record sh.cur) -> sh.gmax.
CLC_HD void gradient_norm(const Problem& pr, JointShared& sh) {
  each_image(pr.P, [&](long long j) {
    JointImage& im = pr.ws[j];
    if (im.st != CLC_JOINT_OK) return;
    im.red[4] = sh.move_i ? block_gradient_norm(im.x, im.E[sh.cur] + E_G) : 0.0;
    im.red[5] = 0.0;
  });
  wg_barrier();
  reduce_red(pr, sh);
  wg_barrier();
  if (wg_lead()) {
    double m = sh.red[4];
    if (sh.move_c) m = fmax(m, block_gradient_norm(sh.xc, sh.tot[sh.cur] + (E_GC - E_C)));
    sh.gmax = m;
  }
  wg_barrier();
}

// The trust-region step at the accepted point for sh.radius: every image's xe and sh.xce become the candidate, sh.step_ok says
// whether it is valid (LevenbergMarquardtStrategy::ComputeStep + the model-cost test, over the arrow).
CLC_HD void compute_step(const JointArgs& a, const Problem& pr, JointShared& sh) {
  const clc_options& o = a.opt;
  const double inv_radius = rcp_pos(sh.radius);
  const int reuse = sh.reuse_diagonal, cur = sh.cur;
  if (sh.move_i) {
    each_image(pr.P, [&](long long j) {
      JointImage& im = pr.ws[j];
      if (im.st != CLC_JOINT_OK) return;
      const double* E = im.E[cur];
      int idx = 0;
      CLC_JT_ROLLED for (int p = 0; p < 6; ++p)
        CLC_JT_ROLLED for (int q = p; q < 6; ++q) {
          const double v = E[E_A + idx++] * (im.scale[p] * im.scale[q]);
          im.As[6 * p + q] = v;
          im.As[6 * q + p] = v;
        }
      if (!reuse) {
        CLC_JT_ROLLED for (int c = 0; c < 6; ++c) {
          double d = im.As[7 * c];
          d = d > o.min_lm_diagonal ? d : o.min_lm_diagonal;
          d = d < o.max_lm_diagonal ? d : o.max_lm_diagonal;
          im.diag[c] = d;
        }
      }
      CLC_JT_ROLLED for (int i = 0; i < 36; ++i) im.Md[i] = im.As[i];
      CLC_JT_ROLLED for (int c = 0; c < 6; ++c) im.Md[7 * c] += im.diag[c] * inv_radius;
      CLC_JT_ROLLED for (int p = 0; p < 6; ++p) im.gs[p] = E[E_G + p] * im.scale[p];
      CLC_JT_ROLLED for (int p = 0; p < 6; ++p)
        CLC_JT_ROLLED for (int q = 0; q < 6; ++q) im.Bs[6 * p + q] = E[E_B + 6 * p + q] * (im.scale[p] * sh.scale_c[q]);
      im.red[5] = 0.0;
      CLC_JT_ROLLED for (int i = 0; i < 27; ++i) im.Ss[i] = 0.0;
      if (!chol_factor6(im.Md, im.L)) { im.red[5] = 1.0; return; }
      chol_apply6(im.L, im.gs, 1, im.yg, 1, im.z);
      if (sh.move_c) {
        schur_share(im, im.Bs);
        CLC_JT_ROLLED for (int p = 0; p < 6; ++p) {
          double s = 0.0;
          CLC_JT_ROLLED for (int k = 0; k < 6; ++k) s += im.Bs[6 * k + p] * im.yg[k];
          im.Ss[21 + p] = s;
        }
      }
    });
    wg_barrier();
    each_lane(27, [&](int k) {
      double s = 0.0;
      for (long long j = 0; j < pr.P; ++j) {
        const JointImage& im = pr.ws[j];
        if (im.st != CLC_JOINT_OK) continue;
        s += im.Ss[k];
      }
      sh.Ss[k] = s;
    });
    wg_barrier();
  }
  // ---- the reduced system, thread 0 ----
  if (wg_lead()) {
    bool ok = true;
    const double* T = sh.tot[cur];
    int idx = 0;
    CLC_JT_ROLLED for (int p = 0; p < 6; ++p)
      CLC_JT_ROLLED for (int q = p; q < 6; ++q) {
        const double v = T[idx++] * (sh.scale_c[p] * sh.scale_c[q]);
        sh.Hs[6 * p + q] = v;
        sh.Hs[6 * q + p] = v;
      }
    CLC_JT_ROLLED for (int p = 0; p < 6; ++p) sh.gs_c[p] = T[(E_GC - E_C) + p] * sh.scale_c[p];
    if (sh.move_c) {
      if (!reuse) {
        CLC_JT_ROLLED for (int c = 0; c < 6; ++c) {
          double d = sh.Hs[7 * c];
          d = d > o.min_lm_diagonal ? d : o.min_lm_diagonal;
          d = d < o.max_lm_diagonal ? d : o.max_lm_diagonal;
          sh.diag_c[c] = d;
        }
      }
      CLC_JT_ROLLED for (int i = 0; i < 36; ++i) sh.A[i] = sh.Hs[i];
      CLC_JT_ROLLED for (int c = 0; c < 6; ++c) sh.A[7 * c] += sh.diag_c[c] * inv_radius;
      CLC_JT_ROLLED for (int p = 0; p < 6; ++p) sh.rhs[p] = sh.gs_c[p];
      if (sh.move_i) {
        CLC_JT_ROLLED for (int p = 0; p < 6; ++p) {
          CLC_JT_ROLLED for (int q = 0; q < 6; ++q) sh.A[6 * p + q] -= sh.Ss[p <= q ? tri<6>(p, q) : tri<6>(q, p)];
          sh.rhs[p] -= sh.Ss[21 + p];
        }
      }
      ok = chol_solve<6>(sh.A, sh.rhs, sh.y, sh.L, sh.z);
      CLC_JT_ROLLED for (int p = 0; p < 6; ++p) {
        sh.step_c[p] = -sh.y[p];
        if (!finite_d(sh.y[p])) ok = false;
      }
    } else {
      CLC_JT_ROLLED for (int p = 0; p < 6; ++p) sh.step_c[p] = 0.0;
    }
    sh.step_ok = ok ? 1 : 0;
  }
  wg_barrier();
  // ---- back-substitution and the candidates ----
  each_image(pr.P, [&](long long j) {
    JointImage& im = pr.ws[j];
    if (im.st != CLC_JOINT_OK) return;
    im.red[0] = im.red[1] = im.red[2] = im.red[3] = 0.0;
    if (!sh.move_i || im.red[5] != 0.0 || !sh.step_ok) return;
    bool fin = true;
    CLC_JT_ROLLED for (int p = 0; p < 6; ++p) {
      double s = im.yg[p];
      if (sh.move_c) CLC_JT_ROLLED for (int q = 0; q < 6; ++q) s += im.Y[6 * p + q] * sh.step_c[q];
      im.step[p] = -s;
      fin = fin && finite_d(s);
    }
    if (!fin) { im.red[5] = 1.0; return; }
    double sg = 0.0, shs = 0.0;
    CLC_JT_ROLLED for (int p = 0; p < 6; ++p) {
      sg += im.step[p] * im.gs[p];
      double row = 0.0;
      CLC_JT_ROLLED for (int q = 0; q < 6; ++q) row += im.As[6 * p + q] * im.step[q] + 2.0 * (im.Bs[6 * p + q] * sh.step_c[q]);
      shs += im.step[p] * row;
    }
    im.red[0] = sg;
    im.red[1] = shs;
    double n2;
    im.red[2] = block_candidate(im.x, im.step, im.scale, im.xe, &n2);
    im.red[3] = n2;
  });
  wg_barrier();
  reduce_red(pr, sh);
  wg_barrier();
  if (wg_lead()) {
    bool ok = sh.step_ok && sh.red[5] == 0.0;
    double sg = sh.red[0], shs = sh.red[1], sn = sh.red[2], xn = sh.red[3];
    if (sh.move_c) {
      CLC_JT_ROLLED for (int p = 0; p < 6; ++p) {
        sg += sh.step_c[p] * sh.gs_c[p];
        double row = 0.0;
        CLC_JT_ROLLED for (int q = 0; q < 6; ++q) row += sh.Hs[6 * p + q] * sh.step_c[q];
        shs += sh.step_c[p] * row;
      }
      double n2;
      sn += block_candidate(sh.xc, sh.step_c, sh.scale_c, sh.xce, &n2);
      xn += n2;
    }
    sh.model_cost_change = -(sg + 0.5 * shs);
    sh.red[2] = sn;
    sh.red[3] = xn;
    sh.reuse_diagonal = 1;
    sh.step_ok = (ok && sh.model_cost_change > 0.0) ? 1 : 0;
  }
  wg_barrier();
}

// H_cl = C - sum B_i^T A_i^-1 B_i at the accepted point (undamped, unscaled); with the board poses held, C itself.
CLC_HD void marginal_information(const JointArgs& a, const Problem& pr, JointShared& sh, double* H) {
  const int cur = sh.cur;
  if (sh.move_i) {
    each_image(pr.P, [&](long long j) {
      JointImage& im = pr.ws[j];
      if (im.st != CLC_JOINT_OK) return;
      const double* E = im.E[cur];
      int idx = 0;
      CLC_JT_ROLLED for (int p = 0; p < 6; ++p)
        CLC_JT_ROLLED for (int q = p; q < 6; ++q) {
          const double v = E[E_A + idx++];
          im.Md[6 * p + q] = v;
          im.Md[6 * q + p] = v;
        }
      im.red[5] = 0.0;
      CLC_JT_ROLLED for (int i = 0; i < 27; ++i) im.Ss[i] = 0.0;
      if (!chol_factor6(im.Md, im.L)) { im.red[5] = 1.0; return; }
      schur_share(im, E + E_B);
    });
    wg_barrier();
    each_lane(22, [&](int k) {
      double s = 0.0;
      for (long long j = 0; j < pr.P; ++j) {
        const JointImage& im = pr.ws[j];
        if (im.st != CLC_JOINT_OK) continue;
        s = k < 21 ? s + im.Ss[k] : fmax(s, im.red[5]);
      }
      sh.Ss[k] = s;
    });
    wg_barrier();
  }
  if (wg_lead()) {
    const bool bad = sh.move_i && sh.Ss[21] != 0.0;
    CLC_JT_ROLLED for (int p = 0; p < 6; ++p)
      CLC_JT_ROLLED for (int q = 0; q < 6; ++q) {
        const int k = p <= q ? tri<6>(p, q) : tri<6>(q, p);
        H[6 * p + q] = bad ? __builtin_nan("") : sh.tot[cur][k] - (sh.move_i ? sh.Ss[k] : 0.0);
      }
  }
  wg_barrier();
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

// One problem: every thread of its workgroup calls it (host: once).
CLC_HD void joint_problem(const JointArgs& a, long long pb, JointShared& sh) {
  const clc_options& o = a.opt;
  Problem pr;
  {
    long long i0 = a.prob_off ? a.prob_off[pb] : a.first_image, i1 = a.prob_off ? a.prob_off[pb + 1] : a.first_image + a.n_images;
    if (i0 < a.first_image) i0 = a.first_image;
    if (i1 > a.first_image + a.n_images) i1 = a.first_image + a.n_images;
    pr.i0 = i0;
    pr.P = i1 > i0 ? i1 - i0 : 0;
    pr.ws = a.ws + (i0 - a.first_image);
  }
  // ---- which images take part; their start poses ----
  each_image_wave(pr.P, [&](long long j) {
    const long long img = pr.i0 + j;
    const int st = image_status(a, img);
    if (bf::lead_lane()) {
      JointImage& im = pr.ws[j];
      im.st = st;
      a.status[img] = st;
      if (st == CLC_JOINT_OK) {
        const double w = a.q[4 * img], x = a.q[4 * img + 1], y = a.q[4 * img + 2], z = a.q[4 * img + 3];
        const double inv = 1.0 / sqrt((w * w + x * x) + (y * y + z * z));
        const double p7[7] = {a.t[3 * img], a.t[3 * img + 1], a.t[3 * img + 2], x * inv, y * inv, z * inv, w * inv};
#pragma unroll
        for (int i = 0; i < 7; ++i) im.x[i] = im.xe[i] = p7[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) { im.scale[i] = 1.0; im.diag[i] = 0.0; im.red[i] = 0.0; }
      }
    }
  });
  wg_barrier();
  if (wg_lead()) {
    int n_part = 0;
    long long n_laser = 0;
    double xn = 0.0;
    for (long long j = 0; j < pr.P; ++j) {
      if (pr.ws[j].st != CLC_JOINT_OK) continue;
      ++n_part;
      n_laser += a.poff[pr.i0 + j + 1] - a.poff[pr.i0 + j];
    }
    bool ok = n_part > 0;
    CLC_JT_ROLLED for (int i = 0; i < 7; ++i) {
      const double v = a.poses_cl[7 * pb + i];
      sh.xc[i] = sh.xce[i] = v;
      ok = ok && finite_d(v);
    }
    sh.n_part = n_part;
    sh.n_laser = n_laser;
    sh.move_i = a.hold_board_poses ? 0 : 1;
    sh.move_c = (a.hold_extrinsic || n_laser == 0) ? 0 : 1;
    if (sh.move_i)
      for (long long j = 0; j < pr.P; ++j) {
        if (pr.ws[j].st != CLC_JOINT_OK) continue;
        CLC_JT_ROLLED for (int i = 0; i < 7; ++i) xn += pr.ws[j].x[i] * pr.ws[j].x[i];
      }
    if (sh.move_c) CLC_JT_ROLLED for (int i = 0; i < 7; ++i) xn += sh.xc[i] * sh.xc[i];
    sh.x_norm = sqrt_pos(xn);
    sh.status = ok ? CLC_RUNNING : CLC_FAILURE;
    sh.n_invalid = 0; sh.reuse_diagonal = 0; sh.num_successful = 0; sh.num_unsuccessful = 0; sh.n_trace = 0; sh.n_evals = 0;
    sh.cur = 0; sh.step_ok = 0;
    sh.x_cost = 0.0; sh.initial_cost = 0.0; sh.min_iter_cost = 0.0;
    sh.radius = o.initial_trust_region_radius; sh.decrease_factor = 2.0; sh.model_cost_change = 0.0; sh.gmax = 0.0;
    CLC_JT_ROLLED for (int i = 0; i < 6; ++i) { sh.scale_c[i] = 1.0; sh.diag_c[i] = 0.0; sh.step_c[i] = 0.0; }
    CLC_JT_ROLLED for (int i = 0; i < TOTAL_DOUBLES; ++i) sh.tot[0][i] = sh.tot[1][i] = 0.0;
    sh.it_iteration = 0; sh.it_successful = 1; sh.it_cost = 0.0; sh.it_gmax = 0.0;
  }
  wg_barrier();
  if (sh.status == CLC_RUNNING) {
    // ---- IterationZero ----
    evaluate(a, pr, sh, 0);
    if (wg_lead()) {
      sh.n_evals = 1;
      const double cost = sh.tot[0][E_COST_CORNER - E_C] + sh.tot[0][E_COST_LASER - E_C];
      if (!finite_d(cost)) sh.status = CLC_FAILURE;
      sh.x_cost = sh.initial_cost = sh.min_iter_cost = cost;
      if (o.jacobi_scaling) CLC_JT_ROLLED for (int c = 0; c < 6; ++c) sh.scale_c[c] = 1.0 / (1.0 + sqrt(sh.tot[0][tri<6>(c, c)]));
    }
    if (o.jacobi_scaling)
      each_image(pr.P, [&](long long j) {
        JointImage& im = pr.ws[j];
        if (im.st != CLC_JOINT_OK) return;
        CLC_JT_ROLLED for (int c = 0; c < 6; ++c) im.scale[c] = 1.0 / (1.0 + sqrt(im.E[0][E_A + tri<6>(c, c)]));
      });
    wg_barrier();
  }
  if (sh.status == CLC_RUNNING) {
    gradient_norm(pr, sh);
    if (wg_lead()) { sh.it_cost = sh.x_cost; sh.it_gmax = sh.gmax; }
    wg_barrier();
  }
  // ---- TrustRegionMinimizer::Minimize, as clc_lm.hpp's lm_iterate / lm_advance ----
  // The rule for every word of `sh` that thread 0 writes and the others read (status, step_ok, cur, radius, reuse_diagonal): a barrier
  // lies between any thread's read and thread 0's next write of it, and between that write and the next read.  A thread that read a
  // terminal status early would leave the loop one barrier short of the others.
  while (sh.status == CLC_RUNNING) {
    for (;;) {
      wg_barrier();  // every thread has read sh.status (the loop conditions above and below) before thread 0 may change it
      if (wg_lead()) {
        // FinalizeIterationAndCheckIfMinimizerCanContinue
        if (sh.it_successful) sh.num_successful++; else sh.num_unsuccessful++;
        sh.n_trace++;
        sh.min_iter_cost = sh.it_cost < sh.min_iter_cost ? sh.it_cost : sh.min_iter_cost;
        if (sh.it_iteration >= o.max_num_iterations) sh.status = CLC_NO_CONVERGENCE;
        else if (sh.it_successful && sh.it_gmax <= o.gradient_tolerance) sh.status = CLC_CONVERGENCE_GRADIENT;
        else if (sh.radius <= o.min_trust_region_radius) sh.status = CLC_CONVERGENCE_RADIUS;
        sh.it_iteration++;
        sh.it_successful = 0;
      }
      wg_barrier();
      if (sh.status != CLC_RUNNING) break;
      compute_step(a, pr, sh);
      if (sh.step_ok) {
        if (wg_lead()) sh.n_invalid = 0;
        wg_barrier();
        break;
      }
      wg_barrier();  // (every thread has read step_ok)
      if (wg_lead()) {
        // HandleInvalidStep
        if (++sh.n_invalid >= o.max_num_consecutive_invalid_steps) sh.status = CLC_FAILURE;
        sh.radius = sh.radius / sh.decrease_factor;
        sh.decrease_factor *= 2.0;
        sh.reuse_diagonal = 1;
        sh.it_cost = sh.x_cost;
        sh.it_gmax = sh.gmax;
      }
      wg_barrier();
      if (sh.status != CLC_RUNNING) break;
    }
    if (sh.status != CLC_RUNNING) break;
    // ---- the candidate ----
    evaluate(a, pr, sh, 1 - sh.cur);
    if (wg_lead()) {
      sh.n_evals++;
      const double* T = sh.tot[1 - sh.cur];
      const double cost_e = T[E_COST_CORNER - E_C] + T[E_COST_LASER - E_C];
      const double candidate_cost = finite_d(cost_e) ? cost_e : 1.7976931348623157e308;
      const double step_norm = sqrt_pos(sh.red[2]);
      const double cost_change = sh.x_cost - candidate_cost;
      sh.step_ok = 0;  // from here: 1 = accepted
      if (step_norm <= o.parameter_tolerance * (sh.x_norm + o.parameter_tolerance)) {
        sh.status = CLC_CONVERGENCE_PARAMETER;
      } else if (fabs(cost_change) <= o.function_tolerance * sh.x_cost) {
        sh.status = CLC_CONVERGENCE_FUNCTION;
      } else {
        const double relative_decrease = cost_change * rcp_pos_safe(sh.model_cost_change);
        if (relative_decrease > o.min_relative_decrease) {
          // HandleSuccessfulStep
          sh.step_ok = 1;
          sh.x_norm = sqrt_pos(sh.red[3]);
          sh.x_cost = candidate_cost;
          const double q = 2.0 * relative_decrease - 1.0;
          double den = 1.0 - q * q * q;
          den = den > (1.0 / 3.0) ? den : (1.0 / 3.0);
          sh.radius = sh.radius * rcp_pos(den);
          sh.radius = sh.radius < o.max_trust_region_radius ? sh.radius : o.max_trust_region_radius;
          sh.decrease_factor = 2.0;
          sh.reuse_diagonal = 0;
          sh.it_successful = 1;
          sh.it_cost = candidate_cost;
        } else {
          // HandleUnsuccessfulStep
          sh.radius = sh.radius / sh.decrease_factor;
          sh.decrease_factor *= 2.0;
          sh.reuse_diagonal = 1;
          sh.it_cost = candidate_cost;
          sh.it_gmax = sh.gmax;
        }
      }
    }
    wg_barrier();
    if (sh.status != CLC_RUNNING) break;
    if (sh.step_ok) {
      if (sh.move_i)
        each_image(pr.P, [&](long long j) {
          JointImage& im = pr.ws[j];
          if (im.st != CLC_JOINT_OK) return;
#pragma unroll
          for (int i = 0; i < 7; ++i) im.x[i] = im.xe[i];
        });
      wg_barrier();  // (every thread has read step_ok and cur)
      if (wg_lead()) {
        sh.cur = 1 - sh.cur;
        CLC_JT_ROLLED for (int i = 0; i < 7; ++i) sh.xc[i] = sh.xce[i];
      }
      wg_barrier();
      gradient_norm(pr, sh);
      if (wg_lead()) sh.it_gmax = sh.gmax;
      wg_barrier();
    } else {
      wg_barrier();
    }
  }
  // ---- the outputs: a candidate that was not accepted leaves no trace ----
  wg_barrier();
  const bool failed = sh.status == CLC_FAILURE;
  if (!failed && sh.move_i)
    each_image(pr.P, [&](long long j) {
      const JointImage& im = pr.ws[j];
      if (im.st != CLC_JOINT_OK) return;
      const long long img = pr.i0 + j;
      const double sgn = im.x[6] < 0.0 ? -1.0 : 1.0;
      a.q[4 * img] = sgn * im.x[6];
      a.q[4 * img + 1] = sgn * im.x[3];
      a.q[4 * img + 2] = sgn * im.x[4];
      a.q[4 * img + 3] = sgn * im.x[5];
#pragma unroll
      for (int i = 0; i < 3; ++i) a.t[3 * img + i] = im.x[i];
    });
  if (wg_lead()) {
    clc_summary sm;
    cp::summary_empty(sm);
    sm.termination = sh.status;
    if (sh.n_evals > 0) {
      sm.num_iterations = sh.n_trace > 0 ? sh.n_trace - 1 : 0;
      sm.num_successful_steps = sh.num_successful;
      sm.num_unsuccessful_steps = sh.num_unsuccessful;
      sm.num_evaluations = sh.n_evals;
      sm.initial_cost = sh.initial_cost;
      sm.final_cost = sh.x_cost;
    }
    a.summaries[pb] = sm;
    if (!failed && sh.move_c) CLC_JT_ROLLED for (int i = 0; i < 7; ++i) a.poses_cl[7 * pb + i] = sh.xc[i];
    if (a.cost_parts) {
      const bool have = sh.n_evals > 0 && !failed;
      a.cost_parts[2 * pb] = have ? sh.tot[sh.cur][E_COST_CORNER - E_C] : __builtin_nan("");
      a.cost_parts[2 * pb + 1] = have ? sh.tot[sh.cur][E_COST_LASER - E_C] : __builtin_nan("");
    }
  }
  if (a.H_cl) {
    if (!failed && sh.n_evals > 0) {
      marginal_information(a, pr, sh, a.H_cl + 36 * pb);
    } else if (wg_lead()) {
      CLC_JT_ROLLED for (int i = 0; i < 36; ++i) a.H_cl[36 * pb + i] = __builtin_nan("");
    }
  }
}

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
