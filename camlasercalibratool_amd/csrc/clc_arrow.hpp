// clc_arrow.hpp — the Levenberg-Marquardt solve of one "arrow" problem, written once for the five problems K18 (clc_joint.hpp), K19
// (clc_camcal.hpp), K21 (clc_laserrange.hpp), K22 and K23, and the bookkeeping of a shared block that their traits have in common.
// A leaf: it holds no kernel.  The kernels live one per unit, each held to its own register figures; what they share is inline code
// here and, for the terms of the four joint problems, in clc_jointterms.hpp.
//
// The unknowns are the tangent [dt, dtheta] of every board pose (Se3Manifold: t += dt, R <- R Exp(dtheta)) and one shared block of NC
// parameters.  The normal matrix is an arrow: a 6x6 block A_i per image, coupled through B_i (6 x NC) only to the NC x NC block C of
// the shared parameters; the Schur complement over the images leaves an NC x NC system.
//
//   arrow_problem<T>   one 256-thread workgroup (4 waves) per problem, the whole solve in one launch.
//     evaluation   the waves take the images round-robin; T::eval_image fills the image's record E (ArrowRecord<NC>: A_i, B_i, g_i
//                  and the image's share of C, g_c and of the cost parts).  The shares are then added over the images in image order,
//                  one entry per lane.
//     step         one image per lane: the scaled, damped A_i + D_i factored, Y_i = (A_i + D_i)^-1 B_i, S_i = B_i^T Y_i,
//                  s_i = B_i^T (A_i + D_i)^-1 g_i; S and s added over the images in image order; thread 0 solves the reduced system
//                  (T::solve_block) for delta_c; the lanes back-substitute delta_i = -(A_i + D_i)^-1 (g_i + B_i delta_c).
//                  A rejected step repeats only this with the new radius: the blocks of the accepted point are kept.
//     controller   thread 0, state in LDS (ArrowControl): the semantics of clc_lm.hpp (Jacobi scaling fixed at the first evaluation
//                  over all NC + 6P columns, the diagonal clamp, the radius rule, the three tolerances, the iteration cap), written
//                  over the arrow.
//   Per-image state (ArrowImage) lives in a workspace in device memory indexed by image: any number of images fits, and every access
//   goes through pointers, so the per-lane 6x6 algebra needs no private arrays (no scratch).  Every sum has a fixed shape (butterflies
//   within a wave, image order across images): no atomics, the same bits on every run, and a problem never reads another problem's
//   state.
//
// The traits T of a problem are static CLC_HD functions (no function pointers), what genuinely differs between the problems:
//   NC, EVAL_DOUBLES, Args, Shared (derives ArrowShared<NC, EVAL_DOUBLES>), Ctx
//   problem(a, pb)                    the image range and workspace of problem pb
//   image_status(a, img)              why an image takes no part (wave-uniform), CLC_JOINT_* / CLC_CAMCAL_*
//   observations(a, img)              what the problem counts per participating image (laser points / corners)
//   context(sh, ctx), eval_image(a, ctx, img, pose7, E)      the shared block at its candidate, prepared once per evaluation
//   init_block(a, pb, n_obs, sh, xn)  the shared block's start into sh, sh.move_c, its share of |x|^2 added to xn; false: no start
//   held(a, p)                        parameter p of the shared block does not move (scale 0, its rows and columns of H zero)
//   cost(tot)                         the cost of a row of totals
//   block_gradient(sh, m)             max(m, the shared block's gradient max norm)
//   solve_block(sh)                   sh.A delta = sh.rhs -> sh.step_c = -delta; false if not positive definite or not finite
//   block_candidate(sh, sn, xn)       the shared block's candidate from sh.step_c; adds |x - xe|^2 to sn and |xe|^2 to xn
//   accept_block(sh)                  the candidate becomes the accepted block
//   information(a)                    where the marginal information of the shared blocks goes, [NC x NC] per problem (nullable)
//   write_outputs(a, pb, sh, failed)  the problem's own outputs (thread 0)
// What several traits do the same way stands below block_candidate, once: problem_range (the clamp of a problem's images), T_cl as
// the leading six of a shared block (tcl_*), the cost in two parts and its cost_parts, the shares of an additive parameter's
// candidate, the list of free parameters, and the reduced system compacted to them, solved (chol_solve<N> by the caller's switch, or
// chol_solve_n at run-time n) and scattered into step_c.
//
// Everything numeric is CLC_HD: the shims of tests/shim (joint, camcal and the three later problems') compile this header for the
// host with g++ and run the same code with the threads as loops, in the same summation order.
#pragma once
#include "clc_campose.hpp"

namespace clc {
namespace aw {

constexpr int ARROW_THREADS = 256;
constexpr int ARROW_WAVES = ARROW_THREADS / 64;

#if defined(__HIP_DEVICE_COMPILE__)
#define CLC_AW_ROLLED _Pragma("nounroll")
#else
#define CLC_AW_ROLLED
#endif

// The status of an image that takes part; the two problems' constants are the same numbers.
constexpr int IMAGE_OK = CLC_JOINT_OK;
static_assert(CLC_JOINT_OK == CLC_CAMCAL_OK && CLC_JOINT_TOO_FEW == CLC_CAMCAL_TOO_FEW && CLC_JOINT_NOT_KEPT == CLC_CAMCAL_NOT_KEPT &&
                  CLC_JOINT_NONFINITE == CLC_CAMCAL_NONFINITE,
              "the image status of K18 and K19 is one enumeration");

// Offsets into an evaluation record E of one image: A tri<6>, B[NC p + q] (pose row p, shared column q), g_i, C tri<NC>, g_c, then
// the problem's cost parts.  The totals over the images are the record from E_C on.
template <int NC>
struct ArrowRecord {
  static constexpr int TRI = NC * (NC + 1) / 2;  // C, S_i
  static constexpr int SS = TRI + NC;            // S_i and s_i
  static constexpr int E_A = 0, E_B = 21, E_G = E_B + 6 * NC, E_C = E_G + 6, E_GC = E_C + TRI, E_COST = E_GC + NC;
};

template <int NC, int EVAL_DOUBLES>
struct ArrowImage {
  double x[7], xe[7];            // accepted pose, pose the next evaluation uses: [t, qx, qy, qz, qw]
  double E[2][EVAL_DOUBLES];     // the blocks at the accepted point (sh.cur) and at the candidate
  double scale[6], diag[6];      // Jacobi scaling, clamped diagonal of the scaled A
  double As[36], Md[36], L[36];  // scaled A, scaled damped A, its Cholesky factor (inverse diagonal)
  double Bs[6 * NC], Y[6 * NC];  // scaled B, (A + D)^-1 B
  double gs[6], yg[6], z[6];     // scaled g, (A + D)^-1 g, substitution scratch
  double Ss[ArrowRecord<NC>::SS];  // S_i (tri<NC> order) and s_i
  double step[6];                // delta_i in the scaled space
  double red[6];                 // shares: step.g, step^T H step, |x - xe|^2, |xe|^2, gradient max norm, bad-step flag
  int32_t st;                    // CLC_JOINT_* / CLC_CAMCAL_*
  int32_t pad_;
};

// The controller's state, thread 0 writes it.
struct ArrowControl {
  double x_cost, x_norm, initial_cost, min_iter_cost, radius, decrease_factor, model_cost_change, gmax;
  double it_cost, it_gmax;
  long long n_evals;
  int32_t status, n_invalid, reuse_diagonal, num_successful, num_unsuccessful, n_trace, cur, step_ok, move_c, move_i, n_part;
  int32_t it_iteration, it_successful;
};

// The workgroup's state of one problem (LDS): the controller and the shared block's side of the step.
template <int NC, int EVAL_DOUBLES>
struct ArrowShared : ArrowControl {
  double tot[2][EVAL_DOUBLES - ArrowRecord<NC>::E_C];
  double scale_c[NC], diag_c[NC], step_c[NC], gs_c[NC], rhs[NC];
  double Ss[ArrowRecord<NC>::SS], red[6];
  double Hs[NC * NC], A[NC * NC], L[NC * NC], z[NC];
};

template <class Image>
struct Problem {
  long long i0, P;  // first image (absolute), images
  Image* ws;        // image i0 first
};

// ---- the workgroup of one problem; on the host the threads are loops ----
template <class F>
CLC_HD void each_image(long long P, F f) {  // one image per thread
#if defined(__HIP_DEVICE_COMPILE__)
  for (long long j = threadIdx.x; j < P; j += ARROW_THREADS) f(j);
#else
  for (long long j = 0; j < P; ++j) f(j);
#endif
}
template <class F>
CLC_HD void each_image_wave(long long P, F f) {  // the waves take the images round-robin
#if defined(__HIP_DEVICE_COMPILE__)
  for (long long j = threadIdx.x >> 6; j < P; j += ARROW_WAVES) f(j);
#else
  for (long long j = 0; j < P; ++j) f(j);
#endif
}
template <class F>
CLC_HD void each_lane(int K, F f) {  // K <= ARROW_THREADS entries, one per thread
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

// The factor of chol_solve (clc_math.hpp): L with the inverse diagonal.  false if a pivot is not positive.
CLC_HD bool chol_factor6(const double* A, double* L) {
  CLC_AW_ROLLED for (int j = 0; j < 6; ++j) {
    double d = A[6 * j + j];
    CLC_AW_ROLLED for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k];
    if (!(d > 0.0)) return false;
    const double inv = rsqrt_pos(d);
    L[6 * j + j] = inv;
    CLC_AW_ROLLED for (int i = j + 1; i < 6; ++i) {
      double s = A[6 * i + j];
      CLC_AW_ROLLED for (int k = 0; k < j; ++k) s -= L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = s * inv;
    }
  }
  return true;
}

// y = (L L^T)^-1 b, b and y strided; z[6] scratch.
CLC_HD void chol_apply6(const double* L, const double* b, int bs, double* y, int ys, double* z) {
  CLC_AW_ROLLED for (int i = 0; i < 6; ++i) {
    double s = b[bs * i];
    CLC_AW_ROLLED for (int k = 0; k < i; ++k) s -= L[6 * i + k] * z[k];
    z[i] = s * L[6 * i + i];
  }
  CLC_AW_ROLLED for (int i = 5; i >= 0; --i) {
    double s = z[i];
    CLC_AW_ROLLED for (int k = i + 1; k < 6; ++k) s -= L[6 * k + i] * y[ys * k];
    y[ys * i] = s * L[6 * i + i];
  }
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

// ---- what the problems' traits have in common -----------------------------------------------------------------------------
// [first image, images) of problem pb and its workspace, clamped to the call's images [first, first + n_images); ws: image `first`
// first.
template <class Image>
CLC_HD Problem<Image> problem_range(const long long* prob_off, long long pb, long long first, long long n_images, Image* ws) {
  long long i0 = prob_off ? prob_off[pb] : first, i1 = prob_off ? prob_off[pb + 1] : first + n_images;
  if (i0 < first) i0 = first;
  if (i1 > first + n_images) i1 = first + n_images;
  return {i0, i1 > i0 ? i1 - i0 : 0, ws + (i0 - first)};
}

// A cost in two parts (corners, laser) behind the record of ArrowRecord<NC>: the cost of a row of totals, and the problem's
// cost_parts[2] (nullable; NaN without an evaluation or after a failure).
template <int NC>
CLC_HD double cost_of_parts(const double* tot) {
  using R = ArrowRecord<NC>;
  return tot[R::E_COST - R::E_C] + tot[R::E_COST + 1 - R::E_C];
}
template <int NC, class Sh>
CLC_HD void write_cost_parts(double* cost_parts, long long pb, const Sh& sh, bool failed) {
  using R = ArrowRecord<NC>;
  if (!cost_parts) return;
  const bool have = sh.n_evals > 0 && !failed;
  cost_parts[2 * pb] = have ? sh.tot[sh.cur][R::E_COST - R::E_C] : __builtin_nan("");
  cost_parts[2 * pb + 1] = have ? sh.tot[sh.cur][R::E_COST + 1 - R::E_C] : __builtin_nan("");
}

// T_cl as the leading six of a shared block; Sh holds it as xc[7] (accepted) and xce[7] (to evaluate), Ctx as Rcl[9], tcl[3].
template <class Sh>
CLC_HD bool tcl_init(const double* pose_cl, Sh& sh) {  // false: not finite
  bool ok = true;
  CLC_AW_ROLLED for (int i = 0; i < 7; ++i) {
    const double v = pose_cl[i];
    sh.xc[i] = sh.xce[i] = v;
    ok = ok && finite_d(v);
  }
  return ok;
}
template <class Sh, class Ctx>
CLC_HD void tcl_context(const Sh& sh, Ctx& c) {
  double q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = sh.xce[3 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) c.tcl[i] = sh.xce[i];
  quat_to_rot(q, c.Rcl);
}
template <class Sh>
CLC_HD void tcl_candidate(Sh& sh, bool hold, double& sn, double& xn) {
  double n2 = 0.0;
  if (!hold) {
    sn += block_candidate(sh.xc, sh.step_c, sh.scale_c, sh.xce, &n2);
  } else {  // a held T_cl keeps its bits
    CLC_AW_ROLLED for (int i = 0; i < 7; ++i) {
      sh.xce[i] = sh.xc[i];
      n2 += sh.xc[i] * sh.xc[i];
    }
  }
  xn += n2;
}
template <class Sh>
CLC_HD void tcl_accept(Sh& sh) {
  CLC_AW_ROLLED for (int i = 0; i < 7; ++i) sh.xc[i] = sh.xce[i];
}
template <int NC, class Sh>
CLC_HD double tcl_gradient(const Sh& sh, double m) {
  return fmax(m, block_gradient_norm(sh.xc, sh.tot[sh.cur] + (ArrowRecord<NC>::E_GC - ArrowRecord<NC>::E_C)));
}

// An additive parameter of a shared block moved from x to its candidate v (a held one keeps its bits: v = x): its shares of
// |x - xe|^2 and |xe|^2.  Returns v.
CLC_HD double additive_candidate(double x, double v, double& sn, double& xn) {
  sn += (x - v) * (x - v);
  xn += v * v;
  return v;
}

// The free parameters of a shared block, Sh holds them as free_idx[NC] (ascending, the rest 0): returns how many.
template <int NC, class F>
CLC_HD int free_parameters(int32_t* free_idx, F is_free) {
  int nf = 0;
  CLC_AW_ROLLED for (int i = 0; i < NC; ++i) {
    free_idx[i] = 0;
    if (is_free(i)) free_idx[nf++] = i;
  }
  return nf;
}

// max(m, the gradient max norm over the free additive parameters from index `from` on)
template <int NC, class Sh>
CLC_HD double free_gradient(const Sh& sh, int from, double m) {
  CLC_AW_ROLLED for (int f = 0; f < sh.n_free; ++f)
    if (sh.free_idx[f] >= from) m = fmax(m, fabs(sh.tot[sh.cur][(ArrowRecord<NC>::E_GC - ArrowRecord<NC>::E_C) + sh.free_idx[f]]));
  return m;
}

// The reduced system sh.A / sh.rhs without the rows and columns of the held parameters: sh.Af (n x n), sh.rf.
template <int NC, class Sh>
CLC_HD void compact_free(Sh& sh, int n) {
  CLC_AW_ROLLED for (int p = 0; p < n; ++p) {
    CLC_AW_ROLLED for (int q = 0; q < n; ++q) sh.Af[n * p + q] = sh.A[NC * sh.free_idx[p] + sh.free_idx[q]];
    sh.rf[p] = sh.rhs[sh.free_idx[p]];
  }
}
// ... solved with chol_solve at N free parameters: sh.yf[0..N)
template <int NC, int N, class Sh>
CLC_HD bool solve_free(Sh& sh) {
  compact_free<NC>(sh, N);
  return chol_solve<N>(sh.Af, sh.rf, sh.yf, sh.L, sh.z);
}
// ... and -sh.yf scattered into sh.step_c; false if `ok` is or a component is not finite.
template <class Sh>
CLC_HD bool scatter_free(Sh& sh, bool ok) {
  CLC_AW_ROLLED for (int f = 0; f < sh.n_free; ++f) {
    sh.step_c[sh.free_idx[f]] = -sh.yf[f];
    if (!finite_d(sh.yf[f])) ok = false;
  }
  return ok;
}

// Y = M^-1 B (6 x NC) and S = B^T Y (tri<NC> order) of one image, from im.L.
template <class T>
CLC_HD void schur_share(typename T::Image& im, const double* B) {
  constexpr int NC = T::NC;
  CLC_AW_ROLLED for (int b = 0; b < NC; ++b) chol_apply6(im.L, B + b, NC, im.Y + b, NC, im.z);
  int idx = 0;
  CLC_AW_ROLLED for (int p = 0; p < NC; ++p)
    CLC_AW_ROLLED for (int q = p; q < NC; ++q) {
      double s = 0.0;
      CLC_AW_ROLLED for (int k = 0; k < 6; ++k) s += B[NC * k + p] * im.Y[NC * k + q];
      im.Ss[idx++] = s;
    }
}

// Adds the images' shares in image order: sh.red (sums of 0..3, maxima of 4..5).
template <class T>
CLC_HD void reduce_red(const Problem<typename T::Image>& pr, typename T::Shared& sh) {
  each_lane(6, [&](int k) {
    double s = 0.0;
    for (long long j = 0; j < pr.P; ++j) {
      const typename T::Image& im = pr.ws[j];
      if (im.st != IMAGE_OK) continue;
      s = k < 4 ? s + im.red[k] : fmax(s, im.red[k]);
    }
    sh.red[k] = s;
  });
}

// Evaluates every participating image at its xe and the shared block at its candidate into record `set`; the totals into sh.tot[set].
template <class T>
CLC_HD void evaluate(const typename T::Args& a, const Problem<typename T::Image>& pr, typename T::Shared& sh, int set) {
  using R = ArrowRecord<T::NC>;
  typename T::Ctx ctx;
  T::context(sh, ctx);
  each_image_wave(pr.P, [&](long long j) {
    typename T::Image& im = pr.ws[j];
    if (im.st != IMAGE_OK) return;
    T::eval_image(a, ctx, pr.i0 + j, im.xe, im.E[set]);
  });
  wg_barrier();
  each_lane(T::EVAL_DOUBLES - R::E_C, [&](int k) {
    double s = 0.0;
    for (long long j = 0; j < pr.P; ++j) {
      const typename T::Image& im = pr.ws[j];
      if (im.st != IMAGE_OK) continue;
      s += im.E[set][R::E_C + k];
    }
    sh.tot[set][k] = s;
  });
  wg_barrier();
}

// The gradient max norm over the moving blocks at the accepted point (record sh.cur) -> sh.gmax.
template <class T>
CLC_HD void gradient_norm(const Problem<typename T::Image>& pr, typename T::Shared& sh) {
  each_image(pr.P, [&](long long j) {
    typename T::Image& im = pr.ws[j];
    if (im.st != IMAGE_OK) return;
    im.red[4] = sh.move_i ? block_gradient_norm(im.x, im.E[sh.cur] + ArrowRecord<T::NC>::E_G) : 0.0;
    im.red[5] = 0.0;
  });
  wg_barrier();
  reduce_red<T>(pr, sh);
  wg_barrier();
  if (wg_lead()) sh.gmax = T::block_gradient(sh, sh.red[4]);
  wg_barrier();
}

// The trust-region step at the accepted point for sh.radius: every image's xe and the shared block's candidate are set, sh.step_ok
// says whether the step is valid (LevenbergMarquardtStrategy::ComputeStep + the model-cost test, over the arrow).
template <class T>
CLC_HD void compute_step(const typename T::Args& a, const Problem<typename T::Image>& pr, typename T::Shared& sh) {
  constexpr int NC = T::NC;
  using R = ArrowRecord<NC>;
  const clc_options& o = a.opt;
  const double inv_radius = rcp_pos(sh.radius);
  const int reuse = sh.reuse_diagonal, cur = sh.cur;
  if (sh.move_i) {
    each_image(pr.P, [&](long long j) {
      typename T::Image& im = pr.ws[j];
      if (im.st != IMAGE_OK) return;
      const double* E = im.E[cur];
      int idx = 0;
      CLC_AW_ROLLED for (int p = 0; p < 6; ++p)
        CLC_AW_ROLLED for (int q = p; q < 6; ++q) {
          const double v = E[R::E_A + idx++] * (im.scale[p] * im.scale[q]);
          im.As[6 * p + q] = v;
          im.As[6 * q + p] = v;
        }
      if (!reuse) {
        CLC_AW_ROLLED for (int c = 0; c < 6; ++c) {
          double d = im.As[7 * c];
          d = d > o.min_lm_diagonal ? d : o.min_lm_diagonal;
          d = d < o.max_lm_diagonal ? d : o.max_lm_diagonal;
          im.diag[c] = d;
        }
      }
      CLC_AW_ROLLED for (int i = 0; i < 36; ++i) im.Md[i] = im.As[i];
      CLC_AW_ROLLED for (int c = 0; c < 6; ++c) im.Md[7 * c] += im.diag[c] * inv_radius;
      CLC_AW_ROLLED for (int p = 0; p < 6; ++p) im.gs[p] = E[R::E_G + p] * im.scale[p];
      CLC_AW_ROLLED for (int p = 0; p < 6; ++p)
        CLC_AW_ROLLED for (int q = 0; q < NC; ++q) im.Bs[NC * p + q] = E[R::E_B + NC * p + q] * (im.scale[p] * sh.scale_c[q]);
      im.red[5] = 0.0;
      CLC_AW_ROLLED for (int i = 0; i < R::SS; ++i) im.Ss[i] = 0.0;
      if (!chol_factor6(im.Md, im.L)) { im.red[5] = 1.0; return; }
      chol_apply6(im.L, im.gs, 1, im.yg, 1, im.z);
      if (sh.move_c) {
        schur_share<T>(im, im.Bs);
        CLC_AW_ROLLED for (int p = 0; p < NC; ++p) {
          double s = 0.0;
          CLC_AW_ROLLED for (int k = 0; k < 6; ++k) s += im.Bs[NC * k + p] * im.yg[k];
          im.Ss[R::TRI + p] = s;
        }
      }
    });
    wg_barrier();
    each_lane(R::SS, [&](int k) {
      double s = 0.0;
      for (long long j = 0; j < pr.P; ++j) {
        const typename T::Image& im = pr.ws[j];
        if (im.st != IMAGE_OK) continue;
        s += im.Ss[k];
      }
      sh.Ss[k] = s;
    });
    wg_barrier();
  }
  // ---- the reduced system, thread 0 ----
  if (wg_lead()) {
    bool ok = true;
    const double* Tc = sh.tot[cur];
    int idx = 0;
    CLC_AW_ROLLED for (int p = 0; p < NC; ++p)
      CLC_AW_ROLLED for (int q = p; q < NC; ++q) {
        const double v = Tc[idx++] * (sh.scale_c[p] * sh.scale_c[q]);
        sh.Hs[NC * p + q] = v;
        sh.Hs[NC * q + p] = v;
      }
    CLC_AW_ROLLED for (int p = 0; p < NC; ++p) { sh.step_c[p] = 0.0; sh.gs_c[p] = sh.rhs[p] = Tc[(R::E_GC - R::E_C) + p] * sh.scale_c[p]; }
    if (sh.move_c) {
      if (!reuse) {
        CLC_AW_ROLLED for (int c = 0; c < NC; ++c) {
          double d = sh.Hs[(NC + 1) * c];
          d = d > o.min_lm_diagonal ? d : o.min_lm_diagonal;
          d = d < o.max_lm_diagonal ? d : o.max_lm_diagonal;
          sh.diag_c[c] = d;
        }
      }
      CLC_AW_ROLLED for (int i = 0; i < NC * NC; ++i) sh.A[i] = sh.Hs[i];
      CLC_AW_ROLLED for (int c = 0; c < NC; ++c) sh.A[(NC + 1) * c] += sh.diag_c[c] * inv_radius;
      if (sh.move_i) {
        CLC_AW_ROLLED for (int p = 0; p < NC; ++p) {
          CLC_AW_ROLLED for (int q = 0; q < NC; ++q) sh.A[NC * p + q] -= sh.Ss[p <= q ? tri<NC>(p, q) : tri<NC>(q, p)];
          sh.rhs[p] -= sh.Ss[R::TRI + p];
        }
      }
      ok = T::solve_block(sh);
    }
    sh.step_ok = ok ? 1 : 0;
  }
  wg_barrier();
  // ---- back-substitution and the candidates ----
  each_image(pr.P, [&](long long j) {
    typename T::Image& im = pr.ws[j];
    if (im.st != IMAGE_OK) return;
    im.red[0] = im.red[1] = im.red[2] = im.red[3] = 0.0;
    if (!sh.move_i || im.red[5] != 0.0 || !sh.step_ok) return;
    bool fin = true;
    CLC_AW_ROLLED for (int p = 0; p < 6; ++p) {
      double s = im.yg[p];
      if (sh.move_c) CLC_AW_ROLLED for (int q = 0; q < NC; ++q) s += im.Y[NC * p + q] * sh.step_c[q];
      im.step[p] = -s;
      fin = fin && finite_d(s);
    }
    if (!fin) { im.red[5] = 1.0; return; }
    double sg = 0.0, shs = 0.0;
    CLC_AW_ROLLED for (int p = 0; p < 6; ++p) {
      sg += im.step[p] * im.gs[p];
      double row = 0.0;
      CLC_AW_ROLLED for (int q = 0; q < 6; ++q) row += im.As[6 * p + q] * im.step[q];
      if (sh.move_c) {  // (unrolled: the row's NC loads of Bs are in flight together)
#pragma unroll
        for (int q = 0; q < NC; ++q) row += 2.0 * (im.Bs[NC * p + q] * sh.step_c[q]);
      }
      shs += im.step[p] * row;
    }
    im.red[0] = sg;
    im.red[1] = shs;
    double n2;
    im.red[2] = block_candidate(im.x, im.step, im.scale, im.xe, &n2);
    im.red[3] = n2;
  });
  wg_barrier();
  reduce_red<T>(pr, sh);
  wg_barrier();
  if (wg_lead()) {
    bool ok = sh.step_ok && sh.red[5] == 0.0;
    double sg = sh.red[0], shs = sh.red[1], sn = sh.red[2], xn = sh.red[3];
    if (sh.move_c) {
      CLC_AW_ROLLED for (int p = 0; p < NC; ++p) {
        sg += sh.step_c[p] * sh.gs_c[p];
        double row = 0.0;
        CLC_AW_ROLLED for (int q = 0; q < NC; ++q) row += sh.Hs[NC * p + q] * sh.step_c[q];
        shs += sh.step_c[p] * row;
      }
      T::block_candidate(sh, sn, xn);
    }
    sh.model_cost_change = -(sg + 0.5 * shs);
    sh.red[2] = sn;
    sh.red[3] = xn;
    sh.reuse_diagonal = 1;
    sh.step_ok = (ok && sh.model_cost_change > 0.0) ? 1 : 0;
  }
  wg_barrier();
}

// H = C - sum B_i^T A_i^-1 B_i at the accepted point (undamped, unscaled), rows and columns of held parameters zero; with the board
// poses held, C itself; NaN where an A_i is not positive definite.
template <class T>
CLC_HD void marginal_information(const typename T::Args& a, const Problem<typename T::Image>& pr, typename T::Shared& sh, double* H) {
  constexpr int NC = T::NC;
  using R = ArrowRecord<NC>;
  const int cur = sh.cur;
  if (sh.move_i) {
    each_image(pr.P, [&](long long j) {
      typename T::Image& im = pr.ws[j];
      if (im.st != IMAGE_OK) return;
      const double* E = im.E[cur];
      int idx = 0;
      CLC_AW_ROLLED for (int p = 0; p < 6; ++p)
        CLC_AW_ROLLED for (int q = p; q < 6; ++q) {
          const double v = E[R::E_A + idx++];
          im.Md[6 * p + q] = v;
          im.Md[6 * q + p] = v;
        }
      im.red[5] = 0.0;
      CLC_AW_ROLLED for (int i = 0; i < R::SS; ++i) im.Ss[i] = 0.0;
      if (!chol_factor6(im.Md, im.L)) { im.red[5] = 1.0; return; }
      schur_share<T>(im, E + R::E_B);
    });
    wg_barrier();
    each_lane(R::TRI + 1, [&](int k) {
      double s = 0.0;
      for (long long j = 0; j < pr.P; ++j) {
        const typename T::Image& im = pr.ws[j];
        if (im.st != IMAGE_OK) continue;
        s = k < R::TRI ? s + im.Ss[k] : fmax(s, im.red[5]);
      }
      sh.Ss[k] = s;
    });
    wg_barrier();
  }
  if (wg_lead()) {
    const bool bad = sh.move_i && sh.Ss[R::TRI] != 0.0;
    CLC_AW_ROLLED for (int p = 0; p < NC; ++p)
      CLC_AW_ROLLED for (int q = 0; q < NC; ++q) {
        const int k = p <= q ? tri<NC>(p, q) : tri<NC>(q, p);
        const bool held = T::held(a, p) || T::held(a, q);
        H[NC * p + q] = held ? 0.0 : bad ? __builtin_nan("") : sh.tot[cur][k] - (sh.move_i ? sh.Ss[k] : 0.0);
      }
  }
  wg_barrier();
}

// One problem: every thread of its workgroup calls it (host: once).
template <class T>
CLC_HD void arrow_problem(const typename T::Args& a, long long pb, typename T::Shared& sh) {
  constexpr int NC = T::NC;
  using R = ArrowRecord<NC>;
  using Image = typename T::Image;
  const clc_options& o = a.opt;
  const Problem<Image> pr = T::problem(a, pb);
  // ---- which images take part; their start poses ----
  each_image_wave(pr.P, [&](long long j) {
    const long long img = pr.i0 + j;
    const int st = T::image_status(a, img);
    if (bf::lead_lane()) {
      Image& im = pr.ws[j];
      im.st = st;
      a.status[img] = st;
      if (st == IMAGE_OK) {
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
    long long n_obs = 0;
    double xn = 0.0;
    for (long long j = 0; j < pr.P; ++j) {
      if (pr.ws[j].st != IMAGE_OK) continue;
      ++n_part;
      n_obs += T::observations(a, pr.i0 + j);
    }
    sh.n_part = n_part;
    sh.move_i = a.hold_board_poses ? 0 : 1;
    if (sh.move_i)
      for (long long j = 0; j < pr.P; ++j) {
        if (pr.ws[j].st != IMAGE_OK) continue;
        CLC_AW_ROLLED for (int i = 0; i < 7; ++i) xn += pr.ws[j].x[i] * pr.ws[j].x[i];
      }
    const bool ok = T::init_block(a, pb, n_obs, sh, xn) && n_part > 0;
    sh.x_norm = sqrt_pos(xn);
    sh.status = ok ? CLC_RUNNING : CLC_FAILURE;
    sh.n_invalid = 0; sh.reuse_diagonal = 0; sh.num_successful = 0; sh.num_unsuccessful = 0; sh.n_trace = 0; sh.n_evals = 0;
    sh.cur = 0; sh.step_ok = 0;
    sh.x_cost = 0.0; sh.initial_cost = 0.0; sh.min_iter_cost = 0.0;
    sh.radius = o.initial_trust_region_radius; sh.decrease_factor = 2.0; sh.model_cost_change = 0.0; sh.gmax = 0.0;
    CLC_AW_ROLLED for (int i = 0; i < NC; ++i) {
      sh.scale_c[i] = T::held(a, i) ? 0.0 : 1.0;
      sh.diag_c[i] = 0.0;
      sh.step_c[i] = 0.0;
    }
    CLC_AW_ROLLED for (int i = 0; i < T::EVAL_DOUBLES - R::E_C; ++i) sh.tot[0][i] = sh.tot[1][i] = 0.0;
    sh.it_iteration = 0; sh.it_successful = 1; sh.it_cost = 0.0; sh.it_gmax = 0.0;
  }
  wg_barrier();
  if (sh.status == CLC_RUNNING) {
    // ---- IterationZero ----
    evaluate<T>(a, pr, sh, 0);
    if (wg_lead()) {
      sh.n_evals = 1;
      const double cost = T::cost(sh.tot[0]);
      if (!finite_d(cost)) sh.status = CLC_FAILURE;
      sh.x_cost = sh.initial_cost = sh.min_iter_cost = cost;
      if (o.jacobi_scaling)
        CLC_AW_ROLLED for (int c = 0; c < NC; ++c)
          if (sh.scale_c[c] != 0.0) sh.scale_c[c] = 1.0 / (1.0 + sqrt(sh.tot[0][tri<NC>(c, c)]));
    }
    if (o.jacobi_scaling)
      each_image(pr.P, [&](long long j) {
        Image& im = pr.ws[j];
        if (im.st != IMAGE_OK) return;
        CLC_AW_ROLLED for (int c = 0; c < 6; ++c) im.scale[c] = 1.0 / (1.0 + sqrt(im.E[0][R::E_A + tri<6>(c, c)]));
      });
    wg_barrier();
  }
  if (sh.status == CLC_RUNNING) {
    gradient_norm<T>(pr, sh);
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
      compute_step<T>(a, pr, sh);
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
    evaluate<T>(a, pr, sh, 1 - sh.cur);
    if (wg_lead()) {
      sh.n_evals++;
      const double cost_e = T::cost(sh.tot[1 - sh.cur]);
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
          Image& im = pr.ws[j];
          if (im.st != IMAGE_OK) return;
#pragma unroll
          for (int i = 0; i < 7; ++i) im.x[i] = im.xe[i];
        });
      wg_barrier();  // (every thread has read step_ok and cur)
      if (wg_lead()) {
        sh.cur = 1 - sh.cur;
        T::accept_block(sh);
      }
      wg_barrier();
      gradient_norm<T>(pr, sh);
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
      const Image& im = pr.ws[j];
      if (im.st != IMAGE_OK) return;
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
    T::write_outputs(a, pb, sh, failed);
  }
  if (double* H = T::information(a)) {
    if (!failed && sh.n_evals > 0) {
      marginal_information<T>(a, pr, sh, H + NC * NC * pb);
    } else if (wg_lead()) {
      CLC_AW_ROLLED for (int i = 0; i < NC * NC; ++i) H[NC * NC * pb + i] = __builtin_nan("");
    }
  }
}

}  // namespace aw
}  // namespace clc
