// clc_laserrange.hpp — K21: K18's joint refinement with the scanner's own two parameters.  The measured point p (laser frame) is
// corrected along its ray,
//
//   p' = (1 + kappa + b / |p|) p          true range = (1 + kappa) measured + b;  b: range offset (metres), kappa: range scale
//
// and the cost is K18's with p' in place of p:
//
//   1/2 sum |((R_i X + t_i)_xy / (R_i X + t_i)_z - x_lifted) / sigma_corner|^2  +  1/2 sum (e3^T R_i^T (R_cl p' + t_cl - t_i) / sigma_laser)^2
//
// The arrow of clc_arrow.hpp with an 8-wide shared block [dt_cl, dtheta_cl, b, kappa]: T_cl moves on its tangent as in K18, b and
// kappa additively.  With u = R_cl^T n, n = R_i e3:  d r / d b = (u . p / |p|) / sigma,  d r / d kappa = (u . p) / sigma; the Jacobians
// over the board pose and T_cl are K18's at p' (range_point of clc_jointterms.hpp, where the terms of the cost are).  The solve
// (step, controller, outputs) is aw::arrow_problem; this file holds K21's arguments, its evaluation with the passes written out, and
// what is its shared block's own.
//
//   range_refine_kernel    one 256-thread workgroup (4 waves) per problem, the whole Levenberg-Marquardt solve in one launch.
//     evaluation   per image a wave all-reduces (wave_sum of clc_campose.hpp) the corners' {H, g, sum r^2} (reproj_accumulate; left
//                  out with the board poses held: the corner terms are then constant and no corner is read) and, in three passes
//                  over the laser points, {J_i J_i^T, J_i r, r^2} (28), J_i J_c^T (48) and {J_c J_c^T, J_c r} (44).
//     reduced 8x8  thread 0 compacts it to the free parameters and solves it with chol_solve<n_free> (as K19): T_cl is held as a
//                  whole by hold_extrinsic, b and kappa one by one by hold_range_mask.  A held parameter has scale 0.
//   range_correct_kernel   elementwise p -> p' for one (b, kappa); a point that is non-finite or has |p| = 0 becomes NaN.
//   Per-image state: RangeImage, 4.4 KB.
//
// Observability: b and kappa separate only through a spread of ranges, and b separates from t_cl only through a spread of plane
// normals and ray directions.  At a single range both cannot be free: the reduced system is then singular along (b, kappa) =
// (rho, -1), the damping keeps the step finite, and H_cr shows it.
//
// Everything numeric is CLC_HD: tests/shim/laserrange_shim.cpp compiles this header for the host with g++ and runs the same code
// with the threads as loops, in the same summation order.
#pragma once
#include "clc_jointterms.hpp"

namespace clc {
namespace lr {

using namespace jtm;

constexpr int RANGE_THREADS = aw::ARROW_THREADS;
constexpr int NR = 8;  // the shared block: T_cl's tangent (6), b, kappa
constexpr int CORRECT_THREADS = 256;

// offsets into an evaluation record E[EVAL_DOUBLES] of one image (aw::ArrowRecord<8> and the two cost parts)
constexpr int E_A = 0, E_B = 21, E_G = 69, E_C = 75, E_GC = 111, E_COST_CORNER = 119, E_COST_LASER = 120, EVAL_DOUBLES = 121;
static_assert(E_G == aw::ArrowRecord<NR>::E_G && E_C == aw::ArrowRecord<NR>::E_C && E_GC == aw::ArrowRecord<NR>::E_GC &&
                  E_COST_CORNER == aw::ArrowRecord<NR>::E_COST, "the record of K21 is the arrow's");

using RangeImage = aw::ArrowImage<NR, EVAL_DOUBLES>;

struct RangeShared : aw::ArrowShared<NR, EVAL_DOUBLES> {
  double xc[7], xce[7];           // T_cl accepted / to evaluate
  double rg[2], rge[2];           // b, kappa accepted / to evaluate
  double Af[64], rf[NR], yf[NR];  // the reduced system of the free parameters, compact
  long long n_laser;
  int32_t n_free, hold_pose;
  int32_t free_idx[NR];
};

struct RangeArgs {
  clc_options opt;
  double sigma_corner, sigma_laser;
  int32_t hold_board_poses, hold_extrinsic, hold_range_mask, pad_;
  const float* lifted;   // rounded x/z, y/z, corner `first_corner` first, n_corners of them; not read with hold_board_poses
  const float* board;    // indexed by the absolute corner offsets; not read with hold_board_poses
  const long long* coff; // [image] absolute; not read with hold_board_poses
  long long first_corner, n_corners;
  const double* pts;
  const long long* poff;
  const unsigned char* keep;      // nullable
  const long long* prob_off;      // nullable: one problem over [first_image, first_image + n_images)
  long long first_image, n_images;
  double *q, *t, *poses_cl, *range;
  clc_summary* summaries;
  double *H_cr, *cost_parts;      // nullable
  int32_t* status;
  RangeImage* ws;                 // [n_images], image first_image first
};

struct RangeCtx { double Rcl[9], tcl[3], b, kappa; };

// One image's evaluation record at pose7 / ctx: every lane of the image's wave calls it (host: once); the lead lane stores.  The
// passes are K18's (jtm::lifted_corner_pass, jtm::laser_passes) written out: through the shared bodies range_refine_kernel computed
// the same sums in another instruction order and measured up to 1 % slower (profiles/joint_terms_refactor.md).
CLC_HD void eval_image(const RangeArgs& a, const RangeCtx& c, long long img, const double* pose7, double* E) {
  CLC_BF_NO_CONTRACT
  double xe[7], R[9];
#pragma unroll
  for (int i = 0; i < 7; ++i) xe[i] = pose7[i];
  quat_to_rot(xe + 3, R);
  if (!a.hold_board_poses) {  // (uniform over the call)
    const long long cb = a.coff[img], n = a.coff[img + 1] - cb;
    const float* __restrict__ lifted = a.lifted + 2 * (cb - a.first_corner);
    const float* __restrict__ board = a.board + 2 * cb;
    double e[28];
    cp::wave_sum<28>([&](int lane, double* acc) {
      for (long long k = lane; k < n; k += cp::POSE_LANES)
        cp::reproj_accumulate(R, xe, board[2 * k], board[2 * k + 1], lifted[2 * k], lifted[2 * k + 1], acc);
    }, e);
    const double wc = 1.0 / (a.sigma_corner * a.sigma_corner);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 21; ++i) E[E_A + i] = e[i] * wc;
#pragma unroll
      for (int i = 0; i < 6; ++i) E[E_G + i] = e[21 + i] * wc;
      E[E_COST_CORNER] = 0.5 * e[27] * wc;
    }
  } else if (bf::lead_lane()) {
    CLC_AW_ROLLED for (int i = 0; i < 21; ++i) E[E_A + i] = 0.0;
    CLC_AW_ROLLED for (int i = 0; i < 6; ++i) E[E_G + i] = 0.0;
    E[E_COST_CORNER] = 0.0;
  }
  const double inv_s = 1.0 / a.sigma_laser;
  const long long pb = a.poff[img], np = a.poff[img + 1] - pb;
  const double* __restrict__ pts = a.pts + 3 * pb;
  if (np <= 0) {  // (wave-uniform)
    if (bf::lead_lane()) {
      CLC_AW_ROLLED for (int i = 0; i < 6 * NR; ++i) E[E_B + i] = 0.0;
      CLC_AW_ROLLED for (int i = E_C; i < E_COST_CORNER; ++i) E[i] = 0.0;
      E[E_COST_LASER] = 0.0;
    }
    return;
  }
  {  // J_i J_i^T, J_i r, r^2
    double s[28];
    cp::wave_sum<28>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[NR], r;
        range_point(R, xe, c.Rcl, c.tcl, c.b, c.kappa, pts + 3 * k, inv_s, Ji, Jc, &r);
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
    double s[6 * NR];
    cp::wave_sum<6 * NR>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[NR], r;
        range_point(R, xe, c.Rcl, c.tcl, c.b, c.kappa, pts + 3 * k, inv_s, Ji, Jc, &r);
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
          for (int q = 0; q < NR; ++q) acc[NR * p + q] = fma(Ji[p], Jc[q], acc[NR * p + q]);
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 6 * NR; ++i) E[E_B + i] = s[i];
    }
  }
  {  // J_c J_c^T, J_c r
    double s[44];
    cp::wave_sum<44>([&](int lane, double* acc) {
      for (long long k = lane; k < np; k += cp::POSE_LANES) {
        double Ji[6], Jc[NR], r;
        range_point(R, xe, c.Rcl, c.tcl, c.b, c.kappa, pts + 3 * k, inv_s, Ji, Jc, &r);
        int idx = 0;
#pragma unroll
        for (int p = 0; p < NR; ++p)
#pragma unroll
          for (int q = p; q < NR; ++q) { acc[idx] = fma(Jc[p], Jc[q], acc[idx]); ++idx; }
#pragma unroll
        for (int p = 0; p < NR; ++p) acc[36 + p] = fma(Jc[p], r, acc[36 + p]);
      }
    }, s);
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 44; ++i) E[E_C + i] = s[i];
    }
  }
}

// With the board poses held an image needs no corners: it takes part if it is kept, its points are usable and its start pose is
// finite.
CLC_HD ImageView view_of(const RangeArgs& a) {
  return {a.lifted, a.board, a.hold_board_poses ? nullptr : a.coff, a.first_corner, a.first_corner, a.first_corner + a.n_corners, a.pts,
          a.poff, a.keep, a.q, a.t, a.status, nullptr, nullptr};
}

// What K21 gives the arrow solve (clc_arrow.hpp): the shared block is T_cl's tangent and the two range parameters.
struct RangeTraits {
  static constexpr int NC = NR, EVAL_DOUBLES = lr::EVAL_DOUBLES;
  using Args = RangeArgs;
  using Image = RangeImage;
  using Shared = RangeShared;
  using Ctx = RangeCtx;

  static CLC_HD aw::Problem<Image> problem(const Args& a, long long pb) {
    return aw::problem_range(a.prob_off, pb, a.first_image, a.n_images, a.ws);
  }
  static CLC_HD int image_status(const Args& a, long long img) {
    return jtm::image_status(view_of(a), img, [](const double* p) { return point_usable(p); });
  }
  static CLC_HD long long observations(const Args& a, long long img) { return a.poff[img + 1] - a.poff[img]; }
  static CLC_HD void context(const Shared& sh, Ctx& c) {
    aw::tcl_context(sh, c);
    c.b = sh.rge[0];
    c.kappa = sh.rge[1];
  }
  static CLC_HD void eval_image(const Args& a, const Ctx& c, long long img, const double* pose7, double* E) {
    lr::eval_image(a, c, img, pose7, E);
  }
  static CLC_HD bool held(const Args& a, int p) { return p < 6 ? a.hold_extrinsic != 0 : ((a.hold_range_mask >> (p - 6)) & 1) != 0; }
  static CLC_HD bool init_block(const Args& a, long long pb, long long n_laser, Shared& sh, double& xn) {
    bool ok = aw::tcl_init(a.poses_cl + 7 * pb, sh);
    CLC_AW_ROLLED for (int i = 0; i < 2; ++i) {
      const double v = a.range[2 * pb + i];
      sh.rg[i] = sh.rge[i] = v;
      ok = ok && finite_d(v);
    }
    sh.n_free = aw::free_parameters<NR>(sh.free_idx, [&](int i) { return !held(a, i); });
    sh.hold_pose = a.hold_extrinsic ? 1 : 0;
    sh.n_laser = n_laser;
    sh.move_c = (sh.n_free == 0 || n_laser == 0) ? 0 : 1;
    if (sh.move_c) {
      CLC_AW_ROLLED for (int i = 0; i < 7; ++i) xn += sh.xc[i] * sh.xc[i];
      CLC_AW_ROLLED for (int i = 0; i < 2; ++i) xn += sh.rg[i] * sh.rg[i];
    }
    return ok;
  }
  static CLC_HD double cost(const double* tot) { return aw::cost_of_parts<NR>(tot); }
  static CLC_HD double block_gradient(const Shared& sh, double m) {
    if (!sh.move_c) return m;
    if (!sh.hold_pose) m = aw::tcl_gradient<NR>(sh, m);
    return aw::free_gradient<NR>(sh, 6, m);
  }
  // held parameters lose their rows and columns: chol_solve at the number of free ones
  static CLC_HD bool solve_block(Shared& sh) {
    bool ok;
    switch (sh.n_free) {
      case 1: ok = aw::solve_free<NR, 1>(sh); break;
      case 2: ok = aw::solve_free<NR, 2>(sh); break;
      case 6: ok = aw::solve_free<NR, 6>(sh); break;
      case 7: ok = aw::solve_free<NR, 7>(sh); break;
      default: ok = aw::solve_free<NR, 8>(sh); break;
    }
    return aw::scatter_free(sh, ok);
  }
  static CLC_HD void block_candidate(Shared& sh, double& sn, double& xn) {
    aw::tcl_candidate(sh, sh.hold_pose != 0, sn, xn);
    CLC_AW_ROLLED for (int p = 0; p < 2; ++p) {
      // a held parameter (scale 0, step 0) keeps its bits
      const double d = sh.step_c[6 + p] * sh.scale_c[6 + p];
      sh.rge[p] = aw::additive_candidate(sh.rg[p], sh.scale_c[6 + p] != 0.0 ? sh.rg[p] + d : sh.rg[p], sn, xn);
    }
  }
  static CLC_HD void accept_block(Shared& sh) {
    aw::tcl_accept(sh);
    CLC_AW_ROLLED for (int i = 0; i < 2; ++i) sh.rg[i] = sh.rge[i];
  }
  static CLC_HD double* information(const Args& a) { return a.H_cr; }
  static CLC_HD void write_outputs(const Args& a, long long pb, const Shared& sh, bool failed) {
    if (!failed && sh.move_c) {
      if (!sh.hold_pose) CLC_AW_ROLLED for (int i = 0; i < 7; ++i) a.poses_cl[7 * pb + i] = sh.xc[i];
      CLC_AW_ROLLED for (int i = 0; i < 2; ++i)
        if (!held(a, 6 + i)) a.range[2 * pb + i] = sh.rg[i];
    }
    aw::write_cost_parts<NR>(a.cost_parts, pb, sh, failed);
  }
};

// One problem: every thread of its workgroup calls it (host: once).
CLC_HD void range_problem(const RangeArgs& a, long long pb, RangeShared& sh) { aw::arrow_problem<RangeTraits>(a, pb, sh); }

// out[3 k ..] = p' of pts[3 k ..], NaN for a point the model does not take.
CLC_HD void range_correct_one(const double* p, double b, double kappa, double* out) {
  double pc[3], uh[3];
  const bool ok = point_usable(p);
  if (ok) correct_point(p, b, kappa, pc, uh);
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = ok ? pc[i] : __builtin_nan("");
}

#if defined(__HIPCC__)

// K21: one 256-thread workgroup per problem.
static __global__ __launch_bounds__(RANGE_THREADS) void range_refine_kernel(const RangeArgs a) {
  __shared__ RangeShared sh;
  range_problem(a, (long long)blockIdx.x, sh);
}

// One point per thread, grid-stride.
static __global__ __launch_bounds__(CORRECT_THREADS) void range_correct_kernel(const double* __restrict__ pts, const long long n,
                                                                               const double b, const double kappa,
                                                                               double* __restrict__ out) {
  for (long long k = (long long)blockIdx.x * CORRECT_THREADS + threadIdx.x; k < n; k += (long long)gridDim.x * CORRECT_THREADS) {
    const double p[3] = {pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]};
    double o[3];
    range_correct_one(p, b, kappa, o);
    out[3 * k] = o[0];
    out[3 * k + 1] = o[1];
    out[3 * k + 2] = o[2];
  }
}

#endif  // __HIPCC__

}  // namespace lr
}  // namespace clc
