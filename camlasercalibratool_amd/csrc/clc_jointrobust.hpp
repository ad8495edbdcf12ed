// clc_jointrobust.hpp — K22: K18's joint refinement with a Cauchy loss on every corner and on every laser point,
//
//   1/2 sum rho_ac(|e_j|^2) + 1/2 sum rho_al(r_k^2)        rho_a(z) = a^2 log1p(z / a^2),  rho_a'(z) = 1 / (1 + z / a^2)
//
//   e_j = ((R_i X + t_i)_xy / (R_i X + t_i)_z - x_lifted) / sigma_corner   (one loss on the squared norm of the corner's 2-vector)
//   r_k = e3^T R_i^T (R_cl p + t_cl - t_i) / sigma_laser
//
// The scales a are in units of sigma (loss_corner, loss_laser); a = 0: no loss on that term, rho(z) = z, and that term's sums are
// K18's expressions, bit for bit.  The Gauss-Newton blocks follow Ceres' corrector for rho'' <= 0: every row of an observation and
// its residual are scaled by sqrt(rho'), so A_i, B_i, C take w J^T J and the gradients w J^T r with w = rho'(z).  An arrow problem
// of clc_arrow.hpp (NC = 6, K18's record): the solve (step, controller, outputs) is aw::arrow_problem, the laser row, the loss and
// the passes are clc_jointterms.hpp's, the same that K18 takes; this file holds K22's arguments, its weighted corner pass and how
// its evaluation and its weights are put together.
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
#include "clc_jointterms.hpp"

namespace clc {
namespace jr {

using namespace jtm;

constexpr int ROBUST_THREADS = aw::ARROW_THREADS;

// an evaluation record E[EVAL_DOUBLES] of one image: aw::ArrowRecord<6> and the two cost parts, K18's
constexpr int EVAL_DOUBLES = aw::ArrowRecord<6>::E_COST + 2;
static_assert(EVAL_DOUBLES == 92, "the record of K22");

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
  const Loss ls = loss_of(a.loss_corner, a.loss_laser);  // (uniform over the call)
  if (!ls.corner) {  // K18's sums
    lifted_corner_pass(lifted, board, n, R, xe, wc, E);
  } else {
    double e[28];
    cp::wave_sum<28>([&](int lane, double* acc) {
      for (long long k = lane; k < n; k += cp::POSE_LANES) {
        double row[28];
        const double z = corner_z(R, xe, board[2 * k], board[2 * k + 1], lifted[2 * k], lifted[2 * k + 1], wc, row);
        const double w = cauchy_weight(z, ls.inv_ac2);
#pragma unroll
        for (int i = 0; i < 27; ++i) acc[i] = fma(w, row[i], acc[i]);
        acc[27] += cauchy_rho(z, ls.ac2, ls.inv_ac2);
      }
    }, e);
    store_corner_sums(e, wc, 0.5 * e[27], E);  // (e[27] is sum rho, in units of sigma already)
  }
  const long long pb = a.poff[img], np = a.poff[img + 1] - pb;
  const double* __restrict__ pts = a.pts + 3 * pb;
  if (np <= 0) {  // (wave-uniform)
    zero_laser_part(E);
    return;
  }
  // The three passes of K18.  Without the loss w is exactly 1 and w J has J's bits.
  laser_passes<true>(np, ls, [&](long long k, double* Ji, double* Jc, double* r) { laser_point(R, xe, Rcl, tcl, pts + 3 * k, inv_s, Ji, Jc, r); }, E);
}

// K18's rule for the images that take part.
CLC_HD ImageView view_of(const RobustArgs& a) {
  return {a.lifted, a.board, a.coff, a.first_corner, a.first_corner, a.first_corner + a.n_corners, a.pts, a.poff, a.keep, a.q, a.t,
          a.status, a.w_corner, a.w_laser};
}

// What K22 gives the arrow solve (clc_arrow.hpp): the shared block is the pose T_cl (jtm::TclTraits, as K18's) under the robust cost.
struct JointRobustTraits : TclTraits<RobustArgs, RobustImage, RobustShared> {
  static CLC_HD int image_status(const Args& a, long long img) {
    return jtm::image_status(view_of(a), img, [](const double* p) { return point_finite(p); });
  }
  static CLC_HD void eval_image(const Args& a, const Ctx& c, long long img, const double* pose7, double* E) {
    jr::eval_image(a, img, pose7, c.Rcl, c.tcl, E);
  }
};

// One problem: every thread of its workgroup calls it (host: once).
CLC_HD void robust_problem(const RobustArgs& a, long long pb, RobustShared& sh) { aw::arrow_problem<JointRobustTraits>(a, pb, sh); }

// The weights of one problem at the returned poses: the waves take its images round-robin (host: a loop).
CLC_HD void weights_problem(const RobustArgs& a, long long pb) {
  CLC_BF_NO_CONTRACT
  const aw::Problem<RobustImage> pr = JointRobustTraits::problem(a, pb);
  const bool failed = a.summaries[pb].termination == CLC_FAILURE;
  double pose_cl[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) pose_cl[i] = a.poses_cl[7 * pb + i];
  const ImageView v = view_of(a);
  const Loss ls = loss_of(a.loss_corner, a.loss_laser);
  const double wc = 1.0 / (a.sigma_corner * a.sigma_corner), inv_s = 1.0 / a.sigma_laser;
  aw::each_image_wave(pr.P, [&](long long j) {
    double Rcl[9];
    quat_to_rot(pose_cl + 3, Rcl);
    weights_image(v, ls, pr.i0 + j, failed,
                  [&](const double* R, const double* xe, const float* lifted, const float* board, long long k) {
                    double row[28];
                    return cauchy_weight(corner_z(R, xe, board[2 * k], board[2 * k + 1], lifted[2 * k], lifted[2 * k + 1], wc, row), ls.inv_ac2);
                  },
                  [&](const double* R, const double* xe, const double* pts, long long k) {
                    const double r = laser_residual(R, xe, Rcl, pose_cl, pts + 3 * k, inv_s);
                    return cauchy_weight(r * r, ls.inv_al2);
                  });
  });
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

#endif  // __HIPCC__

}  // namespace jr
}  // namespace clc
