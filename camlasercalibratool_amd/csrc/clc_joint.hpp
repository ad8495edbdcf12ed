// clc_joint.hpp — K18: joint refinement of the board poses T_ca,i and the camera-laser extrinsic T_cl of one problem, one cost
//
//   1/2 sum |((R_i X + t_i)_xy / (R_i X + t_i)_z - x_lifted) / sigma_corner|^2  +  1/2 sum (e3^T R_i^T (R_cl p + t_cl - t_i) / sigma_laser)^2
//
// over the tangent [dt, dtheta] of every pose.  The arrow of clc_arrow.hpp with the 6 tangent parameters of T_cl as its shared block:
// the solve (step, controller, outputs) is aw::arrow_problem and the terms of the cost are clc_jointterms.hpp's; this file holds
// K18's arguments, how its evaluation groups the passes and what its traits do not share.
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
#include "clc_jointterms.hpp"

namespace clc {
namespace jt {

using namespace jtm;

constexpr int JOINT_THREADS = aw::ARROW_THREADS;

// an evaluation record E[EVAL_DOUBLES] of one image: aw::ArrowRecord<6> and the two cost parts
constexpr int EVAL_DOUBLES = aw::ArrowRecord<6>::E_COST + 2;
static_assert(EVAL_DOUBLES == 92, "the record of K18");

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

// One image's evaluation record at pose7 / (Rcl, tcl): every lane of the image's wave calls it (host: once); the lead lane stores.
CLC_HD void eval_image(const JointArgs& a, long long img, const double* pose7, const double* Rcl, const double* tcl, double* E) {
  CLC_BF_NO_CONTRACT
  double xe[7], R[9];
#pragma unroll
  for (int i = 0; i < 7; ++i) xe[i] = pose7[i];
  quat_to_rot(xe + 3, R);
  const long long cb = a.coff[img], n = a.coff[img + 1] - cb;
  const double wc = 1.0 / (a.sigma_corner * a.sigma_corner), inv_s = 1.0 / a.sigma_laser;
  lifted_corner_pass(a.lifted + 2 * (cb - a.first_corner), a.board + 2 * cb, n, R, xe, wc, E);
  const long long pb = a.poff[img], np = a.poff[img + 1] - pb;
  const double* __restrict__ pts = a.pts + 3 * pb;
  if (np <= 0) {  // (wave-uniform)
    zero_laser_part(E);
    return;
  }
  laser_passes(np, [&](long long k, double* Ji, double* Jc, double* r) { laser_point(R, xe, Rcl, tcl, pts + 3 * k, inv_s, Ji, Jc, r); }, E);
}

CLC_HD ImageView view_of(const JointArgs& a) {
  return {a.lifted, a.board, a.coff, a.first_corner, a.first_corner, a.first_corner + a.n_corners, a.pts, a.poff, a.keep, a.q, a.t,
          a.status, nullptr, nullptr};
}

// What K18 gives the arrow solve (clc_arrow.hpp): the shared block is the pose T_cl (jtm::TclTraits) under K18's cost.
struct JointTraits : TclTraits<JointArgs, JointImage, JointShared> {
  static CLC_HD int image_status(const Args& a, long long img) {
    return jtm::image_status(view_of(a), img, [](const double* p) { return point_finite(p); });
  }
  static CLC_HD void eval_image(const Args& a, const Ctx& c, long long img, const double* pose7, double* E) {
    jt::eval_image(a, img, pose7, c.Rcl, c.tcl, E);
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

#endif  // __HIPCC__

}  // namespace jt
}  // namespace clc
