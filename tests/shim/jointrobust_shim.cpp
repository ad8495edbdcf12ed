// tests/shim/jointrobust_shim.cpp — TEST ONLY.  Compiles K22 (camlasercalibratool_amd/csrc/clc_jointrobust.hpp: the evaluation of an
// image under the Cauchy loss, its traits on the arrow solve, the weights) for the host with g++, on top of K18's shim
// (joint_shim.cpp, included: shim_joint_refine, K10's shim and the pose options come with it).  The threads of a problem's workgroup
// are loops, the sums run in the device's order.  The tests compare it with the numpy / scipy restatement tests/jointrobust_ref.py,
// and the GPU tests compare the device against it.
#include <vector>

#include "joint_shim.cpp"

#include "../../camlasercalibratool_amd/csrc/clc_jointrobust.hpp"

extern "C" {

int shim_joint_loss_options_size() { return (int)sizeof(clc_joint_loss_options); }
int shim_robust_image_doubles() { return (int)(sizeof(clc::jr::RobustImage) / sizeof(double)); }

// clc_joint_loss_options_default (abi_jointrobust.hip)
void shim_joint_loss_options_default(clc_joint_loss_options* lo, const clc_joint_options* jo) {
  lo->loss_corner = 3.0;
  lo->loss_laser = (jo && std::isfinite(jo->sigma_laser) && jo->sigma_laser > 0.0) ? 0.05 / jo->sigma_laser : 5.0;
}

// The evaluation record of one image (92 doubles, K18's layout) at pose7 / pose_cl, its corners already lifted: L / B [2n], pts [3 np].
void shim_robust_eval_image(const clc_joint_options* jo, const clc_joint_loss_options* lo, const float* L, const float* B, long long n,
                            const double* pts, long long np, const double* pose7, const double* pose_cl, double* E) {
  namespace jr = clc::jr;
  jr::RobustArgs a{};
  a.sigma_corner = jo->sigma_corner;
  a.sigma_laser = jo->sigma_laser;
  a.loss_corner = lo->loss_corner;
  a.loss_laser = lo->loss_laser;
  const long long coff[2] = {0, n}, poff[2] = {0, np};
  a.lifted = L; a.board = B; a.coff = coff; a.first_corner = 0; a.n_corners = n; a.pts = pts; a.poff = poff;
  double Rcl[9];
  clc::quat_to_rot(pose_cl + 3, Rcl);
  jr::eval_image(a, 0, pose7, Rcl, pose_cl, E);
}

// clc_joint_refine_robust on the host: the lift kernel's rounding, the per-problem code of joint_robust_kernel, then that of
// joint_weights_kernel.  Offsets absolute (corner_offsets[0] may be > 0; w_corner / w_laser indexed by them), problem_offsets
// nullable; w_corner / w_laser nullable.
void shim_joint_refine_robust(const clc_camera* cam, const clc_options* opt, const clc_joint_options* jo, const clc_joint_loss_options* lo,
                              const float* corners, const float* board, const long long* coff, const double* pts, const long long* poff,
                              const unsigned char* keep, long long n_images, const long long* prob_off, long long n_problems, double* q,
                              double* t, double* poses_cl, clc_summary* sm, double* H_cl, double* cost_parts, int* status, double* w_corner,
                              double* w_laser) {
  namespace jr = clc::jr;
  const long long first = prob_off ? prob_off[0] : 0;
  const long long c0 = n_images > 0 ? coff[first] : 0, M = n_images > 0 ? coff[first + n_images] - c0 : 0;
  std::vector<float> lifted((size_t)(2 * M));
  for (long long i = 0; i < M; ++i) {
    double xy[2];
    clc::cp::cam_lift(*cam, (double)corners[2 * (c0 + i)], (double)corners[2 * (c0 + i) + 1], xy);
    lifted[(size_t)(2 * i)] = (float)xy[0];
    lifted[(size_t)(2 * i + 1)] = (float)xy[1];
  }
  std::vector<jr::RobustImage> ws((size_t)n_images);
  jr::RobustArgs a{};
  a.opt = *opt;
  a.sigma_corner = jo->sigma_corner;
  a.sigma_laser = jo->sigma_laser;
  a.loss_corner = lo->loss_corner;
  a.loss_laser = lo->loss_laser;
  a.hold_board_poses = jo->hold_board_poses ? 1 : 0;
  a.hold_extrinsic = jo->hold_extrinsic ? 1 : 0;
  a.lifted = lifted.data(); a.board = board; a.coff = coff; a.first_corner = c0; a.n_corners = M;
  a.pts = pts; a.poff = poff; a.keep = keep; a.prob_off = prob_off; a.first_image = first; a.n_images = n_images;
  a.q = q; a.t = t; a.poses_cl = poses_cl; a.summaries = sm; a.H_cl = H_cl; a.cost_parts = cost_parts; a.status = status;
  a.w_corner = w_corner; a.w_laser = w_laser;
  a.ws = ws.data();
  jr::RobustShared* sh = new jr::RobustShared;
  for (long long pb = 0; pb < n_problems; ++pb) jr::robust_problem(a, pb, *sh);
  delete sh;
  if (w_corner || w_laser)
    for (long long pb = 0; pb < n_problems; ++pb) jr::weights_problem(a, pb);
}

}  // extern "C"
