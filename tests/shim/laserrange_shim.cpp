// tests/shim/laserrange_shim.cpp — TEST ONLY.  Compiles K21 (camlasercalibratool_amd/csrc/clc_laserrange.hpp: the evaluation of an
// image with the range offset and scale, the traits of its 8-wide shared block, the point correction) for the host with g++, on top
// of K18's shim (joint_shim.cpp, included: shim_joint_refine, K10's shim and the pose options come with it).  The threads of a
// problem's workgroup are loops, the sums run in the device's order.  The tests compare it with the numpy / scipy restatement
// tests/laserrange_ref.py, and the GPU tests compare the device against it.
#include <vector>

#include "joint_shim.cpp"

#include "../../camlasercalibratool_amd/csrc/clc_laserrange.hpp"

extern "C" {

int shim_range_options_size() { return (int)sizeof(clc_range_options); }
int shim_range_image_doubles() { return (int)(sizeof(clc::lr::RangeImage) / sizeof(double)); }
int shim_range_eval_doubles() { return clc::lr::EVAL_DOUBLES; }

// clc_range_options_default (abi_laserrange.hip)
void shim_range_options_default(clc_range_options* o, const clc_camera* cam) {
  clc_joint_options jo;
  shim_joint_options_default(&jo, cam);
  o->sigma_corner = jo.sigma_corner;
  o->sigma_laser = jo.sigma_laser;
  o->hold_board_poses = 0;
  o->hold_extrinsic = 0;
  o->hold_range_mask = 0;
  o->reserved = 0;
}

// The evaluation record of one image (clc::lr::EVAL_DOUBLES doubles: A 21, B 48, g 6, C 36, g_c 8, the two cost parts) at pose7 /
// pose_cl / range, its corners already lifted: L / B [2n], pts [3 np].
void shim_range_eval_image(const clc_range_options* ro, const float* L, const float* B, long long n, const double* pts, long long np,
                           const double* pose7, const double* pose_cl, const double* range, double* E) {
  namespace lr = clc::lr;
  lr::RangeArgs a{};
  a.sigma_corner = ro->sigma_corner;
  a.sigma_laser = ro->sigma_laser;
  a.hold_board_poses = ro->hold_board_poses ? 1 : 0;
  const long long coff[2] = {0, n}, poff[2] = {0, np};
  a.lifted = L; a.board = B; a.coff = coff; a.first_corner = 0; a.n_corners = n; a.pts = pts; a.poff = poff;
  lr::RangeCtx c;
  clc::quat_to_rot(pose_cl + 3, c.Rcl);
  for (int i = 0; i < 3; ++i) c.tcl[i] = pose_cl[i];
  c.b = range[0];
  c.kappa = range[1];
  lr::eval_image(a, c, 0, pose7, E);
}

// clc_joint_refine_range on the host: the lift kernel's rounding (left out with the board poses held: no corner array is read), then
// the per-problem code of range_refine_kernel.  Offsets absolute, problem_offsets nullable.
void shim_joint_refine_range(const clc_camera* cam, const clc_options* opt, const clc_range_options* ro, const float* corners,
                             const float* board, const long long* coff, const double* pts, const long long* poff, const unsigned char* keep,
                             long long n_images, const long long* prob_off, long long n_problems, double* q, double* t, double* poses_cl,
                             double* range, clc_summary* sm, double* H_cr, double* cost_parts, int* status) {
  namespace lr = clc::lr;
  const bool use_corners = !ro->hold_board_poses;
  const long long first = prob_off ? prob_off[0] : 0;
  const long long c0 = (use_corners && n_images > 0) ? coff[first] : 0, M = (use_corners && n_images > 0) ? coff[first + n_images] - c0 : 0;
  std::vector<float> lifted((size_t)(2 * M));
  for (long long i = 0; i < M; ++i) {
    double xy[2];
    clc::cp::cam_lift(*cam, (double)corners[2 * (c0 + i)], (double)corners[2 * (c0 + i) + 1], xy);
    lifted[(size_t)(2 * i)] = (float)xy[0];
    lifted[(size_t)(2 * i + 1)] = (float)xy[1];
  }
  std::vector<lr::RangeImage> ws((size_t)n_images);
  lr::RangeArgs a{};
  a.opt = *opt;
  a.sigma_corner = use_corners ? ro->sigma_corner : 1.0;
  a.sigma_laser = ro->sigma_laser;
  a.hold_board_poses = ro->hold_board_poses ? 1 : 0;
  a.hold_extrinsic = ro->hold_extrinsic ? 1 : 0;
  a.hold_range_mask = ro->hold_range_mask;
  if (use_corners) { a.lifted = lifted.data(); a.board = board; a.coff = coff; a.first_corner = c0; a.n_corners = M; }
  a.pts = pts; a.poff = poff; a.keep = keep; a.prob_off = prob_off; a.first_image = first; a.n_images = n_images;
  a.q = q; a.t = t; a.poses_cl = poses_cl; a.range = range; a.summaries = sm; a.H_cr = H_cr; a.cost_parts = cost_parts; a.status = status;
  a.ws = ws.data();
  lr::RangeShared* sh = new lr::RangeShared;
  for (long long pb = 0; pb < n_problems; ++pb) lr::range_problem(a, pb, *sh);
  delete sh;
}

// clc_range_correct on the host.
void shim_range_correct(const double* range, const double* pts, long long n, double* out) {
  for (long long k = 0; k < n; ++k) {
    const double p[3] = {pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]};
    clc::lr::range_correct_one(p, range[0], range[1], out + 3 * k);
  }
}

}  // extern "C"
