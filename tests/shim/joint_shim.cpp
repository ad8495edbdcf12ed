// tests/shim/joint_shim.cpp — TEST ONLY.  Compiles K18 (camlasercalibratool_amd/csrc/clc_joint.hpp: the evaluation of an image, the
// Schur step, the controller and the outputs of one problem) for the host with g++, on top of K10's shim (campose_shim.cpp,
// included: the camera models, shim_board_poses and the pose options come with it).  The threads of a problem's workgroup are loops,
// the sums run in the device's order.  The tests compare it with the numpy / scipy restatement tests/joint_ref.py, and the GPU tests
// compare the device against it.
#include <vector>

#include "campose_shim.cpp"

#include "../../camlasercalibratool_amd/csrc/clc_joint.hpp"

extern "C" {

int shim_joint_options_size() { return (int)sizeof(clc_joint_options); }
int shim_joint_image_doubles() { return (int)(sizeof(clc::jt::JointImage) / sizeof(double)); }

// clc_joint_options_default (abi_joint.hip)
void shim_joint_options_default(clc_joint_options* o, const clc_camera* cam) {
  const double f = cam ? std::sqrt(std::fabs(cam->proj[0] * cam->proj[1])) : 0.0;
  o->sigma_corner = f > 0.0 ? 0.3 / f : 0.0;
  o->sigma_laser = 0.01;
  o->hold_board_poses = 0;
  o->hold_extrinsic = 0;
}

// The evaluation record of one image (clc::jt::EVAL_DOUBLES doubles: A 21, B 36, g 6, C 21, g_c 6, the two cost parts) at pose7 /
// pose_cl, its corners already lifted: L / B [2n], pts [3 np].
void shim_joint_eval_image(const clc_joint_options* jo, const float* L, const float* B, long long n, const double* pts, long long np,
                           const double* pose7, const double* pose_cl, double* E) {
  namespace jt = clc::jt;
  jt::JointArgs a{};
  a.sigma_corner = jo->sigma_corner;
  a.sigma_laser = jo->sigma_laser;
  const long long coff[2] = {0, n}, poff[2] = {0, np};
  a.lifted = L; a.board = B; a.coff = coff; a.first_corner = 0; a.n_corners = n; a.pts = pts; a.poff = poff;
  double Rcl[9];
  clc::quat_to_rot(pose_cl + 3, Rcl);
  jt::eval_image(a, 0, pose7, Rcl, pose_cl, E);
}

// clc_joint_refine on the host: the lift kernel's rounding, then the per-problem code of joint_refine_kernel.  Offsets absolute
// (corner_offsets[0] may be > 0), problem_offsets nullable.
void shim_joint_refine(const clc_camera* cam, const clc_options* opt, const clc_joint_options* jo, const float* corners, const float* board,
                       const long long* coff, const double* pts, const long long* poff, const unsigned char* keep, long long n_images,
                       const long long* prob_off, long long n_problems, double* q, double* t, double* poses_cl, clc_summary* sm,
                       double* H_cl, double* cost_parts, int* status) {
  namespace jt = clc::jt;
  const long long first = prob_off ? prob_off[0] : 0;
  const long long c0 = n_images > 0 ? coff[first] : 0, M = n_images > 0 ? coff[first + n_images] - c0 : 0;
  std::vector<float> lifted((size_t)(2 * M));
  for (long long i = 0; i < M; ++i) {
    double xy[2];
    clc::cp::cam_lift(*cam, (double)corners[2 * (c0 + i)], (double)corners[2 * (c0 + i) + 1], xy);
    lifted[(size_t)(2 * i)] = (float)xy[0];
    lifted[(size_t)(2 * i + 1)] = (float)xy[1];
  }
  std::vector<jt::JointImage> ws((size_t)n_images);
  jt::JointArgs a{};
  a.opt = *opt;
  a.sigma_corner = jo->sigma_corner;
  a.sigma_laser = jo->sigma_laser;
  a.hold_board_poses = jo->hold_board_poses ? 1 : 0;
  a.hold_extrinsic = jo->hold_extrinsic ? 1 : 0;
  a.lifted = lifted.data(); a.board = board; a.coff = coff; a.first_corner = c0; a.n_corners = M;
  a.pts = pts; a.poff = poff; a.keep = keep; a.prob_off = prob_off; a.first_image = first; a.n_images = n_images;
  a.q = q; a.t = t; a.poses_cl = poses_cl; a.summaries = sm; a.H_cl = H_cl; a.cost_parts = cost_parts; a.status = status;
  a.ws = ws.data();
  jt::JointShared* sh = new jt::JointShared;
  for (long long pb = 0; pb < n_problems; ++pb) jt::joint_problem(a, pb, *sh);
  delete sh;
}

}  // extern "C"
