// tests/shim/camcal_shim.cpp — TEST ONLY.  Compiles K19 (camlasercalibratool_amd/csrc/clc_camcal.hpp: the projection's derivatives, the
// evaluation of an image, the Schur step, the controller, the outputs of one problem and the closed-form focal start) for the host with
// g++, on top of K10's shim (campose_shim.cpp, included: the camera models, shim_board_poses and the pose options come with it).  The
// threads of a problem's workgroup are loops, the sums run in the device's order.  The tests compare it with the numpy / scipy
// restatement tests/camcal_ref.py, and the GPU tests compare the device against it.
#include <vector>

#include "campose_shim.cpp"

#include "../../camlasercalibratool_amd/csrc/clc_camcal.hpp"

extern "C" {

int shim_camcal_options_size() { return (int)sizeof(clc_camcal_options); }
int shim_camcal_image_doubles() { return (int)(sizeof(clc::cc::CalImage) / sizeof(double)); }
int shim_camcal_shared_bytes() { return (int)sizeof(clc::cc::CalShared); }

// clc_camcal_options_default (abi_camcal.hip)
void shim_camcal_options_default(clc_camcal_options* o, int model) {
  o->sigma_px = 0.3;
  o->hold_mask = model == CLC_CAMERA_KANNALA_BRANDT ? (1u << 6) | (1u << 7) : 0u;
  o->hold_board_poses = 0;
}

// The two residuals of one corner and their Jacobians: r[2], J[2 x 6] over the image's tangent, JK[2 x 8] over the intrinsics.
int shim_camcal_corner(const clc_camera* cam, const double* pose7, double X, double Y, double u, double v, double inv_s, double* r,
                       double* J, double* JK) {
  double R[9];
  clc::quat_to_rot(pose7 + 3, R);
  return clc::cc::corner_terms(*cam, R, pose7, X, Y, u, v, inv_s, r, J, JK) ? 1 : 0;
}

// The evaluation record of one image (clc::cc::EVAL_DOUBLES doubles: A 21, B 48, g 6, C 36, g_c 8, the cost).
void shim_camcal_eval_image(const clc_camera* cam, double sigma_px, const float* px, const float* B, long long n, const double* pose7,
                            double* E) {
  clc::cc::CalArgs a{};
  a.sigma_px = sigma_px;
  const long long coff[2] = {0, n};
  a.corners = px; a.board = B; a.coff = coff;
  clc::cc::eval_image(a, *cam, 0, pose7, E);
}

// clc_camera_calibrate on the host: the per-problem code of camcal_kernel.  Offsets absolute, prob_off nullable.
void shim_camera_calibrate(const clc_options* opt, const clc_camcal_options* co, const float* corners, const float* board,
                           const long long* coff, const unsigned char* keep, long long n_images, const long long* prob_off,
                           long long n_problems, clc_camera* cams, double* q, double* t, clc_summary* sm, double* H_cam, double* rms,
                           int* status) {
  namespace cc = clc::cc;
  std::vector<cc::CalImage> ws((size_t)(n_images > 0 ? n_images : 1));
  cc::CalArgs a{};
  a.opt = *opt;
  a.sigma_px = co->sigma_px;
  a.hold_mask = co->hold_mask;
  a.hold_board_poses = co->hold_board_poses ? 1 : 0;
  a.corners = corners; a.board = board; a.coff = coff; a.keep = keep; a.prob_off = prob_off; a.n_images = n_images;
  a.q = q; a.t = t; a.cams = cams; a.summaries = sm; a.H_cam = H_cam; a.rms = rms; a.status = status; a.ws = ws.data();
  cc::CalShared* sh = new cc::CalShared;
  for (long long pb = 0; pb < n_problems; ++pb) cc::camcal_problem(a, pb, *sh);
  delete sh;
}

// The per-image half of clc_camera_guess: H[9 n], status[n]; then its host half.  Returns the focal length (NaN: none).
double shim_camera_guess(int width, int height, const float* corners, const float* board, const long long* off, long long n_images,
                         double* H, int* status, int* n_used) {
  namespace cc = clc::cc;
  cc::GuessShared* sh = new cc::GuessShared;
  for (long long img = 0; img < n_images; ++img) {
    const long long b = off[img], n = off[img + 1] - b;
    double h[9];
    const int st = cc::homography_image(corners + 2 * b, board + 2 * b, n, 0.5 * width, 0.5 * height, *sh, h);
    status[img] = st;
    for (int i = 0; i < 9; ++i) H[9 * img + i] = st == CLC_POSE_OK ? h[i] : __builtin_nan("");
  }
  delete sh;
  return cc::guess_focal(H, status, n_images, n_used);
}

}  // extern "C"
