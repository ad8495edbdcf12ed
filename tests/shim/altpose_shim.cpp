// tests/shim/altpose_shim.cpp — TEST ONLY.  Compiles K17 (camlasercalibratool_amd/csrc/clc_altpose.hpp: the mirror start, the LM
// stage from a given start, the costs, the classification and the sequential per-image driver) for the host with g++, on top of
// K16's shim (robustpose_shim.cpp, included: shim_board_poses, shim_board_poses_robust and the camera models come with it).  The
// tests compare it with the numpy restatement tests/altpose_ref.py, and the GPU tests compare the device against it.
#include "robustpose_shim.cpp"

#include "../../camlasercalibratool_amd/csrc/clc_altpose.hpp"

extern "C" {

int shim_alt_options_size() { return (int)sizeof(clc_alt_pose_options); }

// clc_alt_pose_options_default (abi_campose.hip)
void shim_alt_options_default(clc_alt_pose_options* o) {
  o->same_angle = 0.01;
  o->ratio_gate = 2.0;
}

// One image, its arrays given directly: L / B [2n], mask (nullable) [n], sub_l / sub_b scratch [2n]; the outputs at index img.
void shim_alt_image(const clc_options* opt, const clc_alt_pose_options* ao, const float* L, const float* B, long long n,
                    const unsigned char* mask, const double* q_in, const double* t_in, const int* status_in, long long img, float* sub_l,
                    float* sub_b, double* q, double* t, double* rms, double* cost_in, double* cost_alt, double* ratio, double* rot_angle,
                    double* normal_angle, int* kind, unsigned char* ambiguous, unsigned char* better, clc_summary* sm) {
  clc::cp::PoseShared* sh = new clc::cp::PoseShared;
  const clc::ap::AltOut out{q, t, rms, cost_in, cost_alt, ratio, rot_angle, normal_angle, kind, ambiguous, better, sm};
  clc::ap::alt_image(*opt, *ao, L, B, n, mask, q_in, t_in, status_in, img, sub_l, sub_b, *sh, out);
  delete sh;
}

// clc_board_poses_alternate on the host: the lift kernel's rounding, then the per-image code of the two kernels.  inlier (nullable)
// indexed like the corners.
void shim_board_poses_alternate(const clc_camera* cam, const clc_options* opt, const clc_alt_pose_options* ao, const float* corners,
                                const float* board, const long long* off, long long n_images, const unsigned char* inlier,
                                const double* q_in, const double* t_in, const int* status_in, double* q, double* t, double* rms,
                                double* cost_in, double* cost_alt, double* ratio, double* rot_angle, double* normal_angle, int* kind,
                                unsigned char* ambiguous, unsigned char* better, clc_summary* sm) {
  const long long M = off[n_images] - off[0];
  float* lifted = new float[2 * (M > 0 ? M : 1)];
  float* sub_l = new float[2 * (M > 0 ? M : 1)];
  float* sub_b = new float[2 * (M > 0 ? M : 1)];
  for (long long i = 0; i < M; ++i) {
    double xy[2];
    const long long k = off[0] + i;
    clc::cp::cam_lift(*cam, (double)corners[2 * k], (double)corners[2 * k + 1], xy);
    lifted[2 * i] = (float)xy[0];
    lifted[2 * i + 1] = (float)xy[1];
  }
  for (long long img = 0; img < n_images; ++img) {
    const long long b = off[img], n = off[img + 1] - b, s = b - off[0];
    shim_alt_image(opt, ao, lifted + 2 * s, board + 2 * b, n, inlier ? inlier + b : nullptr, q_in, t_in, status_in, img, sub_l + 2 * s,
                   sub_b + 2 * s, q, t, rms, cost_in, cost_alt, ratio, rot_angle, normal_angle, kind, ambiguous, better, sm);
  }
  delete[] lifted;
  delete[] sub_l;
  delete[] sub_b;
}

}  // extern "C"
