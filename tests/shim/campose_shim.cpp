// tests/shim/campose_shim.cpp — TEST ONLY.  Compiles the camera models and the per-image planar PnP of K10
// (camlasercalibratool_amd/csrc/clc_campose.hpp) for the host with g++: the 64 lanes of an image's wave are a loop, the wave
// all-reduce a butterfly over them in the device's order, the 9x9 Jacobi a LaneRows with its rows in one array.  The tests compare
// it with numpy / scipy restatements here, and the GPU tests compare the device against it.
#include <cmath>

#include "../../camlasercalibratool_amd/csrc/clc_campose.hpp"

extern "C" {

int shim_camera_size() { return (int)sizeof(clc_camera); }

void shim_camera_lift(const clc_camera* cam, const float* px, long long n, double* xy) {
  for (long long i = 0; i < n; ++i) clc::cp::cam_lift(*cam, (double)px[2 * i], (double)px[2 * i + 1], xy + 2 * i);
}

// kb_theta for the test of the root choice: theta of |p_u| = p under the camera's k2..k5
double shim_kb_theta(const clc_camera* cam, double p) { return clc::cp::kb_theta(clc::cp::kb_poly(cam->dist), p); }

void shim_camera_project(const clc_camera* cam, const double* pose7, const double* pts, long long n, double* px) {
  for (long long i = 0; i < n; ++i) {
    double P[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    if (pose7) {
      double Q[3];
      clc::cp::pose_apply(pose7, P, Q);
      P[0] = Q[0]; P[1] = Q[1]; P[2] = Q[2];
    }
    clc::cp::cam_project(*cam, P, px + 2 * i);
  }
}

void shim_pose_options_default(clc_options* o) {  // clc_options_default + clc_pose_options_default (abi_core.hip, abi_campose.hip)
  o->max_num_iterations = 50;
  o->max_num_consecutive_invalid_steps = 5;
  o->jacobi_scaling = 1;
  o->use_loss = 0;
  o->loss_scale_factor = 0.05;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->function_tolerance = 1e-15;
  o->gradient_tolerance = 1e-16;
  o->parameter_tolerance = 1e-14;
  o->launch_ahead = 0;
  o->profile_events = 0;
}

// clc_board_poses on the host: the lift kernel's rounding, then the per-image code of board_pose_kernel.
void shim_board_poses(const clc_camera* cam, const clc_options* opt, const float* corners, const float* board, const long long* off,
                      long long n_images, double* q, double* t, double* rms, int* status, clc_summary* sm) {
  const long long M = off[n_images] - off[0];
  float* lifted = new float[2 * (M > 0 ? M : 1)];
  for (long long i = 0; i < M; ++i) {
    double xy[2];
    const long long k = off[0] + i;
    clc::cp::cam_lift(*cam, (double)corners[2 * k], (double)corners[2 * k + 1], xy);
    lifted[2 * i] = (float)xy[0];
    lifted[2 * i + 1] = (float)xy[1];
  }
  clc::cp::PoseShared* sh = new clc::cp::PoseShared;
  for (long long img = 0; img < n_images; ++img) {
    const long long b = off[img], n = off[img + 1] - b;
    double pose7[7], r = 0.0;
    const int st = clc::cp::board_pose_image(*opt, lifted + 2 * (b - off[0]), board + 2 * b, n, *sh, pose7, &r);
    clc::cp::board_pose_store(st, pose7, r, img, q, t, rms, status);
    if (sm) {
      if (st == CLC_POSE_OK) sm[img] = sh->sm;
      else clc::cp::summary_empty(sm[img]);
    }
  }
  delete sh;
  delete[] lifted;
}

}  // extern "C"
