// abi_lift.hpp — the grid of the lift kernels, and the one launch of the rounded camera lift ahead of the board-pose kernels
// (abi_campose.hip: K10, K16, K17) and of the joint refinement (abi_joint.hip: K18).  A header of its own: a unit that includes it
// instantiates campose_lift_kernel<true>.
// Host code only: _build.csrc_sha16() does not cover this file.
#pragma once
#include "abi_staging.hpp"
#include "clc_campose.hpp"

namespace clc_abi {

inline unsigned lift_blocks(size_t n) { return (unsigned)((n + clc::cp::LIFT_THREADS - 1) / clc::cp::LIFT_THREADS); }

// The corners [first, first + n_corners) of corners_dev lifted (rounded to float32) into a scratch array of the call:
// lifted[0] is corner `first`.  No launch at n_corners == 0.  nullptr: an error is held by st.
inline float* enqueue_lift(Staging& st, const clc_camera& cam, const float* corners_dev, long long first, size_t n_corners) {
  float* lifted = st.scratch<float>(2 * n_corners);
  if (!lifted || n_corners == 0) return lifted;
  hipLaunchKernelGGL((clc::cp::campose_lift_kernel<true>), dim3(lift_blocks(n_corners)), dim3(clc::cp::LIFT_THREADS), 0, st.stream(), cam,
                     corners_dev + 2 * first, (long long)n_corners, nullptr, lifted);
  st.launched();
  return st.ok() ? lifted : nullptr;
}

}  // namespace clc_abi
