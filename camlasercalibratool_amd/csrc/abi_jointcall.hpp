// abi_jointcall.hpp — host code the units of the joint problems share (abi_joint.hip, abi_laserrange.hip, abi_jointrobust.hip,
// abi_fullcal.hip): the option checks with their messages, the read of a device-array call's ranges, and the arrays that K18's and K22's calls
// have in common, staged (host form) or named (device form) into the kernel's arguments.  No kernel lives here: the one the ranges
// are read with is the unit's, from clc_jointterms.hpp through its kernel header.
#pragma once
#include <cmath>
#include <string>

#include "abi_drive.hpp"
#include "abi_staging.hpp"

namespace clc_abi {

// ---- the option checks; the order in which a unit makes them is its own ----
inline int check_sigma(const char* who, const char* name, double v) {
  if (std::isfinite(v) && v > 0.0) return CLC_OK;
  return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": " + name + " must be finite and > 0").c_str());
}
// sigma_corner (where the corners take part), sigma_laser, then the two hold flags: what K18, K21 and K22 refuse first.
inline int check_sigmas_and_holds(const char* who, bool corners, double sigma_corner, double sigma_laser, int hold_board_poses,
                                  int hold_extrinsic) {
  if (corners) CLC_TRY(check_sigma(who, "sigma_corner", sigma_corner));
  CLC_TRY(check_sigma(who, "sigma_laser", sigma_laser));
  if (hold_board_poses && hold_extrinsic) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": both hold flags set").c_str());
  return CLC_OK;
}
inline int check_loss_scales(const char* who, double loss_corner, double loss_laser) {
  const std::string w(who);
  if (!(std::isfinite(loss_corner) && loss_corner >= 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": loss_corner must be finite and >= 0").c_str());
  if (!(std::isfinite(loss_laser) && loss_laser >= 0.0)) return fail(CLC_ERR_INVALID_ARG, (w + ": loss_laser must be finite and >= 0").c_str());
  return CLC_OK;
}
inline int check_range_mask(const char* who, int32_t hold_range_mask) {
  if (hold_range_mask < 0 || hold_range_mask > 3) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": hold_range_mask outside 0..3").c_str());
  return CLC_OK;
}

// ---- the ranges of a device-array call ----
// Reads {first image, first corner, end of the corners} with the unit's ends kernel (one small read ahead of the enqueue, as
// clc_board_poses_device reads the ends of its offsets; `read` false: nothing to read, all 0) into a.first_image, a.first_corner,
// a.n_corners, and refuses offsets that do not ascend and corners without their arrays.
template <class Args, class Kernel>
int read_joint_ends(clc_handle* h, const char* who, Kernel ends_kernel, bool read, size_t n_images, const float* corners_px_dev, Args& a) {
  long long ends[3] = {0, 0, 0};
  if (read) {
    Staging rd(h);
    long long* ends_dev = rd.out(ends, 3);
    if (rd.ok()) {
      hipLaunchKernelGGL(ends_kernel, dim3(1), dim3(64), 0, rd.stream(), a.prob_off, a.coff, (long long)n_images, ends_dev);
      rd.launched();
    }
    CLC_TRY(rd.finish(who));
  }
  const std::string w(who);
  if (ends[0] < 0 || ends[1] < 0 || ends[2] < ends[1]) return fail(CLC_ERR_INVALID_ARG, (w + ": offsets not monotone").c_str());
  a.first_image = ends[0];
  a.first_corner = ends[1];
  a.n_corners = ends[2] - ends[1];
  if (a.n_corners > 0 && (!corners_px_dev || !a.board)) return fail(CLC_ERR_INVALID_ARG, (w + ": bad argument").c_str());
  return CLC_OK;
}

// ---- the arrays of clc_joint_refine and of K22's call, host or device ----
struct JointArrays {
  const float *corners_px, *board_xy;
  const int64_t* corner_offsets;
  const double* pts;
  const int64_t* pts_offsets;
  const uint8_t* keep;
  size_t n_images;
  const int64_t* problem_offsets;
  size_t n_problems;
  double *q_ca_wxyz, *t_ca, *poses_cl;
  clc_summary* summaries;
  double *H_cl, *cost_parts;
  int32_t* image_status;
};

// The host form's refusals after the options, everything that can be refused without the device: crel / prel the offsets rebased,
// M / N the corners / points they span.
inline int joint_host_checks(const char* who, clc_handle* h, const JointArrays& c, std::vector<long long>* crel, std::vector<long long>* prel,
                             size_t* M, size_t* N) {
  const std::string bad = std::string(who) + ": bad argument";
  if ((c.n_images > 0 && (!c.corner_offsets || !c.pts_offsets || !c.q_ca_wxyz || !c.t_ca || !c.image_status)) ||
      (c.n_problems > 0 && (!c.poses_cl || !c.summaries)))
    return fail(CLC_ERR_INVALID_ARG, bad.c_str());
  CLC_TRY(problem_count_checks(who, c.n_images, c.problem_offsets != nullptr, c.n_problems));
  CLC_TRY(host_offsets(who, c.corner_offsets, c.n_images, true, nullptr, crel, M));
  CLC_TRY(host_offsets(who, c.pts_offsets, c.n_images, true, nullptr, prel, N));
  CLC_TRY(host_problem_offsets(who, c.problem_offsets, c.n_problems, c.n_images));
  if (!h || (*M > 0 && (!c.corners_px || !c.board_xy)) || (*N > 0 && !c.pts)) return fail(CLC_ERR_INVALID_ARG, bad.c_str());
  return CLC_OK;
}

// The host form's arrays staged into `a`: they start at image 0 and, rebased, at corner 0 and point 0.  not_kept [n_images]: the
// status of the images outside every problem.  Returns the corners on the device, for the lift.
template <class Args>
const float* stage_joint_arrays(Staging& st, const JointArrays& c, const std::vector<long long>& crel, const std::vector<long long>& prel,
                                size_t M, size_t N, const int32_t* not_kept, Args& a) {
  const size_t n = c.n_images, np = c.n_problems;
  const size_t n_off = n > 0 ? n + 1 : 0;  // a call without images sends no offsets
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  const float* corners_dev = st.in(M > 0 ? c.corners_px + 2 * c.corner_offsets[0] : nullptr, 2 * M);
  a.board = st.in(M > 0 ? c.board_xy + 2 * c.corner_offsets[0] : nullptr, 2 * M);
  a.coff = st.in(crel.data(), n_off);
  a.n_corners = (long long)M;
  a.pts = st.in(N > 0 ? c.pts + 3 * c.pts_offsets[0] : nullptr, 3 * N);
  a.poff = st.in(prel.data(), n_off);
  a.keep = st.in_opt(c.keep, n);
  a.prob_off = st.in_opt(reinterpret_cast<const long long*>(c.problem_offsets), np + 1);
  a.n_images = (long long)n;
  a.q = st.inout(c.q_ca_wxyz, 4 * n);
  a.t = st.inout(c.t_ca, 3 * n);
  a.status = st.inout(c.image_status, n, not_kept);
  a.poses_cl = st.inout(c.poses_cl, 7 * np);
  a.summaries = st.out(c.summaries, np);
  a.H_cl = st.out_opt(c.H_cl, 36 * np);
  a.cost_parts = st.out_opt(c.cost_parts, 2 * np);
  return corners_dev;
}

// The device form's refusals after the options.
inline int joint_device_checks(const char* who, clc_handle* h, const JointArrays& c) {
  if (!h || (c.n_images > 0 && (!c.corner_offsets || !c.pts_offsets || !c.q_ca_wxyz || !c.t_ca || !c.image_status)) ||
      (c.n_problems > 0 && (!c.poses_cl || !c.summaries)))
    return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": bad argument").c_str());
  return problem_count_checks(who, c.n_images, c.problem_offsets != nullptr, c.n_problems);
}

// The device form's arrays named in `a`, indexed by the absolute offsets.
template <class Args>
void name_joint_arrays(const JointArrays& c, Args& a) {
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  a.board = c.board_xy;
  a.coff = reinterpret_cast<const long long*>(c.corner_offsets);
  a.pts = c.pts;
  a.poff = reinterpret_cast<const long long*>(c.pts_offsets);
  a.keep = c.keep;
  a.prob_off = reinterpret_cast<const long long*>(c.problem_offsets);
  a.n_images = (long long)c.n_images;
  a.q = c.q_ca_wxyz;
  a.t = c.t_ca;
  a.status = c.image_status;
  a.poses_cl = c.poses_cl;
  a.summaries = c.summaries;
  a.H_cl = c.H_cl;
  a.cost_parts = c.cost_parts;
}

}  // namespace clc_abi
