// clc_altpose.hpp — K17: the second minimum of the planar fit.  The reprojection cost of a plane has two local minima, the true pose
// and its mirror about the line of sight (Schweighofer-Pinz / IPPE); K10 (clc_campose.hpp) returns the one its DLT start leads to.
// Given the poses of clc_board_poses / clc_board_poses_robust this finds, per image, the other minimum and how close its cost is.
//
//   set          the corners with inlier != 0, compacted in corner order (all of them without a mask), after K10's lift
//   mirror start c = R Xbar + t (Xbar: the set's mean board point), s = c / |c|, R' = (I - 2 s s^T) R diag(1, 1, -1), t' = c - R' Xbar:
//                the centroid stays, every corner's offset from it is reflected through the plane perpendicular to the line of
//                sight — the same image under weak perspective
//   fit          K10's LM stage alone from (R', t'): board_pose_refine, a twin of the loop of cp::board_pose_image (which is left
//                as it is: board_pose_kernel and board_pose_subset_kernel keep their bits and their resource figures)
//   costs        cost_in = 1/2 sum |r|^2 of the input pose on the compacted set through reproj_accumulate, in the lane assignment and
//                summation order of the fit's own evaluations; cost_alt = the fit's final cost
//   kind         rot_angle = angle of R^T R_alt < same_angle: the start fell back into the input's minimum (SAME), else DISTINCT
//
//   alt_start_kernel              one wave per image: the set's compaction into the image's own slot of two scratch arrays (ballot +
//                                 popcount), the centroid by wave all-reduce, the mirror start on lane 0; writes the outputs of the
//                                 images that end CLC_ALT_NONE here
//   board_pose_from_start_kernel  one wave per image whose flag is up: cost_in on the slot, board_pose_refine from the stored start,
//                                 the classification, the outputs
//
// FP64, fixed order, no atomics, no read-back between the launches.  The per-image pieces are CLC_HD: tests/shim/altpose_shim.cpp
// compiles them (and the sequential per-image driver at the end of this header) for the host with g++.
// Included by abi_campose.hip only.
#pragma once
#include "clc_robustpose.hpp"

namespace clc {
namespace ap {

// What the call leaves per image (every pointer but kind nullable).
struct AltOut {
  double *q, *t, *rms, *cost_in, *cost_alt, *ratio, *rot_angle, *normal_angle;
  int32_t* kind;
  uint8_t *ambiguous, *better;
  clc_summary* summaries;
};

// The mirror start and its rotation, where lane 0 builds them (rot_to_quat_xyzw indexes its matrix at run time: memory, not registers).
struct AltStartShared {
  double R[9];
  double x0[7];
  int32_t ok;
};

CLC_HD bool finite4(float a, float b, float c, float d) { return isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d); }

// The outputs of an image that ends CLC_ALT_NONE (lead lane / host).
CLC_HD void alt_store_none(long long img, const AltOut& o) {
  const double nan = __builtin_nan("");
  o.kind[img] = CLC_ALT_NONE;
  if (o.q) { o.q[4 * img] = 1.0; o.q[4 * img + 1] = 0.0; o.q[4 * img + 2] = 0.0; o.q[4 * img + 3] = 0.0; }
  if (o.t) { o.t[3 * img] = 0.0; o.t[3 * img + 1] = 0.0; o.t[3 * img + 2] = 0.0; }
  if (o.rms) o.rms[img] = nan;
  if (o.cost_in) o.cost_in[img] = nan;
  if (o.cost_alt) o.cost_alt[img] = nan;
  if (o.ratio) o.ratio[img] = nan;
  if (o.rot_angle) o.rot_angle[img] = nan;
  if (o.normal_angle) o.normal_angle[img] = nan;
  if (o.ambiguous) o.ambiguous[img] = 0;
  if (o.better) o.better[img] = 0;
  if (o.summaries) cp::summary_empty(o.summaries[img]);
}

// (R', t') of the header comment from (R, t) and the set's mean board point (Xb, Yb, 0): Rm[9] and x0 = [t', qx, qy, qz, qw] in
// memory.  False: c is zero or not finite, or the start is not finite.
CLC_HD bool mirror_start(const double* R, const double* t, double Xb, double Yb, double* Rm, double* x0) {
  CLC_BF_NO_CONTRACT
  const double c0 = (R[0] * Xb + R[1] * Yb) + t[0], c1 = (R[3] * Xb + R[4] * Yb) + t[1], c2 = (R[6] * Xb + R[7] * Yb) + t[2];
  const double nn = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
  if (!(isfinite(nn) && nn > 0.0)) return false;
  const double s[3] = {c0 / nn, c1 / nn, c2 / nn};
  double M[9];  // R diag(1, 1, -1)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    M[3 * i] = R[3 * i];
    M[3 * i + 1] = R[3 * i + 1];
    M[3 * i + 2] = -R[3 * i + 2];
  }
  double w[3];  // s^T M
#pragma unroll
  for (int j = 0; j < 3; ++j) w[j] = (s[0] * M[j] + s[1] * M[3 + j]) + s[2] * M[6 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rm[3 * i + j] = M[3 * i + j] - (2.0 * s[i]) * w[j];
  x0[0] = c0 - (Rm[0] * Xb + Rm[1] * Yb);
  x0[1] = c1 - (Rm[3] * Xb + Rm[4] * Yb);
  x0[2] = c2 - (Rm[6] * Xb + Rm[7] * Yb);
  bf::rot_to_quat_xyzw(Rm, x0 + 3);
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 7; ++i) ok = ok && isfinite(x0[i]);
  return ok;
}

// K10's LM stage alone: the loop of cp::board_pose_image from the start pose x0 = [t, qx, qy, qz, qw] (memory every lane can read),
// on the K = I reprojection error of lifted[2n] / board[2n], the same options, the same reproj_accumulate and the same rule for a
// point behind the camera.  Every lane calls it (device: the image's wave; host: once).  Returns CLC_POSE_OK or CLC_POSE_NONFINITE
// (wave-uniform); on CLC_POSE_OK pose7, *rms and sh.sm are set.
CLC_HD int board_pose_refine(const clc_options& o, const float* __restrict__ lifted, const float* __restrict__ board, long long n,
                             cp::PoseShared& sh, const double* x0, double* pose7, double* rms) {
  CLC_BF_NO_CONTRACT
  if (bf::lead_lane()) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      sh.x0[i] = x0[i];
      ok = ok && isfinite(sh.x0[i]);
    }
    sh.status = ok ? CLC_POSE_OK : CLC_POSE_NONFINITE;
    if (ok) lm_init(sh.st, o, sh.x0);
  }
  cp::wave_barrier();
  if (sh.status != CLC_POSE_OK) return CLC_POSE_NONFINITE;
  while (sh.st.status == CLC_RUNNING) {
    double xe[7], R[9];
#pragma unroll
    for (int i = 0; i < 7; ++i) xe[i] = sh.st.x_eval[i];
    quat_to_rot(xe + 3, R);
    double e[28];
    cp::wave_sum<28>([&](int lane, double* a) {
      for (long long k = lane; k < n; k += cp::POSE_LANES)
        cp::reproj_accumulate(R, xe, board[2 * k], board[2 * k + 1], lifted[2 * k], lifted[2 * k + 1], a);
    }, e);
    cp::wave_barrier();
    if (bf::lead_lane()) {
#pragma unroll
      for (int i = 0; i < 28; ++i) sh.e[i] = e[i];
      lm_advance(sh.st, sh.w, o, nullptr, 0, 0.5 * sh.e[27], sh.e + 21, sh.e);
    }
    cp::wave_barrier();
  }
  if (bf::lead_lane()) lm_fill_summary(sh.st, sh.sm);
  cp::wave_barrier();
#pragma unroll
  for (int i = 0; i < 7; ++i) pose7[i] = sh.st.x_out[i];
  const double fc = sh.sm.final_cost;
  bool finite = isfinite(fc) && sh.st.status != CLC_FAILURE;
#pragma unroll
  for (int i = 0; i < 7; ++i) finite = finite && isfinite(pose7[i]);
  if (!finite) return CLC_POSE_NONFINITE;
  *rms = sqrt(2.0 * fc / (double)n);
  return CLC_POSE_OK;
}

// cost_in: 1/2 sum |r|^2 of the pose (R, t) over the compacted set lifted[2n] / board[2n], each lane over the corners lane, lane + 64,
// ... and a wave all-reduce — one evaluation of the fit, lane for lane (infinite when a corner lies behind the camera).
CLC_HD double set_cost(const double* R, const double* t, const float* __restrict__ lifted, const float* __restrict__ board, long long n) {
  double e[28];
  cp::wave_sum<28>([&](int lane, double* a) {
    for (long long k = lane; k < n; k += cp::POSE_LANES)
      cp::reproj_accumulate(R, t, board[2 * k], board[2 * k + 1], lifted[2 * k], lifted[2 * k + 1], a);
  }, e);
  return 0.5 * e[27];
}

// The sum of the set's board points: each lane over the image's corners lane, lane + 64, ... that the mask keeps (the original order:
// nothing the wave has just written is read back), and a wave all-reduce.
CLC_HD void set_board_sum(const float* __restrict__ board, const unsigned char* __restrict__ mask, long long n, double* sum2) {
  cp::wave_sum<2>([&](int lane, double* a) {
    for (long long k = lane; k < n; k += cp::POSE_LANES)
      if (!mask || mask[k] != 0) {
        a[0] += (double)board[2 * k];
        a[1] += (double)board[2 * k + 1];
      }
  }, sum2);
}

// The angle of the rotation A^T B (atan2 of the norm of its skew part and its trace: good at both ends of [0, pi]).
CLC_HD double rotation_angle(const double* A, const double* B) {
  CLC_BF_NO_CONTRACT
  double D[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) D[3 * i + j] = (A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j];
  const double a = D[7] - D[5], b = D[2] - D[6], c = D[3] - D[1];
  return atan2(sqrt((a * a + b * b) + c * c), ((D[0] + D[4]) + D[8]) - 1.0);
}

// The angle between the third columns of A and B (the board's normal in the camera frame).
CLC_HD double normal_angle_of(const double* A, const double* B) {
  CLC_BF_NO_CONTRACT
  const double a[3] = {A[2], A[5], A[8]}, b[3] = {B[2], B[5], B[8]};
  double x[3];
  bf::cross3(a, b, x);
  return atan2(sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]);
}

// Steps 4-6 for an image whose fit ended CLC_POSE_OK (lead lane / host): the classification against the input rotation R_in and the
// outputs.  pose7 = [t, qx, qy, qz, qw] of the fit, cin = cost_in.
CLC_HD void alt_store_fit(const clc_alt_pose_options& ao, const double* R_in, const double* pose7, double rms, double cin,
                          const clc_summary& sm, long long img, const AltOut& o) {
  double R_alt[9];
  quat_to_rot(pose7 + 3, R_alt);
  const double calt = sm.final_cost;
  const double ra = rotation_angle(R_in, R_alt), na = normal_angle_of(R_in, R_alt);
  const double ratio = (cin != 0.0 && isfinite(cin) && isfinite(calt)) ? calt / cin : __builtin_nan("");
  const bool distinct = !(ra < ao.same_angle);
  o.kind[img] = distinct ? CLC_ALT_DISTINCT : CLC_ALT_SAME;
  if (o.q) {
    const double sgn = pose7[6] < 0.0 ? -1.0 : 1.0;
    o.q[4 * img] = sgn * pose7[6];
    o.q[4 * img + 1] = sgn * pose7[3];
    o.q[4 * img + 2] = sgn * pose7[4];
    o.q[4 * img + 3] = sgn * pose7[5];
  }
  if (o.t)
    for (int i = 0; i < 3; ++i) o.t[3 * img + i] = pose7[i];
  if (o.rms) o.rms[img] = rms;
  if (o.cost_in) o.cost_in[img] = cin;
  if (o.cost_alt) o.cost_alt[img] = calt;
  if (o.ratio) o.ratio[img] = ratio;
  if (o.rot_angle) o.rot_angle[img] = ra;
  if (o.normal_angle) o.normal_angle[img] = na;
  if (o.ambiguous) o.ambiguous[img] = (distinct && ratio < ao.ratio_gate) ? 1 : 0;
  if (o.better) o.better[img] = (distinct && calt < cin) ? 1 : 0;
  if (o.summaries) o.summaries[img] = sm;
}

#if defined(__HIPCC__)

// One 64-thread workgroup (one wave) per image.  lifted: campose_lift_kernel<true>'s output for the corners [first, off[n_images])
// (lifted[0] is corner `first`); board and inlier (nullable) indexed by the absolute offsets; sub_l / sub_b indexed like lifted: the
// image's set goes to [off[img] - first, off[img] - first + cnt[img]).  flag[img] = 1: the image wants its fit, from start7[7 img].
static __global__ __launch_bounds__(64) void alt_start_kernel(
    const float* __restrict__ lifted, const float* __restrict__ board, const long long* __restrict__ off, const long long first,
    const unsigned char* __restrict__ inlier, const double* __restrict__ q_in, const double* __restrict__ t_in,
    const int32_t* __restrict__ status_in, float* __restrict__ sub_l, float* __restrict__ sub_b, int32_t* __restrict__ cnt,
    int32_t* __restrict__ flag, double* __restrict__ start7, const AltOut o) {
  __shared__ AltStartShared sh;
  const int lane = threadIdx.x;
  const long long img = blockIdx.x;
  const long long b = off[img], n = off[img + 1] - b, s = b - first;
  const float* __restrict__ L = lifted + 2 * s;
  const float* __restrict__ B = board + 2 * b;
  const unsigned char* __restrict__ mask = inlier ? inlier + b : nullptr;
  bool none = status_in[img] != CLC_POSE_OK;  // wave-uniform
  int run = 0;
  if (!none) {
    bool bad = false;
    for (long long k0 = 0; k0 < n; k0 += 64) {
      const long long k = k0 + lane;
      bool in = false;
      float lx = 0.f, ly = 0.f, bx = 0.f, by = 0.f;
      if (k < n) {
        in = !mask || mask[k] != 0;
        lx = L[2 * k]; ly = L[2 * k + 1]; bx = B[2 * k]; by = B[2 * k + 1];
      }
      bad = bad || __ballot(in && !finite4(lx, ly, bx, by)) != 0ull;
      const unsigned long long m = __ballot(in);
      if (in) {
        const long long r = s + run + rp::rank_below(m, lane);
        sub_l[2 * r] = lx; sub_l[2 * r + 1] = ly; sub_b[2 * r] = bx; sub_b[2 * r + 1] = by;
      }
      run += __popcll(m);
    }
    none = bad || run < 4;
  }
  double R[9], tt[3] = {0.0, 0.0, 0.0};
  if (!none) {
    const double qq[4] = {q_in[4 * img], q_in[4 * img + 1], q_in[4 * img + 2], q_in[4 * img + 3]};
    tt[0] = t_in[3 * img]; tt[1] = t_in[3 * img + 1]; tt[2] = t_in[3 * img + 2];
    rp::rot_of_wxyz(qq, R);
    double sum2[2];
    set_board_sum(B, mask, n, sum2);
    if (lane == 0) sh.ok = mirror_start(R, tt, sum2[0] / (double)run, sum2[1] / (double)run, sh.R, sh.x0) ? 1 : 0;
    __syncthreads();
    none = sh.ok == 0;
  }
  if (none) {
    if (lane == 0) {
      alt_store_none(img, o);
      cnt[img] = 0;
      flag[img] = 0;
    }
    return;
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 7; ++i) start7[7 * img + i] = sh.x0[i];
    cnt[img] = run;
    flag[img] = 1;
  }
}

// For the images whose flag is up: cost_in of the input pose on the image's slot of the compacted arrays, the LM stage on it from the
// stored start, then the classification and the outputs.
static __global__ __launch_bounds__(64) void board_pose_from_start_kernel(
    const clc_options opt, const clc_alt_pose_options aopt, const float* __restrict__ sub_l, const float* __restrict__ sub_b,
    const long long* __restrict__ off, const long long first, const int32_t* __restrict__ flag, const int32_t* __restrict__ cnt,
    const double* __restrict__ start7, const double* __restrict__ q_in, const double* __restrict__ t_in, const AltOut o) {
  __shared__ cp::PoseShared sh;
  const long long img = blockIdx.x;
  if (flag[img] == 0) return;
  const long long s = off[img] - first, n = cnt[img];
  double cin;
  {
    const double qq[4] = {q_in[4 * img], q_in[4 * img + 1], q_in[4 * img + 2], q_in[4 * img + 3]};
    const double tt[3] = {t_in[3 * img], t_in[3 * img + 1], t_in[3 * img + 2]};
    double R_in[9];
    rp::rot_of_wxyz(qq, R_in);
    cin = set_cost(R_in, tt, sub_l + 2 * s, sub_b + 2 * s, n);
  }
  double pose7[7], r = 0.0;
  const int st = board_pose_refine(opt, sub_l + 2 * s, sub_b + 2 * s, n, sh, start7 + 7 * img, pose7, &r);
  if (threadIdx.x == 0) {
    if (st != CLC_POSE_OK) {
      alt_store_none(img, o);
    } else {
      const double qq[4] = {q_in[4 * img], q_in[4 * img + 1], q_in[4 * img + 2], q_in[4 * img + 3]};
      double R_in[9];
      rp::rot_of_wxyz(qq, R_in);
      alt_store_fit(aopt, R_in, pose7, r, cin, sh.sm, img, o);
    }
  }
}

#else  // the host build: one image at a time, the lanes as loops

// Both kernels for one image: L / B its lifted corners and board points [2n], mask (nullable) [n], sub_l / sub_b scratch [2n].
inline void alt_image(const clc_options& opt, const clc_alt_pose_options& ao, const float* L, const float* B, long long n,
                      const unsigned char* mask, const double* q_in, const double* t_in, const int32_t* status_in, long long img,
                      float* sub_l, float* sub_b, cp::PoseShared& psh, const AltOut& o) {
  if (status_in[img] != CLC_POSE_OK) return alt_store_none(img, o);
  long long run = 0;
  bool bad = false;
  for (long long k = 0; k < n; ++k) {
    if (mask && mask[k] == 0) continue;
    bad = bad || !finite4(L[2 * k], L[2 * k + 1], B[2 * k], B[2 * k + 1]);
    sub_l[2 * run] = L[2 * k]; sub_l[2 * run + 1] = L[2 * k + 1]; sub_b[2 * run] = B[2 * k]; sub_b[2 * run + 1] = B[2 * k + 1];
    ++run;
  }
  if (bad || run < 4) return alt_store_none(img, o);
  double R[9], sum2[2];
  const double tt[3] = {t_in[3 * img], t_in[3 * img + 1], t_in[3 * img + 2]};
  rp::rot_of_wxyz(q_in + 4 * img, R);
  set_board_sum(B, mask, n, sum2);
  AltStartShared sh;
  if (!mirror_start(R, tt, sum2[0] / (double)run, sum2[1] / (double)run, sh.R, sh.x0)) return alt_store_none(img, o);
  const double c = set_cost(R, tt, sub_l, sub_b, run);
  double pose7[7], r = 0.0;
  const int st = board_pose_refine(opt, sub_l, sub_b, run, psh, sh.x0, pose7, &r);
  if (st != CLC_POSE_OK) return alt_store_none(img, o);
  alt_store_fit(ao, R, pose7, r, c, psh.sm, img, o);
}

#endif

}  // namespace ap
}  // namespace clc
