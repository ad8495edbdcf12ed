// clc_robustpose.hpp — K16: robust board poses.  A consensus over the tags of an image ahead of K10's planar PnP (clc_campose.hpp),
// the protection the reference left commented out (cv::solvePnPRansac beside cv::solvePnP, src/calcCamPose.cpp:226-227): one
// AprilTag decoded with a wrong id, or one mis-refined corner, otherwise enters the least-squares fit of its image unopposed.
//
//   hypotheses   group g of an image = its corners 4g .. 4g+3 (one tag, the order FindTargetCorner emits them); the four planar
//                correspondences of a tag fix a homography in closed form: H_g = S(lifted quad) adj(S(board quad)), S the
//                unit-square -> quad map.  No sampling: the hypothesis set is deterministic.
//   score        every corner of the image under every H_g: e = |H_g X / w - x|^2; inlier iff e finite, e < hyp_threshold^2 and w on
//                the side of the group's first corner; count_g, cost_g = sum min(e, hyp_threshold^2) in corner order.  The winner:
//                largest count, then smallest cost, then smallest g.
//   fit          board_pose_image (K10, unchanged) on the winner's inliers, compacted in corner order
//   re-gate      every corner against the fitted pose, gate `threshold`; refit until the set stops changing (at most max_fits fits)
//
// Every product and sum of the hypothesis, the score and the re-gate is rounded on its own (rn_mul / rn_add / rn_sub; IEEE divisions),
// so the counts, the costs and the winner are those of the sequential restatement tests/robustpose_ref.py, bit for bit.
//
//   tag_consensus_kernel       one wave per image, ONE HYPOTHESIS PER LANE (H_g in registers; groups beyond 64 in chunks of 64, the
//                              best (count, cost, g) carried); the corner loop runs over wave-uniform addresses and holds no
//                              reduction, so a lane's cost is the sequential sum; a wave arg-max on the total order picks the winner.
//                              Then the lanes go over the corners with the winner's H (the same arithmetic), write the mask and copy
//                              the inliers, ranked by ballot + popcount, into the image's own slot of two scratch arrays.
//   board_pose_subset_kernel   a twin of board_pose_kernel on that slot, for the images whose refit flag is up
//   pose_rescore_kernel        one wave per image, lanes over corners: the re-gate, the comparison with the previous mask by ballot,
//                              the re-compaction, the refit flag and the terminal statuses
//
// FP64, fixed order, no atomics, no read-back between the launches.  The per-corner pieces are CLC_HD: tests/shim/robustpose_shim.cpp
// compiles them (and the sequential per-image drivers at the end of this header) for the host with g++.
// Included by abi_campose.hip only.
#pragma once
#include "clc_campose.hpp"

namespace clc {
namespace rp {

CLC_HD double rn_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}
CLC_HD double rn_add(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(a, b);
#else
  return a + b;
#endif
}
CLC_HD double rn_sub(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsub_rn(a, b);
#else
  return a - b;
#endif
}

// The closed-form map of the unit square (0,0) (1,0) (1,1) (0,1) onto the quad p = x0 y0 x1 y1 x2 y2 x3 y3, row-major in S[9]
// (S[8] = 1); returns its denominator d1 x d2 (zero: three corners of the quad are collinear).
CLC_HD double square_to_quad(const double* p, double* S) {
  const double x0 = p[0], y0 = p[1], x1 = p[2], y1 = p[3], x2 = p[4], y2 = p[5], x3 = p[6], y3 = p[7];
  const double sx = rn_sub(rn_add(rn_sub(x0, x1), x2), x3), sy = rn_sub(rn_add(rn_sub(y0, y1), y2), y3);
  const double d1x = rn_sub(x1, x2), d1y = rn_sub(y1, y2), d2x = rn_sub(x3, x2), d2y = rn_sub(y3, y2);
  const double den = rn_sub(rn_mul(d1x, d2y), rn_mul(d1y, d2x));
  const double g = rn_sub(rn_mul(sx, d2y), rn_mul(sy, d2x)) / den;
  const double h = rn_sub(rn_mul(d1x, sy), rn_mul(d1y, sx)) / den;
  S[0] = rn_add(rn_sub(x1, x0), rn_mul(g, x1)); S[1] = rn_add(rn_sub(x3, x0), rn_mul(h, x3)); S[2] = x0;
  S[3] = rn_add(rn_sub(y1, y0), rn_mul(g, y1)); S[4] = rn_add(rn_sub(y3, y0), rn_mul(h, y3)); S[5] = y0;
  S[6] = g; S[7] = h; S[8] = 1.0;
  return den;
}

// H = S(lifted quad) adj(S(board quad)): board plane -> normalized image plane, up to scale.  No pivoting, no iteration.
// *w0 = the projective depth of the group's first corner.  False: either denominator zero or not finite, or an entry of H not finite.
CLC_HD bool tag_hypothesis(const double* quad_lifted, const double* quad_board, double* H, double* w0) {
  double Si[9], Sb[9], A[9];
  const double den_i = square_to_quad(quad_lifted, Si), den_b = square_to_quad(quad_board, Sb);
  const double a = Sb[0], b = Sb[1], c = Sb[2], d = Sb[3], e = Sb[4], f = Sb[5], g = Sb[6], h = Sb[7], i = Sb[8];
  A[0] = rn_sub(rn_mul(e, i), rn_mul(f, h)); A[1] = rn_sub(rn_mul(c, h), rn_mul(b, i)); A[2] = rn_sub(rn_mul(b, f), rn_mul(c, e));
  A[3] = rn_sub(rn_mul(f, g), rn_mul(d, i)); A[4] = rn_sub(rn_mul(a, i), rn_mul(c, g)); A[5] = rn_sub(rn_mul(c, d), rn_mul(a, f));
  A[6] = rn_sub(rn_mul(d, h), rn_mul(e, g)); A[7] = rn_sub(rn_mul(b, g), rn_mul(a, h)); A[8] = rn_sub(rn_mul(a, e), rn_mul(b, d));
  bool ok = isfinite(den_i) && isfinite(den_b) && den_i != 0.0 && den_b != 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double v = rn_add(rn_add(rn_mul(Si[3 * r], A[k]), rn_mul(Si[3 * r + 1], A[3 + k])), rn_mul(Si[3 * r + 2], A[6 + k]));
      H[3 * r + k] = v;
      ok = ok && isfinite(v);
    }
  *w0 = rn_add(rn_add(rn_mul(H[6], quad_board[0]), rn_mul(H[7], quad_board[1])), H[8]);
  return ok;
}

// Corner (x, y) <-> board point (X, Y) under H: returns min(e, thr2) (thr2 for a non-finite e), *inlier as in the header comment.
CLC_HD double tag_score(const double* H, double w0, double X, double Y, double x, double y, double thr2, bool* inlier) {
  const double u = rn_add(rn_add(rn_mul(H[0], X), rn_mul(H[1], Y)), H[2]);
  const double v = rn_add(rn_add(rn_mul(H[3], X), rn_mul(H[4], Y)), H[5]);
  const double w = rn_add(rn_add(rn_mul(H[6], X), rn_mul(H[7], Y)), H[8]);
  const double du = rn_sub(u / w, x), dv = rn_sub(v / w, y);
  const double e = rn_add(rn_mul(du, du), rn_mul(dv, dv));
  const bool below = isfinite(e) && e < thr2;
  *inlier = below && rn_mul(w, w0) > 0.0;
  return below ? e : thr2;
}

// The total order of the hypotheses: a before b.  An invalid group carries count -1.
CLC_HD bool tag_better(int count_a, double cost_a, int g_a, int count_b, double cost_b, int g_b) {
  if (count_a != count_b) return count_a > count_b;
  if (cost_a != cost_b) return cost_a < cost_b;
  return g_a < g_b;
}

// The re-gate of one corner under the fitted pose: P = R (X, Y, 0) + t in front, e = |P_xy / P_z - x|^2 finite and below thr2.
CLC_HD bool pose_gate(const double* R, const double* t, double X, double Y, double x, double y, double thr2) {
  const double P0 = rn_add(rn_add(rn_mul(R[0], X), rn_mul(R[1], Y)), t[0]);
  const double P1 = rn_add(rn_add(rn_mul(R[3], X), rn_mul(R[4], Y)), t[1]);
  const double P2 = rn_add(rn_add(rn_mul(R[6], X), rn_mul(R[7], Y)), t[2]);
  const double du = rn_sub(P0 / P2, x), dv = rn_sub(P1 / P2, y);
  const double e = rn_add(rn_mul(du, du), rn_mul(dv, dv));
  return P2 > 0.0 && isfinite(e) && e < thr2;
}

// The rotation of an output quaternion (w, x, y, z).
CLC_HD void rot_of_wxyz(const double* q_wxyz, double* R) {
  const double q[4] = {q_wxyz[1], q_wxyz[2], q_wxyz[3], q_wxyz[0]};
  quat_to_rot(q, R);
}

// What follows a re-gate, in this order: the set is the one just fitted — done; too small — no consensus; the fits are used up — done
// with the last fit; otherwise a refit on the new set.
constexpr int RESCORE_DONE = 0, RESCORE_REFIT = 1, RESCORE_LOST = 2;
CLC_HD int rescore_decide(bool changed, int total, int min_inliers, int n_fits, int max_fits) {
  if (!changed) return RESCORE_DONE;
  if (total < min_inliers) return RESCORE_LOST;
  if (n_fits >= max_fits) return RESCORE_DONE;
  return RESCORE_REFIT;
}

#if defined(__HIPCC__)

// lanes [0, lane) of a ballot
__device__ __forceinline__ int rank_below(unsigned long long ballot, int lane) { return __popcll(ballot & ((1ull << lane) - 1ull)); }

__device__ __forceinline__ void zero_mask(unsigned char* __restrict__ mask, long long n) {
  for (long long k = threadIdx.x; k < n; k += 64) mask[k] = 0;
}

// The outputs of an image that ends without a pose at status st (lead lane).
__device__ __forceinline__ void image_without_pose(int st, long long img, double* q, double* t, double* rms, int32_t* status,
                                                   clc_summary* summaries, int32_t* cnt, int32_t* flag) {
  cp::board_pose_store(st, nullptr, 0.0, img, q, t, rms, status);
  if (summaries) cp::summary_empty(summaries[img]);
  cnt[img] = 0;
  flag[img] = 0;
}

// One 64-thread workgroup (one wave) per image.  lifted: campose_lift_kernel<true>'s output for the corners [first, off[n_images])
// (lifted[0] is corner `first`); board and mask indexed by the absolute offsets; sub_l / sub_b indexed like lifted: the image's
// inliers go to [off[img] - first, off[img] - first + cnt[img]).  flag[img] = 1: the image wants a fit.
static __global__ __launch_bounds__(64) void tag_consensus_kernel(
    const float* __restrict__ lifted, const float* __restrict__ board, const long long* __restrict__ off, const long long first,
    const double hyp_threshold, const int min_inliers, unsigned char* __restrict__ mask, float* __restrict__ sub_l,
    float* __restrict__ sub_b, int32_t* __restrict__ cnt, int32_t* __restrict__ flag, int32_t* __restrict__ n_fits,
    int32_t* __restrict__ best_group, double* __restrict__ q_wxyz, double* __restrict__ t, double* __restrict__ rms,
    int32_t* __restrict__ status, clc_summary* __restrict__ summaries) {
  const int lane = threadIdx.x;
  const long long img = blockIdx.x;
  const long long b = off[img], n = off[img + 1] - b, s = b - first;
  const float* __restrict__ L = lifted + 2 * s;
  const float* __restrict__ B = board + 2 * b;
  const double thr2 = rn_mul(hyp_threshold, hyp_threshold);
  const long long G = n > 0 ? n / 4 : 0;
  int bc = -1, bg = -1;  // the best so far: count, group
  double bs = 0.0, w0b = 0.0, Hb[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Hb[i] = 0.0;
  for (long long base = 0; base < G; base += 64) {
    const long long g = base + lane;
    double H[9], w0 = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
    bool valid = false;
    if (g < G) {
      double pl[8], pb[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        pl[i] = (double)L[8 * g + i];
        pb[i] = (double)B[8 * g + i];
      }
      valid = tag_hypothesis(pl, pb, H, &w0);
    }
    int count = 0;
    double cost = 0.0;
    for (long long k = 0; k < n; ++k) {  // wave-uniform addresses; no reduction: the lane's sum is the sequential one
      bool in;
      const double e = tag_score(H, w0, (double)B[2 * k], (double)B[2 * k + 1], (double)L[2 * k], (double)L[2 * k + 1], thr2, &in);
      cost = rn_add(cost, e);
      count += in ? 1 : 0;
    }
    int c = valid ? count : -1, gg = (int)g;
    double sc = cost;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {  // arg-max on a total order: every lane ends with the same triple
      const int oc = __shfl_xor(c, d, 64), og = __shfl_xor(gg, d, 64);
      const double os = __shfl_xor(sc, d, 64);
      if (tag_better(oc, os, og, c, sc, gg)) { c = oc; sc = os; gg = og; }
    }
    if (c >= 0 && (bc < 0 || tag_better(c, sc, gg, bc, bs, bg))) {  // wave-uniform
      bc = c; bs = sc; bg = gg;
      const int wl = (int)(gg - base);
#pragma unroll
      for (int i = 0; i < 9; ++i) Hb[i] = __shfl(H[i], wl, 64);
      w0b = __shfl(w0, wl, 64);
    }
  }
  if (bc < min_inliers) {  // no valid group, or too small a set
    zero_mask(mask + b, n);
    if (lane == 0) {
      image_without_pose(CLC_POSE_NO_CONSENSUS, img, q_wxyz, t, rms, status, summaries, cnt, flag);
      n_fits[img] = 0;
      if (best_group) best_group[img] = -1;
    }
    return;
  }
  int run = 0;
  for (long long k0 = 0; k0 < n; k0 += 64) {
    const long long k = k0 + lane;
    bool in = false;
    float lx = 0.f, ly = 0.f, bx = 0.f, by = 0.f;
    if (k < n) {
      lx = L[2 * k]; ly = L[2 * k + 1]; bx = B[2 * k]; by = B[2 * k + 1];
      (void)tag_score(Hb, w0b, (double)bx, (double)by, (double)lx, (double)ly, thr2, &in);
      mask[b + k] = in ? 1 : 0;
    }
    const unsigned long long m = __ballot(in);
    if (in) {
      const long long r = s + run + rank_below(m, lane);
      sub_l[2 * r] = lx; sub_l[2 * r + 1] = ly; sub_b[2 * r] = bx; sub_b[2 * r + 1] = by;
    }
    run += __popcll(m);
  }
  if (lane == 0) {
    cnt[img] = run;
    flag[img] = 1;
    n_fits[img] = 0;
    if (best_group) best_group[img] = bg;
  }
}

// board_pose_kernel on the image's slot of the compacted arrays, for the images whose flag is up; counts the fit.
static __global__ __launch_bounds__(64) void board_pose_subset_kernel(
    const clc_options opt, const float* __restrict__ sub_l, const float* __restrict__ sub_b, const long long* __restrict__ off,
    const long long first, const int32_t* __restrict__ flag, const int32_t* __restrict__ cnt, int32_t* __restrict__ n_fits,
    double* __restrict__ q_wxyz, double* __restrict__ t, double* __restrict__ rms, int32_t* __restrict__ status,
    clc_summary* __restrict__ summaries) {
  __shared__ cp::PoseShared sh;
  const long long img = blockIdx.x;
  if (flag[img] == 0) return;
  const long long s = off[img] - first, n = cnt[img];
  double pose7[7], r = 0.0;
  const int st = cp::board_pose_image(opt, sub_l + 2 * s, sub_b + 2 * s, n, sh, pose7, &r);
  if (threadIdx.x == 0) {
    cp::board_pose_store(st, pose7, r, img, q_wxyz, t, rms, status);
    if (summaries) {
      if (st == CLC_POSE_OK) summaries[img] = sh.sm;
      else cp::summary_empty(summaries[img]);
    }
    n_fits[img] += 1;
  }
}

// The re-gate of the images whose flag is up, after their fit.
static __global__ __launch_bounds__(64) void pose_rescore_kernel(
    const float* __restrict__ lifted, const float* __restrict__ board, const long long* __restrict__ off, const long long first,
    const double threshold, const int min_inliers, const int max_fits, unsigned char* __restrict__ mask, float* __restrict__ sub_l,
    float* __restrict__ sub_b, int32_t* __restrict__ cnt, int32_t* __restrict__ flag, const int32_t* __restrict__ n_fits,
    double* __restrict__ q_wxyz, double* __restrict__ t, double* __restrict__ rms, int32_t* __restrict__ status,
    clc_summary* __restrict__ summaries) {
  const int lane = threadIdx.x;
  const long long img = blockIdx.x;
  if (flag[img] == 0) return;
  const long long b = off[img], n = off[img + 1] - b, s = b - first;
  if (status[img] != CLC_POSE_OK) {  // the fit failed: the image ends with its status (pose_store wrote the empty pose)
    zero_mask(mask + b, n);
    if (lane == 0) { cnt[img] = 0; flag[img] = 0; }
    return;
  }
  const float* __restrict__ L = lifted + 2 * s;
  const float* __restrict__ B = board + 2 * b;
  const double thr2 = rn_mul(threshold, threshold);
  double R[9];
  const double qq[4] = {q_wxyz[4 * img], q_wxyz[4 * img + 1], q_wxyz[4 * img + 2], q_wxyz[4 * img + 3]};
  const double tt[3] = {t[3 * img], t[3 * img + 1], t[3 * img + 2]};
  rot_of_wxyz(qq, R);
  bool changed = false;
  int total = 0;
  for (long long k0 = 0; k0 < n; k0 += 64) {
    const long long k = k0 + lane;
    bool in = false, old = false;
    if (k < n) {
      in = pose_gate(R, tt, (double)B[2 * k], (double)B[2 * k + 1], (double)L[2 * k], (double)L[2 * k + 1], thr2);
      old = mask[b + k] != 0;
    }
    changed = changed || __ballot(in != old) != 0ull;
    total += __popcll(__ballot(in));
  }
  const int what = rescore_decide(changed, total, min_inliers, n_fits[img], max_fits);
  if (what == RESCORE_DONE) {
    if (lane == 0) flag[img] = 0;
    return;
  }
  if (what == RESCORE_LOST) {
    zero_mask(mask + b, n);
    if (lane == 0) image_without_pose(CLC_POSE_NO_CONSENSUS, img, q_wxyz, t, rms, status, summaries, cnt, flag);
    return;
  }
  int run = 0;
  for (long long k0 = 0; k0 < n; k0 += 64) {
    const long long k = k0 + lane;
    bool in = false;
    float lx = 0.f, ly = 0.f, bx = 0.f, by = 0.f;
    if (k < n) {
      lx = L[2 * k]; ly = L[2 * k + 1]; bx = B[2 * k]; by = B[2 * k + 1];
      in = pose_gate(R, tt, (double)bx, (double)by, (double)lx, (double)ly, thr2);
      mask[b + k] = in ? 1 : 0;
    }
    const unsigned long long m = __ballot(in);
    if (in) {
      const long long r = s + run + rank_below(m, lane);
      sub_l[2 * r] = lx; sub_l[2 * r + 1] = ly; sub_b[2 * r] = bx; sub_b[2 * r + 1] = by;
    }
    run += __popcll(m);
  }
  if (lane == 0) cnt[img] = run;
}

#else  // the host build: one image at a time, the lanes as loops

// tag_consensus_kernel for one image: mask[n], sub_l / sub_b [2 n] (the image's slot).  Returns the winner's count (the size of the
// first set) or -1 when no group is valid; *best_group = the winner or -1.  counts / costs (nullable): per group, count -1 = invalid.
inline int consensus_image(const float* L, const float* B, long long n, double hyp_threshold, unsigned char* mask, float* sub_l,
                           float* sub_b, int* best_group, int* counts, double* costs) {
  const double thr2 = rn_mul(hyp_threshold, hyp_threshold);
  const long long G = n > 0 ? n / 4 : 0;
  int bc = -1, bg = -1;
  double bs = 0.0, w0b = 0.0, Hb[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long long g = 0; g < G; ++g) {
    double pl[8], pb[8], H[9], w0 = 0.0;
    for (int i = 0; i < 8; ++i) { pl[i] = (double)L[8 * g + i]; pb[i] = (double)B[8 * g + i]; }
    const bool valid = tag_hypothesis(pl, pb, H, &w0);
    int count = 0;
    double cost = 0.0;
    for (long long k = 0; k < n; ++k) {
      bool in;
      const double e = tag_score(H, w0, (double)B[2 * k], (double)B[2 * k + 1], (double)L[2 * k], (double)L[2 * k + 1], thr2, &in);
      cost = rn_add(cost, e);
      count += in ? 1 : 0;
    }
    if (counts) counts[g] = valid ? count : -1;
    if (costs) costs[g] = cost;
    if (valid && (bc < 0 || tag_better(count, cost, (int)g, bc, bs, bg))) {
      bc = count; bs = cost; bg = (int)g; w0b = w0;
      for (int i = 0; i < 9; ++i) Hb[i] = H[i];
    }
  }
  *best_group = bg;
  long long run = 0;
  for (long long k = 0; k < n; ++k) {
    bool in = false;
    if (bg >= 0) (void)tag_score(Hb, w0b, (double)B[2 * k], (double)B[2 * k + 1], (double)L[2 * k], (double)L[2 * k + 1], thr2, &in);
    mask[k] = in ? 1 : 0;
    if (in) {
      sub_l[2 * run] = L[2 * k]; sub_l[2 * run + 1] = L[2 * k + 1]; sub_b[2 * run] = B[2 * k]; sub_b[2 * run + 1] = B[2 * k + 1];
      ++run;
    }
  }
  return bc;
}

// pose_rescore_kernel for one image after a fit that ended CLC_POSE_OK: RESCORE_*; on RESCORE_REFIT mask / sub_l / sub_b hold the new
// set and *cnt its size; otherwise they are left as they are.
inline int rescore_image(const double* q_wxyz, const double* t, const float* L, const float* B, long long n, double threshold,
                         int min_inliers, int n_fits, int max_fits, unsigned char* mask, float* sub_l, float* sub_b, int* cnt) {
  const double thr2 = rn_mul(threshold, threshold);
  double R[9];
  rot_of_wxyz(q_wxyz, R);
  bool changed = false;
  int total = 0;
  for (long long k = 0; k < n; ++k) {
    const bool in = pose_gate(R, t, (double)B[2 * k], (double)B[2 * k + 1], (double)L[2 * k], (double)L[2 * k + 1], thr2);
    changed = changed || in != (mask[k] != 0);
    total += in ? 1 : 0;
  }
  const int what = rescore_decide(changed, total, min_inliers, n_fits, max_fits);
  if (what != RESCORE_REFIT) return what;
  long long run = 0;
  for (long long k = 0; k < n; ++k) {
    const bool in = pose_gate(R, t, (double)B[2 * k], (double)B[2 * k + 1], (double)L[2 * k], (double)L[2 * k + 1], thr2);
    mask[k] = in ? 1 : 0;
    if (in) {
      sub_l[2 * run] = L[2 * k]; sub_l[2 * run + 1] = L[2 * k + 1]; sub_b[2 * run] = B[2 * k]; sub_b[2 * run + 1] = B[2 * k + 1];
      ++run;
    }
  }
  *cnt = (int)run;
  return what;
}

#endif

}  // namespace rp
}  // namespace clc
