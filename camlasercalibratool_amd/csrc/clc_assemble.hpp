// clc_assemble.hpp — K13: the glue of the offline flow, main/calibr_offline.cpp:62-155, between the kernels that already exist
// (TranScanToPoints, K7 board segments, K6 line fit): key-frame thinning of the stamped tag poses, scan -> pose association by
// time stamp, compaction of the scans that have both a segment and a pose, the gather of their points into the handle's pose-major
// arrays (with the tag pose Twc -> (Qca, tca) of :145-146), and the two points on the fitted line (:126-142).
// FP64, fixed order, no atomics: the observations come out in scan order and a second run gives the same bits.
// A scan whose segment status is SEG_REF_THROWS is dropped and counted: the reference would terminate there (std::out_of_range
// out of AutoGetLinePts, src/selectScanPoints.cpp:46,:121, is not caught by main/calibr_offline.cpp).
// Included by abi_frontend.hip only (after clc_scanseg.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "clc_scanseg.hpp"

namespace clc {

constexpr int ASM_SCAN_NO_SEGMENT = -1, ASM_SCAN_REF_THROWS = -2, ASM_SCAN_NO_POSE = -3;  // include/clc.h CLC_SCAN_*
// most points a segment of K7 can have: both ends inside the window of 2 * SEG_DELTA + 1 points, widened by up to 3 at either end
constexpr int ASM_SEG_MAX_POINTS = 2 * SEG_DELTA + 7;
constexpr int ASM_SCAN_BLOCK = 1024;  // the compaction's workgroup: 16 waves, one scan per thread and chunk

// counters of one assembly (long long each), in device memory; read back once
enum AsmCounter {
  ASM_N_KEYFRAMES = 0, ASM_KF_SORTED, ASM_N_SEGMENTS, ASM_N_REF_THROWS, ASM_N_UNMATCHED, ASM_N_OBS, ASM_N_POINTS, ASM_N_LINE_POINTS,
  ASM_OVERFLOW, ASM_COUNTERS
};

// ---- key frames, :62-78 -------------------------------------------------------------------------------------------------------
// true when pose (qn, tn) is far enough from the key frame (qo, to): dist > dist_min || fabs(theta) > theta_min (:70-72).
// dist: Eigen's norm() of the difference, each square and sum rounded (no FMA).  theta = 2 acos(w), w the scalar part of
// qo.inverse() * qn = (qo . qn) / |qo|^2.  |w| > 1: acos is NaN and the angle test false; w < 0: theta > pi, kept; NaN dist: false.
__device__ __forceinline__ bool keyframe_moved(const double* __restrict__ qo, const double* __restrict__ to, const double* __restrict__ qn,
                                               const double* __restrict__ tn, const double dist_min, const double theta_min) {
  const double dx = to[0] - tn[0], dy = to[1] - tn[1], dz = to[2] - tn[2];
  const double dist = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
  const double dot = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(qo[0], qn[0]), __dmul_rn(qo[1], qn[1])), __dmul_rn(qo[2], qn[2])), __dmul_rn(qo[3], qn[3]));
  const double n2 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(qo[0], qo[0]), __dmul_rn(qo[1], qo[1])), __dmul_rn(qo[2], qo[2])), __dmul_rn(qo[3], qo[3]));
  const double theta = 2.0 * acos(dot / n2);
  return (dist > dist_min) || (fabs(theta) > theta_min);
}

// ONE wavefront.  The filter is greedy and sequential in the reference; here the 64 lanes test the next 64 candidates against the
// current key frame, a ballot finds the first that moved, it becomes the key frame and the walk continues behind it: about
// n / 64 + kept steps.  keep[n] (1 / 0), kf[0 .. n_kf) the kept poses' indices in order, cnt[ASM_N_KEYFRAMES], cnt[ASM_KF_SORTED]
// (1: the kept stamps never decrease — NaN counts as a decrease; stamp == nullptr: not looked at, 0).
__global__ __launch_bounds__(64) void keyframe_kernel(const double* __restrict__ q_wc, const double* __restrict__ t_wc,
                                                      const double* __restrict__ stamp, const long long n, const double dist_min,
                                                      const double theta_min, unsigned char* __restrict__ keep, int* __restrict__ kf,
                                                      long long* __restrict__ cnt) {
  const int lane = threadIdx.x;
  long long n_kf = 0, base = 1;
  int sorted = stamp != nullptr ? 1 : 0;
  double qo[4] = {1.0, 0.0, 0.0, 0.0}, to[3] = {0.0, 0.0, 0.0}, so = 0.0;
  if (n > 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) qo[c] = q_wc[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) to[c] = t_wc[c];
    if (stamp != nullptr) so = stamp[0];
    if (lane == 0) { keep[0] = 1; kf[0] = 0; }
    n_kf = 1;
  }
  while (base < n) {
    const long long j = base + lane;
    bool hit = false;
    if (j < n) hit = keyframe_moved(qo, to, q_wc + 4 * j, t_wc + 3 * j, dist_min, theta_min);
    const unsigned long long mask = __ballot(hit);
    if (mask == 0ull) {
      if (j < n) keep[j] = 0;
      base += 64;
      continue;
    }
    const int f = __ffsll((long long)mask) - 1;  // the first candidate that moved (wave-uniform)
    const long long jh = base + f;
    if (lane < f) keep[j] = 0;
    if (lane == f) { keep[j] = 1; kf[n_kf] = (int)jh; }
    ++n_kf;
#pragma unroll
    for (int c = 0; c < 4; ++c) qo[c] = q_wc[4 * jh + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) to[c] = t_wc[3 * jh + c];
    if (stamp != nullptr) {
      const double sn = stamp[jh];
      if (!(sn >= so)) sorted = 0;
      so = sn;
    }
    base = jh + 1;
  }
  if (lane == 0) {
    cnt[ASM_N_KEYFRAMES] = n_kf;
    cnt[ASM_KF_SORTED] = sorted;
  }
}

// ---- scan -> pose, :102-116 ---------------------------------------------------------------------------------------------------
// the reference's update, one candidate: if (t < min_dt) { min_dt = t; closest = i; }  (NaN never wins)
__device__ __forceinline__ void assoc_try(const double* __restrict__ stamp, const int* __restrict__ kf, const long long i, const double ts,
                                          double& min_dt, long long& best) {
  const double t = fabs(stamp[kf[i]] - ts);
  if (t < min_dt) { min_dt = t; best = i; }
}

// One thread per scan.  A scan with a segment takes the key frame with the smallest |pose stamp - scan stamp|, the first of equal
// minima in key-frame order (strict <, from 10000), accepted when that minimum < max_dt.  Non-decreasing key-frame stamps: binary
// search; only the last stamp below the scan's (its FIRST occurrence) and the first stamp at or above it can be the reference's
// answer, and they are tried in index order.  Otherwise the reference's linear walk.
// scan_pose[s]: the ORIGINAL index of the pose, or ASM_SCAN_*.
__global__ void associate_kernel(const int* __restrict__ status, const double* __restrict__ scan_stamp, const long long n_scans,
                                 const double* __restrict__ stamp, const int* __restrict__ kf, const long long* __restrict__ cnt,
                                 const double max_dt, int* __restrict__ scan_pose) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_scans) return;
  const int st = status[s];
  if (st != SEG_FOUND) {
    scan_pose[s] = st == SEG_REF_THROWS ? ASM_SCAN_REF_THROWS : ASM_SCAN_NO_SEGMENT;
    return;
  }
  const long long n_kf = cnt[ASM_N_KEYFRAMES];
  const double ts = scan_stamp[s];
  double min_dt = 10000.0;
  long long best = -1;
  if (cnt[ASM_KF_SORTED] != 0) {
    long long lo = 0, hi = n_kf;  // first i with stamp[kf[i]] >= ts
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (stamp[kf[mid]] < ts) lo = mid + 1; else hi = mid;
    }
    const long long right = lo;
    if (right > 0) {
      const double sl = stamp[kf[right - 1]];
      long long a = 0, b = right - 1;  // first i with stamp[kf[i]] >= sl: the first of the equal stamps
      while (a < b) {
        const long long mid = (a + b) >> 1;
        if (stamp[kf[mid]] < sl) a = mid + 1; else b = mid;
      }
      assoc_try(stamp, kf, a, ts, min_dt, best);
    }
    if (right < n_kf) assoc_try(stamp, kf, right, ts, min_dt, best);
  } else {
    for (long long i = 0; i < n_kf; ++i) assoc_try(stamp, kf, i, ts, min_dt, best);
  }
  scan_pose[s] = (best >= 0 && min_dt < max_dt) ? kf[best] : ASM_SCAN_NO_POSE;
}

// ---- compaction ---------------------------------------------------------------------------------------------------------------
// inclusive sum over the workgroup's threads of three counters at once; *total = the workgroup's sum.  sh: [3][ASM_SCAN_BLOCK / 64].
__device__ __forceinline__ void block_scan3(long long v[3], long long total[3], long long (*sh)[ASM_SCAN_BLOCK / 64]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long u = __shfl_up(v[c], d, 64);
      if (lane >= d) v[c] += u;
    }
    if (lane == 63) sh[c][w] = v[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    long long before = 0, all = 0;
    for (int i = 0; i < ASM_SCAN_BLOCK / 64; ++i) {
      const long long t = sh[c][i];
      if (i < w) before += t;
      all += t;
    }
    v[c] += before;
    total[c] = all;
  }
  __syncthreads();
}

// ONE workgroup: exclusive prefix sums over the scans of {kept, kept segment length, points on the line (2 with >= 2 points)}, a
// chunk of ASM_SCAN_BLOCK scans at a time with the running totals carried from chunk to chunk.  A scan is kept when scan_pose >= 0.
// Out: obs_scan[k] = the scan of observation k; fit_off[0 .. n_scans]: pts_off of the observations, then the total for every
// k >= P (the line fit runs over n_scans rows, the rows behind P empty); soff: the handle's packed offsets, pts_off[P + 1] then
// ptl_off[P + 1]; the counters.  cap_points: what the gather's destination holds (ASM_OVERFLOW is set beyond it, nothing is gathered).
__global__ __launch_bounds__(ASM_SCAN_BLOCK) void compact_kernel(const int* __restrict__ scan_pose, const long long* __restrict__ seg,
                                                                 const long long n_scans, const long long cap_points,
                                                                 long long* __restrict__ obs_scan, long long* __restrict__ fit_off,
                                                                 long long* __restrict__ soff, long long* __restrict__ cnt) {
  __shared__ long long sh[3][ASM_SCAN_BLOCK / 64];
  __shared__ long long sh_c[3][ASM_SCAN_BLOCK / 64];
  const int tid = threadIdx.x;
  long long carry[3] = {0, 0, 0};              // observations, points, line points before this chunk
  long long c_seg = 0, c_thr = 0, c_unm = 0;   // this thread's scans
  // pass 1: the observation index of every kept scan -> obs_scan, fit_off; the line points' offsets wait for P (pass 2)
  for (long long base = 0; base < n_scans; base += ASM_SCAN_BLOCK) {
    const long long s = base + tid;
    long long v[3] = {0, 0, 0}, len = 0;
    bool kept = false;
    if (s < n_scans) {
      const int sp = scan_pose[s];
      kept = sp >= 0;
      c_seg += (sp >= 0 || sp == ASM_SCAN_NO_POSE) ? 1 : 0;
      c_thr += sp == ASM_SCAN_REF_THROWS ? 1 : 0;
      c_unm += sp == ASM_SCAN_NO_POSE ? 1 : 0;
      if (kept) {
        len = seg[2 * s + 1] - seg[2 * s] + 1;
        v[0] = 1; v[1] = len; v[2] = len >= 2 ? 2 : 0;
      }
    }
    long long total[3];
    block_scan3(v, total, sh);
    if (kept) {
      const long long k = carry[0] + v[0] - 1;
      obs_scan[k] = s;
      fit_off[k] = carry[1] + v[1] - len;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) carry[c] += total[c];
  }
  const long long P = carry[0], M = carry[1], ML = carry[2];
  for (long long k = P + tid; k <= n_scans; k += ASM_SCAN_BLOCK) fit_off[k] = M;
  // the three counts: a sum over the workgroup (order of an integer sum does not matter)
  {
    long long v[3] = {c_seg, c_thr, c_unm}, total[3];
    block_scan3(v, total, sh_c);
    if (tid == 0) {
      cnt[ASM_N_SEGMENTS] = total[0];
      cnt[ASM_N_REF_THROWS] = total[1];
      cnt[ASM_N_UNMATCHED] = total[2];
      cnt[ASM_N_OBS] = P;
      cnt[ASM_N_POINTS] = M;
      cnt[ASM_N_LINE_POINTS] = ML;
      cnt[ASM_OVERFLOW] = M > cap_points ? 1 : 0;
    }
  }
  __syncthreads();  // (this workgroup's own global writes of pass 1 are visible to it behind the barrier)
  if (M > cap_points) {  // more points than the destination holds: every row of the fit empty, nothing gathered, the call fails
    for (long long k = tid; k <= n_scans; k += ASM_SCAN_BLOCK) fit_off[k] = 0;
    return;
  }
  // pass 2: the packed offsets; ptl_off by a second running sum over the observations
  long long lcarry = 0;
  for (long long base = 0; base < P; base += ASM_SCAN_BLOCK) {
    const long long k = base + tid;
    long long v[3] = {0, 0, 0}, mine = 0;
    if (k < P) {
      const long long s = obs_scan[k];
      const long long len = seg[2 * s + 1] - seg[2 * s] + 1;
      mine = len >= 2 ? 2 : 0;
      v[0] = mine;
    }
    long long total[3];
    block_scan3(v, total, sh);
    if (k < P) {
      soff[k] = fit_off[k];
      soff[P + 1 + k] = lcarry + v[0] - mine;
    }
    lcarry += total[0];
  }
  if (tid == 0) {
    soff[P] = M;
    soff[2 * P + 1] = ML;
  }
}

// ---- gather -------------------------------------------------------------------------------------------------------------------
// One workgroup per observation k (workgroups behind P leave): the segment's points, (x, y, z) as TranScanToPoints wrote them, into
// spts at pts_off[k] — consecutive lanes on consecutive doubles — and their (x, y) into the line fit's xy; the start line; the tag
// pose, :145-146:  Qca = qwc.inverse() (conjugate / squared norm),  tca = -R(Qca) twc  (toRotationMatrix).
__global__ __launch_bounds__(256) void gather_kernel(const double* __restrict__ points, const long long* __restrict__ off,
                                                     const long long* __restrict__ seg, const int* __restrict__ scan_pose,
                                                     const long long* __restrict__ obs_scan, const long long* __restrict__ fit_off,
                                                     const long long* __restrict__ cnt, const double* __restrict__ q_wc,
                                                     const double* __restrict__ t_wc, const double line0_a, const double line0_b,
                                                     double* __restrict__ spts, double* __restrict__ xy, double* __restrict__ lines,
                                                     double* __restrict__ sq, double* __restrict__ st) {
  const long long k = blockIdx.x;
  if (threadIdx.x == 0) {  // every row of the fit starts from the start line, the empty rows behind the observations too
    lines[2 * k] = line0_a;
    lines[2 * k + 1] = line0_b;
  }
  if (k >= cnt[ASM_N_OBS] || cnt[ASM_OVERFLOW] != 0) return;
  const long long s = obs_scan[k];
  const long long first = seg[2 * s], len = seg[2 * s + 1] - first + 1;
  const long long dst0 = fit_off[k];
  const double* __restrict__ src = points + 3 * (off[s] + first);
  double* __restrict__ d3 = spts + 3 * dst0;
  for (long long i = threadIdx.x; i < 3 * len; i += blockDim.x) d3[i] = src[i];
  double* __restrict__ d2 = xy + 2 * dst0;
  for (long long i = threadIdx.x; i < 2 * len; i += blockDim.x) d2[i] = src[3 * (i >> 1) + (i & 1)];
  if (threadIdx.x == 0) {
    const long long p = scan_pose[s];
    const double w0 = q_wc[4 * p], x0 = q_wc[4 * p + 1], y0 = q_wc[4 * p + 2], z0 = q_wc[4 * p + 3];
    const double n2 = w0 * w0 + x0 * x0 + y0 * y0 + z0 * z0;
    const double w = w0 / n2, x = -x0 / n2, y = -y0 / n2, z = -z0 / n2;
    sq[4 * k] = w; sq[4 * k + 1] = x; sq[4 * k + 2] = y; sq[4 * k + 3] = z;
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double a = t_wc[3 * p], b = t_wc[3 * p + 1], c = t_wc[3 * p + 2];
    st[3 * k] = -((1.0 - (tyy + tzz)) * a + (txy - twz) * b + (txz + twy) * c);
    st[3 * k + 1] = -((txy + twz) * a + (1.0 - (txx + tzz)) * b + (tyz - twx) * c);
    st[3 * k + 2] = -((txz - twy) * a + (tyz + twx) * b + (1.0 - (txx + tyy)) * c);
  }
}

// ---- the two points on the fitted line, :126-142 ------------------------------------------------------------------------------
// One thread per observation, the arithmetic of calib.points_on_fitted_lines: the first and the LAST point of the segment (the
// reference reads points.end(), one past the end; the last point is this project's convention), the abscissa branch when
// |dx| > |dy|, the ordinate branch otherwise; z = 0.  An observation with fewer than 2 points gets none.
__global__ void endpoints_kernel(const double* __restrict__ spts, const long long* __restrict__ soff, const long long* __restrict__ cnt,
                                 const double* __restrict__ lines, double* __restrict__ sptl) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long P = cnt[ASM_N_OBS];
  if (k >= P || cnt[ASM_OVERFLOW] != 0) return;
  const long long lo = soff[k], hi = soff[k + 1];
  if (hi - lo < 2) return;
  double xs = spts[3 * lo], ys = spts[3 * lo + 1], xe = spts[3 * (hi - 1)], ye = spts[3 * (hi - 1) + 1];
  const double m0 = lines[2 * k], m1 = lines[2 * k + 1];
  if (fabs(xe - xs) > fabs(ye - ys)) {
    ys = -(xs * m0 + 1.0) / m1;
    ye = -(xe * m0 + 1.0) / m1;
  } else {
    xs = -(ys * m1 + 1.0) / m0;
    xe = -(ye * m1 + 1.0) / m0;
  }
  double* __restrict__ o = sptl + 3 * soff[P + 1 + k];
  o[0] = xs; o[1] = ys; o[2] = 0.0;
  o[3] = xe; o[4] = ye; o[5] = 0.0;
}

}  // namespace clc
