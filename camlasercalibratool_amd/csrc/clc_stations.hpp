// clc_stations.hpp — K14: static stations.  GetStaticPose (src/utilities.cpp:86-155) on the device — the runs of stamped tag poses
// that stay within center_dist_max of their running centre, each run that is long enough averaged into one pose (mean translation,
// quaternion mean = dominant eigenvector of sum q q^T / n, getAvergeQwc :156-166) stamped with the run's start_time / end_time
// (include/utilities.h:19-20) — and the association of every scan with the station whose interval holds its stamp.
// FP64, fixed order, no atomics: a second run gives the same bits.
// The interval matching is THIS PROJECT'S design: the reference has no node that consumes GetStaticPose's output; the averaged
// pose stands in for the single nearest key frame of main/calibr_offline.cpp:102-116 (K13, clc_assemble.hpp), and everything behind
// the association (compaction, gather, line fit, end points) is K13's, unchanged.
// Included by abi_frontend.hip only (after clc_assemble.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "clc_assemble.hpp"

namespace clc {

constexpr int STATION_OK = 1, STATION_NONFINITE = -1;  // include/clc.h CLC_STATION_*
constexpr int STATION_WAVES_PER_BLOCK = 4;             // the average's workgroup: one wave per station

// counters of one walk (long long each), in device memory
enum StationCounter { ST_N_RUNS = 0, ST_N_STATIONS, ST_SORTED, ST_COUNTERS };

// ---- the walk, :96-124 ----------------------------------------------------------------------------------------------------------
// The reference's state is xy_sum and staticPose.size().  A run starts at pose a: xy_sum = t_a, size = 1 (the pose is pushed, :103).
// Candidate j = a, a + 1, ... is a member iff |t_j - xy_sum / size| < center_dist_max (norm(): every square and sum rounded, no FMA;
// the centre a per-component division), and a member does xy_sum += t_j, ++size — so the first pose of a run is tested against
// itself and counted twice.  The first candidate that is no member closes the run and is discarded; the next run starts behind it.
// A NaN never is a member.  The run open at the end of the list is dropped (:114-123 push at a break only) unless close_last_run.
//
// ONE wavefront.  The 64 lanes take the next 64 candidates of the current run.  Lane l needs the centre that would hold had every
// candidate before it been a member: the carried xy_sum + t_base + ... + t_{base + l - 1}, ADDED IN THAT ORDER, over size + l.  The
// sum is built in the sequential order by 64 wave-uniform steps (broadcast lane i's t, add under i < lane), so every decision has
// the reference's bits; a ballot finds the first non-member, the lanes before it are members whatever came behind.  About
// n / 64 + runs steps.
// Out: station k = first[k], last[k] (pose indices of the first and the last member), members[k] = staticPose.size() (the first
// pose counted twice: a station's members are pose first[k], then poses first[k] .. first[k] + members[k] - 2); cnt[ST_N_RUNS] every
// closed run, cnt[ST_N_STATIONS] those with members > min_members, cnt[ST_SORTED] 1 when neither the stations' first stamps nor
// their last stamps ever decrease (NaN counts as a decrease; stamp == nullptr: all stamps are 0, sorted).  first / last / members
// hold n entries: a run consumes at least one pose.
__global__ __launch_bounds__(64) void station_walk_kernel(const double* __restrict__ t_wc, const double* __restrict__ stamp, const long long n,
                                                          const double dist_max, const long long min_members, const int close_last_run,
                                                          long long* __restrict__ first, long long* __restrict__ last,
                                                          long long* __restrict__ members, long long* __restrict__ cnt) {
  const int lane = threadIdx.x;
  long long n_runs = 0, n_st = 0;
  int sorted = 1;
  double s_start = 0.0, s_end = 0.0;  // stamps of the last station
  auto close_run = [&](const long long a, const long long l, const long long m) {  // wave-uniform
    ++n_runs;
    if (m > min_members) {
      if (stamp != nullptr) {
        const double ss = stamp[a], se = stamp[l];
        if (n_st > 0 ? !(ss >= s_start && se >= s_end) : !(ss == ss && se == se)) sorted = 0;
        s_start = ss;
        s_end = se;
      }
      if (lane == 0) { first[n_st] = a; last[n_st] = l; members[n_st] = m; }
      ++n_st;
    }
  };
  long long a = 0;  // the current run's first pose
  while (a < n) {
    double xs[3] = {t_wc[3 * a], t_wc[3 * a + 1], t_wc[3 * a + 2]};  // xy_sum
    long long size = 1, base = a;
    bool open = true;
    while (base < n) {
      const long long j = base + lane;
      const bool valid = j < n;
      double tj[3] = {0.0, 0.0, 0.0};
      if (valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) tj[c] = t_wc[3 * j + c];
      }
      double pre[3] = {xs[0], xs[1], xs[2]};  // xy_sum before candidate j, had every candidate of this chunk before it been a member
#pragma unroll
      for (int i = 0; i < 63; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double v = __shfl(tj[c], i, 64);
          if (i < lane) pre[c] = __dadd_rn(pre[c], v);
        }
      }
      const double den = (double)(size + lane);
      const double dx = tj[0] - pre[0] / den, dy = tj[1] - pre[1] / den, dz = tj[2] - pre[2] / den;
      const double dist = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
      const unsigned long long mask = __ballot(valid && !(dist < dist_max));
      if (mask == 0ull) {  // every candidate of the chunk is a member: carry xy_sum and size on
        const long long nv = n - base < 64 ? n - base : 64;
#pragma unroll
        for (int c = 0; c < 3; ++c) xs[c] = __shfl(__dadd_rn(pre[c], tj[c]), (int)(nv - 1), 64);
        size += nv;
        base += 64;
        continue;
      }
      const int f = __ffsll((long long)mask) - 1;  // the first non-member (wave-uniform)
      const long long jb = base + f;
      close_run(a, jb > a ? jb - 1 : a, size + f);
      a = jb + 1;
      open = false;
      break;
    }
    if (open) {  // the list ended inside the run
      if (close_last_run) close_run(a, n - 1, size);
      break;
    }
  }
  if (lane == 0) {
    cnt[ST_N_RUNS] = n_runs;
    cnt[ST_N_STATIONS] = n_st;
    cnt[ST_SORTED] = sorted;
  }
}

// ---- the average, :129-152 ------------------------------------------------------------------------------------------------------
// sum over the wave, every lane gets the same bits (a + b == b + a at every level of the butterfly)
__device__ __forceinline__ double station_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = __dadd_rn(v, __shfl_xor(v, d, 64));
  return v;
}

// Cyclic Jacobi on the symmetric 4 x 4 A (10 unique entries, row-major upper triangle: 00 01 02 03 11 12 13 22 23 33) -> the unit
// eigenvector of its largest eigenvalue (the first of equal ones in index order).  Every index is a compile-time constant (registers).
__device__ __forceinline__ void station_dominant_eigvec(const double u[10], double q[4]) {
  double A[4][4], V[4][4];
  {
    int idx = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = r; c < 4; ++c) { A[r][c] = u[idx]; A[c][r] = u[idx]; ++idx; }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 24; ++sweep) {
    double off = 0.0, diag = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      diag += fabs(A[r][r]);
#pragma unroll
      for (int c = r + 1; c < 4; ++c) off += fabs(A[r][c]);
    }
    if (!(off > 0x1p-70 * diag)) break;  // converged (far below the eigenvector's own rounding error), or not finite
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int r = p + 1; r < 4; ++r) {
        const double apq = A[p][r];
        if (apq != 0.0) {
          const double theta = (A[r][r] - A[p][p]) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // A <- A J
            const double akp = A[k][p], akq = A[k][r];
            A[k][p] = c * akp - s * akq;
            A[k][r] = s * akp + c * akq;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // A <- J^T A
            const double apk = A[p][k], aqk = A[r][k];
            A[p][k] = c * apk - s * aqk;
            A[r][k] = s * apk + c * aqk;
          }
          A[p][r] = 0.0;
          A[r][p] = 0.0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {  // V <- V J
            const double vkp = V[k][p], vkq = V[k][r];
            V[k][p] = c * vkp - s * vkq;
            V[k][r] = s * vkp + c * vkq;
          }
        }
      }
    }
  }
  double best = A[0][0];
#pragma unroll
  for (int c = 0; c < 4; ++c) q[c] = V[c][0];
#pragma unroll
  for (int e = 1; e < 4; ++e)
    if (A[e][e] > best) {
      best = A[e][e];
#pragma unroll
      for (int c = 0; c < 4; ++c) q[c] = V[c][e];
    }
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int c = 0; c < 4; ++c) q[c] /= nrm;
}

// One wave per station (waves behind the walk's count leave; more stations than waves: a grid-stride loop).  The members — pose
// first, then poses first .. first + members - 2 — are strided over the lanes; each lane accumulates sum t (3) and the 10 unique
// entries of sum q q^T with q = (w, x, y, z), the wave all-reduces them in a fixed order and divides by n = members.  The quaternion
// is the unit eigenvector of the largest eigenvalue, its sign fixed (the reference's is arbitrary): w > 0, or the first non-zero
// component positive when w == 0.  start_time / end_time = stamp[first] / stamp[last] (stamp == nullptr: 0).  A result that is not
// finite: status STATION_NONFINITE, q = (1, 0, 0, 0), t = 0 — such a station takes no scan.
__global__ __launch_bounds__(64 * STATION_WAVES_PER_BLOCK) void station_average_kernel(
    const double* __restrict__ q_wc, const double* __restrict__ t_wc, const double* __restrict__ stamp, const long long* __restrict__ first,
    const long long* __restrict__ last, const long long* __restrict__ members, const long long* __restrict__ cnt,
    double* __restrict__ q_avg, double* __restrict__ t_avg, double* __restrict__ start_time, double* __restrict__ end_time,
    int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const long long n_st = cnt[ST_N_STATIONS];
  const long long n_waves = (long long)gridDim.x * STATION_WAVES_PER_BLOCK;
  for (long long k = (long long)blockIdx.x * STATION_WAVES_PER_BLOCK + (threadIdx.x >> 6); k < n_st; k += n_waves) {
    const long long a = first[k], m = members[k];
    double acc[13];
#pragma unroll
    for (int c = 0; c < 13; ++c) acc[c] = 0.0;
    for (long long i = lane; i < m; i += 64) {
      const long long p = i == 0 ? a : a + i - 1;
      const double w = q_wc[4 * p], x = q_wc[4 * p + 1], y = q_wc[4 * p + 2], z = q_wc[4 * p + 3];
      acc[0] += t_wc[3 * p]; acc[1] += t_wc[3 * p + 1]; acc[2] += t_wc[3 * p + 2];
      acc[3] = fma(w, w, acc[3]); acc[4] = fma(w, x, acc[4]); acc[5] = fma(w, y, acc[5]); acc[6] = fma(w, z, acc[6]);
      acc[7] = fma(x, x, acc[7]); acc[8] = fma(x, y, acc[8]); acc[9] = fma(x, z, acc[9]);
      acc[10] = fma(y, y, acc[10]); acc[11] = fma(y, z, acc[11]);
      acc[12] = fma(z, z, acc[12]);
    }
    const double nd = (double)m;
#pragma unroll
    for (int c = 0; c < 13; ++c) acc[c] = station_wave_sum(acc[c]) / nd;
    double q[4];
    station_dominant_eigvec(acc + 3, q);
    bool neg = q[0] < 0.0;
    if (q[0] == 0.0) neg = q[1] != 0.0 ? q[1] < 0.0 : (q[2] != 0.0 ? q[2] < 0.0 : q[3] < 0.0);
    if (neg) {
#pragma unroll
      for (int c = 0; c < 4; ++c) q[c] = -q[c];
    }
    bool finite = isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]) && isfinite(q[3]);
#pragma unroll
    for (int c = 0; c < 13; ++c) finite = finite && isfinite(acc[c]);  // (a NaN in A stops the Jacobi sweeps at once, V = I is finite)
    if (lane == 0) {
      q_avg[4 * k] = finite ? q[0] : 1.0;
#pragma unroll
      for (int c = 1; c < 4; ++c) q_avg[4 * k + c] = finite ? q[c] : 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) t_avg[3 * k + c] = finite ? acc[c] : 0.0;
      start_time[k] = stamp != nullptr ? stamp[a] : 0.0;
      end_time[k] = stamp != nullptr ? stamp[last[k]] : 0.0;
      status[k] = finite ? STATION_OK : STATION_NONFINITE;
    }
  }
}

// ---- scan -> station ------------------------------------------------------------------------------------------------------------
// One thread per scan.  A scan with a board segment takes the FIRST station, in station order, that is finite and has
// start_time <= scan_stamp <= end_time (both ends inclusive; a NaN stamp never matches).  When neither the start nor the end stamps
// ever decrease (cnt[ST_SORTED]) the matching stations are the range [first end >= stamp, first start > stamp), found by two binary
// searches and walked for the first finite one; otherwise the linear walk over every station.
// scan_station[s]: the station's index, or ASM_SCAN_NO_SEGMENT / _REF_THROWS / _NO_POSE.
__global__ void station_associate_kernel(const int* __restrict__ seg_status, const double* __restrict__ scan_stamp, const long long n_scans,
                                         const double* __restrict__ start_time, const double* __restrict__ end_time,
                                         const int* __restrict__ st_status, const long long* __restrict__ cnt, int* __restrict__ scan_station) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_scans) return;
  const int st = seg_status[s];
  if (st != SEG_FOUND) {
    scan_station[s] = st == SEG_REF_THROWS ? ASM_SCAN_REF_THROWS : ASM_SCAN_NO_SEGMENT;
    return;
  }
  const long long n_st = cnt[ST_N_STATIONS];
  const double ts = scan_stamp[s];
  long long lo = 0, hi = n_st;
  if (cnt[ST_SORTED] != 0) {
    long long a = 0, b = n_st;  // first i with end_time[i] >= ts
    while (a < b) {
      const long long mid = (a + b) >> 1;
      if (end_time[mid] >= ts) b = mid; else a = mid + 1;
    }
    lo = a;
    b = n_st;  // first i >= lo with start_time[i] > ts
    while (a < b) {
      const long long mid = (a + b) >> 1;
      if (start_time[mid] > ts) b = mid; else a = mid + 1;
    }
    hi = a;
  }
  int best = ASM_SCAN_NO_POSE;
  for (long long i = lo; i < hi; ++i)
    if (st_status[i] == STATION_OK && start_time[i] <= ts && ts <= end_time[i]) { best = (int)i; break; }
  scan_station[s] = best;
}

}  // namespace clc
