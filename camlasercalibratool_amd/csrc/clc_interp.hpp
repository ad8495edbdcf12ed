// clc_interp.hpp — K15: tag poses interpolated at the scans' stamps.  Key-frame mode (K13, clc_assemble.hpp) ties a scan to the NEAREST
// key frame within max_dt, station mode (K14, clc_stations.hpp) to the averaged pose of a station the board was held still at; here
// every scan with a board segment takes the pose between the two stamped tag poses that bracket its stamp (plus a clock offset):
// translation linear, rotation slerp.  Everything behind the association (compaction, gather, line fit, end points) is K13's, unchanged.
// FP64, fixed order, no atomics: a second run gives the same bits.
// The bracket rule and the interpolation are THIS PROJECT'S design: the reference interpolates nowhere (main/calibr_offline.cpp:102-116
// takes the nearest key frame).
// Included by abi_frontend.hip only (after clc_stations.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "clc_assemble.hpp"

namespace clc {

constexpr double INTERP_NLERP_ABOVE = 1.0 - 1e-10;  // slerp while dot <= this, normalised lerp above

// ---- the pose list -----------------------------------------------------------------------------------------------------------------
// pair i = poses (i, i + 1) is a bracket candidate when both stamps are finite and 0 < stamp[i + 1] - stamp[i] <= max_gap
__device__ __forceinline__ bool interp_pair_ok(const double* __restrict__ stamp, const long long i, const double max_gap) {
  const double a = stamp[i], b = stamp[i + 1];
  const double gap = b - a;
  return isfinite(a) && isfinite(b) && gap > 0.0 && gap <= max_gap;
}

// ONE wavefront over the n - 1 pairs of the list: cnt[ASM_N_KEYFRAMES] = the pairs that can bracket a stamp (interp_pair_ok),
// cnt[ASM_KF_SORTED] = 1 when the stamps never decrease (a NaN counts as a decrease, as in keyframe_kernel).
__global__ __launch_bounds__(64) void interp_stamps_kernel(const double* __restrict__ stamp, const long long n, const double max_gap,
                                                           long long* __restrict__ cnt) {
  const int lane = threadIdx.x;
  long long ok = 0;
  int sorted = 1;
  for (long long i = lane; i + 1 < n; i += 64) {
    if (!(stamp[i + 1] >= stamp[i])) sorted = 0;
    ok += interp_pair_ok(stamp, i, max_gap) ? 1 : 0;
  }
  if (n == 1 && !(stamp[0] == stamp[0])) sorted = 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) ok += __shfl_xor(ok, d, 64);
  const int all_sorted = __all(sorted);
  if (lane == 0) {
    cnt[ASM_N_KEYFRAMES] = ok;
    cnt[ASM_KF_SORTED] = all_sorted ? 1 : 0;
  }
}

// ---- the bracket -------------------------------------------------------------------------------------------------------------------
// pair i brackets x: a candidate pair with stamp[i] <= x <= stamp[i + 1] (both ends inclusive)
__device__ __forceinline__ bool interp_brackets(const double* __restrict__ stamp, const long long i, const double x, const double max_gap) {
  return interp_pair_ok(stamp, i, max_gap) && stamp[i] <= x && x <= stamp[i + 1];
}

// The FIRST pair in file order that brackets x, or -1; a NaN x never matches.  Stamps that never decrease (sorted): with
// lo = the first index whose stamp is >= x and ub = the first whose stamp is > x, the only pairs with stamp[i] <= x <= stamp[i + 1]
// are lo - 1 (stamp[lo - 1] < x <= stamp[lo]), the pairs lo .. ub - 2 inside a run of stamps equal to x (gap 0: never a candidate)
// and ub - 1 (stamp[ub - 1] == x < stamp[ub]) — so lo - 1, then ub - 1 are tried, in that order, with the linear rule's own test.
__device__ __forceinline__ long long interp_find_bracket(const double* __restrict__ stamp, const long long n, const double x,
                                                         const double max_gap, const bool sorted) {
  if (!(x == x) || n < 2) return -1;
  if (!sorted) {
    for (long long i = 0; i + 1 < n; ++i)
      if (interp_brackets(stamp, i, x, max_gap)) return i;
    return -1;
  }
  long long a = 0, b = n;  // first index with stamp >= x
  while (a < b) {
    const long long mid = (a + b) >> 1;
    if (stamp[mid] >= x) b = mid; else a = mid + 1;
  }
  const long long lo = a;
  b = n;  // first index >= lo with stamp > x
  while (a < b) {
    const long long mid = (a + b) >> 1;
    if (stamp[mid] > x) b = mid; else a = mid + 1;
  }
  const long long ub = a;
  if (lo >= 1 && lo < n && interp_brackets(stamp, lo - 1, x, max_gap)) return lo - 1;
  if (ub > lo && ub < n && interp_brackets(stamp, ub - 1, x, max_gap)) return ub - 1;
  return -1;
}

// ---- the pose between two poses ----------------------------------------------------------------------------------------------------
// u in [0, 1] between poses (q0, t0) and (q1, t1), quaternions as stored, (w, x, y, z): t = t0 + u (t1 - t0); each quaternion
// normalised, q1 negated when the dot product is < 0, slerp (sin((1 - u) th) q0 + sin(u th) q1) / sin(th) with th = acos(dot) while
// dot <= INTERP_NLERP_ABOVE, (1 - u) q0 + u q1 above; the result normalised.  Every product and sum rounded on its own (no FMA), so
// the restatement's arithmetic is this arithmetic.  Returns false when a component of the result is not finite.
__device__ __forceinline__ bool interp_pose(const double* __restrict__ q0s, const double* __restrict__ t0, const double* __restrict__ q1s,
                                            const double* __restrict__ t1, const double u, double q[4], double t[3]) {
  double q0[4], q1[4];
  {
    const double n0 = sqrt(__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(q0s[0], q0s[0]), __dmul_rn(q0s[1], q0s[1])), __dmul_rn(q0s[2], q0s[2])), __dmul_rn(q0s[3], q0s[3])));
    const double n1 = sqrt(__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(q1s[0], q1s[0]), __dmul_rn(q1s[1], q1s[1])), __dmul_rn(q1s[2], q1s[2])), __dmul_rn(q1s[3], q1s[3])));
#pragma unroll
    for (int c = 0; c < 4; ++c) { q0[c] = q0s[c] / n0; q1[c] = q1s[c] / n1; }
  }
  double dot = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(q0[0], q1[0]), __dmul_rn(q0[1], q1[1])), __dmul_rn(q0[2], q1[2])), __dmul_rn(q0[3], q1[3]));
  if (dot < 0.0) {
    dot = -dot;
#pragma unroll
    for (int c = 0; c < 4; ++c) q1[c] = -q1[c];
  }
  double w0 = 1.0 - u, w1 = u;
  if (dot <= INTERP_NLERP_ABOVE) {
    const double th = acos(dot), s = sin(th);
    w0 = sin(__dmul_rn(1.0 - u, th)) / s;
    w1 = sin(__dmul_rn(u, th)) / s;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) q[c] = __dadd_rn(__dmul_rn(w0, q0[c]), __dmul_rn(w1, q1[c]));
  const double nq = sqrt(__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(q[0], q[0]), __dmul_rn(q[1], q[1])), __dmul_rn(q[2], q[2])), __dmul_rn(q[3], q[3])));
  bool finite = true;
#pragma unroll
  for (int c = 0; c < 4; ++c) { q[c] = q[c] / nq; finite = finite && isfinite(q[c]); }
#pragma unroll
  for (int c = 0; c < 3; ++c) { t[c] = __dadd_rn(t0[c], __dmul_rn(u, t1[c] - t0[c])); finite = finite && isfinite(t[c]); }
  return finite;
}

// ---- query -> interpolated pose ----------------------------------------------------------------------------------------------------
// One thread per query (a scan's stamp).  x = query_stamp + time_offset; the bracket by interp_find_bracket (cnt[ASM_KF_SORTED] of
// interp_stamps_kernel chooses the search); u = (x - stamp[i]) / (stamp[i + 1] - stamp[i]); the pose by interp_pose.  No bracket, or
// a result that is not finite: ASM_SCAN_NO_POSE, u = 0, q = (1, 0, 0, 0), t = 0.
// seg_status (nullable): K7's status per query — a query without a segment gets ASM_SCAN_NO_SEGMENT / _REF_THROWS and is not looked up.
// Out, each nullable: bracket[m] (the pair's first pose, or the code), u_out[m], q_out[4 m], t_out[3 m], and self[m] — the query's OWN
// index where bracket holds a pose, the code elsewhere: the scan_pose that makes gather_kernel index the per-scan arrays q_out / t_out.
__global__ void interp_kernel(const int* __restrict__ seg_status, const double* __restrict__ query_stamp, const long long m,
                              const double* __restrict__ stamp, const double* __restrict__ q_wc, const double* __restrict__ t_wc,
                              const long long n, const long long* __restrict__ cnt, const double time_offset, const double max_gap,
                              int* __restrict__ bracket, double* __restrict__ u_out, double* __restrict__ q_out, double* __restrict__ t_out,
                              int* __restrict__ self) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= m) return;
  int code = ASM_SCAN_NO_POSE;
  double u = 0.0, q[4] = {1.0, 0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
  const int st = seg_status != nullptr ? seg_status[s] : SEG_FOUND;
  if (st != SEG_FOUND) {
    code = st == SEG_REF_THROWS ? ASM_SCAN_REF_THROWS : ASM_SCAN_NO_SEGMENT;
  } else {
    const double x = query_stamp[s] + time_offset;
    const long long i = interp_find_bracket(stamp, n, x, max_gap, cnt[ASM_KF_SORTED] != 0);
    if (i >= 0) {
      const double a = stamp[i];
      const double ui = (x - a) / (stamp[i + 1] - a);
      double qi[4], ti[3];
      if (interp_pose(q_wc + 4 * i, t_wc + 3 * i, q_wc + 4 * (i + 1), t_wc + 3 * (i + 1), ui, qi, ti)) {
        code = (int)i;
        u = ui;
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = qi[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = ti[c];
      }
    }
  }
  if (bracket != nullptr) bracket[s] = code;
  if (u_out != nullptr) u_out[s] = u;
  if (q_out != nullptr) {
#pragma unroll
    for (int c = 0; c < 4; ++c) q_out[4 * s + c] = q[c];
  }
  if (t_out != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) t_out[3 * s + c] = t[c];
  }
  if (self != nullptr) self[s] = code >= 0 ? (int)s : code;
}

// ---- the clock sweep: one problem per candidate offset on the same scans ----------------------------------------------------------------
enum SweepCounter { SW_N_USED = 0, SW_N_RECORDS, SW_COUNTERS };  // long long each, in device memory; read back once

// points taken from a segment of len points: all of them, or per_scan > 0 of them spread evenly when it has more
__device__ __forceinline__ long long sweep_take(const long long len, const long long per_scan) {
  return (per_scan > 0 && len > per_scan) ? per_scan : len;
}

// One thread per scan: take[s] = the points the scan contributes to EVERY problem — sweep_take of its segment when it has one
// (SEG_FOUND) and a bracket with a finite pose at every candidate offset, 0 otherwise (so all problems hold the same records and
// their costs are comparable).
__global__ void sweep_member_kernel(const int* __restrict__ seg_status, const long long* __restrict__ seg, const double* __restrict__ scan_stamp,
                                    const long long n_scans, const double* __restrict__ stamp, const double* __restrict__ q_wc,
                                    const double* __restrict__ t_wc, const long long n, const long long* __restrict__ cnt,
                                    const double* __restrict__ offsets, const int n_offsets, const double max_gap, const long long per_scan,
                                    long long* __restrict__ take) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_scans) return;
  bool used = seg_status[s] == SEG_FOUND;
  const bool sorted = cnt[ASM_KF_SORTED] != 0;
  const double ts = scan_stamp[s];
  for (int j = 0; used && j < n_offsets; ++j) {
    const double x = ts + offsets[j];
    const long long i = interp_find_bracket(stamp, n, x, max_gap, sorted);
    if (i < 0) { used = false; break; }
    const double a = stamp[i];
    double q[4], t[3];
    used = interp_pose(q_wc + 4 * i, t_wc + 3 * i, q_wc + 4 * (i + 1), t_wc + 3 * (i + 1), (x - a) / (stamp[i + 1] - a), q, t);
  }
  take[s] = used ? sweep_take(seg[2 * s + 1] - seg[2 * s] + 1, per_scan) : 0;
}

constexpr int SWEEP_SCAN_BLOCK = 256;  // the workgroup of sweep_offsets_kernel: 4 waves, one scan per thread and chunk

// inclusive sum of v over the wave's lanes
__device__ __forceinline__ long long sweep_wave_scan(long long v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// ONE workgroup: exclusive prefix sums over the scans of {used, points taken}, a chunk of SWEEP_SCAN_BLOCK scans at a time with the running
// totals carried from chunk to chunk.  Out: used_scan[k] = the scan of the k-th used scan, rec_off[k] = its first record within a problem
// (rec_off[n_used] = the records of a problem), sw[SW_N_USED], sw[SW_N_RECORDS].  used_scan holds n_scans entries, rec_off n_scans + 1.
__global__ __launch_bounds__(SWEEP_SCAN_BLOCK) void sweep_offsets_kernel(const long long* __restrict__ take, const long long n_scans,
                                                                         long long* __restrict__ used_scan, long long* __restrict__ rec_off,
                                                                         long long* __restrict__ sw) {
  constexpr int NW = SWEEP_SCAN_BLOCK / 64;
  __shared__ long long sh_k[NW], sh_r[NW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  long long carry_k = 0, carry_r = 0;  // used scans, records before this chunk
  for (long long base = 0; base < n_scans; base += SWEEP_SCAN_BLOCK) {
    const long long s = base + tid;
    const long long mine = s < n_scans ? take[s] : 0;
    long long vk = sweep_wave_scan(mine > 0 ? 1 : 0), vr = sweep_wave_scan(mine);
    if (lane == 63) { sh_k[w] = vk; sh_r[w] = vr; }
    __syncthreads();
    long long all_k = 0, all_r = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const long long tk = sh_k[i], tr = sh_r[i];
      if (i < w) { vk += tk; vr += tr; }
      all_k += tk;
      all_r += tr;
    }
    __syncthreads();
    if (mine > 0) {
      const long long k = carry_k + vk - 1;
      used_scan[k] = s;
      rec_off[k] = carry_r + vr - mine;
    }
    carry_k += all_k;
    carry_r += all_r;
  }
  if (tid == 0) {
    rec_off[carry_k] = carry_r;
    sw[SW_N_USED] = carry_k;
    sw[SW_N_RECORDS] = carry_r;
  }
}

// One workgroup per (used scan k, candidate offset j) = (blockIdx.x, blockIdx.y): the records of scan k in problem j, at
// rec[(j * n_records + rec_off[k]) * 8 ...], the reference's assembly loop (src/LaseCamCalCeres.cpp:222-254) with
// use_linefitting_data = false and no edge terms.  The bracket, the interpolated pose at scan_stamp + offsets[j], Qca = q.inverse(),
// tca = -R(Qca) t (:145-146, as gather_kernel) and the plane n = R(Qca) e3, d = -n . tca depend on (k, j) alone: every lane computes
// them from the same addresses — wave-uniform values, no exchange, no barrier.  The points: all of the segment, or per_scan of its L
// points at index floor((2 i + 1) L / (2 per_scan)); scale = 1 / sqrt(points taken).  Consecutive lanes write consecutive doubles of
// the 64-byte records (n0 n1 n2 d px py pz scale).  The scans were chosen by sweep_member_kernel: the bracket exists.
__global__ __launch_bounds__(128) void sweep_records_kernel(const double* __restrict__ points, const long long* __restrict__ off,
                                                            const long long* __restrict__ seg, const double* __restrict__ scan_stamp,
                                                            const long long* __restrict__ used_scan, const long long* __restrict__ rec_off,
                                                            const long long* __restrict__ sw, const double* __restrict__ stamp,
                                                            const double* __restrict__ q_wc, const double* __restrict__ t_wc, const long long n,
                                                            const long long* __restrict__ cnt, const double* __restrict__ offsets,
                                                            const double max_gap, const long long per_scan, double* __restrict__ rec) {
  const long long k = blockIdx.x;
  if (k >= sw[SW_N_USED]) return;
  const int j = blockIdx.y;
  const long long s = used_scan[k];
  const double x = scan_stamp[s] + offsets[j];
  const long long i = interp_find_bracket(stamp, n, x, max_gap, cnt[ASM_KF_SORTED] != 0);
  if (i < 0) return;  // (never: the scan is a member)
  const double a = stamp[i];
  double qi[4], ti[3];
  interp_pose(q_wc + 4 * i, t_wc + 3 * i, q_wc + 4 * (i + 1), t_wc + 3 * (i + 1), (x - a) / (stamp[i + 1] - a), qi, ti);
  const double n2 = qi[0] * qi[0] + qi[1] * qi[1] + qi[2] * qi[2] + qi[3] * qi[3];
  const double w = qi[0] / n2, qx = -qi[1] / n2, qy = -qi[2] / n2, qz = -qi[3] / n2;
  const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
  const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  const double c0 = -((1.0 - (tyy + tzz)) * ti[0] + (txy - twz) * ti[1] + (txz + twy) * ti[2]);  // tca
  const double c1 = -((txy + twz) * ti[0] + (1.0 - (txx + tzz)) * ti[1] + (tyz - twx) * ti[2]);
  const double c2 = -((txz - twy) * ti[0] + (tyz + twx) * ti[1] + (1.0 - (txx + tyy)) * ti[2]);
  const double n0 = txz + twy, n1 = tyz - twx, nz = 1.0 - (txx + tyy);  // the third column of R(Qca)
  const double d = -((n0 * c0 + n1 * c1) + nz * c2);
  const long long first = seg[2 * s], len = seg[2 * s + 1] - first + 1;
  const long long m = sweep_take(len, per_scan);
  const double scale = 1.0 / sqrt((double)m);
  const double* __restrict__ src = points + 3 * (off[s] + first);
  double* __restrict__ dst = rec + 8 * ((long long)j * sw[SW_N_RECORDS] + rec_off[k]);
  for (long long e = threadIdx.x; e < 8 * m; e += blockDim.x) {
    const long long r = e >> 3;
    const int c = (int)(e & 7);
    const long long p = m < len ? ((2 * r + 1) * len) / (2 * m) : r;
    double v;
    if (c >= 4 && c < 7) v = src[3 * p + (c - 4)];
    else v = c == 0 ? n0 : c == 1 ? n1 : c == 2 ? nz : c == 3 ? d : scale;
    dst[e] = v;
  }
}

}  // namespace clc
