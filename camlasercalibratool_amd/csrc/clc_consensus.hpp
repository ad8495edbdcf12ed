// clc_consensus.hpp — K12: block scores of many candidate poses on ONE resident copy of the observations (clc_score_blocks).
//
// A consensus (RANSAC / least-median) step judges EVERY candidate pose against EVERY recorded pose (block of records) of the full
// problem.  The launch is a sibling of multi-start / subsets (clc_resident.hpp): a workgroup per candidate, all of them on problem 0's
// lane layout — one copy in HBM, served from L2 after the first round of workgroups — and the lane -> block map that
// subset_lane_map_kernel built for clc_solve_subsets.  ONE evaluation pass, no Jacobian, no LM controller, so nothing is kept on chip
// between passes: a lane streams its ppl slots once (16-byte loads, j-major, coalesced) and keeps three sums of its valid points,
//     sum r0^2,   sum log(1 + r0^2 / lf^2)   (without the loss: nothing),   #{|r0| <= tau},     r0 = n.(R p + t) + d = m.p + c0,
// the residual before the scale, exactly as accumulate_observation (clc_device.hpp) forms it.  A lane holds points of ONE scan, so
// scale^2 and the loss scale a = lf scale multiply its sums once:  ssq = s^2 sum r0^2,  cost = 1/2 lf^2 s^2 sum log(.)  (1/2 ssq
// without the loss).  The logarithm is taken per point (log1p_pos: log_ge1, < 1 ulp, corrected for the rounding of 1 + x): one pass
// has no use for the running-product trick of the solve kernels, and a far candidate's product would need their renormalisation.
//
// Reduction over a block, in a FIXED order (two calls return the same bits; no floating-point atomics): res_build_kernel deals the
// records to the lanes in order, so the lanes of a block are consecutive.  The lane sums go to LDS; the FIRST lane of every block
// (the lane before it is in another block) adds its block's lanes one after the other; the block sums are staged in LDS and leave the
// workgroup as whole rows (coalesced: the tables live in page-locked host memory behind PCIe).  A block without records has no lane
// and scores 0 / 0 / 0.  A candidate with a non-finite pose gets NaN / NaN / 0 in every block.
//
// LDS: 6 arrays of NL entries (40 bytes per lane: 10 KB / 20 KB); no scratch; the kernel holds no state worth an occupancy bound.
#pragma once
#include "clc_resident.hpp"

namespace clc {

// log(1 + x) for finite x >= 0, accurate RELATIVE to the result also where x is tiny.  u = fl(1 + x) drops the low bits of a small x
// (x = 3e-9, a residual of a few micrometres: 4e-8 of log(u) — nothing in a solve's total, but a block of ONE record is judged on its
// own cost); log(u) x / (u - 1) puts them back: log_ge1 is accurate relative to u - 1 next to 1 (f = u - 1 is exact there), and the
// factor x / (u - 1) is the ratio of the wanted argument to the rounded one.  u == 1: the series' first term.
__device__ __forceinline__ double log1p_pos(double x) {
  const double u = 1.0 + x;
  const double d = u - 1.0;
  return d == 0.0 ? x : log_ge1(u) * (x / d);
}

template <int NL>
__global__ __launch_bounds__(NL) void block_scores_kernel(
    const double* __restrict__ xyl, const double* __restrict__ zl, const ResLane* __restrict__ lane_desc,
    const double* __restrict__ groups, const unsigned int* __restrict__ lane_block, const int ppl, const int n_blocks,
    const double* __restrict__ poses, const double lf, const int use_loss, const double tau, double* __restrict__ ssq,
    double* __restrict__ cost, int32_t* __restrict__ inliers) {
  __shared__ double sh_q[NL], sh_c[NL], sh_bq[NL], sh_bc[NL];
  __shared__ int sh_i[NL], sh_bi[NL];
  __shared__ int sh_blk[NL];  // the lane's block; -1: idle lane
  const int k = blockIdx.x, tid = threadIdx.x;
  // candidate pose: host memory behind PCIe — requested first, consumed after the lane's first points are on their way
  double x[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) x[i] = poses[7 * (size_t)k + i];
  const ResLane dl = lane_desc[tid];
  const int cnt = dl.cnt;
  sh_blk[tid] = cnt > 0 ? (int)lane_block[tid] : -1;
  const double* __restrict__ gp = groups + (size_t)dl.gid * GROUP_DOUBLES;
  const bool on = cnt > 0;
  const double nx = on ? gp[0] : 0.0, ny = on ? gp[1] : 0.0, nz = on ? gp[2] : 0.0, pd = on ? gp[3] : 0.0, ps = on ? gp[4] : 0.0;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 7; ++i) finite = finite && ((__double2hiint(x[i]) >> 20) & 0x7FF) != 0x7FF;  // (the same pose in every lane)
  double R[9];
  quat_to_rot(x + 3, R);
  RowPlane q;
  rows_plane_setup(R, x, nx, ny, nz, pd, ps, q);
  const double inv_lf2 = 1.0 / (lf * lf);
  const v2d* __restrict__ src = reinterpret_cast<const v2d*>(xyl) + tid;
  const double* __restrict__ srcz = zl != nullptr ? zl + tid : nullptr;
  double a_q = 0.0, a_l = 0.0;
  int a_i = 0;
  // slots [0, cnt) are the lane's points, [cnt, ppl) zero padding; every lane reads the ppl rows of the layout (in bounds for idle lanes
  // too: a row holds NL slots)
#pragma unroll 4
  for (int j = 0; j < ppl; ++j) {
    const v2d v = src[(size_t)j * NL];
    const double vz = srcz != nullptr ? srcz[(size_t)j * NL] : 0.0;
    const double r0 = fma(q.mz, vz, fma(q.my, v[1], fma(q.mx, v[0], q.c0)));
    const bool valid = j < cnt;
    const double r2 = valid ? r0 * r0 : 0.0;
    a_q += r2;
    if (use_loss) a_l += log1p_pos(r2 * inv_lf2);  // (a padded slot: log1p(0) = 0)
    a_i += (valid && fabs(r0) <= tau) ? 1 : 0;
  }
  const double l_q = q.s2 * a_q;
  sh_q[tid] = l_q;
  sh_c[tid] = use_loss ? 0.5 * (lf * lf) * (q.s2 * a_l) : 0.5 * l_q;
  sh_i[tid] = a_i;
  __syncthreads();
  // the first lane of every block adds the block's lanes, in lane order
  const int b = sh_blk[tid];
  const bool head = b >= 0 && (tid == 0 || sh_blk[tid - 1] != b);
  double t_q = 0.0, t_c = 0.0;
  int t_i = 0;
  if (head) {
    for (int u = tid; u < NL && sh_blk[u] == b; ++u) {
      t_q += sh_q[u];
      t_c += sh_c[u];
      t_i += sh_i[u];
    }
    if (!finite) { t_q = __builtin_nan(""); t_c = __builtin_nan(""); t_i = 0; }
  }
  // out, NL blocks at a time: staged in LDS so that a row leaves as consecutive stores
  for (int base = 0; base < n_blocks; base += NL) {
    sh_bq[tid] = finite ? 0.0 : __builtin_nan("");
    sh_bc[tid] = finite ? 0.0 : __builtin_nan("");
    sh_bi[tid] = 0;
    __syncthreads();
    if (head && b >= base && b < base + NL) {
      sh_bq[b - base] = t_q;
      sh_bc[b - base] = t_c;
      sh_bi[b - base] = t_i;
    }
    __syncthreads();
    if (base + tid < n_blocks) {
      const size_t o = (size_t)k * (size_t)n_blocks + (size_t)(base + tid);
      if (ssq != nullptr) ssq[o] = sh_bq[tid];
      if (cost != nullptr) cost[o] = sh_bc[tid];
      if (inliers != nullptr) inliers[o] = sh_bi[tid];
    }
    __syncthreads();
  }
}

}  // namespace clc
