// clc_guidance.hpp — K20: pose guidance.  For every candidate board pose T_ca the information H_add that clc_information's
// H = sum J^T J would gain at the current T_cl if that pose were recorded, the eigenvalues of M + H_add and a score of them; and a
// greedy choice of k candidates.  H depends on the laser points and the poses only, not on the residuals: the prediction needs no
// noise model.
//
//   per candidate   n = R_ca e3, d = -n.t_ca, m = R_cl^T n, d_l = n.t_cl + d
//   per ray i       dir = (cos th_i, sin th_i, 0), th_i = angle_min + i angle_increment;  rho = -d_l / (m.dir);  p = rho dir;
//                   X = R_ca^T (R_cl p + t_cl - t_ca);  a hit: rho finite, range_min <= rho < range_max, board_min <= X_xy <= board_max
//   seen            c = #hits >= min_points:  H_add = (1 / c) sum_hits u u^T,  u = [n, p x m]  (the factor's Jacobian row with the
//                   reference's per-pose scale 1 / sqrt(c), clc_device.hpp);  unseen: H_add = 0
//
//   guidance_dirs_kernel    the n_rays directions (cos, sin), once per call, into a table in device memory (17 KB for 1 081 rays)
//   guidance_cast_kernel    one wave per candidate, 4 per workgroup: the lanes stride over the rays, 22 sums per lane (the count and
//                           the 21 upper-triangle entries), wave_sum of clc_campose.hpp; no atomics, a fixed order: the same bits on
//                           every run, and for a candidate alone or in a batch
//   guidance_score_kernel   one candidate per lane: cyclic Jacobi on the 6x6 M + H_add in registers (jacobi_small of
//                           clc_batchflow.hpp), the score; in a selection round also the first stage of the argmax (a workgroup's best)
//   guidance_pick_kernel    one workgroup: the second stage of the argmax over the workgroups' bests, then M += H_add[chosen]
//
// Everything numeric is CLC_HD: tests/shim/guidance_shim.cpp compiles this header for the host with g++ and runs the same code with
// the lanes as loops, in the same summation order.
#pragma once
#include "clc_campose.hpp"

namespace clc {
namespace gd {

constexpr int CAST_WAVES = 4, CAST_THREADS = 64 * CAST_WAVES;
constexpr int SCORE_THREADS = 256;
constexpr int PICK_THREADS = 256;

CLC_HD bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }

// What the kernels take of clc_guidance_options and of T_cl.
struct GuideModel {
  int32_t n_rays, min_points, criterion, reserved;
  double angle_min, angle_increment, range_min, range_max;
  double board_min[2], board_max[2];
  double eig_floor;
  double Rcl[9], tcl[3];
};

struct CastArgs {
  GuideModel g;
  const double* dirs;  // [2 n_rays] (cos, sin)
  const double* q;     // [4 n] (w, x, y, z)
  const double* t;     // [3 n]
  long long n_cand;
  int32_t* n_hits;     // [n]
  double* H_add;       // [36 n]
};

struct ScoreArgs {
  int32_t criterion, min_points;
  double eig_floor;
  const double* M;        // [36]
  const double* H_add;    // [36 n]
  const int32_t* n_hits;  // [n]
  long long n_cand;
  double* sv;             // [6 n] nullable
  double* score;          // [n] nullable
  // a selection round: candidates already chosen, and the best of every workgroup
  const unsigned char* taken;  // [n] nullable
  double* best_score;          // [workgroups]
  long long* best_index;       // [workgroups], -1: none
};

struct PickArgs {
  int round;
  long long n_blocks;
  const double* best_score;
  const long long* best_index;
  const double* H_add;
  const double* sv;      // [6 n] of this round
  const double* score;   // [n]
  double* M;             // [36] in / out
  unsigned char* taken;  // [n]
  long long* chosen;     // [k]
  double* sv_after;      // [6 k]
  double* score_after;   // [k]
};

// Direction i of the scan: th in double, as TranScanToPoints takes it.
CLC_HD void ray_dir(const GuideModel& g, int i, double* c, double* s) {
  CLC_BF_NO_CONTRACT
  const double th = g.angle_min + (double)i * g.angle_increment;
  *c = cos(th);
  *s = sin(th);
}

// One candidate: every lane of its wave calls it (host: once).  TABLE: the directions come from a.dirs; otherwise a sincos per ray.
template <bool TABLE>
CLC_HD void cast_candidate(const CastArgs& a, long long cand) {
  CLC_BF_NO_CONTRACT
  const GuideModel& g = a.g;
  double q[4], t[3];
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 4; ++i) { q[i] = a.q[4 * cand + i]; fin = fin && finite_d(q[i]); }
#pragma unroll
  for (int i = 0; i < 3; ++i) { t[i] = a.t[3 * cand + i]; fin = fin && finite_d(t[i]); }
  if (!fin) {  // (wave-uniform)
    if (bf::lead_lane()) {
      a.n_hits[cand] = -1;
#pragma unroll
      for (int i = 0; i < 36; ++i) a.H_add[36 * cand + i] = 0.0;
    }
    return;
  }
  const double qx[4] = {q[1], q[2], q[3], q[0]};
  double R[9];
  quat_to_rot(qx, R);
  const double n0 = R[2], n1 = R[5], n2 = R[8];
  const double d = -((n0 * t[0] + n1 * t[1]) + n2 * t[2]);
  const double* Rcl = g.Rcl;
  const double m0 = (Rcl[0] * n0 + Rcl[3] * n1) + Rcl[6] * n2;
  const double m1 = (Rcl[1] * n0 + Rcl[4] * n1) + Rcl[7] * n2;
  const double m2 = (Rcl[2] * n0 + Rcl[5] * n1) + Rcl[8] * n2;
  const double dl = ((n0 * g.tcl[0] + n1 * g.tcl[1]) + n2 * g.tcl[2]) + d;
  double o[3];  // t_cl - t_ca
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = g.tcl[i] - t[i];
  double s[22];
  cp::wave_sum<22>([&](int lane, double* acc) {
    for (int i = lane; i < g.n_rays; i += cp::POSE_LANES) {
      double c, sn;
      if (TABLE) { c = a.dirs[2 * i]; sn = a.dirs[2 * i + 1]; }
      else ray_dir(g, i, &c, &sn);
      const double rho = -dl / (m0 * c + m1 * sn);
      if (!(finite_d(rho) && rho >= g.range_min && rho < g.range_max)) continue;
      const double px = rho * c, py = rho * sn;
      double w[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] = (Rcl[3 * k] * px + Rcl[3 * k + 1] * py) + o[k];
      const double X = (R[0] * w[0] + R[3] * w[1]) + R[6] * w[2];
      const double Y = (R[1] * w[0] + R[4] * w[1]) + R[7] * w[2];
      if (!(X >= g.board_min[0] && X <= g.board_max[0] && Y >= g.board_min[1] && Y <= g.board_max[1])) continue;
      const double u[6] = {n0, n1, n2, py * m2, -(px * m2), px * m1 - py * m0};  // [n, p x m], p = (px, py, 0)
      acc[0] += 1.0;
      int idx = 1;
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int r = p; r < 6; ++r) { acc[idx] = fma(u[p], u[r], acc[idx]); ++idx; }
    }
  }, s);
  if (!bf::lead_lane()) return;
  const bool seen = s[0] >= (double)g.min_points;
  a.n_hits[cand] = (int32_t)s[0];
#pragma unroll
  for (int p = 0; p < 6; ++p)
#pragma unroll
    for (int r = p; r < 6; ++r) {
      const double v = seen ? s[1 + tri<6>(p, r)] / s[0] : 0.0;
      a.H_add[36 * cand + 6 * p + r] = v;
      a.H_add[36 * cand + 6 * r + p] = v;
    }
}

// Sum_k log max(sv_k, eig_floor), or sv[5].
CLC_HD double criterion_score(int criterion, double eig_floor, const double* sv) {
  CLC_BF_NO_CONTRACT
  if (criterion == CLC_GUIDE_MIN_EIG) return sv[5];
  double sc = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) sc += log(sv[k] > eig_floor ? sv[k] : eig_floor);
  return sc;
}

// One candidate (one lane; host: once): the eigenvalues of M + H_add, descending, and the score.  An unseen candidate's H_add is 0.
CLC_HD double score_candidate(const ScoreArgs& a, long long cand, double* sv) {
  CLC_BF_NO_CONTRACT
  double A[36], V[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) A[i] = a.M[i] + a.H_add[36 * cand + i];
  bf::jacobi_small<6>(A, sv, V);
  return criterion_score(a.criterion, a.eig_floor, sv);
}

// May round r choose the candidate?  Seen, not yet chosen, and a score that compares.
CLC_HD bool selectable(const ScoreArgs& a, long long cand, double score) {
  return a.n_hits[cand] >= a.min_points && !(a.taken && a.taken[cand]) && score == score;
}

// The order of the argmax: the larger score; among equal scores the lower index.  (A total order: the shape of the reduction cannot
// change its result.)  index < 0: no candidate.
CLC_HD bool better(double s, long long i, double best_s, long long best_i) {
  return i >= 0 && (best_i < 0 || s > best_s || (s == best_s && i < best_i));
}

// The round's update on the host and on the device: chosen[round], the candidate's sv and score, M += H_add[chosen], taken.
CLC_HD void pick_apply(const PickArgs& a, long long best, int lane, int lanes) {
  CLC_BF_NO_CONTRACT
  if (lane == 0) {
    a.chosen[a.round] = best;
    a.score_after[a.round] = best >= 0 ? a.score[best] : __builtin_nan("");
    if (best >= 0) a.taken[best] = 1;
  }
  for (int i = lane; i < 6; i += lanes) a.sv_after[6 * a.round + i] = best >= 0 ? a.sv[6 * best + i] : __builtin_nan("");
  if (best >= 0)
    for (int i = lane; i < 36; i += lanes) a.M[i] = a.M[i] + a.H_add[36 * best + i];
}

#if defined(__HIPCC__)

static __global__ void guidance_dirs_kernel(const GuideModel g, double* __restrict__ dirs) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= g.n_rays) return;
  double c, s;
  ray_dir(g, i, &c, &s);
  dirs[2 * i] = c;
  dirs[2 * i + 1] = s;
}

// K20 cast: one wave per candidate.
template <bool TABLE>
static __global__ __launch_bounds__(CAST_THREADS) void guidance_cast_kernel(const CastArgs a) {
  const long long cand = (long long)blockIdx.x * CAST_WAVES + (threadIdx.x >> 6);
  if (cand >= a.n_cand) return;  // (wave-uniform)
  cast_candidate<TABLE>(a, cand);
}

__device__ __forceinline__ void argmax_step(double& s, long long& i, int mask) {
  const double os = __shfl_xor(s, mask, 64);
  const long long oi = __shfl_xor(i, mask, 64);
  if (better(os, oi, s, i)) { s = os; i = oi; }
}

// The best (score, index) over the workgroup's threads, on thread 0.  (s, i) of a thread without a candidate: i = -1.
template <int WAVES>
__device__ __forceinline__ void block_argmax(double& s, long long& i, double* lds_s, long long* lds_i) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) argmax_step(s, i, m);
  if ((threadIdx.x & 63) == 0) { lds_s[threadIdx.x >> 6] = s; lds_i[threadIdx.x >> 6] = i; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < WAVES; ++w)
      if (better(lds_s[w], lds_i[w], s, i)) { s = lds_s[w]; i = lds_i[w]; }
  }
}

// K20 score: one candidate per lane.  ARGMAX: a selection round — also the workgroup's best selectable candidate.
template <bool ARGMAX>
static __global__ __launch_bounds__(SCORE_THREADS) void guidance_score_kernel(const ScoreArgs a) {
  const long long cand = (long long)blockIdx.x * SCORE_THREADS + threadIdx.x;
  double s = 0.0;
  long long idx = -1;
  if (cand < a.n_cand) {
    double sv[6];
    s = score_candidate(a, cand, sv);
    if (a.sv) {
#pragma unroll
      for (int k = 0; k < 6; ++k) a.sv[6 * cand + k] = sv[k];
    }
    if (a.score) a.score[cand] = s;
    if (ARGMAX && selectable(a, cand, s)) idx = cand;
  }
  if (ARGMAX) {
    __shared__ double lds_s[SCORE_THREADS / 64];
    __shared__ long long lds_i[SCORE_THREADS / 64];
    block_argmax<SCORE_THREADS / 64>(s, idx, lds_s, lds_i);
    if (threadIdx.x == 0) { a.best_score[blockIdx.x] = s; a.best_index[blockIdx.x] = idx; }
  }
}

#if defined(CLC_TEST_HOOKS)
// The score stage's other mapping, kept for its measurement (hooks build, clc_debug_guidance_score_rows; profiles/guidance.md): one
// wave per candidate, one matrix row per lane (LaneRows broadcasts from a wave-uniform lane: a wave holds one matrix).  The same
// statements in the same order as the one-candidate-per-lane form: the same bits.
static __global__ __launch_bounds__(CAST_THREADS) void guidance_score_rows_kernel(const ScoreArgs a) {
  const long long cand = (long long)blockIdx.x * CAST_WAVES + (threadIdx.x >> 6);
  if (cand >= a.n_cand) return;  // (wave-uniform)
  bf::LaneRows<6> A;
  A.each([&](int k, double* r) {
#pragma unroll
    for (int c = 0; c < 6; ++c) r[c] = a.M[6 * k + c] + a.H_add[36 * cand + 6 * k + c];
  });
  double sv[6];
  bf::jacobi_rows<6, false>(A, A, sv);
  if (!bf::lead_lane()) return;
  if (a.sv) {
#pragma unroll
    for (int k = 0; k < 6; ++k) a.sv[6 * cand + k] = sv[k];
  }
  if (a.score) a.score[cand] = criterion_score(a.criterion, a.eig_floor, sv);
}
#endif

// K20 pick: one workgroup; the threads stride over the workgroups' bests in index order.
static __global__ __launch_bounds__(PICK_THREADS) void guidance_pick_kernel(const PickArgs a) {
  __shared__ double lds_s[PICK_THREADS / 64];
  __shared__ long long lds_i[PICK_THREADS / 64];
  __shared__ long long best;
  double s = 0.0;
  long long idx = -1;
  for (long long b = threadIdx.x; b < a.n_blocks; b += PICK_THREADS)
    if (better(a.best_score[b], a.best_index[b], s, idx)) { s = a.best_score[b]; idx = a.best_index[b]; }
  block_argmax<PICK_THREADS / 64>(s, idx, lds_s, lds_i);
  if (threadIdx.x == 0) best = idx;
  __syncthreads();
  pick_apply(a, best, (int)threadIdx.x, PICK_THREADS);
}

#endif  // __HIPCC__

}  // namespace gd
}  // namespace clc
