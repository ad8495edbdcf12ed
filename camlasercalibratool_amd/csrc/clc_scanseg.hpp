// clc_scanseg.hpp — K7: the calibration board's segment in every scan at once, AutoGetLinePts of
// src/selectScanPoints.cpp:17-190 (the detection part, :35-165; the drawing is not reproduced).  Sequential inside a scan,
// independent across scans: one wavefront per scan.  The wave computes the range d = |p.xy| of the scan's search grid
// (every 3rd point of the window, at most 178) into LDS; one lane then runs the reference's state machine from LDS, and
// extends and ranks each segment as it is pushed (both depend on that segment alone; the first maximum wins, :139-148).
// Included by abi_frontend.hip only.
#pragma once
#include <hip/hip_runtime.h>

namespace clc {

constexpr int SEG_DELTA = 266;               // (int)(80/0.3), :42
constexpr int SEG_SKIP = 3;                  // :53
constexpr int SEG_GRID_MAX = 192;            // grid points of one window: (2 * 266 - 1) / 3 + 1 = 178 at most
constexpr int SEG_WAVES_PER_BLOCK = 4;
constexpr int SEG_FOUND = 1, SEG_NONE = 0, SEG_REF_THROWS = -1;  // include/clc.h CLC_SEG_*

// |p.xy| as Eigen's head(2).norm() computes it: each square rounded, then their sum rounded, then sqrt — no FMA (a fused
// x*x + y*y differs in the last bit, and every decision below is a threshold test on these values)
__device__ __forceinline__ double seg_range(const double* __restrict__ p) {
  return sqrt(__dadd_rn(__dmul_rn(p[0], p[0]), __dmul_rn(p[1], p[1])));
}

// points: (x, y, z) doubles of every scan; scan s owns points [off[s], off[s+1]) (absolute offsets).  seg[2 s], seg[2 s + 1]: the
// chosen segment's first and last index (inclusive, relative to the scan), or -1, -1; status[s] (nullable): SEG_*.
__global__ __launch_bounds__(64 * SEG_WAVES_PER_BLOCK) void board_segment_kernel(
    const double* __restrict__ points, const long long* __restrict__ off, const long long n_scans,
    long long* __restrict__ seg, int* __restrict__ status) {
  __shared__ double d_grid[SEG_WAVES_PER_BLOCK][SEG_GRID_MAX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long s = (long long)blockIdx.x * SEG_WAVES_PER_BLOCK + w;
  const bool active = s < n_scans;
  long long n = 0;
  const double* P = points;
  if (active) {
    n = off[s + 1] - off[s];
    P = points + 3 * off[s];
  }
  // window, :39-45 (n and the indices are int in the reference; a scan has far fewer than 2^31 points)
  const int ni = (int)n, id = ni / 2;
  const int id_left = min(id + SEG_DELTA, ni - 1), id_right = max(id - SEG_DELTA, 0);
  const int n_grid = (ni > 0 && id_left >= id_right) ? (id_left - id_right) / SEG_SKIP + 1 : 0;  // grid points in [id_right, id_left]
  for (int m = lane; m < n_grid; m += 64) d_grid[w][m] = seg_range(P + 3 * (id_right + SEG_SKIP * m));
  __syncthreads();
  if (!active || lane != 0) return;

  long long first = -1, last = -1;
  int st = SEG_NONE;
  if (ni == 0) {  // points.at(id_left = -1), :46
    st = SEG_REF_THROWS;
  } else {
    // every index the loop reads is a grid point id_right + 3 m below id_left (:57, nextPt < id_left): m < n_grid
    int cur = 0, nxt = 1;            // grid positions of currentPt, nextPt
    int seg_start = 0, seg_end = 0;  // grid positions of the open segment
    bool new_seg = true, throws = false;
    int best_cnt = -1, best_start = 0, best_end = 0;
    for (int i = id_right; i < id_left - SEG_SKIP; i += SEG_SKIP) {
      if (new_seg) {  // :59-64
        seg_start = cur;
        seg_end = nxt;
        new_seg = false;
      }
      const double d1 = d_grid[w][cur], d2 = d_grid[w][nxt];
      if (d1 < 100.0 && d2 < 100.0) {
        if (fabs(d1 - d2) < 0.05) {
          seg_end = nxt;
        } else {  // close the open segment, :75-89
          new_seg = true;
          const int ps = id_right + SEG_SKIP * seg_start, pe = id_right + SEG_SKIP * seg_end;
          const double dx = P[3 * ps] - P[3 * pe], dy = P[3 * ps + 1] - P[3 * pe + 1];
          const double dist = sqrt(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
          if (dist > 0.2 && d_grid[w][seg_start] < 2.0 && d_grid[w][seg_end] < 2.0 && pe - ps > 50) {
            // pushed: extend it (:104-126, always against the original ends) and rank it (:139-148)
            if (pe + 3 >= ni || ps - 3 < 0) {  // (pe + 3 is at most the point that closed the segment: the right side never fires)
              throws = true;  // points.at() out of range, :110 / :121
            } else {
              int a = ps, b = pe;
              const double de = d_grid[w][seg_end], ds = d_grid[w][seg_start];
              for (int j = 1; j < 4; ++j)
                if (fabs(de - seg_range(P + 3 * (pe + j))) < 0.05) b = pe + j;
              for (int j = -1; j > -4; --j)
                if (fabs(ds - seg_range(P + 3 * (ps + j))) < 0.05) a = ps + j;
              if (b - a > best_cnt) {
                best_cnt = b - a;
                best_start = a;
                best_end = b;
              }
            }
          }
        }
        cur = nxt;
      } else if (d1 > 100.0) {  // a current point at d == 100 or NaN never moves, :96-99
        cur = nxt;
      }
      ++nxt;
    }
    if (throws) {
      st = SEG_REF_THROWS;
    } else if (best_cnt >= 0) {
      st = SEG_FOUND;
      first = best_start;
      last = best_end;
    }
  }
  seg[2 * s] = first;
  seg[2 * s + 1] = last;
  if (status) status[s] = st;
}

}  // namespace clc
