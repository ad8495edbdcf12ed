// clc_batchflow.hpp — the two steps either side of the batched solve, for every problem of an uploaded batch at once
// (main/calibr_offline.cpp:166-170 runs them around CamLaserCalibration):
//
//   K8  closed-form start (CamLaserCalClosedSolution, src/LaseCamCalCeres.cpp:112-203)
//       bf_normal9_rows_kernel / bf_normal9_tiles_kernel   the 45 accumulators of K5 (accumulate_normal9 layout) per
//                                                           workgroup, blocks_per_problem workgroups per problem
//       bf_closed_form_kernel                               one wave per problem: fixed-order sum of the partial rows,
//                                                           9x9 Jacobi eigenvalues, pivoted LDL^T, U V^T, Tlc -> Tcl pose
//   K9  analysis pass (src/LaseCamCalCeres.cpp:316-381: H, b, chi2 without the loss, SVD of H, null-space count)
//       bf_info_rows_kernel / bf_info_tiles_kernel         the 28 accumulators of K4 at the problem's own pose, no loss
//       bf_info_kernel                                      one wave per problem: sum, 6x6 Jacobi eigen-decomposition
//
// The dense back end restates clc_host.hpp (jacobi_eig_sym, ldlt_solve_n, nearest_orthogonal3,
// closed_form_from_normal) statement for statement: same cyclic sweep order and stopping rule, same pivot rule, same
// pseudo-inverse of D.  The Jacobi rotations run one matrix row per lane (LaneRows: a single lane holding 81 + 81
// doubles spills); the O(n^3 / 6) LDL^T solve and the 3x3 steps run on the wave's first lane.  The same source
// compiles for the host (tests/shim/batchflow_shim.cpp, g++), where the lanes of a LaneRows are a loop over the rows.
#pragma once
#include "../../include/clc.h"
#include "clc_math.hpp"
#if defined(__HIPCC__)
#include "clc_frontend.hpp"
#endif

namespace clc {
namespace bf {

// The dense back end runs without FMA contraction (hipcc's -ffp-contract=on would fuse a*b - c*d): every operation rounds as in the
// host back end, so a normal equation that arrives bit for bit as the single-problem call reduces it gives bit for bit its answer —
// on a rank-deficient system the Schur complements then cancel to the same exact zeros instead of to rounding residues that the
// pseudo-inverse of D would amplify.
#if defined(__clang__)
#define CLC_BF_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CLC_BF_NO_CONTRACT
#endif

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ double bcast_d(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ bool lead_lane() { return (threadIdx.x & 63) == 0; }
#else
CLC_HD bool lead_lane() { return true; }
#endif

// An N x N matrix, one row per lane (lanes 0..N-1 of the wave).  at(r, j): element (r, j) broadcast to every lane (wave-uniform
// r); each(f): f(k, row) on the lane that holds row k; rotate_rows: the row half of a Jacobi rotation.  Host: all rows in one array, each() a loop — the same statements in the
// same order as the wave runs them.
template <int N>
struct LaneRows {
#if defined(__HIP_DEVICE_COMPILE__)
  double r[N];
  __device__ __forceinline__ double at(int row, int j) const { return bcast_d(r[j], row); }
  template <class F>
  __device__ __forceinline__ void each(F f) {
    const int k = threadIdx.x & 63;
    if (k < N) f(k, r);
  }
  // rows p, q <- c row_p - s row_q, s row_p + c row_q: the two lanes swap rows through ds_bpermute (a broadcast of both rows
  // through v_readlane would hold 2 N doubles in SGPRs — the 9x9 kernel then spills SGPRs)
  __device__ __forceinline__ void rotate_rows(int p, int q, double c, double s) {
    CLC_BF_NO_CONTRACT
    const int k = threadIdx.x & 63;
    const int partner = (k == p) ? q : p;
    double o[N];
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = __shfl(r[j], partner, 64);
    if (k == p) {
#pragma unroll
      for (int j = 0; j < N; ++j) r[j] = c * r[j] - s * o[j];
    } else if (k == q) {
#pragma unroll
      for (int j = 0; j < N; ++j) r[j] = s * o[j] + c * r[j];
    }
  }
#else  // (the host pass of hipcc compiles the kernels against this form too: never run there)
  double m[N][N];
  CLC_HD double at(int row, int j) const { return m[row][j]; }
  template <class F>
  CLC_HD void each(F f) {
    for (int k = 0; k < N; ++k) f(k, m[k]);
  }
  CLC_HD void rotate_rows(int p, int q, double c, double s) {
    CLC_BF_NO_CONTRACT
    for (int j = 0; j < N; ++j) {
      const double apk = m[p][j], aqk = m[q][j];
      m[p][j] = c * apk - s * aqk;
      m[q][j] = s * apk + c * aqk;
    }
  }
#endif
};

// jacobi_eig_sym (clc_host.hpp) on a LaneRows matrix: cyclic sweeps over (p, q) in row order, stop when the sum of the squared
// strictly-upper entries is exactly zero (the order of that sum cannot change a zero test), at most 64 sweeps.  Eigenvalues
// descending into w (every lane), the eigenvectors (WANT_V) into the columns of V.  The descending order is the stable one of
// std::sort on at most 16 elements (insertion sort): rank of i = #{j : d_j > d_i} + #{j < i : d_j == d_i}.
template <int N, bool WANT_V>
CLC_HD void jacobi_rows(LaneRows<N>& A, LaneRows<N>& V, double* w) {
  CLC_BF_NO_CONTRACT
  if (WANT_V)
    V.each([&](int k, double* v) {
#pragma unroll
      for (int j = 0; j < N; ++j) v[j] = (k == j) ? 1.0 : 0.0;
    });
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = i + 1; j < N; ++j) {
        const double a = A.at(i, j);
        off += a * a;
      }
    if (off == 0.0) break;
#pragma unroll
    for (int p = 0; p < N; ++p)
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double apq = A.at(p, q);
        if (apq == 0.0) continue;
        const double theta = (A.at(q, q) - A.at(p, p)) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        A.each([&](int, double* a) {  // A <- A G
          const double akp = a[p], akq = a[q];
          a[p] = c * akp - s * akq;
          a[q] = s * akp + c * akq;
        });
        A.rotate_rows(p, q, c, s);  // A <- G^T A
        if (WANT_V)
          V.each([&](int, double* v) {  // V <- V G
            const double vkp = v[p], vkq = v[q];
            v[p] = c * vkp - s * vkq;
            v[q] = s * vkp + c * vkq;
          });
      }
  }
  double d[N];
  int rank[N];
#pragma unroll
  for (int i = 0; i < N; ++i) d[i] = A.at(i, i);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) r += (d[j] > d[i] || (j < i && d[j] == d[i])) ? 1 : 0;
    rank[i] = r;
  }
#pragma unroll
  for (int c = 0; c < N; ++c) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) v = (rank[i] == c) ? d[i] : v;
    w[c] = v;
  }
  if (WANT_V)
    V.each([&](int, double* v) {
      double o[N];
#pragma unroll
      for (int c = 0; c < N; ++c) {
        double x = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) x = (rank[i] == c) ? v[i] : x;
        o[c] = x;
      }
#pragma unroll
      for (int c = 0; c < N; ++c) v[c] = o[c];
    });
}

// jacobi_eig_sym of a small matrix in one thread (the 3x3 M^T M of nearest_orthogonal3).
template <int N>
CLC_HD void jacobi_small(const double* Ain, double* w, double* V) {
  CLC_BF_NO_CONTRACT
#if defined(__HIP_DEVICE_COMPILE__)
  // one thread: its own LaneRows are the whole matrix — restate the host loop on local arrays
  double a[N * N];
  for (int i = 0; i < N * N; ++i) a[i] = Ain[i];
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) V[i * N + j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0;
    for (int i = 0; i < N; ++i)
      for (int j = i + 1; j < N; ++j) off += a[i * N + j] * a[i * N + j];
    if (off == 0.0) break;
#pragma unroll
    for (int p = 0; p < N; ++p)
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double apq = a[p * N + q];
        if (apq == 0.0) continue;
        const double theta = (a[q * N + q] - a[p * N + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double akp = a[k * N + p], akq = a[k * N + q];
          a[k * N + p] = c * akp - s * akq;
          a[k * N + q] = s * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double apk = a[p * N + k], aqk = a[q * N + k];
          a[p * N + k] = c * apk - s * aqk;
          a[q * N + k] = s * apk + c * aqk;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double vkp = V[k * N + p], vkq = V[k * N + q];
          V[k * N + p] = c * vkp - s * vkq;
          V[k * N + q] = s * vkp + c * vkq;
        }
      }
  }
  double d[N], Vt[N * N];
  int rank[N];
#pragma unroll
  for (int i = 0; i < N; ++i) d[i] = a[i * N + i];
#pragma unroll
  for (int i = 0; i < N * N; ++i) Vt[i] = V[i];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) r += (d[j] > d[i] || (j < i && d[j] == d[i])) ? 1 : 0;
    rank[i] = r;
  }
#pragma unroll
  for (int c = 0; c < N; ++c) {
    double x = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) x = (rank[i] == c) ? d[i] : x;
    w[c] = x;
#pragma unroll
    for (int r = 0; r < N; ++r) {
      double y = 0.0;
#pragma unroll
      for (int i = 0; i < N; ++i) y = (rank[i] == c) ? Vt[r * N + i] : y;
      V[r * N + c] = y;
    }
  }
#else
  LaneRows<N> A, Vr;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) A.m[i][j] = Ain[i * N + j];
  jacobi_rows<N, true>(A, Vr, w);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) V[i * N + j] = Vr.m[i][j];
#endif
}

// ldlt_solve_n (clc_host.hpp) for n = 9, one thread; A (81, both triangles) is overwritten — the wave keeps it in LDS.
CLC_HD void ldlt_solve9(double* A, const double* b, double* x) {
  CLC_BF_NO_CONTRACT
  constexpr int n = 9;
  double D[9], y[9];
  int perm[9];
#pragma unroll
  for (int i = 0; i < n; ++i) perm[i] = i;
#pragma unroll
  for (int k = 0; k < n; ++k) {
    int piv = k;
    double big = fabs(A[k * n + k]);
#pragma unroll
    for (int i = k + 1; i < n; ++i)
      if (fabs(A[i * n + i]) > big) { big = fabs(A[i * n + i]); piv = i; }
    if (piv != k) {  // symmetric row/column swap (the full matrix is kept, both triangles)
      for (int j = 0; j < n; ++j) { const double t = A[k * n + j]; A[k * n + j] = A[piv * n + j]; A[piv * n + j] = t; }
      for (int i = 0; i < n; ++i) { const double t = A[i * n + k]; A[i * n + k] = A[i * n + piv]; A[i * n + piv] = t; }
      // perm[k] <-> perm[piv] with compile-time indices only (a dynamically indexed register array goes to scratch)
      int pk = 0;
#pragma unroll
      for (int i = k + 1; i < n; ++i) pk = (i == piv) ? perm[i] : pk;
#pragma unroll
      for (int i = k + 1; i < n; ++i) perm[i] = (i == piv) ? perm[k] : perm[i];
      perm[k] = pk;
    }
    double d = A[k * n + k];
#pragma unroll
    for (int j = 0; j < k; ++j) d -= A[k * n + j] * A[k * n + j] * D[j];
    D[k] = d;
#pragma unroll
    for (int i = k + 1; i < n; ++i) {
      double v = A[i * n + k];
#pragma unroll
      for (int j = 0; j < k; ++j) v -= A[i * n + j] * A[k * n + j] * D[j];
      A[i * n + k] = (d != 0.0) ? v / d : 0.0;
    }
  }
#pragma unroll
  for (int i = 0; i < n; ++i) {  // P b
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < n; ++j) v = (perm[i] == j) ? b[j] : v;
    y[i] = v;
  }
#pragma unroll
  for (int i = 0; i < n; ++i)  // L^-1
#pragma unroll
    for (int j = 0; j < i; ++j) y[i] -= A[i * n + j] * y[j];
#pragma unroll
  for (int i = 0; i < n; ++i) y[i] = (fabs(D[i]) > 2.2250738585072014e-308) ? y[i] / D[i] : 0.0;  // D^+
#pragma unroll
  for (int i = n - 1; i >= 0; --i)  // L^-T
#pragma unroll
    for (int j = i + 1; j < n; ++j) y[i] -= A[j * n + i] * y[j];
#pragma unroll
  for (int j = 0; j < n; ++j) {  // P^T
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < n; ++i) v = (perm[i] == j) ? y[i] : v;
    x[j] = v;
  }
}

CLC_HD void cross3(const double* a, const double* b, double* c) {
  CLC_BF_NO_CONTRACT
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// nearest_orthogonal3 (clc_host.hpp), one thread.
CLC_HD void nearest_orthogonal3(const double* M, double* Q) {
  CLC_BF_NO_CONTRACT
  double MtM[9], w[3], V[9], U[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) s += M[3 * k + i] * M[3 * k + j];
      MtM[3 * i + j] = s;
    }
  jacobi_small<3>(MtM, w, V);  // descending
  const double smax = sqrt(fmax(w[0], 0.0));
  int have[3] = {0, 0, 0};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double u[3] = {0, 0, 0};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) u[r] += M[3 * r + k] * V[3 * k + c];
    const double nrm = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
    if (nrm > 1e-14 * smax && nrm > 0.0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) U[3 * r + c] = u[r] / nrm;
      have[c] = 1;
    }
  }
  if (!have[0]) { U[0] = 1; U[3] = 0; U[6] = 0; have[0] = 1; }
  if (!have[1]) {  // any unit vector orthogonal to column 0
    const double a[3] = {U[0], U[3], U[6]};
    const int m = fabs(a[0]) <= fabs(a[1]) ? (fabs(a[0]) <= fabs(a[2]) ? 0 : 2) : (fabs(a[1]) <= fabs(a[2]) ? 1 : 2);
    const double e[3] = {m == 0 ? 1.0 : 0.0, m == 1 ? 1.0 : 0.0, m == 2 ? 1.0 : 0.0};
    double c1[3];
    cross3(a, e, c1);
    const double nrm = sqrt((c1[0] * c1[0] + c1[1] * c1[1]) + c1[2] * c1[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) U[3 * r + 1] = c1[r] / nrm;
    have[1] = 1;
  }
  if (!have[2]) {
    const double a[3] = {U[0], U[3], U[6]}, b2[3] = {U[1], U[4], U[7]};
    double c2[3];
    cross3(a, b2, c2);
#pragma unroll
    for (int r = 0; r < 3; ++r) U[3 * r + 2] = c2[r];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) s += U[3 * i + k] * V[3 * j + k];
      Q[3 * i + j] = s;
    }
}

// Eigen::Quaterniond(Matrix3d) (simdata.rot_to_quat_wxyz: the same branch order) -> (x, y, z, w).
CLC_HD void rot_to_quat_xyzw(const double* m, double* q) {
  CLC_BF_NO_CONTRACT
  double t = (m[0] + m[4]) + m[8];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t;
    q[1] = (m[2] - m[6]) * t;
    q[2] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[4 * i]) i = 2;
    // (j, k) = the two indices after i, cyclically; the three cases spelled out (no runtime indexing)
    double mij[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) mij[r][c] = m[3 * r + c];
    double v[3];
    double w;
    if (i == 0) {
      t = sqrt(mij[0][0] - mij[1][1] - mij[2][2] + 1.0);
      v[0] = 0.5 * t; t = 0.5 / t;
      w = (mij[2][1] - mij[1][2]) * t; v[1] = (mij[1][0] + mij[0][1]) * t; v[2] = (mij[2][0] + mij[0][2]) * t;
    } else if (i == 1) {
      t = sqrt(mij[1][1] - mij[2][2] - mij[0][0] + 1.0);
      v[1] = 0.5 * t; t = 0.5 / t;
      w = (mij[0][2] - mij[2][0]) * t; v[2] = (mij[2][1] + mij[1][2]) * t; v[0] = (mij[0][1] + mij[1][0]) * t;
    } else {
      t = sqrt(mij[2][2] - mij[0][0] - mij[1][1] + 1.0);
      v[2] = 0.5 * t; t = 0.5 / t;
      w = (mij[1][0] - mij[0][1]) * t; v[0] = (mij[0][2] + mij[2][0]) * t; v[1] = (mij[1][2] + mij[2][1]) * t;
    }
    q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; q[3] = w;
  }
}

// The 9x9 normal equation from the 45 accumulators of K5 (the expansion of clc_closed_form): row k = 3 ci + ri of A^T A on the
// lane of row k, A^T b to every lane.
CLC_HD int tri3(int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo * 3 - (lo * (lo - 1)) / 2 + (hi - lo);
}

// Back end of closed_form_from_normal (clc_host.hpp) + the start pose: A holds A^T A (one row per lane), A81 the same matrix
// where the first lane reads it (LDS on the device; overwritten), Atb the right-hand side.  Returns CLC_OK / CLC_ERR_NONFINITE on
// the first lane; Tlc[16], *unobservable, sv9[9] and pose7 = [t, qx, qy, qz, qw] of Tcl = Tlc^-1 (simdata.tlc_to_tcl,
// pose7_from_T) are valid on the first lane.
CLC_HD int closed_form_rows(LaneRows<9>& A, double* A81, const double* Atb, double* Tlc, int* unobservable, double* sv9,
                            double* pose7) {
    CLC_BF_NO_CONTRACT
  double w[9];
  jacobi_rows<9, false>(A, A, w);  // :162 (the eigenvectors are not used)
  int un = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    if (w[i] < 1e-10) un = 1;  // :167
    sv9[i] = w[i];
  }
  *unobservable = un;
  if (!lead_lane()) return CLC_OK;
  double H[9];
  ldlt_solve9(A81, Atb, H);  // :181
  const double *h1 = H, *h2 = H + 3, *h3 = H + 6;
  double h12[3];
  cross3(h1, h2, h12);
  const double Rlc[9] = {h1[0], h1[1], h1[2], h2[0], h2[1], h2[2], h12[0], h12[1], h12[2]};  // :187-191
  double tlc[3], Q[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)  // :192
    tlc[i] = -((Rlc[3 * i] * h3[0] + Rlc[3 * i + 1] * h3[1]) + Rlc[3 * i + 2] * h3[2]);
  nearest_orthogonal3(Rlc, Q);  // :195-196
#pragma unroll
  for (int i = 0; i < 16; ++i) Tlc[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Tlc[4 * i + j] = Q[3 * i + j];
    Tlc[4 * i + 3] = tlc[i];
  }
  Tlc[15] = 1.0;
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 16; ++i) finite = finite && isfinite(Tlc[i]);
  // Tcl = [Rlc^T, -Rlc^T t] (calibr_simulation.cpp:129), pose [t, q] (LaseCamCalCeres.cpp:215-219)
  double Rcl[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rcl[3 * i + j] = Q[3 * j + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) pose7[i] = -((Rcl[3 * i] * tlc[0] + Rcl[3 * i + 1] * tlc[1]) + Rcl[3 * i + 2] * tlc[2]);
  rot_to_quat_xyzw(Rcl, pose7 + 3);
  return finite ? CLC_OK : CLC_ERR_NONFINITE;
}

// Per-problem outputs (doubles) of the two finishing kernels.
constexpr int CF_OUT = 34;    // Tlc[16] pose7[7] sv9[9] unobservable status
constexpr int INFO_OUT = 71;  // H21 b[6] chi2 sv[6] V[36] n_null

#if defined(__HIPCC__)

// ---------------------------------------------------------------------------------------
// K8 — the 9x9 normal equation of every problem (K5's accumulators and accumulate_normal9 / Normal9Rows arithmetic),
// blocks_per_problem workgroups per problem, one 45-double partial row per workgroup.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void block_store45(const double (&acc)[NACC9], double* __restrict__ out) {
  __shared__ double wsum[BLOCK / 64][NACC9];
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < NACC9; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) wsum[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < NACC9) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) s += wsum[w][threadIdx.x];
    out[threadIdx.x] = s;
  }
}

template <int STRIDE>
__global__ __launch_bounds__(BLOCK) void bf_normal9_rows_kernel(const double* __restrict__ xy, const RowDesc* __restrict__ desc,
                                                                const long long* __restrict__ prob_row, const int blocks_per_problem,
                                                                double* __restrict__ partials) {
  const int prob = blockIdx.x / blocks_per_problem;
  const int j = blockIdx.x - prob * blocks_per_problem;
  double acc[NACC9];
#pragma unroll
  for (int i = 0; i < NACC9; ++i) acc[i] = 0.0;
  const int lane = threadIdx.x & 63;
  const long long r0 = prob_row[prob], r1 = prob_row[prob + 1];
  const WaveMap wm = make_wave_map<BLOCK>(j, blocks_per_problem, threadIdx.x >> 6);
  Normal9Rows pol;
  stream_rows_policy<Normal9Rows, false, ROWS_DEPTH, STRIDE>(pol, xy, desc, r0 + wm.begin(r1 - r0), r0 + wm.end(r1 - r0), lane,
                                                              [](PoseU&) { return true; }, acc);
  block_store45(acc, partials + (size_t)blockIdx.x * NACC9);
}

static __global__ __launch_bounds__(BLOCK) void bf_normal9_tiles_kernel(const double* __restrict__ tiles, const long long* __restrict__ tile_off,
                                                                        const long long* __restrict__ n_obs, const int blocks_per_problem,
                                                                        double* __restrict__ partials) {
  const int prob = blockIdx.x / blocks_per_problem;
  const int j = blockIdx.x - prob * blocks_per_problem;
  double acc[NACC9];
#pragma unroll
  for (int i = 0; i < NACC9; ++i) acc[i] = 0.0;
  const int lane = threadIdx.x & 63;
  const long long n = n_obs[prob];
  const double* base_p = tiles + tile_off[prob] * TILE_DOUBLES;
  const WaveMap wm = make_wave_map<BLOCK>(j, blocks_per_problem, threadIdx.x >> 6);
  const long long T = (n + TILE - 1) / TILE;
  const long long t1 = wm.end(T);
  for (long long tile = wm.begin(T); tile < t1; ++tile) {  // fields n.x n.y n.z d p.x p.y of the 64-byte tile
    const double2* base = reinterpret_cast<const double2*>(base_p + tile * TILE_DOUBLES) + lane;
    double2 f[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) f[k] = base[k * 64];
    const long long k0 = tile * TILE + 2 * lane;
    if (k0 < n) accumulate_normal9(f[0].x, f[1].x, f[2].x, f[3].x, f[4].x, f[5].x, acc);
    if (k0 + 1 < n) accumulate_normal9(f[0].y, f[1].y, f[2].y, f[3].y, f[4].y, f[5].y, acc);
  }
  block_store45(acc, partials + (size_t)blockIdx.x * NACC9);
}

// Fixed-order sum over the problem's partial rows (row j = 0, 1, ... in order, eight loads in flight): lane c < NA -> column c.
template <int NA>
__device__ __forceinline__ double sum_partials(const double* __restrict__ partials, int prob, int bpp, int c) {
  double s = 0.0;
  if (c >= NA) return s;
  const double* p = partials + (size_t)prob * bpp * NA + c;
  int j = 0;
  for (; j + 8 <= bpp; j += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(j + u) * NA];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; j < bpp; ++j) s += p[(size_t)j * NA];
  return s;
}

// One wave per problem: reduce, expand, back end of the closed form, the start pose.  out: CF_OUT doubles per problem
// (page-locked host memory mapped into the device).
static __global__ __launch_bounds__(64) void bf_closed_form_kernel(const double* __restrict__ partials, const int blocks_per_problem,
                                                                   const long long* __restrict__ n_obs, double* __restrict__ out) {
  const int prob = blockIdx.x;
  const int lane = threadIdx.x;
  __shared__ double acc[NACC9];
  __shared__ double A81[81];
  const double s = sum_partials<NACC9>(partials, prob, blocks_per_problem, lane);
  if (lane < NACC9) acc[lane] = s;
  __syncthreads();
  double* o = out + (size_t)prob * CF_OUT;
  if (n_obs[prob] == 0) {
    if (lane == 0) o[33] = (double)CLC_ERR_NO_DATA;
    return;
  }
  LaneRows<9> A;
  double Atb[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Atb[k] = acc[36 + k];
  A.each([&](int k, double* a) {  // row k = 3 ci + ri (clc_closed_form's expansion)
    const int ci = k / 3, ri = k - 3 * (k / 3);
#pragma unroll
    for (int cj = 0; cj < 3; ++cj)
#pragma unroll
      for (int rj = 0; rj < 3; ++rj) {
        const double v = acc[6 * tri3(ci, cj) + tri3(ri, rj)];
        a[3 * cj + rj] = v;
        A81[9 * k + 3 * cj + rj] = v;
      }
  });
  __syncthreads();
  double Tlc[16], sv9[9], pose7[7];
  int un = 0;
  const int rc = closed_form_rows(A, A81, Atb, Tlc, &un, sv9, pose7);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = Tlc[i];
#pragma unroll
    for (int i = 0; i < 7; ++i) o[16 + i] = pose7[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) o[23 + i] = sv9[i];
    o[32] = (double)un;
    o[33] = (double)rc;
  }
}

// ---------------------------------------------------------------------------------------
// K9 — the analysis pass of every problem: K4's streaming without the loss at the problem's own pose (poses[7 P]).
// ---------------------------------------------------------------------------------------
template <bool Z>
__global__ __launch_bounds__(BLOCK) void bf_info_rows_kernel(const double* __restrict__ xy, const RowDesc* __restrict__ desc,
                                                             const long long* __restrict__ prob_row, const double* __restrict__ poses,
                                                             const int blocks_per_problem, double* __restrict__ partials) {
  const int prob = blockIdx.x / blocks_per_problem;
  const int j = blockIdx.x - prob * blocks_per_problem;
  auto get_pose = [&](PoseU& P) -> bool {
    load_pose(poses + 7 * (size_t)prob, P);
    return true;
  };
  const double inv_lf2 = 1.0;  // (no loss: not read)
  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
  const int lane = threadIdx.x & 63;
  const long long r0 = prob_row[prob], r1 = prob_row[prob + 1];
  const WaveMap wm = make_wave_map<BLOCK>(j, blocks_per_problem, threadIdx.x >> 6);
  stream_rows<false, false, ROWS_DEPTH, Z>(xy, desc, r0 + wm.begin(r1 - r0), r0 + wm.end(r1 - r0), lane, get_pose, inv_lf2, acc);
  block_reduce_store<BLOCK / 64>(acc, 0, partials + (size_t)blockIdx.x * NACC);
}

static __global__ __launch_bounds__(BLOCK) void bf_info_tiles_kernel(const double* __restrict__ tiles, const long long* __restrict__ tile_off,
                                                                     const long long* __restrict__ n_obs, const double* __restrict__ poses,
                                                                     const int blocks_per_problem, double* __restrict__ partials) {
  const int prob = blockIdx.x / blocks_per_problem;
  const int j = blockIdx.x - prob * blocks_per_problem;
  auto get_pose = [&](PoseU& P) -> bool {
    load_pose(poses + 7 * (size_t)prob, P);
    return true;
  };
  const double inv_lf2 = 1.0;
  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
  const int lane = threadIdx.x & 63;
  const WaveMap wm = make_wave_map<BLOCK>(j, blocks_per_problem, threadIdx.x >> 6);
  stream_tiles<false, true, true, false>(tiles + tile_off[prob] * TILE_DOUBLES, n_obs[prob], wm, lane, get_pose, inv_lf2, acc);
  block_reduce_store<BLOCK / 64>(acc, 0, partials + (size_t)blockIdx.x * NACC);
}

// One wave per problem: H (21), b = -g, chi2 = 2 cost, the 6x6 eigen-decomposition of H (sv descending, V), n_null (sv < 1e-8).
static __global__ __launch_bounds__(64) void bf_info_kernel(const double* __restrict__ partials, const int blocks_per_problem,
                                                            double* __restrict__ out) {
  const int prob = blockIdx.x;
  const int lane = threadIdx.x;
  __shared__ double acc[NACC];
  const double s = sum_partials<NACC>(partials, prob, blocks_per_problem, lane);
  if (lane < NACC) acc[lane] = s;
  __syncthreads();
  double* o = out + (size_t)prob * INFO_OUT;
  if (lane < 27) o[lane] = lane < 21 ? s : -s;  // H21, b = -g (:357)
  if (lane == 27) o[27] = 2.0 * (0.5 * s);      // chi2 = 2 cost, cost = finalize_cost(acc27) (:359)
  LaneRows<6> H, V;
  H.each([&](int k, double* h) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const int a = k < c ? k : c, b = k < c ? c : k;
      h[c] = acc[6 * a - (a * (a - 1)) / 2 + (b - a)];
    }
  });
  double sv[6];
  jacobi_rows<6, true>(H, V, sv);  // JacobiSVD(H), :366
  V.each([&](int k, double* v) {
#pragma unroll
    for (int c = 0; c < 6; ++c) o[34 + 6 * k + c] = v[c];
  });
  if (lane == 0) {
    int nn = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      o[28 + i] = sv[i];
      if (sv[i] < 1e-8) ++nn;  // :371
    }
    o[70] = (double)nn;
  }
}

#endif  // __HIPCC__

}  // namespace bf
}  // namespace clc
