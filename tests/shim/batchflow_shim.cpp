// tests/shim/batchflow_shim.cpp — TEST ONLY.  Compiles the dense back end of the batched closed form and analysis pass
// (camlasercalibratool_amd/csrc/clc_batchflow.hpp: jacobi_rows on LaneRows, ldlt_solve9, nearest_orthogonal3, closed_form_rows —
// the code one wave per problem runs) for the host with g++, where the lanes of a LaneRows are a loop over the rows, next to the
// host back end it restates (clc_host.hpp), so the two can be compared here, where there is no GPU.
#include "../../camlasercalibratool_amd/csrc/clc_batchflow.hpp"
#include "../../camlasercalibratool_amd/csrc/clc_host.hpp"

namespace {
template <int N>
void bf_eig(const double* A, double* w, double* V) {
  clc::bf::LaneRows<N> a, v;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) a.m[i][j] = A[i * N + j];
  clc::bf::jacobi_rows<N, true>(a, v, w);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) V[i * N + j] = v.m[i][j];
}
}  // namespace

extern "C" {

int shim_bf_eig(const double* A, int n, double* w, double* V) {
  if (n == 3) bf_eig<3>(A, w, V);
  else if (n == 6) bf_eig<6>(A, w, V);
  else if (n == 9) bf_eig<9>(A, w, V);
  else return -1;
  return 0;
}

void shim_host_eig(const double* A, int n, double* w, double* V) { clc::host::jacobi_eig_sym(A, n, w, V); }

void shim_bf_ldlt9(const double* A, const double* b, double* x) {
  double a[81];
  for (int i = 0; i < 81; ++i) a[i] = A[i];
  clc::bf::ldlt_solve9(a, b, x);
}

void shim_host_ldlt9(const double* A, const double* b, double* x) { clc::host::ldlt_solve_n(A, b, x, 9); }

void shim_bf_orth3(const double* M, double* Q) { clc::bf::nearest_orthogonal3(M, Q); }

void shim_host_orth3(const double* M, double* Q) { clc::host::nearest_orthogonal3(M, Q); }

// closed form from the 9x9 normal equation -> rc; Tlc[16], *un, sv9[9], pose7[7]
int shim_bf_closed_form(const double* AtA, const double* Atb, double* Tlc, int* un, double* sv9, double* pose7) {
  clc::bf::LaneRows<9> A;
  double a81[81];
  for (int i = 0; i < 9; ++i)
    for (int j = 0; j < 9; ++j) A.m[i][j] = a81[9 * i + j] = AtA[9 * i + j];
  return clc::bf::closed_form_rows(A, a81, Atb, Tlc, un, sv9, pose7);
}

int shim_host_closed_form(const double* AtA, const double* Atb, double* Tlc, int* un, double* sv9) {
  return clc::host::closed_form_from_normal(AtA, Atb, Tlc, un, sv9);
}

// the expansion of the 45 accumulators (K5 layout) into A^T A the finishing kernel does, row k on lane k
void shim_bf_expand45(const double* acc, double* AtA) {
  for (int k = 0; k < 9; ++k) {
    const int ci = k / 3, ri = k - 3 * (k / 3);
    for (int cj = 0; cj < 3; ++cj)
      for (int rj = 0; rj < 3; ++rj) AtA[9 * k + 3 * cj + rj] = acc[6 * clc::bf::tri3(ci, cj) + clc::bf::tri3(ri, rj)];
  }
}

}  // extern "C"
