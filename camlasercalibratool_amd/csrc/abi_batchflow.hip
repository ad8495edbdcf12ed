// abi_batchflow.hip — clc_closed_form_batched, clc_information_batched: the closed-form start and the analysis pass of every
// problem of the uploaded batch (K8, K9 in clc_batchflow.hpp).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "clc_batchflow.hpp"

using namespace clc_abi;

namespace {

// Workgroups per problem: enough workgroups in all to give every CU four (a batch of one large problem uses the chip), never
// fewer than eight streaming units (rows of 64 points, or 128-point tiles) per workgroup.  A batch of >= 4 x CUs problems:
// one workgroup per problem.
int flow_blocks_per_problem(const clc_handle* h, bool rows) {
  const long long P = (long long)h->n_problems;
  const long long units = rows ? h->batch_max_rows : h->batch_max_tiles;
  const long long want = 4LL * std::max(1, h->num_cus);
  long long bpp = (want + P - 1) / P;
  bpp = std::min(bpp, std::max(1LL, units / 8));
  return (int)std::max(1LL, bpp);
}

int flow_check(clc_handle* h, const char* who) {
  if (!h) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": bad argument").c_str());
  if (!h->batch.d_tiles || h->n_problems == 0) return fail(CLC_ERR_NO_DATA, (std::string(who) + ": no problems uploaded").c_str());
  if (h->n_problems > 0x7FFFFFFull) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": too many problems").c_str());
  return CLC_OK;
}

}  // namespace

extern "C" {

int clc_closed_form_batched(clc_handle* h, double* poses, double* Tlc, int32_t* unobservable, double* sv9, int32_t* status) {
  CLC_TRY(flow_check(h, "clc_closed_form_batched"));
  if (!status) return fail(CLC_ERR_INVALID_ARG, "clc_closed_form_batched: status is required");
  CLC_HIP(hipSetDevice(h->device));
  const size_t P = h->n_problems;
  const bool rows = h->batch.rows_ok;
  const int bpp = flow_blocks_per_problem(h, rows);
  const size_t n_blocks = P * (size_t)bpp;
  if (n_blocks > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_closed_form_batched: too many workgroups");
  CLC_HIP(h->d_bpartials.grow(n_blocks * clc::NACC9));
  CLC_HIP(h->h_flow.grow(P * clc::bf::CF_OUT));
  if (rows) {  // 16 B per point; rows that carry z: bar_p = (x, y, 1), only the row stride differs
    with_flags([&](auto Z) {
      hipLaunchKernelGGL((clc::bf::bf_normal9_rows_kernel<Z ? clc::ROW_DOUBLES_Z : clc::ROW_DOUBLES>), dim3((unsigned)n_blocks), dim3(clc::BLOCK), 0,
                         h->stream, h->batch.d_rxy, h->batch.d_rdesc(), h->d_prob_row, bpp, h->d_bpartials);
    }, h->batch.rows_z);
  } else {
    hipLaunchKernelGGL(clc::bf::bf_normal9_tiles_kernel, dim3((unsigned)n_blocks), dim3(clc::BLOCK), 0, h->stream, h->batch.d_tiles,
                       h->d_tile_off, h->d_nobs, bpp, h->d_bpartials);
  }
  CLC_HIP(hipGetLastError());
  hipLaunchKernelGGL(clc::bf::bf_closed_form_kernel, dim3((unsigned)P), dim3(64), 0, h->stream, h->d_bpartials, bpp, h->d_nobs,
                     h->h_flow.dev());
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipStreamSynchronize(h->stream));  // (kernel completion makes the outputs written over PCIe visible)
  for (size_t k = 0; k < P; ++k) {
    const double* o = h->h_flow + k * clc::bf::CF_OUT;
    const int st = (int)o[33];
    status[k] = st;
    if (st == CLC_ERR_NO_DATA) continue;
    if (Tlc) std::memcpy(Tlc + 16 * k, o, 16 * sizeof(double));
    if (sv9) std::memcpy(sv9 + 9 * k, o + 23, 9 * sizeof(double));
    if (unobservable) unobservable[k] = (int32_t)o[32];
    if (st == CLC_OK && poses) std::memcpy(poses + 7 * k, o + 16, 7 * sizeof(double));
  }
  return CLC_OK;
}

int clc_information_batched(clc_handle* h, const double* poses, double* H, double* b, double* chi2, double* sv, double* V,
                            int32_t* n_null) {
  CLC_TRY(flow_check(h, "clc_information_batched"));
  if (!poses || !chi2 || !sv || !n_null) return fail(CLC_ERR_INVALID_ARG, "clc_information_batched: bad argument");
  const size_t P = h->n_problems;
  {
    clc_options opt;
    clc_options_default(&opt);
    CLC_TRY(batched_check_inputs("clc_information_batched", opt, poses, P));
  }
  CLC_HIP(hipSetDevice(h->device));
  const bool rows = h->batch.rows_ok;
  const int bpp = flow_blocks_per_problem(h, rows);
  const size_t n_blocks = P * (size_t)bpp;
  if (n_blocks > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_information_batched: too many workgroups");
  CLC_HIP(h->d_bpartials.grow(n_blocks * clc::NACC));
  CLC_HIP(h->h_flow.grow(P * (clc::bf::INFO_OUT + 7)));
  // the handle's own pose buffer is read where it is; any other array is staged behind the outputs
  // (the previous call ended with a stream synchronisation: nothing still reads or writes the staging area)
  const double* d_poses;
  if (poses == h->h_poses) {
    d_poses = h->h_poses.dev();
  } else {
    std::memcpy(h->h_flow + P * clc::bf::INFO_OUT, poses, 7 * P * sizeof(double));
    d_poses = h->h_flow.dev() + P * clc::bf::INFO_OUT;
  }
  if (rows) {
    with_flags([&](auto Z) {
      hipLaunchKernelGGL((clc::bf::bf_info_rows_kernel<Z>), dim3((unsigned)n_blocks), dim3(clc::BLOCK), 0, h->stream, h->batch.d_rxy,
                         h->batch.d_rdesc(), h->d_prob_row, d_poses, bpp, h->d_bpartials);
    }, h->batch.rows_z);
  } else {
    hipLaunchKernelGGL(clc::bf::bf_info_tiles_kernel, dim3((unsigned)n_blocks), dim3(clc::BLOCK), 0, h->stream, h->batch.d_tiles, h->d_tile_off,
                       h->d_nobs, d_poses, bpp, h->d_bpartials);
  }
  CLC_HIP(hipGetLastError());
  hipLaunchKernelGGL(clc::bf::bf_info_kernel, dim3((unsigned)P), dim3(64), 0, h->stream, h->d_bpartials, bpp, h->h_flow.dev());
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipStreamSynchronize(h->stream));
  for (size_t k = 0; k < P; ++k) {
    const double* o = h->h_flow + k * clc::bf::INFO_OUT;
    if (H) {
      double* Hk = H + 36 * k;
      int idx = 0;
      for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) {
          Hk[6 * a + c] = o[idx];
          Hk[6 * c + a] = o[idx];
          ++idx;
        }
    }
    if (b) std::memcpy(b + 6 * k, o + 21, 6 * sizeof(double));
    chi2[k] = o[27];
    std::memcpy(sv + 6 * k, o + 28, 6 * sizeof(double));
    if (V) std::memcpy(V + 36 * k, o + 34, 36 * sizeof(double));
    n_null[k] = (int32_t)o[70];
  }
  return CLC_OK;
}

}  // extern "C"
