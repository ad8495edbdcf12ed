// abi_frontend.hip — the calls either side of the solve: factor evaluation, manifold plus, information matrix and closed form, line fitting, scan conversion,
// board-segment detection, assembly of the offline flow's observations (K13), static stations (K14), interpolated tag poses (K15).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "abi_staging.hpp"
#include "clc_scanseg.hpp"
#include "clc_assemble.hpp"
#include "clc_stations.hpp"
#include "clc_interp.hpp"
#include "abi_assemble.hpp"

using namespace clc_abi;

namespace clc_abi {
void warm_frontend() {
  warm_kernel(reinterpret_cast<const void*>(&clc::factor_kernel));
  warm_kernel(reinterpret_cast<const void*>(&clc::normal9_kernel));
  warm_kernel(reinterpret_cast<const void*>(&clc::line_fit_kernel<true>));
}
}  // namespace clc_abi

extern "C" {

int clc_factor_evaluate(clc_handle* h, const double pose[7], double* residuals, double* jacobians) {
  if (!h || !pose || !residuals) return fail(CLC_ERR_INVALID_ARG, "clc_factor_evaluate: bad argument");
  if (!h->obs.d_tiles) return fail(CLC_ERR_NO_DATA, "clc_factor_evaluate: no observations uploaded");
  CLC_HIP(hipSetDevice(h->device));
  const size_t n = h->n_obs;
  if (n == 0) return CLC_OK;
  DevBuf<double> br(&h->pool), bj(&h->pool);
  CLC_HIP(br.alloc(n));
  if (jacobians) CLC_HIP(bj.alloc(n * 7));
  double *d_r = br.p, *d_j = bj.p;
  std::memcpy(h->h_small, pose, 7 * sizeof(double));
  CLC_HIP(hipMemcpyAsync(h->d_small, h->h_small, 7 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const int threads = 256;
  hipLaunchKernelGGL(clc::factor_kernel, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0,
                     h->stream, h->obs.d_tiles, (long long)n, h->d_small, d_r, d_j);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipStreamSynchronize(h->stream));
  CLC_HIP(hipMemcpy(residuals, d_r, n * sizeof(double), hipMemcpyDeviceToHost));
  if (jacobians) CLC_HIP(hipMemcpy(jacobians, d_j, n * 7 * sizeof(double), hipMemcpyDeviceToHost));
  return CLC_OK;
}

int clc_pose_plus(clc_handle* h, const double* x, const double* delta, double* out, size_t n) {
  if (!h || (n > 0 && (!x || !delta || !out))) return fail(CLC_ERR_INVALID_ARG, "clc_pose_plus: bad argument");
  if (n == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  DevBuf<double> buf(&h->pool);
  CLC_HIP(buf.alloc(n * 20));
  double *d_x = buf.p, *d_d = buf.p + 7 * n, *d_o = buf.p + 13 * n;
  CLC_HIP(hipMemcpy(d_x, x, n * 7 * sizeof(double), hipMemcpyHostToDevice));
  CLC_HIP(hipMemcpy(d_d, delta, n * 6 * sizeof(double), hipMemcpyHostToDevice));
  const int threads = 256;
  hipLaunchKernelGGL(clc::plus_kernel, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0,
                     h->stream, d_x, d_d, d_o, (long long)n);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipStreamSynchronize(h->stream));
  CLC_HIP(hipMemcpy(out, d_o, n * 7 * sizeof(double), hipMemcpyDeviceToHost));
  return CLC_OK;
}

int clc_pose_plus_jacobian(const double* /*x*/, double jacobian[42]) {
  if (!jacobian) return fail(CLC_ERR_INVALID_ARG, "clc_pose_plus_jacobian: NULL output");
  for (int i = 0; i < 42; ++i) jacobian[i] = 0.0;
  for (int i = 0; i < 6; ++i) jacobian[6 * i + i] = 1.0;  // [I6; 0], pose_local_parameterization.cpp:36-37
  return CLC_OK;
}

int clc_information(clc_handle* h, const double pose[7], double H[36], double b[6], double* chi2,
                    double sv[6], double V[36], int* n_null) {
  if (!h || !pose || !H || !b || !chi2 || !sv || !n_null)
    return fail(CLC_ERR_INVALID_ARG, "clc_information: bad argument");
  double cost, g[6], H21[21];
  int rc = clc_eval(h, pose, /*with_loss=*/0, 0.0, &cost, g, H21);  // :323-362: no loss
  if (rc != CLC_OK) return rc;
  int idx = 0;
  for (int a = 0; a < 6; ++a)
    for (int c = a; c < 6; ++c) {
      H[6 * a + c] = H21[idx];
      H[6 * c + a] = H21[idx];
      ++idx;
    }
  for (int a = 0; a < 6; ++a) b[a] = -g[a];  // b -= J^T r, :357
  *chi2 = 2.0 * cost;                        // chi += r*r, :359
  double Vtmp[36];
  clc::host::jacobi_eig_sym(H, 6, sv, V ? V : Vtmp);  // JacobiSVD(H), :366
  int n = 0;
  for (int i = 0; i < 6; ++i)
    if (sv[i] < 1e-8) ++n;  // :371
  *n_null = n;
  return CLC_OK;
}

int clc_closed_form(clc_handle* h, double Tlc[16], int* unobservable, double sv9[9]) {
  if (!h || !Tlc || !unobservable) return fail(CLC_ERR_INVALID_ARG, "clc_closed_form: bad argument");
  if (!h->obs.d_tiles || h->n_obs == 0) return fail(CLC_ERR_NO_DATA, "clc_closed_form: no observations uploaded");
  CLC_HIP(hipSetDevice(h->device));
  const StreamPlan sp = stream_plan(h);
  const int grid = sp.grid;
  CLC_TRY(ensure_partials(h, grid));
  if (sp.rows()) {  // rows that carry z: bar_p = (x, y, 1) — z is not read, only the row stride differs
    with_flags([&](auto Z, auto NT) {
      hipLaunchKernelGGL((clc::normal9_rows_kernel<NT, Z ? clc::ROW_DOUBLES_Z : clc::ROW_DOUBLES>), dim3(grid), dim3(clc::BLOCK), 0, h->stream,
                         h->obs.d_rxy, h->obs.d_rdesc(), h->obs.n_rows, h->d_partials);
    }, sp.layout == Layout::rows_z, sp.nt);
  } else {
    hipLaunchKernelGGL(clc::normal9_kernel, dim3(grid), dim3(clc::BLOCK), 0, h->stream, h->obs.d_tiles,
                       (long long)h->n_obs, h->d_partials);
  }
  CLC_HIP(hipGetLastError());
  hipLaunchKernelGGL(clc::reduce9_kernel, dim3(1), dim3(clc::BLOCK), 0, h->stream, h->d_partials, grid,
                     h->d_small + 128);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipMemcpyAsync(h->h_small + 128, h->d_small + 128, clc::NACC9 * sizeof(double),
                         hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  const double* r = h->h_small + 128;
  auto tri3 = [](int a, int b) { if (a > b) std::swap(a, b); return a * 3 - (a * (a - 1)) / 2 + (b - a); };
  double AtA[81], Atb[9];
  for (int ci = 0; ci < 3; ++ci)
    for (int ri = 0; ri < 3; ++ri) {
      for (int cj = 0; cj < 3; ++cj)
        for (int rj = 0; rj < 3; ++rj) AtA[9 * (3 * ci + ri) + (3 * cj + rj)] = r[6 * tri3(ci, cj) + tri3(ri, rj)];
      Atb[3 * ci + ri] = r[36 + 3 * ci + ri];
    }
  const int rc = clc::host::closed_form_from_normal(AtA, Atb, Tlc, unobservable, sv9);
  if (rc != CLC_OK) return fail(rc, "clc_closed_form: non-finite solution of the 9x9 normal equation");
  return CLC_OK;
}

}  // extern "C"

// ---- line fitting ---------------------------------------------------------------------------
namespace {
// K6 on device arrays, enqueued on the handle's stream (no wait)
void launch_line_fit(clc_handle* h, const clc_options& opt, const double* xy_dev, const long long* d_off, size_t n_scans, double* lines_dev,
                     clc_summary* summaries_dev) {
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  const unsigned blocks = (unsigned)((n_scans + clc::LINE_SCANS_PER_BLOCK - 1) / clc::LINE_SCANS_PER_BLOCK);
  if (opt.use_loss)
    hipLaunchKernelGGL((clc::line_fit_kernel<true>), dim3(blocks), dim3(clc::BLOCK), 0, h->stream, xy_dev, d_off,
                       (int)n_scans, opt, lines_dev, summaries_dev);
  else
    hipLaunchKernelGGL((clc::line_fit_kernel<false>), dim3(blocks), dim3(clc::BLOCK), 0, h->stream, xy_dev, d_off,
                       (int)n_scans, opt, lines_dev, summaries_dev);
}
}  // namespace

extern "C" {

void clc_line_options_default(clc_options* o) {
  clc_options_default(o);
  if (!o) return;
  o->max_num_iterations = 10;   // src/LaseCamCalCeres.cpp:425
  o->loss_scale_factor = 0.05;  // CauchyLoss(0.05), :416 (no per-residual scale here)
}

int clc_line_fit_batched(clc_handle* h, const clc_options* opt_in, const double* xy, const int64_t* offsets,
                         size_t n_scans, double* lines, clc_summary* summaries) {
  if (!h || !offsets || !lines || (n_scans > 0 && offsets[n_scans] > offsets[0] && !xy))
    return fail(CLC_ERR_INVALID_ARG, "clc_line_fit_batched: bad argument");
  clc_options opt;
  CLC_TRY(line_options(opt_in, &opt, "clc_line_fit_batched"));
  if (n_scans == 0) return CLC_OK;
  if (n_scans > 0x7FFFFFF0ull) return fail(CLC_ERR_INVALID_ARG, "clc_line_fit_batched: too many scans");
  std::vector<long long> rel;
  size_t n_pts;
  CLC_TRY(host_offsets("clc_line_fit_batched", offsets, n_scans, false, nullptr, &rel, &n_pts));
  for (size_t i = 0; i < 2 * n_scans; ++i)
    if (!std::isfinite(lines[i])) return fail(CLC_ERR_NONFINITE, "clc_line_fit_batched: non-finite initial line");
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  DevBuf<double> bxy(&h->pool), blines(&h->pool);
  DevBuf<long long> boff(&h->pool);
  DevBuf<clc_summary> bsum(&h->pool);
  CLC_HIP(bxy.alloc(n_pts * 2));
  CLC_HIP(boff.alloc(n_scans + 1));
  CLC_HIP(blines.alloc(n_scans * 2));
  if (summaries) CLC_HIP(bsum.alloc(n_scans));
  if (n_pts > 0) CLC_HIP(hipMemcpyAsync(bxy.p, xy + 2 * offsets[0], n_pts * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(boff.p, rel.data(), (n_scans + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(blines.p, lines, n_scans * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  launch_line_fit(h, opt, bxy.p, boff.p, n_scans, blines.p, bsum.p);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipMemcpyAsync(lines, blines.p, n_scans * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (summaries) CLC_HIP(hipMemcpyAsync(summaries, bsum.p, n_scans * sizeof(clc_summary), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  if (summaries) {
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (size_t k = 0; k < n_scans; ++k) summaries[k].solve_ms = ms;
  }
  return CLC_OK;
}

int clc_scan_to_points(clc_handle* h, const float* ranges, const int64_t* offsets, size_t n_scans,
                       const float* angle_min, const float* angle_increment, const float* range_min,
                       double* points) {
  if (!h || !offsets || (n_scans > 0 && (!angle_min || !angle_increment || !range_min)))
    return fail(CLC_ERR_INVALID_ARG, "clc_scan_to_points: bad argument");
  if (n_scans == 0) return CLC_OK;
  if (n_scans > 65535) return fail(CLC_ERR_INVALID_ARG, "clc_scan_to_points: at most 65535 scans per call");
  std::vector<long long> rel;
  size_t n;
  CLC_TRY(host_offsets("clc_scan_to_points", offsets, n_scans, false, nullptr, &rel, &n));
  if (n == 0) return CLC_OK;
  if (!ranges || !points) return fail(CLC_ERR_INVALID_ARG, "clc_scan_to_points: bad argument");
  CLC_HIP(hipSetDevice(h->device));
  long long longest = 0;
  for (size_t k = 0; k < n_scans; ++k) longest = std::max(longest, rel[k + 1] - rel[k]);
  DevBuf<float> br(&h->pool), bam(&h->pool), bai(&h->pool), brm(&h->pool);
  DevBuf<long long> boff(&h->pool);
  DevBuf<double> bp(&h->pool);
  CLC_HIP(br.alloc(n)); CLC_HIP(bam.alloc(n_scans)); CLC_HIP(bai.alloc(n_scans)); CLC_HIP(brm.alloc(n_scans));
  CLC_HIP(boff.alloc(n_scans + 1)); CLC_HIP(bp.alloc(3 * n));
  CLC_HIP(hipMemcpyAsync(br.p, ranges + offsets[0], n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(bam.p, angle_min, n_scans * sizeof(float), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(bai.p, angle_increment, n_scans * sizeof(float), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(brm.p, range_min, n_scans * sizeof(float), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(boff.p, rel.data(), (n_scans + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  const int threads = 256;
  const unsigned gx = (unsigned)std::min<long long>(64, std::max<long long>(1, (longest + threads - 1) / threads));
  hipLaunchKernelGGL(clc::scan_to_points_kernel, dim3(gx, (unsigned)n_scans), dim3(threads), 0, h->stream, br.p, boff.p,
                     (int)n_scans, bam.p, bai.p, brm.p, bp.p);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipMemcpyAsync(points + 3 * offsets[0], bp.p, 3 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
}

int clc_line_fit_batched_device(clc_handle* h, const clc_options* opt_in, const double* xy_dev, const int64_t* offsets_dev,
                                size_t n_scans, double* lines_dev, clc_summary* summaries_dev) {
  if (!h || (n_scans > 0 && (!offsets_dev || !lines_dev || !xy_dev)))
    return fail(CLC_ERR_INVALID_ARG, "clc_line_fit_batched_device: bad argument");
  clc_options opt;
  CLC_TRY(line_options(opt_in, &opt, "clc_line_fit_batched_device"));
  if (n_scans == 0) return CLC_OK;
  if (n_scans > 0x7FFFFFF0ull) return fail(CLC_ERR_INVALID_ARG, "clc_line_fit_batched_device: too many scans");
  CLC_HIP(hipSetDevice(h->device));
  launch_line_fit(h, opt, xy_dev, reinterpret_cast<const long long*>(offsets_dev), n_scans, lines_dev, summaries_dev);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
}

int clc_scan_to_points_device(clc_handle* h, const float* ranges_dev, const int64_t* offsets_dev, size_t n_scans,
                              size_t n_rays, const float* angle_min_dev, const float* angle_increment_dev,
                              const float* range_min_dev, double* points_dev) {
  if (!h || (n_scans > 0 && (!offsets_dev || !angle_min_dev || !angle_increment_dev || !range_min_dev)) ||
      (n_rays > 0 && (!ranges_dev || !points_dev || n_scans == 0)))
    return fail(CLC_ERR_INVALID_ARG, "clc_scan_to_points_device: bad argument");
  if (n_rays == 0) return CLC_OK;
  CLC_HIP(hipSetDevice(h->device));
  const int threads = 256;
  hipLaunchKernelGGL(clc::scan_to_points_flat_kernel, dim3((unsigned)((n_rays + threads - 1) / threads)), dim3(threads), 0,
                     h->stream, ranges_dev, reinterpret_cast<const long long*>(offsets_dev), (long long)n_scans,
                     (long long)n_rays, angle_min_dev, angle_increment_dev, range_min_dev, points_dev);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
}

// ---- board-segment detection (K7) -------------------------------------------------------------
namespace {
void launch_board_segments(clc_handle* h, const double* points_dev, const int64_t* offsets_dev, size_t n_scans, int64_t* seg_dev,
                          int32_t* status_dev) {
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  const unsigned blocks = (unsigned)((n_scans + clc::SEG_WAVES_PER_BLOCK - 1) / clc::SEG_WAVES_PER_BLOCK);
  hipLaunchKernelGGL(clc::board_segment_kernel, dim3(blocks), dim3(64 * clc::SEG_WAVES_PER_BLOCK), 0, h->stream, points_dev,
                     reinterpret_cast<const long long*>(offsets_dev), (long long)n_scans, reinterpret_cast<long long*>(seg_dev),
                     reinterpret_cast<int*>(status_dev));
}
}  // namespace

int clc_board_segments(clc_handle* h, const double* points, const int64_t* offsets, size_t n_scans, int64_t* seg, int32_t* status) {
  if (!h || (n_scans > 0 && (!offsets || !seg)))
    return fail(CLC_ERR_INVALID_ARG, "clc_board_segments: bad argument");
  if (n_scans == 0) return CLC_OK;
  if (n_scans > 0x1FFFFFFF0ull) return fail(CLC_ERR_INVALID_ARG, "clc_board_segments: too many scans");
  std::vector<long long> rel;
  size_t n_pts;
  CLC_TRY(host_offsets("clc_board_segments", offsets, n_scans, false, "points", &rel, &n_pts));
  if (n_pts > 0 && !points) return fail(CLC_ERR_INVALID_ARG, "clc_board_segments: bad argument");
  CLC_HIP(hipSetDevice(h->device));
  DevBuf<double> bp(&h->pool);
  DevBuf<long long> boff(&h->pool), bseg(&h->pool);
  DevBuf<int32_t> bst(&h->pool);
  CLC_HIP(bp.alloc(std::max<size_t>(1, 3 * n_pts)));
  CLC_HIP(boff.alloc(n_scans + 1));
  CLC_HIP(bseg.alloc(2 * n_scans));
  if (status) CLC_HIP(bst.alloc(n_scans));
  if (n_pts > 0) CLC_HIP(hipMemcpyAsync(bp.p, points + 3 * offsets[0], 3 * n_pts * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(boff.p, rel.data(), (n_scans + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  launch_board_segments(h, bp.p, reinterpret_cast<const int64_t*>(boff.p), n_scans, reinterpret_cast<int64_t*>(bseg.p), status ? bst.p : nullptr);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipMemcpyAsync(seg, bseg.p, 2 * n_scans * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  if (status) CLC_HIP(hipMemcpyAsync(status, bst.p, n_scans * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
}

int clc_board_segments_device(clc_handle* h, const double* points_dev, const int64_t* offsets_dev, size_t n_scans, int64_t* seg_dev,
                              int32_t* status_dev) {
  if (!h || (n_scans > 0 && (!offsets_dev || !points_dev || !seg_dev)))
    return fail(CLC_ERR_INVALID_ARG, "clc_board_segments_device: bad argument");
  if (n_scans == 0) return CLC_OK;
  if (n_scans > 0x1FFFFFFF0ull) return fail(CLC_ERR_INVALID_ARG, "clc_board_segments_device: too many scans");
  CLC_HIP(hipSetDevice(h->device));
  launch_board_segments(h, points_dev, offsets_dev, n_scans, seg_dev, status_dev);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
}

}  // extern "C"

// ---- the offline flow's observations (K13, clc_assemble.hpp) ----------------------------------------------------------------------
namespace {

#ifdef CLC_TEST_HOOKS
std::vector<double> g_last_lines;  // (m0, m1) per observation of the last assembly in this process (hooks build only)
#endif

// The one argument check of the assemble and sweep calls, host and _device forms (host forms: n_rays = 0, not known yet).
int scan_call_check(const char* who, bool handles, size_t n_poses, bool poses, size_t n_scans, bool scans, size_t n_rays, const void* ranges) {
  if (!handles || (n_poses > 0 && !poses) || (n_scans > 0 && !scans) || (n_rays > 0 && (!ranges || n_scans == 0)) ||
      n_poses > 0x7FFFFFF0ull || n_scans > 0x7FFFFFF0ull)
    return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": bad argument").c_str());
  return CLC_OK;
}

// The stamped poses and the scans of such a call in device memory: offsets from 0, ranges from the first ray.
struct ScanCall {
  const double *stamp, *q, *t, *sstamp;
  const float *ranges, *am, *ai, *rm;
  const int64_t* off;
  size_t n_rays;
};
// The host arrays of a host form: the offsets checked and rebased, then everything up into blocks of st.
int upload_scan_call(clc_handle* h, Staging& st, const char* who, size_t n_poses, const double* pose_stamp, const double* q_wc_wxyz,
                     const double* t_wc, const float* ranges, const int64_t* offsets, size_t n_scans, const float* angle_min,
                     const float* angle_increment, const float* range_min, const double* scan_stamp, ScanCall* c) {
  std::vector<long long> rel;
  CLC_TRY(host_offsets(who, offsets, n_scans, true, "rays", &rel, &c->n_rays));
  if (c->n_rays > 0 && !ranges) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": NULL ranges").c_str());
  CLC_HIP(hipSetDevice(h->device));
  c->stamp = st.in(pose_stamp, n_poses);
  c->q = st.in(q_wc_wxyz, 4 * n_poses);
  c->t = st.in(t_wc, 3 * n_poses);
  c->sstamp = st.in(scan_stamp, n_scans);
  c->ranges = st.in(c->n_rays ? ranges + offsets[0] : nullptr, c->n_rays);
  c->am = st.in(angle_min, n_scans);
  c->ai = st.in(angle_increment, n_scans);
  c->rm = st.in(range_min, n_scans);
  c->off = reinterpret_cast<const int64_t*>(st.in(rel.data(), n_scans + 1));
  return st.status(who);
}

int check_assemble_options(const char* who, const clc_assemble_options* in, clc_assemble_options* opt) {
  if (in) *opt = *in; else clc_assemble_options_default(opt);
  if (opt->line.max_num_iterations < 0 || (opt->line.use_loss && !(opt->line.loss_scale_factor > 0.0))) return fail(CLC_ERR_INVALID_ARG, who);
  if (!std::isfinite(opt->line0[0]) || !std::isfinite(opt->line0[1])) return fail(CLC_ERR_NONFINITE, who);
  return CLC_OK;
}

// The stages every assembly shares, whatever ties a scan to a pose (K13: the nearest key frame; K14: the station that holds its
// stamp).  Every array in device memory; host_scan_pose (nullable): where scan_pose is copied to on the host.  associate(cnt, status,
// scan_pose) enqueues the mode's kernels: they fill scan_pose[S] with an index into (d_q, d_t) or a CLC_SCAN_* code (status: K7's, valid
// when S > 0).  read_back() enqueues the mode's own copies to the host in front of the ONE wait.  The kernels run at sizes the host
// knows — n_scans, n_rays — and learn the number of observations from the counters on the device: workgroups and rows behind it
// leave at once, so nothing is read back before the wait at the end.  c: the counters (clc::AsmCounter).
template <class Associate, class ReadBack>
int assemble_on_device(clc_handle* h, const char* who, const double line0[2], const clc_options& line, const double* d_q, const double* d_t,
                       const float* d_ranges, const int64_t* d_off, size_t S, size_t n_rays, const float* d_am, const float* d_ai,
                       const float* d_rm, int32_t* d_scan_pose, int32_t* host_scan_pose, long long c[clc::ASM_COUNTERS], Associate&& associate,
                       ReadBack&& read_back) {
  const size_t cap_points = std::min(n_rays, S * (size_t)clc::ASM_SEG_MAX_POINTS);
  h->store_poses = -1;
  // the handle's pose-major arrays at what S scans can need at most (the number of observations is not known on the host yet)
  CLC_HIP(h->d_sq.grow(std::max<size_t>(S * 4, 1)));
  CLC_HIP(h->d_st.grow(std::max<size_t>(S * 3, 1)));
  CLC_HIP(h->d_spts.grow(std::max<size_t>(cap_points * 3, 1)));
  CLC_HIP(h->d_sptl.grow(std::max<size_t>(S * 6, 1)));
  CLC_HIP(h->d_soff.grow(3 * (S + 1)));
  DevBuf<long long> cnt(&h->pool), seg(&h->pool), obs_scan(&h->pool), fit_off(&h->pool);
  DevBuf<int> status(&h->pool), spose(&h->pool);
  DevBuf<double> points(&h->pool), xy(&h->pool), lines(&h->pool);
  CLC_HIP(cnt.alloc(clc::ASM_COUNTERS)); CLC_HIP(seg.alloc(2 * S)); CLC_HIP(obs_scan.alloc(S)); CLC_HIP(fit_off.alloc(S + 1));
  CLC_HIP(status.alloc(S));
  if (!d_scan_pose) { CLC_HIP(spose.alloc(S)); d_scan_pose = spose.p; }
  CLC_HIP(points.alloc(3 * n_rays)); CLC_HIP(xy.alloc(2 * cap_points)); CLC_HIP(lines.alloc(2 * S));
  const long long* off = reinterpret_cast<const long long*>(d_off);
  long long* soff = h->d_soff;
  CLC_HIP(hipMemsetAsync(cnt.p, 0, clc::ASM_COUNTERS * sizeof(long long), h->stream));
  const int threads = 256;
  if (S > 0) {
    if (n_rays > 0) {
      hipLaunchKernelGGL(clc::scan_to_points_flat_kernel, dim3((unsigned)((n_rays + threads - 1) / threads)), dim3(threads), 0, h->stream,
                         d_ranges, off, (long long)S, (long long)n_rays, d_am, d_ai, d_rm, points.p);
      CLC_HIP(hipGetLastError());
    }
    launch_board_segments(h, points.p, d_off, S, reinterpret_cast<int64_t*>(seg.p), status.p);
    CLC_HIP(hipGetLastError());
  }
  CLC_TRY(associate(cnt.p, status.p, d_scan_pose));
  hipLaunchKernelGGL(clc::compact_kernel, dim3(1), dim3(clc::ASM_SCAN_BLOCK), 0, h->stream, d_scan_pose, seg.p, (long long)S,
                     (long long)cap_points, obs_scan.p, fit_off.p, soff, cnt.p);
  CLC_HIP(hipGetLastError());
  if (S > 0) {
    hipLaunchKernelGGL(clc::gather_kernel, dim3((unsigned)S), dim3(256), 0, h->stream, points.p, off, seg.p, d_scan_pose, obs_scan.p, fit_off.p,
                       cnt.p, d_q, d_t, line0[0], line0[1], h->d_spts.get(), xy.p, lines.p, h->d_sq.get(), h->d_st.get());
    CLC_HIP(hipGetLastError());
    launch_line_fit(h, line, xy.p, fit_off.p, S, lines.p, nullptr);  // rows behind the observations are empty scans
    CLC_HIP(hipGetLastError());
    hipLaunchKernelGGL(clc::endpoints_kernel, dim3((unsigned)((S + threads - 1) / threads)), dim3(threads), 0, h->stream, h->d_spts.get(), soff,
                       cnt.p, lines.p, h->d_sptl.get());
    CLC_HIP(hipGetLastError());
  }
  // what comes back: the counters, the packed offsets, the tag poses a reference-size store keeps on the host
  std::vector<long long> hoff(2 * (S + 1));
  const size_t n_small = std::min<size_t>(S, 4096);
  std::vector<double> tq(4 * n_small + 1), tt(3 * n_small + 1);
  CLC_HIP(hipMemcpyAsync(c, cnt.p, clc::ASM_COUNTERS * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(hoff.data(), soff, hoff.size() * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  if (n_small > 0) {
    CLC_HIP(hipMemcpyAsync(tq.data(), h->d_sq.get(), 4 * n_small * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    CLC_HIP(hipMemcpyAsync(tt.data(), h->d_st.get(), 3 * n_small * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  if (host_scan_pose && S > 0) CLC_HIP(hipMemcpyAsync(host_scan_pose, d_scan_pose, S * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  CLC_TRY(read_back());
  CLC_HIP(hipStreamSynchronize(h->stream));
  if (c[clc::ASM_OVERFLOW] != 0) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": the segments hold more points than the scans").c_str());
  const size_t P = (size_t)c[clc::ASM_N_OBS];
#ifdef CLC_TEST_HOOKS
  g_last_lines.assign(2 * P, 0.0);  // test hook: the lines the end points were computed from (clc_debug_assemble_lines)
  if (P > 0) CLC_HIP(hipMemcpy(g_last_lines.data(), lines.p, 2 * P * sizeof(double), hipMemcpyDeviceToHost));
#endif
  h->s_pts_off.assign(hoff.begin(), hoff.begin() + (P + 1));
  h->s_ptl_off.assign(hoff.begin() + (P + 1), hoff.begin() + 2 * (P + 1));
  StoreFacts f;  // scan points have z = 0 (TranScanToPoints), the points on the line too; points_on_line is never the points
  f.tag_q = tq.data();
  f.tag_t = tt.data();
  return adopt_store(h, (int)P, f);
}

// K13: key frames, then the nearest key frame within max_dt
int assemble_keyframes_on_device(clc_handle* h, const clc_assemble_options& opt, size_t n_poses, const double* d_stamp, const double* d_q,
                                 const double* d_t, const float* d_ranges, const int64_t* d_off, size_t S, size_t n_rays, const float* d_am,
                                 const float* d_ai, const float* d_rm, const double* d_sstamp, int32_t* d_scan_pose, int32_t* host_scan_pose,
                                 clc_assemble_info* info) {
  DevBuf<unsigned char> keep(&h->pool);
  DevBuf<int> kf(&h->pool);
  CLC_HIP(keep.alloc(n_poses)); CLC_HIP(kf.alloc(n_poses));
  long long c[clc::ASM_COUNTERS];
  CLC_TRY(assemble_on_device(
      h, "clc_assemble_observations", opt.line0, opt.line, d_q, d_t, d_ranges, d_off, S, n_rays, d_am, d_ai, d_rm, d_scan_pose, host_scan_pose, c,
      [&](long long* cnt, const int* status, int32_t* scan_pose) {
        hipLaunchKernelGGL(clc::keyframe_kernel, dim3(1), dim3(64), 0, h->stream, d_q, d_t, d_stamp, (long long)n_poses, opt.keyframe_dist_min,
                           opt.keyframe_theta_min, keep.p, kf.p, cnt);
        CLC_HIP(hipGetLastError());
        if (S > 0) {
          hipLaunchKernelGGL(clc::associate_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, h->stream, status, d_sstamp, (long long)S,
                             d_stamp, kf.p, cnt, opt.max_dt, scan_pose);
          CLC_HIP(hipGetLastError());
        }
        return (int)CLC_OK;
      },
      [] { return (int)CLC_OK; }));
  if (info) {
    info->n_keyframes = c[clc::ASM_N_KEYFRAMES];
    info->n_segments = c[clc::ASM_N_SEGMENTS];
    info->n_ref_throws = c[clc::ASM_N_REF_THROWS];
    info->n_unmatched = c[clc::ASM_N_UNMATCHED];
    info->n_observations = c[clc::ASM_N_OBS];
    info->n_points = c[clc::ASM_N_POINTS];
    info->n_line_points = c[clc::ASM_N_LINE_POINTS];
  }
  return CLC_OK;
}

// ---- static stations (K14, clc_stations.hpp) ----------------------------------------------------------------------------------------
int check_station_options(const char* who, const clc_station_options* in, clc_station_options* opt) {
  if (in) *opt = *in; else clc_station_options_default(opt);
  if (!std::isfinite(opt->center_dist_max) || opt->center_dist_max < 0.0 || opt->min_members < 0) return fail(CLC_ERR_INVALID_ARG, who);
  if (opt->line.max_num_iterations < 0 || (opt->line.use_loss && !(opt->line.loss_scale_factor > 0.0))) return fail(CLC_ERR_INVALID_ARG, who);
  if (!std::isfinite(opt->line0[0]) || !std::isfinite(opt->line0[1])) return fail(CLC_ERR_NONFINITE, who);
  return CLC_OK;
}

// the stations of one call in device memory.  cap: no call can find more — a station has members > min_members, that is at least
// max(1, min_members) poses of its own
struct StationBufs {
  DevBuf<long long> cnt, first, last, members;
  DevBuf<double> q, t, start, end;
  DevBuf<int> status;
  size_t cap = 0;
  explicit StationBufs(DevPool* p) : cnt(p), first(p), last(p), members(p), q(p), t(p), start(p), end(p), status(p) {}
  hipError_t alloc(size_t n_poses, const clc_station_options& opt) {
    cap = n_poses / (size_t)std::max<int64_t>(1, opt.min_members) + 1;
    hipError_t e = cnt.alloc(clc::ST_COUNTERS);
    if (e == hipSuccess) e = first.alloc(cap);
    if (e == hipSuccess) e = last.alloc(cap);
    if (e == hipSuccess) e = members.alloc(cap);
    if (e == hipSuccess) e = q.alloc(4 * cap);
    if (e == hipSuccess) e = t.alloc(3 * cap);
    if (e == hipSuccess) e = start.alloc(cap);
    if (e == hipSuccess) e = end.alloc(cap);
    if (e == hipSuccess) e = status.alloc(cap);
    return e;
  }
};

// the walk and the averages, enqueued on the handle's stream (no wait); d_stamp nullable
int launch_stations(clc_handle* h, const clc_station_options& opt, size_t n_poses, const double* d_stamp, const double* d_q, const double* d_t,
                    StationBufs& b, bool average = true) {
  hipLaunchKernelGGL(clc::station_walk_kernel, dim3(1), dim3(64), 0, h->stream, d_t, d_stamp, (long long)n_poses, opt.center_dist_max,
                     (long long)opt.min_members, (int)(opt.close_last_run != 0), b.first.p, b.last.p, b.members.p, b.cnt.p);
  CLC_HIP(hipGetLastError());
  if (!average) return CLC_OK;
  const size_t blocks = std::min<size_t>((b.cap + clc::STATION_WAVES_PER_BLOCK - 1) / clc::STATION_WAVES_PER_BLOCK, 1024);
  hipLaunchKernelGGL(clc::station_average_kernel, dim3((unsigned)blocks), dim3(64 * clc::STATION_WAVES_PER_BLOCK), 0, h->stream, d_q, d_t, d_stamp,
                     b.first.p, b.last.p, b.members.p, b.cnt.p, b.q.p, b.t.p, b.start.p, b.end.p, b.status.p);
  CLC_HIP(hipGetLastError());
  return CLC_OK;
}

// K14: stations, then the station whose [start_time, end_time] holds the scan's stamp; the gather takes the averaged poses
int assemble_stations_on_device(clc_handle* h, const clc_station_options& opt, size_t n_poses, const double* d_stamp, const double* d_q,
                                const double* d_t, const float* d_ranges, const int64_t* d_off, size_t S, size_t n_rays, const float* d_am,
                                const float* d_ai, const float* d_rm, const double* d_sstamp, int32_t* d_scan_station,
                                int32_t* host_scan_station, clc_station_info* info) {
  StationBufs b(&h->pool);
  CLC_HIP(b.alloc(n_poses, opt));
  long long c[clc::ASM_COUNTERS], sc[clc::ST_COUNTERS];
  std::vector<int> st_status(b.cap);
  CLC_TRY(assemble_on_device(
      h, "clc_assemble_stations", opt.line0, opt.line, b.q.p, b.t.p, d_ranges, d_off, S, n_rays, d_am, d_ai, d_rm, d_scan_station,
      host_scan_station, c,
      [&](long long*, const int* status, int32_t* scan_station) {
        CLC_TRY(launch_stations(h, opt, n_poses, d_stamp, d_q, d_t, b));
        if (S > 0) {
          hipLaunchKernelGGL(clc::station_associate_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, h->stream, status, d_sstamp,
                             (long long)S, b.start.p, b.end.p, b.status.p, b.cnt.p, scan_station);
          CLC_HIP(hipGetLastError());
        }
        return (int)CLC_OK;
      },
      [&] {
        CLC_HIP(hipMemcpyAsync(sc, b.cnt.p, sizeof(sc), hipMemcpyDeviceToHost, h->stream));
        CLC_HIP(hipMemcpyAsync(st_status.data(), b.status.p, b.cap * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        return (int)CLC_OK;
      }));
  if (info) {
    info->n_runs = sc[clc::ST_N_RUNS];
    info->n_stations = sc[clc::ST_N_STATIONS];
    info->n_nonfinite = 0;
    for (long long k = 0; k < sc[clc::ST_N_STATIONS]; ++k) info->n_nonfinite += st_status[(size_t)k] == clc::STATION_NONFINITE ? 1 : 0;
    info->n_segments = c[clc::ASM_N_SEGMENTS];
    info->n_ref_throws = c[clc::ASM_N_REF_THROWS];
    info->n_unmatched = c[clc::ASM_N_UNMATCHED];
    info->n_observations = c[clc::ASM_N_OBS];
    info->n_points = c[clc::ASM_N_POINTS];
    info->n_line_points = c[clc::ASM_N_LINE_POINTS];
  }
  return CLC_OK;
}

// ---- interpolated tag poses (K15, clc_interp.hpp) -----------------------------------------------------------------------------------
int check_interp_options(const char* who, const clc_interp_options* in, clc_interp_options* opt) {
  if (in) *opt = *in; else clc_interp_options_default(opt);
  if (!std::isfinite(opt->max_gap) || !(opt->max_gap > 0.0) || !std::isfinite(opt->time_offset)) return fail(CLC_ERR_INVALID_ARG, who);
  if (opt->line.max_num_iterations < 0 || (opt->line.use_loss && !(opt->line.loss_scale_factor > 0.0))) return fail(CLC_ERR_INVALID_ARG, who);
  if (!std::isfinite(opt->line0[0]) || !std::isfinite(opt->line0[1])) return fail(CLC_ERR_NONFINITE, who);
  return CLC_OK;
}

// the look at the pose list and the interpolation at m query stamps, enqueued on the handle's stream (no wait); cnt: ASM_COUNTERS
int launch_interp(clc_handle* h, const clc_interp_options& opt, size_t n_poses, const double* d_stamp, const double* d_q, const double* d_t,
                  const int* d_status, const double* d_query, size_t m, long long* cnt, int32_t* d_bracket, double* d_u, double* d_qo, double* d_to,
                  int32_t* d_self) {
  hipLaunchKernelGGL(clc::interp_stamps_kernel, dim3(1), dim3(64), 0, h->stream, d_stamp, (long long)n_poses, opt.max_gap, cnt);
  CLC_HIP(hipGetLastError());
  if (m > 0) {
    hipLaunchKernelGGL(clc::interp_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, d_status, d_query, (long long)m, d_stamp,
                       d_q, d_t, (long long)n_poses, cnt, opt.time_offset, opt.max_gap, d_bracket, d_u, d_qo, d_to, d_self);
    CLC_HIP(hipGetLastError());
  }
  return CLC_OK;
}

// K15: every scan with a segment takes the pose interpolated at its stamp; the gather reads the per-scan poses (scan_pose[s] = s)
int assemble_interpolated_on_device(clc_handle* h, const clc_interp_options& opt, size_t n_poses, const double* d_stamp, const double* d_q,
                                    const double* d_t, const float* d_ranges, const int64_t* d_off, size_t S, size_t n_rays, const float* d_am,
                                    const float* d_ai, const float* d_rm, const double* d_sstamp, int32_t* d_bracket, double* d_u,
                                    int32_t* host_bracket, double* host_u, clc_assemble_info* info) {
  DevBuf<double> sq(&h->pool), st(&h->pool), su(&h->pool);
  DevBuf<int> sbr(&h->pool);
  CLC_HIP(sq.alloc(4 * S)); CLC_HIP(st.alloc(3 * S));
  if (!d_bracket && host_bracket) { CLC_HIP(sbr.alloc(S)); d_bracket = sbr.p; }
  if (!d_u && host_u) { CLC_HIP(su.alloc(S)); d_u = su.p; }
  long long c[clc::ASM_COUNTERS];
  CLC_TRY(assemble_on_device(
      h, "clc_assemble_interpolated", opt.line0, opt.line, sq.p, st.p, d_ranges, d_off, S, n_rays, d_am, d_ai, d_rm, nullptr, nullptr, c,
      [&](long long* cnt, const int* status, int32_t* scan_pose) {
        return launch_interp(h, opt, n_poses, d_stamp, d_q, d_t, status, d_sstamp, S, cnt, d_bracket, d_u, sq.p, st.p, scan_pose);
      },
      [&] {
        if (host_bracket && S > 0) CLC_HIP(hipMemcpyAsync(host_bracket, d_bracket, S * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        if (host_u && S > 0) CLC_HIP(hipMemcpyAsync(host_u, d_u, S * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        return (int)CLC_OK;
      }));
  if (info) {
    info->n_keyframes = c[clc::ASM_N_KEYFRAMES];
    info->n_segments = c[clc::ASM_N_SEGMENTS];
    info->n_ref_throws = c[clc::ASM_N_REF_THROWS];
    info->n_unmatched = c[clc::ASM_N_UNMATCHED];
    info->n_observations = c[clc::ASM_N_OBS];
    info->n_points = c[clc::ASM_N_POINTS];
    info->n_line_points = c[clc::ASM_N_LINE_POINTS];
  }
  return CLC_OK;
}

// ---- the clock sweep (K15) ------------------------------------------------------------------------------------------------------------
#ifdef CLC_TEST_HOOKS
std::vector<double> g_last_sweep_records;  // the records of the last sweep in this process, problem-major (hooks build only)
#endif

int check_sweep_options(const char* who, const clc_clock_offset_options* in, clc_clock_offset_options* opt) {
  if (in) *opt = *in; else clc_clock_offset_options_default(opt);
  if (opt->n_offsets < 3 || opt->n_offsets > 1024 || !std::isfinite(opt->offset_min) || !std::isfinite(opt->offset_max) ||
      !(opt->offset_max > opt->offset_min) || opt->points_per_scan < 0 || !std::isfinite(opt->interp.max_gap) || !(opt->interp.max_gap > 0.0))
    return fail(CLC_ERR_INVALID_ARG, who);
  return CLC_OK;
}

int sweep_on_device(clc_handle* h, const clc_clock_offset_options& opt, size_t n_poses, const double* d_stamp, const double* d_q, const double* d_t,
                    const float* d_ranges, const int64_t* d_off, size_t S, size_t n_rays, const float* d_am, const float* d_ai, const float* d_rm,
                    const double* d_sstamp, const double pose7[7], double* offsets_out, double* final_cost, double* poses, clc_summary* summaries,
                    clc_clock_offset_result* result) {
  const size_t J = (size_t)opt.n_offsets;
  std::vector<double> cand(J);
  for (size_t j = 0; j < J; ++j) cand[j] = opt.offset_min + (double)j * (opt.offset_max - opt.offset_min) / (double)(J - 1);
  if (offsets_out) std::memcpy(offsets_out, cand.data(), J * sizeof(double));
  result->n_scans_used = 0;
  result->records_per_problem = 0;
  result->best_index = -1;
  result->at_edge = 0;
  result->best_offset = std::nan("");
  if (S == 0) return CLC_OK;
  DevBuf<long long> cnt(&h->pool), sw(&h->pool), seg(&h->pool), take(&h->pool), used_scan(&h->pool), rec_off(&h->pool);
  DevBuf<int> status(&h->pool);
  DevBuf<double> points(&h->pool), dcand(&h->pool), rec(&h->pool);
  CLC_HIP(cnt.alloc(clc::ASM_COUNTERS)); CLC_HIP(sw.alloc(clc::SW_COUNTERS)); CLC_HIP(seg.alloc(2 * S)); CLC_HIP(take.alloc(S));
  CLC_HIP(used_scan.alloc(S)); CLC_HIP(rec_off.alloc(S + 1)); CLC_HIP(status.alloc(S)); CLC_HIP(points.alloc(3 * n_rays)); CLC_HIP(dcand.alloc(J));
  const long long* off = reinterpret_cast<const long long*>(d_off);
  const int threads = 256;
  CLC_HIP(hipMemcpyAsync(dcand.p, cand.data(), J * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (n_rays > 0) {
    hipLaunchKernelGGL(clc::scan_to_points_flat_kernel, dim3((unsigned)((n_rays + threads - 1) / threads)), dim3(threads), 0, h->stream, d_ranges,
                       off, (long long)S, (long long)n_rays, d_am, d_ai, d_rm, points.p);
    CLC_HIP(hipGetLastError());
  }
  launch_board_segments(h, points.p, d_off, S, reinterpret_cast<int64_t*>(seg.p), status.p);
  CLC_HIP(hipGetLastError());
  hipLaunchKernelGGL(clc::interp_stamps_kernel, dim3(1), dim3(64), 0, h->stream, d_stamp, (long long)n_poses, opt.interp.max_gap, cnt.p);
  CLC_HIP(hipGetLastError());
  hipLaunchKernelGGL(clc::sweep_member_kernel, dim3((unsigned)((S + threads - 1) / threads)), dim3(threads), 0, h->stream, status.p, seg.p, d_sstamp,
                     (long long)S, d_stamp, d_q, d_t, (long long)n_poses, cnt.p, dcand.p, (int)J, opt.interp.max_gap, (long long)opt.points_per_scan,
                     take.p);
  CLC_HIP(hipGetLastError());
  hipLaunchKernelGGL(clc::sweep_offsets_kernel, dim3(1), dim3(clc::SWEEP_SCAN_BLOCK), 0, h->stream, take.p, (long long)S, used_scan.p, rec_off.p, sw.p);
  CLC_HIP(hipGetLastError());
  long long c[clc::SW_COUNTERS];
  CLC_HIP(hipMemcpyAsync(c, sw.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));  // the one read-back: the sizes of the batch
  const size_t U = (size_t)c[clc::SW_N_USED], R = (size_t)c[clc::SW_N_RECORDS];
  result->n_scans_used = (int64_t)U;
  result->records_per_problem = (int64_t)R;
  if (U == 0) return CLC_OK;
  CLC_HIP(rec.alloc(J * R * 8));
  hipLaunchKernelGGL(clc::sweep_records_kernel, dim3((unsigned)U, (unsigned)J), dim3(128), 0, h->stream, points.p, off, seg.p, d_sstamp, used_scan.p,
                     rec_off.p, sw.p, d_stamp, d_q, d_t, (long long)n_poses, cnt.p, dcand.p, opt.interp.max_gap, (long long)opt.points_per_scan, rec.p);
  CLC_HIP(hipGetLastError());
#ifdef CLC_TEST_HOOKS
  g_last_sweep_records.assign(J * R * 8, 0.0);  // test hook: clc_debug_sweep_records
  CLC_HIP(hipStreamSynchronize(h->stream));
  CLC_HIP(hipMemcpy(g_last_sweep_records.data(), rec.p, J * R * 8 * sizeof(double), hipMemcpyDeviceToHost));
#endif
  std::vector<int64_t> poff(J + 1);
  for (size_t j = 0; j <= J; ++j) poff[j] = (int64_t)(j * R);
  CLC_TRY(clc_upload_batched_device(h, reinterpret_cast<const clc_observation*>(rec.p), poff.data(), J));
  std::vector<double> p7(7 * J);
  std::vector<clc_summary> sm(J);
  for (size_t j = 0; j < J; ++j) std::memcpy(&p7[7 * j], pose7, 7 * sizeof(double));
  CLC_TRY(clc_solve_batched(h, &opt.solve, p7.data(), sm.data()));
  std::vector<double> cost(J);
  std::vector<int32_t> term(J);
  for (size_t j = 0; j < J; ++j) { cost[j] = sm[j].final_cost; term[j] = sm[j].termination; }
  if (final_cost) std::memcpy(final_cost, cost.data(), J * sizeof(double));
  if (poses) std::memcpy(poses, p7.data(), 7 * J * sizeof(double));
  if (summaries) std::memcpy(summaries, sm.data(), J * sizeof(clc_summary));
  return clc_clock_offset_best(J, cand.data(), cost.data(), term.data(), &result->best_index, &result->best_offset, &result->at_edge);
}

}  // namespace

extern "C" {

void clc_assemble_options_default(clc_assemble_options* o) {
  if (!o) return;
  o->keyframe_dist_min = 0.20;                     // main/calibr_offline.cpp:66
  o->keyframe_theta_min = 3.1415926 * 10 / 180.;   // :67
  o->max_dt = 0.02;                                // :116
  o->line0[0] = o->line0[1] = 0.0;
  clc_line_options_default(&o->line);
}

int clc_keyframes(clc_handle* h, const clc_assemble_options* opt_in, size_t n_poses, const double* q_wc_wxyz, const double* t_wc,
                  uint8_t* keep, int64_t* n_kept) {
  if (!h || (n_poses > 0 && (!q_wc_wxyz || !t_wc)) || n_poses > 0x7FFFFFF0ull) return fail(CLC_ERR_INVALID_ARG, "clc_keyframes: bad argument");
  clc_assemble_options opt;
  CLC_TRY(check_assemble_options("clc_keyframes: bad options", opt_in, &opt));
  CLC_HIP(hipSetDevice(h->device));
  DevBuf<double> bq(&h->pool), bt(&h->pool);
  DevBuf<unsigned char> bkeep(&h->pool);
  DevBuf<int> bkf(&h->pool);
  DevBuf<long long> bcnt(&h->pool);
  CLC_HIP(bq.alloc(4 * n_poses)); CLC_HIP(bt.alloc(3 * n_poses)); CLC_HIP(bkeep.alloc(n_poses)); CLC_HIP(bkf.alloc(n_poses));
  CLC_HIP(bcnt.alloc(clc::ASM_COUNTERS));
  if (n_poses > 0) {
    CLC_HIP(hipMemcpyAsync(bq.p, q_wc_wxyz, 4 * n_poses * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bt.p, t_wc, 3 * n_poses * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  hipLaunchKernelGGL(clc::keyframe_kernel, dim3(1), dim3(64), 0, h->stream, bq.p, bt.p, (const double*)nullptr, (long long)n_poses,
                     opt.keyframe_dist_min, opt.keyframe_theta_min, bkeep.p, bkf.p, bcnt.p);
  CLC_HIP(hipGetLastError());
  long long c[2] = {0, 0};
  CLC_HIP(hipMemcpyAsync(c, bcnt.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  if (keep && n_poses > 0) CLC_HIP(hipMemcpyAsync(keep, bkeep.p, n_poses, hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  if (n_kept) *n_kept = c[clc::ASM_N_KEYFRAMES];
  return CLC_OK;
}

int clc_assemble_observations_device(clc_handle* h, const clc_assemble_options* opt_in, size_t n_poses, const double* pose_stamp_dev,
                                     const double* q_wc_wxyz_dev, const double* t_wc_dev, const float* ranges_dev,
                                     const int64_t* offsets_dev, size_t n_scans, size_t n_rays, const float* angle_min_dev,
                                     const float* angle_increment_dev, const float* range_min_dev, const double* scan_stamp_dev,
                                     int32_t* scan_pose_dev, clc_assemble_info* info) {
  CLC_TRY(scan_call_check("clc_assemble_observations_device", h != nullptr, n_poses, pose_stamp_dev && q_wc_wxyz_dev && t_wc_dev, n_scans,
                          offsets_dev && angle_min_dev && angle_increment_dev && range_min_dev && scan_stamp_dev, n_rays, ranges_dev));
  clc_assemble_options opt;
  CLC_TRY(check_assemble_options("clc_assemble_observations_device: bad options", opt_in, &opt));
  CLC_HIP(hipSetDevice(h->device));
  return assemble_keyframes_on_device(h, opt, n_poses, pose_stamp_dev, q_wc_wxyz_dev, t_wc_dev, ranges_dev, offsets_dev, n_scans, n_rays, angle_min_dev,
                            angle_increment_dev, range_min_dev, scan_stamp_dev, scan_pose_dev, nullptr, info);
}

int clc_assemble_observations(clc_handle* h, const clc_assemble_options* opt_in, size_t n_poses, const double* pose_stamp,
                              const double* q_wc_wxyz, const double* t_wc, const float* ranges, const int64_t* offsets, size_t n_scans,
                              const float* angle_min, const float* angle_increment, const float* range_min, const double* scan_stamp,
                              int32_t* scan_pose, clc_assemble_info* info) {
  const char* who = "clc_assemble_observations";
  CLC_TRY(scan_call_check(who, h != nullptr, n_poses, pose_stamp && q_wc_wxyz && t_wc, n_scans,
                          offsets && angle_min && angle_increment && range_min && scan_stamp, 0, nullptr));
  clc_assemble_options opt;
  CLC_TRY(check_assemble_options("clc_assemble_observations: bad options", opt_in, &opt));
  Staging st(h);
  ScanCall c;
  CLC_TRY(upload_scan_call(h, st, who, n_poses, pose_stamp, q_wc_wxyz, t_wc, ranges, offsets, n_scans, angle_min, angle_increment, range_min,
                           scan_stamp, &c));
  return assemble_keyframes_on_device(h, opt, n_poses, c.stamp, c.q, c.t, c.ranges, c.off, n_scans, c.n_rays, c.am, c.ai, c.rm, c.sstamp, nullptr,
                                      scan_pose, info);
}

int clc_stored_observations(clc_handle* h, int* n_poses, double* tag_q_wxyz, double* tag_t, int64_t* pts_off, double* pts,
                            int64_t* ptl_off, double* ptl) {
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_stored_observations: NULL handle");
  if (h->store_poses < 0) return fail(CLC_ERR_NO_DATA, "clc_stored_observations: no scans stored");
  const size_t P = (size_t)h->store_poses;
  if (n_poses) *n_poses = h->store_poses;
  const size_t M = (size_t)h->s_pts_off[P], ML = (size_t)h->s_ptl_off[P];
  if (pts_off) for (size_t i = 0; i <= P; ++i) pts_off[i] = h->s_pts_off[i];
  if (ptl_off) for (size_t i = 0; i <= P; ++i) ptl_off[i] = h->s_ptl_off[i];
  CLC_HIP(hipSetDevice(h->device));
  auto down = [&](void* dst, const double* src, size_t count) {
    return (!dst || count == 0) ? hipSuccess : hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyDeviceToHost, h->stream);
  };
  CLC_HIP(down(tag_q_wxyz, h->d_sq.get(), 4 * P));
  CLC_HIP(down(tag_t, h->d_st.get(), 3 * P));
  CLC_HIP(down(pts, h->d_spts.get(), 3 * M));
  CLC_HIP(down(ptl, h->d_sptl.get(), 3 * ML));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
}

// ---- static stations (K14) ----------------------------------------------------------------------------------------------------------
void clc_station_options_default(clc_station_options* o) {
  if (!o) return;
  o->center_dist_max = 0.002;  // src/utilities.cpp:108
  o->min_members = 30;         // :119: staticPose.size() > 30, the first pose counted twice
  o->close_last_run = 0;       // :114-123: a run is pushed at a break only
  o->reserved = 0;
  o->line0[0] = o->line0[1] = 0.0;
  clc_line_options_default(&o->line);
}

int clc_static_poses(clc_handle* h, const clc_station_options* opt_in, size_t n_poses, const double* pose_stamp, const double* q_wc_wxyz,
                     const double* t_wc, size_t cap_stations, int64_t* first, int64_t* last, double* start_time, double* end_time,
                     double* q_avg_wxyz, double* t_avg, int32_t* status, int64_t* n_stations) {
  if (!h || (n_poses > 0 && (!q_wc_wxyz || !t_wc)) || n_poses > 0x7FFFFFF0ull) return fail(CLC_ERR_INVALID_ARG, "clc_static_poses: bad argument");
  clc_station_options opt;
  CLC_TRY(check_station_options("clc_static_poses: bad options", opt_in, &opt));
  CLC_HIP(hipSetDevice(h->device));
  DevBuf<double> bstamp(&h->pool), bq(&h->pool), bt(&h->pool);
  StationBufs b(&h->pool);
  CLC_HIP(bq.alloc(4 * n_poses)); CLC_HIP(bt.alloc(3 * n_poses));
  if (pose_stamp) CLC_HIP(bstamp.alloc(n_poses));
  CLC_HIP(b.alloc(n_poses, opt));
  if (n_poses > 0) {
    CLC_HIP(hipMemcpyAsync(bq.p, q_wc_wxyz, 4 * n_poses * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(bt.p, t_wc, 3 * n_poses * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (pose_stamp) CLC_HIP(hipMemcpyAsync(bstamp.p, pose_stamp, n_poses * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  CLC_TRY(launch_stations(h, opt, n_poses, pose_stamp ? bstamp.p : nullptr, bq.p, bt.p, b));
  long long sc[clc::ST_COUNTERS];
  CLC_HIP(hipMemcpyAsync(sc, b.cnt.p, sizeof(sc), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  if (n_stations) *n_stations = sc[clc::ST_N_STATIONS];
  const size_t rows = std::min<size_t>((size_t)sc[clc::ST_N_STATIONS], cap_stations);  // (the count never exceeds b.cap)
  static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "station row types");
  auto down = [&](void* dst, const void* src, size_t bytes) {
    return (!dst || bytes == 0) ? hipSuccess : hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream);
  };
  CLC_HIP(down(first, b.first.p, rows * sizeof(int64_t)));
  CLC_HIP(down(last, b.last.p, rows * sizeof(int64_t)));
  CLC_HIP(down(start_time, b.start.p, rows * sizeof(double)));
  CLC_HIP(down(end_time, b.end.p, rows * sizeof(double)));
  CLC_HIP(down(q_avg_wxyz, b.q.p, 4 * rows * sizeof(double)));
  CLC_HIP(down(t_avg, b.t.p, 3 * rows * sizeof(double)));
  CLC_HIP(down(status, b.status.p, rows * sizeof(int32_t)));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
}

int clc_assemble_stations_device(clc_handle* h, const clc_station_options* opt_in, size_t n_poses, const double* pose_stamp_dev,
                                 const double* q_wc_wxyz_dev, const double* t_wc_dev, const float* ranges_dev, const int64_t* offsets_dev,
                                 size_t n_scans, size_t n_rays, const float* angle_min_dev, const float* angle_increment_dev,
                                 const float* range_min_dev, const double* scan_stamp_dev, int32_t* scan_station_dev, clc_station_info* info) {
  CLC_TRY(scan_call_check("clc_assemble_stations_device", h != nullptr, n_poses, pose_stamp_dev && q_wc_wxyz_dev && t_wc_dev, n_scans,
                          offsets_dev && angle_min_dev && angle_increment_dev && range_min_dev && scan_stamp_dev, n_rays, ranges_dev));
  clc_station_options opt;
  CLC_TRY(check_station_options("clc_assemble_stations_device: bad options", opt_in, &opt));
  CLC_HIP(hipSetDevice(h->device));
  return assemble_stations_on_device(h, opt, n_poses, pose_stamp_dev, q_wc_wxyz_dev, t_wc_dev, ranges_dev, offsets_dev, n_scans, n_rays,
                                     angle_min_dev, angle_increment_dev, range_min_dev, scan_stamp_dev, scan_station_dev, nullptr, info);
}

int clc_assemble_stations(clc_handle* h, const clc_station_options* opt_in, size_t n_poses, const double* pose_stamp, const double* q_wc_wxyz,
                          const double* t_wc, const float* ranges, const int64_t* offsets, size_t n_scans, const float* angle_min,
                          const float* angle_increment, const float* range_min, const double* scan_stamp, int32_t* scan_station,
                          clc_station_info* info) {
  const char* who = "clc_assemble_stations";
  CLC_TRY(scan_call_check(who, h != nullptr, n_poses, pose_stamp && q_wc_wxyz && t_wc, n_scans,
                          offsets && angle_min && angle_increment && range_min && scan_stamp, 0, nullptr));
  clc_station_options opt;
  CLC_TRY(check_station_options("clc_assemble_stations: bad options", opt_in, &opt));
  Staging st(h);
  ScanCall c;
  CLC_TRY(upload_scan_call(h, st, who, n_poses, pose_stamp, q_wc_wxyz, t_wc, ranges, offsets, n_scans, angle_min, angle_increment, range_min,
                           scan_stamp, &c));
  return assemble_stations_on_device(h, opt, n_poses, c.stamp, c.q, c.t, c.ranges, c.off, n_scans, c.n_rays, c.am, c.ai, c.rm, c.sstamp, nullptr,
                                     scan_station, info);
}

// ---- interpolated tag poses (K15) ---------------------------------------------------------------------------------------------------
void clc_interp_options_default(clc_interp_options* o) {
  if (!o) return;
  o->time_offset = 0.0;
  o->max_gap = 0.1;
  o->line0[0] = o->line0[1] = 0.0;
  clc_line_options_default(&o->line);
}

int clc_interpolate_poses(clc_handle* h, const clc_interp_options* opt_in, size_t n_poses, const double* pose_stamp, const double* q_wc_wxyz,
                          const double* t_wc, size_t n_queries, const double* query_stamp, int32_t* bracket, double* u, double* q_out_wxyz,
                          double* t_out) {
  if (!h || (n_poses > 0 && (!pose_stamp || !q_wc_wxyz || !t_wc)) || (n_queries > 0 && !query_stamp) || n_poses > 0x7FFFFFF0ull ||
      n_queries > 0x7FFFFFF0ull)
    return fail(CLC_ERR_INVALID_ARG, "clc_interpolate_poses: bad argument");
  clc_interp_options opt;
  CLC_TRY(check_interp_options("clc_interpolate_poses: bad options", opt_in, &opt));
  CLC_HIP(hipSetDevice(h->device));
  const size_t m = n_queries;
  DevBuf<double> bstamp(&h->pool), bq(&h->pool), bt(&h->pool), bx(&h->pool), bu(&h->pool), bqo(&h->pool), bto(&h->pool);
  DevBuf<int> bbr(&h->pool);
  DevBuf<long long> bcnt(&h->pool);
  CLC_HIP(bstamp.alloc(n_poses)); CLC_HIP(bq.alloc(4 * n_poses)); CLC_HIP(bt.alloc(3 * n_poses)); CLC_HIP(bx.alloc(m));
  CLC_HIP(bu.alloc(m)); CLC_HIP(bqo.alloc(4 * m)); CLC_HIP(bto.alloc(3 * m)); CLC_HIP(bbr.alloc(m)); CLC_HIP(bcnt.alloc(clc::ASM_COUNTERS));
  auto up = [&](void* dst, const void* src, size_t bytes) {
    return bytes == 0 ? hipSuccess : hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream);
  };
  CLC_HIP(up(bstamp.p, pose_stamp, n_poses * sizeof(double)));
  CLC_HIP(up(bq.p, q_wc_wxyz, 4 * n_poses * sizeof(double)));
  CLC_HIP(up(bt.p, t_wc, 3 * n_poses * sizeof(double)));
  CLC_HIP(up(bx.p, query_stamp, m * sizeof(double)));
  CLC_TRY(launch_interp(h, opt, n_poses, bstamp.p, bq.p, bt.p, nullptr, bx.p, m, bcnt.p, bbr.p, bu.p, bqo.p, bto.p, nullptr));
  auto down = [&](void* dst, const void* src, size_t bytes) {
    return (!dst || bytes == 0) ? hipSuccess : hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream);
  };
  CLC_HIP(down(bracket, bbr.p, m * sizeof(int32_t)));
  CLC_HIP(down(u, bu.p, m * sizeof(double)));
  CLC_HIP(down(q_out_wxyz, bqo.p, 4 * m * sizeof(double)));
  CLC_HIP(down(t_out, bto.p, 3 * m * sizeof(double)));
  CLC_HIP(hipStreamSynchronize(h->stream));
  return CLC_OK;
}

int clc_assemble_interpolated_device(clc_handle* h, const clc_interp_options* opt_in, size_t n_poses, const double* pose_stamp_dev,
                                     const double* q_wc_wxyz_dev, const double* t_wc_dev, const float* ranges_dev, const int64_t* offsets_dev,
                                     size_t n_scans, size_t n_rays, const float* angle_min_dev, const float* angle_increment_dev,
                                     const float* range_min_dev, const double* scan_stamp_dev, int32_t* scan_bracket_dev, double* scan_u_dev,
                                     clc_assemble_info* info) {
  CLC_TRY(scan_call_check("clc_assemble_interpolated_device", h != nullptr, n_poses, pose_stamp_dev && q_wc_wxyz_dev && t_wc_dev, n_scans,
                          offsets_dev && angle_min_dev && angle_increment_dev && range_min_dev && scan_stamp_dev, n_rays, ranges_dev));
  clc_interp_options opt;
  CLC_TRY(check_interp_options("clc_assemble_interpolated_device: bad options", opt_in, &opt));
  CLC_HIP(hipSetDevice(h->device));
  return assemble_interpolated_on_device(h, opt, n_poses, pose_stamp_dev, q_wc_wxyz_dev, t_wc_dev, ranges_dev, offsets_dev, n_scans, n_rays,
                                         angle_min_dev, angle_increment_dev, range_min_dev, scan_stamp_dev, scan_bracket_dev, scan_u_dev, nullptr,
                                         nullptr, info);
}

int clc_assemble_interpolated(clc_handle* h, const clc_interp_options* opt_in, size_t n_poses, const double* pose_stamp, const double* q_wc_wxyz,
                              const double* t_wc, const float* ranges, const int64_t* offsets, size_t n_scans, const float* angle_min,
                              const float* angle_increment, const float* range_min, const double* scan_stamp, int32_t* scan_bracket,
                              double* scan_u, clc_assemble_info* info) {
  const char* who = "clc_assemble_interpolated";
  CLC_TRY(scan_call_check(who, h != nullptr, n_poses, pose_stamp && q_wc_wxyz && t_wc, n_scans,
                          offsets && angle_min && angle_increment && range_min && scan_stamp, 0, nullptr));
  clc_interp_options opt;
  CLC_TRY(check_interp_options("clc_assemble_interpolated: bad options", opt_in, &opt));
  Staging st(h);
  ScanCall c;
  CLC_TRY(upload_scan_call(h, st, who, n_poses, pose_stamp, q_wc_wxyz, t_wc, ranges, offsets, n_scans, angle_min, angle_increment, range_min,
                           scan_stamp, &c));
  return assemble_interpolated_on_device(h, opt, n_poses, c.stamp, c.q, c.t, c.ranges, c.off, n_scans, c.n_rays, c.am, c.ai, c.rm, c.sstamp,
                                         nullptr, nullptr, scan_bracket, scan_u, info);
}

// ---- the clock sweep (K15) ------------------------------------------------------------------------------------------------------------
void clc_clock_offset_options_default(clc_clock_offset_options* o) {
  if (!o) return;
  o->offset_min = -0.02;
  o->offset_max = 0.02;
  o->n_offsets = 41;
  o->points_per_scan = 16;
  clc_interp_options_default(&o->interp);
  clc_options_default(&o->solve);
}

int clc_clock_offset_best(size_t n_offsets, const double* offsets, const double* final_cost, const int32_t* termination, int32_t* best_index,
                         double* best_offset, int32_t* at_edge) {
  if ((n_offsets > 0 && (!offsets || !final_cost)) || !best_index || !best_offset || !at_edge || n_offsets > 0x7FFFFFF0ull)
    return fail(CLC_ERR_INVALID_ARG, "clc_clock_offset_best: bad argument");
  auto usable = [&](size_t j) { return !(termination && termination[j] == CLC_FAILURE) && final_cost[j] == final_cost[j]; };
  long long b = -1;
  for (size_t j = 0; j < n_offsets; ++j)
    if (usable(j) && (b < 0 || final_cost[j] < final_cost[(size_t)b])) b = (long long)j;
  *best_index = (int32_t)b;
  *at_edge = 0;
  *best_offset = b < 0 ? std::nan("") : offsets[(size_t)b];
  if (b < 0) return CLC_OK;
  if (b == 0 || (size_t)b + 1 == n_offsets) { *at_edge = 1; return CLC_OK; }
  const size_t k = (size_t)b;
  if (!usable(k - 1) || !usable(k + 1)) return CLC_OK;
  // the vertex of the parabola through (x0, y0), (x1, y1), (x2, y2): x1 - 1/2 (a^2 (y1 - y2) - c^2 (y1 - y0)) / (a (y1 - y2) - c (y1 - y0))
  const double a = offsets[k] - offsets[k - 1], c = offsets[k] - offsets[k + 1];
  const double f0 = final_cost[k] - final_cost[k - 1], f2 = final_cost[k] - final_cost[k + 1];  // both <= 0 at a minimum
  const double den = a * f2 - c * f0;
  const double v = offsets[k] - 0.5 * (a * a * f2 - c * c * f0) / den;
  const double lo = std::min(offsets[k - 1], offsets[k + 1]), hi = std::max(offsets[k - 1], offsets[k + 1]);
  if (f0 < 0.0 && f2 < 0.0 && std::isfinite(v) && v >= lo && v <= hi) *best_offset = v;
  return CLC_OK;
}

int clc_clock_offset_sweep_device(clc_handle* h, const clc_clock_offset_options* opt_in, size_t n_poses, const double* pose_stamp_dev,
                                 const double* q_wc_wxyz_dev, const double* t_wc_dev, const float* ranges_dev, const int64_t* offsets_dev,
                                 size_t n_scans, size_t n_rays, const float* angle_min_dev, const float* angle_increment_dev,
                                 const float* range_min_dev, const double* scan_stamp_dev, const double pose7[7], double* offsets_out,
                                 double* final_cost, double* poses, clc_summary* summaries, clc_clock_offset_result* result) {
  CLC_TRY(scan_call_check("clc_clock_offset_sweep_device", h && pose7 && result, n_poses, pose_stamp_dev && q_wc_wxyz_dev && t_wc_dev, n_scans,
                          offsets_dev && angle_min_dev && angle_increment_dev && range_min_dev && scan_stamp_dev, n_rays, ranges_dev));
  clc_clock_offset_options opt;
  CLC_TRY(check_sweep_options("clc_clock_offset_sweep_device: bad options", opt_in, &opt));
  CLC_HIP(hipSetDevice(h->device));
  return sweep_on_device(h, opt, n_poses, pose_stamp_dev, q_wc_wxyz_dev, t_wc_dev, ranges_dev, offsets_dev, n_scans, n_rays, angle_min_dev,
                         angle_increment_dev, range_min_dev, scan_stamp_dev, pose7, offsets_out, final_cost, poses, summaries, result);
}

int clc_clock_offset_sweep(clc_handle* h, const clc_clock_offset_options* opt_in, size_t n_poses, const double* pose_stamp, const double* q_wc_wxyz,
                          const double* t_wc, const float* ranges, const int64_t* offsets, size_t n_scans, const float* angle_min,
                          const float* angle_increment, const float* range_min, const double* scan_stamp, const double pose7[7],
                          double* offsets_out, double* final_cost, double* poses, clc_summary* summaries, clc_clock_offset_result* result) {
  const char* who = "clc_clock_offset_sweep";
  CLC_TRY(scan_call_check(who, h && pose7 && result, n_poses, pose_stamp && q_wc_wxyz && t_wc, n_scans,
                          offsets && angle_min && angle_increment && range_min && scan_stamp, 0, nullptr));
  clc_clock_offset_options opt;
  CLC_TRY(check_sweep_options("clc_clock_offset_sweep: bad options", opt_in, &opt));
  Staging st(h);
  ScanCall c;
  CLC_TRY(upload_scan_call(h, st, who, n_poses, pose_stamp, q_wc_wxyz, t_wc, ranges, offsets, n_scans, angle_min, angle_increment, range_min,
                           scan_stamp, &c));
  return sweep_on_device(h, opt, n_poses, c.stamp, c.q, c.t, c.ranges, c.off, n_scans, c.n_rays, c.am, c.ai, c.rm, c.sstamp, pose7, offsets_out,
                         final_cost, poses, summaries, result);
}

}  // extern "C"

#ifdef CLC_TEST_HOOKS
#pragma GCC visibility push(default)
// test hook: the fitted lines (m0, m1 per observation) of the last clc_assemble_observations[_device] of this process
extern "C" int clc_debug_assemble_lines(double* lines_out, int64_t cap_lines, int64_t* n_lines) {
  if (!n_lines) return fail(CLC_ERR_INVALID_ARG, "clc_debug_assemble_lines: bad argument");
  *n_lines = (int64_t)(g_last_lines.size() / 2);
  if (lines_out) {
    if (cap_lines < *n_lines) return fail(CLC_ERR_INVALID_ARG, "clc_debug_assemble_lines: buffer too small");
    std::memcpy(lines_out, g_last_lines.data(), g_last_lines.size() * sizeof(double));
  }
  return CLC_OK;
}
// test hook: the walk of clc_static_poses alone on host translations -> the stations' first / last / members (at most cap rows each,
// nullable), *n_stations, *n_runs (every closed run)
extern "C" int clc_debug_station_walk(clc_handle* h, const clc_station_options* opt_in, size_t n_poses, const double* t_wc, int64_t cap,
                                      int64_t* first, int64_t* last, int64_t* members, int64_t* n_stations, int64_t* n_runs) {
  if (!h || (n_poses > 0 && !t_wc) || cap < 0) return fail(CLC_ERR_INVALID_ARG, "clc_debug_station_walk: bad argument");
  clc_station_options opt;
  CLC_TRY(check_station_options("clc_debug_station_walk: bad options", opt_in, &opt));
  CLC_HIP(hipSetDevice(h->device));
  DevBuf<double> bt(&h->pool);
  StationBufs b(&h->pool);
  CLC_HIP(bt.alloc(3 * n_poses));
  CLC_HIP(b.alloc(n_poses, opt));
  if (n_poses > 0) CLC_HIP(hipMemcpyAsync(bt.p, t_wc, 3 * n_poses * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CLC_TRY(launch_stations(h, opt, n_poses, nullptr, nullptr, bt.p, b, /*average=*/false));
  long long sc[clc::ST_COUNTERS];
  CLC_HIP(hipMemcpyAsync(sc, b.cnt.p, sizeof(sc), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  if (n_stations) *n_stations = sc[clc::ST_N_STATIONS];
  if (n_runs) *n_runs = sc[clc::ST_N_RUNS];
  const size_t rows = std::min<size_t>((size_t)sc[clc::ST_N_STATIONS], (size_t)cap);
  if (rows > 0) {
    if (first) CLC_HIP(hipMemcpy(first, b.first.p, rows * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (last) CLC_HIP(hipMemcpy(last, b.last.p, rows * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (members) CLC_HIP(hipMemcpy(members, b.members.p, rows * sizeof(int64_t), hipMemcpyDeviceToHost));
  }
  return CLC_OK;
}
// test hook: the records (8 doubles each, problem-major) the last clc_clock_offset_sweep[_device] of this process uploaded
extern "C" int clc_debug_sweep_records(double* records_out, int64_t cap_doubles, int64_t* n_doubles) {
  if (!n_doubles) return fail(CLC_ERR_INVALID_ARG, "clc_debug_sweep_records: bad argument");
  *n_doubles = (int64_t)g_last_sweep_records.size();
  if (records_out) {
    if (cap_doubles < *n_doubles) return fail(CLC_ERR_INVALID_ARG, "clc_debug_sweep_records: buffer too small");
    std::memcpy(records_out, g_last_sweep_records.data(), g_last_sweep_records.size() * sizeof(double));
  }
  return CLC_OK;
}
#pragma GCC visibility pop
#endif  // CLC_TEST_HOOKS
