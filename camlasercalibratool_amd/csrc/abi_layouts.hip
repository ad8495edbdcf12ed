// abi_layouts.hip — the upload paths: staged records -> 64-byte tiles, scan structure, compact / row / lane layouts; stored scans.
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "clc_abi_internal.hpp"
#include "abi_assemble.hpp"

using namespace clc_abi;

namespace {

int retile_into(clc_handle* h, const double* d_aos, size_t n, StreamLayout& L) {
  const size_t n_padded = ((n + clc::TILE - 1) / clc::TILE) * clc::TILE;
  CLC_HIP(L.d_tiles.grow(std::max<size_t>(n_padded, clc::TILE) * 8));
  if (n_padded > 0) {
    const int threads = 256;
    const long long blocks = ((long long)n_padded + threads - 1) / threads;
    hipLaunchKernelGGL(clc::retile_kernel, dim3((unsigned)blocks), dim3(threads), 0, h->stream, d_aos,
                       L.d_tiles, (long long)n, (long long)n_padded);
    CLC_HIP(hipGetLastError());
  }
  return CLC_OK;
}

// Upload-time re-encoding of staged AoS records, entirely on the device (O(1) host work, a few words copied back):
//   * scans = runs of records with bit-identical (n, d, scale) (and never across two problems): flags, prefix sum ->
//     scan index per record, scan starts;
//   * compact layout (clc_kernels.hpp "Compact layout"): group table + 28-byte tiles, bitwise lossless;
//   * row layout (clc_rows.hpp): every scan padded to whole rows of 64 points, (x, y) rows + one descriptor per row —
//     only when every record has p.z == 0 and the padding at most doubles the array.
// Nothing is kept when the records do not group at least 4:1 (hand-made arrays without scan structure).
template <class TIn>
int device_scan(clc_handle* h, const TIn* d_in, long long n, unsigned int minus_one, unsigned int* d_out,
                unsigned long long* d_totals /* [blocks + 1] */) {
  const long long blocks = (n + clc::SCAN_CHUNK - 1) / clc::SCAN_CHUNK;
  hipLaunchKernelGGL((clc::scan_block_totals_kernel<TIn>), dim3((unsigned)blocks), dim3(clc::SCAN_THREADS), 0, h->stream,
                     d_in, n, d_totals);
  hipLaunchKernelGGL(clc::scan_totals_kernel, dim3(1), dim3(clc::SCAN_THREADS), 0, h->stream, d_totals, blocks);
  hipLaunchKernelGGL((clc::scan_apply_kernel<TIn>), dim3((unsigned)blocks), dim3(clc::SCAN_THREADS), 0, h->stream, d_in, n,
                     d_totals, minus_one, d_out);
  CLC_HIP(hipGetLastError());
  return CLC_OK;
}

// The lane layout of the batched problems (clc_resident.hpp) from the staged records and their scan structure: plan
// (points per lane of every problem, on the device), offsets (O(P) on the host), lane descriptors + j-major point rows.
// Leaves L.ok false — and the streaming layouts in charge — when some problem does not fit a workgroup.
int build_resident(clc_handle* h, ResLayout& L, int first_try, const double* d_aos, long long n, size_t P, size_t G,
                   const long long* d_rec_off, const unsigned int* d_gid, const long long* d_starts, int max_ppl_override = 0,
                   bool with_z = false) {
  L.ok = false;
  L.with_z = false;
  L.lanes = 0;
  L.max_ppl = 0;
  L.rows = 0;
  if (!plan_upload(h->steer, h->auto_disable, false).resident) return CLC_OK;
  const int threads = 256;
  DevBuf<unsigned int> bppl(&h->pool), bfail(&h->pool);
  CLC_HIP(bppl.alloc(P));
  CLC_HIP(bfail.alloc(1));
  std::vector<unsigned int> ppl(P);
  int lanes = 0;
  for (int nl = first_try; nl <= (max_ppl_override > 0 ? first_try : 512) && lanes == 0; nl *= 2) {
    unsigned int failed = 0;
    CLC_HIP(hipMemsetAsync(bfail.p, 0, sizeof(unsigned int), h->stream));
    hipLaunchKernelGGL(clc::res_plan_kernel, dim3((unsigned)((P + threads - 1) / threads)), dim3(threads), 0, h->stream, d_rec_off,
                       d_gid, d_starts, (long long)P, n, (long long)G, nl, max_ppl_override > 0 ? max_ppl_override : (nl == 256 ? kResPR256 + kResPL256 : kResPR512 + kResPL512), bppl.p, bfail.p);
    CLC_HIP(hipGetLastError());
    CLC_HIP(hipMemcpyAsync(&failed, bfail.p, sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
    CLC_HIP(hipMemcpyAsync(ppl.data(), bppl.p, sizeof(unsigned int) * P, hipMemcpyDeviceToHost, h->stream));
    CLC_HIP(hipStreamSynchronize(h->stream));
    if (!failed) lanes = nl;
  }
  if (lanes == 0) return CLC_OK;  // some problem is too long (or has too many scans) for one workgroup
  std::vector<unsigned int> row(P + 1, 0u);
  unsigned long long total = 0;
  unsigned int max_ppl = 0;
  bool uniform = true;
  for (size_t k = 0; k < P; ++k) {
    row[k] = (unsigned int)total;
    total += ppl[k];
    max_ppl = std::max(max_ppl, ppl[k]);
    uniform = uniform && ppl[k] == ppl[0];
  }
  if (total >= 0xFFFFFFF0ull) return CLC_OK;
  row[P] = (unsigned int)total;
  CLC_HIP(L.d_row.grow(P + 1));
  CLC_HIP(L.d_desc.grow(P * (size_t)lanes));
  // one padding row: the kernel's loads run unconditionally from clamped row indices (an empty last problem reads it)
  CLC_HIP(L.d_xy.grow(((size_t)total + 1) * (size_t)lanes * 2));
  CLC_HIP(hipMemcpyAsync(L.d_row, row.data(), (P + 1) * sizeof(unsigned int), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemsetAsync(L.d_xy + (size_t)total * (size_t)lanes * 2, 0, (size_t)lanes * 2 * sizeof(double), h->stream));
  if (with_z) {
    CLC_HIP(L.d_z.grow(((size_t)total + 1) * (size_t)lanes));
    CLC_HIP(hipMemsetAsync(L.d_z + (size_t)total * (size_t)lanes, 0, (size_t)lanes * sizeof(double), h->stream));
  }
  double* d_zl = with_z ? L.d_z : nullptr;
  if (lanes == 256)
    hipLaunchKernelGGL((clc::res_build_kernel<256>), dim3((unsigned)P), dim3(256), 0, h->stream, d_aos, d_rec_off, d_gid, d_starts, n,
                       (long long)G, L.d_row, L.d_desc, L.d_xy, d_zl);
  else
    hipLaunchKernelGGL((clc::res_build_kernel<512>), dim3((unsigned)P), dim3(512), 0, h->stream, d_aos, d_rec_off, d_gid, d_starts, n,
                       (long long)G, L.d_row, L.d_desc, L.d_xy, d_zl);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipStreamSynchronize(h->stream));  // `row` is a host temporary
  L.lanes = lanes;
  L.max_ppl = (int)max_ppl;
  L.uni_ppl = uniform && P > 0 ? (int)ppl[0] : -1;
  L.rows = (long long)total;
  L.with_z = with_z;
  L.ok = true;
  return CLC_OK;
}

// The scan structure of an observation array: what the layout builds are enqueued from.  Planned on the device (build_layouts:
// scan flags, prefix sums, read-backs) or, for a single problem one workgroup holds, on the host (plan_small_on_host: no read-back).
struct LayoutPlan {
  size_t P = 0, G = 0;    // problems, scans
  long long n = 0;        // records
  size_t tiles = 0;       // 64-record tiles of all problems ...
  long long max_tiles = 0;  // ... and of the longest one
  bool sparse = false;    // fewer than 4 records per scan on average: the streaming layouts do not pay (the step chain keeps the
                          // 64-byte tiles) — the on-chip layouts, where a lane carries its own plane anyway, are still built
  bool any_z = false;     // some record has p.z != 0
  long long R = 0;        // rows of the row layout
  bool rows_ok = false;
  const long long* d_rec_off = nullptr;       // [P + 1]
  const long long* d_tile_off = nullptr;      // [P + 1]
  const long long* d_starts = nullptr;        // [G + 1] first record of every scan
  const unsigned int* d_gid = nullptr;        // [n] scan of every record
  const unsigned int* d_row_begin = nullptr;  // [G + 1] first row of every scan
  int ppl = 0;                                // host plan: points per lane of the 512-lane layout (0: build_resident plans it) ...
  const unsigned int* d_res_row = nullptr;    // ... and its row offsets {0, ppl}
  void set_scans(size_t g) { G = g; sparse = G * 4 > (size_t)n; }
  void set_rows(long long r) { R = r; rows_ok = !sparse && R > 0 && (size_t)R * clc::ROW <= 3 * (size_t)n + 64 * P; }  // a third full
  void publish(StreamLayout& L) const {
    L.n_groups = (long long)G; L.compact_ok = !sparse; L.n_rows = R; L.rows_ok = rows_ok; L.rows_z = any_z;
  }
};

// The builds of a plan, first part: the compact layout — group table (what the on-chip kernels take a lane's plane from) + 28-byte tiles.
int emit_compact(clc_handle* h, const double* d_aos, const LayoutPlan& p, StreamLayout& L) {
  const int threads = 256;
  CLC_HIP(L.d_ctiles.grow(std::max<size_t>(p.tiles, 1) * clc::CTILE_DOUBLES));
  CLC_HIP(L.d_groups.grow(p.G * clc::GROUP_DOUBLES));
  hipLaunchKernelGGL(clc::build_groups_dev_kernel, dim3((unsigned)((p.G + threads - 1) / threads)), dim3(threads), 0, h->stream, d_aos,
                     p.d_starts, (long long)p.G, L.d_groups);
  const long long max_padded = p.max_tiles * clc::TILE;
  const unsigned ydim = (unsigned)std::min<long long>(4096, std::max<long long>(1, (max_padded + threads - 1) / threads));
  hipLaunchKernelGGL(clc::build_ctiles_kernel, dim3((unsigned)p.P, ydim), dim3(threads), 0, h->stream, d_aos, p.d_gid, p.d_rec_off,
                     p.d_tile_off, L.d_ctiles);
  CLC_HIP(hipGetLastError());
  return CLC_OK;
}

// ... second part: the row layout, the batch's first row of every problem (d_prob_row), the lane layouts res / coop.
int emit_rows_and_lanes(clc_handle* h, const double* d_aos, const LayoutPlan& p, StreamLayout& L, long long* d_prob_row, ResLayout* res,
                        ResLayout* coop) {
  const int threads = 256;
  const long long n = p.n, R = p.R;
  int rc = CLC_OK;
  if (p.rows_ok) {
    // one padding row each: the streaming loop's prologue loads run unconditionally from clamped row indices; + the wave split table
    const size_t row_doubles = p.any_z ? clc::ROW_DOUBLES_Z : clc::ROW_DOUBLES;
    CLC_HIP(L.d_rxy.grow(((size_t)R + 1) * row_doubles));
    CLC_HIP(L.rdesc_bytes.grow(((size_t)R + 1) * sizeof(clc::RowDesc) + clc::wave_split_bytes(R)));
    CLC_HIP(hipMemsetAsync(L.d_rxy + (size_t)R * row_doubles, 0, row_doubles * sizeof(double), h->stream));
    CLC_HIP(hipMemsetAsync(L.d_rdesc() + R, 0, sizeof(clc::RowDesc), h->stream));
    const long long slots = R * clc::ROW;
    hipLaunchKernelGGL(clc::build_rows_kernel, dim3((unsigned)((slots + threads - 1) / threads)), dim3(threads), 0, h->stream, d_aos,
                       p.d_starts, p.d_row_begin, (long long)p.G, R, (int)row_doubles, L.d_rxy, L.d_rdesc());
    if (d_prob_row)
      hipLaunchKernelGGL(clc::problem_rows_kernel, dim3((unsigned)((p.P + 1 + threads - 1) / threads)), dim3(threads), 0, h->stream,
                         p.d_rec_off, p.d_gid, p.d_row_begin, (long long)p.P, n, R, d_prob_row);
    CLC_HIP(hipGetLastError());
  }
  if (res != nullptr && p.ppl > 0) {  // planned on the host: one problem's 512-lane layout (build_resident with first_try = 512)
    CLC_HIP(res->d_row.grow(2));
    CLC_HIP(res->d_desc.grow(512));
    CLC_HIP(res->d_xy.grow(((size_t)p.ppl + 1) * 512 * 2));
    CLC_HIP(hipMemcpyAsync(res->d_row, p.d_res_row, 2 * sizeof(unsigned int), hipMemcpyDeviceToDevice, h->stream));
    CLC_HIP(hipMemsetAsync(res->d_xy + (size_t)p.ppl * 512 * 2, 0, (size_t)512 * 2 * sizeof(double), h->stream));
    hipLaunchKernelGGL((clc::res_build_kernel<512>), dim3(1), dim3(512), 0, h->stream, d_aos, p.d_rec_off, p.d_gid, p.d_starts, n,
                       (long long)p.G, p.d_res_row, res->d_desc, res->d_xy, (double*)nullptr);
    CLC_HIP(hipGetLastError());
    res->lanes = 512; res->max_ppl = p.ppl; res->uni_ppl = p.ppl; res->rows = p.ppl; res->with_z = false; res->ok = true;
  } else if (res != nullptr) {
    res->ok = false;
    if (!p.any_z) {
      rc = build_resident(h, *res, plan_upload(h->steer, h->auto_disable, d_prob_row != nullptr).first_lanes, d_aos, n, p.P, p.G, p.d_rec_off, p.d_gid, p.d_starts);
      if (rc != CLC_OK) return rc;
    } else if (d_prob_row != nullptr) {
      // a BATCH whose points carry z: the 512-lane form with 24-byte slots (one problem per CU; resident_solve_kernel<.., WITH_Z>) — the
      // batch is still read from HBM once per solve.  (A single problem with z: the cooperative kernel's z form, below.)
      rc = build_resident(h, *res, 512, d_aos, n, p.P, p.G, p.d_rec_off, p.d_gid, p.d_starts, kResPRz + kResPLz, /*with_z=*/true);
      if (rc != CLC_OK) return rc;
    }
  }
  if (coop != nullptr) {
    coop->ok = false;
    // (records with p.z != 0: the cooperative kernel's WITH_Z form holds 24-byte slots)
    // (clc_set_small_on_coop: the cooperative layout also for a problem one workgroup holds — clc_solve then prefers it)
    if (p.P == 1 && n > 0 && h->num_cus >= clc::COOP_WGS && (h->small_on_coop || !(res != nullptr && res->ok))) {
      // the one problem in chunks of equal record counts, one per workgroup (a chunk may begin and end inside a scan: res_scan_extent):
      // COOP_WGS of them, or COOP_SMALL_WGS where that leaves a lane at most kCoopSmallMaxPpl points (the one-hop form of the kernel)
      const int cap_ppl = p.any_z ? clc::COOP_PR_Z + clc::COOP_PL_Z : clc::COOP_PR + clc::COOP_PL;
      // Up to this many points per lane of 32 workgroups the one-hop form runs (a host-side choice between two launch forms of the same
      // kernel).  Round 5 sweep (scripts/r05_small_form.py, us per pass, 32 / 256 workgroups): 1e5 observations 5.00 / 5.61, 1.3e5
      // 5.61 / 5.54, 1.6e5 5.55 / 5.51, 2e5 5.94 / 5.53 — a lane's extra points cost 0.065 us each, the second hop ~1 us: 13 points
      // per lane (106 496 observations) is where the one-hop form stops paying (round 4: 10).
      constexpr int kCoopSmallMaxPpl = 13;
      int small_cap = kCoopSmallMaxPpl;
#ifdef CLC_TEST_HOOKS
      if (const char* e = std::getenv("CLC_COOP_SMALL_MAX_PPL")) small_cap = std::max(1, std::atoi(e));  // (tuning hook, hooks build only: scripts/r05_small_form.py)
#endif
      const int small_ppl = std::min(small_cap, cap_ppl);
      const bool small_ok = n <= (long long)clc::COOP_SMALL_WGS * clc::COOP_NL * small_ppl && plan_upload(h->steer, h->auto_disable, false).one_hop;
      for (int attempt = small_ok ? 0 : 1; attempt < 2 && !coop->ok; ++attempt) {
        const int wgs = attempt == 0 ? clc::COOP_SMALL_WGS : clc::COOP_WGS;
        std::vector<long long> chunk((size_t)wgs + 1);
        for (int c = 0; c <= wgs; ++c) chunk[c] = (long long)((__int128)n * c / wgs);
        DevBuf<long long> bchunk(&h->pool);
        CLC_HIP(bchunk.alloc(chunk.size()));
        CLC_HIP(hipMemcpyAsync(bchunk.p, chunk.data(), chunk.size() * sizeof(long long), hipMemcpyHostToDevice, h->stream));
        CLC_HIP(hipStreamSynchronize(h->stream));
        rc = build_resident(h, *coop, clc::COOP_NL, d_aos, n, (size_t)wgs, p.G, bchunk.p, p.d_gid, p.d_starts,
                            attempt == 0 ? small_ppl : cap_ppl, p.any_z);
        if (rc != CLC_OK) return rc;
        coop->wgs = wgs;
      }  // (the small form's layout did not fit — scans that leave half-filled lanes: the 256-workgroup form is tried next)
    }
  }
  return CLC_OK;
}

}  // namespace

namespace clc_abi {

void warm_layouts() {
  warm_kernel(reinterpret_cast<const void*>(&clc::retile_kernel));
  warm_kernel(reinterpret_cast<const void*>(&clc::scan_flag_kernel));
  warm_kernel(reinterpret_cast<const void*>(&clc::build_rows_kernel));
  warm_kernel(reinterpret_cast<const void*>(&clc::res_plan_kernel));
  warm_kernel(reinterpret_cast<const void*>(&clc::res_build_kernel<512>));
  warm_kernel(reinterpret_cast<const void*>(&clc::flatten_kernel));
}

// The device pipeline: the plan on the device, the builds enqueued from it.  (The row plan is made after the compact layout is enqueued:
// its read-back then waits for the compact build too.)
int build_layouts(clc_handle* h, const double* d_aos, size_t n_total, const std::vector<long long>& rec_off,
                  const std::vector<long long>& tile_off, StreamLayout& L, long long* d_prob_row, ResLayout* res, ResLayout* coop) {
  L.invalidate();
  L.n_groups = L.n_rows = 0;
  const size_t P = rec_off.size() - 1;
  if (n_total == 0 || P == 0) return CLC_OK;
  if (n_total >= 0xFFFFFFF0ull) return CLC_OK;  // scan indices are 32-bit; such arrays keep the 64-byte tiles
  LayoutPlan p;
  p.P = P; p.n = (long long)n_total; p.tiles = (size_t)tile_off[P];
  for (size_t k = 0; k < P; ++k) p.max_tiles = std::max(p.max_tiles, tile_off[k + 1] - tile_off[k]);
  const long long n = p.n;
  const int threads = 256;
  const long long scan_blocks = (n + clc::SCAN_CHUNK - 1) / clc::SCAN_CHUNK;
  DevBuf<unsigned char> bflag(&h->pool);
  DevBuf<unsigned int> bgid(&h->pool), bzflag(&h->pool);
  DevBuf<unsigned long long> btotals(&h->pool);
  DevBuf<long long> broff(&h->pool), btoff(&h->pool);
  CLC_HIP(bflag.alloc(n_total));
  CLC_HIP(bgid.alloc(n_total));
  CLC_HIP(bzflag.alloc(1));
  CLC_HIP(btotals.alloc((size_t)scan_blocks + 1));
  CLC_HIP(broff.alloc(P + 1));
  CLC_HIP(btoff.alloc(P + 1));
  CLC_HIP(hipMemcpyAsync(broff.p, rec_off.data(), (P + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemcpyAsync(btoff.p, tile_off.data(), (P + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemsetAsync(bzflag.p, 0, sizeof(unsigned int), h->stream));
  hipLaunchKernelGGL(clc::scan_flag_kernel, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, h->stream, d_aos,
                     n, bflag.p, bzflag.p);
  hipLaunchKernelGGL(clc::mark_problem_starts_kernel, dim3((unsigned)((P + threads - 1) / threads)), dim3(threads), 0,
                     h->stream, broff.p, (long long)P, n, bflag.p);
  CLC_HIP(hipGetLastError());
  int rc = device_scan<unsigned char>(h, bflag.p, n, 1u, bgid.p, btotals.p);
  if (rc != CLC_OK) return rc;
  unsigned int last_gid = 0, any_z = 0;
  CLC_HIP(hipMemcpyAsync(&last_gid, bgid.p + (n - 1), sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(&any_z, bzflag.p, sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  p.set_scans((size_t)last_gid + 1);
  p.any_z = any_z != 0;
  if (p.sparse && res == nullptr && coop == nullptr) return CLC_OK;
  const size_t G = p.G;
  DevBuf<long long> bstarts(&h->pool);
  CLC_HIP(bstarts.alloc(G + 1));
  hipLaunchKernelGGL(clc::scan_starts_kernel, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, h->stream,
                     bflag.p, bgid.p, n, (long long)G, bstarts.p);
  CLC_HIP(hipGetLastError());
  p.d_rec_off = broff.p; p.d_tile_off = btoff.p; p.d_starts = bstarts.p; p.d_gid = bgid.p;
  rc = emit_compact(h, d_aos, p, L);
  if (rc != CLC_OK) return rc;
  // rows per scan (scan_rows_kernel) -> first row of every scan
  DevBuf<unsigned int> brows(&h->pool), brbeg(&h->pool);
  DevBuf<unsigned long long> btot2(&h->pool);
  const long long gblocks = ((long long)G + clc::SCAN_CHUNK - 1) / clc::SCAN_CHUNK;
  CLC_HIP(brows.alloc(G));
  CLC_HIP(brbeg.alloc(G + 1));
  CLC_HIP(btot2.alloc((size_t)gblocks + 1));
  hipLaunchKernelGGL(clc::scan_rows_kernel, dim3((unsigned)((G + threads - 1) / threads)), dim3(threads), 0, h->stream,
                     bstarts.p, (long long)G, brows.p);
  CLC_HIP(hipMemsetAsync(brbeg.p, 0, sizeof(unsigned int), h->stream));
  rc = device_scan<unsigned int>(h, brows.p, (long long)G, 0u, brbeg.p + 1, btot2.p);
  if (rc != CLC_OK) return rc;
  unsigned int total_rows = 0;
  CLC_HIP(hipMemcpyAsync(&total_rows, brbeg.p + G, sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  p.set_rows((long long)total_rows);
  p.d_row_begin = brbeg.p;
  rc = emit_rows_and_lanes(h, d_aos, p, L, d_prob_row, res, coop);
  if (rc != CLC_OK) return rc;
  CLC_HIP(hipStreamSynchronize(h->stream));  // the temporaries above are freed on return
  p.publish(L);
  return CLC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Small single problems — the reference's own sizes (main/calibr_simulation.cpp: 50 poses x ~114 points; main/calibr_offline.cpp:
// O(10^2) poses): at most 512 x 22 records, p.z == 0, so that ONE workgroup holds the problem.  The device pipeline above reads the
// scan structure back twice and waits on host temporaries: ~0.2 ms of waiting for ~20 us of kernels.  Here the HOST knows the scans —
// from the stored scans (clc_select_observations) or from the records themselves (clc_upload) — and plans the layouts, with the
// arithmetic of scan_rows_kernel / res_plan_kernel; ONE copy of the tables and the same builds follow, without a read-back or a
// synchronisation (tests/test_gpu_edge_cases.py::test_small_problems_planned_on_the_host_...).
struct SmallFlatten {  // clc_select_observations: the records are built on the device first (flatten_kernel)
  int n_poses;
  bool linefit, boundary;
  const std::vector<long long>* rec_off;  // [n_poses + 1]
};

constexpr size_t kSmallMaxRecords = (size_t)512 * (kResPR512 + kResPL512);

static size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

// The single problem's layouts are being replaced: forget the current ones (and the selection they were built from).
void forget_layouts(clc_handle* h) {
  h->obs.invalidate(); h->sres.ok = h->cres.ok = false; h->split_grid = -1; h->selection_key = -1;
}

// The pinned staging block of the small-problem path (+ its device twin), at least `bytes` long and free to be written.
int ensure_stage(clc_handle* h, size_t bytes) {
  if (bytes > std::min(h->h_stage.size(), h->d_stage.size())) {
    CLC_HIP(hipStreamSynchronize(h->stream));
    h->stage_busy = false;
    const size_t cap = std::max<size_t>(bytes + bytes / 2, (size_t)256 << 10);
    CLC_HIP(h->h_stage.grow(cap));
    CLC_HIP(h->d_stage.grow(cap));
  }
  if (!h->ev_stage) CLC_HIP(hipEventCreateWithFlags(h->ev_stage.out(), hipEventDisableTiming));
  if (h->stage_busy) CLC_HIP(hipEventSynchronize(h->ev_stage));  // the previous copy out of the pinned block (long done in practice)
  return CLC_OK;
}

// The host planner: rows per scan, points per lane of the 512-lane layout, and the tables staged and copied to the device —
// [flatten's record offsets][rec_off, tile_off of the one problem][starts][gid][row_begin][res_row][records].  *used = false: not a
// case for this path (nothing was enqueued).  Otherwise the handle's layouts are forgotten and the copy is enqueued; *d_records /
// *d_foff: the staged records / flatten offsets.
int plan_small_on_host(clc_handle* h, const std::vector<long long>& starts, long long n, bool any_z, const clc_observation* host_records,
                       const SmallFlatten* fj, LayoutPlan* p, const double** d_records, const long long** d_foff, bool* used) {
  *used = false;
  const size_t G = starts.size() - 1;
  if (!h->fast_small || n <= 0 || (size_t)n > kSmallMaxRecords || any_z || h->small_on_coop || G == 0 || G > 512) return CLC_OK;
  if (!plan_upload(h->steer, h->auto_disable, false).resident) return CLC_OK;
  p->P = 1; p->n = n; p->tiles = (size_t)((n + clc::TILE - 1) / clc::TILE); p->max_tiles = (long long)p->tiles;
  p->set_scans(G);
  std::vector<unsigned int> brbeg(G + 1, 0u);
  for (size_t g = 0; g < G; ++g) brbeg[g + 1] = brbeg[g] + (unsigned int)((starts[g + 1] - starts[g] + clc::ROW - 1) / clc::ROW);
  p->set_rows((long long)brbeg[G]);
  for (long long c = std::max<long long>(1, (n + 511) / 512); c <= kResPR512 + kResPL512 && p->ppl == 0; ++c) {
    long long lanes = 0;
    for (size_t g = 0; g < G && lanes <= 512; ++g) lanes += (starts[g + 1] - starts[g] + c - 1) / c;
    if (lanes <= 512) p->ppl = (int)c;
  }
  if (p->ppl == 0) return CLC_OK;  // scans that leave too many half-filled lanes: the generic path (cooperative layout)
  const size_t P1 = fj ? (size_t)fj->n_poses + 1 : 0;
  const size_t o_foff = 0, o_off = align8(o_foff + P1 * 8), o_starts = o_off + 4 * 8, o_gid = o_starts + (G + 1) * 8,
               o_brbeg = align8(o_gid + (size_t)n * 4), o_row = align8(o_brbeg + (G + 1) * 4), o_rec = align8(o_row + 8),
               total = o_rec + (host_records ? (size_t)n * sizeof(clc_observation) : 0);
  CLC_HIP(hipSetDevice(h->device));
  int rc = ensure_stage(h, total);
  if (rc != CLC_OK) return rc;
  char* b = h->h_stage;
  if (fj) std::memcpy(b + o_foff, fj->rec_off->data(), P1 * 8);
  long long* off = reinterpret_cast<long long*>(b + o_off);
  off[0] = 0; off[1] = n; off[2] = 0; off[3] = (long long)p->tiles;
  std::memcpy(b + o_starts, starts.data(), (G + 1) * 8);
  unsigned int* gid = reinterpret_cast<unsigned int*>(b + o_gid);
  for (size_t g = 0; g < G; ++g)
    for (long long k = starts[g]; k < starts[g + 1]; ++k) gid[k] = (unsigned int)g;
  std::memcpy(b + o_brbeg, brbeg.data(), (G + 1) * 4);
  unsigned int* row = reinterpret_cast<unsigned int*>(b + o_row);
  row[0] = 0u; row[1] = (unsigned int)p->ppl;
  if (host_records) std::memcpy(b + o_rec, host_records, (size_t)n * sizeof(clc_observation));
  // from here on things are enqueued: an error leaves the handle without observations rather than with half of them
  forget_layouts(h);
  h->n_obs = 0;
  CLC_HIP(hipMemcpyAsync(h->d_stage, h->h_stage, total, hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipEventRecord(h->ev_stage, h->stream));
  h->stage_busy = true;
  const char* d = h->d_stage;
  p->d_rec_off = reinterpret_cast<const long long*>(d + o_off);
  p->d_tile_off = p->d_rec_off + 2;
  p->d_starts = reinterpret_cast<const long long*>(d + o_starts);
  p->d_gid = reinterpret_cast<const unsigned int*>(d + o_gid);
  p->d_row_begin = reinterpret_cast<const unsigned int*>(d + o_brbeg);
  p->d_res_row = reinterpret_cast<const unsigned int*>(d + o_row);
  *d_records = reinterpret_cast<const double*>(d + o_rec);
  *d_foff = reinterpret_cast<const long long*>(d + o_foff);
  *used = true;
  return CLC_OK;
}

// *used = false: not a case for this path (nothing was enqueued) — the caller runs the device pipeline.
int small_fast_upload(clc_handle* h, const std::vector<long long>& starts, long long n, bool any_z, const clc_observation* host_records,
                      const SmallFlatten* fj, bool* used) {
  LayoutPlan p;
  const double* d_aos = nullptr;
  const long long* d_foff = nullptr;
  int rc = plan_small_on_host(h, starts, n, any_z, host_records, fj, &p, &d_aos, &d_foff, used);
  if (rc != CLC_OK || !*used) return rc;
  if (fj) {  // the selection's records, built on the device from the resident scans (bitwise clc_flatten_observations')
    CLC_HIP(h->d_small_aos.grow((size_t)n * (sizeof(clc_observation) / sizeof(double))));
    hipLaunchKernelGGL(clc::flatten_kernel, dim3((unsigned)fj->n_poses), dim3(clc::BLOCK), 0, h->stream, fj->n_poses, h->d_sq, h->d_st, h->d_soff,
                       h->d_spts, h->d_soff + (fj->n_poses + 1), h->d_sptl, fj->linefit ? 1 : 0, fj->boundary ? 1 : 0, d_foff, h->d_small_aos);
    CLC_HIP(hipGetLastError());
    d_aos = h->d_small_aos;
  }
  rc = retile_into(h, d_aos, (size_t)n, h->obs);
  if (rc == CLC_OK) rc = emit_compact(h, d_aos, p, h->obs);
  if (rc == CLC_OK) rc = emit_rows_and_lanes(h, d_aos, p, h->obs, nullptr, &h->sres, nullptr);
  if (rc != CLC_OK) return rc;
  p.publish(h->obs);
  h->n_obs = (size_t)n;
  ++h->fast_small_uploads;
  return CLC_OK;
}

// The scan structure of a selection of the stored scans, on the host: record k starts a scan when its (n, d, scale) differ bitwise from
// record k - 1's (scan_flag_kernel's rule) — the records of one pose share the tag plane and the scale, its two board-edge records
// carry the edge planes.  false: not known on the host (stored scans too large: clc_store_observations keeps no host copy).
bool plan_selection_scans(const clc_handle* h, bool linefit, bool boundary, const std::vector<long long>& rec_off, std::vector<long long>* starts,
                          bool* any_z) {
  if (!h->store_small) return false;
  const int P = h->store_poses;
  const std::vector<long long>& off = linefit ? h->s_ptl_off : h->s_pts_off;
  starts->clear();
  unsigned long long prev[5] = {0, 0, 0, 0, 0};
  bool have = false;
  auto record = [&](long long k, const double* n3, double d, double scale) {
    unsigned long long key[5];
    std::memcpy(key, n3, 24); std::memcpy(key + 3, &d, 8); std::memcpy(key + 4, &scale, 8);
    if (!have || std::memcmp(key, prev, sizeof(key)) != 0) starts->push_back(k);
    std::memcpy(prev, key, sizeof(key));
    have = true;
  };
  for (int i = 0; i < P; ++i) {
    const long long cnt = off[(size_t)i + 1] - off[(size_t)i];
    const bool edges = boundary && linefit;
    if (cnt <= 0 && !edges) continue;
    clc::host::PosePlanes pp;
    clc::host::pose_planes(h->s_tag_q.data(), h->s_tag_t.data(), i, edges, pp);
    const double scale = 1.0 / std::sqrt((double)cnt);  // :239-240
    long long k = rec_off[(size_t)i];
    if (cnt > 0) record(k, pp.n, pp.d, scale);
    k += cnt;
    if (edges) {
      record(k, pp.pi1, pp.pi1[3], scale);
      record(k + 1, pp.pi2, pp.pi2[3], scale);
    }
  }
  starts->push_back(rec_off[(size_t)P]);
  *any_z = (linefit ? h->s_any_z_ptl : h->s_any_z_pts) || (boundary && linefit && h->s_any_z_ends);
  return true;
}

// ... and of an array of records on the host (clc_upload).
void plan_record_scans(const clc_observation* rec, long long n, std::vector<long long>* starts, bool* any_z) {
  starts->clear();
  bool z = false;
  for (long long k = 0; k < n; ++k) {
    const clc_observation& a = rec[k];
    bool nw = k == 0;
    if (!nw) {
      const clc_observation& b = rec[k - 1];
      nw = std::memcmp(a.n, b.n, 32) != 0 || std::memcmp(&a.scale, &b.scale, 8) != 0;  // n[3], d are contiguous: 32 bytes
    }
    if (nw) starts->push_back(k);
    z = z || a.p[2] != 0.0;
  }
  starts->push_back(n);
  *any_z = z;
}

}  // namespace clc_abi

extern "C" {

int clc_flatten_observations(int n_poses, const double* tag_q_wxyz, const double* tag_t,
                             const int64_t* pts_off, const double* pts, const int64_t* ptl_off,
                             const double* ptl, int use_linefitting_data,
                             int use_boundary_constraint, clc_observation* records,
                             int64_t* n_records) {
  if (n_poses < 0 || !n_records || (n_poses > 0 && (!tag_q_wxyz || !tag_t || !pts_off || !ptl_off)))
    return fail(CLC_ERR_INVALID_ARG, "clc_flatten_observations: bad argument");
  int rc = clc::host::flatten(n_poses, tag_q_wxyz, tag_t, pts_off, pts, ptl_off, ptl,
                              use_linefitting_data != 0, use_boundary_constraint != 0, records, n_records);
  if (rc == CLC_ERR_EMPTY_SCAN)
    return fail(rc, "clc_flatten_observations: boundary constraint on an empty scan (reference: std::out_of_range at LaseCamCalCeres.cpp:278)");
  return rc;
}

int clc_upload_device(clc_handle* h, const clc_observation* records_dev, size_t n) {
  if (!h || (n > 0 && !records_dev)) return fail(CLC_ERR_INVALID_ARG, "clc_upload_device: bad argument");
  CLC_HIP(hipSetDevice(h->device));
  forget_layouts(h);
  int rc = retile_into(h, reinterpret_cast<const double*>(records_dev), n, h->obs);
  if (rc != CLC_OK) return rc;
  CLC_HIP(hipStreamSynchronize(h->stream));
  h->n_obs = n;
  const std::vector<long long> rec_off = {0, (long long)n};
  const std::vector<long long> tile_off = {0, (long long)((n + clc::TILE - 1) / clc::TILE)};
  // a problem one workgroup can hold (<= 512 lanes x 22 points) also gets the lane layout: clc_solve then runs its whole LM loop in
  // ONE single-workgroup launch from registers + LDS (solve_resident_single)
  ResLayout* res = n <= kSmallMaxRecords ? &h->sres : nullptr;
  // what one workgroup cannot hold (more points; or more than 512 scans, or scans whose lengths leave too many half-filled lanes: a
  // lane holds points of ONE scan), up to 65 536 lanes x 40 points, is dealt to 256 workgroups: the cooperative solve (clc_coop.hpp)
  ResLayout* coop = n <= (size_t)clc::COOP_WGS * clc::COOP_NL * (clc::COOP_PR + clc::COOP_PL) ? &h->cres : nullptr;
  return build_layouts(h, reinterpret_cast<const double*>(records_dev), n, rec_off, tile_off, h->obs, nullptr, res, coop);
}

int clc_upload(clc_handle* h, const clc_observation* records, size_t n) {
  if (!h || (n > 0 && !records)) return fail(CLC_ERR_INVALID_ARG, "clc_upload: bad argument");
  CLC_HIP(hipSetDevice(h->device));
  if (n > 0 && n <= kSmallMaxRecords && h->fast_small) {  // a problem one workgroup holds: planned on the host, no read-backs
    std::vector<long long> starts;
    bool any_z = false, used = false;
    plan_record_scans(records, (long long)n, &starts, &any_z);
    const int rc = small_fast_upload(h, starts, (long long)n, any_z, records, nullptr, &used);
    if (rc != CLC_OK || used) return rc;
  }
  DevBuf<double> aos(&h->pool);
  if (n > 0) {
    CLC_HIP(aos.alloc(n * 8));
    CLC_HIP(hipMemcpy(aos.p, records, n * sizeof(clc_observation), hipMemcpyHostToDevice));
  }
  return clc_upload_device(h, reinterpret_cast<const clc_observation*>(aos.p), n);
}

}  // extern "C"

// ---- resident scans + device-side problem assembly ---------------------------------------------------------------
namespace {

// per-pose record offsets of a selection (host, O(poses)); CLC_ERR_EMPTY_SCAN mirrors the reference's .at(0) throw

int selection_offsets(const clc_handle* h, bool linefit, bool boundary, std::vector<long long>* rec_off) {
  const int P = h->store_poses;
  rec_off->assign((size_t)P + 1, 0);
  const std::vector<long long>& off = linefit ? h->s_ptl_off : h->s_pts_off;
  for (int i = 0; i < P; ++i) {
    long long c = off[(size_t)i + 1] - off[(size_t)i];
    if (boundary && linefit) {
      if (h->s_pts_off[(size_t)i + 1] - h->s_pts_off[(size_t)i] <= 0) return CLC_ERR_EMPTY_SCAN;
      c += 2;
    }
    (*rec_off)[(size_t)i + 1] = (*rec_off)[(size_t)i] + c;
  }
  return CLC_OK;
}


}  // namespace

namespace clc_abi {
int adopt_store(clc_handle* h, int n_poses, const StoreFacts& f) {
  const size_t P = (size_t)n_poses;
  const size_t M = (size_t)h->s_pts_off[P], ML = (size_t)h->s_ptl_off[P];
  h->store_small = store_is_reference_size(P, M, ML);
  if (h->store_small) {
    h->s_tag_q.assign(f.tag_q, f.tag_q + 4 * P);
    h->s_tag_t.assign(f.tag_t, f.tag_t + 3 * P);
    h->s_any_z_pts = f.any_z_pts;
    h->s_any_z_ptl = f.any_z_ptl;
    h->s_any_z_ends = f.any_z_ends;
  }
  h->store_lines_equal_points = f.lines_equal_points;
  CLC_HIP(hipStreamSynchronize(h->stream));
  h->store_poses = n_poses;
  h->store_generation++;
  return CLC_OK;
}

// builds the records of the selection on the device into *aos (allocated here)
int flatten_on_device(clc_handle* h, bool linefit, bool boundary, DevBuf<double>* aos, long long* n_out) {
  if (h->store_poses < 0) return fail(CLC_ERR_NO_DATA, "clc_select_observations: no scans stored (clc_store_observations)");
  std::vector<long long> rec_off;
  const int rc = selection_offsets(h, linefit, boundary, &rec_off);
  if (rc == CLC_ERR_EMPTY_SCAN)
    return fail(rc, "clc_select_observations: boundary constraint on an empty scan (reference: std::out_of_range at LaseCamCalCeres.cpp:278)");
  const int P = h->store_poses;
  const long long N = rec_off[(size_t)P];
  *n_out = N;
  CLC_HIP(aos->alloc((size_t)std::max<long long>(N, 1) * 8));
  if (N == 0 || P == 0) return CLC_OK;
  long long* d_off = h->d_soff;
  CLC_HIP(hipMemcpyAsync(d_off + 2 * ((size_t)P + 1), rec_off.data(), sizeof(long long) * ((size_t)P + 1), hipMemcpyHostToDevice,
                         h->stream));
  hipLaunchKernelGGL(clc::flatten_kernel, dim3((unsigned)P), dim3(clc::BLOCK), 0, h->stream, P, h->d_sq, h->d_st, d_off,
                     h->d_spts, d_off + ((size_t)P + 1), h->d_sptl, linefit ? 1 : 0, boundary ? 1 : 0,
                     d_off + 2 * ((size_t)P + 1), aos->p);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipStreamSynchronize(h->stream));  // rec_off (host vector) must outlive the copy
  return CLC_OK;
}


}  // namespace clc_abi

extern "C" {

int clc_store_observations(clc_handle* h, int n_poses, const double* tag_q_wxyz, const double* tag_t,
                           const int64_t* pts_off, const double* pts, const int64_t* ptl_off, const double* ptl) {
  if (!h || n_poses < 0 || (n_poses > 0 && (!tag_q_wxyz || !tag_t || !pts_off || !ptl_off)))
    return fail(CLC_ERR_INVALID_ARG, "clc_store_observations: bad argument");
  const size_t P = (size_t)n_poses;
  h->store_poses = -1;
  h->s_pts_off.assign(P + 1, 0);
  h->s_ptl_off.assign(P + 1, 0);
  for (size_t i = 0; i <= P && P > 0; ++i) {
    h->s_pts_off[i] = pts_off[i] - pts_off[0];
    h->s_ptl_off[i] = ptl_off[i] - ptl_off[0];
    if (i > 0 && (h->s_pts_off[i] < h->s_pts_off[i - 1] || h->s_ptl_off[i] < h->s_ptl_off[i - 1]))
      return fail(CLC_ERR_INVALID_ARG, "clc_store_observations: offsets not monotone");
  }
  const size_t M = (size_t)h->s_pts_off[P], ML = (size_t)h->s_ptl_off[P];
  if ((M > 0 && !pts) || (ML > 0 && !ptl)) return fail(CLC_ERR_INVALID_ARG, "clc_store_observations: NULL points");
  CLC_HIP(hipSetDevice(h->device));
  // (never empty: at least one element each)
  CLC_HIP(h->d_sq.grow(std::max<size_t>(P * 4, 1)));
  CLC_HIP(h->d_st.grow(std::max<size_t>(P * 3, 1)));
  CLC_HIP(h->d_spts.grow(std::max<size_t>(M * 3, 1)));
  CLC_HIP(h->d_sptl.grow(std::max<size_t>(ML * 3, 1)));
  CLC_HIP(h->d_soff.grow(3 * (P + 1)));
  if (P > 0) {
    CLC_HIP(hipMemcpyAsync(h->d_sq, tag_q_wxyz, P * 4 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(h->d_st, tag_t, P * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    long long* d_off = h->d_soff;
    CLC_HIP(hipMemcpyAsync(d_off, h->s_pts_off.data(), (P + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    CLC_HIP(hipMemcpyAsync(d_off + (P + 1), h->s_ptl_off.data(), (P + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  }
  if (M > 0) CLC_HIP(hipMemcpyAsync(h->d_spts, pts + 3 * pts_off[0], M * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (ML > 0) CLC_HIP(hipMemcpyAsync(h->d_sptl, ptl + 3 * ptl_off[0], ML * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  // reference-size scans: the host keeps what it needs to plan a selection's layouts itself (tag poses, whether any z is non-zero)
  StoreFacts f;
  if (store_is_reference_size(P, M, ML)) {
    f.tag_q = tag_q_wxyz;
    f.tag_t = tag_t;
    auto any_z = [](const double* p, size_t count) { for (size_t k = 0; k < count; ++k) if (p[3 * k + 2] != 0.0) return true; return false; };
    f.any_z_pts = M > 0 && any_z(pts + 3 * pts_off[0], M);
    f.any_z_ptl = ML > 0 && any_z(ptl + 3 * ptl_off[0], ML);
    for (size_t i = 0; i < P; ++i)
      if (pts_off[i + 1] > pts_off[i] && (pts[3 * pts_off[i] + 2] != 0.0 || pts[3 * (pts_off[i + 1] - 1) + 2] != 0.0)) f.any_z_ends = true;
  }
  // points_on_line bit-identical to points (the simulation node's input): the selections (linefit, no boundary) and (no linefit) are
  // then the same records and clc_select_observations builds them once.  Checked for reference-size inputs only (a memcmp of <= 384 KB).
  f.lines_equal_points = M == ML && M <= 16384 && h->s_pts_off == h->s_ptl_off &&
                         (M == 0 || std::memcmp(pts + 3 * pts_off[0], ptl + 3 * ptl_off[0], M * 3 * sizeof(double)) == 0);
  return adopt_store(h, n_poses, f);  // (waits for the stream: the caller's arrays may go away)
}

int64_t clc_store_generation(const clc_handle* h) { return h ? h->store_generation : -1; }

int clc_select_observations(clc_handle* h, int use_linefitting_data, int use_boundary_constraint, int64_t* n_records) {
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_select_observations: NULL handle");
  CLC_HIP(hipSetDevice(h->device));
  // The selection the handle's observation array already IS (same stored scans, same residual blocks): nothing to build.  The sequence
  // of main/calibr_offline.cpp:166-170 selects points_on_line for the closed form and again for the refinement; the simulation node
  // stores points_on_line == points (main/calibr_simulation.cpp:102), so its two selections are the same records as well.
  bool linefit = use_linefitting_data != 0;
  const bool boundary = use_boundary_constraint != 0 && linefit;  // (the board-edge terms exist with points_on_line only, :258)
  if (linefit && !boundary && h->store_lines_equal_points) linefit = false;
  const long long key = h->store_poses < 0 ? -1 : h->store_generation * 4 + (linefit ? 2 : 0) + (boundary ? 1 : 0);
  const long long cfg = ((long long)h->launch_flags << 8) | ((long long)h->auto_disable << 1) | (h->small_on_coop ? 1 : 0);  // what an upload depends on
  if (key >= 0 && key == h->selection_key && cfg == h->selection_cfg) {
    if (n_records) *n_records = (int64_t)h->n_obs;
    return CLC_OK;
  }
  if (h->store_small && h->fast_small && h->store_poses > 0) {  // reference-size scans: planned on the host, enqueued without a read-back
    std::vector<long long> rec_off, starts;
    const int orc = selection_offsets(h, linefit, boundary, &rec_off);
    bool any_z = false, used = false;
    if (orc == CLC_OK && rec_off.back() > 0 && (size_t)rec_off.back() <= kSmallMaxRecords &&
        plan_selection_scans(h, linefit, boundary, rec_off, &starts, &any_z)) {
      const SmallFlatten fj = {h->store_poses, linefit, boundary, &rec_off};
      const int frc = small_fast_upload(h, starts, rec_off.back(), any_z, nullptr, &fj, &used);
      if (frc != CLC_OK) return frc;
      if (used) {
        if (n_records) *n_records = (int64_t)rec_off.back();
        h->selection_key = key; h->selection_cfg = cfg;
        return CLC_OK;
      }
    }
  }
  DevBuf<double> aos(&h->pool);
  long long N = 0;
  int rc = flatten_on_device(h, linefit, boundary, &aos, &N);
  if (rc != CLC_OK) return rc;
  if (n_records) *n_records = (int64_t)N;
  rc = clc_upload_device(h, reinterpret_cast<const clc_observation*>(aos.p), (size_t)N);
  if (rc == CLC_OK) { h->selection_key = key; h->selection_cfg = cfg; }  // (clc_upload_device — any upload — forgets the previous selection)
  return rc;
}


}  // extern "C"

// ---- batched ---------------------------------------------------------------------------
namespace {
// records: host pointer (on_device = false: staged through a temporary device buffer) or device pointer
int upload_batched_impl(clc_handle* h, const clc_observation* records, bool on_device, const int64_t* offsets,
                        size_t n_problems) {
  if (!h || !offsets || (n_problems > 0 && !records))
    return fail(CLC_ERR_INVALID_ARG, "clc_upload_batched: bad argument");
  CLC_HIP(hipSetDevice(h->device));
  {  // the batched unit's code object: loaded here, once per device and process, before the first batched solve (see clc_create)
    static std::atomic<bool> warm[64];
    std::atomic<bool>& w = warm[h->device >= 0 && h->device < 64 ? h->device : 0];
    if (!w.exchange(true) && !std::getenv("CLC_LAZY_MODULES")) warm_batched();
  }
  const size_t P = n_problems;
  std::vector<long long> tile_off(P + 1, 0), nobs(P, 0);
  long long max_tiles = 0;
  for (size_t k = 0; k < P; ++k) {
    const int64_t n = offsets[k + 1] - offsets[k];
    if (n < 0) return fail(CLC_ERR_INVALID_ARG, "clc_upload_batched: offsets not monotone");
    nobs[k] = n;
    tile_off[k + 1] = tile_off[k] + (n + clc::TILE - 1) / clc::TILE;
    max_tiles = std::max<long long>(max_tiles, tile_off[k + 1] - tile_off[k]);
  }
  h->batch_max_tiles = max_tiles;
  const size_t total_tiles = (size_t)tile_off[P];
  h->batch_total_tiles = total_tiles;
  CLC_HIP(h->batch.d_tiles.grow(std::max<size_t>(total_tiles, 1) * clc::TILE_DOUBLES));
  if (P == 0) { h->n_problems = 0; return CLC_OK; }
  const size_t rec_doubles = sizeof(clc_result_record) / sizeof(double);
  if (P * rec_doubles > h->d_results.size()) h->results_valid = 0;  // (the records are about to be freed)
  CLC_HIP(h->d_tile_off.grow(P + 1));
  CLC_HIP(h->d_nobs.grow(P));
  CLC_HIP(h->h_poses.grow(7 * P));
  CLC_HIP(h->h_summaries.grow(P));
  CLC_HIP(h->d_states.grow(P));
  CLC_HIP(h->d_results.grow(P * rec_doubles));
  CLC_HIP(h->d_prob_row.grow(P + 1));
  CLC_HIP(hipMemcpy(h->d_tile_off, tile_off.data(), sizeof(long long) * (P + 1), hipMemcpyHostToDevice));
  CLC_HIP(hipMemcpy(h->d_nobs, nobs.data(), sizeof(long long) * P, hipMemcpyHostToDevice));
  // stage the AoS records, then re-tile every problem into its own whole tiles
  const size_t n_total = (size_t)(offsets[P] - offsets[0]);
  DevBuf<double> baos(&h->pool);
  DevBuf<long long> boff(&h->pool);
  double* d_aos = nullptr;
  if (n_total > 0 && on_device) {
    d_aos = const_cast<double*>(reinterpret_cast<const double*>(records + offsets[0]));
  } else if (n_total > 0) {
    CLC_HIP(baos.alloc(n_total * 8));
    CLC_HIP(hipMemcpy(baos.p, records + offsets[0], n_total * sizeof(clc_observation), hipMemcpyHostToDevice));
    d_aos = baos.p;
  }
  std::vector<long long> rel(P + 1);
  for (size_t k = 0; k <= P; ++k) rel[k] = offsets[k] - offsets[0];
  CLC_HIP(boff.alloc(P + 1));
  long long* d_off = boff.p;
  CLC_HIP(hipMemcpy(d_off, rel.data(), sizeof(long long) * (P + 1), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(clc::retile_batched_kernel, dim3((unsigned)P), dim3(256), 0, h->stream, d_aos, d_off,
                     h->d_tile_off, h->batch.d_tiles);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  int crc = CLC_OK;
  h->batch.invalidate();
  h->bres.ok = false;
  h->sub_offsets.clear();  // (the lane -> block map of clc_solve_subsets belongs to the layout about to be rebuilt)
  h->results_valid = 0;
  if (e == hipSuccess && d_aos) crc = build_layouts(h, d_aos, n_total, rel, tile_off, h->batch, h->d_prob_row, &h->bres, nullptr);
  if (e != hipSuccess) return fail(CLC_ERR_HIP, "clc_upload_batched: retile", e);
  if (crc != CLC_OK) return crc;
  h->batch_max_rows = 0;
  if (h->batch.rows_ok) {  // O(P) words back: the whole-solve kernel is chosen on the real longest problem, not an estimate
    std::vector<long long> pr(P + 1);
    CLC_HIP(hipMemcpy(pr.data(), h->d_prob_row, sizeof(long long) * (P + 1), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < P; ++k) h->batch_max_rows = std::max(h->batch_max_rows, pr[k + 1] - pr[k]);
  }
  h->n_problems = P;
  h->batch_records = n_total;
  return CLC_OK;
}
}  // namespace

int clc_upload_batched(clc_handle* h, const clc_observation* records, const int64_t* offsets, size_t n_problems) {
  return upload_batched_impl(h, records, false, offsets, n_problems);
}

int clc_upload_batched_device(clc_handle* h, const clc_observation* records_dev, const int64_t* offsets, size_t n_problems) {
  return upload_batched_impl(h, records_dev, true, offsets, n_problems);
}

size_t clc_num_problems(const clc_handle* h) { return h ? h->n_problems : 0; }

