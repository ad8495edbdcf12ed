// abi_batched.hip — clc_solve_batched: many independent problems per launch (resident kernel, whole-solve kernel, lockstep launches);
// clc_solve_multistart / clc_solve_subsets / clc_score_blocks: many starts / weighted pose subsets / block scores of many poses on ONE
// uploaded problem.
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"
#include "clc_consensus.hpp"

using namespace clc_abi;

namespace clc_abi {

void warm_batched() {
  warm_kernel(reinterpret_cast<const void*>(&clc::resident_solve_kernel<true, true, 4, kResPR256, kResPL256, kResCtrl4>));
  warm_kernel(reinterpret_cast<const void*>(&clc::batched_init_kernel));
}

int batched_launch_setup(clc_handle* h, BatchedLaunch* bl) {
  const StreamLayout& L = h->batch;
  const BatchShape b = {h->n_problems, h->batch_total_tiles, h->batch_max_tiles, L.n_rows, h->batch_max_rows, L.compact_ok, L.rows_ok, L.rows_z,
                        h->bres.ok, h->bres.with_z, h->bres.rows, h->bres.lanes};
  *bl = plan_batched(h->steer, b, h->num_cus);
  CLC_HIP(h->d_bpartials.grow(bl->n_blocks * clc::NACC));
  return CLC_OK;
}

void launch_batched_eval(clc_handle* h, const clc_options& opt, const BatchedLaunch& bl) {
  const unsigned n_blocks = (unsigned)bl.n_blocks;
  const int bpp = bl.bpp;
  if (bl.rows) {  // WAVE: one wave per workgroup
    with_flags([&](auto Z, auto WAVE, auto LOSS, auto NT) {
      constexpr int BT = WAVE ? 64 : 256;
      hipLaunchKernelGGL((clc::batched_rows_eval_kernel<LOSS, NT, BT, Z>), dim3(n_blocks), dim3(BT), 0, h->stream, h->batch.d_rxy,
                         h->batch.d_rdesc(), h->d_prob_row, h->d_states, bpp, opt.loss_scale_factor,
                         h->d_bpartials);
    }, h->batch.rows_z, bl.rows_wave, opt.use_loss != 0, bl.rows_nt);
    return;
  }
  const auto launch = [&](auto CP, auto DEEP, auto LOSS, auto NT) {
    hipLaunchKernelGGL((clc::batched_eval_kernel<LOSS, CP, NT, DEEP>), dim3(n_blocks), dim3(clc::BLOCK), 0, h->stream,
                       CP ? h->batch.d_ctiles : h->batch.d_tiles, h->batch.d_groups, h->d_tile_off, h->d_nobs, h->d_states, bpp, opt.loss_scale_factor,
                       h->d_bpartials);
  };
  if (bl.compact) with_flags(launch, std::true_type{}, bl.deep, opt.use_loss != 0, bl.nt);
  else with_flags(launch, std::false_type{}, std::false_type{}, opt.use_loss != 0, bl.nt);
}

void launch_resident(clc_handle* h, const clc_options& opt, const BatchedLaunch& bl, const ResidentLaunch& w) {
  // one workgroup per problem (start, subset), the problem read from HBM once and kept in registers + LDS for its whole solve
  // W4: the 256-lane form (4 waves); Z: 24-byte slots (p.z != 0 in some record of the batch), on 512 lanes
  const auto launch = [&](auto WEIGHTED, auto Z, auto W4, auto LOSS, auto NT) {
    constexpr int NW = W4 ? 4 : 8;
    constexpr int PR = Z ? kResPRz : W4 ? kResPR256 : kResPR512, PL = Z ? kResPLz : W4 ? kResPL256 : kResPL512;
    // The weighted form's three inputs ride in res_row, trace and trace_cap (clc_resident.hpp, WEIGHTED): a multi-start launch reads
    // none of the three, and the kernel's argument list must not grow (profiles/subset_solves.md).  The one place they are cast.
    const unsigned int* const res_row = WEIGHTED ? w.d_lane_block : h->bres.d_row.get();
    clc_iteration* const trace = WEIGHTED ? reinterpret_cast<clc_iteration*>(w.d_weights) : nullptr;
    hipLaunchKernelGGL((clc::resident_solve_kernel<LOSS, NT, NW, PR, PL, W4 ? kResCtrl4 : kResCtrl8, Z, WEIGHTED>), dim3((unsigned)w.workgroups),
                       dim3(NW * 64), 0, h->stream, h->bres.d_xy, res_row, h->bres.d_desc, h->batch.d_groups, w.uni_ppl, opt, trace,
                       WEIGHTED ? w.n_blocks : 0, w.d_poses, w.d_summaries, w.d_results, nullptr, nullptr, w.rec_base, w.rec_host, w.seg_off,
                       w.goal, Z ? h->bres.d_z : nullptr);
  };
  const bool weighted = w.d_weights != nullptr;
  if (h->bres.with_z) with_flags(launch, weighted, std::true_type{}, std::false_type{}, opt.use_loss != 0, bl.res_nt);
  else with_flags(launch, weighted, std::false_type{}, h->bres.lanes == 256, opt.use_loss != 0, bl.res_nt);
}

int batched_check_inputs(const char* who, const clc_options& opt, const double* poses, size_t P) {
  if (opt.max_num_iterations < 0) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": max_num_iterations < 0").c_str());
  if (opt.use_loss && !(opt.loss_scale_factor > 0.0))
    return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": loss_scale_factor must be > 0").c_str());
  // all 7 P start-pose doubles finite: exponent field not all ones — an integer OR-reduction the compiler vectorises (57 344 values at C4)
  unsigned long long bad = 0;
  for (size_t i = 0; i < 7 * P; ++i) {
    unsigned long long b;
    std::memcpy(&b, &poses[i], sizeof(b));
    bad |= (unsigned long long)(((b >> 52) & 0x7FFull) == 0x7FFull);
  }
  if (bad) return fail(CLC_ERR_NONFINITE, (std::string(who) + ": non-finite initial pose").c_str());
  return CLC_OK;
}

}  // namespace clc_abi

namespace {

// What clc_solve_batched and the calls on a batch of one do between their own argument checks and their staging: the options (the
// caller's or the defaults) and the n_poses start poses checked, the device made current, the wall clock started, the launch planned.
struct BatchedCall {
  clc_options opt;
  BatchedLaunch bl;
  std::chrono::steady_clock::time_point t0;
  bool timed() const { return opt.profile_events == 1; }  // HIP event pair around the one launch -> clc_summary.eval_kernel_ms of every row
};
int begin_batched_call(const char* who, clc_handle* h, const clc_options* opt_in, const double* poses, size_t n_poses, BatchedCall* c) {
  if (opt_in) c->opt = *opt_in; else clc_options_default(&c->opt);
  CLC_TRY(batched_check_inputs(who, c->opt, poses, n_poses));
  CLC_HIP(hipSetDevice(h->device));
  c->t0 = std::chrono::steady_clock::now();
  return batched_launch_setup(h, &c->bl);
}

// clc_solve_multistart / clc_solve_subsets / clc_score_blocks: the shared observations are ONE uploaded problem ...
int require_batch_of_one(const char* who, const clc_handle* h) {
  if (!h->batch.d_tiles || h->n_problems != 1)
    return fail(CLC_ERR_NO_DATA, (std::string(who) + ": the shared observations must be uploaded as a batch of ONE problem (clc_upload_batched, "
                                                     "n_problems = 1)").c_str());
  return CLC_OK;
}
// ... and, for the calls without another route, one that a workgroup holds (`instead`: what the caller can do otherwise)
int require_resident(const char* who, const BatchedLaunch& bl, const char* instead) {
  if (bl.resident) return CLC_OK;
  return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": the problem is not held by one workgroup (clc_path_info.batched_resident == 0, or the "
                                                       "launch flags rule the resident kernel out): " + instead).c_str());
}

// ONE launch (launch() enqueues it on the handle's stream), between the two events when timed
template <class Launch>
int launch_once(clc_handle* h, bool timed, Launch&& launch) {
  if (timed) {
    CLC_TRY(ensure_events(h, 2));
    CLC_HIP(hipEventRecord(h->ev[0], h->stream));
  }
  launch();
  CLC_HIP(hipGetLastError());
  if (timed) CLC_HIP(hipEventRecord(h->ev[1], h->stream));
  return CLC_OK;
}
// ... and its end: the stream synchronised (kernel completion makes the outcomes written over PCIe visible), the kernel time of the
// event pair.  (A completion flag raised by the last workgroup to finish, polled by the host instead of this blocking synchronisation,
// was measured: every workgroup then needs a system-scope release before it counts itself in, which on this part writes back L2 —
// C4 shard 0.93 -> 1.28 ms, C3 0.150 -> 0.166.  The single-workgroup solve keeps its flag: one release per solve.  Polling the stream
// with hipStreamQuery was measured too: no difference — the 70-80 us between the kernel's end event and the return are not the wake-up.)
int wait_launch(clc_handle* h, bool timed, float* kernel_ms) {
  CLC_HIP(hipStreamSynchronize(h->stream));
  *kernel_ms = 0.0f;
  if (timed) CLC_HIP(hipEventElapsedTime(kernel_ms, h->ev[0], h->ev[1]));
  return CLC_OK;
}
// the wall time since t0 (and with `timed` the kernel time of the one launch) in every summary
void stamp_summaries(clc_summary* summaries, size_t n, std::chrono::steady_clock::time_point t0, bool timed, float kernel_ms) {
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (size_t k = 0; k < n; ++k) {
    summaries[k].solve_ms = ms;
    if (timed) { summaries[k].eval_kernel_ms = (double)kernel_ms; summaries[k].eval_kernel_launches = 1; }
  }
}

// The end of every clc_solve_batched path: the launches waited for, the results valid for clc_gather_results, copied out unless solved
// in place, the times in every summary.
int finish_batched(clc_handle* h, bool in_place, double* poses, clc_summary* summaries, std::chrono::steady_clock::time_point t0,
                   bool timed) {
  const size_t P = h->n_problems;
  float kernel_ms;
  CLC_TRY(wait_launch(h, timed, &kernel_ms));
  h->results_valid = P;
  if (!in_place) {
    std::memcpy(poses, h->h_poses, sizeof(double) * 7 * P);
    std::memcpy(summaries, h->h_summaries, sizeof(clc_summary) * P);
  }
  stamp_summaries(summaries, P, t0, timed, kernel_ms);
  return CLC_OK;
}

// clc_solve_multistart / clc_solve_subsets: the n start poses into the multi-start staging arrays (pinned, device-mapped), room for
// the n outcomes.  (The previous call ended with a stream synchronisation: nothing still reads or writes the staging buffers.)
int stage_starts(clc_handle* h, const double* poses, size_t n) {
  CLC_HIP(h->h_ms_poses.grow(7 * n));
  CLC_HIP(h->h_ms_summaries.grow(n));
  CLC_HIP(h->d_ms_results.grow(sizeof(clc_result_record) / sizeof(double) * n));
  std::memcpy(h->h_ms_poses, poses, sizeof(double) * 7 * n);
  return CLC_OK;
}

std::atomic<long long> g_lane_map_builds{0};  // lane -> block maps built in this process (hooks build: clc_debug_lane_map_builds)

// clc_solve_subsets / clc_score_blocks: the cut of the one uploaded problem's records into consecutive blocks
int check_block_offsets(const char* who, const clc_handle* h, size_t n_blocks, const int64_t* block_offsets) {
  const std::string w(who);
  if (n_blocks > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, (w + ": too many blocks").c_str());
  if (block_offsets[0] != 0 || block_offsets[n_blocks] != (int64_t)h->batch_records)
    return fail(CLC_ERR_INVALID_ARG, (w + ": block_offsets must start at 0 and end at the problem's record count").c_str());
  for (size_t b = 0; b < n_blocks; ++b)
    if (block_offsets[b + 1] < block_offsets[b]) return fail(CLC_ERR_INVALID_ARG, (w + ": block_offsets not monotone").c_str());
  return CLC_OK;
}

// The lane -> block map of problem 0's lane layout (h->d_sub_lane_block): built once per (n_blocks, offsets) and upload, shared by
// clc_solve_subsets and clc_score_blocks.  Ends with the stream synchronised when it builds.
int ensure_lane_block_map(const char* who, clc_handle* h, size_t n_blocks, const int64_t* block_offsets) {
  if (h->sub_offsets.size() == n_blocks + 1 && std::memcmp(h->sub_offsets.data(), block_offsets, sizeof(int64_t) * (n_blocks + 1)) == 0)
    return CLC_OK;
  const std::string w(who);
  const int lanes = h->bres.lanes;
  h->sub_offsets.clear();
  CLC_HIP(h->d_sub_lane_block.grow((size_t)lanes));
  DevBuf<long long> d_off(&h->pool);
  DevBuf<unsigned int> d_flag(&h->pool);
  CLC_HIP(d_off.alloc(n_blocks + 1));
  CLC_HIP(d_flag.alloc(1));
  static_assert(sizeof(long long) == sizeof(int64_t), "block offsets are copied as they are");
  CLC_HIP(hipMemcpyAsync(d_off.p, block_offsets, sizeof(int64_t) * (n_blocks + 1), hipMemcpyHostToDevice, h->stream));
  CLC_HIP(hipMemsetAsync(d_flag.p, 0, sizeof(unsigned int), h->stream));
  const auto launch = [&](auto NL) {
    hipLaunchKernelGGL(clc::subset_lane_map_kernel<NL>, dim3(1), dim3(NL), 0, h->stream, h->bres.d_desc, d_off.p, (int)n_blocks,
                       (long long)h->batch_records, h->d_sub_lane_block, d_flag.p);
  };
  if (lanes == 256) launch(cint<256>); else launch(cint<512>);
  CLC_HIP(hipGetLastError());
  unsigned int flag = 0;
  CLC_HIP(hipMemcpyAsync(&flag, d_flag.p, sizeof(flag), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  g_lane_map_builds.fetch_add(1, std::memory_order_relaxed);
  if (flag & 2u) return fail(CLC_ERR_INVALID_ARG, (w + ": the lane layout does not match the record count").c_str());
  if (flag & 1u)
    return fail(CLC_ERR_INVALID_ARG, (w + ": a block boundary falls inside a scan (consecutive records of one plane): "
                                          "a block must hold whole scans").c_str());
  h->sub_offsets.assign(block_offsets, block_offsets + n_blocks + 1);
  return CLC_OK;
}

}  // namespace

extern "C" {

int clc_batched_host_buffers(clc_handle* h, double** poses, clc_summary** summaries) {
  if (!h) return fail(CLC_ERR_INVALID_ARG, "clc_batched_host_buffers: NULL handle");
  if (h->n_problems == 0 || !h->h_poses) return fail(CLC_ERR_NO_DATA, "clc_batched_host_buffers: no problems uploaded");
  if (poses) *poses = h->h_poses;
  if (summaries) *summaries = h->h_summaries;
  return CLC_OK;
}

int clc_solve_batched(clc_handle* h, const clc_options* opt_in, double* poses, clc_summary* summaries) {
  if (!h || !poses || !summaries) return fail(CLC_ERR_INVALID_ARG, "clc_solve_batched: bad argument");
  if (!h->batch.d_tiles || h->n_problems == 0) return fail(CLC_ERR_NO_DATA, "clc_solve_batched: no problems uploaded");
  // the handle's own pinned arrays (clc_batched_host_buffers): solved in place, no staging copies
  const bool in_place = poses == h->h_poses && summaries == h->h_summaries;
  if ((poses == h->h_poses) != (summaries == h->h_summaries))
    return fail(CLC_ERR_INVALID_ARG, "clc_solve_batched: pass both of the handle's host buffers or neither");
  const size_t P = h->n_problems;
  BatchedCall c;
  CLC_TRY(begin_batched_call("clc_solve_batched", h, opt_in, poses, P, &c));
  const clc_options& opt = c.opt;
  const BatchedLaunch& bl = c.bl;
  const int bpp = bl.bpp;
  // (the previous batch ended with a stream synchronisation: nothing still reads or writes the staging buffers)
  if (!in_place) std::memcpy(h->h_poses, poses, sizeof(double) * 7 * P);
  if (bl.resident) {
    ResidentLaunch w = ResidentLaunch::whole_batch(h);
    w.d_summaries = h->h_summaries.dev();
    w.d_results = h->d_results;
    CLC_TRY(launch_once(h, c.timed(), [&] { launch_resident(h, opt, bl, w); }));
    return finish_batched(h, in_place, poses, summaries, c.t0, c.timed());
  }
  if (bl.whole_solve) {
    // one 256-thread workgroup per problem: the whole solve of every problem in ONE launch (batched_solve_kernel)
    const clc::RowDesc* bdesc = h->batch.d_rdesc();
    with_flags([&](auto LOSS, auto NT) {
      hipLaunchKernelGGL((clc::batched_solve_kernel<LOSS, NT>), dim3((unsigned)P), dim3(clc::BLOCK), 0, h->stream, h->batch.d_rxy, bdesc,
                         h->d_prob_row, opt, h->h_poses.dev(), h->h_summaries.dev(), h->d_results);
    }, opt.use_loss != 0, bl.rows_nt);
    CLC_HIP(hipGetLastError());
    return finish_batched(h, in_place, poses, summaries, c.t0, false);
  }
  const int lm_threads = bl.lm_threads;
  const unsigned lm_blocks = bl.lm_blocks;
  hipLaunchKernelGGL(clc::batched_init_kernel, dim3(lm_blocks), dim3(lm_threads), 0, h->stream, h->d_states,
                     opt, h->h_poses.dev(), (int)P, h->d_queue, h->d_ticket);
  CLC_HIP(hipGetLastError());
  const int lookahead = opt.launch_ahead > 0 ? opt.launch_ahead : default_lookahead();
  // at the iteration cap the loop ends once every launch is consumed: batched_finish_kernel closes the stragglers
  const LaunchAhead la = {"clc_solve_batched", opt.max_num_iterations + 1, lookahead, LaunchAhead::kReturn, 60.0};
  int launched = 0;
  const int rc = launch_ahead(h->h_mailbox, h->stream, la, [&](const int k) {
    launch_batched_eval(h, opt, bl);
    hipLaunchKernelGGL(clc::batched_lm_kernel, dim3(lm_blocks), dim3(lm_threads), 0, h->stream,
                       h->d_bpartials, bpp, h->d_states, opt, (int)P, h->d_queue, h->d_ticket, k,
                       h->h_mailbox.dev(), h->h_poses.dev(), h->h_summaries.dev(), h->d_results);
    return CLC_OK;
  }, &launched);
  if (rc != CLC_OK) return rc;
  CLC_HIP(hipGetLastError());
  if (__atomic_load_n(&h->h_mailbox->status, __ATOMIC_ACQUIRE) == CLC_RUNNING) {  // iteration cap of this loop: some problem still runs
    hipLaunchKernelGGL(clc::batched_finish_kernel, dim3(lm_blocks), dim3(lm_threads), 0, h->stream, h->d_states,
                       (int)P, h->h_poses.dev(), h->h_summaries.dev(), h->d_results);
    CLC_HIP(hipGetLastError());
  }
  CLC_TRY(finish_batched(h, in_place, poses, summaries, c.t0, false));
  for (size_t k = 0; k < P; ++k)
    if (summaries[k].termination == CLC_RUNNING) summaries[k].termination = CLC_FAILURE;
  return CLC_OK;
}


// Multi-hypothesis calibration on SHARED observations (BASELINE.json north_star: "batched/multi-hypothesis calibration"): n_starts
// independent LM solves — one ceres::Solve each, src/LaseCamCalCeres.cpp:299-309 — from n_starts start poses on the ONE problem the handle
// holds as a batch of one (clc_upload_batched* with n_problems = 1).  Where the problem fits a workgroup (the on-chip lane layout: at most
// 256 x 44 points and 256 scans, or 512 x 22 / 512 scans) ONE launch runs every start: a workgroup per start, every workgroup loading the
// SAME lane layout (one copy in HBM — 0.17 MB for 1e4 observations where 1 024 uploaded copies are 178 MB — read by the first round of
// workgroups, served from L2 to the rest) and solving from its own pose; otherwise the starts run one after the other on the batch's
// streaming path.  Same kernel, same arithmetic as clc_solve_batched of n_starts uploaded copies: bit-identical results.
int clc_solve_multistart(clc_handle* h, const clc_options* opt_in, size_t n_starts, double* poses, clc_summary* summaries) {
  if (!h || !poses || !summaries || n_starts == 0) return fail(CLC_ERR_INVALID_ARG, "clc_solve_multistart: bad argument");
  CLC_TRY(require_batch_of_one("clc_solve_multistart", h));
  BatchedCall c;
  CLC_TRY(begin_batched_call("clc_solve_multistart", h, opt_in, poses, n_starts, &c));
  if (!c.bl.resident) {  // the problem does not fit a workgroup (or explicit flags): one start after the other, still ONE copy of the data
    for (size_t k = 0; k < n_starts; ++k) CLC_TRY(clc_solve_batched(h, &c.opt, poses + 7 * k, summaries + k));
    h->results_valid = 0;  // (the handle's result buffer holds the last start only: nothing for clc_gather_results)
    return CLC_OK;
  }
  CLC_TRY(stage_starts(h, poses, n_starts));
  ResidentLaunch w = ResidentLaunch::on_problem0(h, n_starts, h->h_ms_poses.dev());
  w.d_summaries = h->h_ms_summaries.dev();
  w.d_results = h->d_ms_results;
  CLC_TRY(launch_once(h, c.timed(), [&] { launch_resident(h, c.opt, c.bl, w); }));
  float kernel_ms;
  CLC_TRY(wait_launch(h, c.timed(), &kernel_ms));
  std::memcpy(poses, h->h_ms_poses, sizeof(double) * 7 * n_starts);
  std::memcpy(summaries, h->h_ms_summaries, sizeof(clc_summary) * n_starts);
  stamp_summaries(summaries, n_starts, c.t0, c.timed(), kernel_ms);
  for (size_t k = 0; k < n_starts; ++k)
    if (!all_finite(poses + 7 * k, 7)) return fail(CLC_ERR_NONFINITE, "clc_solve_multistart: non-finite result");
  return CLC_OK;
}


// Resampled calibrations on SHARED observations: n_subsets independent LM solves of the ONE problem the handle holds as a batch of one,
// subset k being the problem in which every record of block b (records [block_offsets[b], block_offsets[b + 1]) — a pose's rows)
// appears weights[k * n_blocks + b] times (0: left out).  One launch of the weighted resident kernel: a workgroup per subset on problem 0's lane
// layout, which is neither re-planned nor touched (clc_solve_multistart before and after returns the same bits).
int clc_solve_subsets(clc_handle* h, const clc_options* opt_in, size_t n_blocks, const int64_t* block_offsets, size_t n_subsets,
                      const uint8_t* weights, double* poses, clc_summary* summaries) {
  if (!h || !block_offsets || !weights || !poses || !summaries || n_blocks == 0 || n_subsets == 0)
    return fail(CLC_ERR_INVALID_ARG, "clc_solve_subsets: bad argument");
  CLC_TRY(require_batch_of_one("clc_solve_subsets", h));
  if (n_subsets > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_solve_subsets: too many subsets");
  CLC_TRY(check_block_offsets("clc_solve_subsets", h, n_blocks, block_offsets));
  BatchedCall c;
  CLC_TRY(begin_batched_call("clc_solve_subsets", h, opt_in, poses, n_subsets, &c));
  CLC_TRY(require_resident("clc_solve_subsets", c.bl, "materialise the subsets and use clc_solve_batched"));
  CLC_TRY(ensure_lane_block_map("clc_solve_subsets", h, n_blocks, block_offsets));
  CLC_TRY(stage_starts(h, poses, n_subsets));
  CLC_HIP(h->h_sub_weights.grow(n_subsets * n_blocks));
  std::memcpy(h->h_sub_weights, weights, n_subsets * n_blocks);
  // a workgroup whose subset is empty writes nothing: its summary stays what it is set to here
  clc_summary none;
  std::memset(&none, 0, sizeof(none));
  none.termination = CLC_FAILURE;
  none.num_evaluations = -1;  // (no written summary has it)
  for (size_t k = 0; k < n_subsets; ++k) h->h_ms_summaries[k] = none;
  ResidentLaunch w = ResidentLaunch::on_problem0(h, n_subsets, h->h_ms_poses.dev());
  w.d_summaries = h->h_ms_summaries.dev();
  w.d_results = h->d_ms_results;
  w.d_lane_block = h->d_sub_lane_block;
  w.n_blocks = (int)n_blocks;
  w.d_weights = h->h_sub_weights.dev();
  CLC_TRY(launch_once(h, c.timed(), [&] { launch_resident(h, c.opt, c.bl, w); }));
  float kernel_ms;
  CLC_TRY(wait_launch(h, c.timed(), &kernel_ms));
  std::memcpy(summaries, h->h_ms_summaries, sizeof(clc_summary) * n_subsets);
  stamp_summaries(summaries, n_subsets, c.t0, c.timed(), kernel_ms);
  for (size_t k = 0; k < n_subsets; ++k) {
    // an empty subset or a non-finite end: CLC_FAILURE in its summary, its pose left as the caller passed it — never the call's failure
    const double* out = h->h_ms_poses + 7 * k;
    const bool written = summaries[k].num_evaluations >= 0;
    if (written && all_finite(out, 7)) std::memcpy(poses + 7 * k, out, sizeof(double) * 7);
    else summaries[k].termination = CLC_FAILURE;
    if (!written) summaries[k].num_evaluations = 0;
  }
  return CLC_OK;
}

// Consensus scores on SHARED observations: every one of n_poses candidate poses judged against every block of the ONE problem the
// handle holds as a batch of one — per (pose k, block b) the sum of squared residuals, the robust cost and the number of records within
// tau of their plane.  One launch of block_scores_kernel (clc_consensus.hpp): a workgroup per pose on problem 0's lane layout and the
// lane -> block map clc_solve_subsets uses (built here when the offsets are new, kept for both).  Nothing of the layout or the stored
// observations is written.  The tables are staged in h_flow (pinned, device-mapped: the per-call output area of the batched analysis
// calls), the poses in the multi-start staging array.
int clc_score_blocks(clc_handle* h, const clc_options* opt_in, size_t n_blocks, const int64_t* block_offsets, size_t n_poses,
                     const double* poses, double tau, double* ssq, double* cost, int32_t* inliers) {
  if (!h || !block_offsets || !poses || n_blocks == 0 || n_poses == 0 || tau != tau)
    return fail(CLC_ERR_INVALID_ARG, "clc_score_blocks: bad argument");
  CLC_TRY(require_batch_of_one("clc_score_blocks", h));
  if (n_poses > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, "clc_score_blocks: too many poses");
  CLC_TRY(check_block_offsets("clc_score_blocks", h, n_blocks, block_offsets));
  // the options as clc_solve_batched checks them; a non-finite pose is not an error here: its row reports NaN / NaN / 0
  BatchedCall c;
  CLC_TRY(begin_batched_call("clc_score_blocks", h, opt_in, poses, 0, &c));
  const clc_options& opt = c.opt;
  CLC_TRY(require_resident("clc_score_blocks", c.bl, "score the poses one by one with clc_factor_evaluate"));
  CLC_TRY(ensure_lane_block_map("clc_score_blocks", h, n_blocks, block_offsets));
  const size_t cells = n_poses * n_blocks;
  CLC_HIP(h->h_ms_poses.grow(7 * n_poses));
  CLC_HIP(h->h_flow.grow(2 * cells + (cells + 1) / 2));  // [ssq | cost | inliers (int32)]
  // (the previous call ended with a stream synchronisation: nothing still reads or writes the staging buffers)
  std::memcpy(h->h_ms_poses, poses, sizeof(double) * 7 * n_poses);
  double* const d_ssq = h->h_flow.dev();
  double* const d_cost = d_ssq + cells;
  int32_t* const d_inl = reinterpret_cast<int32_t*>(d_cost + cells);
  const auto launch = [&](auto NL) {
    hipLaunchKernelGGL(clc::block_scores_kernel<NL>, dim3((unsigned)n_poses), dim3(NL), 0, h->stream, h->bres.d_xy,
                       h->bres.with_z ? h->bres.d_z.get() : nullptr, h->bres.d_desc, h->batch.d_groups, h->d_sub_lane_block, h->bres.max_ppl,
                       (int)n_blocks, h->h_ms_poses.dev(), opt.loss_scale_factor, opt.use_loss != 0 ? 1 : 0, tau, ssq ? d_ssq : nullptr,
                       cost ? d_cost : nullptr, inliers ? d_inl : nullptr);
  };
  if (h->bres.lanes == 256) launch(cint<256>); else launch(cint<512>);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipStreamSynchronize(h->stream));  // (kernel completion makes the tables written over PCIe visible)
  const double* const o_ssq = h->h_flow;
  if (ssq) std::memcpy(ssq, o_ssq, sizeof(double) * cells);
  if (cost) std::memcpy(cost, o_ssq + cells, sizeof(double) * cells);
  if (inliers) std::memcpy(inliers, o_ssq + 2 * cells, sizeof(int32_t) * cells);
  return CLC_OK;
}

}  // extern "C"

#ifdef CLC_TEST_HOOKS
// Test hook: how many lane -> block maps this process has built (clc_solve_subsets and clc_score_blocks share one per offsets and upload).
#pragma GCC visibility push(default)
extern "C" int clc_debug_lane_map_builds(long long* count) {
  if (!count) return fail(CLC_ERR_INVALID_ARG, "clc_debug_lane_map_builds: NULL count");
  *count = g_lane_map_builds.load(std::memory_order_relaxed);
  return CLC_OK;
}
#pragma GCC visibility pop
#endif

#if defined(CLC_STAMPS) && defined(CLC_TEST_HOOKS)
// Debug build only (scripts/*_stamps.py): copy the stamp buffers of THIS unit's kernels out (and clear them).
#pragma GCC visibility push(default)
extern "C" int clc_debug_res_stamps(void* dst, size_t bytes) {
  if (bytes > sizeof(clc::clc_res_stamp_buf)) bytes = sizeof(clc::clc_res_stamp_buf);
  if (hipDeviceSynchronize() != hipSuccess) return CLC_ERR_HIP;
  if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(clc::clc_res_stamp_buf), bytes) != hipSuccess) return CLC_ERR_HIP;
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(clc::clc_res_stamp_buf)) != hipSuccess) return CLC_ERR_HIP;
  return hipMemset(p, 0, sizeof(clc::clc_res_stamp_buf)) == hipSuccess ? CLC_OK : CLC_ERR_HIP;
}
extern "C" int clc_debug_res_ctrl_stamps(void* dst, size_t bytes) {
  if (bytes > sizeof(clc::clc_res_stamp_ctrl)) bytes = sizeof(clc::clc_res_stamp_ctrl);
  if (hipDeviceSynchronize() != hipSuccess) return CLC_ERR_HIP;
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(clc::clc_res_stamp_ctrl), bytes) == hipSuccess ? CLC_OK : CLC_ERR_HIP;
}
#pragma GCC visibility pop
#endif
