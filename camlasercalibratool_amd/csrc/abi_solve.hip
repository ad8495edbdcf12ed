// abi_solve.hip — clc_eval and clc_solve: the launch sequences of one problem (step-kernel chain, single-workgroup resident kernel, cooperative kernel).
// (one of the translation units of the C-ABI; see clc_abi_internal.hpp)
#include "abi_drive.hpp"

using namespace clc_abi;

namespace {

template <bool WITH_LOSS, bool WITH_JAC>
void launch_eval_v(clc_handle* h, const StreamPlan& sp, const double* d_pose, const int32_t* d_status, double lf,
                   const clc::Pose7& pose_arg, int use_pose_arg) {
  const int grid = sp.grid, fl = h->launch_flags;
  const bool big = sp.threads == 512;
  if (sp.rows()) {  // row layout: the Jacobian comes with the moments, a cost-only pass would save nothing
    // rows in flight per wave: 8 while the array is served by the Infinity Cache, 12 (206 VGPRs, still 2 waves/SIMD) when it
    // streams from HBM with non-temporal loads — throughput there tracks the bytes in flight per CU (profiles/r03_occupancy.md:
    // 4 rows 0.40 of peak, 8 rows 0.81, 12 rows 0.82-0.83, 16 rows 0.81; 3 waves/SIMD cannot hold more than 6 rows each: 0.80);
    // rows that carry z keep 8.  BIG: 512-thread workgroups; EQ: equal wave shares (the unweighted form)
    const auto launch = [&](auto BIG, auto EQ, auto NT, auto Z) {
      constexpr int BT = BIG ? 512 : 256;
      hipLaunchKernelGGL((clc::eval_rows_kernel<WITH_LOSS, NT, BT, !EQ, (NT && !Z) ? 12 : clc::ROWS_DEPTH, Z>), dim3(grid), dim3(BT), 0,
                         h->stream, h->obs.d_rxy, h->obs.d_rdesc(), h->obs.n_rows, d_pose, d_status, lf, fl,
                         h->d_partials, pose_arg, use_pose_arg);
    };
    if (sp.eval_equal) ensure_wave_split(h, grid);
    if (sp.layout == Layout::rows_z) with_flags(launch, big, std::false_type{}, sp.nt, std::true_type{});
    else if (big) with_flags(launch, std::true_type{}, sp.eval_equal, sp.nt, std::false_type{});
    else with_flags(launch, std::false_type{}, std::false_type{}, sp.nt, std::false_type{});
    return;
  }
  const auto launch = [&](auto CP, auto BIG, auto PF, auto NT) {
    constexpr int BT = BIG ? 512 : 256;
    hipLaunchKernelGGL((clc::eval_kernel<WITH_LOSS, WITH_JAC, PF, NT, CP, BT>), dim3(grid), dim3(BT), 0, h->stream,
                       CP ? h->obs.d_ctiles : h->obs.d_tiles, h->obs.d_groups, (long long)h->n_obs, d_pose, d_status, lf, fl, h->d_partials, pose_arg,
                       use_pose_arg);
  };
  if (sp.layout == Layout::compact) with_flags(launch, std::true_type{}, big, sp.prefetch, sp.nt);
  else if (big) with_flags(launch, std::false_type{}, std::true_type{}, std::true_type{}, sp.nt);
  else with_flags(launch, std::false_type{}, std::false_type{}, sp.prefetch, sp.nt);
}

template <bool WITH_JAC>
void launch_eval(clc_handle* h, const StreamPlan& sp, bool with_loss, const double* d_pose,
                 const int32_t* d_status, double lf, const clc::Pose7* pose_arg = nullptr) {
  const clc::Pose7 zero = {};
  const clc::Pose7& pa = pose_arg ? *pose_arg : zero;
  if (with_loss) launch_eval_v<true, WITH_JAC>(h, sp, d_pose, d_status, lf, pa, pose_arg ? 1 : 0);
  else launch_eval_v<false, WITH_JAC>(h, sp, d_pose, d_status, lf, pa, pose_arg ? 1 : 0);
}

}  // namespace

namespace clc_abi {
void warm_solve() {
  warm_kernel(reinterpret_cast<const void*>(&clc::resident_solve_kernel<true, false, 8, kResPR512, kResPL512, 0>));
  warm_kernel(reinterpret_cast<const void*>(&clc::coop_solve_kernel<true, false>));
}

void launch_eval(clc_handle* h, const StreamPlan& sp, bool with_jac, bool with_loss, const double* d_pose, const int32_t* d_status, double lf,
                 const clc::Pose7* pose_arg) {
  if (with_jac) ::launch_eval<true>(h, sp, with_loss, d_pose, d_status, lf, pose_arg);
  else ::launch_eval<false>(h, sp, with_loss, d_pose, d_status, lf, pose_arg);
}
}  // namespace clc_abi

extern "C" {

size_t clc_num_observations(const clc_handle* h) { return h ? h->n_obs : 0; }

int clc_eval(clc_handle* h, const double pose[7], int with_loss, double loss_scale_factor,
             double* cost, double g[6], double H[21]) {
  if (!h || !pose || !cost) return fail(CLC_ERR_INVALID_ARG, "clc_eval: bad argument");
  if (!h->obs.d_tiles) return fail(CLC_ERR_NO_DATA, "clc_eval: no observations uploaded");
  if (!all_finite(pose, 7)) return fail(CLC_ERR_NONFINITE, "clc_eval: non-finite pose");
  if (with_loss && !(loss_scale_factor > 0.0)) return fail(CLC_ERR_INVALID_ARG, "clc_eval: loss_scale_factor must be > 0");
  CLC_HIP(hipSetDevice(h->device));
  const StreamPlan sp = stream_plan(h);
  int rc = ensure_partials(h, sp.grid);
  if (rc != CLC_OK) return rc;
  std::memcpy(h->h_small, pose, 7 * sizeof(double));
  CLC_HIP(hipMemcpyAsync(h->d_small, h->h_small, 7 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const bool want_jac = (g != nullptr) || (H != nullptr);
  if (want_jac)
    launch_eval<true>(h, sp, with_loss != 0, h->d_small, nullptr, loss_scale_factor);
  else
    launch_eval<false>(h, sp, with_loss != 0, h->d_small, nullptr, loss_scale_factor);
  CLC_HIP(hipGetLastError());
  hipLaunchKernelGGL(clc::reduce_kernel, dim3(1), dim3(clc::BLOCK), 0, h->stream, h->d_partials, sp.grid,
                     with_loss, loss_scale_factor, h->d_small + 16);
  CLC_HIP(hipGetLastError());
  CLC_HIP(hipMemcpyAsync(h->h_small + 16, h->d_small + 16, clc::NACC * sizeof(double), hipMemcpyDeviceToHost,
                         h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  const double* r = h->h_small + 16;
  *cost = r[27];
  if (g) for (int i = 0; i < 6; ++i) g[i] = want_jac ? r[21 + i] : 0.0;
  if (H) for (int i = 0; i < 21; ++i) H[i] = r[i];
  return CLC_OK;
}

}  // extern "C"

namespace {

// Trace rows wanted?  Then the handle's trace buffer holds every row of the solve.
int prepare_trace(clc_handle* h, const clc_options& opt, const clc_iteration* trace, int trace_cap, bool* want_trace) {
  *want_trace = trace != nullptr && trace_cap > 0;
  return *want_trace ? ensure_trace(h, opt.max_num_iterations + 8) : CLC_OK;
}

// The end of every clc_solve path, once the stream is synchronised where the trace or the events need it: summary and pose out of
// the pinned buffers the device wrote, the trace rows, the kernel-time fields, the wall time and the finite check.
int finish_solve(clc_handle* h, const clc_summary& out, const double* out_pose, double pose[7], clc_summary* summary,
                 clc_iteration* trace, int trace_cap, double kernel_ms, int64_t kernel_launches,
                 std::chrono::steady_clock::time_point t0) {
  *summary = out;
  // A solve whose first evaluation is not finite ends CLC_FAILURE before iteration zero is recorded, and the kernels' epilogue
  // (lm_fill_summary: recorded iterations - 1) says -1 then.  clc_solve reports 0 iterations, as the oracle's restatement of Ceres does.
  if (summary->num_iterations < 0) summary->num_iterations = 0;
  for (int i = 0; i < 7; ++i) pose[i] = out_pose[i];
  if (trace != nullptr && trace_cap > 0) {
    const int n = std::min(std::min(out.num_iterations + 1, trace_cap), (int)h->d_trace.size());  // (the rows recorded: none for such a solve)
    if (n > 0) CLC_HIP(hipMemcpy(trace, h->d_trace, sizeof(clc_iteration) * (size_t)n, hipMemcpyDeviceToHost));
  }
  summary->eval_kernel_ms = kernel_ms;
  summary->eval_kernel_launches = kernel_launches;
  summary->solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (!all_finite(pose, 7)) return fail(CLC_ERR_NONFINITE, "clc_solve: non-finite result");
  return CLC_OK;
}

}  // namespace

namespace clc_abi {
// clc_solve as a chain of step_kernel launches (clc_kernels.hpp "Step kernel"): launch 0 evaluates at the initial
// pose, launch k >= 1 consumes the rows of launch k-1 in every workgroup and evaluates at the next point.  The
// host only keeps `lookahead` launches queued beyond the last pass the device reported consumed.
// win_first/win_last/win_ms (profiling hook clc_time_steps): HIP events are recorded on the stream right before launch
// `win_first` and right after launch `win_last`; *win_ms receives the elapsed time between them.
int solve_stepped(clc_handle* h, const clc_options& opt, const StreamPlan& sp, double pose[7], clc_summary* summary,
                  clc_iteration* trace, int trace_cap, std::chrono::steady_clock::time_point t0,
                  int win_first, int win_last, float* win_ms) {
  bool want_trace;
  int rc = prepare_trace(h, opt, trace, trace_cap, &want_trace);
  if (rc != CLC_OK) return rc;
  const int lookahead = opt.launch_ahead > 0 ? opt.launch_ahead : default_lookahead();
  clc::Pose7 p0;
  for (int i = 0; i < 7; ++i) p0.v[i] = pose[i];
  clc::SolveParams prm;
  std::memset(&prm, 0, sizeof(prm));
  prm.opt = opt;
  prm.pose0 = p0;
  prm.trace = want_trace ? h->d_trace : nullptr;
  prm.mailbox = h->h_mailbox.dev();
  prm.trace_cap = want_trace ? (int)h->d_trace.size() : 0;
  const int grid = sp.grid;
  if (sp.step_equal) ensure_wave_split(h, grid);
  double* rows_buf[2] = {h->d_partials, h->d_partials_b()};
  // (max_iterations + 1) evaluations + the final controller pass; launch k is made while k - (passes consumed) <= lookahead
  const LaunchAhead la = {"clc_solve", opt.max_num_iterations + 2, lookahead + 1, LaunchAhead::kFail, 30.0};
  int launched = 0;
  rc = launch_ahead(h->h_mailbox, h->stream, la, [&](const int k) -> int {
    if (win_ms && k == win_first) CLC_HIP(hipEventRecord(h->ev[0], h->stream));
    // launch k reads state[(k-1)&1] / rows[(k-1)&1] and writes state[k&1] / rows[k&1]
    const double* r_in = rows_buf[(k + 1) & 1];
    double* r_out = rows_buf[k & 1];
    // LAYOUT 0: compact tiles (NT is DEEP there), 1: rows, 2: rows that carry z; EQ: equal wave shares, the unweighted form;
    // MODE 0: launch 0, 1: launch 1, 2: the rest
    const auto launch = [&](auto LAYOUT, auto LOSS, auto EQ, auto NT, auto MODE) {
      hipLaunchKernelGGL((clc::step_kernel<LOSS, NT, MODE, LAYOUT, !EQ>), dim3(grid), dim3(512), 0, h->stream, r_in,
                         LAYOUT ? h->obs.d_rxy : h->obs.d_ctiles, LAYOUT ? reinterpret_cast<const double*>(h->obs.d_rdesc()) : h->obs.d_groups.get(), LAYOUT ? (int)h->obs.n_rows : (int)h->n_obs,
                         grid | ((k & 1) << 30), k, r_out, h->d_block, prm);
    };
    const auto at_mode = [&](auto... c) {
      if (k == 0) launch(c..., cint<0>);
      else if (k == 1) launch(c..., cint<1>);
      else launch(c..., cint<2>);
    };
    if (sp.layout == Layout::rows_z) with_flags(at_mode, cint<2>, opt.use_loss != 0, std::false_type{}, sp.nt);  // 3:2 wave shares
    else if (sp.rows()) with_flags(at_mode, cint<1>, opt.use_loss != 0, sp.step_equal, sp.nt);
    else with_flags(at_mode, cint<0>, opt.use_loss != 0, std::false_type{}, sp.deep);
    if (win_ms && k == win_last) CLC_HIP(hipEventRecord(h->ev[1], h->stream));
    return CLC_OK;
  }, &launched);
  if (rc != CLC_OK) return rc;
  CLC_HIP(hipGetLastError());
  std::atomic_thread_fence(std::memory_order_acquire);
  if (want_trace) CLC_HIP(hipStreamSynchronize(h->stream));
  rc = finish_solve(h, h->h_mailbox->summary, h->h_mailbox->pose, pose, summary, trace, trace_cap, 0.0, 0, t0);
  if (rc != CLC_OK || !win_ms) return rc;
  *win_ms = -1.f;
  if (launched > win_last && win_first >= 0) {
    CLC_HIP(hipStreamSynchronize(h->stream));
    CLC_HIP(hipEventElapsedTime(win_ms, h->ev[0], h->ev[1]));
  }
  return CLC_OK;
}
}  // namespace clc_abi

namespace {

// The whole-solve kernels raise a completion flag behind the pose (same pinned allocation) with a system-scope release after the
// outcome is written.  arm_done_flag clears it and returns its device address.
int32_t* arm_done_flag(clc_handle* h) {
  __atomic_store_n(reinterpret_cast<int32_t*>(h->h_spose + 7), 0, __ATOMIC_RELAXED);
  std::atomic_thread_fence(std::memory_order_seq_cst);
  return reinterpret_cast<int32_t*>(h->h_spose.dev() + 7);
}

// Polling the flag avoids the wake-up latency of a blocking stream synchronisation (~15 us of a ~120 us solve).  Bounded: a wedged
// queue falls through to the caller's synchronisation, which reports the error.  Returns the flag (0: not raised).
int32_t wait_done_flag(clc_handle* h) {
  const int32_t* h_done = reinterpret_cast<const int32_t*>(h->h_spose + 7);
  long long spins = 0;
  const auto t_spin = std::chrono::steady_clock::now();
  while (__atomic_load_n(h_done, __ATOMIC_ACQUIRE) == 0) {
    if ((++spins & 0xFFFF) == 0) {
      if (hipStreamQuery(h->stream) != hipErrorNotReady) break;
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_spin).count() > 30.0) break;
    }
  }
  return __atomic_load_n(h_done, __ATOMIC_ACQUIRE);
}

// A problem that fits ONE workgroup (<= 512 lanes x 22 points; the lane layout was built at upload): the whole LM solve in a
// single launch of resident_solve_kernel<8 waves> — points read from HBM once into registers + LDS, every pass, reduction and
// controller step on chip, no kernel boundary and no partial rows between LM iterations.  This is the reference's own problem
// size (main/calibr_simulation.cpp: 50 poses x ~114 points; main/calibr_offline.cpp: O(10^2) poses): 4.3 us per LM
// iteration instead of the 7.1 us of the 256-workgroup step chain, which at this size is all launch boundary, row
// exchange and controller.  One CU works, 255 idle — the problem has 5.7e3 points.
int solve_resident_single(clc_handle* h, const clc_options& opt, double pose[7], clc_summary* summary, clc_iteration* trace,
                          int trace_cap, std::chrono::steady_clock::time_point t0) {
  bool want_trace;
  int rc = prepare_trace(h, opt, trace, trace_cap, &want_trace);
  if (rc != CLC_OK) return rc;
  for (int i = 0; i < 7; ++i) h->h_spose[i] = pose[i];
  int32_t* d_done = arm_done_flag(h);
  clc_iteration* d_trace = want_trace ? h->d_trace : nullptr;
  const int d_cap = want_trace ? (int)h->d_trace.size() : 0;
  const bool uni_ctrl = h->single_uni_ctrl;  // the cooperative kernel's controller here: the bit-identity test of the two (hooks build)
  const bool timed = opt.profile_events == 2;  // an event pair around the one launch -> eval_kernel_ms, eval_kernel_launches = 1
  if (timed) {
    rc = ensure_events(h, 2);
    if (rc != CLC_OK) return rc;
    CLC_HIP(hipEventRecord(h->ev[0], h->stream));
  }
  with_flags([&](auto LOSS, auto CTRL) {
    hipLaunchKernelGGL((clc::resident_solve_kernel<LOSS, false, 8, kResPR512, kResPL512, CTRL>), dim3(1), dim3(512), 0, h->stream,
                       h->sres.d_xy, h->sres.d_row, h->sres.d_desc, h->obs.d_groups, h->sres.uni_ppl, opt, d_trace, d_cap, h->h_spose.dev(), h->d_ssummary(),
                       h->d_small, d_done, nullptr);
  }, opt.use_loss != 0, uni_ctrl);
  CLC_HIP(hipGetLastError());
  if (timed) CLC_HIP(hipEventRecord(h->ev[1], h->stream));
  if (wait_done_flag(h) == 0 || want_trace || timed) CLC_HIP(hipStreamSynchronize(h->stream));
  float kernel_ms = 0.0f;
  if (timed) CLC_HIP(hipEventElapsedTime(&kernel_ms, h->ev[0], h->ev[1]));
  return finish_solve(h, *h->h_ssummary(), h->h_spose, pose, summary, trace, trace_cap, kernel_ms, timed ? 1 : 0, t0);
}

// clc_solve as ONE launch of 256 co-resident workgroups that keep the problem on chip (clc_coop.hpp).  Returns kCoopFallback when
// the path cannot be used (device too small, or the launch timed out in its exchange): the caller runs the step chain instead.
constexpr int kCoopFallback = -1000;

// One cooperative launch at a time per device in this process.  The kernel needs a CU per workgroup; a second cooperative launch from
// another handle (another stream, another thread) interleaves its workgroups with the first one's, neither grid becomes co-resident,
// and BOTH time out at their census — round 4: two threads alternated aborts.  A solve is ~0.1 ms, so the second caller waits for the
// gate (bounded: 5 ms) rather than fall back to the slower step chain; if the wait runs out it takes the step chain without counting
// an abort.  (Other PROCESSES on the same GPU cannot be seen from here: for them the census, the abort word and the back-off remain.)
struct CoopGate {
  static constexpr int kMaxDevices = 64;
  static std::atomic<int>& slot(int device) {
    static std::atomic<int> busy[kMaxDevices];
    return busy[device >= 0 && device < kMaxDevices ? device : 0];
  }
  std::atomic<int>* held = nullptr;
  bool acquire(int device) {
    std::atomic<int>& a = slot(device);
    const auto t0 = std::chrono::steady_clock::now();
    long long spins = 0;
    for (;;) {
      int expected = 0;
      if (a.compare_exchange_weak(expected, 1, std::memory_order_acquire)) { held = &a; return true; }
      // the holder's solve is ~0.1 ms: spin briefly, then give the core away (with more solver threads than cores the spinners would
      // otherwise take the CPU the gate's holder needs to finish)
      if (++spins < 64) continue;
      std::this_thread::yield();
      if ((spins & 0xF) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 5e-3) return false;
    }
  }
  ~CoopGate() { if (held) held->store(0, std::memory_order_release); }
};

int solve_coop(clc_handle* h, const clc_options& opt, double pose[7], clc_summary* summary, clc_iteration* trace, int trace_cap,
               std::chrono::steady_clock::time_point t0) {
  if (h->coop_checked == 0) {
    // every instantiation that can be launched below must fit a CU (one workgroup each: co-residency is what makes the polling safe)
    const void* forms[] = {
        (const void*)clc::coop_solve_kernel<true, false, false, false>, (const void*)clc::coop_solve_kernel<false, false, false, false>,
        (const void*)clc::coop_solve_kernel<true, false, true, false>,  (const void*)clc::coop_solve_kernel<false, false, true, false>,
        (const void*)clc::coop_solve_kernel<true, false, false, true>,  (const void*)clc::coop_solve_kernel<false, false, false, true>,
        (const void*)clc::coop_solve_kernel<true, false, true, true>,   (const void*)clc::coop_solve_kernel<false, false, true, true>};
    bool fits = true;
    for (const void* f : forms) {
      int n = 0;
      fits = fits && hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, clc::COOP_THREADS, 0) == hipSuccess && n >= 1;
    }
    h->coop_checked = (fits && h->num_cus >= clc::COOP_SMALL_WGS) ? 1 : -1;
    (void)hipGetLastError();
  }
  if (h->coop_checked < 0) return kCoopFallback;
  if (h->num_cus < (h->cres.wgs > 0 ? h->cres.wgs : clc::COOP_WGS)) return kCoopFallback;  // one workgroup per CU, or not at all
  CoopGate gate;  // (released when this function returns: the kernel has finished, or was never launched)
  if (!gate.acquire(h->device)) { ++h->coop_gate_waits_expired; return kCoopFallback; }
  if (!h->d_board) {
    CLC_HIP(h->d_board.grow(1));
    // (ordered on the handle's stream AND waited for: the caller may switch streams, clc_set_stream, before the next solve)
    CLC_HIP(hipMemsetAsync(h->d_board, 0, sizeof(clc::CoopBoard), h->stream));
    CLC_HIP(hipStreamSynchronize(h->stream));
    h->coop_tag = 1;
#ifdef CLC_TEST_HOOKS
    {  // (tuning hook, hooks build only: first-poll offsets, clc_coop.hpp)
      unsigned long long d[2] = {0, 0};
      if (const char* e = std::getenv("CLC_COOP_D1")) d[0] = (unsigned long long)std::atoll(e);
      if (const char* e = std::getenv("CLC_COOP_D2")) d[1] = (unsigned long long)std::atoll(e);
      if (d[0] || d[1]) CLC_HIP(hipMemcpy(&h->d_board->ctl[1], d, sizeof(d), hipMemcpyHostToDevice));
    }
#endif
  }
  const unsigned int passes = (unsigned int)opt.max_num_iterations + 4u;
  if (h->coop_tag > 0xFFFFFFFFu - passes - 8u) {  // the 32-bit pass tags are used up: start over on clean boards
    CLC_HIP(hipMemsetAsync(h->d_board, 0, sizeof(clc::CoopBoard), h->stream));
    CLC_HIP(hipStreamSynchronize(h->stream));
    h->coop_tag = 1;
  }
  bool want_trace;
  int rc = prepare_trace(h, opt, trace, trace_cap, &want_trace);
  if (rc != CLC_OK) return rc;
  const bool timed = opt.profile_events == 2;  // HIP event pair around the one launch -> clc_summary.eval_kernel_ms
  if (timed) {
    rc = ensure_events(h, 2);
    if (rc != CLC_OK) return rc;
  }
  int32_t* d_done = arm_done_flag(h);
  clc::Pose7 p0;
  for (int i = 0; i < 7; ++i) p0.v[i] = pose[i];
  clc_iteration* d_trace = want_trace ? h->d_trace : nullptr;
  const int d_cap = want_trace ? (int)h->d_trace.size() : 0;
  const unsigned int tag0 = h->coop_tag;
  h->coop_tag += passes;
  const int n_wgs = h->cres.wgs > 0 ? h->cres.wgs : clc::COOP_WGS;  // COOP_WGS, or COOP_SMALL_WGS: the one-hop form
  const unsigned int wgs = (unsigned int)std::max(1, n_wgs - h->coop_test_drop);
  h->coop_test_drop = 0;
  if (timed) CLC_HIP(hipEventRecord(h->ev[0], h->stream));
  // Z: 24-byte slots (p.z != 0); ONE: the one-hop form on 32 workgroups
  with_flags([&](auto Z, auto ONE, auto LOSS) {
    hipLaunchKernelGGL((clc::coop_solve_kernel<LOSS, false, Z, ONE>), dim3(wgs), dim3(clc::COOP_THREADS), 0, h->stream, h->cres.d_xy,
                       h->cres.d_z, h->cres.d_row, h->cres.d_desc, h->obs.d_groups, h->cres.uni_ppl, opt, p0, d_trace, d_cap, h->d_board, tag0, h->h_spose.dev(),
                       h->d_ssummary(), h->d_small, d_done, n_wgs);
  }, h->cres.with_z, n_wgs == clc::COOP_SMALL_WGS, opt.use_loss != 0);
  CLC_HIP(hipGetLastError());
  if (timed) CLC_HIP(hipEventRecord(h->ev[1], h->stream));
  int32_t done = wait_done_flag(h);
  if (done != clc::COOP_DONE_OK || want_trace || timed) {
    CLC_HIP(hipStreamSynchronize(h->stream));
    done = __atomic_load_n(reinterpret_cast<const int32_t*>(h->h_spose + 7), __ATOMIC_ACQUIRE);
  }
  if (done != clc::COOP_DONE_OK) {
    // an exchange timed out (a workgroup was not resident in time): nothing was written; the path rests (see coop_backoff)
    h->coop_retry_at = h->coop_eligible + h->coop_backoff;
    h->coop_backoff = std::min<long long>(h->coop_backoff * 2, 1LL << 20);
    ++h->coop_aborts;
    return kCoopFallback;
  }
  ++h->coop_solves;
  float kernel_ms = 0.0f;
  if (timed) CLC_HIP(hipEventElapsedTime(&kernel_ms, h->ev[0], h->ev[1]));
  return finish_solve(h, *h->h_ssummary(), h->h_spose, pose, summary, trace, trace_cap, kernel_ms, timed ? 1 : 0, t0);
}

}  // namespace

extern "C" {

int clc_solve(clc_handle* h, const clc_options* opt_in, double pose[7], clc_summary* summary,
              clc_iteration* trace, int trace_cap) {
  if (!h || !pose || !summary || trace_cap < 0) return fail(CLC_ERR_INVALID_ARG, "clc_solve: bad argument");
  if (!h->obs.d_tiles) return fail(CLC_ERR_NO_DATA, "clc_solve: no observations uploaded");
  if (!all_finite(pose, 7)) return fail(CLC_ERR_NONFINITE, "clc_solve: non-finite initial pose");
  clc_options opt;
  if (opt_in) opt = *opt_in; else clc_options_default(&opt);
  if (opt.max_num_iterations < 0) return fail(CLC_ERR_INVALID_ARG, "clc_solve: max_num_iterations < 0");
  if (opt.use_loss && !(opt.loss_scale_factor > 0.0))
    return fail(CLC_ERR_INVALID_ARG, "clc_solve: loss_scale_factor must be > 0");
  CLC_HIP(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();

  // a problem one workgroup holds: the whole solve in one single-workgroup launch; a problem the 256 CUs hold together: in one
  // launch of 256 (or 32) co-resident workgroups (clc_set_small_on_coop: a problem one workgroup holds tries that first — 4.6 instead
  // of 5.3-5.9 us per pass —, with the single-workgroup kernel as the fall-back when the cooperative launch times out or rests)
  const StreamPlan sp = stream_plan(h);
  const SolvePlan route = plan_solve(h->steer, sp, h->n_obs, h->sres.ok, h->cres.ok, h->small_on_coop, h->auto_disable, opt.profile_events);
  if (route.single && !route.coop) return solve_resident_single(h, opt, pose, summary, trace, trace_cap, t0);
  if (route.coop && ++h->coop_eligible > h->coop_retry_at) {
    const int rc = solve_coop(h, opt, pose, summary, trace, trace_cap, t0);
    if (rc != kCoopFallback) return rc;
  }
  if (route.single) return solve_resident_single(h, opt, pose, summary, trace, trace_cap, t0);
  const int grid = sp.grid;
  int rc = ensure_partials(h, grid);
  if (rc != CLC_OK) return rc;
  if (route.step_chain) return solve_stepped(h, opt, sp, pose, summary, trace, trace_cap, t0);  // (profile_events 1: the launch pair)
  const int max_evals = opt.max_num_iterations + 1;
  bool want_trace;
  rc = prepare_trace(h, opt, trace, trace_cap, &want_trace);
  if (rc != CLC_OK) return rc;
  if (opt.profile_events) {
    rc = ensure_events(h, 2 * (size_t)max_evals);
    if (rc != CLC_OK) return rc;
  }
  // Launch-ahead depth: the host keeps this many LM iterations queued beyond the last one the device has reported done.
  const int lookahead = opt.launch_ahead > 0 ? opt.launch_ahead : default_lookahead();
  clc::Pose7 p0;
  for (int i = 0; i < 7; ++i) p0.v[i] = pose[i];
  const double* d_x_eval = reinterpret_cast<const double*>(
      reinterpret_cast<const char*>(h->d_state()) + offsetof(clc::LmState, x_eval));
  const int32_t* d_status = reinterpret_cast<const int32_t*>(
      reinterpret_cast<const char*>(h->d_state()) + offsetof(clc::LmState, status));
  clc_iteration* d_trace = want_trace ? h->d_trace : nullptr;
  const int d_trace_cap = want_trace ? (int)h->d_trace.size() : 0;
  const LaunchAhead la = {"clc_solve", max_evals, lookahead, LaunchAhead::kFailOnceConsumed, 30.0};
  int launched = 0;
  rc = launch_ahead(h->h_mailbox, h->stream, la, [&](const int k) -> int {
    if (opt.profile_events) CLC_HIP(hipEventRecord(h->ev[2 * k], h->stream));
    // iteration 0 carries the initial pose by value and initialises the LM state in lm_kernel
    launch_eval<true>(h, sp, opt.use_loss != 0, d_x_eval, d_status, opt.loss_scale_factor, k == 0 ? &p0 : nullptr);
    if (opt.profile_events) CLC_HIP(hipEventRecord(h->ev[2 * k + 1], h->stream));
    with_flags([&](auto FIRST) {
      hipLaunchKernelGGL(clc::lm_kernel<FIRST>, dim3(1), dim3(clc::BLOCK), 0, h->stream, h->d_partials, grid, h->d_state(), opt,
                         d_trace, d_trace_cap, h->h_mailbox.dev(), p0);
    }, k == 0);
    return CLC_OK;
  }, &launched);
  if (rc != CLC_OK) return rc;
  CLC_HIP(hipGetLastError());
  std::atomic_thread_fence(std::memory_order_acquire);
  if (want_trace || opt.profile_events) CLC_HIP(hipStreamSynchronize(h->stream));
  double kernel_ms = 0.0;
  int64_t kernel_launches = 0;
  if (opt.profile_events) {
    kernel_launches = std::min<int64_t>(h->h_mailbox->summary.num_evaluations, launched);
    for (int i = 0; i < kernel_launches; ++i) {
      float ms = 0.f;
      CLC_HIP(hipEventElapsedTime(&ms, h->ev[2 * i], h->ev[2 * i + 1]));
      kernel_ms += ms;
    }
  }
  return finish_solve(h, h->h_mailbox->summary, h->h_mailbox->pose, pose, summary, trace, trace_cap, kernel_ms, kernel_launches, t0);
}

}  // extern "C"

#if defined(CLC_STAMPS) && defined(CLC_TEST_HOOKS)
// Debug build only (scripts/*_stamps.py): copy the stamp buffers of THIS unit's kernels out (and clear them).
#pragma GCC visibility push(default)
extern "C" int clc_debug_stamps(void* dst, size_t bytes) {
  if (bytes > sizeof(clc::clc_stamp_buf)) bytes = sizeof(clc::clc_stamp_buf);
  if (hipDeviceSynchronize() != hipSuccess) return CLC_ERR_HIP;
  if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(clc::clc_stamp_buf), bytes) != hipSuccess) return CLC_ERR_HIP;
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(clc::clc_stamp_buf)) != hipSuccess) return CLC_ERR_HIP;
  return hipMemset(p, 0, sizeof(clc::clc_stamp_buf)) == hipSuccess ? CLC_OK : CLC_ERR_HIP;
}
extern "C" int clc_debug_coop_stamps(void* dst, size_t bytes) {
  if (bytes > sizeof(clc::clc_coop_stamp_buf)) bytes = sizeof(clc::clc_coop_stamp_buf);
  if (hipDeviceSynchronize() != hipSuccess) return CLC_ERR_HIP;
  if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(clc::clc_coop_stamp_buf), bytes) != hipSuccess) return CLC_ERR_HIP;
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(clc::clc_coop_stamp_buf)) != hipSuccess) return CLC_ERR_HIP;
  return hipMemset(p, 0, sizeof(clc::clc_coop_stamp_buf)) == hipSuccess ? CLC_OK : CLC_ERR_HIP;
}
extern "C" int clc_debug_lmregs_stamps(void* dst, size_t bytes) {
  if (bytes > sizeof(clc::clc_lmu_ck)) bytes = sizeof(clc::clc_lmu_ck);
  if (hipDeviceSynchronize() != hipSuccess) return CLC_ERR_HIP;
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(clc::clc_lmu_ck), bytes) == hipSuccess ? CLC_OK : CLC_ERR_HIP;
}
#pragma GCC visibility pop
#endif
