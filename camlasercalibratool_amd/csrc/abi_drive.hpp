// abi_drive.hpp — host-side pieces the units of the C-ABI share: run-time flags to template arguments, the launch-ahead loop on
// the pinned mailbox (abi_solve.hip, abi_batched.hip), the one launcher of the batched resident kernel (abi_batched.hip, abi_comm.hip),
// and the checks of options, host CSR offsets and problem offsets (abi_frontend.hip, abi_campose.hip, abi_joint.hip, abi_camcal.hip,
// abi_guidance.hip).  The device memory of one call — uploads, scratch, copies back — is abi_staging.hpp's.  Host code only (no kernel
// is defined or changed here): _build.csrc_sha16(), the identity of what the kernels are built from, does not cover this file.
#pragma once
#include "clc_abi_internal.hpp"

#include <string>
#include <type_traits>
#include <vector>

namespace clc_abi {

template <int V>
constexpr std::integral_constant<int, V> cint{};

// with_flags(f, a, b, ...) calls f(A, B, ...): a bool argument arrives as std::true_type / std::false_type, an
// std::integral_constant as itself.  The callee uses them as template arguments, so a kernel's argument list is written once, and
// only the combinations a call names are instantiated (a constant where a choice has one value).
template <class F>
void with_flags(F&& f) { f(); }
template <class F, class T, T V, class... R>
void with_flags(F&& f, std::integral_constant<T, V> c, R... r) {
  with_flags([&](auto... t) { f(c, t...); }, r...);
}
template <class F, class... R>
void with_flags(F&& f, bool b, R... r) {
  if (b) with_flags([&](auto... t) { f(std::true_type{}, t...); }, r...);
  else with_flags([&](auto... t) { f(std::false_type{}, t...); }, r...);
}

// Launch-ahead loop of the solves whose LM passes are separate launches (clc_solve's step chain and [eval, lm] pair,
// clc_solve_batched's lockstep launches): the host keeps launches queued beyond the last pass the device has reported consumed
// (pinned HostMailbox), so the stream never drains and the host never blocks; the launches still queued at termination turn
// into no-ops.  What differs between the loops is a value here.
struct LaunchAhead {
  const char* who;  // prefix of the error texts
  int cap;          // launches at most
  int depth;        // launch k is made while k - (passes consumed) < depth
  // every launch made, the stream drained and no final status: kFail an error; kFailOnceConsumed the same once the device has
  // also counted every launch consumed; kReturn: the loop ends normally once every launch is consumed (the caller finishes)
  enum { kFail, kFailOnceConsumed, kReturn } at_cap;
  double stall_s;   // no progress from the device for this long: an error
};

// launch(k) makes launch k and returns CLC_OK or the error it set; *launched receives the number of launches made.
template <class Launch>
int launch_ahead(clc::HostMailbox* mb, hipStream_t stream, const LaunchAhead& p, Launch&& launch, int* launched) {
  mb->n_done = 0;
  mb->status = CLC_RUNNING;
  std::atomic_thread_fence(std::memory_order_seq_cst);
  int& n = *launched;
  n = 0;
  int last_done = 0;
  long long spins = 0;
  auto t_last_progress = std::chrono::steady_clock::now();
  for (;;) {
    if (__atomic_load_n(&mb->status, __ATOMIC_ACQUIRE) != CLC_RUNNING) return CLC_OK;
    // passes consumed = launches whose rows are used up.  Clamped to what this solve has launched: the early progress store of
    // the PREVIOUS solve's last launches is relaxed and may land after the reset above.
    const int done = std::min(__atomic_load_n(&mb->n_done, __ATOMIC_ACQUIRE), n);
    if (n < p.cap && n - done < p.depth) {
      const int rc = launch(n);
      if (rc != CLC_OK) return rc;
      ++n;
      continue;
    }
    if (p.at_cap == LaunchAhead::kReturn && n >= p.cap && done >= n) return CLC_OK;
    // nothing to launch: wait for the device (bounded: a wedged queue must not hang the caller)
    if (done != last_done) { last_done = done; t_last_progress = std::chrono::steady_clock::now(); spins = 0; }
    if ((++spins & 0xFFFF) == 0) {
      const hipError_t e = hipStreamQuery(stream);
      if (e != hipSuccess && e != hipErrorNotReady) return fail(CLC_ERR_HIP, (std::string(p.who) + ": stream error").c_str(), e);
      if (e == hipSuccess) {  // queue drained: the mailbox must be final now
        if (__atomic_load_n(&mb->status, __ATOMIC_ACQUIRE) != CLC_RUNNING) return CLC_OK;
        if (p.at_cap != LaunchAhead::kReturn && n >= p.cap &&
            (p.at_cap == LaunchAhead::kFail || __atomic_load_n(&mb->n_done, __ATOMIC_ACQUIRE) >= n))
          return fail(CLC_ERR_HIP, (std::string(p.who) + ": controller did not terminate").c_str());
      }
      const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_last_progress).count();
      if (waited > p.stall_s)
        return fail(CLC_ERR_HIP, (std::string(p.who) + ": no progress from the device for " + std::to_string((int)p.stall_s) + " s").c_str());
    }
  }
}

// as CLC_HIP, for the calls that return CLC_OK or an error already set (fail)
#define CLC_TRY(expr)                      \
  do {                                     \
    const int rc_ = (expr);                \
    if (rc_ != CLC_OK) return rc_;         \
  } while (0)

// ---- abi_batched.hip ----
// The launch plan of the handle's batch under its flags (plan_batched), the partial rows grown to it.
int batched_launch_setup(clc_handle* h, BatchedLaunch* bl);

// ONE launch of resident_solve_kernel on the handle's lane layout (bl.resident), on the handle's stream: what it works on.  Every
// batched launch of that kernel is made by launch_resident (clc_solve_batched, clc_solve_multistart, clc_solve_subsets, the
// communicator's step) — it supersedes launch_resident_batch / MultiStartLaunch, which clc_abi_internal.hpp still declares (that
// header is part of csrc_sha16: the declarations, defined nowhere, go with the next change that re-measures the kernels).
struct ResidentLaunch {
  size_t workgroups = 0;       // one per problem of the batch; or one per start / subset, every one of them on problem 0's layout
  double* d_poses = nullptr;   // start poses in, results out
  int uni_ppl = -1;            // resident_solve_kernel's: the batch's (h->bres.uni_ppl), or <= -2: every workgroup on problem 0
  // outcomes into d_poses / d_summaries / d_results; d_summaries == nullptr: the records-only form (clc_solve_batched_gather) —
  // d_results / rec_host = the communicator's gather buffer and its pinned host twin ([totals record][gathered array]), this rank's
  // segment seg_off doubles into the array, global index rec_base + k, goal = the totals' arrival count at the end of this launch
  // (batched_write_record, clc_kernels.hpp)
  clc_summary* d_summaries = nullptr;
  double* d_results = nullptr;
  double rec_base = 0.0;
  double* rec_host = nullptr;
  long long seg_off = 0;
  unsigned long long goal = 0;
  // d_weights != nullptr: the weighted form (clc_solve_subsets; on problem 0 only) — the lane -> block map, the number of blocks, the
  // weight rows [workgroups * n_blocks]
  const unsigned int* d_lane_block = nullptr;
  int n_blocks = 0;
  uint8_t* d_weights = nullptr;

  // a workgroup per uploaded problem, start poses in the handle's pinned buffer / n workgroups on problem 0, each from its own pose
  static ResidentLaunch whole_batch(const clc_handle* h) { return {h->n_problems, h->h_poses.dev(), h->bres.uni_ppl}; }
  static ResidentLaunch on_problem0(const clc_handle* h, size_t n, double* d_poses) { return {n, d_poses, -2 - h->bres.max_ppl}; }
};
void launch_resident(clc_handle* h, const clc_options& opt, const BatchedLaunch& bl, const ResidentLaunch& w);

// ---- the front end's argument checks (abi_frontend.hip, abi_campose.hip) ----
// CSR offsets [n + 1] given on the host: checked in the order every caller reports — (first_nonneg) offsets[0] >= 0, then scan by
// scan: not decreasing, and (span_unit != nullptr) fewer than 2^31 of them in the scan — and rebased: rel[k] = offsets[k] - offsets[0],
// *total = rel[n].  n == 0: offsets is not read (rel = {0}).  CLC_OK or the error set, its text beginning with `who`.
inline int host_offsets(const char* who, const int64_t* offsets, size_t n, bool first_nonneg, const char* span_unit,
                        std::vector<long long>* rel, size_t* total) {
  const std::string w(who);
  if (n > 0 && first_nonneg && offsets[0] < 0) return fail(CLC_ERR_INVALID_ARG, (w + ": negative offset").c_str());
  for (size_t k = 0; k < n; ++k) {
    if (offsets[k + 1] < offsets[k]) return fail(CLC_ERR_INVALID_ARG, (w + ": offsets not monotone").c_str());
    if (span_unit && offsets[k + 1] - offsets[k] > 0x7FFFFFFF)
      return fail(CLC_ERR_INVALID_ARG, (w + ": a scan has 2^31 " + span_unit + " or more").c_str());
  }
  rel->assign(n + 1, 0);  // (after the checks: n itself may be what is wrong)
  for (size_t k = 1; k <= n; ++k) (*rel)[k] = offsets[k] - offsets[0];
  *total = (size_t)rel->back();
  return CLC_OK;
}

// The corner range of a _device call (abi_campose.hip, abi_subpix.hip): the two ends of its offsets [n + 1] in device memory (a small
// read and a synchronise ahead of the call's enqueue).  The offsets in between are not validated.
inline int device_offset_ends(clc_handle* h, const char* who, const int64_t* offsets_dev, size_t n, long long ends[2]) {
  static_assert(sizeof(long long) == sizeof(int64_t), "offset type");
  CLC_HIP(hipMemcpyAsync(&ends[0], offsets_dev, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipMemcpyAsync(&ends[1], offsets_dev + n, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  CLC_HIP(hipStreamSynchronize(h->stream));
  if (ends[1] < ends[0] || ends[0] < 0) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": offsets not monotone").c_str());
  return CLC_OK;
}

// The counts and the problem offsets of the calls over problems of images (abi_joint.hip, abi_camcal.hip): what both forms of a
// pair refuse alike, then (host form) the offsets [n_problems + 1] themselves, NULL being one problem over every image.
inline int problem_count_checks(const char* who, size_t n_images, bool has_problem_offsets, size_t n_problems) {
  const std::string w(who);
  if (n_images > 0x7FFFFFFFull || n_problems > 0x7FFFFFFFull) return fail(CLC_ERR_INVALID_ARG, (w + ": too many images").c_str());
  if (!has_problem_offsets && n_problems > 1) return fail(CLC_ERR_INVALID_ARG, (w + ": bad argument").c_str());
  return CLC_OK;
}
inline int host_problem_offsets(const char* who, const int64_t* problem_offsets, size_t n_problems, size_t n_images) {
  if (!problem_offsets) return CLC_OK;
  std::vector<long long> rel;
  size_t span = 0;
  CLC_TRY(host_offsets(who, problem_offsets, n_problems, true, nullptr, &rel, &span));
  if (n_problems > 0 && (size_t)problem_offsets[n_problems] > n_images)
    return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": problem_offsets beyond n_images").c_str());
  return CLC_OK;
}

// The options of a line fit / of a board-pose refinement: the caller's, or the call's defaults; checked.
inline int line_options(const clc_options* in, clc_options* o, const char* who) {
  if (in) *o = *in; else clc_line_options_default(o);
  if (o->max_num_iterations < 0) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": max_num_iterations < 0").c_str());
  if (o->use_loss && !(o->loss_scale_factor > 0.0))
    return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": loss_scale_factor must be > 0").c_str());
  return CLC_OK;
}
inline int pose_options(const clc_options* in, clc_options* o, const char* who) {
  if (in) *o = *in; else clc_pose_options_default(o);
  if (o->max_num_iterations < 0) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": max_num_iterations < 0").c_str());
  if (o->use_loss) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": the pose refinement has no loss (use_loss must be 0)").c_str());
  return CLC_OK;
}
inline bool known_model(int32_t model) { return model == CLC_CAMERA_PINHOLE || model == CLC_CAMERA_KANNALA_BRANDT; }
// A camera the lift and the projection can use: a known model, finite parameters, focal lengths not 0.
inline int camera_check(const clc_camera* c, const char* who) {
  if (!c || !known_model(c->model)) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": unknown camera model").c_str());
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(c->proj[i]) || !std::isfinite(c->dist[i]))
      return fail(CLC_ERR_NONFINITE, (std::string(who) + ": non-finite camera parameter").c_str());
  if (c->proj[0] == 0.0 || c->proj[1] == 0.0) return fail(CLC_ERR_INVALID_ARG, (std::string(who) + ": zero focal length").c_str());
  return CLC_OK;
}

}  // namespace clc_abi
