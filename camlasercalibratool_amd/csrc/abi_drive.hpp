// abi_drive.hpp — host-side pieces of the solve drivers (abi_solve.hip, abi_batched.hip): run-time flags to template arguments,
// and the launch-ahead loop on the pinned mailbox.  Host code only (no kernel is defined or changed here): _build.csrc_sha16(),
// the identity of what the kernels are built from, does not cover this file.
#pragma once
#include "clc_abi_internal.hpp"

#include <string>
#include <type_traits>

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

}  // namespace clc_abi
