// abi_staging.hpp — the device memory of ONE call of the C-ABI: the uploads of its host arrays, its scratch, and the copies back
// (abi_camcal.hip, abi_guidance.hip, the assemble and sweep forms of abi_frontend.hip; abi_campose.hip through abi_lift.hpp; the units
// of the joint problems through abi_jointcall.hpp; those of the image front end, abi_subpix.hip, abi_chess.hip and abi_tags.hip,
// through abi_imagecall.hpp).  Host code only: _build.csrc_sha16() does not cover this file.
//
// A host-array form is: checks, one in / out / inout line per array, the pair's device-side function, finish().  The _device form is:
// checks, the same function, finish().  That function takes device pointers and takes its scratch from the Staging it is given, so
// scratch outlives every enqueue until finish()'s synchronise; a nullable array is decided on its one line (the `_opt` variants hand
// back nullptr and record nothing).
#pragma once
#include "clc_abi_internal.hpp"

#include <chrono>
#include <memory>
#include <vector>

namespace clc_abi {

class Staging {
 public:
  explicit Staging(clc_handle* h) : h_(h) {}
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  ~Staging() {
    for (const DevPool::Block& b : blocks_) h_->pool.release(b.p, b.cap);
  }

  // A pool block of its own for `count` elements (one of at least one element even at count == 0: the kernels get non-null
  // pointers for empty required arrays) that lives until this object dies.  nullptr once an error is held.
  template <class T>
  T* scratch(size_t count) {
    if (err_ != hipSuccess) return nullptr;
    DevPool::Block b{nullptr, 0};
    err_ = h_->pool.acquire(std::max<size_t>(count, 1) * sizeof(T), &b.p, &b.cap);
    if (err_ != hipSuccess) return nullptr;
    blocks_.push_back(b);
    return static_cast<T*>(b.p);
  }
  // host[count] up (nothing is copied at count == 0, and host is not read).
  template <class T>
  T* in(const T* host, size_t count) {
    T* d = scratch<T>(count);
    if (d && count > 0) err_ = hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, h_->stream);
    return d;
  }
  // The same for a small array that the call builds inside a helper: this object keeps the vector until it dies, so the copy's source
  // outlives finish()'s synchronise whatever scope built it.
  template <class T>
  const T* in_owned(std::vector<T> host) {
    auto kept = std::make_shared<const std::vector<T>>(std::move(host));
    owned_.push_back(kept);
    return in(kept->data(), kept->size());
  }
  // A block whose first `count` elements finish() copies to host.
  template <class T>
  T* out(T* host, size_t count) {
    T* d = scratch<T>(count);
    if (d && count > 0) back_.push_back({host, d, count * sizeof(T)});
    return d;
  }
  // Both; `from`: what goes up where that is not host itself.
  template <class T>
  T* inout(T* host, size_t count, const T* from = nullptr) {
    T* d = out(host, count);
    if (d && count > 0) err_ = hipMemcpyAsync(d, from ? from : host, count * sizeof(T), hipMemcpyHostToDevice, h_->stream);
    return d;
  }
  // The same for an array the caller may leave out: host == NULL takes no block and gives nullptr.
  template <class T>
  T* in_opt(const T* host, size_t count) { return host ? in(host, count) : nullptr; }
  template <class T>
  T* out_opt(T* host, size_t count) { return host ? out(host, count) : nullptr; }

  // The first HIP error of this call (an allocation, a copy, or a launch handed to launched()): checked before the first launch and
  // by finish().  After an error every in / out / scratch gives nullptr: nothing may be launched on them.
  bool ok() const { return err_ == hipSuccess; }
  void check(hipError_t e) {
    if (err_ == hipSuccess) err_ = e;
  }
  void launched() { check(hipGetLastError()); }
  // CLC_OK, or the held error reported (no synchronise): for a call that reads something back and waits ahead of its finish()
  int status(const char* who) const { return err_ == hipSuccess ? CLC_OK : fail(CLC_ERR_HIP, who, err_); }
  // The recorded copies back, then the call's ONE synchronise.  Nothing is enqueued or waited for once an error is held.
  int finish(const char* who) {
    for (const Back& b : back_)
      if (err_ == hipSuccess) err_ = hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, h_->stream);
    if (err_ == hipSuccess) err_ = hipStreamSynchronize(h_->stream);
    return status(who);
  }

  hipStream_t stream() const { return h_->stream; }

 private:
  struct Back { void* host; const void* dev; size_t bytes; };
  clc_handle* h_;
  hipError_t err_ = hipSuccess;
  std::vector<DevPool::Block> blocks_;
  std::vector<Back> back_;
  std::vector<std::shared_ptr<const void>> owned_;
};

using Clock = std::chrono::steady_clock;

// The wall time since t0 into solve_ms of n summaries (host memory; nullptr: none were asked for).
inline void stamp_solve_ms(clc_summary* summaries, size_t n, Clock::time_point t0) {
  if (!summaries) return;
  const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
  for (size_t k = 0; k < n; ++k) summaries[k].solve_ms = ms;
}

}  // namespace clc_abi
