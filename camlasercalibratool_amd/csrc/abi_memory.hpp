// abi_memory.hpp — the owners of the C-ABI's host-side memory (no kernels): the per-call device pool, typed owning arrays for the
// handle's and the communicator's device / page-locked buffers, and owners of their streams and events.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace clc_abi {

// Temporaries of one call come from a per-handle pool of device blocks: hipMalloc / hipFree of tens of megabytes cost
// milliseconds each with the system runtime (and hipFree synchronises the device), which made a 0.7 ms
// clc_select_observations take 20 ms when called from a plain C++ program.  A block goes back to the pool on scope
// exit and is handed out again (best fit) to later calls; blocks beyond 1 GiB are really freed.  Every entry point
// synchronises its stream before it returns, so a recycled block is never still in use.
struct DevPool {
  struct Block { void* p; size_t cap; };
  std::vector<Block> free_blocks;
  static constexpr size_t kKeepLimit = (size_t)1 << 30;
  DevPool() = default;
  DevPool(const DevPool&) = delete;
  DevPool& operator=(const DevPool&) = delete;
  ~DevPool() { clear(); }
  hipError_t acquire(size_t bytes, void** out, size_t* cap) {
    bytes = std::max<size_t>(bytes, 256);
    int best = -1;
    for (int i = 0; i < (int)free_blocks.size(); ++i)
      if (free_blocks[(size_t)i].cap >= bytes && (best < 0 || free_blocks[(size_t)i].cap < free_blocks[(size_t)best].cap)) best = i;
    if (best >= 0 && free_blocks[(size_t)best].cap <= 4 * bytes + ((size_t)1 << 20)) {
      *out = free_blocks[(size_t)best].p;
      *cap = free_blocks[(size_t)best].cap;
      free_blocks.erase(free_blocks.begin() + best);
      return hipSuccess;
    }
    *cap = bytes;
    return hipMalloc(out, bytes);
  }
  void release(void* p, size_t cap) {
    if (!p) return;
    if (cap > kKeepLimit || free_blocks.size() >= 64) { (void)hipFree(p); return; }
    free_blocks.push_back({p, cap});
  }
  void clear() {
    for (const Block& b : free_blocks) (void)hipFree(b.p);
    free_blocks.clear();
  }
};

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap_bytes = 0;
  DevPool* pool;
  explicit DevBuf(DevPool* pl) : pool(pl) {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) pool->release(p, cap_bytes); }
  hipError_t alloc(size_t count) {
    if (p) { pool->release(p, cap_bytes); p = nullptr; }
    return pool->acquire(std::max<size_t>(count, 1) * sizeof(T), reinterpret_cast<void**>(&p), &cap_bytes);
  }
};

// Where an OwnedArray lives: device memory, or page-locked host memory with the given hipHostMalloc flags (mapped: the array also
// has a device address, dev()).
struct DeviceMemory {
  static constexpr bool kMapped = false;
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void* p) { return hipFree(p); }
};
template <unsigned Flags>
struct PinnedMemory {
  static constexpr bool kMapped = (Flags & hipHostMallocMapped) != 0;
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
  static hipError_t free(void* p) { return hipHostFree(p); }
};

// A typed, move-only array that owns its block; it converts to T* (nullptr while empty).  grow(count): nothing when `count` elements
// fit already; otherwise the old block is freed FIRST (no doubled peak at layouts of 1e8-1e9 bytes) and a block of exactly `count`
// elements is allocated.  On any failure the array is left empty, never dangling.  The contents do not survive a grow.
template <class T, class Memory>
class OwnedArray {
 public:
  OwnedArray() = default;
  OwnedArray(OwnedArray&& o) noexcept { swap(o); }
  OwnedArray& operator=(OwnedArray&& o) noexcept { swap(o); return *this; }
  ~OwnedArray() { (void)reset(); }

  hipError_t grow(size_t count) {
    if (count <= n_) return hipSuccess;
    hipError_t e = reset();
    T* p = nullptr;
    if (e == hipSuccess) e = Memory::alloc(reinterpret_cast<void**>(&p), count * sizeof(T));
    if (e != hipSuccess) return e;
    p_ = p;
    n_ = count;
    if constexpr (Memory::kMapped) {
      e = hipHostGetDevicePointer(reinterpret_cast<void**>(&d_), p, 0);
      if (e != hipSuccess) (void)reset();
    }
    return e;
  }
  // frees the block now (the array is empty afterwards, whatever the free returned)
  hipError_t reset() {
    T* p = p_;
    p_ = d_ = nullptr;
    n_ = 0;
    return p ? Memory::free(p) : hipSuccess;
  }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }
  T* dev() const {
    static_assert(Memory::kMapped, "dev(): only mapped page-locked arrays have a device address");
    return d_;
  }
  size_t size() const { return n_; }

 private:
  void swap(OwnedArray& o) noexcept { std::swap(p_, o.p_); std::swap(d_, o.d_); std::swap(n_, o.n_); }
  T* p_ = nullptr;
  T* d_ = nullptr;  // mapped arrays: the device address of p_
  size_t n_ = 0;
};

template <class T>
using DeviceArray = OwnedArray<T, DeviceMemory>;
template <class T, unsigned Flags = hipHostMallocDefault>
using PinnedArray = OwnedArray<T, PinnedMemory<Flags>>;
template <class T>
using MappedArray = PinnedArray<T, hipHostMallocMapped>;

// A move-only owner of a stream or an event: create through out(), destroyed with the owner.
template <class H, hipError_t (*Destroy)(H)>
class HipObject {
 public:
  HipObject() = default;
  HipObject(HipObject&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  HipObject& operator=(HipObject&& o) noexcept { std::swap(h_, o.h_); return *this; }
  ~HipObject() { if (h_) (void)Destroy(h_); }
  H* out() {  // for the create call
    if (h_) (void)Destroy(std::exchange(h_, nullptr));
    return &h_;
  }
  operator H() const { return h_; }

 private:
  H h_ = nullptr;
};
using Stream = HipObject<hipStream_t, hipStreamDestroy>;
using Event = HipObject<hipEvent_t, hipEventDestroy>;

}  // namespace clc_abi
