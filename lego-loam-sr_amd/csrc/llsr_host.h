// llsr_host.h — host-only resource helpers of the C-ABI layer (llsr_capi*.hip): the carver that
// sizes and places a pool's pieces with one layout function, move-only owners of device memory,
// pinned host memory, events and streams, and the build-aside step that keeps a failed reserve
// from leaving half-built state. No kernels, no device types: tests/native/host_pool_check.cpp
// compiles it for the CPU against its own definitions of the HIP calls used here.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

// (hidden: none of this is part of the library's exported set)
namespace llsr_host __attribute__((visibility("hidden"))) {

// Pieces of a pool, each padded to 256 bytes. With a null base take() only advances `off` (the
// measuring pass) and hands out null; with a base it places. A pool's layout function runs once
// each way, so the size allocated is by construction the size carved.
struct Carver {
  char* base;
  size_t off = 0;
  std::vector<std::pair<size_t, size_t>>* log = nullptr;  // (offset, bytes) of every piece, for checks
  explicit Carver(void* b = nullptr) : base(static_cast<char*>(b)) {}
  template <class T>
  void take(T*& out, size_t n) {
    out = base ? reinterpret_cast<T*>(base + off) : nullptr;
    if (log) log->emplace_back(off, n * sizeof(T));
    off += (n * sizeof(T) + 255) & ~size_t(255);
  }
};

// Move-only owner of one HIP object, released exactly once; converts to the raw handle.
template <class T, hipError_t (*Release)(T)>
class Owned {
  T v_ = nullptr;

 public:
  Owned() = default;
  explicit Owned(T v) : v_(v) {}
  Owned(Owned&& o) noexcept : v_(o.release()) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) reset(o.release());
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }
  T get() const { return v_; }
  operator T() const { return v_; }
  T release() {
    T v = v_;
    v_ = nullptr;
    return v;
  }
  void reset(T v = nullptr) {
    if (v_) (void)Release(v_);
    v_ = v;
  }
};

using DevMem = Owned<void*, hipFree>;
using PinnedMem = Owned<void*, hipHostFree>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

// Acquire into an owner; on failure the owner keeps what it held.
inline hipError_t alloc(DevMem& m, size_t bytes) {
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  if (e == hipSuccess) m.reset(p);
  return e;
}
inline hipError_t alloc(PinnedMem& m, size_t bytes) {
  void* p = nullptr;
  const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
  if (e == hipSuccess) m.reset(p);
  return e;
}
inline hipError_t create(Event& ev, unsigned flags = hipEventDefault) {
  hipEvent_t e = nullptr;
  const hipError_t rc = hipEventCreateWithFlags(&e, flags);
  if (rc == hipSuccess) ev.reset(e);
  return rc;
}
inline hipError_t create(Stream& st, unsigned flags) {
  hipStream_t s = nullptr;
  const hipError_t rc = hipStreamCreateWithFlags(&s, flags);
  if (rc == hipSuccess) st.reset(s);
  return rc;
}

// Measure, allocate (plus `slack` bytes past the last piece), place: layout(Carver&) runs twice.
template <class Mem, class Layout>
hipError_t alloc_pool(Mem& m, size_t slack, Layout&& layout) {
  Carver measure;
  layout(measure);
  const hipError_t e = alloc(m, measure.off + slack);
  if (e != hipSuccess) return e;
  Carver place(m.get());
  layout(place);
  return hipSuccess;
}

// Commit on success: `dst` is emptied first (its buffers go before the new ones are allocated, so
// peak memory is one generation), the replacement is built aside by build(S&) and moved in only
// when that returns 0. After a failure dst reads as never built and what the build had acquired
// is released.
template <class S, class Build>
int32_t rebuild(S& dst, Build&& build) {
  dst = S{};
  S next;
  const int32_t rc = build(next);
  if (rc == 0) dst = std::move(next);
  return rc;
}

}  // namespace llsr_host
