// device_buf.h — device buffers, pinned host buffers, events and streams that
// release themselves: deleting a context, stream or job frees what it holds.
// Every holder is non-copyable and converts to the raw handle it owns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <utility>

namespace dgrep {

// A device array and its capacity in elements. Two ways to grow, no others.
template <class T>
struct DevBuf {
  T* p = nullptr;
  uint64_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  operator T*() const { return p; }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  bool holds(uint64_t need) const { return cap >= need && p; }

  // Discard: at least `need` elements (one at the least), the contents dropped;
  // the old buffer is freed before the new one is allocated. *what names the
  // call that failed.
  hipError_t discard(uint64_t need, const char** what) {
    if (holds(need)) return hipSuccess;
    hipError_t e;
    *what = "hipFree(*p)";
    if (p && (e = hipFree(p)) != hipSuccess) return e;
    p = nullptr;
    cap = 0;
    const uint64_t n = std::max<uint64_t>(need, 1);
    *what = "hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T))";
    if ((e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T))) != hipSuccess) return e;
    cap = n;
    return hipSuccess;
  }

  // Keep: a new buffer of `want` elements is allocated first, the first `keep`
  // elements copied on `stream` (after `drain`, if given, has been waited for),
  // `stream` synchronised and the old buffer freed. *nomem: the allocation
  // failed (the sticky HIP error is cleared; the old buffer stands).
  hipError_t regrow(uint64_t want, uint64_t keep, hipStream_t stream, bool* nomem, hipStream_t drain = nullptr) {
    *nomem = false;
    T* fresh = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&fresh), want * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      *nomem = true;
      return hipErrorOutOfMemory;
    }
    DevBuf old;
    old.swap(*this);
    p = fresh;
    cap = want;
    if (!old.p) return hipSuccess;
    hipError_t e = drain ? hipStreamSynchronize(drain) : hipSuccess;
    if (e == hipSuccess && keep) e = hipMemcpyAsync(p, old.p, keep * sizeof(T), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e;  // `old` goes here
  }
};

// A pinned host array.
template <class T>
struct PinnedBuf {
  T* p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  operator T*() const { return p; }
  hipError_t alloc(size_t count) {
    return p ? hipSuccess : hipHostMalloc(reinterpret_cast<void**>(&p), count * sizeof(T), hipHostMallocDefault);
  }
};

// An event, made on the first create() (a second one keeps it).
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  operator hipEvent_t() const { return e; }
  hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
};

// A non-blocking stream, made on the first create(). Declared before the
// members whose work runs on it, so that it is destroyed after them.
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
  hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};

}  // namespace dgrep
