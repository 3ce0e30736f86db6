// Host-only HIP helpers shared by every host translation unit of the library: the error
// macro and the owners of device memory, streams and events.  Needs only the runtime API
// header, so plain C++ (gh_io.cpp, the sanitizer programs) can include it.  The owners
// free on the device that is current when they are released: their holders call
// hipSetDevice first.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>
#include <utility>

#include "gh_internal.hpp"

// Returns the library's GH_E_HIP code with the failing call's text from the enclosing
// function.
#define GH_HIP(expr)                                                                        \
  do {                                                                                      \
    hipError_t gh_err_ = (expr);                                                            \
    if (gh_err_ != hipSuccess)                                                              \
      return ::gh::fail(GH_E_HIP, std::string(#expr) + ": " + hipGetErrorString(gh_err_));  \
  } while (0)

namespace gh {

// An owning device allocation.
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      cap_ = std::exchange(o.cap_, 0);
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  // A new allocation of `bytes` (the old one is freed first), optionally zeroed.
  int alloc(uint64_t bytes, bool zero = false) {
    reset();
    GH_HIP(hipMalloc(&p_, bytes));
    cap_ = bytes;
    if (zero && bytes) GH_HIP(hipMemset(p_, 0, bytes));
    return GH_OK;
  }
  // At least `bytes`: grows only (the contents are lost when it grows).
  int reserve(uint64_t bytes) { return bytes > cap_ ? alloc(bytes) : (int)GH_OK; }
  // A new allocation holding a copy of host memory.
  int upload(const void* src, uint64_t bytes) {
    if (int rc = alloc(bytes)) return rc;
    GH_HIP(hipMemcpy(p_, src, bytes, hipMemcpyHostToDevice));
    return GH_OK;
  }
  template <class T = void>
  T* get() const {
    return static_cast<T*>(p_);
  }
  uint64_t capacity() const { return cap_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
  uint64_t cap_ = 0;
};

// An owning stream (non-blocking).
class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (s_) (void)hipStreamDestroy(s_);
  }
  int create() {
    GH_HIP(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
    return GH_OK;
  }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

// An owning event, created on first use.
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event& operator=(Event&& o) noexcept {
    std::swap(e_, o.e_);
    return *this;
  }
  ~Event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  int create(unsigned flags = hipEventDefault) {
    if (!e_) GH_HIP(hipEventCreateWithFlags(&e_, flags));
    return GH_OK;
  }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

// The two timing events around a piece of work on a stream.
struct EventPair {
  Event a, b;
  int create() {
    if (int rc = a.create()) return rc;
    return b.create();
  }
  int elapsed(float* ms) const {
    GH_HIP(hipEventElapsedTime(ms, a, b));
    return GH_OK;
  }
};

}  // namespace gh
