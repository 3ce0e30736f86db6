// Host-only HIP helpers shared by every host translation unit of the library: the error
// macro, the owners of device memory, streams and events, the device gate of the contexts
// (open_device) and the host skeleton of the two batched paths (BatchQueue, unit_grid and
// the upload helpers).  Needs only the runtime API header, so plain C++ (gh_io.cpp, the
// sanitizer programs) can include it.  The owners free on the device that is current when
// they are released: their holders call hipSetDevice first.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
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

// The gate of every context: a visible device of that ordinal, gfx950, made current.
// no_device_msg: the caller's "no CPU fallback" text.  Sets *num_cu.
inline int open_device(int device, const char* no_device_msg, int* num_cu) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(GH_E_NODEV, no_device_msg);
  if (device < 0 || device >= n) return fail(GH_E_ARG, "device ordinal out of range");
  hipDeviceProp_t prop;
  GH_HIP(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return fail(GH_E_NODEV, std::string("device is ") + prop.gcnArchName + ", need gfx950");
  GH_HIP(hipSetDevice(device));
  *num_cu = prop.multiProcessorCount;
  return GH_OK;
}

// Makes `consumer` wait for what the producer's stream holds now (ev: created on first use).
inline int stream_follow(Event& ev, void* producer_stream, hipStream_t consumer) {
  if (int rc = ev.create(hipEventDisableTiming)) return rc;
  GH_HIP(hipEventRecord(ev, (hipStream_t)producer_stream));
  GH_HIP(hipStreamWaitEvent(consumer, ev, 0));
  return GH_OK;
}

// At least `bytes` (and never an empty allocation), then a copy of host memory.
inline int upload_at_least(DevBuf& d, const void* src, uint64_t bytes) {
  if (int rc = d.reserve(std::max<uint64_t>(bytes, 16))) return rc;
  if (bytes) GH_HIP(hipMemcpy(d.get(), src, bytes, hipMemcpyHostToDevice));
  return GH_OK;
}

// A host-assembled arena into d (already reserved): large ones through the pinned staging.
inline int upload_arena(int device, DevBuf& d, const void* host, uint64_t bytes) {
  if (!bytes) return GH_OK;
  if (use_staged(bytes)) return h2d_staged(device, host, bytes, d.get());
  GH_HIP(hipMemcpy(d.get(), host, bytes, hipMemcpyHostToDevice));
  return GH_OK;
}

// Workgroups of a batch's per-unit kernels: `env` (GH_BATCH_GRID / GH_EBATCH_GRID, tests)
// when set, so that one wave walks many units and streams; else one unit per wave, at most
// 8 workgroups per CU.  Read at each use.
inline uint32_t unit_grid(const char* env, uint64_t nunits, uint32_t waves, int num_cu) {
  if (const char* eg = getenv(env)) return (uint32_t)std::clamp<long>(atol(eg), 1, 1l << 20);
  return (uint32_t)std::clamp<uint64_t>(ceil_div(nunits, waves), 1, 8ull * (uint64_t)num_cu);
}

// What the batched decode (gh_batch) and the batched encode (gh_ebatch) share on the host:
// the device, a stream of their own, and the order of the work enqueued on them.  One run
// (begin .. end) may go to a caller's stream; runs of one queue share the holder's scratch,
// so each waits for the one before it.  The holder calls hipSetDevice(device) first.
struct BatchQueue {
  int device = 0, num_cu = 0;
  Stream stream;
  Event done;   // end of the last run, on whatever stream it ran
  Event ev_in;  // follow(): the producer stream's position
  EventPair ev;
  bool enqueued = false, timed = false;
  ~BatchQueue() {
    (void)hipSetDevice(device);
    if (enqueued) (void)hipEventSynchronize(done);  // (it may run on a caller's stream)
    if (stream) (void)hipStreamSynchronize(stream);
  }
  int create(int dev, const char* no_device_msg) {
    if (int rc = open_device(dev, no_device_msg, &num_cu)) return rc;
    device = dev;
    if (int rc = stream.create()) return rc;
    if (int rc = done.create(hipEventDisableTiming)) return rc;
    return ev.create();
  }
  // Nothing of the queue's is in flight afterwards: the last run is over (it reads what a
  // load replaces) and the queue's own stream is idle.
  int quiesce() {
    if (enqueued) GH_HIP(hipEventSynchronize(done));
    GH_HIP(hipStreamSynchronize(stream));
    enqueued = false;
    return GH_OK;
  }
  int follow(void* producer_stream) { return stream_follow(ev_in, producer_stream, stream); }
  // Starts a run on hip_stream (null: the queue's own): st waits for the previous run.
  int begin(void* hip_stream, bool want_timed, hipStream_t* st) {
    *st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)stream;
    if (enqueued) GH_HIP(hipStreamWaitEvent(*st, done, 0));
    if (want_timed) GH_HIP(hipEventRecord(ev.a, *st));
    pending_timed_ = want_timed;
    return GH_OK;
  }
  int end(hipStream_t st) {
    if (pending_timed_) GH_HIP(hipEventRecord(ev.b, st));
    GH_HIP(hipEventRecord(done, st));
    enqueued = true;
    timed = pending_timed_;
    return GH_OK;
  }
  // Waits for the last run; *ms: its event time when it was timed, else 0.
  int wait(float* ms) {
    GH_HIP(hipEventSynchronize(done));
    *ms = 0;
    return timed ? ev.elapsed(ms) : (int)GH_OK;
  }

 private:
  bool pending_timed_ = false;
};

}  // namespace gh
