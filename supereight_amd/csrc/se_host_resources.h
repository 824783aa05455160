// Owners of what a handle of the host library (se_hip_api.hip) holds on the device and in the runtime: device buffers, pinned host buffers, events
// and streams.  Host only, move-only, and nothing cleverer: no pool, no sharing, no exceptions.  A failed creation goes through the library's fail()
// (declared by the including file before this one) and comes back as its SE_HIP_* code, "hipMalloc <name>: <hip error string>".
//
// Destruction order.  se_hip_destroy selects the handle's device and synchronises both streams; deleting the handle then lets the members release
//   themselves in reverse order of declaration.  The two streams are declared first in se_hip_pipeline, so they go last, behind every buffer and event.
// Borrowed streams.  A stream handed in by the caller (se_hip_set_stream, se_hip_set_scan_stream) is borrowed: the handle enqueues on it and never
//   destroys it -- it is the caller's before, during and after.  Only a stream the handle created itself (Stream::create) is destroyed with it.
// Free and synchronisation.  hipFree waits for the device, so releasing a buffer is always safe but never free of cost or of ordering effects: a
//   buffer is released behind enqueued work in one place only, sort_block_list (a few times in a map's life).  The other growing sites
//   (reserve_staging, stage_input) synchronise the streams that may still read the old buffer themselves, then call reserve().
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>

// n items of T in device memory (PINNED: in page-locked host memory, hipHostMalloc's default flags)
template <typename T, bool PINNED>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }   // (move only: no copy, no assignment)
  ~Buf() { reset(); }
  int alloc(size_t n, const char* name) {   // (what it held is released first)
    reset();
    const hipError_t e = PINNED ? hipHostMalloc((void**)&p_, n * sizeof(T)) : hipMalloc((void**)&p_, n * sizeof(T));
    if (e != hipSuccess) { p_ = nullptr; return fail(SE_HIP_E_DEVICE, std::string(PINNED ? "hipHostMalloc " : "hipMalloc ") + name + ": " + hipGetErrorString(e)); }
    n_ = n;
    return SE_HIP_OK;
  }
  // grow-only: keeps a buffer that is large enough, else releases it and allocates n items (the contents are not carried over)
  int reserve(size_t n, const char* name) { return n <= n_ ? SE_HIP_OK : alloc(n, name); }
  void reset() { if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_)); p_ = nullptr; n_ = 0; }
  T* get() const { return p_; }
  size_t size() const { return n_; }   // items
  operator T*() const { return p_; }   // (launch arguments, copies, pointer arithmetic: an owner reads as the pointer it holds)
  T* operator->() const { return p_; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};
template <typename T = unsigned char> using DevBuf = Buf<T, false>;
template <typename T = unsigned char> using PinnedBuf = Buf<T, true>;

// An event and the flags it is created with; create() is a no-op once it exists, so "created on first use" is one call at the place of use
class Event {
 public:
  explicit Event(unsigned flags) : flags_(flags) {}
  Event(Event&& o) noexcept : e_(o.e_), flags_(o.flags_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept { std::swap(e_, o.e_); std::swap(flags_, o.flags_); return *this; }
  ~Event() { if (e_) (void)hipEventDestroy(e_); }
  int create(const char* name) {
    if (e_) return SE_HIP_OK;
    const hipError_t e = hipEventCreateWithFlags(&e_, flags_);
    if (e != hipSuccess) { e_ = nullptr; return fail(SE_HIP_E_DEVICE, std::string("hipEventCreate ") + name + ": " + hipGetErrorString(e)); }
    return SE_HIP_OK;
  }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
  unsigned flags_;
};

// A stream the handle created (non-blocking; destroyed with it) or one it borrowed from the caller (never destroyed here)
class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { reset(); }
  int create(const char* name) {   // (what it held is let go first)
    reset();
    const hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
    if (e != hipSuccess) { s_ = nullptr; return fail(SE_HIP_E_DEVICE, std::string("hipStreamCreate ") + name + ": " + hipGetErrorString(e)); }
    owned_ = true;
    return SE_HIP_OK;
  }
  void borrow(hipStream_t s) { reset(); s_ = s; }
  void reset() { if (owned_ && s_) (void)hipStreamDestroy(s_); s_ = nullptr; owned_ = false; }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
  bool owned_ = false;
};
