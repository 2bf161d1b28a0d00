// afs_buf.h -- the one owner of the library's device and pinned host memory (afs_ctx.h, afs_capi.cpp,
// afs_comm.cpp).  Host only.  AFS_BUF_HOST_ONLY leaves the HIP allocators out, for a CPU program
// that brings an allocator of its own (tests/cpp/buf_main.cpp).
#pragma once

#include <cstddef>

#ifndef AFS_BUF_HOST_ONLY
#include <hip/hip_runtime.h>
#endif

namespace afs {

// A block of Alloc's memory, grown on demand, freed by the destructor; moved, never copied.
// Alloc: a type `error` whose value-initialised value means success, and
//   static error alloc(void **p, size_t bytes);   static void release(void *p);
template <class Alloc>
class Buf {
 public:
  using error = typename Alloc::error;
  Buf() = default;
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  Buf(Buf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) {
      release();
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~Buf() { release(); }

  // At least `bytes`: nothing happens while the capacity suffices (the block and its contents stay).
  // Else the old block is freed first and only then the new one allocated, its contents undefined:
  // two blocks never live at once (the metric batch's buffers hold ~62 GB).  A failed allocation
  // leaves the buffer empty.
  error reserve(size_t bytes) {
    if (bytes <= cap_) return error{};
    release();
    const error e = Alloc::alloc(&p_, bytes);
    if (e != error{}) {
      p_ = nullptr;
      return e;
    }
    cap_ = bytes;
    return error{};
  }
  void release() {
    if (p_) Alloc::release(p_);
    p_ = nullptr, cap_ = 0;
  }
  void *data() const { return p_; }
  template <class T>
  T *as() const { return static_cast<T *>(p_); }
  size_t capacity() const { return cap_; }

 private:
  void *p_ = nullptr;
  size_t cap_ = 0;
};

#ifndef AFS_BUF_HOST_ONLY
struct DeviceAlloc {
  using error = hipError_t;
  static error alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void *p) { (void)hipFree(p); }
};
struct PinnedAlloc {
  using error = hipError_t;
  static error alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void *p) { (void)hipHostFree(p); }
};
using DeviceBuf = Buf<DeviceAlloc>;
using PinnedBuf = Buf<PinnedAlloc>;
#endif

}  // namespace afs
