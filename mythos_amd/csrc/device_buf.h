// Ownership of device memory and of pinned host memory: the one place of the library that allocates and frees them.
// Also home of the error plumbing every translation unit shares (set_error / hip_fail / MYTHOS_HIP_TRY) and of
// select_device, so that this header stands on <hip/hip_runtime.h> alone (the host test of oracle/cpu_port compiles it
// against a malloc-backed one).
#ifndef MYTHOS_DEVICE_BUF_H
#define MYTHOS_DEVICE_BUF_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mythos_hip.h"

namespace mythos {

void set_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what);

#define MYTHOS_HIP_TRY(expr)                                   \
  do {                                                         \
    hipError_t _e = (expr);                                    \
    if (_e != hipSuccess) return ::mythos::hip_fail(_e, #expr); \
  } while (0)

// Makes `device` the calling thread's device: 0, or an error code with "<who>: ..." as the message.
inline int select_device(int device, const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    set_error(std::string(who) + ": no usable HIP device (the HIP path has no CPU fallback)");
    return MYTHOS_ERR_HIP;
  }
  if (device < 0 || device >= ndev) {
    set_error(std::string(who) + ": device index out of range");
    return MYTHOS_ERR_INVALID_ARGUMENT;
  }
  if (hipSetDevice(device) != hipSuccess) {
    set_error(std::string(who) + ": hipSetDevice failed");
    return MYTHOS_ERR_HIP;
  }
  return MYTHOS_OK;
}

// Move-only owner of one device allocation of `capacity()` elements of T.  DeviceBuf<void> counts bytes: it serves the
// arrays whose element type follows a handle's dtype.  Never a zero-byte allocation: a count of 0 allocates one element.
// Every fallible member returns 0 or an error code (hip_fail has set the message); the calling thread's device must be
// the one the buffer lives on, also when it is destroyed.
template <typename T>
class DeviceBuf {
  using Elem = std::conditional_t<std::is_void_v<T>, unsigned char, T>;

 public:
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
  DeviceBuf(DeviceBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  DeviceBuf& operator=(DeviceBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~DeviceBuf() { reset(); }

  T* get() const { return p_; }
  size_t capacity() const { return cap_; }
  explicit operator bool() const { return p_ != nullptr; }

  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr, cap_ = 0;
  }
  // a new allocation of max(count, 1) elements; the old one is freed first and its contents are gone
  int alloc(size_t count) {
    reset();
    count = std::max<size_t>(count, 1);
    MYTHOS_HIP_TRY(hipMalloc((void**)&p_, count * sizeof(Elem)));
    cap_ = count;
    return 0;
  }
  // a buffer that only grows: reallocated, contents not kept, when more than capacity() elements are needed
  int grow(size_t need) { return need <= cap_ ? 0 : alloc(need); }
  // a new allocation holding host[0 .. count)
  int upload(const T* host, size_t count) {
    if (int rc = alloc(count)) return rc;
    if (count > 0) MYTHOS_HIP_TRY(hipMemcpy(p_, host, count * sizeof(Elem), hipMemcpyHostToDevice));
    return 0;
  }
  template <typename U>
  int upload(const std::vector<U>& v) {
    static_assert(std::is_void_v<T> || std::is_same_v<U, Elem>, "a typed buffer takes a vector of its own element type");
    return upload(v.data(), std::is_void_v<T> ? v.size() * sizeof(U) : v.size());
  }
  // count doubles -> a new allocation of reals in the precision `dtype` names (MYTHOS_F32 / MYTHOS_F64)
  int upload_real(int dtype, const double* src, size_t count) {
    static_assert(std::is_void_v<T>, "the element type follows dtype: a byte-sized buffer");
    if (dtype != MYTHOS_F32) return upload(src, count * sizeof(double));
    std::vector<float> tmp(src, src + count);
    return upload(tmp);
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

using DeviceBytes = DeviceBuf<void>;

// Move-only owner of one allocation of pinned host memory (hipHostMalloc) of `capacity()` elements of T, with the address
// the device reads and writes the same memory at: what a kernel publishes to the host, or the host stages for a kernel,
// without a copy command.  The rules of DeviceBuf: never a zero-byte allocation, 0 or an error code, and the calling
// thread's device is the one the buffer was made on, also when it is destroyed.
template <typename T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  PinnedBuf(PinnedBuf&& o) noexcept : h_(o.h_), d_(o.d_), cap_(o.cap_) { o.h_ = o.d_ = nullptr, o.cap_ = 0; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_, d_ = o.d_, cap_ = o.cap_;
      o.h_ = o.d_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~PinnedBuf() { reset(); }

  T* host() const { return h_; }
  T* dev() const { return d_; }
  size_t capacity() const { return cap_; }
  explicit operator bool() const { return h_ != nullptr; }

  void reset() {
    if (h_) (void)hipHostFree(h_);
    h_ = d_ = nullptr, cap_ = 0;
  }
  // a new allocation of max(count, 1) elements; the old one is freed first and its contents are gone
  int alloc(size_t count) {
    reset();
    count = std::max<size_t>(count, 1);
    MYTHOS_HIP_TRY(hipHostMalloc((void**)&h_, count * sizeof(T), hipHostMallocDefault));
    if (const hipError_t e = hipHostGetDevicePointer((void**)&d_, h_, 0); e != hipSuccess) {
      reset();
      return hip_fail(e, "hipHostGetDevicePointer");
    }
    cap_ = count;
    return 0;
  }
  // allocated once, or again - contents not kept - when more than capacity() elements are needed
  int grow(size_t need) { return need <= cap_ ? 0 : alloc(need); }

 private:
  T* h_ = nullptr;
  T* d_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace mythos

#endif  // MYTHOS_DEVICE_BUF_H
