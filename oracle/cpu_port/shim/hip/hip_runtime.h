// Host stand-in for <hip/hip_runtime.h>, used ONLY by oracle/cpu_port (the CPU baseline / sanitizer build of the
// physics templates in mythos_amd/csrc/oxdna_math.h, oxdna_pair.h, martini_terms.h and philox.h, and the host test of
// device_buf.h).  TEST INFRASTRUCTURE: nothing
// under mythos_amd/ sees this file; the product is compiled by hipcc against the real header.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))

static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
// the device fast-math intrinsics (glibc declares functions of these names itself: map them by macro)
#define __expf expf
#define __logf logf
#define __sinf sinf
#define __cosf cosf
static inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }
// (named by a branch of the templates that only the GPU's dU/d(sequence distribution) instantiation compiles)
static inline double atomicAdd(double* p, double v) {
  const double old = *p;
  *p += v;
  return old;
}

// ---- malloc-backed stand-ins for the runtime calls of mythos_amd/csrc/device_buf.h (selftest.cpp --device-buf): one
// "device", a count of live allocations, and a switch that makes the k-th allocation from now on fail
enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorInvalidDevice = 101 };
enum hipMemcpyKind { hipMemcpyHostToHost, hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
inline long& shim_live_allocations() {
  static long live = 0;
  return live;
}
inline long& shim_fail_allocation_in() {  // k > 0: the k-th hipMalloc / hipHostMalloc from now fails (once); 0: none does
  static long k = 0;
  return k;
}
static inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : (e == hipErrorOutOfMemory ? "out of memory" : "error"); }
static inline hipError_t hipMalloc(void** p, size_t bytes) {
  *p = nullptr;
  if (bytes == 0) return hipErrorInvalidValue;  // (the real runtime returns a null pointer: owners never ask for it)
  long& k = shim_fail_allocation_in();
  if (k > 0 && --k == 0) return hipErrorOutOfMemory;
  if (!(*p = malloc(bytes))) return hipErrorOutOfMemory;
  ++shim_live_allocations();
  return hipSuccess;
}
static inline hipError_t hipFree(void* p) {
  if (p) free(p), --shim_live_allocations();
  return hipSuccess;
}
// pinned host memory: the same allocator, count and switch; the "device" reads it at the host's address
enum { hipHostMallocDefault = 0 };
static inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
static inline hipError_t hipHostFree(void* p) { return hipFree(p); }
static inline hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned) {
  *dev = host;
  return host ? hipSuccess : hipErrorInvalidValue;
}
static inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  memcpy(dst, src, bytes);
  return hipSuccess;
}
static inline hipError_t hipMemset(void* dst, int value, size_t bytes) {
  memset(dst, value, bytes);
  return hipSuccess;
}
static inline hipError_t hipGetDeviceCount(int* n) {
  *n = 1;
  return hipSuccess;
}
static inline hipError_t hipSetDevice(int device) { return device == 0 ? hipSuccess : hipErrorInvalidDevice; }
