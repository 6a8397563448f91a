// TEST-ONLY stand-in for the HIP calls that direct_amd/csrc/host_stage.h uses, so that the header runs on the CPU under
// AddressSanitizer: device memory is malloc'd host memory, copies and fills are memcpy and memset and happen at once,
// synchronisation does nothing.  The counters and the fail_malloc_at switch are what tests/cpp/test_host_stage.cpp observes.
#pragma once
#define HOST_STAGE_FAKE_HIP 1
#include <cstddef>
#include <cstdlib>
#include <cstring>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorNotReady = 600 };
typedef void* hipStream_t;
struct FakeEvent { int recorded; };
typedef FakeEvent* hipEvent_t;
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };

namespace fake_hip {
inline int n_malloc = 0, n_free = 0, n_sync = 0, n_copy = 0, n_fill = 0;
constexpr int kFresh = 0x5a;
inline int fail_malloc_at = -1;  // the n-th hipMalloc from now on (0: the next one) fails once
}  // namespace fake_hip

inline hipError_t hipMalloc(void** p, size_t bytes) {
  if (fake_hip::fail_malloc_at >= 0 && fake_hip::fail_malloc_at-- == 0) {
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  fake_hip::n_malloc++;
  if (posix_memalign(p, 256, bytes ? bytes : 1) != 0) return hipErrorOutOfMemory;  // 256-aligned, as the runtime's blocks are
  std::memset(*p, fake_hip::kFresh, bytes);  // "what was there" in a fresh block, so that a test can recognise it
  return hipSuccess;
}
inline hipError_t hipFree(void* p) {
  fake_hip::n_free++;
  std::free(p);
  return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) {
  fake_hip::n_sync++;
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
  fake_hip::n_copy++;
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}
inline hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
  fake_hip::n_fill++;
  std::memset(dst, value, bytes);
  return hipSuccess;
}
inline hipError_t hipEventCreate(hipEvent_t* e) {
  *e = new FakeEvent{0};
  return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e) {
  delete e;
  return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {
  e->recorded++;
  return hipSuccess;
}
inline hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  *ms = a->recorded && b->recorded ? 1.0f : -1.0f;
  return hipSuccess;
}
