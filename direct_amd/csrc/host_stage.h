// Host-side plumbing shared by the batched C-ABI entry points.  Host code only, four pieces:
//   Block      a device block that grows on demand and never shrinks (ONE rule for when the old block may be freed)
//   Stage      the staging plan of one call: host arrays through one Block at 256-byte offsets, device arrays passed through
//   alloc_all  several device allocations, all or nothing, owned by a handle's `allocs`
//   EventPair  the two events around a call's kernels and their read-out
// tests/cpp/test_host_stage.cpp runs all of it on the CPU against a fake of the HIP calls used here.
#pragma once
#ifndef HOST_STAGE_FAKE_HIP  // defined by tests/cpp/fake_hip_runtime.h, which then stands in for the runtime
#include <hip/hip_runtime.h>
#endif

#include <cstddef>
#include <cstring>
#include <initializer_list>
#include <vector>

namespace hs {

// ---- a grown device block -----------------------------------------------------------------------------------------------
struct Block {
  void* p = nullptr;
  size_t bytes = 0;
};
inline void release(Block& b) {
  if (b.p) (void)hipFree(b.p);
  b = Block{};
}
// At least `bytes` behind b.p.  A block that is large enough is left alone; otherwise the stream is drained FIRST (work
// enqueued on it may still use the old block), the old block freed and a new one allocated.  Empty after a failure.
inline hipError_t grow(Block& b, hipStream_t stream, size_t bytes) {
  if (bytes <= b.bytes) return hipSuccess;
  hipError_t e = b.p ? hipStreamSynchronize(stream) : hipSuccess;
  release(b);
  if (e == hipSuccess) e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) b.p = nullptr;
  else b.bytes = bytes;
  return e;
}

// ---- the staging plan of one call ---------------------------------------------------------------------------------------
// Register every array with the address of the pointer the kernels will read (`dev`), then stage_upload, launch,
// stage_download.  Host memory: every non-null array gets a 256-aligned slice of ONE block; inputs are copied up, outputs
// registered with a fill byte are filled with it (what the kernels leave unwritten then reads as that byte on the host), outputs
// without one hold whatever the block held.  Device memory: *dev is the caller's own pointer, nothing is allocated or copied.
// A null array stays null either way.  Scratch slices live in the block in both modes.  No heap allocation: 32 slots inline.
struct Stage {
  static constexpr int kMaxSlots = 32;
  enum Kind : unsigned char { kIn, kOut, kScratch };
  struct Slot {
    void* bind;   // where the device pointer goes
    void* user;   // the caller's array
    void* dev;    // the device pointer (after stage_upload)
    size_t bytes, off;
    int fill;     // fill byte of a staged output, -1: none
    Kind kind;
    bool staged;  // has a slice of the block
  };
  bool host;
  bool overflow = false;  // more than kMaxSlots registrations: stage_upload fails
  int n = 0;
  size_t total = 0;
  Slot s[kMaxSlots];
  explicit Stage(bool host_memory) : host(host_memory) {}
};
inline void stage_add(Stage& st, void* bind, const void* user, size_t bytes, int fill, Stage::Kind kind) {
  if (st.n == Stage::kMaxSlots) {
    st.overflow = true;
    return;
  }
  const bool staged = kind == Stage::kScratch || (st.host && user);
  st.s[st.n++] = Stage::Slot{bind, const_cast<void*>(user), nullptr, bytes, st.total, fill, kind, staged};
  if (staged) st.total += bytes ? (bytes + 255) & ~(size_t)255 : 256;  // an empty array still gets an address of its own
}
template <typename T>
inline void stage_in(Stage& st, T** dev, const void* src, size_t bytes) {
  stage_add(st, dev, src, bytes, -1, Stage::kIn);
}
template <typename T>
inline void stage_out(Stage& st, T** dev, void* dst, size_t bytes, int fill = -1) {
  stage_add(st, dev, dst, bytes, fill, Stage::kOut);
}
template <typename T>
inline void stage_scratch(Stage& st, T** dev, size_t bytes) {
  stage_add(st, dev, nullptr, bytes, -1, Stage::kScratch);
}
// Grows the block, hands every slot its device pointer and enqueues the uploads and fills.  After a failure the staged
// pointers are null and (host memory) the stream has drained: no copy still reads the caller's arrays.
inline hipError_t stage_upload(Stage& st, Block& blk, hipStream_t stream) {
  hipError_t e = st.overflow ? hipErrorInvalidValue : grow(blk, stream, st.total);
  for (int i = 0; i < st.n; i++) {
    Stage::Slot& q = st.s[i];
    q.dev = !q.staged ? q.user : (e == hipSuccess ? (char*)blk.p + q.off : nullptr);
    std::memcpy(q.bind, &q.dev, sizeof(void*));
    if (e != hipSuccess || !q.staged || !q.bytes) continue;
    if (q.kind == Stage::kIn) e = hipMemcpyAsync(q.dev, q.user, q.bytes, hipMemcpyHostToDevice, stream);
    else if (q.fill >= 0) e = hipMemsetAsync(q.dev, q.fill, q.bytes, stream);
  }
  if (e != hipSuccess && st.host) (void)hipStreamSynchronize(stream);
  return e;
}
// The tail of a call: `e` is what the launches left; the staged outputs are copied back only when that is no error.
inline hipError_t stage_download(const Stage& st, hipStream_t stream, hipError_t e) {
  for (int i = 0; i < st.n && e == hipSuccess; i++) {
    const Stage::Slot& q = st.s[i];
    if (q.kind == Stage::kOut && q.staged && q.bytes) e = hipMemcpyAsync(q.user, q.dev, q.bytes, hipMemcpyDeviceToHost, stream);
  }
  return e;
}
// synchronises whatever `e` says, and reports the first of the two errors
inline hipError_t drain(hipStream_t stream, hipError_t e) {
  const hipError_t e2 = hipStreamSynchronize(stream);
  return e != hipSuccess ? e : e2;
}

// ---- all-or-nothing allocation ------------------------------------------------------------------------------------------
struct Want {
  void* bind;  // address of the pointer that receives the allocation
  size_t bytes;
};
template <typename T>
inline Want want(T** p, size_t bytes) {
  return Want{p, bytes};
}
// Every allocation of the list, appended to `owner` (the handle's list of what its destroy frees), or none of them: after a
// failure what was allocated is freed again, `owner` and the pointers are as before, and the error is returned.
inline hipError_t alloc_all(std::vector<void*>& owner, std::initializer_list<Want> list) {
  const size_t had = owner.size();
  for (const Want& w : list) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, w.bytes ? w.bytes : 16);
    if (e != hipSuccess) {
      for (; owner.size() > had; owner.pop_back()) (void)hipFree(owner.back());
      return e;
    }
    owner.push_back(q);
  }
  size_t i = had;
  for (const Want& w : list) std::memcpy(w.bind, &owner[i++], sizeof(void*));
  return hipSuccess;
}

// ---- the event pair around a call's kernels -----------------------------------------------------------------------------
struct EventPair {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;  // ev1 has been recorded behind ev0: there is something to read, or to wait for
};
inline hipError_t create(EventPair& t) {
  const hipError_t e = hipEventCreate(&t.ev0);
  return e != hipSuccess ? e : hipEventCreate(&t.ev1);
}
inline void destroy(EventPair& t) {
  if (t.ev0) (void)hipEventDestroy(t.ev0);
  if (t.ev1) (void)hipEventDestroy(t.ev1);
  t = EventPair{};
}
inline hipError_t start(EventPair& t, hipStream_t stream) {
  t.timed = false;
  return hipEventRecord(t.ev0, stream);
}
inline hipError_t stop(EventPair& t, hipStream_t stream) {
  const hipError_t e = hipEventRecord(t.ev1, stream);
  t.timed = e == hipSuccess;
  return e;
}
// milliseconds between the two events of the last start / stop; waits for the second one.  Fails when nothing has been timed.
inline hipError_t elapsed(const EventPair& t, float* ms) {
  if (!t.timed) return hipErrorNotReady;
  const hipError_t e = hipEventSynchronize(t.ev1);
  return e != hipSuccess ? e : hipEventElapsedTime(ms, t.ev0, t.ev1);
}

}  // namespace hs
