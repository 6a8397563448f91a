// CPU test of direct_amd/csrc/host_stage.h against tests/cpp/fake_hip_runtime.h (built with -fsanitize=address,undefined by
// tests/test_host_stage_cpp.py): layout of the staging plan, fills, the grow rule, device mode, all-or-nothing allocation and
// the event pair.  Prints PASS and returns 0, or says which check failed.
#include "fake_hip_runtime.h"

#include "../../direct_amd/csrc/host_stage.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                         \
    }                                                                   \
  } while (0)

namespace {
constexpr int kAuditSlots = 23;  // direct_traj_audit_batch with every input and output: the largest plan of the library

// one random plan of n slots in host memory: alignment, disjointness, bounds, null arrays, uploaded contents
int layout_case(std::mt19937& rng, int n, hs::Block& blk) {
  std::vector<std::vector<unsigned char>> host(n);
  std::vector<void*> dev(n, (void*)0x1);
  std::vector<int> kind(n);
  hs::Stage st(true);
  for (int i = 0; i < n; i++) {
    const int pick = (int)(rng() % 8);
    const size_t bytes = pick == 0 ? 0 : (pick == 1 ? 256 * (1 + rng() % 4) : 1 + rng() % 5000);  // empty, tile multiples, odd sizes
    kind[i] = (int)(rng() % 4);  // 0 input, 1 output, 2 scratch, 3 a null optional array
    host[i].assign(bytes ? bytes : 1, 0);
    for (unsigned char& c : host[i]) c = (unsigned char)rng();
    if (kind[i] == 0) hs::stage_in(st, &dev[i], host[i].data(), bytes);
    else if (kind[i] == 1) hs::stage_out(st, &dev[i], host[i].data(), bytes, (int)(rng() % 3) - 1);
    else if (kind[i] == 2) hs::stage_scratch(st, &dev[i], bytes);
    else if (rng() % 2) hs::stage_in(st, &dev[i], nullptr, bytes);
    else hs::stage_out(st, &dev[i], nullptr, bytes, 0);
    host[i].resize(bytes);
  }
  CHECK(hs::stage_upload(st, blk, nullptr) == hipSuccess);
  std::vector<std::pair<uintptr_t, size_t>> span;
  for (int i = 0; i < n; i++) {
    if (kind[i] == 3) {
      CHECK(dev[i] == nullptr);
      continue;
    }
    const uintptr_t p = (uintptr_t)dev[i], base = (uintptr_t)blk.p;
    CHECK(dev[i] != nullptr && p % 256 == 0);
    CHECK(p >= base && p + host[i].size() <= base + blk.bytes);
    span.push_back({p, host[i].size()});
    if (kind[i] == 0) CHECK(std::memcmp(dev[i], host[i].data(), host[i].size()) == 0);
  }
  std::sort(span.begin(), span.end());
  for (size_t i = 1; i < span.size(); i++) CHECK(span[i - 1].first + std::max<size_t>(span[i - 1].second, 1) <= span[i].first);
  CHECK(hs::stage_download(st, nullptr, hipSuccess) == hipSuccess);
  return 0;
}

int test_layout() {
  std::mt19937 rng(12345);
  hs::Block blk;
  for (int trial = 0; trial < 200; trial++)
    if (layout_case(rng, trial == 0 ? kAuditSlots : 1 + (int)(rng() % kAuditSlots), blk)) return 1;
  // one slot too many is refused, and nothing is written past the inline arrays
  hs::Stage st(true);
  void* dev[hs::Stage::kMaxSlots + 1];
  unsigned char byte = 0;
  for (void*& d : dev) hs::stage_in(st, &d, &byte, 1);
  CHECK(st.n == hs::Stage::kMaxSlots && hs::stage_upload(st, blk, nullptr) != hipSuccess);
  hs::release(blk);
  CHECK(blk.p == nullptr && blk.bytes == 0);
  return 0;
}

// a host loop stands for a kernel that writes only a prefix of its outputs
int test_fills() {
  constexpr int n = 300, prefix = 37;
  std::vector<int32_t> zero(n, 99), ones(n, 99), raw(n, 99);
  int32_t *dz = nullptr, *do_ = nullptr, *dr = nullptr;
  hs::Block blk;  // fresh
  hs::Stage st(true);
  hs::stage_out(st, &dz, zero.data(), n * 4, 0);
  hs::stage_out(st, &do_, ones.data(), n * 4, 0xff);
  hs::stage_out(st, &dr, raw.data(), n * 4);
  CHECK(hs::stage_upload(st, blk, nullptr) == hipSuccess);
  for (int i = 0; i < prefix; i++) dz[i] = do_[i] = dr[i] = 1000 + i;
  CHECK(hs::stage_download(st, nullptr, hipSuccess) == hipSuccess && hs::drain(nullptr, hipSuccess) == hipSuccess);
  int32_t fresh;
  std::memset(&fresh, fake_hip::kFresh, 4);
  for (int i = 0; i < n; i++) {
    CHECK(zero[i] == (i < prefix ? 1000 + i : 0));
    CHECK(ones[i] == (i < prefix ? 1000 + i : -1));
    CHECK(raw[i] == (i < prefix ? 1000 + i : fresh));  // no fill: what the block held
  }
  // an error from the launches: nothing is copied back, and drain reports that error, not its own success
  std::fill(zero.begin(), zero.end(), 5);
  CHECK(hs::stage_download(st, nullptr, hipErrorInvalidValue) == hipErrorInvalidValue && zero[0] == 5);
  CHECK(hs::drain(nullptr, hipErrorInvalidValue) == hipErrorInvalidValue);
  hs::release(blk);
  return 0;
}

int test_grow() {
  hs::Block blk;
  const int m0 = fake_hip::n_malloc, f0 = fake_hip::n_free, s0 = fake_hip::n_sync;
  CHECK(hs::grow(blk, nullptr, 1000) == hipSuccess && blk.bytes == 1000);
  void* small = blk.p;
  CHECK(hs::grow(blk, nullptr, 1000) == hipSuccess && blk.p == small);
  CHECK(hs::grow(blk, nullptr, 100000) == hipSuccess && blk.bytes == 100000);
  void* large = blk.p;
  CHECK(hs::grow(blk, nullptr, 1000) == hipSuccess && blk.p == large && blk.bytes == 100000);  // never shrinks
  CHECK(fake_hip::n_malloc - m0 == 2 && fake_hip::n_free - f0 == 1);
  CHECK(fake_hip::n_sync - s0 == 1);  // only the old block's users are waited for
  fake_hip::fail_malloc_at = 0;
  CHECK(hs::grow(blk, nullptr, 200000) != hipSuccess && blk.p == nullptr && blk.bytes == 0);  // empty after a failure
  CHECK(fake_hip::n_free - f0 == 2);
  // a plan whose block cannot grow hands out null pointers and reports the error
  unsigned char src[8] = {};
  void* d = (void*)0x1;
  hs::Stage st(true);
  hs::stage_in(st, &d, src, 8);
  fake_hip::fail_malloc_at = 0;
  CHECK(hs::stage_upload(st, blk, nullptr) != hipSuccess && d == nullptr && blk.p == nullptr);
  return 0;
}

int test_device_mode() {
  const int m0 = fake_hip::n_malloc, c0 = fake_hip::n_copy, f0 = fake_hip::n_fill, s0 = fake_hip::n_sync;
  hs::Block blk;
  const double* in = nullptr;
  const double* absent = (const double*)0x1;
  int32_t* out = nullptr;
  double a[4] = {1, 2, 3, 4};
  int32_t b[4] = {5, 6, 7, 8};
  hs::Stage st(false);
  hs::stage_in(st, &in, a, sizeof a);
  hs::stage_in(st, &absent, nullptr, 64);
  hs::stage_out(st, &out, b, sizeof b, 0);
  CHECK(hs::stage_upload(st, blk, nullptr) == hipSuccess);
  CHECK(in == a && out == b && absent == nullptr && blk.p == nullptr);  // the caller's pointers, bit for bit
  CHECK(hs::stage_download(st, nullptr, hipSuccess) == hipSuccess);
  CHECK(b[0] == 5 && b[3] == 8);
  CHECK(fake_hip::n_malloc == m0 && fake_hip::n_copy == c0 && fake_hip::n_fill == f0 && fake_hip::n_sync == s0);
  // a scratch slice is device memory of the call in either mode
  int* ring = nullptr;
  hs::Stage st2(false);
  hs::stage_scratch(st2, &ring, 100);
  hs::stage_out(st2, &out, b, sizeof b);
  CHECK(hs::stage_upload(st2, blk, nullptr) == hipSuccess && ring == blk.p && blk.bytes == 256 && out == b);
  hs::release(blk);
  return 0;
}

int test_alloc_all() {
  constexpr int n = 5;
  void* const untouched = (void*)0x1;
  int marker = 0;
  for (int k = 0; k <= n; k++) {  // k == n: nothing fails
    std::vector<void*> owner = {&marker};
    void* p[n] = {untouched, untouched, untouched, untouched, untouched};
    const int m0 = fake_hip::n_malloc, f0 = fake_hip::n_free;
    fake_hip::fail_malloc_at = k < n ? k : -1;
    const hipError_t e = hs::alloc_all(owner, {hs::want(&p[0], 10), hs::want(&p[1], 0), hs::want(&p[2], 300), hs::want(&p[3], 7),
                                               hs::want(&p[4], 4096)});
    if (k < n) {
      CHECK(e == hipErrorOutOfMemory);
      CHECK(fake_hip::n_malloc - m0 == k && fake_hip::n_free - f0 == k);  // every earlier allocation freed again
      CHECK(owner.size() == 1 && owner[0] == &marker);
      for (void* q : p) CHECK(q == untouched);
    } else {
      CHECK(e == hipSuccess && fake_hip::n_malloc - m0 == n && fake_hip::n_free == f0 && owner.size() == 1 + n);
      for (int i = 0; i < n; i++) {
        CHECK(p[i] != nullptr && p[i] != untouched && owner[1 + i] == p[i]);
        (void)hipFree(p[i]);
      }
    }
  }
  fake_hip::fail_malloc_at = -1;
  return 0;
}

int test_event_pair() {
  hs::EventPair t;
  float ms = 0.f;
  CHECK(hs::create(t) == hipSuccess && !t.timed);
  CHECK(hs::elapsed(t, &ms) != hipSuccess);  // nothing timed yet
  CHECK(hs::start(t, nullptr) == hipSuccess);
  CHECK(hs::elapsed(t, &ms) != hipSuccess);  // not before the first stop
  CHECK(hs::stop(t, nullptr) == hipSuccess && t.timed);
  CHECK(hs::elapsed(t, &ms) == hipSuccess && ms == 1.0f);
  CHECK(hs::start(t, nullptr) == hipSuccess && hs::elapsed(t, &ms) != hipSuccess);  // a call that never reached its stop
  hs::destroy(t);
  CHECK(t.ev0 == nullptr && t.ev1 == nullptr && !t.timed);
  return 0;
}
}  // namespace

int main() {
  if (test_layout() || test_fills() || test_grow() || test_device_mode() || test_alloc_all() || test_event_pair()) return 1;
  std::printf("PASS\n");
  return 0;
}
