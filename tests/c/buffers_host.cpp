// buffers_host.cpp -- raftsql_amd/csrc/raftq_buffers.hpp against a fake HIP runtime (tests/test_buffers_host.py builds this
// with g++ -fsanitize=address,undefined and runs it: no GPU, no HIP library).  The fakes below count over malloc: every
// allocation is registered with the API that made it, a free through the wrong API or of an unknown pointer fails the run, and
// `fail_at` makes the k-th fallible call (allocation, alias lookup, memset, synchronise) return an error.
#include "raftq_buffers.hpp"

#include <algorithm>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

namespace fake {
enum Api { kDev, kHost, kExt };
struct Rec {
  Api api;
  size_t bytes;
  unsigned flags;
};
std::map<void*, Rec> live;
std::vector<std::string> log;  // "malloc", "hostmalloc:<flags>", "ext", "alias", "memset", "sync", "free", "hostfree"
int calls = 0, fail_at = 0;    // fail_at: 1-based index of the fallible call that fails (0 = none)
uint64_t frees = 0, allocs = 0;
hipStream_t the_stream = (hipStream_t)(uintptr_t)0x1000;
int wrong = 0;

bool trip() { return ++calls == fail_at; }
void* alias_of(void* h) { return (void*)((uintptr_t)h ^ ((uintptr_t)1 << 62)); }
hipError_t make(void** p, size_t bytes, Api api, unsigned flags) {
  if (trip()) {
    *p = (void*)(uintptr_t)0xdead;  // a failed call may leave anything behind
    return hipErrorOutOfMemory;
  }
  *p = std::malloc(bytes ? bytes : 1);
  std::memset(*p, 0xa5, bytes);
  live[*p] = Rec{api, bytes, flags};
  ++allocs;
  return hipSuccess;
}
hipError_t drop(void* p, bool host_api) {
  if (!p) return hipSuccess;
  auto it = live.find(p);
  if (it == live.end() || (it->second.api == kHost) != host_api) {
    std::fprintf(stderr, "FAIL: %s of %p: %s\n", host_api ? "hipHostFree" : "hipFree", p,
                 it == live.end() ? "not a live allocation (double free?)" : "made by the other API");
    ++wrong;
    return hipErrorInvalidValue;
  }
  live.erase(it);
  std::free(p);
  ++frees;
  return hipSuccess;
}
void reset() {
  log.clear();
  calls = 0;
  fail_at = 0;
}
}  // namespace fake

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
  fake::log.push_back("malloc");
  return fake::make(p, bytes, fake::kDev, 0);
}
hipError_t hipExtMallocWithFlags(void** p, size_t bytes, unsigned int flags) {
  fake::log.push_back("ext");
  if (flags != hipDeviceMallocFinegrained) ++fake::wrong;
  return fake::make(p, bytes, fake::kExt, flags);
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int flags) {
  fake::log.push_back("hostmalloc:" + std::to_string(flags));
  return fake::make(p, bytes, fake::kHost, flags);
}
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned int) {
  fake::log.push_back("alias");
  if (fake::trip()) return hipErrorInvalidValue;
  auto it = fake::live.find(h);
  if (it == fake::live.end() || it->second.api != fake::kHost || !(it->second.flags & hipHostMallocMapped)) {
    ++fake::wrong;
    return hipErrorInvalidValue;
  }
  *d = fake::alias_of(h);
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  fake::log.push_back("free");
  return fake::drop(p, false);
}
hipError_t hipHostFree(void* p) {
  fake::log.push_back("hostfree");
  return fake::drop(p, true);
}
hipError_t hipMemsetAsync(void* p, int value, size_t bytes, hipStream_t s) {
  fake::log.push_back("memset");
  if (fake::trip()) return hipErrorInvalidValue;
  auto it = fake::live.find(p);
  if (it == fake::live.end() || it->second.bytes != bytes || s != fake::the_stream) {
    ++fake::wrong;
    return hipErrorInvalidValue;
  }
  std::memset(p, value, bytes);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
  fake::log.push_back("sync");
  if (s != fake::the_stream) ++fake::wrong;
  return fake::trip() ? hipErrorUnknown : hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
}

using raftq_buf::Buffer;
using raftq_buf::Kind;

static int failures = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                              \
    }                                                                          \
  } while (0)

static std::string joined() {
  std::string s;
  for (const auto& e : fake::log) s += (s.empty() ? "" : " ") + e;
  return s;
}
static std::string alloc_log(Kind k) {
  switch (k) {
    case Kind::device: return "malloc";
    case Kind::pinned: return "hostmalloc:" + std::to_string(hipHostMallocDefault);
    case Kind::mapped: return "hostmalloc:" + std::to_string(hipHostMallocMapped) + " alias";
    case Kind::mapped_coherent: return "hostmalloc:" + std::to_string(hipHostMallocMapped | hipHostMallocCoherent) + " alias";
    case Kind::bar: return "ext";
  }
  return "?";
}
static std::string free_log(Kind k) { return k == Kind::device || k == Kind::bar ? "free" : "hostfree"; }

// the buffer holds exactly `cap` bytes of `k`, its pointers are the ones the runtime handed out for this allocation
static void check_holds(const Buffer<>& b, Kind k, size_t cap) {
  CHECK(b.cap == cap && b.kind == k);
  void* owner = k == Kind::device ? b.d : b.h;
  CHECK(owner && fake::live.count(owner) && fake::live[owner].bytes == cap);
  if (k == Kind::device) CHECK(b.h == nullptr);
  if (k == Kind::pinned) CHECK(b.d == nullptr);
  if (k == Kind::mapped || k == Kind::mapped_coherent) CHECK(b.d == fake::alias_of(b.h));  // refreshed on every regrow
  if (k == Kind::bar) CHECK(b.d == b.h);
}
static void check_empty(const Buffer<>& b) { CHECK(b.h == nullptr && b.d == nullptr && b.cap == 0); }

constexpr size_t MiB = (size_t)1 << 20;
// the handle's sizing rules, one row per buffer (DESIGN.md "who owns the memory"): capacity when `need` does not fit `have`
struct Rule {
  const char* name;
  Kind kind;
  std::function<size_t(size_t need, size_t have)> capacity;
  bool sync, zeroed;
  size_t small, large;  // two needs: the second exceeds the first's capacity
};
static const Rule kRules[] = {
    {"stage", Kind::mapped, [](size_t n, size_t h) { return std::max({n, 2 * h, MiB}); }, true, false, 24 * 16, MiB + 1},
    {"adv", Kind::mapped_coherent, [](size_t n, size_t h) { return std::min(std::max({n, 2 * h, (size_t)4096 * 24}), (size_t)65536 * 24); }, true, false, 24 * 8, 4097 * 24},
    {"delta_dev", Kind::device, [](size_t n, size_t) { return std::max(2 * n, MiB); }, true, false, 24 * 16, MiB + 24},
    {"tl", Kind::mapped_coherent, [](size_t n, size_t) { return std::max(n, (size_t)1 << 16); }, true, false, 8704, 270592},
    {"seg_h", Kind::mapped_coherent, [](size_t n, size_t) { return n; }, true, false, 64 * 4, 65 * 4},
    {"seg_d", Kind::device, [](size_t n, size_t) { return n; }, true, false, 64 * 4, 65 * 4},
    {"slot dev", Kind::device, [](size_t n, size_t) { return 2 * std::max(n, MiB); }, true, false, 4096, 2 * MiB + 1},
    {"slot out", Kind::mapped, [](size_t n, size_t) { return std::max(2 * n, MiB); }, false, false, 16 * 64 + 16, MiB + 1},
    {"slot in_h", Kind::pinned, [](size_t n, size_t) { return std::max(2 * n, MiB); }, false, false, 16 * 48, MiB + 1},
    {"slot w_pin", Kind::pinned, [](size_t n, size_t) { return std::max(2 * n, MiB); }, false, false, 16 * 48, MiB + 1},
    {"ld_nowait", Kind::mapped, [](size_t n, size_t) { return std::max(2 * n, (size_t)1 << 16); }, false, false, 16 * 32, (1 << 16) + 32},
    {"wire_dev", Kind::device, [](size_t n, size_t) { return std::max(n + n / 2, MiB); }, true, false, 4096, MiB + 1},
    {"resp_dev", Kind::device, [](size_t n, size_t) { return std::max(n + n / 2, MiB); }, true, true, 4096, MiB + 1},
    {"wire_lb", Kind::device, [](size_t n, size_t) { return n; }, true, true, 32 + 4096 * 24, 32 + 6144 * 24},
};

static hipError_t grow(Buffer<>& b, const Rule& r, size_t need) {
  const size_t capacity = r.capacity(need, b.cap);
  if (r.zeroed) return b.grow_zeroed(need, capacity, fake::the_stream);
  return b.grow(need, capacity, r.sync ? &fake::the_stream : nullptr);
}

static void lifecycle(const Rule& r) {
  const uint64_t frees0 = fake::frees, allocs0 = fake::allocs;
  {
    Buffer<> b(r.kind);
    const std::string zero = r.zeroed ? " memset" : "";
    fake::reset();
    CHECK(grow(b, r, r.small) == hipSuccess);  // from empty: nothing to wait for, nothing to free
    const size_t cap1 = r.capacity(r.small, 0);
    check_holds(b, r.kind, cap1);
    CHECK(joined() == alloc_log(r.kind) + zero);
    fake::reset();
    CHECK(grow(b, r, r.small) == hipSuccess && grow(b, r, cap1) == hipSuccess);  // fits: no call is made
    CHECK(fake::log.empty());
    check_holds(b, r.kind, cap1);
    CHECK(r.large > cap1);
    fake::reset();
    const size_t cap2 = r.capacity(r.large, cap1);
    CHECK(grow(b, r, r.large) == hipSuccess);  // past the capacity: the stream is waited for BEFORE the free, where the rule says so
    check_holds(b, r.kind, cap2);
    CHECK(joined() == (r.sync ? "sync " : "") + free_log(r.kind) + " " + alloc_log(r.kind) + zero);
    CHECK(fake::live.size() == 1);
    fake::reset();
    CHECK(b.release() == hipSuccess);
    CHECK(joined() == free_log(r.kind));
    check_empty(b);
    fake::reset();
    CHECK(b.release() == hipSuccess && fake::log.empty());  // released twice: nothing happens
    CHECK(grow(b, r, r.small) == hipSuccess);               // ... and the destructor frees what is held
  }
  CHECK(fake::live.empty());
  CHECK(fake::frees - frees0 == 3 && fake::allocs - allocs0 == 3);  // each allocation freed exactly once
  if (failures) std::fprintf(stderr, "  (rule %s)\n", r.name);
}

// the k-th fallible call of a grow fails, for every k: the buffer is empty afterwards, nothing is live, a retry succeeds
static void grow_failures(const Rule& r, bool regrow) {
  for (int k = 1;; ++k) {
    Buffer<> b(r.kind);
    if (regrow) CHECK(grow(b, r, r.small) == hipSuccess);
    fake::reset();
    fake::fail_at = k;
    const hipError_t e = grow(b, r, regrow ? r.large : r.small);
    const bool tripped = fake::calls >= k;
    fake::fail_at = 0;
    if (!tripped) {
      CHECK(e == hipSuccess);
      CHECK(k > 1);
      break;
    }
    CHECK(e != hipSuccess);
    if (regrow && r.sync && k == 1) {
      check_holds(b, r.kind, r.capacity(r.small, 0));  // the wait itself failed: the memory may be in use, it is kept
    } else {
      check_empty(b);
      CHECK(fake::live.empty());
    }
    fake::reset();
    const size_t need = regrow ? r.large : r.small, want = r.capacity(need, b.cap);
    CHECK(grow(b, r, need) == hipSuccess);  // the retry
    check_holds(b, r.kind, want);
    CHECK(fake::live.size() == 1);
  }
  CHECK(fake::live.empty());
}

static void groups() {
  void *a = nullptr, *b = nullptr, *c = nullptr, *pin = nullptr, *pin_d = nullptr, *e = nullptr, *f = nullptr;
  auto make = [&]() {
    return raftq_buf::alloc_group({{&a, 100}, {&b, 400}, {&c, 100, Kind::device, nullptr, false}, {&pin, 256, Kind::mapped, &pin_d}, {&e, 64}, {&f, 4096}}, fake::the_stream);
  };
  for (int k = 1;; ++k) {
    fake::reset();
    fake::fail_at = k;
    const hipError_t err = make();
    const bool tripped = fake::calls >= k;
    fake::fail_at = 0;
    if (!tripped) {
      CHECK(err == hipSuccess && k == 4 * 2 + 1 + 2 + 1);  // four zeroed device arrays, one left as it comes, one mapped block with its alias
      break;
    }
    CHECK(err != hipSuccess);
    CHECK(!a && !b && !c && !pin && !pin_d && !e && !f);  // every pointer of the group is null ...
    CHECK(fake::live.empty());                             // ... and nothing is live
    fake::reset();
    CHECK(make() == hipSuccess);  // the retry
    CHECK(a && b && c && pin && e && f && pin_d == fake::alias_of(pin) && fake::live.size() == 6);
    for (void* p : {a, b, e, f}) CHECK(*(unsigned char*)p == 0);  // zeroed
    CHECK(*(unsigned char*)c == 0xa5);                            // ... but for the one that asked not to be
    raftq_buf::free_device(a, b, c, e, f);
    raftq_buf::free_host(pin);
    pin_d = nullptr;
    CHECK(fake::live.empty() && !a && !f && !pin);
  }
  raftq_buf::free_device(a, b, c, e, f);
  raftq_buf::free_host(pin);
  CHECK(fake::live.empty());
  // one array: a failed memset leaves nothing behind
  void* one = nullptr;
  fake::reset();
  fake::fail_at = 2;
  CHECK(raftq_buf::alloc_filled(&one, 128, 0xff, fake::the_stream) != hipSuccess && !one && fake::live.empty());
  fake::reset();
  CHECK(raftq_buf::alloc_filled(&one, 128, 0xff, fake::the_stream) == hipSuccess && *(unsigned char*)one == 0xff);
  raftq_buf::free_device(one);
  raftq_buf::free_device(one);  // null: nothing happens
  CHECK(fake::live.empty());
}

// the seam: BarRule::can_write stands in for host_can_write's answer
static int probes = 0;
static bool probe_answer = true;
static bool fake_can_write(void* p, size_t bytes) {
  ++probes;
  CHECK(fake::live.count(p) && fake::live[p].api == fake::kExt && fake::live[p].bytes == bytes);
  return probe_answer;
}

static void host_writable() {
  const std::string pinned = alloc_log(Kind::mapped);
  {  // accepted: device memory is kept, later allocations are taken on trust
    raftq_buf::BarRule bar{true, false, fake_can_write};
    raftq_buf::HostWritable w;
    probes = 0, probe_answer = true;
    fake::reset();
    CHECK(w.grow(100, MiB, &fake::the_stream, bar) == hipSuccess);
    CHECK(joined() == "ext" && probes == 1 && bar.staging && bar.probed);
    CHECK(w.in_device());
    check_holds(w, Kind::bar, MiB);
    CHECK(w.holds_in_device(w.h, MiB) && !w.holds_in_device((char*)w.h + 1, MiB) && !w.holds_in_device(&bar, 1));
    fake::reset();
    CHECK(w.grow(MiB, 2 * MiB, &fake::the_stream, bar) == hipSuccess && fake::log.empty());
    CHECK(w.grow(MiB + 1, 2 * MiB, &fake::the_stream, bar) == hipSuccess);
    CHECK(joined() == "sync free ext" && probes == 1);
    check_holds(w, Kind::bar, 2 * MiB);
    fake::reset();
    CHECK(w.release() == hipSuccess && joined() == "free");
  }
  {  // refused: the device memory is freed, the flag cleared, pinned memory used -- and device memory is never tried again
    raftq_buf::BarRule bar{true, false, fake_can_write};
    raftq_buf::HostWritable w;
    probes = 0, probe_answer = false;
    fake::reset();
    CHECK(w.grow(100, MiB, &fake::the_stream, bar) == hipSuccess);
    CHECK(joined() == "ext free " + pinned && probes == 1 && !bar.staging && !bar.probed);
    CHECK(!w.in_device() && !w.holds_in_device(w.h, 1));
    check_holds(w, Kind::mapped, MiB);
    fake::reset();
    CHECK(w.grow(MiB + 1, 2 * MiB, &fake::the_stream, bar) == hipSuccess);
    CHECK(joined() == "sync hostfree " + pinned && probes == 1);
    check_holds(w, Kind::mapped, 2 * MiB);
  }
  {  // device memory alone (a Step slot): refused leaves the buffer empty, and that is no error
    raftq_buf::BarRule bar{true, false, fake_can_write};
    raftq_buf::HostWritable w;
    probe_answer = false;
    fake::reset();
    CHECK(w.grow_bar(100, MiB, nullptr, bar) == hipSuccess);
    CHECK(joined() == "ext free" && !bar.staging);
    check_empty(w);
    fake::reset();
    CHECK(w.grow_bar(100, MiB, nullptr, bar) == hipSuccess && fake::log.empty());  // staging is off: nothing is tried
    check_empty(w);
    bar.staging = true, probe_answer = true;
    CHECK(w.grow_bar(100, MiB, nullptr, bar) == hipSuccess && w.in_device());
    fake::reset();
    CHECK(w.grow_bar(MiB + 1, 4 * MiB, nullptr, bar) == hipSuccess && joined() == "free ext");  // no wait: the slot is idle
  }
  // every k: the allocation of device memory failing means pinned memory; anything else failing leaves the buffer empty
  for (const bool answer : {true, false})
    for (const bool regrow : {false, true})
      for (int k = 1;; ++k) {
        raftq_buf::BarRule bar{true, false, fake_can_write};
        raftq_buf::HostWritable w;
        probe_answer = true;
        if (regrow) CHECK(w.grow(100, MiB, &fake::the_stream, bar) == hipSuccess);
        probe_answer = answer;
        bar.probed = false;
        fake::reset();
        fake::fail_at = k;
        const hipError_t e = w.grow(2 * MiB, 4 * MiB, &fake::the_stream, bar);
        const bool tripped = fake::calls >= k;
        fake::fail_at = 0;
        if (!tripped) {
          CHECK(e == hipSuccess);
          break;
        }
        if (e == hipSuccess) {  // it was the device allocation that failed
          CHECK(!bar.staging);
          check_holds(w, Kind::mapped, 4 * MiB);
        } else if (regrow && k == 1) {
          check_holds(w, Kind::bar, MiB);  // the wait failed: kept
        } else {
          check_empty(w);
          CHECK(fake::live.empty());
        }
        fake::reset();
        CHECK(w.grow(2 * MiB, 4 * MiB, &fake::the_stream, bar) == hipSuccess && w.cap == 4 * MiB && fake::live.size() == 1);
      }
  CHECK(fake::live.empty());
}

int main() {
  static_assert(!std::is_copy_constructible<Buffer<>>::value && !std::is_copy_assignable<Buffer<>>::value, "a buffer is not copyable");
  static_assert(!std::is_copy_constructible<raftq_buf::HostWritable>::value, "a buffer is not copyable");
  for (const Rule& r : kRules) {
    lifecycle(r);
    grow_failures(r, false);
    grow_failures(r, true);
  }
  groups();
  host_writable();
  CHECK(fake::wrong == 0);
  CHECK(fake::live.empty());
  CHECK(fake::allocs == fake::frees);
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("ok: %llu allocations, each freed once\n", (unsigned long long)fake::allocs);
  return 0;
}
