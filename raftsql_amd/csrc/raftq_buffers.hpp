// raftq_buffers.hpp -- who owns the memory a handle grows or allocates lazily.  Host code only: the HIP runtime's API and the
// standard library, no kernels, no raftq_t.  Every function takes the stream it needs and returns hipError_t (callers wrap
// them in HIPCHK); tests/c/buffers_host.cpp runs the whole header against a fake runtime.
//   Buffer<T>        a growable buffer of one memory kind that owns its memory
//   HostWritable     ... device memory behind the BAR where this process can store into it, pinned memory elsewhere
//   alloc_group      the fixed, lazily allocated arrays (raw pointers: kernel arguments all over): all of a group or none
#pragma once
#include <hip/hip_runtime_api.h>

#include <fcntl.h>
#include <unistd.h>
#include <cerrno>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

// (hidden: none of this is part of what the library exports)
namespace raftq_buf __attribute__((visibility("hidden"))) {

enum class Kind : uint8_t {
  device,           // hipMalloc
  pinned,           // hipHostMallocDefault: the runtime's copies go through it, no kernel addresses it
  mapped,           // pinned and device-mapped: kernels address it over PCIe through the alias
  mapped_coherent,  // ... fine-grained: the device's stores go out as they are issued (what the host reads while a kernel runs)
  bar,              // fine-grained DEVICE memory the host writes through the BAR (HostWritable only): one pointer for both sides
};

// one allocation of `kind`: *h what the host addresses, *d what the kernels address (nullptr where that side has no access).
// All or nothing: on failure both are null and nothing is held.
inline hipError_t alloc_kind(Kind kind, size_t bytes, void** h, void** d) {
  *h = *d = nullptr;
  if (kind == Kind::device) return hipMalloc(d, bytes);
  if (kind == Kind::bar) {
    const hipError_t e = hipExtMallocWithFlags(d, bytes, hipDeviceMallocFinegrained);
    if (e == hipSuccess) *h = *d;
    else *d = nullptr;
    return e;
  }
  const unsigned flags = kind == Kind::pinned   ? hipHostMallocDefault
                         : kind == Kind::mapped ? hipHostMallocMapped
                                                : hipHostMallocMapped | hipHostMallocCoherent;
  hipError_t e = hipHostMalloc(h, bytes, flags);
  if (e != hipSuccess) {
    *h = nullptr;
    return e;
  }
  if (kind == Kind::pinned) return hipSuccess;
  e = hipHostGetDevicePointer(d, *h, 0);
  if (e != hipSuccess) {
    (void)hipHostFree(*h);
    *h = *d = nullptr;
  }
  return e;
}
inline hipError_t free_kind(Kind kind, void* h, void* d) {
  if (!h && !d) return hipSuccess;
  return kind == Kind::device || kind == Kind::bar ? hipFree(d) : hipHostFree(h);
}

// A buffer whose contents are not kept across a regrow.  h / d: the host's and the device's pointer (see alloc_kind), cap: bytes.
// Either it holds `cap` bytes or it is empty (null, null, 0): a failed grow never leaves it dangling or half-set.
template <typename T = void>
struct Buffer {
  T* h = nullptr;
  T* d = nullptr;
  size_t cap = 0;
  Kind kind;

  explicit Buffer(Kind k) : kind(k) {}
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { (void)release(); }

  hipError_t release() {
    const hipError_t e = free_kind(kind, h, d);
    h = d = nullptr;
    cap = 0;
    return e;
  }
  // At least `need` bytes: nothing happens when they fit.  Otherwise `sync` (unless nullptr: the caller knows the memory idle)
  // is waited for -- kernels of earlier calls may still use the memory --, the memory is freed and `capacity` bytes are
  // allocated.  The sizing rule is the caller's: it passes the capacity it wants.
  hipError_t grow(size_t need, size_t capacity, const hipStream_t* sync) {
    if (need <= cap) return hipSuccess;
    if (hipError_t e = vacate(sync); e != hipSuccess) return e;
    return take(kind, capacity);
  }
  // ... a fresh buffer is zeroed on `stream`, which is also the one waited for (device memory)
  hipError_t grow_zeroed(size_t need, size_t capacity, hipStream_t stream) {
    if (need <= cap) return hipSuccess;
    if (hipError_t e = grow(need, capacity, &stream); e != hipSuccess) return e;
    const hipError_t e = hipMemsetAsync(d, 0, cap, stream);
    if (e != hipSuccess) (void)release();
    return e;
  }

 protected:
  hipError_t vacate(const hipStream_t* sync) {
    if (!h && !d) return hipSuccess;
    if (sync)
      if (hipError_t e = hipStreamSynchronize(*sync); e != hipSuccess) return e;
    return release();
  }
  hipError_t take(Kind k, size_t capacity) {
    void *nh = nullptr, *nd = nullptr;
    const hipError_t e = alloc_kind(k, capacity, &nh, &nd);
    if (e != hipSuccess) return e;
    kind = k;
    h = (T*)nh;
    d = (T*)nd;
    cap = capacity;
    return hipSuccess;
  }
};

// Can this process really store into `p` (device memory behind the BAR)?  hipDeviceAttributeIsLargeBar says the aperture
// exists; whether the allocation is mapped writable into THIS process is read off /proc/self/maps -- no store is tried
// and no signal handler is touched.  (Round 2 probed with a guarded store and a temporary SIGSEGV / SIGBUS handler that
// siglongjmp'd out of the fault: undefined behaviour in a host with other threads that use those signals -- the Go
// runtime this library is meant to sit under requires SA_ONSTACK handlers, a JVM installs its own)
inline bool host_can_write(void* p, size_t bytes) {
  const uintptr_t lo = (uintptr_t)p, hi = lo + bytes;
  std::FILE* f = std::fopen("/proc/self/maps", "r");
  if (!f) return false;  // cannot tell: stay on pinned host memory
  char line[512];
  uintptr_t covered = lo;  // [lo, covered) is mapped writable so far (maps is sorted by address)
  while (covered < hi && std::fgets(line, sizeof line, f)) {
    unsigned long long a = 0, b = 0;
    char perms[8] = {0};
    if (std::sscanf(line, "%llx-%llx %7s", &a, &b, perms) != 3) continue;
    if ((uintptr_t)b <= covered) continue;
    if ((uintptr_t)a > covered) break;           // a hole in front of the next mapping
    if (perms[0] != 'r' || perms[1] != 'w') break;  // mapped, but not for stores
    covered = (uintptr_t)b;
  }
  std::fclose(f);
  if (covered < hi) return false;
  // Mapped "rw" is not yet "a store works": in some containers / VMs the aperture is mapped and a store to it still faults
  // (ADVICE r03).  Try one without risking a signal: a one-byte pwrite through /proc/self/mem goes through the kernel's
  // access path and FAILS (EFAULT / EIO) where a store would have raised SIGBUS.  The buffer is fresh and about to be
  // overwritten by its producer, so the byte written does not matter.  Three outcomes: written -> device staging;
  // refused with EFAULT -> pinned host staging; the probe itself unavailable (no /proc/self/mem, EPERM, EIO: the mapping
  // has no access method) -> the maps answer stands.  RAFTQ_STAGE=host forces pinned staging whatever is found here.
  const int fd = ::open("/proc/self/mem", O_WRONLY | O_CLOEXEC);
  if (fd < 0) return true;
  const char zero = 0;
  bool ok = true;
  for (const uintptr_t at : {lo, hi - 1}) {
    if (::pwrite(fd, &zero, 1, (off_t)at) == 1) continue;
    if (errno == EFAULT) ok = false;
    break;
  }
  ::close(fd);
  return ok;
}

// What a handle knows about device memory behind the BAR.  `staging`: decided at create (large BAR present and not disabled),
// cleared for good by the first allocation this process turns out not to be able to store into; `probed`: such memory has been
// found mapped writable into this process once, later allocations are taken on trust; `can_write`: the probe (the tests' seam).
struct BarRule {
  bool staging = false;
  bool probed = false;
  bool (*can_write)(void*, size_t) = host_can_write;
};

// The buffer a producer on the host fills and the kernels read: in HBM where the host can write it, in pinned memory elsewhere.
// It knows which one it got (in_device).
struct HostWritable : Buffer<void> {
  HostWritable() : Buffer<void>(Kind::mapped) {}
  bool in_device() const { return h && kind == Kind::bar; }
  // the producer's stores into device memory are write-combined: drain them before the doorbell
  void publish() const {
#if defined(__x86_64__)
    if (in_device()) __builtin_ia32_sfence();
#endif
  }
  // [p, p + bytes) lies in this buffer and the buffer is device memory
  bool holds_in_device(const void* p, size_t bytes) const {
    return in_device() && (const uint8_t*)p >= (const uint8_t*)h && (const uint8_t*)p + bytes <= (const uint8_t*)h + cap;
  }
  // grow() over device memory alone: afterwards the buffer holds `capacity` bytes of it, or -- this process cannot store into
  // such memory: bar.staging is cleared -- it is empty.  For a caller that has its pinned memory elsewhere.
  hipError_t grow_bar(size_t need, size_t capacity, const hipStream_t* sync, BarRule& bar) {
    if (need <= cap) return hipSuccess;
    if (hipError_t e = vacate(sync); e != hipSuccess) return e;
    if (!bar.staging) return hipSuccess;
    if (take(Kind::bar, capacity) == hipSuccess) {
      if (bar.probed || bar.can_write(h, capacity)) {
        bar.probed = true;
        return hipSuccess;
      }
      (void)release();
    }
    (void)hipGetLastError();
    bar.staging = false;  // no host-writable device memory here: pinned host memory from now on
    if (std::getenv("RAFTQ_PROFILE"))
      std::fprintf(stderr, "[raftq] the ack / inbound staging stays in pinned host memory: device memory behind the BAR is not "
                           "host-writable here (RAFTQ_STAGE=host asks for this outright)\n");
    return hipSuccess;
  }
  hipError_t grow(size_t need, size_t capacity, const hipStream_t* sync, BarRule& bar) {
    if (need <= cap) return hipSuccess;
    if (hipError_t e = grow_bar(need, capacity, sync, bar); e != hipSuccess || h) return e;
    return take(Kind::mapped, capacity);
  }
};

// ---- the fixed arrays: allocated once, raw pointers in the handle ------------------------------------------------------------
// *p: `bytes` of device memory as it comes; left null on failure
inline hipError_t alloc_device(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) *p = nullptr;
  return e;
}
// ... filled with `value` on `stream`; left null when either step fails
inline hipError_t alloc_filled(void** p, size_t bytes, int value, hipStream_t stream) {
  hipError_t e = alloc_device(p, bytes);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(*p, value, bytes, stream);
  if (e != hipSuccess) {
    (void)hipFree(*p);
    *p = nullptr;
  }
  return e;
}
inline hipError_t alloc_zeroed(void** p, size_t bytes, hipStream_t stream) { return alloc_filled(p, bytes, 0, stream); }

// One array of a group: zeroed device memory unless a kind says otherwise; `alias` gets a mapped kind's device pointer;
// zero = false: device memory that the caller's own kernel initialises.
struct Array {
  void** p;
  size_t bytes;
  Kind kind = Kind::device;
  void** alias = nullptr;
  bool zero = true;
};
inline void free_array(const Array& a) {
  (void)free_kind(a.kind, *a.p, *a.p);
  *a.p = nullptr;
  if (a.alias) *a.alias = nullptr;
}
// Every array of the group is allocated (device memory: and its memset enqueued), or none is: those already made are freed and
// nulled.  A caller may therefore test ANY pointer of the group for "the group exists".
inline hipError_t alloc_group(std::initializer_list<Array> group, hipStream_t stream) {
  for (const Array& a : group) {
    hipError_t e;
    if (a.kind == Kind::device) {
      e = a.zero ? alloc_zeroed(a.p, a.bytes, stream) : alloc_device(a.p, a.bytes);
    } else {
      void* d = nullptr;
      e = alloc_kind(a.kind, a.bytes, a.p, &d);
      if (a.alias) *a.alias = d;
    }
    if (e == hipSuccess) continue;
    for (const Array& b : group) {
      if (&b == &a) break;
      free_array(b);
    }
    return e;
  }
  return hipSuccess;
}

// teardown of fixed arrays: the matching free, the pointers nulled
template <typename... T>
inline void free_device(T*&... p) {
  (((void)hipFree((void*)p), p = nullptr), ...);
}
template <typename... T>
inline void free_host(T*&... p) {
  ((p ? (void)hipHostFree((void*)p) : (void)0, p = nullptr), ...);
}

}  // namespace raftq_buf
