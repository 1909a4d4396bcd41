// raftq_wire.hip -- implementation of include/raftq_wire.h: batched raftpb.Message stream frames
// and walpb.Record WAL frames on the GPU (raftq_wire_kernels.hpp).  Host side: move the caller's
// buffers to the device, run the launch chain on the handle's stream, move the results back.
// No CPU path: without the handle's GPU nothing here encodes or decodes a byte
// (raftq_wire_scan_frames, the serial length-word walk, is the one host-only entry point).
#include "raftq_wire.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "raftq_beat_kernels.hpp"
#include "raftq_elect_kernels.hpp"
#include "raftq_internal.hpp"
#include "raftq_propose_kernels.hpp"
#include "raftq_respond_kernels.hpp"
#include "raftq_wire_kernels.hpp"

using namespace raftqk;
using raftq_detail::fail;
using raftq_detail::use_device;

static_assert(sizeof(raftq_wire_msg_t) == sizeof(WireMsg) && sizeof(raftq_wire_ent_t) == sizeof(WireEnt) &&
                  sizeof(raftq_wal_rec_t) == sizeof(WalRec) && sizeof(raftq_prop_t) == sizeof(PropRec) && sizeof(raftq_prop_ent_t) == sizeof(PropEnt),
              "ABI struct mismatch");

namespace {

constexpr uint64_t kMaxItems = 0x7ffffffeull;  // batch positions travel as 31-bit values

// The pinned result block (h->wire_pin, 32 words; h->wire_pin_d as the device addresses it).  Up to three users have results in
// it at a time, each four words behind its base; a kernel is handed wire_pin_d + base and knows the words as pin[0 .. 3].
enum : uint32_t {
  kPinCall = 0,        // the call that is waiting (raftq_step_frames_respond: its decoder)
  kPinWalPending = 8,  // a raftq_wal_encode_begin whose _end has not come: the call enqueued behind it uses the words at kPinCall
  kPinRespond = 16,    // raftq_step_frames_respond's encoder
};
enum : uint32_t {
  kPinTotal = 0,    // bytes written (encoders), entry headers found (raftq_wire_decode*), valid records (raftq_wal_decode)
  kPinRefused = 1,  // records refused (encoders), malformed frames (raftq_wire_decode*); raftq_wal_decode: the running CRC
  kPinThird = 2,    // the chain's last CRC (WAL encoders), wide records (the narrow decode forms)
  kPinGaveUp = 3,   // streaming kernels only: a look-back waited a second and gave up (tile_ctl_check)
  kPinMembers = 4,  // behind kPinCall only: the frames raftq_tick_frames / raftq_tick_elect_frames / raftq_propose_frames built for members (members_tail_kernel)
};

size_t align256(size_t x) { return (x + 255) / 256 * 256; }

struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += align256(bytes + 16);  // 16 bytes of slack behind every byte buffer
    return o;
  }
};

constexpr uint64_t kLbHead = 4;  // words in front of the look-back block's status arrays

// How the codecs' device buffers grow: half as large again as what is asked for, a megabyte at least; a buffer that is too small
// is freed after a stream synchronisation (kernels of earlier calls may still use it), its contents are not kept.
size_t grown(size_t want) { return std::max(want + want / 2, (size_t)1 << 20); }
int grow(raftq_t* h, raftq_buf::Buffer<>& buf, size_t want) {
  HIPCHK(h, buf.grow(want, grown(want), &h->stream));
  return RAFTQ_OK;
}

int ensure_pin(raftq_t* h) {
  if (h->wire_pin) return RAFTQ_OK;
  // both or neither (wire_tail_kernel leaves a used word of wire_flags zero again)
  HIPCHK(h, raftq_buf::alloc_group({{(void**)&h->wire_pin, 256, raftq_buf::Kind::mapped, (void**)&h->wire_pin_d}, {(void**)&h->wire_flags, 64}},
                                   h->stream));
  return RAFTQ_OK;
}

// the address the device has for caller memory, or nullptr when it has none (pageable memory: the runtime's copies then)
void* dev_view(const void* p) {
  if (!p) return nullptr;
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, const_cast<void*>(p), 0) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return d;
}

// The caller's arrays as the device addresses them, and whether the streaming form can take them: `ok` stays true while every
// array asked for is page-locked, mapped and 16-byte aligned (the kernels move whole 16-byte quads -- raftq_wire.h "odd
// alignment").  `pre`: the call's own conditions (its size limits, RAFTQ_WIRE_STREAMING); nothing is looked up once ok is false.
struct Views {
  bool ok;
  explicit Views(bool pre = true) : ok(pre) {}
  // an array the call reads or writes; used == false: the call does not touch it (an empty input, an output nobody wants)
  void* add(const void* p, bool used = true) {
    if (!used || !ok) return nullptr;
    void* v = dev_view(p);
    ok = v != nullptr && ((uintptr_t)v & 15) == 0;
    return v;
  }
  void* opt(const void* p) { return add(p, p != nullptr); }  // an array the caller may leave out
};

unsigned blocks_for(uint64_t lanes) { return (unsigned)((lanes + kBlock - 1) / kBlock); }

// the stream's length as the boundaries give it
uint64_t span_of(const uint64_t* frame_off, uint64_t n) { return frame_off[n] >= frame_off[0] ? frame_off[n] - frame_off[0] : 0; }

// ---- the streaming form (one persistent kernel per call; raftq_wire_kernels.hpp) -----------------------------------
bool streaming_on() {  // RAFTQ_WIRE_STREAMING=0: the copying form even for page-locked buffers (for A/B and the tests)
  const char* e = std::getenv("RAFTQ_WIRE_STREAMING");  // (read per call: the tests switch forms inside one process)
  return !(e && e[0] == '0');
}
// Worker workgroups of a streaming kernel (RAFTQ_WIRE_WGS overrides): a tile is ~25 us of dependent work (flags, scratch
// reads, the parse at one wave per SIMD, the look-back), the link moves a tile every ~0.3 us.
unsigned fused_grid(uint32_t n_tiles) {
  const char* e = std::getenv("RAFTQ_WIRE_WGS");  // read per call: the tests drive tiny grids through one process
  const long v = e ? std::strtol(e, nullptr, 10) : 0;
  return std::min<unsigned>(v > 0 && v <= 4096 ? (unsigned)v : 208u, n_tiles);
}
// frames per tile = threads per workgroup of the streaming decoder (raftq_wire_kernels.hpp wire_dec_fused_kernel)
constexpr unsigned kDecTile = 256;

// reader workgroups of a streaming kernel (RAFTQ_WIRE_READERS overrides): 48 pull a caller's array at 55 GB/s, more are slower
// RAFTQ_WIRE_READERS=0: NO reader workgroups -- every chunk is brought in by a worker that found nobody else doing it (the
// liveness argument's limit case, tests/test_wire_gpu.py::test_streaming_codecs_without_readers).
unsigned fused_readers(uint32_t chunks) {
  const char* e = std::getenv("RAFTQ_WIRE_READERS");
  char* end = nullptr;
  const long v = e ? std::strtol(e, &end, 10) : -1;
  if (e && end != e && v == 0) return 0;
  return std::min<unsigned>(v > 0 && v <= 1024 ? (unsigned)v : 48u, chunks);
}
// bytes of all arrays together that a reader brings in before it raises a flag
constexpr uint64_t kFeedChunk = 8192;

// One launch of a streaming kernel: what the caller asks for, and what stream_prepare answers.
struct StreamCall {
  // -- the request --
  uint32_t n_tiles = 0;
  struct Seg {
    const void* src;  // the caller's array as the device addresses it (16-byte aligned), or nullptr
    uint64_t bytes;   // ... and its size: what the readers bring into the scratch
    uint64_t extra;   // bytes that follow it in the scratch: records a kernel of the call writes there itself
  } seg[3] = {};
  size_t carve[2] = {0, 0};  // further scratch of the call's kernels, n_carves pieces
  int n_carves = 0;
  uint64_t out_bytes = 0;  // what h->wire_out.d has to hold (0: the kernel does not use it)
  size_t keep = 0;         // bytes at the front of the scratch the call leaves alone: an earlier launch's, which a kernel of this one reads
  // -- the answer --
  InFeed in{};
  TileCtl ctl;
  unsigned workers = 0;
  dim3 grid;           // readers + workers
  uint8_t* carved[2];  // the pieces asked for
  size_t off[5];       // (where the segments and the pieces lie in h->wire_dev.d)
};

// ticket word + status arrays for one launch: a new launch is a new epoch (the words of older ones read as "not published
// yet"); the arrays are zeroed again when the 16-bit epoch wraps
int tile_ctl(raftq_t* h, TileCtl* ctl) {
  if (++h->wire_epoch > 0xffffu) {
    HIPCHK(h, hipMemsetAsync(h->wire_lb.d + kLbHead, 0, kLbArrays * h->wire_lb_tiles * 8, h->stream));
    h->wire_epoch = 1;
  }
  ctl->ticket = reinterpret_cast<unsigned int*>(h->wire_lb.d);
  ctl->ticket_base = h->wire_ticket_base;
  ctl->epoch = h->wire_epoch;
  for (int k = 0; k < kLbArrays; ++k) ctl->status[k] = h->wire_lb.d + kLbHead + (uint64_t)k * h->wire_lb_tiles;
  return RAFTQ_OK;
}
// every worker of a launch draws exactly one ticket beyond the tiles
void tile_ctl_launched(raftq_t* h, uint32_t n_tiles, unsigned workers) {
  h->wire_ticket_base += n_tiles + workers;
  h->wire_chunk_base += h->wire_chunk_pending;
  h->wire_chunk_pending = 0;
}
// after the call's wait: did a look-back give up (kPinGaveUp, copied from the control block by the last tile)?
int tile_ctl_check(raftq_t* h, const char* who, uint32_t pin_base) {
  if (h->wire_pin[pin_base + kPinGaveUp] == 0) return RAFTQ_OK;
  h->wire_lb_tiles = 0;  // the control block is not trusted any more: the next call allocates a fresh one
  return fail(h, RAFTQ_EHIP, std::string(who) + ": a workgroup waited a second for its predecessor's tile and gave up; the results are not valid");
}

// The readers' plan for the call's arrays: how many chunks (at most max_chunks, the flags available), how many bytes of every
// array per chunk.
void plan_feed(StreamCall& sc, uint64_t max_chunks) {
  uint64_t total = 0;
  for (int k = 0; k < 3; ++k) total += sc.seg[k].bytes;
  const uint64_t chunks = std::max<uint64_t>(1, std::min<uint64_t>(max_chunks, (total + kFeedChunk - 1) / kFeedChunk));
  for (int k = 0; k < 3; ++k) {
    sc.in.seg[k].src = (const uint8_t*)sc.seg[k].src;
    sc.in.seg[k].bytes = sc.seg[k].bytes;
    sc.in.seg[k].per_chunk = std::max<uint64_t>(256, ((sc.seg[k].bytes + chunks - 1) / chunks + 255) / 256 * 256);
  }
  sc.in.chunks = (uint32_t)chunks;
  sc.in.readers = fused_readers(sc.in.chunks);
}
// The chunk ticket is monotonic across calls: a launch with reader workgroups draws exactly chunks + readers tickets whoever
// copies what (a worker that serves itself claims by compare-and-swap and never draws past the end; the readers draw the rest
// and one beyond each), so the next call's base is known without asking the device.  A launch with NO readers (RAFTQ_WIRE_READERS=0)
// only claims the chunks somebody waited for -- a chunk past every array's end, or one that holds bytes no tile
// names, stays unclaimed -- so its count is not known: the ticket word is zeroed in front of such a launch and in front of the
// first launch after one (a 4-byte memset in the stream: test and A/B shapes only).
int bind_feed(raftq_t* h, StreamCall& sc) {
  for (int k = 0; k < 3; ++k) sc.in.seg[k].dst = (uint8_t*)h->wire_dev.d + sc.off[k];
  sc.in.flag = sc.ctl.status[kLbFlags];
  sc.in.chunk_ticket = reinterpret_cast<unsigned int*>(h->wire_lb.d + 3);  // the head's fourth word
  if (sc.in.readers == 0 || h->wire_chunk_unknown) {
    HIPCHK(h, hipMemsetAsync(sc.in.chunk_ticket, 0, 4, h->stream));
    h->wire_chunk_base = 0;
    h->wire_chunk_unknown = sc.in.readers == 0;
  }
  sc.in.chunk_base = h->wire_chunk_base;
  h->wire_chunk_pending = sc.in.readers ? sc.in.chunks + sc.in.readers : 0;  // every reader workgroup draws exactly one ticket beyond the chunks
  return RAFTQ_OK;
}

// The launch sequence of every streaming call: stream_prepare, the call's own kernels, stream_launch.  Its order is a protocol:
//   1. the control block is sized first (a status word per tile and a flag per kFeedChunk of input): plan_feed takes its
//      number of chunks from h->wire_lb_tiles;
//   2. the scratch is carved -- the segments with their extras, the call's own pieces behind them -- and, with the output
//      buffer, grown: that may move either, so nothing holds an address into them before;
//   3. only then is the launch's epoch drawn and the feed bound to the scratch (tile_ctl, bind_feed);
//   4. the launch is accounted for exactly once, with its own tile and worker counts (tile_ctl_launched): the tile and chunk
//      tickets are monotonic across calls, and a launch counted wrongly derails every later call on the handle.
// stream_reserve is steps 1 and 2 alone: after it, a stream_prepare of the same request (or a smaller one) allocates nothing.
int stream_reserve(raftq_t* h, StreamCall& sc) {
  uint64_t total = 0;
  for (int k = 0; k < 3; ++k) total += sc.seg[k].bytes;
  const uint64_t n_status = std::max<uint64_t>(sc.n_tiles, total / kFeedChunk + 1);
  if (n_status > h->wire_lb_tiles) {  // a fresh control block is all zero: tickets and epochs start over
    // capacity in status words per array: bytes = head + arrays x words x 8, zeroed.  The block in hand is replaced whatever its
    // size: it is too small, or not trusted any more (tile_ctl_check)
    const uint64_t words = std::max<uint64_t>(n_status + n_status / 2, 4096);
    const size_t bytes = kLbHead * 8 + words * kLbArrays * 8;
    h->wire_lb_tiles = 0;
    if (h->wire_lb.d) {
      HIPCHK(h, hipStreamSynchronize(h->stream));
      HIPCHK(h, h->wire_lb.release());
    }
    HIPCHK(h, h->wire_lb.grow_zeroed(bytes, bytes, h->stream));
    h->wire_lb_tiles = words;
    h->wire_ticket_base = h->wire_chunk_base = h->wire_epoch = 0;
    h->wire_chunk_unknown = false;
  }
  Carver c;
  c.off = sc.keep;
  for (int k = 0; k < 3; ++k) sc.off[k] = c.take(sc.seg[k].bytes + sc.seg[k].extra);
  for (int k = 0; k < sc.n_carves; ++k) sc.off[3 + k] = c.take(sc.carve[k]);
  if (int rc = grow(h, h->wire_dev, c.off)) return rc;
  return grow(h, h->wire_out, sc.out_bytes);
}
int stream_prepare(raftq_t* h, StreamCall& sc) {
  if (int rc = stream_reserve(h, sc)) return rc;
  if (int rc = tile_ctl(h, &sc.ctl)) return rc;
  plan_feed(sc, h->wire_lb_tiles);
  if (int rc = bind_feed(h, sc)) return rc;
  for (int k = 0; k < sc.n_carves; ++k) sc.carved[k] = (uint8_t*)h->wire_dev.d + sc.off[3 + k];
  sc.workers = fused_grid(sc.n_tiles);
  sc.grid = dim3(sc.in.readers + sc.workers);
  return RAFTQ_OK;
}
// the streaming kernel itself, enqueued on the handle's stream behind whatever the call launched in front of it
template <class Kernel, class... Args>
int stream_launch(raftq_t* h, const StreamCall& sc, Kernel kernel, unsigned block, Args... args) {
  hipLaunchKernelGGL(kernel, sc.grid, dim3(block), 0, h->stream, args...);
  HIPCHK(h, hipGetLastError());
  tile_ctl_launched(h, sc.n_tiles, sc.workers);
  return RAFTQ_OK;
}

// ---- the copying form (pageable caller memory: the runtime's copies, a chain of plain kernels) -------------------------
// totals / flags of the call -> wire_pin[kPinTotal], [kPinRefused] (read after the next hipStreamSynchronize)
int tail_to_pin(raftq_t* h, const uint64_t* total, unsigned long long* flag) {
  hipLaunchKernelGGL(wire_tail_kernel, dim3(1), dim3(64), 0, h->stream, total, flag, h->wire_pin_d + kPinCall);
  HIPCHK(h, hipGetLastError());
  return RAFTQ_OK;
}

// chain[i] = pair[0] . pair[1] . ... . pair[i]; tot: scratch for ceil(n / kBlock) pairs
int crc_chain_scan(raftq_t* h, const CrcPair* pair, CrcPair* chain, uint64_t n, CrcPair* tot) {
  const unsigned nb = blocks_for(n);
  hipLaunchKernelGGL(crc_scan_blocks_kernel, dim3(nb), dim3(kBlock), 0, h->stream, pair, chain, n, tot);
  if (nb > 1)
    hipLaunchKernelGGL(crc_scan_apply_kernel, dim3(nb), dim3(kBlock), 0, h->stream, chain, n, (const CrcPair*)tot);
  HIPCHK(h, hipGetLastError());
  return RAFTQ_OK;
}

int h2d(raftq_t* h, void* dst, const void* src, size_t bytes) {
  if (bytes) HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
  return RAFTQ_OK;
}
int d2h(raftq_t* h, void* dst, const void* src, size_t bytes) {
  if (bytes) HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  return RAFTQ_OK;
}

// ---- raftq_wire_encode ------------------------------------------------------------------------------------------------
// What either form of an encoder learns once the sizes are known: a refusal (`state`: what that means for out), the size for the
// caller, out too small.  who: raftq_wire_encode, or a WAL encoder with its own `what`.
template <class Counts>
int encode_sized(raftq_t* h, const char* who, const char* what, const char* state, uint64_t total, uint64_t refused, uint64_t cap, Counts* counts,
                 const Counts& sized) {
  if (refused) return fail(h, RAFTQ_EINVAL, std::string(who) + what + state);
  if (counts) *counts = sized;
  if (total > cap) return fail(h, RAFTQ_EINVAL, std::string(who) + ": out is too small (counts->bytes is the size needed)");
  return RAFTQ_OK;
}
constexpr const char* kWireEncRefused = ": a message has to / from >= 255, an entry range outside ents[], or a payload outside the pool; ";
constexpr const char* kWalEncRefused = ": a record has an unknown kind or a payload outside the pool; ";

// page-locked caller buffers (v_*: as the device addresses them): readers | workers in one launch (raftq_wire_kernels.hpp)
int wire_encode_streaming(raftq_t* h, const void* v_msgs, uint64_t n, const void* v_ents, uint64_t n_ents, const void* v_pool, uint64_t pool_bytes,
                          void* v_out, uint64_t cap, void* v_off, raftq_wire_counts_t* counts) {
  StreamCall sc;
  sc.n_tiles = blocks_for(n);
  sc.seg[0] = {v_msgs, n * sizeof(WireMsg), 0};
  sc.seg[1] = {v_ents, n_ents * sizeof(WireEnt), 0};
  sc.seg[2] = {v_pool, pool_bytes, 0};
  sc.out_bytes = cap + 16;
  if (int rc = stream_prepare(h, sc)) return rc;
  if (int rc = stream_launch(h, sc, wire_enc_fused_kernel, kBlock, sc.in, n, n_ents, pool_bytes, (uint8_t*)h->wire_out.d, (uint8_t*)v_out, cap,
                             (uint64_t*)v_off, sc.ctl, h->wire_pin_d + kPinCall, (const unsigned int*)nullptr, 0u))
    return rc;
  HIPCHK(h, raftq_detail::wait_call(h));
  if (int rc = tile_ctl_check(h, "raftq_wire_encode", kPinCall)) return rc;
  const uint64_t total = h->wire_pin[kPinCall + kPinTotal];
  return encode_sized(h, "raftq_wire_encode", kWireEncRefused, "the output is not valid", total, h->wire_pin[kPinCall + kPinRefused], cap, counts,
                      raftq_wire_counts_t{n, n_ents, 0, total});
}

// the runtime's copies, a wait in the middle to learn the size
int wire_encode_copying(raftq_t* h, const raftq_wire_msg_t* msgs, uint64_t n, const raftq_wire_ent_t* ents, uint64_t n_ents, const void* pool,
                        uint64_t pool_bytes, void* out, uint64_t cap, uint64_t* frame_off, raftq_wire_counts_t* counts) {
  const size_t scan_bytes = scan_sum_scratch_bytes(n + 1);  // tile totals of the hand-written scan
  Carver c;
  const size_t o_msgs = c.take(n * sizeof(WireMsg)), o_ents = c.take(n_ents * sizeof(WireEnt)),
               o_pool = c.take(pool_bytes), o_sizes = c.take((n + 1) * 8), o_off = c.take((n + 1) * 8), o_scan = c.take(scan_bytes);
  if (int rc = grow(h, h->wire_dev, c.off)) return rc;
  uint8_t* base = (uint8_t*)h->wire_dev.d;
  WireMsg* d_msgs = (WireMsg*)(base + o_msgs);
  WireEnt* d_ents = (WireEnt*)(base + o_ents);
  uint8_t* d_pool = base + o_pool;
  uint64_t *d_sizes = (uint64_t*)(base + o_sizes), *d_off = (uint64_t*)(base + o_off);
  unsigned int* d_bad = (unsigned int*)(h->wire_flags + 0);
  if (int rc = h2d(h, d_msgs, msgs, n * sizeof(WireMsg))) return rc;
  if (int rc = h2d(h, d_ents, ents, n_ents * sizeof(WireEnt))) return rc;
  if (int rc = h2d(h, d_pool, pool, pool_bytes)) return rc;
  hipLaunchKernelGGL(wire_enc_size_kernel, dim3(blocks_for(n + 1)), dim3(kBlock), 0, h->stream, (const WireMsg*)d_msgs, n,
                     (const WireEnt*)d_ents, n_ents, pool_bytes, d_sizes, d_bad);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, exclusive_sum_u64((const uint64_t*)d_sizes, d_off, n + 1, (uint64_t*)(base + o_scan), h->stream));
  if (int rc = tail_to_pin(h, d_off + n, h->wire_flags + 0)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const uint64_t total = h->wire_pin[kPinCall + kPinTotal];
  if (int rc = encode_sized(h, "raftq_wire_encode", kWireEncRefused, "nothing was written", total, (uint32_t)h->wire_pin[kPinCall + kPinRefused], cap,
                            counts, raftq_wire_counts_t{n, n_ents, 0, total}))
    return rc;
  if (int rc = grow(h, h->wire_out, total + 16)) return rc;
  uint8_t* d_out = (uint8_t*)h->wire_out.d;
  hipLaunchKernelGGL(wire_enc_write_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, h->stream, (const WireMsg*)d_msgs, n,
                     (const WireEnt*)d_ents, (const uint64_t*)d_off, d_out);
  if (n_ents)
    hipLaunchKernelGGL(wire_enc_payload_kernel, dim3(blocks_for(n * 64)), dim3(kBlock), 0, h->stream,
                       (const WireMsg*)d_msgs, n, (const WireEnt*)d_ents, (const uint64_t*)d_off,
                       (const uint8_t*)d_pool, d_out);
  HIPCHK(h, hipGetLastError());
  if (int rc = d2h(h, out, d_out, total)) return rc;
  if (frame_off)
    if (int rc = d2h(h, frame_off, d_off, (n + 1) * 8)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return RAFTQ_OK;
}

// ---- raftq_wire_decode, raftq_wire_decode_packed, raftq_step_frames' decoder ------------------------------------------------
// where the streaming decoder's request puts the stream's copy in the scratch, and where that copy ends (raftq_respond_set_props
// lays its marshal out behind it: stream_reserve carves the segments in order)
size_t decode_stream_off(uint64_t n) { return align256((size_t)(n + 1) * 8 + 16); }
size_t decode_stream_end(uint64_t n, uint64_t nbytes) { return decode_stream_off(n) + align256((size_t)nbytes + 16); }
// The streaming decode (raftq_wire_kernels.hpp "the streaming form"), enqueued on the handle's stream and NOT waited for;
// v_*: the caller's arrays as the device addresses them.  msgs_d / ff: see wire_dec_fused_kernel (raftq_step_frames).
// form: 0 -- v_msgs receives 64-byte records; RAFTQ_WIRE_FORM_40 / _HEAD -- v_msgs is the narrow array, pk the wide one.
int decode_streaming_enqueue(raftq_t* h, const void* v_stream, uint64_t nbytes, const void* v_off, uint64_t n, void* v_msgs, void* v_ents,
                             uint64_t ents_cap, WireMsg* msgs_d, FrameFilter ff, int form = 0, PackedOut pk = PackedOut{nullptr, 0, 0, 0}) {
  // (the default of 208 workers, one per CU beside the readers as in round 5 -- at 68 KB two fit, but 464 workers measured SLOWER
  // than 208 (173.9 against 167.6 us a call, profiles/r06/wire_tile_ab.jsonl): with 256 tiles in a 64K-frame call every tile has
  // its own waiting worker at 208 already, and twice the workgroups are twice the pollers of the chunk flags)
  StreamCall sc;
  sc.n_tiles = (uint32_t)((n + kDecTile - 1) / kDecTile);
  sc.seg[0] = {v_off, (n + 1) * 8, 0};
  sc.seg[1] = {v_stream, nbytes, 0};
  sc.carve[0] = (size_t)sc.n_tiles * kDecTile * kEntQ * sizeof(WireEnt);  // a slot of kEntQ entry headers per lane
  sc.n_carves = 1;
  if (int rc = stream_prepare(h, sc)) return rc;
  const auto kernel = form == RAFTQ_WIRE_FORM_40     ? wire_dec_fused_kernel<kDecTile, RAFTQ_WIRE_FORM_40>
                      : form == RAFTQ_WIRE_FORM_HEAD ? wire_dec_fused_kernel<kDecTile, RAFTQ_WIRE_FORM_HEAD>
                                                     : wire_dec_fused_kernel<kDecTile, 0>;
  return stream_launch(h, sc, kernel, kDecTile, sc.in, nbytes, n, (WireMsg*)v_msgs, (WireEnt*)v_ents, ents_cap, sc.ctl, h->wire_pin_d + kPinCall, msgs_d, ff,
                       (WireEnt*)sc.carved[0], pk);
}
// What either form of a decode reports once its totals are in the pinned words.  too_many_is_error: raftq_wire_decode's
// contract; raftq_step_frames only reports the count.
int decode_counted(raftq_t* h, const char* who, const uint64_t* frame_off, uint64_t n, bool have_ents, uint64_t ents_cap, bool too_many_is_error,
                   raftq_wire_counts_t* counts) {
  const uint64_t total = h->wire_pin[kPinCall + kPinTotal];
  if (counts) *counts = raftq_wire_counts_t{n, total, h->wire_pin[kPinCall + kPinRefused], span_of(frame_off, n)};
  if (too_many_is_error && have_ents && total > ents_cap)
    return fail(h, RAFTQ_EINVAL, std::string(who) + ": more entries than ents_cap (counts->n_ents is the number needed)");
  return RAFTQ_OK;
}
// ... the streaming form, after the wait that covers it
int decode_streaming_finish(raftq_t* h, const char* who, const uint64_t* frame_off, uint64_t n, bool have_ents, uint64_t ents_cap,
                            bool too_many_is_error, raftq_wire_counts_t* counts) {
  if (int rc = tile_ctl_check(h, who, kPinCall)) return rc;
  return decode_counted(h, who, frame_off, n, have_ents, ents_cap, too_many_is_error, counts);
}

int wire_decode_copying(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off, uint64_t n, raftq_wire_msg_t* msgs,
                        raftq_wire_ent_t* ents, uint64_t ents_cap, raftq_wire_counts_t* counts) {
  // an entry costs its message at least two bytes (tag, length), so this many can never be exceeded
  const uint64_t dev_cap = std::min<uint64_t>(ents_cap, nbytes / 2 + 1);
  const size_t scan_bytes = scan_sum_scratch_bytes(n + 1);  // tile totals of the hand-written scan
  Carver c;
  const size_t o_stream = c.take(nbytes), o_off = c.take((n + 1) * 8), o_msgs = c.take(n * sizeof(WireMsg)),
               o_cnt = c.take((n + 1) * 8), o_base = c.take((n + 1) * 8), o_scan = c.take(scan_bytes);
  if (int rc = grow(h, h->wire_dev, c.off)) return rc;
  if (int rc = grow(h, h->wire_out, dev_cap * sizeof(WireEnt) + 16)) return rc;
  uint8_t* base = (uint8_t*)h->wire_dev.d;
  uint8_t* d_stream = base + o_stream;
  uint64_t *d_off = (uint64_t*)(base + o_off), *d_cnt = (uint64_t*)(base + o_cnt), *d_base = (uint64_t*)(base + o_base);
  WireMsg* d_msgs = (WireMsg*)(base + o_msgs);
  WireEnt* d_ents = (WireEnt*)h->wire_out.d;
  unsigned long long* d_bad = h->wire_flags + 1;
  if (int rc = h2d(h, d_stream, stream, nbytes)) return rc;
  if (int rc = h2d(h, d_off, frame_off, (n + 1) * 8)) return rc;
  hipLaunchKernelGGL(wire_dec_kernel, dim3(blocks_for(n + 1)), dim3(kBlock), 0, h->stream, (const uint8_t*)d_stream,
                     nbytes, (const uint64_t*)d_off, n, d_msgs, d_cnt, d_bad);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, exclusive_sum_u64((const uint64_t*)d_cnt, d_base, n + 1, (uint64_t*)(base + o_scan), h->stream));
  hipLaunchKernelGGL(wire_dec_ents_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, h->stream, (const uint8_t*)d_stream,
                     nbytes, (const uint64_t*)d_off, n, d_msgs, (const uint64_t*)d_base, dev_cap ? d_ents : (WireEnt*)nullptr,
                     dev_cap);
  HIPCHK(h, hipGetLastError());
  if (int rc = tail_to_pin(h, d_base + n, d_bad)) return rc;
  if (int rc = d2h(h, msgs, d_msgs, n * sizeof(WireMsg))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (int rc = decode_counted(h, "raftq_wire_decode", frame_off, n, ents != nullptr, ents_cap, true, counts)) return rc;
  const uint64_t total = h->wire_pin[kPinCall + kPinTotal];
  if (ents && total) {
    if (int rc = d2h(h, ents, d_ents, total * sizeof(WireEnt))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return RAFTQ_OK;
}

// Broadcasts over each group's own members (raftq_tick_set_voters / raftq_bcast_set_voters with masks loaded; raftq_beat_kernels.hpp,
// raftq_propose_kernels.hpp): the masked build kernels add the frames they built for members to the fifth word of wire_flags, zeroed here in the same submission in front of them ...
unsigned long long* members_word(raftq_t* h) { return h->wire_flags + 4; }
int members_begin(raftq_t* h) {
  HIPCHK(h, hipMemsetAsync(members_word(h), 0, 8, h->stream));
  return RAFTQ_OK;
}
// ... and behind the encoder the sum goes to the pinned block, where the host reads it beside the encoder's totals
int members_end(raftq_t* h) {
  hipLaunchKernelGGL(members_tail_kernel, dim3(1), dim3(64), 0, h->stream, members_word(h), h->wire_pin_d + kPinCall + kPinMembers);
  HIPCHK(h, hipGetLastError());
  return RAFTQ_OK;
}

}  // namespace

void raftq_detail::free_wire_state(raftq_t* h) {
  raftq_buf::free_device(h->wire_flags);
  raftq_buf::free_host(h->wire_pin);
}

// ---- raftpb.Message stream frames: the entry points ---------------------------------------------------------------------------
extern "C" {

int raftq_wire_scan_frames(const void* buf, uint64_t nbytes, int big_endian, uint64_t* off, uint64_t cap,
                           uint64_t* n_frames, uint64_t* consumed) {
  if ((!buf && nbytes) || !off || !n_frames || !consumed) return fail(nullptr, RAFTQ_EINVAL, "raftq_wire_scan_frames: null argument");
  const uint8_t* p = (const uint8_t*)buf;
  uint64_t at = 0, k = 0;
  for (; k < cap && nbytes - at >= 8; ++k) {
    uint64_t len;
    std::memcpy(&len, p + at, 8);  // this library only runs on little-endian hosts
    if (big_endian) len = __builtin_bswap64(len);
    if (len > nbytes - at - 8) break;  // the tail is torn: leave it to the caller
    off[k] = at;
    at += 8 + len;
  }
  off[k] = at;
  *n_frames = k;
  *consumed = at;
  return RAFTQ_OK;
}

int raftq_wire_encode(raftq_t* h, const raftq_wire_msg_t* msgs, uint64_t n, const raftq_wire_ent_t* ents,
                      uint64_t n_ents, const void* pool, uint64_t pool_bytes, void* out, uint64_t cap,
                      uint64_t* frame_off, raftq_wire_counts_t* counts) {
  if (int rc = use_device(h)) return rc;
  if (counts) *counts = raftq_wire_counts_t{0, 0, 0, 0};
  if (n == 0) {
    if (frame_off) frame_off[0] = 0;
    return RAFTQ_OK;
  }
  if (!msgs || (n_ents && !ents) || (pool_bytes && !pool) || (cap && !out))
    return fail(h, RAFTQ_EINVAL, "raftq_wire_encode: null argument");
  if (n > kMaxItems || n_ents > kMaxItems) return fail(h, RAFTQ_EINVAL, "raftq_wire_encode: batch too large");
  if (int rc = ensure_pin(h)) return rc;
  // page-locked caller buffers (what a node passes every turn) take the streaming form; anything else the copying form
  Views v(streaming_on() && cap != 0 && cap <= ((uint64_t)1 << 31));
  void *v_msgs = v.add(msgs), *v_ents = v.add(ents, n_ents != 0), *v_pool = v.add(pool, pool_bytes != 0), *v_out = v.add(out), *v_off = v.opt(frame_off);
  if (v.ok) return wire_encode_streaming(h, v_msgs, n, v_ents, n_ents, v_pool, pool_bytes, v_out, cap, v_off, counts);
  return wire_encode_copying(h, msgs, n, ents, n_ents, pool, pool_bytes, out, cap, frame_off, counts);
}

int raftq_propose_frames(raftq_t* h, const raftq_prop_t* props, uint64_t n_props, const raftq_prop_ent_t* prop_ents, uint64_t n_prop_ents,
                         const raftq_wire_msg_t* msgs, uint64_t n_msgs, const raftq_wire_ent_t* ents, uint64_t n_ents, const void* pool,
                         uint64_t pool_bytes, void* out, uint64_t cap, uint64_t* frame_off, raftq_wire_counts_t* counts) {
  if (int rc = raftq_detail::use_device_idle(h, "raftq_propose_frames")) return rc;
  if (counts) *counts = raftq_wire_counts_t{0, 0, 0, 0};
  if (int rc = raftq_detail::refuse_lead_transfer(h, "raftq_propose_frames")) return rc;
  h->prop_what_n = 0;  // (raftq_propose_outcomes: valid until the next call)
  if (n_props == 0)  // nothing proposed: the marshal of what the caller queued
    return raftq_wire_encode(h, msgs, n_msgs, ents, n_ents, pool, pool_bytes, out, cap, frame_off, counts);
  if (!props || !prop_ents || n_prop_ents == 0 || (n_msgs && !msgs) || (n_ents && !ents) || (pool_bytes && !pool) || !out || cap == 0)
    return fail(h, RAFTQ_EINVAL, "raftq_propose_frames: null argument");
  if (h->N < 2)
    return fail(h, RAFTQ_EINVAL, "raftq_propose_frames: a single-peer group commits what it appends -- raftq_apply_log_deltas reports that");
  const uint64_t n_dev = n_props * (h->N - 1), n = n_msgs + n_dev, n_e = n_ents + n_prop_ents;
  if (n > kMaxItems || n_e > kMaxItems) return fail(h, RAFTQ_EINVAL, "raftq_propose_frames: batch too large");
  if (int rc = ensure_pin(h)) return rc;
  const bool fwd = h->prop_forward;  // raftq_propose_set_forward: the *_fwd_kernel forms, one outcome byte per record
  if (fwd) HIPCHK(h, h->prop_what.grow((n_props + 7) / 8 * 8, std::max<size_t>((n_props + n_props / 2 + 7) / 8 * 8, 4096), &h->stream));
  Views v(cap <= ((uint64_t)1 << 31));
  void *v_props = v.add(props), *v_pe = v.add(prop_ents), *v_msgs = v.add(msgs, n_msgs != 0), *v_ents = v.add(ents, n_ents != 0),
       *v_pool = v.add(pool, pool_bytes != 0), *v_out = v.add(out), *v_off = v.opt(frame_off);
  if (!v.ok)
    return fail(h, RAFTQ_EINVAL, "raftq_propose_frames: every array must be page-locked (raftq_host_alloc, hipHostMalloc, hipHostRegister) and "
                                 "16-byte aligned -- append with raftq_apply_log_deltas and marshal with raftq_wire_encode otherwise");
  NodeArrays na;
  if (int rc = raftq_detail::node_arrays_of(h, &na)) return rc;
  const uint64_t msgs_bytes = n_msgs * sizeof(WireMsg), ents_bytes = n_ents * sizeof(WireEnt);
  StreamCall sc;
  sc.n_tiles = blocks_for(n);
  sc.seg[0] = {v_msgs, msgs_bytes, n_dev * sizeof(WireMsg)};
  sc.seg[1] = {v_ents, ents_bytes, n_prop_ents * sizeof(WireEnt)};
  sc.seg[2] = {v_pool, pool_bytes, 0};
  sc.carve[0] = n_props * sizeof(PropRec);  // the check kernel's copies of the records
  sc.carve[1] = n_prop_ents * sizeof(PropEnt);
  sc.n_carves = 2;
  sc.out_bytes = cap + 16;
  if (int rc = stream_prepare(h, sc)) return rc;
  // what appendEntry + bcastAppend send, built on the device INTO the encoder's input (the scratch behind what its readers bring) ...
  // the validation's verdict: a word that holds THIS call's stamp when a record was refused (no memset in the chain: a stamp
  // of an earlier call reads as "fine")
  unsigned int* bad = (unsigned int*)(h->wire_flags + 2);
  if (++h->prop_stamp == 0) h->prop_stamp = 1;
  const unsigned int stamp = h->prop_stamp;
  WireMsg* msgs_dev = (WireMsg*)(sc.in.seg[0].dst + msgs_bytes);
  WireEnt* ents_dev = (WireEnt*)(sc.in.seg[1].dst + ents_bytes);
  const dim3 pg((unsigned)((n_props + kBlock - 1) / kBlock)), cg((unsigned)((std::max(n_props, n_prop_ents) + kBlock - 1) / kBlock));
  PropRec* props_d = (PropRec*)sc.carved[0];
  PropEnt* pe_d = (PropEnt*)sc.carved[1];
  const bool members = raftq_detail::masked_bcast(h);  // the MsgApps go to each group's own members (propose_check_voters_kernel, propose_build_voters_kernel)
  const bool counted = members || fwd;  // fillers among the device's slots: the build kernel counts the frames that have bytes
  if (counted)
    if (int rc = members_begin(h)) return rc;
  if (fwd && members) {
    hipLaunchKernelGGL(propose_check_fwd_voters_kernel, cg, dim3(kBlock), 0, h->stream, na, (const PropRec*)v_props, n_props, (const PropEnt*)v_pe, n_prop_ents,
                       pool_bytes, bad, stamp, props_d, pe_d, h->wire_flags + 3, (const uint16_t*)h->voters, (uint64_t*)h->prop_what.d);
    hipLaunchKernelGGL(propose_build_fwd_voters_kernel, pg, dim3(kBlock), 0, h->stream, na, (const PropRec*)props_d, n_props, (const PropEnt*)pe_d,
                       (const unsigned int*)bad, stamp, msgs_dev, ents_dev, (uint32_t)n_ents, (const uint16_t*)h->voters, members_word(h));
  } else if (fwd) {
    hipLaunchKernelGGL(propose_check_fwd_kernel, cg, dim3(kBlock), 0, h->stream, na, (const PropRec*)v_props, n_props, (const PropEnt*)v_pe, n_prop_ents,
                       pool_bytes, bad, stamp, props_d, pe_d, h->wire_flags + 3, (uint64_t*)h->prop_what.d);
    hipLaunchKernelGGL(propose_build_fwd_kernel, pg, dim3(kBlock), 0, h->stream, na, (const PropRec*)props_d, n_props, (const PropEnt*)pe_d,
                       (const unsigned int*)bad, stamp, msgs_dev, ents_dev, (uint32_t)n_ents, members_word(h));
  } else if (members) {
    hipLaunchKernelGGL(propose_check_voters_kernel, cg, dim3(kBlock), 0, h->stream, na, (const PropRec*)v_props, n_props, (const PropEnt*)v_pe, n_prop_ents,
                       pool_bytes, bad, stamp, props_d, pe_d, h->wire_flags + 3, (const uint16_t*)h->voters);
    hipLaunchKernelGGL(propose_build_voters_kernel, pg, dim3(kBlock), 0, h->stream, na, (const PropRec*)props_d, n_props, (const PropEnt*)pe_d,
                       (const unsigned int*)bad, stamp, msgs_dev, ents_dev, (uint32_t)n_ents, (const uint16_t*)h->voters, members_word(h));
  } else {
    hipLaunchKernelGGL(propose_check_kernel, cg, dim3(kBlock), 0, h->stream, na, (const PropRec*)v_props, n_props, (const PropEnt*)v_pe, n_prop_ents, pool_bytes,
                       bad, stamp, props_d, pe_d, h->wire_flags + 3);
    hipLaunchKernelGGL(propose_build_kernel, pg, dim3(kBlock), 0, h->stream, na, (const PropRec*)props_d, n_props, (const PropEnt*)pe_d,
                       (const unsigned int*)bad, stamp, msgs_dev, ents_dev, (uint32_t)n_ents);
  }
  // ... the marshal of everything right behind it ...
  const unsigned long long* members_d = counted ? (const unsigned long long*)members_word(h) : nullptr;
  const auto commit = fwd ? propose_commit_fwd_kernel : propose_commit_kernel;
  if (int rc = stream_launch(h, sc, wire_enc_fused_kernel, kBlock, sc.in, n, n_e, pool_bytes, (uint8_t*)h->wire_out.d, (uint8_t*)v_out, cap, (uint64_t*)v_off,
                             sc.ctl, h->wire_pin_d + kPinCall, (const unsigned int*)bad, stamp)) {
    // no marshal, no verdict: the check's marks still come off (a null `pin` makes every lane of the commit kernel refuse)
    hipLaunchKernelGGL(commit, pg, dim3(kBlock), 0, h->stream, na, (const PropRec*)props_d, n_props, (const unsigned int*)bad, stamp,
                       (const uint64_t*)nullptr, cap, n_dev, members_d);
    (void)hipGetLastError();
    return rc;
  }
  // ... and appendEntry's stores behind both verdicts, the check's and the marshal's, which the encoder's last tile has left in the
  // pinned words: a call that fails has applied nothing.  Still one submission and one wait
  hipLaunchKernelGGL(commit, pg, dim3(kBlock), 0, h->stream, na, (const PropRec*)props_d, n_props, (const unsigned int*)bad, stamp,
                     (const uint64_t*)(h->wire_pin_d + kPinCall), cap, n_dev, members_d);
  HIPCHK(h, hipGetLastError());
  if (counted)
    if (int rc = members_end(h)) return rc;
  HIPCHK(h, raftq_detail::wait_call(h));
  if (int rc = tile_ctl_check(h, "raftq_propose_frames", kPinCall)) return rc;
  // (from here on the host reads the words propose_commit_kernel decided on: it fails exactly where that kernel stored nothing)
  const uint64_t total = h->wire_pin[kPinCall + kPinTotal];
  // the frames that have bytes: every slot, or -- over members, or with followers' records forwarded -- what the build kernel counted
  const uint64_t frames = counted ? h->wire_pin[kPinCall + kPinMembers] : n_dev;
  // over members a non-member's slot is a filler the encoder refuses.  A refused call counted no member frame (its build kernel built
  // nothing), so a count above zero that accounts for every refusal needs no look at the check's word
  const uint64_t refused = h->wire_pin[kPinCall + kPinRefused];
  const bool fillers_only = counted && refused == n_dev - frames;
  if (refused != 0 && !(fillers_only && frames != 0)) {
    // which record, and why (the check kernel left the largest (stamp, reason, record) it met; an older call's stamp: the marshal refused)
    unsigned long long why = 0;
    (void)hipMemcpy(&why, h->wire_flags + 3, 8, hipMemcpyDeviceToHost);
    static const char* const kWhy[] = {"?", "an entry's payload lies outside the pool", "its group is out of range", "it carries no entries (or more than 1024)",
                                       "its entries lie outside prop_ents[]", "this node does not lead its group", "its group is named twice",
                                       "this node is no member of its group",
                                       "its append would move the commit index (a one-voter group, or a membership that shrank since the last "
                                       "acknowledgement): raftq_apply_log_deltas reports that"};
    const uint32_t reason = (uint32_t)(why >> 32) & 0xffu;
    if ((why >> 40) == (stamp & 0xffffffu) && reason >= 1 && reason <= 8)
      return fail(h, RAFTQ_EINVAL, std::string("raftq_propose_frames: record ") + std::to_string((uint32_t)why) + ": " + kWhy[reason] + " -- nothing was appended");
    // (over members: proposals whose groups have no member but this node build no frame at all; forwarding: neither do dropped ones)
    if (!fillers_only)
      return fail(h, RAFTQ_EINVAL, "raftq_propose_frames: a queued message has to / from >= 255, an entry range outside ents[] or a payload outside the pool -- "
                                   "nothing was appended, the output is not valid");
  }
  if (counts) *counts = raftq_wire_counts_t{n_msgs + frames, n_e, 0, total};
  if (total > cap) return fail(h, RAFTQ_EINVAL, "raftq_propose_frames: out is too small (counts->bytes is the size needed) -- nothing was appended");
  if (fwd) h->prop_what_n = n_props;  // the check kernel's stores are behind the same wait
  return RAFTQ_OK;
}

int raftq_propose_outcomes(raftq_t* h, const uint8_t** what, uint64_t* n) {
  if (!h) return fail(nullptr, RAFTQ_EINVAL, "null handle");
  if (!what || !n) return fail(h, RAFTQ_EINVAL, "raftq_propose_outcomes: null argument");
  *what = h->prop_what_n ? h->prop_what.h : nullptr;
  *n = h->prop_what_n;
  return RAFTQ_OK;
}

int raftq_wire_decode(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off, uint64_t n,
                      raftq_wire_msg_t* msgs, raftq_wire_ent_t* ents, uint64_t ents_cap, raftq_wire_counts_t* counts) {
  if (int rc = use_device(h)) return rc;
  if (counts) *counts = raftq_wire_counts_t{0, 0, 0, 0};
  if (n == 0) return RAFTQ_OK;
  if ((!stream && nbytes) || !frame_off || !msgs) return fail(h, RAFTQ_EINVAL, "raftq_wire_decode: null argument");
  if (n > kMaxItems) return fail(h, RAFTQ_EINVAL, "raftq_wire_decode: batch too large");
  if (!ents) ents_cap = 0;
  if (int rc = ensure_pin(h)) return rc;
  // page-locked caller buffers: ONE kernel -- readers bring boundaries and stream into the scratch in order, workers parse
  // tile by tile behind them and push records and entry headers out (raftq_wire_kernels.hpp "the streaming form")
  Views v(streaming_on() && nbytes < (1ull << (kLbValueBits - 1)));
  void *v_stream = v.add(stream, nbytes != 0), *v_off = v.add(frame_off), *v_msgs = v.add(msgs), *v_ents = v.opt(ents);
  if (!v.ok) return wire_decode_copying(h, stream, nbytes, frame_off, n, msgs, ents, ents_cap, counts);
  if (int rc = decode_streaming_enqueue(h, v_stream, nbytes, v_off, n, v_msgs, v_ents, ents_cap, nullptr, FrameFilter{0, 0, 0, 0, 0, nullptr})) return rc;
  HIPCHK(h, raftq_detail::wait_call(h));
  return decode_streaming_finish(h, "raftq_wire_decode", frame_off, n, ents != nullptr, ents_cap, true, counts);
}

int raftq_wire_decode_packed(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off, uint64_t n, int form, uint32_t head_types,
                             uint32_t to_slot, void* narrow, raftq_wire_msg_t* wide, uint64_t wide_cap, raftq_wire_ent_t* ents, uint64_t ents_cap,
                             raftq_wire_counts_t* counts, uint64_t* n_wide) {
  const char* who = "raftq_wire_decode_packed";
  if (int rc = raftq_detail::use_device_idle(h, who)) return rc;  // (kPinThird and the scratch are a Step batch's while one is in flight)
  if (counts) *counts = raftq_wire_counts_t{0, 0, 0, 0};
  if (n_wide) *n_wide = 0;
  if (form != RAFTQ_WIRE_FORM_40 && form != RAFTQ_WIRE_FORM_HEAD) return fail(h, RAFTQ_EINVAL, std::string(who) + ": form is neither RAFTQ_WIRE_FORM_40 nor RAFTQ_WIRE_FORM_HEAD");
  if (to_slot >= 255) return fail(h, RAFTQ_EINVAL, std::string(who) + ": to_slot must be a peer slot (< 255)");
  if (n == 0) return RAFTQ_OK;
  if ((!stream && nbytes) || !frame_off || !narrow || (wide_cap && !wide)) return fail(h, RAFTQ_EINVAL, std::string(who) + ": null argument");
  if (n > kMaxItems) return fail(h, RAFTQ_EINVAL, std::string(who) + ": batch too large");
  if (!ents) ents_cap = 0;
  if (int rc = ensure_pin(h)) return rc;
  Views v(nbytes < (1ull << (kLbValueBits - 1)));
  void *v_stream = v.add(stream, nbytes != 0), *v_off = v.add(frame_off), *v_narrow = v.add(narrow), *v_wide = v.add(wide, wide_cap != 0),
       *v_ents = v.opt(ents);
  if (!v.ok)
    return fail(h, RAFTQ_EINVAL, std::string(who) + ": every array must be page-locked (raftq_host_alloc, hipHostMalloc, hipHostRegister) and "
                                                    "16-byte aligned -- the narrow forms exist in the streaming form only");
  if (int rc = decode_streaming_enqueue(h, v_stream, nbytes, v_off, n, v_narrow, v_ents, ents_cap, nullptr, FrameFilter{0, 0, 0, 0, 0, nullptr}, form,
                                        PackedOut{(WireMsg*)v_wide, wide_cap, head_types, to_slot}))
    return rc;
  HIPCHK(h, raftq_detail::wait_call(h));
  const int rc = decode_streaming_finish(h, who, frame_off, n, ents != nullptr, ents_cap, true, counts);
  if (rc == RAFTQ_EHIP) return rc;  // a look-back gave up: no total is to be trusted
  const uint64_t total_wide = h->wire_pin[kPinCall + kPinThird];
  if (n_wide) *n_wide = total_wide;
  if (rc != RAFTQ_OK) return rc;
  if (total_wide > wide_cap) return fail(h, RAFTQ_EINVAL, std::string(who) + ": more wide frames than wide_cap (*n_wide is the number needed)");
  return RAFTQ_OK;
}

}  // extern "C"

// ---- raftq_step_frames*: the decoder in front of Step (raftq_step.hip) --------------------------------------------------------
int raftq_detail::wire_frames_enqueue(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off, uint64_t n, void* msgs, void* ents,
                                      uint64_t ents_cap, void* msgs_d, int tail_appends, void* zero2, const PackedDst* packed) {
  if (n > kMaxItems) return fail(h, RAFTQ_EINVAL, "raftq_step_frames: batch too large");
  if (int rc = ensure_pin(h)) return rc;
  const bool wide = packed && packed->wide_cap != 0;
  Views v(nbytes < (1ull << (kLbValueBits - 1)));
  void *v_stream = v.add(stream, nbytes != 0), *v_off = v.add(frame_off), *v_msgs = v.add(msgs), *v_ents = v.opt(ents),
       *v_wide = v.add(wide ? packed->wide : nullptr, wide);
  if (!v.ok)
    return fail(h, RAFTQ_EINVAL, "raftq_step_frames: the stream, the boundaries and the result arrays must be page-locked (raftq_host_alloc, "
                                 "hipHostMalloc, hipHostRegister) and 16-byte aligned -- decode and step in two calls otherwise");
  const FrameFilter ff{(h->step_props ? 3u : 1u) | (h->pre_vote ? 4u : 0u) | (h->lead_transfer ? 8u : 0u) | (h->read_index ? 16u : 0u), h->N, h->self_peer, tail_appends ? 1u : 0u, h->G, (unsigned long long*)zero2};
  if (packed)
    return decode_streaming_enqueue(h, v_stream, nbytes, v_off, n, v_msgs, v_ents, ents ? ents_cap : 0, (WireMsg*)msgs_d, ff, packed->form,
                                    PackedOut{(WireMsg*)v_wide, wide ? packed->wide_cap : 0, packed->head_types, h->self_peer});
  return decode_streaming_enqueue(h, v_stream, nbytes, v_off, n, v_msgs, v_ents, ents ? ents_cap : 0, (WireMsg*)msgs_d, ff);
}
uint64_t raftq_detail::wire_frames_n_wide(raftq_t* h) { return h->wire_pin[kPinCall + kPinThird]; }

int raftq_detail::wire_frames_finish(raftq_t* h, const uint64_t* frame_off, uint64_t n, bool have_ents, uint64_t ents_cap, raftq_wire_counts_t* counts) {
  return decode_streaming_finish(h, "raftq_step_frames", frame_off, n, have_ents, ents_cap, false, counts);
}

// ---- raftq_step_frames_respond ----------------------------------------------------------------------------------------
namespace {
struct RespScratch {
  size_t o_blk_cnt, o_blk_off, o_peer_off, bytes;
};
RespScratch resp_scratch(uint64_t n) {
  const uint64_t blocks = (n + kBlock - 1) / kBlock;
  RespScratch r;
  r.o_blk_cnt = align256((size_t)n * sizeof(RespRec));
  r.o_blk_off = r.o_blk_cnt + align256((size_t)blocks * kMaxPeers * 4);
  r.o_peer_off = r.o_blk_off + align256((size_t)blocks * kMaxPeers * 8);
  r.bytes = r.o_peer_off + 256;
  return r;
}
// the marshal of the responses: the records go where the encoder's readers would have put a caller's messages -- the scratch
// behind an empty feed
StreamCall resp_marshal_call(const raftq_detail::RespPlan& p) {
  StreamCall sc;
  sc.n_tiles = blocks_for(p.n_max);
  sc.seg[0] = {nullptr, 0, p.n_max * sizeof(WireMsg)};
  // raftq_respond_set_lead: the entry headers too -- one slot per result, written by resp_scatter_lead_kernel
  // raftq_respond_set_props: ... behind one slot per header the decoder handed back; and the whole request lies behind the
  // decoder's copy of the stream, the encoder's pool (segment 2 has nothing to feed: respond_enqueue points it there)
  if (p.lead || p.props) sc.seg[1] = {nullptr, 0, (p.ent_base + p.n) * sizeof(WireEnt)};
  // (RAFTQ_RESPOND_PROPS_POOL=feed, the measured alternative: the encoder's readers bring the pool in from the caller's stream)
  if (p.props && p.v_stream != nullptr) sc.seg[2] = {p.v_stream, p.nbytes, 0};
  sc.keep = p.keep;
  sc.out_bytes = p.cap + 16;
  return sc;
}
}  // namespace

int raftq_detail::respond_prepare(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off, const void* msgs, const void* ents,
                                  uint64_t ents_cap, const uint64_t* at_tail, void* out, uint64_t cap, uint64_t* resp_off, uint64_t* peer_off,
                                  uint64_t n, RespPlan* p) {
  const char* who = "raftq_step_frames_respond";
  if (n > kMaxItems) return fail(h, RAFTQ_EINVAL, std::string(who) + ": batch too large");
  if (int rc = ensure_pin(h)) return rc;
  // what raftq_step_frames' decoder takes, and what this call adds: all of it checked here, before anything is enqueued
  Views v(nbytes < (1ull << (kLbValueBits - 1)));
  void* v_stream = v.add(stream, nbytes != 0);
  v.add(frame_off), v.add(msgs);
  void* v_ents = v.opt(ents);
  void *v_tail = v.opt(at_tail), *v_out = v.add(out), *v_roff = v.opt(resp_off);
  v.add(peer_off);
  if (!v.ok)
    return fail(h, RAFTQ_EINVAL, std::string(who) + ": every array must be page-locked (raftq_host_alloc, hipHostMalloc, hipHostRegister) and "
                                                    "16-byte aligned -- nothing was applied");
  const size_t resp_bytes = resp_scratch(n).bytes;
  HIPCHK(h, h->resp_dev.grow_zeroed(resp_bytes, grown(resp_bytes), h->stream));  // (zeroed: stamp 0 is no call's)
  p->n = n;
  p->n_max = n * (h->N - 1);
  p->lead = h->resp_lead;
  p->props = h->resp_props;
  const uint64_t frame_max = p->lead ? RAFTQ_RESPOND_LEAD_FRAME_MAX : RAFTQ_RESPOND_FRAME_MAX;
  if (p->props) {
    // (the caller has checked cap against this very bound, and the bound against 2^31)
    p->cap = std::min<uint64_t>(cap, p->n_max * frame_max + (h->N - 1) * (nbytes + ents_cap * RAFTQ_RESPOND_ENT_MAX));
    // (an entry costs its frame two bytes at least: more headers than that the decoder cannot find)
    p->ent_base = std::min<uint64_t>(ents_cap, nbytes / 2 + 1);
    p->nbytes = nbytes;
    p->v_ents = v_ents;
    // The pool: the decoder's copy of the stream, kept alive in front of the marshal's scratch -- no payload byte crosses the link
    // inbound twice.  RAFTQ_RESPOND_PROPS_POOL=feed (read per call, for the A/B of tools/profile_respond_props.py and one test):
    // the marshal overlays the decoder's scratch as it always did and its readers pull the stream from the caller's array again.
    const char* pool_env = std::getenv("RAFTQ_RESPOND_PROPS_POOL");
    if (pool_env != nullptr && std::strcmp(pool_env, "feed") == 0) {
      p->v_stream = v_stream;
    } else {
      p->pool_off = decode_stream_off(n);
      p->keep = decode_stream_end(n, nbytes);
    }
  } else {
    // what the encoder may write: never more than the worst case
    p->cap = std::min<uint64_t>(cap, p->n_max * frame_max);
  }
  // everything the layout and the marshal will need is allocated NOW, before anything is stepped: a call that has stepped cannot
  // fail for memory (the calls behind the step find the control block, the scratch and the output buffer big enough)
  if (p->n_max != 0) {
    StreamCall sc = resp_marshal_call(*p);
    if (int rc = stream_reserve(h, sc)) return rc;
  }
  if (++h->resp_stamp == 0) h->resp_stamp = 1;
  h->resp_at_tail_d = (const uint64_t*)v_tail;
  h->resp_ent_base = (uint32_t)p->ent_base;
  p->v_out = v_out;
  p->v_resp_off = (uint64_t*)v_roff;
  p->peer_off = peer_off;
  return RAFTQ_OK;
}

int raftq_detail::respond_enqueue(raftq_t* h, const RespPlan& p) {
  const RespScratch rs = resp_scratch(p.n);
  uint8_t* rd = (uint8_t*)h->resp_dev.d;
  const uint32_t blocks = blocks_for(p.n);
  RespLayout L{(const RespRec*)rd, p.n, h->N, h->self_peer, h->resp_stamp, (uint32_t*)(rd + rs.o_blk_cnt), (uint64_t*)(rd + rs.o_blk_off),
               (uint64_t*)(rd + rs.o_peer_off)};
  const bool members = raftq_detail::masked_bcast(h);  // the commit broadcasts go to each group's own members (the resp_*_voters_kernel entry points)
  if (members) hipLaunchKernelGGL(resp_count_voters_kernel, dim3(blocks), dim3(kBlock), 0, h->stream, L, (const uint16_t*)h->voters);
  else hipLaunchKernelGGL(resp_count_kernel, dim3(blocks), dim3(kBlock), 0, h->stream, L);
  hipLaunchKernelGGL(resp_scan_kernel, dim3(1), dim3(kBlock), 0, h->stream, L, blocks);
  HIPCHK(h, hipGetLastError());
  if (p.n_max != 0) {
    StreamCall sc = resp_marshal_call(p);
    if (int rc = stream_prepare(h, sc)) return rc;  // (allocates nothing: respond_prepare reserved this very request)
    WireMsg* const enc = (WireMsg*)sc.in.seg[0].dst;
    WireEnt* const ents = (WireEnt*)sc.in.seg[1].dst;
    const uint16_t* const voters = (const uint16_t*)h->voters;
    // the two switches, one entry point each way
    // raftq_respond_set_props: the decoder's records of this batch (its slot's, in HBM), its headers in the caller's array, and its
    // copy of the stream -- still in the scratch in front of this request -- as the encoder's pool
    RespProps rp{nullptr, nullptr, (uint32_t)p.ent_base};
    uint64_t pool_bytes = 0;
    if (p.props) {
      rp.dec = (const WireMsg*)h->step_slot[(h->step_submitted - 1) % raftq::kStepSlots].w_msgs_d;
      rp.heads = (const WireEnt*)p.v_ents;
      if (p.v_stream == nullptr) sc.in.seg[2].dst = (uint8_t*)h->wire_dev.d + p.pool_off;
      pool_bytes = p.nbytes;
    }
    const bool with_ents = p.lead || p.props;
    if (with_ents && members) hipLaunchKernelGGL(resp_scatter_lead_voters_kernel, dim3(blocks), dim3(kBlock), 0, h->stream, L, enc, p.n_max, voters, ents, rp);
    else if (with_ents) hipLaunchKernelGGL(resp_scatter_lead_kernel, dim3(blocks), dim3(kBlock), 0, h->stream, L, enc, p.n_max, (const uint16_t*)nullptr, ents, rp);
    else if (members) hipLaunchKernelGGL(resp_scatter_voters_kernel, dim3(blocks), dim3(kBlock), 0, h->stream, L, enc, p.n_max, voters);
    else hipLaunchKernelGGL(resp_scatter_kernel, dim3(blocks), dim3(kBlock), 0, h->stream, L, enc, p.n_max);
    // (the entry array: ent_base + p.n slots with either switch on, none otherwise)
    if (int rc = stream_launch(h, sc, wire_enc_fused_kernel, kBlock, sc.in, p.n_max, with_ents ? p.ent_base + p.n : (uint64_t)0, pool_bytes, (uint8_t*)h->wire_out.d, (uint8_t*)p.v_out,
                               p.cap, p.v_resp_off, sc.ctl, h->wire_pin_d + kPinRespond, (const unsigned int*)nullptr, 0u))
      return rc;
  }
  // the slices' bounds: a copy of the runtime's (no new kernel writes host memory)
  HIPCHK(h, hipMemcpyAsync(p.peer_off, rd + rs.o_peer_off, (size_t)(h->N + 1) * 8, hipMemcpyDeviceToHost, h->stream));
  return RAFTQ_OK;
}

int raftq_detail::respond_pass_ok(raftq_t* h) { return tile_ctl_check(h, "raftq_step_frames_respond", kPinRespond); }

int raftq_detail::respond_finish(raftq_t* h, const RespPlan& p, raftq_wire_counts_t* resp_counts) {
  const uint64_t frames = p.peer_off[h->N];
  uint64_t bytes = 0;
  if (p.n_max != 0) {
    if (int rc = tile_ctl_check(h, "raftq_step_frames_respond", kPinRespond)) return rc;
    bytes = h->wire_pin[kPinRespond + kPinTotal];
    // every record past the last frame is a filler the encoder refuses; any other refusal, or bytes beyond the bound, is a bug here
    if (h->wire_pin[kPinRespond + kPinRefused] != p.n_max - frames || bytes > p.cap)
      return fail(h, RAFTQ_EHIP, "raftq_step_frames_respond: the marshal of the responses disagrees with their layout; the output is not valid");
  }
  if (resp_counts) *resp_counts = raftq_wire_counts_t{frames, 0, 0, bytes};
  return RAFTQ_OK;
}

// ---- raftq_tick_frames, raftq_tick_elect_frames ------------------------------------------------------------------------
namespace {
// the marshal of the heartbeats: as resp_marshal_call, the records go into the scratch behind an empty feed
StreamCall beat_marshal_call(uint64_t n_max, uint64_t cap) {
  StreamCall sc;
  sc.n_tiles = blocks_for(n_max);
  sc.seg[0] = {nullptr, 0, n_max * sizeof(WireMsg)};
  sc.out_bytes = cap + 16;
  return sc;
}
// The device-built round of raftq_tick_frames and raftq_tick_elect_frames: Tick -> lists -> beat_build -> elect_build -> encoder ->
// flag, back to back; one wait.  elect: the election round behind the heartbeat round.  The encoder's input then holds
// (beat_cap + hup_cap) * (N - 1) records: beat_build_kernel runs over the first beat_cap * (N - 1) (its fillers start where the
// heartbeats end), elect_build_kernel, behind it in stream order, puts the votes directly behind the heartbeats and the fillers
// behind both; peer_off gets a second section of N + 1 words and camp the campaigns' results.  Without it -- and with hup_cap == 0,
// which is the same call -- hup_cap bounds the MsgHup list alone, camp is not looked at and peer_off is N + 1 words.
int tick_round(raftq_t* h, bool elect, unsigned flags, uint64_t hup_cap, uint64_t beat_cap, uint64_t* n_hup, uint64_t* n_beat, raftq_step_out_s_t* camp,
               void* out, uint64_t cap, uint64_t* frame_off, uint64_t* peer_off, raftq_wire_counts_t* counts) {
  const char* who = elect ? "raftq_tick_elect_frames" : "raftq_tick_frames";
  const char *const caps = elect ? "beat_cap + hup_cap" : "beat_cap", *const product = elect ? "(beat_cap + hup_cap)" : "beat_cap";  // (in the refusals' texts)
  if (int rc = raftq_detail::use_device_idle(h, who)) return rc;
  if (counts) *counts = raftq_wire_counts_t{0, 0, 0, 0};
  // (raftq_tick_set_checks opens the call: the beat bitmap beat_build_kernel ranks never held a group whose check failed, and under
  // both switches the election round is elect_build_cq_kernel's, Step's own MsgHup arm)
  if (elect)
    if (int rc = raftq_detail::refuse_pre_vote(h, who, true)) return rc;
  if (int rc = raftq_detail::refuse_check_quorum(h, who, true)) return rc;
  if (int rc = raftq_detail::refuse_read_index(h, who)) return rc;
  if (!n_hup || !n_beat || !peer_off) return fail(h, RAFTQ_EINVAL, std::string(who) + ": null argument");
  if (flags & ~RAFTQ_TICK_BEAT_BITMAP) return fail(h, RAFTQ_EINVAL, std::string(who) + ": unknown flag");
  if (h->N < 2)
    return fail(h, RAFTQ_EINVAL, std::string(who) + ": a single-peer group has nobody to " + (elect ? "ask for a vote" : "send a heartbeat to") +
                                     " -- use raftq_tick_collect_lists");
  // the exact worst case: beat_cap + vote_cap groups, N - 1 frames of RAFTQ_RESPOND_FRAME_MAX bytes each -- refused before anything
  // runs, so a call that has ticked never fails for output space
  const uint64_t vote_cap = elect ? hup_cap : 0;  // the groups the election round is built for
  const uint64_t slices = h->N - 1;
  const uint64_t frames_cap = ((uint64_t)1 << 31) / RAFTQ_RESPOND_FRAME_MAX;
  if (beat_cap >= ((uint64_t)1 << 31) || vote_cap >= ((uint64_t)1 << 31) || (beat_cap + vote_cap) * slices > kMaxItems || (beat_cap + vote_cap) * slices > frames_cap)
    return fail(h, RAFTQ_EINVAL, std::string(who) + ": " + caps + " too large (" + product + " * (N - 1) * RAFTQ_RESPOND_FRAME_MAX must stay within 2^31 bytes)");
  const uint64_t n_max = (beat_cap + vote_cap) * slices;
  if (cap < n_max * RAFTQ_RESPOND_FRAME_MAX)
    return fail(h, RAFTQ_EINVAL, std::string(who) + ": cap is below " + product + " * (N - 1) * RAFTQ_RESPOND_FRAME_MAX = " +
                                     std::to_string(n_max * RAFTQ_RESPOND_FRAME_MAX) + " bytes -- the call has not ticked");
  if ((n_max != 0 && !out) || (vote_cap != 0 && !camp)) return fail(h, RAFTQ_EINVAL, std::string(who) + ": null argument");
  if (!h->node_rec && !h->self_set)
    return fail(h, RAFTQ_ESTATE, std::string(who) + ": the handle holds no node state (raftq_set_self / raftq_load_node first)");
  if (int rc = ensure_pin(h)) return rc;
  Views v;
  void *v_out = v.opt(out), *v_off = v.opt(frame_off), *v_camp = v.add(camp, vote_cap != 0);
  v.add(peer_off);
  if (!v.ok)
    return fail(h, RAFTQ_EINVAL,
                std::string(who) + (elect ? ": camp, out, frame_off and peer_off must be page-locked (raftq_host_alloc, hipHostMalloc, "
                                            "hipHostRegister) and 16-byte aligned -- the call has neither ticked nor campaigned"
                                          : ": out, frame_off and peer_off must be page-locked (raftq_host_alloc, hipHostMalloc, hipHostRegister) "
                                            "and 16-byte aligned -- the call has not ticked"));
  // every allocation before the tick kernel: the records (and, where something other than Step wrote the dense arrays, their
  // refresh), the Tick's lists, the encoder's control block, scratch and output buffer
  NodeArrays na;
  if (int rc = raftq_detail::node_records_of(h, who, &na, true)) return rc;
  const bool members = raftq_detail::masked_tick(h);  // the rounds go to each group's own members (the *_voters_kernel entry points)
  raftq_detail::TickLists tl;
  if (int rc = raftq_detail::tick_lists_prepare(h, who, flags, hup_cap, beat_cap, &tl)) return rc;
  const uint64_t enc_cap = n_max * RAFTQ_RESPOND_FRAME_MAX;  // what the encoder may write: never more than the worst case
  StreamCall sc = beat_marshal_call(n_max, enc_cap);
  if (n_max != 0)
    if (int rc = stream_prepare(h, sc)) return rc;  // (the launch's epoch and feed: nothing of it runs before the encoder below)
  if (vote_cap != 0) h->last_flags &= ~RAFTQ_SWEEP_NO_ADOPT;  // as in raftq_step_submit: the live state moves
  if (int rc = raftq_detail::tick_lists_enqueue(h, &tl)) return rc;
  if (n_max != 0) {
    const uint64_t nw = h->gpad / 256;
    const dim3 grid((unsigned)((nw + kWaves - 1) / kWaves));
    WireMsg* const enc = (WireMsg*)sc.in.seg[0].dst;
    if (members)
      if (int rc = members_begin(h)) return rc;
    if (beat_cap != 0) {  // the heartbeat round, over each group's own members where the Tick is
      BeatArgs ba{(const uint64_t*)h->beat_bits, (const uint4*)h->tick_partials, nw, tl.off_beat, (const uint64_t*)h->d_total, na.rec, h->G, h->N,
                  h->self_peer, beat_cap, enc};
      if (members) hipLaunchKernelGGL(beat_build_voters_kernel, grid, dim3(kBlock), 0, h->stream, ba, (const uint16_t*)h->voters, members_word(h));
      else hipLaunchKernelGGL(beat_build_kernel, grid, dim3(kBlock), 0, h->stream, ba);
    }
    if (vote_cap != 0) {  // (without it the fillers behind beat_cap * (N - 1) are beat_build_kernel's own)
      ElectArgs ea{(const uint64_t*)h->hup_bits, (const uint4*)h->tick_partials, nw, tl.off_h, (const uint64_t*)h->d_total, na, vote_cap, beat_cap,
                   (StepOutS*)v_camp, enc};
      if (raftq_detail::tick_checks(h)) {  // Node's CQ form: na carries cq, election_tick and pv (node_records_of)
        if (members) hipLaunchKernelGGL(elect_build_cq_voters_kernel, grid, dim3(kBlock), 0, h->stream, ea, (const uint16_t*)h->voters, members_word(h));
        else hipLaunchKernelGGL(elect_build_cq_kernel, grid, dim3(kBlock), 0, h->stream, ea);
      } else if (members) hipLaunchKernelGGL(elect_build_voters_kernel, grid, dim3(kBlock), 0, h->stream, ea, (const uint16_t*)h->voters, members_word(h));
      else hipLaunchKernelGGL(elect_build_kernel, grid, dim3(kBlock), 0, h->stream, ea);
    }
    HIPCHK(h, hipGetLastError());
    if (int rc = stream_launch(h, sc, wire_enc_fused_kernel, kBlock, sc.in, n_max, (uint64_t)0, (uint64_t)0, (uint8_t*)h->wire_out.d, (uint8_t*)v_out, enc_cap,
                               (uint64_t*)v_off, sc.ctl, h->wire_pin_d + kPinCall, (const unsigned int*)nullptr, 0u))
      return rc;
    if (members)
      if (int rc = members_end(h)) return rc;
  }
  if (int rc = raftq_detail::tick_lists_finish(h, who, tl, n_hup, n_beat)) return rc;
  const uint64_t n_bb = std::min(*n_beat, beat_cap), n_vb = std::min(*n_hup, vote_cap);
  // the frames that have bytes: every slot of both sections, or -- over members -- what the build kernels counted
  const uint64_t frames = !members ? (n_bb + n_vb) * slices : n_max != 0 ? h->wire_pin[kPinCall + kPinMembers] : 0;
  uint64_t at = 0;
  for (int sec = 0; sec < (elect ? 2 : 1); ++sec)  // the heartbeat section's slices, then the vote section's
    for (uint32_t p = 0; p <= h->N; ++p) {
      peer_off[sec * (h->N + 1) + p] = at;
      if (p < h->N && p != h->self_peer) at += sec ? n_vb : n_bb;
    }
  uint64_t bytes = 0;
  if (n_max != 0) {
    if (int rc = tile_ctl_check(h, who, kPinCall)) return rc;
    bytes = h->wire_pin[kPinCall + kPinTotal];
    // every record past the last frame is a filler the encoder refuses, and so is -- over members -- every slot of a peer that is
    // no member of its group or is not asked; any other refusal, or bytes beyond the bound, is a bug here
    if (h->wire_pin[kPinCall + kPinRefused] != n_max - frames || bytes > enc_cap)
      return fail(h, RAFTQ_EHIP, std::string(who) + ": the marshal of the heartbeats" + (elect ? " and votes" : "") +
                                     " disagrees with their layout; the output is not valid");
  } else if (frame_off) {
    frame_off[0] = 0;
  }
  if (counts) *counts = raftq_wire_counts_t{frames, 0, 0, bytes};
  return RAFTQ_OK;
}
}  // namespace

extern "C" int raftq_tick_frames(raftq_t* h, unsigned flags, uint64_t hup_cap, uint64_t beat_cap, uint64_t* n_hup, uint64_t* n_beat, void* out,
                                 uint64_t cap, uint64_t* frame_off, uint64_t* peer_off, raftq_wire_counts_t* counts) {
  return tick_round(h, false, flags, hup_cap, beat_cap, n_hup, n_beat, nullptr, out, cap, frame_off, peer_off, counts);
}
extern "C" int raftq_tick_elect_frames(raftq_t* h, unsigned flags, uint64_t hup_cap, uint64_t beat_cap, uint64_t* n_hup, uint64_t* n_beat,
                                       raftq_step_out_s_t* camp, void* out, uint64_t cap, uint64_t* frame_off, uint64_t* peer_off,
                                       raftq_wire_counts_t* counts) {
  return tick_round(h, true, flags, hup_cap, beat_cap, n_hup, n_beat, camp, out, cap, frame_off, peer_off, counts);
}

// ---- walpb.Record WAL frames --------------------------------------------------------------------------------------------------
namespace {

// The streaming WAL encode, enqueued and NOT waited for; its totals go to the pinned words behind pin_base (raftq_wal_encode:
// kPinCall; raftq_wal_encode_begin: kPinWalPending).
int wal_streaming_enqueue(raftq_t* h, const void* v_recs, uint64_t n, const void* v_pool, uint64_t pool_bytes, uint32_t prev_crc, void* v_out,
                          uint64_t cap, void* v_off, uint32_t pin_base) {
  StreamCall sc;
  sc.n_tiles = blocks_for(n);
  sc.seg[0] = {v_recs, n * sizeof(WalRec), 0};
  sc.seg[1] = {v_pool, pool_bytes, 0};
  sc.out_bytes = cap + 16;
  if (int rc = stream_prepare(h, sc)) return rc;
  return stream_launch(h, sc, wal_enc_fused_kernel, kBlock, sc.in, n, pool_bytes, prev_crc, (uint8_t*)h->wire_out.d, (uint8_t*)v_out, cap, (uint64_t*)v_off,
                       sc.ctl, h->wire_pin_d + pin_base);
}
int wal_streaming_finish(raftq_t* h, const char* who, uint64_t n, uint64_t cap, uint32_t prev_crc, uint32_t pin_base, raftq_wal_counts_t* counts) {
  if (counts) *counts = raftq_wal_counts_t{0, 0, 0, prev_crc, 0};
  if (int rc = tile_ctl_check(h, who, pin_base)) return rc;
  const uint64_t* pin = h->wire_pin + pin_base;
  if (int rc = encode_sized(h, who, kWalEncRefused, "the output is not valid", pin[kPinTotal], pin[kPinRefused], cap, counts,
                            raftq_wal_counts_t{n, 0, pin[kPinTotal], prev_crc, 0}))
    return rc;
  if (counts) {
    counts->n_valid = n;
    counts->last_crc = (uint32_t)pin[kPinThird];
  }
  return RAFTQ_OK;
}
// a raftq_wal_encode_begin whose _end has not come yet: wait for it and keep what _end will report (called by whatever else
// is about to use its pinned words' neighbours' scratch from the host side)
int wal_pending_complete(raftq_t* h) {
  if (!h->wal_pending || h->wal_pending_done) return RAFTQ_OK;
  // (the wait of the marshal called in between has usually covered it: then there is nothing to wait for, and nothing to launch)
  if (!h->wal_pending_waited) HIPCHK(h, raftq_detail::wait_call(h));
  h->wal_pending_rc =
      wal_streaming_finish(h, "raftq_wal_encode_begin", h->wal_pending_n, h->wal_pending_cap, h->wal_pending_prev, kPinWalPending, &h->wal_pending_counts);
  if (h->wal_pending_rc != RAFTQ_OK) h->wal_pending_err = h->err;
  h->wal_pending_done = true;
  return RAFTQ_OK;
}

int wal_encode_copying(raftq_t* h, const raftq_wal_rec_t* recs, uint64_t n, const void* pool, uint64_t pool_bytes, uint32_t prev_crc, void* out,
                       uint64_t cap, uint64_t* frame_off, raftq_wal_counts_t* counts) {
  const size_t scan_bytes = scan_sum_scratch_bytes(n + 1);  // tile totals of the hand-written scan
  Carver c;
  const size_t o_recs = c.take(n * sizeof(WalRec)), o_pool = c.take(pool_bytes), o_pcrc = c.take(n * 4),
               o_pair = c.take(n * 8), o_chain = c.take(n * 8), o_sizes = c.take((n + 1) * 8),
               o_off = c.take((n + 1) * 8), o_flags = c.take(8), o_scan = c.take(scan_bytes),
               o_tot = c.take((size_t)blocks_for(n) * sizeof(CrcPair));
  if (int rc = grow(h, h->wire_dev, c.off)) return rc;
  uint8_t* base = (uint8_t*)h->wire_dev.d;
  WalRec* d_recs = (WalRec*)(base + o_recs);
  uint8_t* d_pool = base + o_pool;
  uint32_t* d_pcrc = (uint32_t*)(base + o_pcrc);
  CrcPair *d_pair = (CrcPair*)(base + o_pair), *d_chain = (CrcPair*)(base + o_chain);
  uint64_t *d_sizes = (uint64_t*)(base + o_sizes), *d_off = (uint64_t*)(base + o_off);
  uint32_t* d_last = (uint32_t*)(base + o_flags) + 1;
  unsigned int* d_bad = (unsigned int*)(base + o_flags);
  uint64_t* pin = h->wire_pin + kPinCall;
  if (int rc = h2d(h, d_recs, recs, n * sizeof(WalRec))) return rc;
  if (int rc = h2d(h, d_pool, pool, pool_bytes)) return rc;
  HIPCHK(h, hipMemsetAsync(d_bad, 0, 8, h->stream));
  hipLaunchKernelGGL(wal_enc_payload_crc_kernel, dim3(blocks_for(n * 64)), dim3(kBlock), 0, h->stream,
                     (const WalRec*)d_recs, n, (const uint8_t*)d_pool, pool_bytes, d_pcrc);
  hipLaunchKernelGGL(wal_enc_crc_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, h->stream, (const WalRec*)d_recs, n,
                     (const uint8_t*)d_pool, pool_bytes, (const uint32_t*)d_pcrc, prev_crc, d_pair, d_bad);
  HIPCHK(h, hipGetLastError());
  if (int rc = crc_chain_scan(h, d_pair, d_chain, n, (CrcPair*)(base + o_tot))) return rc;
  hipLaunchKernelGGL(wal_enc_size_kernel, dim3(blocks_for(n + 1)), dim3(kBlock), 0, h->stream, (const WalRec*)d_recs, n,
                     (const CrcPair*)d_chain, d_sizes);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, exclusive_sum_u64((const uint64_t*)d_sizes, d_off, n + 1, (uint64_t*)(base + o_scan), h->stream));
  if (int rc = d2h(h, &pin[kPinTotal], d_off + n, 8)) return rc;
  if (int rc = d2h(h, &pin[kPinRefused], d_bad, 4)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const uint64_t total = pin[kPinTotal];
  if (int rc = encode_sized(h, "raftq_wal_encode", kWalEncRefused, "nothing was written", total, (uint32_t)pin[kPinRefused], cap, counts,
                            raftq_wal_counts_t{n, 0, total, prev_crc, 0}))
    return rc;
  if (int rc = grow(h, h->wire_out, total + 16)) return rc;
  uint8_t* d_out = (uint8_t*)h->wire_out.d;
  hipLaunchKernelGGL(wal_enc_write_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, h->stream, (const WalRec*)d_recs, n,
                     (const CrcPair*)d_chain, (const uint64_t*)d_off, d_out, d_last);
  if (pool_bytes)
    hipLaunchKernelGGL(wal_enc_payload_kernel, dim3(blocks_for(n * 64)), dim3(kBlock), 0, h->stream,
                       (const WalRec*)d_recs, n, (const CrcPair*)d_chain, (const uint64_t*)d_off,
                       (const uint8_t*)d_pool, d_out);
  HIPCHK(h, hipGetLastError());
  if (int rc = d2h(h, out, d_out, total)) return rc;
  if (frame_off)
    if (int rc = d2h(h, frame_off, d_off, (n + 1) * 8)) return rc;
  if (int rc = d2h(h, &pin[kPinThird], d_last, 4)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (counts) {
    counts->n_valid = n;
    counts->last_crc = (uint32_t)pin[kPinThird];
  }
  return RAFTQ_OK;
}

// what either form of raftq_wal_decode reports: records before the first bad one (kPinTotal), the running CRC there (kPinRefused's word)
void wal_decode_counted(raftq_t* h, const uint64_t* frame_off, uint64_t n, raftq_wal_counts_t* counts) {
  const uint64_t* pin = h->wire_pin + kPinCall;
  if (counts) *counts = raftq_wal_counts_t{n, pin[kPinTotal], span_of(frame_off, n), (uint32_t)pin[kPinRefused], 0};
}

// page-locked caller buffers (v_*: as the device addresses them): readers | workers in one launch
int wal_decode_streaming(raftq_t* h, const void* v_bytes, uint64_t nbytes, const uint64_t* frame_off, const void* v_off, uint64_t n, uint32_t prev_crc,
                         void* v_recs, raftq_wal_counts_t* counts) {
  StreamCall sc;
  sc.n_tiles = blocks_for(n);
  sc.seg[0] = {v_off, (n + 1) * 8, 0};
  sc.seg[1] = {v_bytes, nbytes, 0};
  if (int rc = stream_prepare(h, sc)) return rc;
  if (int rc = stream_launch(h, sc, wal_dec_fused_kernel, kBlock, sc.in, nbytes, n, prev_crc, (WalRec*)v_recs, sc.ctl, h->wire_pin_d + kPinCall)) return rc;
  HIPCHK(h, raftq_detail::wait_call(h));
  if (int rc = tile_ctl_check(h, "raftq_wal_decode", kPinCall)) return rc;
  wal_decode_counted(h, frame_off, n, counts);
  return RAFTQ_OK;
}

int wal_decode_copying(raftq_t* h, const void* bytes, uint64_t nbytes, const uint64_t* frame_off, uint64_t n, uint32_t prev_crc, raftq_wal_rec_t* recs,
                       raftq_wal_counts_t* counts) {
  Carver c;
  const size_t o_bytes = c.take(nbytes), o_off = c.take((n + 1) * 8), o_recs = c.take(n * sizeof(WalRec)),
               o_span = c.take(n * sizeof(WalSpan)), o_pair = c.take(n * 8), o_chain = c.take(n * 8),
               o_tail = c.take(32), o_tot = c.take((size_t)blocks_for(n) * sizeof(CrcPair));
  if (int rc = grow(h, h->wire_dev, c.off)) return rc;
  uint8_t* base = (uint8_t*)h->wire_dev.d;
  uint8_t* d_bytes = base + o_bytes;
  uint64_t* d_off = (uint64_t*)(base + o_off);
  WalRec* d_recs = (WalRec*)(base + o_recs);
  WalSpan* d_span = (WalSpan*)(base + o_span);
  CrcPair *d_pair = (CrcPair*)(base + o_pair), *d_chain = (CrcPair*)(base + o_chain);
  unsigned long long* d_first_bad = (unsigned long long*)(base + o_tail);
  uint64_t* d_tail = (uint64_t*)(base + o_tail) + 1;
  if (int rc = h2d(h, d_bytes, bytes, nbytes)) return rc;
  if (int rc = h2d(h, d_off, frame_off, (n + 1) * 8)) return rc;
  HIPCHK(h, hipMemsetAsync(d_first_bad, 0xff, 8, h->stream));
  hipLaunchKernelGGL(wal_dec_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, h->stream, (const uint8_t*)d_bytes, nbytes,
                     (const uint64_t*)d_off, n, prev_crc, d_recs, d_span, d_pair);
  hipLaunchKernelGGL(wal_dec_long_crc_kernel, dim3(blocks_for(n * 64)), dim3(kBlock), 0, h->stream,
                     (const uint8_t*)d_bytes, n, (const WalSpan*)d_span, prev_crc, d_pair);
  HIPCHK(h, hipGetLastError());
  if (int rc = crc_chain_scan(h, d_pair, d_chain, n, (CrcPair*)(base + o_tot))) return rc;
  hipLaunchKernelGGL(wal_dec_check_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, h->stream, d_recs, n,
                     (const CrcPair*)d_chain, prev_crc, d_first_bad);
  hipLaunchKernelGGL(wal_dec_tail_kernel, dim3(1), dim3(64), 0, h->stream, (const CrcPair*)d_chain, n, prev_crc,
                     (const unsigned long long*)d_first_bad, d_tail);
  HIPCHK(h, hipGetLastError());
  if (int rc = d2h(h, recs, d_recs, n * sizeof(WalRec))) return rc;
  if (int rc = d2h(h, h->wire_pin + kPinCall, d_tail, 16)) return rc;  // kPinTotal and the word behind it
  HIPCHK(h, hipStreamSynchronize(h->stream));
  wal_decode_counted(h, frame_off, n, counts);
  return RAFTQ_OK;
}

}  // namespace

extern "C" {

int raftq_wal_encode(raftq_t* h, const raftq_wal_rec_t* recs, uint64_t n, const void* pool, uint64_t pool_bytes,
                     uint32_t prev_crc, void* out, uint64_t cap, uint64_t* frame_off, raftq_wal_counts_t* counts) {
  if (int rc = use_device(h)) return rc;
  if (counts) *counts = raftq_wal_counts_t{0, 0, 0, prev_crc, 0};
  if (n == 0) {
    if (frame_off) frame_off[0] = 0;
    return RAFTQ_OK;
  }
  if (!recs || (pool_bytes && !pool) || (cap && !out)) return fail(h, RAFTQ_EINVAL, "raftq_wal_encode: null argument");
  if (n > kMaxItems) return fail(h, RAFTQ_EINVAL, "raftq_wal_encode: batch too large");
  if (int rc = ensure_pin(h)) return rc;
  // page-locked caller buffers take the streaming form; anything else the copying form
  Views v(streaming_on() && cap != 0 && cap <= ((uint64_t)1 << 31));
  void *v_recs = v.add(recs), *v_pool = v.add(pool, pool_bytes != 0), *v_out = v.add(out), *v_off = v.opt(frame_off);
  if (!v.ok) return wal_encode_copying(h, recs, n, pool, pool_bytes, prev_crc, out, cap, frame_off, counts);
  if (int rc = wal_pending_complete(h)) return rc;  // (a raftq_wal_encode_begin nobody ended: its results are kept for its _end)
  if (int rc = wal_streaming_enqueue(h, v_recs, n, v_pool, pool_bytes, prev_crc, v_out, cap, v_off, kPinCall)) return rc;
  HIPCHK(h, raftq_detail::wait_call(h));
  return wal_streaming_finish(h, "raftq_wal_encode", n, cap, prev_crc, kPinCall, counts);
}

int raftq_wal_encode_begin(raftq_t* h, const raftq_wal_rec_t* recs, uint64_t n, const void* pool, uint64_t pool_bytes, uint32_t prev_crc,
                           void* out, uint64_t cap, uint64_t* frame_off) {
  if (int rc = use_device(h)) return rc;
  if (h->wal_pending) return fail(h, RAFTQ_ESTATE, "raftq_wal_encode_begin: the previous one has not been ended (raftq_wal_encode_end)");
  if (n == 0 || !recs || (pool_bytes && !pool) || !out || cap == 0) return fail(h, RAFTQ_EINVAL, "raftq_wal_encode_begin: null argument or empty batch");
  if (n > kMaxItems) return fail(h, RAFTQ_EINVAL, "raftq_wal_encode_begin: batch too large");
  if (int rc = ensure_pin(h)) return rc;
  Views v(cap <= ((uint64_t)1 << 31));
  void *v_recs = v.add(recs), *v_pool = v.add(pool, pool_bytes != 0), *v_out = v.add(out), *v_off = v.opt(frame_off);
  if (!v.ok)
    return fail(h, RAFTQ_EINVAL, "raftq_wal_encode_begin: the records, the pool and the output must be page-locked (raftq_host_alloc, hipHostMalloc, "
                                 "hipHostRegister) and 16-byte aligned -- raftq_wal_encode otherwise");
  if (int rc = wal_streaming_enqueue(h, v_recs, n, v_pool, pool_bytes, prev_crc, v_out, cap, v_off, kPinWalPending)) return rc;
  h->wal_pending = true;
  h->wal_pending_done = false;
  h->wal_pending_waited = false;
  h->wal_pending_n = n;
  h->wal_pending_cap = cap;
  h->wal_pending_prev = prev_crc;
  return RAFTQ_OK;
}

int raftq_wal_encode_end(raftq_t* h, raftq_wal_counts_t* counts) {
  if (int rc = use_device(h)) return rc;
  if (!h->wal_pending) return fail(h, RAFTQ_ESTATE, "raftq_wal_encode_end: nothing was begun");
  if (int rc = wal_pending_complete(h)) return rc;  // (no wait left to make when a later call on the handle has waited already)
  h->wal_pending = false;
  if (counts) *counts = h->wal_pending_counts;
  if (h->wal_pending_rc != RAFTQ_OK) return fail(h, h->wal_pending_rc, h->wal_pending_err);
  return RAFTQ_OK;
}

int raftq_wal_decode(raftq_t* h, const void* bytes, uint64_t nbytes, const uint64_t* frame_off, uint64_t n,
                     uint32_t prev_crc, raftq_wal_rec_t* recs, raftq_wal_counts_t* counts) {
  if (int rc = use_device(h)) return rc;
  if (counts) *counts = raftq_wal_counts_t{0, 0, 0, prev_crc, 0};
  if (n == 0) return RAFTQ_OK;
  if ((!bytes && nbytes) || !frame_off || !recs) return fail(h, RAFTQ_EINVAL, "raftq_wal_decode: null argument");
  if (n > kMaxItems) return fail(h, RAFTQ_EINVAL, "raftq_wal_decode: batch too large");
  if (int rc = ensure_pin(h)) return rc;
  Views v(streaming_on() && nbytes < (1ull << (kLbValueBits - 1)));
  void *v_bytes = v.add(bytes, nbytes != 0), *v_off = v.add(frame_off), *v_recs = v.add(recs);
  if (v.ok) return wal_decode_streaming(h, v_bytes, nbytes, frame_off, v_off, n, prev_crc, v_recs, counts);
  return wal_decode_copying(h, bytes, nbytes, frame_off, n, prev_crc, recs, counts);
}

}  // extern "C"
