// raftq_beat_kernels.hpp -- raftq_tick_frames' heartbeat round (include/raftq_wire.h): bcastHeartbeat for the groups the Tick in
// front of it flagged MsgBeat, written into the encoder's input in HBM, peer-major -- for every peer slot p != self, ascending,
// one MsgHeartbeat per MsgBeat group in ascending group order -- where the encoder (wire_enc_fused_kernel) marshals them.
//
// A heartbeat is a function of one 128-byte line: MsgHeartbeat{to = p, from = self, group, term, commit = min(match[p],
// committed)} (etcd's sendHeartbeat), all of it in the group's NodeRec (raftq_step_kernels.hpp).  Order comes from the Tick's own
// per-wave counts and popcounts, as in tick_lists32_kernel -- no atomics, the same layout on every run.
//
// One lane per MsgBeat group, not eight lanes per record.  A workgroup first compacts its block's MsgBeat ids in LDS, so the
// lanes that build records are dense whatever share of the block leads.  A lane then pulls the words it needs of its line with
// 16-byte loads (term; role / committed; the match words: 3 to 7 requests, the line itself is fetched once) and keeps every field
// in its own registers -- the min per peer and the N - 1 records need no cross-lane traffic -- and writes each 64-byte record as
// four 16-byte stores, neighbouring lanes to neighbouring records of a peer's slice.  Eight lanes per record would make each
// load instruction cover whole lines, but would then have to shuffle term and committed to the lanes that hold the match words
// and gather 64-byte records from them again; the kernel moves 128 B in and (N - 1) * 64 B out per led group -- 4 MB + 4 MB for
// 32,768 groups x 3 peers, a few microseconds of HBM time -- so it is bounded by its launch and its offset sums, not by how
// the requests are shaped.
//
// MASKED -- rounds over each group's own members (raftq_tick_set_voters on a handle with voter masks loaded): the heartbeat and
// the election round (raftq_elect_kernels.hpp) send to the slots of voters[g] only: upstream's bcastHeartbeat and campaign range
// over r.prs, which IS the membership.  The encoder's input stays POSITIONAL -- n_built slots per peer slice, exactly where the
// unmasked form puts them -- and a slot whose peer is not a member of its group holds a filler record (to = 0xff), which the
// encoder counts as refused and gives zero bytes wherever it stands.  So fillers then lie inside the sections, and "records
// refused" no longer says how many frames were built: each workgroup sums the member frames it wrote (lanes -> wave by shuffles,
// waves in LDS) and adds the sum once, with a 64-bit device-scope atomic, to a device word zeroed in the same submission.  A sum
// does not depend on the order of arrival: the layout stays the same on every run.
// One body per round, one instantiation per entry point (raftq_respond_kernels.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raftq_respond_kernels.hpp"
#include "raftq_step_kernels.hpp"
#include "raftq_wire_kernels.hpp"

namespace raftqk {

struct BeatArgs {
  const uint64_t* beat_bits;      // [gpad / 64] the Tick's MsgBeat bits: word 4 w + k, bit l = group 256 w + 4 l + k
  const uint4* partials;          // [gpad / 256] the Tick's per-wave {MsgHup, MsgBeat} counts
  uint64_t n_chunks;              // gpad / 256
  const uint64_t* wave_off_beat;  // scan_partials_kernel's exclusive MsgBeat offsets (handles of more than 16K waves), or nullptr
  const uint64_t* totals;         // [2] the lists kernel's totals: totals[1] = MsgBeat groups of this Tick
  const NodeRec* rec;             // [ld]
  uint64_t n_groups;
  uint32_t n_peers, self;
  uint64_t beat_cap;              // groups built at most; enc holds beat_cap * (n_peers - 1) records
  WireMsg* enc;                   // the encoder's input
};

__device__ __forceinline__ void beat_store(WireMsg* dst, uint64_t group, uint64_t term, uint64_t commit, uint32_t from, uint32_t to) {
  uint4* q = reinterpret_cast<uint4*>(dst);
  q[0] = make_uint4((uint32_t)group, (uint32_t)(group >> 32), (uint32_t)term, (uint32_t)(term >> 32));
  q[1] = make_uint4(0u, 0u, 0u, 0u);                                               // log_term, index
  q[2] = make_uint4((uint32_t)commit, (uint32_t)(commit >> 32), 0u, 0u);           // commit, reject_hint
  q[3] = make_uint4(from, (uint32_t)kMsgHeartbeat | (to << 16), 0u, 0u);           // from | type, reject, to, flags | ent_first | n_ents
}

// what a heartbeat needs of a group's NodeRec line: term, committed and the first n_peers match words (the others stay zero)
__device__ __forceinline__ void beat_load(const NodeRec* rec, uint32_t n_peers, uint64_t& term, uint64_t& committed, uint64_t (&m)[kMaxPeers]) {
  const uint4* line = reinterpret_cast<const uint4*>(rec);
  const uint4 c0 = line[0], c2 = line[2], c3 = line[3], c4 = line[4];
  term = (uint64_t)c0.x | ((uint64_t)c0.y << 32);
  committed = (uint64_t)c2.z | ((uint64_t)c2.w << 32);
  m[0] = (uint64_t)c3.z | ((uint64_t)c3.w << 32);
  m[1] = (uint64_t)c4.x | ((uint64_t)c4.y << 32);
  m[2] = (uint64_t)c4.z | ((uint64_t)c4.w << 32);
  if (n_peers > 3) {
    const uint4 c5 = line[5];
    m[3] = (uint64_t)c5.x | ((uint64_t)c5.y << 32);
    m[4] = (uint64_t)c5.z | ((uint64_t)c5.w << 32);
  }
  if (n_peers > 5) {
    const uint4 c6 = line[6];
    m[5] = (uint64_t)c6.x | ((uint64_t)c6.y << 32);
    m[6] = (uint64_t)c6.z | ((uint64_t)c6.w << 32);
  }
  if (n_peers > 7) {
    const uint4 c7 = line[7];
    m[7] = (uint64_t)c7.x | ((uint64_t)c7.y << 32);
    m[8] = (uint64_t)c7.z | ((uint64_t)c7.w << 32);
  }
}

// The rank of a workgroup's 1,024-group block among the groups one of the Tick's bitmaps flags (WHICH = 0: MsgHup, the counts'
// .x; 1: MsgBeat, .y) -- the sum of the earlier waves' counts, or the scan's offsets -- and the block's flagged ids compacted
// into ids[] when any of them has a rank below n_built.  red / mine: kWaves words of LDS each; ids: 4 * kBlock.  Ends behind a
// barrier.
template <int WHICH>
__device__ __forceinline__ void tick_rank(const uint64_t* bits, const uint4* partials, uint64_t n_chunks, const uint64_t* wave_off, uint64_t n_built,
                                          uint64_t* red, uint32_t* mine, uint32_t* ids, uint64_t& pos, uint32_t& tot) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t first_wave = (uint64_t)blockIdx.x * kWaves;
  auto count = [&](uint64_t i) { return WHICH == 0 ? partials[i].x : partials[i].y; };
  uint64_t acc = 0;
  if (wave_off == nullptr) {
    uint32_t b0 = 0, b1 = 0;
    uint64_t i = tid;
    for (; i + kBlock < first_wave; i += 2 * kBlock) {
      b0 += count(i);
      b1 += count(i + kBlock);
    }
    if (i < first_wave) b0 += count(i);
    acc = (uint64_t)b0 + b1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  } else if (lane == 0 && wave == 0) {
    acc = wave_off[first_wave];
  }
  if (lane == 0) red[wave] = acc;
  if (tid < (uint32_t)kWaves) mine[tid] = first_wave + tid < n_chunks ? count(first_wave + tid) : 0u;
  __syncthreads();
  pos = 0;
  tot = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    pos += red[k];
    tot += mine[k];
  }
  const uint64_t wv = first_wave + wave;
  if (wv < n_chunks && pos < n_built) {  // wave-uniform
    uint32_t loc = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) loc += (uint32_t)k < wave ? mine[k] : 0u;
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    uint64_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = bits[wv * 4 + k];
    uint32_t r = loc + __popcll(w[0] & below) + __popcll(w[1] & below) + __popcll(w[2] & below) + __popcll(w[3] & below);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((w[k] >> lane) & 1) ids[r++] = (uint32_t)(wv * 256 + 4ull * lane + k);
  }
  __syncthreads();
}

// The workgroup's member frames, added once to *members.  red: kWaves words of LDS nobody reads any more.
__device__ __forceinline__ void members_add(uint32_t wrote, uint64_t* red, unsigned long long* members) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wrote += __shfl_xor(wrote, o, 64);
  __syncthreads();  // (red was read behind tick_rank's first barrier)
  if (lane == 0) red[wave] = wrote;
  __syncthreads();
  if (tid == 0) {
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) sum += red[k];
    if (sum != 0) atomicAdd(members, (unsigned long long)sum);
  }
}

// One workgroup per 1,024-group block of the Tick (its four waves' 256-group chunks): for the built groups, MsgHeartbeat to
// every slot p != self.  MASKED: to every such slot of voters[g], a filler in the slot of every other p.  The mask is one 2-byte
// load per built group from the dense `voters` array (its address depends on g alone: it is issued beside the record's loads).
// Whether self is a voter is not asked: a leader whose own bit is clear still beats its members, as upstream's loop over prs
// does.  A built group with an empty mask (a leader by role in an unused slot) gives N - 1 fillers.
template <bool MASKED>
__device__ __forceinline__ void beat_build_body(BeatArgs a, const uint16_t* __restrict__ voters, unsigned long long* members) {
  __shared__ uint64_t red[kWaves];
  __shared__ uint32_t mine[kWaves];
  __shared__ uint32_t ids[kBlock * 4];
  const uint32_t tid = threadIdx.x;
  const uint64_t n_beat = a.totals[1];
  const uint64_t n_built = n_beat < a.beat_cap ? n_beat : a.beat_cap;
  uint64_t pos;  // rank of this block's first MsgBeat group
  uint32_t tot;  // MsgBeat groups of this block
  tick_rank<1>(a.beat_bits, a.partials, a.n_chunks, a.wave_off_beat, n_built, red, mine, ids, pos, tot);
  [[maybe_unused]] uint32_t wrote = 0;
  if (pos < n_built) {
    const uint64_t left = n_built - pos;
    const uint32_t take = left < tot ? (uint32_t)left : tot;  // this block's groups of rank < n_built
    for (uint32_t r = tid; r < take; r += kBlock) {
      const uint64_t g = ids[r];
      const uint64_t at = pos + r;
      uint64_t term = 0, committed = 0;
      uint64_t m[kMaxPeers];
#pragma unroll
      for (int p = 0; p < kMaxPeers; ++p) m[p] = 0;
      uint32_t vm = 0;       // the slots a heartbeat goes to
      if (g < a.n_groups) {  // (the Tick flags no padding group)
        if constexpr (MASKED) vm = voters[g];
        else vm = ~0u;
        beat_load(a.rec + g, a.n_peers, term, committed, m);
      }
#pragma unroll
      for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
        if (p >= a.n_peers || p == a.self) continue;
        const uint64_t slice = p < a.self ? p : p - 1;
        const uint64_t commit = m[p] < committed ? m[p] : committed;
        const bool member = ((vm >> p) & 1u) != 0;
        beat_store(a.enc + slice * n_built + at, g, term, commit, a.self, member ? p : 0xffu);
        if constexpr (MASKED) wrote += member ? 1u : 0u;
      }
    }
  }
  const uint64_t n_slices = a.n_peers - 1;
  fill_refused(a.enc, n_built * n_slices, a.beat_cap * n_slices);  // behind the section
  if constexpr (MASKED) members_add(wrote, red, members);
}
static __global__ __launch_bounds__(kBlock) void beat_build_kernel(BeatArgs a) { beat_build_body<false>(a, nullptr, nullptr); }
static __global__ __launch_bounds__(kBlock) void beat_build_voters_kernel(BeatArgs a, const uint16_t* __restrict__ voters, unsigned long long* members) {
  beat_build_body<true>(a, voters, members);
}

// Behind the encoder: the member frames of the call into the pinned word the host reads beside the encoder's totals; the device
// word is left zero again.
static __global__ void members_tail_kernel(unsigned long long* members, uint64_t* pin_word) {
  if (threadIdx.x == 0) {
    *pin_word = *members;
    *members = 0;
  }
}

}  // namespace raftqk
