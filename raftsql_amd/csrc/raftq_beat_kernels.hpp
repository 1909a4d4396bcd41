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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// One workgroup per 1,024-group block of the Tick (its four waves' 256-group chunks).
static __global__ __launch_bounds__(kBlock) void beat_build_kernel(BeatArgs a) {
  __shared__ uint64_t red[kWaves];
  __shared__ uint32_t mine[kWaves];
  __shared__ uint32_t ids[kBlock * 4];
  __shared__ uint64_t n_beat_s;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t first_wave = (uint64_t)blockIdx.x * kWaves;
  // the block's exclusive offset among the MsgBeat groups: the sum of the earlier waves' counts, or the scan's offsets
  uint64_t acc = 0;
  if (a.wave_off_beat == nullptr) {
    uint32_t b0 = 0, b1 = 0;
    uint64_t i = tid;
    for (; i + kBlock < first_wave; i += 2 * kBlock) {
      b0 += a.partials[i].y;
      b1 += a.partials[i + kBlock].y;
    }
    if (i < first_wave) b0 += a.partials[i].y;
    acc = (uint64_t)b0 + b1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  } else if (lane == 0 && wave == 0) {
    acc = a.wave_off_beat[first_wave];
  }
  if (lane == 0) red[wave] = acc;
  if (tid < (uint32_t)kWaves) mine[tid] = first_wave + tid < a.n_chunks ? a.partials[first_wave + tid].y : 0u;
  if (tid == 0) n_beat_s = a.totals[1];
  __syncthreads();
  uint64_t pos = 0;  // rank of this block's first MsgBeat group
  uint32_t tot = 0;  // MsgBeat groups of this block
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    pos += red[k];
    tot += mine[k];
  }
  const uint64_t n_built = n_beat_s < a.beat_cap ? n_beat_s : a.beat_cap;
  const uint64_t wv = first_wave + wave;
  if (wv < a.n_chunks && pos < n_built) {  // wave-uniform
    uint32_t loc = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) loc += (uint32_t)k < wave ? mine[k] : 0u;
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    uint64_t bb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) bb[k] = a.beat_bits[wv * 4 + k];
    uint32_t r = loc + __popcll(bb[0] & below) + __popcll(bb[1] & below) + __popcll(bb[2] & below) + __popcll(bb[3] & below);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((bb[k] >> lane) & 1) ids[r++] = (uint32_t)(wv * 256 + 4ull * lane + k);
  }
  __syncthreads();
  if (pos < n_built) {
    const uint64_t left = n_built - pos;
    const uint32_t take = left < tot ? (uint32_t)left : tot;  // this block's groups of rank < n_built
    for (uint32_t r = tid; r < take; r += kBlock) {
      const uint64_t g = ids[r];
      const uint64_t at = pos + r;
      const uint4* line = reinterpret_cast<const uint4*>(a.rec + g);
      uint64_t term = 0, committed = 0;
      uint64_t m[kMaxPeers];
#pragma unroll
      for (int p = 0; p < kMaxPeers; ++p) m[p] = 0;
      const bool known = g < a.n_groups;  // (the Tick flags no padding group)
      if (known) {
        const uint4 c0 = line[0], c2 = line[2], c3 = line[3], c4 = line[4];
        term = (uint64_t)c0.x | ((uint64_t)c0.y << 32);
        committed = (uint64_t)c2.z | ((uint64_t)c2.w << 32);
        m[0] = (uint64_t)c3.z | ((uint64_t)c3.w << 32);
        m[1] = (uint64_t)c4.x | ((uint64_t)c4.y << 32);
        m[2] = (uint64_t)c4.z | ((uint64_t)c4.w << 32);
        if (a.n_peers > 3) {
          const uint4 c5 = line[5];
          m[3] = (uint64_t)c5.x | ((uint64_t)c5.y << 32);
          m[4] = (uint64_t)c5.z | ((uint64_t)c5.w << 32);
        }
        if (a.n_peers > 5) {
          const uint4 c6 = line[6];
          m[5] = (uint64_t)c6.x | ((uint64_t)c6.y << 32);
          m[6] = (uint64_t)c6.z | ((uint64_t)c6.w << 32);
        }
        if (a.n_peers > 7) {
          const uint4 c7 = line[7];
          m[7] = (uint64_t)c7.x | ((uint64_t)c7.y << 32);
          m[8] = (uint64_t)c7.z | ((uint64_t)c7.w << 32);
        }
      }
#pragma unroll
      for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
        if (p >= a.n_peers || p == a.self) continue;
        const uint64_t slice = p < a.self ? p : p - 1;
        const uint64_t commit = m[p] < committed ? m[p] : committed;
        beat_store(a.enc + slice * n_built + at, g, term, commit, a.self, known ? p : 0xffu);
      }
    }
  }
  // fillers: the encoder counts them as refused and writes nothing for them
  const uint64_t n_slices = a.n_peers - 1;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t k = n_built * n_slices + (uint64_t)blockIdx.x * kBlock + tid; k < a.beat_cap * n_slices; k += stride) {
    WireMsg f{};
    f.to = 0xff;
    a.enc[k] = f;
  }
}

}  // namespace raftqk
