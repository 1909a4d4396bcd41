// raftq_respond_kernels.hpp -- raftq_step_frames_respond's layout (include/raftq_wire.h): the walk lanes have written one
// RespRec per stepped message (raftq_step_kernels.hpp Node::respond); these kernels turn them into the encoder's input in HBM,
// peer-major -- for every peer slot p != self, ascending, the frames addressed to p in result order -- and the encoder
// (wire_enc_fused_kernel) marshals them where they lie.
//
// Order comes from scans, never from atomics: (1) per workgroup of kBlock results, how many frames go to each peer;
// (2) one workgroup scans those counts per peer and adds the peers up (peer_off); (3) every result finds its frames' places
// with a ballot / popcount scan inside its workgroup and writes the WireMsg records.  The encoder's message count is fixed at
// launch (n * (N - 1), the worst case): the records behind the last frame are fillers it refuses (to = 255: an empty frame,
// no byte written) -- so the frame offsets past the last frame all hold the total.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raftq_step_kernels.hpp"
#include "raftq_wire_kernels.hpp"

namespace raftqk {

struct RespLayout {
  const RespRec* resp;  // [n], written by the walk
  uint64_t n;
  uint32_t n_peers, self, stamp;
  uint32_t* blk_cnt;    // [blocks][kMaxPeers]
  uint64_t* blk_off;    // [blocks][kMaxPeers]: frames to p in the workgroups before this one
  uint64_t* peer_off;   // [kMaxPeers + 1]: peer_off[p] .. peer_off[p + 1] = p's slice; peer_off[n_peers] = total
};

// does result r send a frame to peer p?
__device__ __forceinline__ bool resp_to(const RespRec& r, bool valid, uint32_t p, const RespLayout& L) {
  return valid && p < L.n_peers && p != L.self && (r.kind == kMsgApp || r.to == p);
}

// (1) frames per peer of every workgroup's kBlock results
static __global__ __launch_bounds__(kBlock) void resp_count_kernel(RespLayout L) {
  __shared__ uint32_t wc[kWaves][kMaxPeers];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  RespRec r{};
  if (i < L.n) r = L.resp[i];
  const bool valid = i < L.n && r.stamp == L.stamp && r.kind != 0;
#pragma unroll
  for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
    const uint64_t b = __ballot(resp_to(r, valid, p, L));
    if (lane == 0) wc[wave][p] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)kMaxPeers) {
    uint32_t t = 0;
    for (int w = 0; w < kWaves; ++w) t += wc[w][threadIdx.x];
    L.blk_cnt[(uint64_t)blockIdx.x * kMaxPeers + threadIdx.x] = t;
  }
}

// (2) ONE workgroup: exclusive scan of every peer's workgroup counts, then the peers' slices one after the other
static __global__ __launch_bounds__(kBlock) void resp_scan_kernel(RespLayout L, uint32_t blocks) {
  __shared__ uint64_t wave_tot[kWaves];
  __shared__ uint64_t tot[kMaxPeers];
  for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < blocks; b0 += kBlock) {
      const uint32_t b = b0 + threadIdx.x;
      const uint64_t v = b < blocks ? L.blk_cnt[(uint64_t)b * kMaxPeers + p] : 0;
      uint64_t chunk;
      const uint64_t ex = block_exclusive_u64(v, wave_tot, &chunk);
      if (b < blocks) L.blk_off[(uint64_t)b * kMaxPeers + p] = carry + ex;
      carry += chunk;
      __syncthreads();  // wave_tot is reused by the next chunk
    }
    if (threadIdx.x == 0) tot[p] = carry;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t at = 0;
    for (uint32_t p = 0; p < L.n_peers; ++p) {
      L.peer_off[p] = at;
      at += tot[p];
    }
    L.peer_off[L.n_peers] = at;
  }
}

// (3) the records, peer-major, into the encoder's input; then the fillers up to n_max
static __global__ __launch_bounds__(kBlock) void resp_scatter_kernel(RespLayout L, WireMsg* __restrict__ enc, uint64_t n_max) {
  __shared__ uint32_t wc[kWaves][kMaxPeers];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  RespRec r{};
  if (i < L.n) r = L.resp[i];
  const bool valid = i < L.n && r.stamp == L.stamp && r.kind != 0;
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint32_t in_wave[kMaxPeers];
#pragma unroll
  for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
    const uint64_t b = __ballot(resp_to(r, valid, p, L));
    in_wave[p] = (uint32_t)__popcll(b & below);
    if (lane == 0) wc[wave][p] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (valid) {
    WireMsg m;
    m.group = r.group;
    m.term = r.term;
    m.log_term = r.log_term;
    m.index = r.index;
    m.commit = r.commit;
    m.reject_hint = 0;
    m.from = L.self;
    m.type = r.kind;
    m.reject = r.reject;
    m.flags = 0;
    m.ent_first = 0;
    m.n_ents = 0;
#pragma unroll
    for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
      if (!resp_to(r, valid, p, L)) continue;
      uint64_t at = L.peer_off[p] + L.blk_off[(uint64_t)blockIdx.x * kMaxPeers + p] + in_wave[p];
      for (uint32_t w = 0; w < wave; ++w) at += wc[w][p];
      m.to = (uint8_t)p;
      enc[at] = m;
    }
  }
  // fillers: the encoder counts them as refused and writes nothing for them
  const uint64_t total = L.peer_off[L.n_peers];
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t k = total + i; k < n_max; k += stride) {
    WireMsg f{};
    f.to = 0xff;
    enc[k] = f;
  }
}

// ---- the layout over each group's own members (raftq_bcast_set_voters on a handle with voter masks loaded) ------------------------
// Twins of (1) and (3); (2) is shared.  One rule changes: the commit broadcast (kind == kMsgApp) goes to slot p only if p's bit
// is set in voters[group] -- upstream's bcastAppend ranges over r.prs, which IS the membership.  A response to a sender goes to
// r.to as always, member or not: upstream answers whoever sent.  Everything else is the parents': peer-major, result order inside
// a slice, fillers only behind the total; a broadcast of a group with no member but self has no frame at all.
// The mask is a 2-byte gather of the dense `voters` array by the record's group, issued by broadcast records only.  (The walk lane
// holds the mask in a register and could have written it into the record's `to` / `pad` bytes, which a broadcast does not use;
// that would have changed NodeT<true>::respond and with it the assembly of the masked walks -- profiles/r14/isa_unchanged.txt
// keeps them what they were, and the gather costs one 32-byte sector per broadcast.)
// Kernels of their own, with the masks as an argument behind the parents': RespLayout keeps its members and the parents their
// kernarg offsets and their assembly.

// the slots result r sends a frame to, as a bit mask (bit p: resp_to's verdict over members)
__device__ __forceinline__ uint32_t resp_to_voters(const RespRec& r, bool valid, const RespLayout& L, const uint16_t* __restrict__ voters) {
  if (!valid) return 0u;
  const uint32_t peers = ((1u << L.n_peers) - 1u) & ~(1u << L.self);
  const uint32_t want = r.kind == kMsgApp ? (uint32_t)voters[r.group] : (1u << r.to);
  return want & peers;
}

// (1) over members
static __global__ __launch_bounds__(kBlock) void resp_count_voters_kernel(RespLayout L, const uint16_t* __restrict__ voters) {
  __shared__ uint32_t wc[kWaves][kMaxPeers];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  RespRec r{};
  if (i < L.n) r = L.resp[i];
  const bool valid = i < L.n && r.stamp == L.stamp && r.kind != 0;
  const uint32_t to = resp_to_voters(r, valid, L, voters);
#pragma unroll
  for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
    const uint64_t b = __ballot(((to >> p) & 1u) != 0);
    if (lane == 0) wc[wave][p] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)kMaxPeers) {
    uint32_t t = 0;
    for (int w = 0; w < kWaves; ++w) t += wc[w][threadIdx.x];
    L.blk_cnt[(uint64_t)blockIdx.x * kMaxPeers + threadIdx.x] = t;
  }
}

// (3) over members
static __global__ __launch_bounds__(kBlock) void resp_scatter_voters_kernel(RespLayout L, WireMsg* __restrict__ enc, uint64_t n_max,
                                                                            const uint16_t* __restrict__ voters) {
  __shared__ uint32_t wc[kWaves][kMaxPeers];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  RespRec r{};
  if (i < L.n) r = L.resp[i];
  const bool valid = i < L.n && r.stamp == L.stamp && r.kind != 0;
  const uint32_t to = resp_to_voters(r, valid, L, voters);
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint32_t in_wave[kMaxPeers];
#pragma unroll
  for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
    const uint64_t b = __ballot(((to >> p) & 1u) != 0);
    in_wave[p] = (uint32_t)__popcll(b & below);
    if (lane == 0) wc[wave][p] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (to != 0) {
    WireMsg m;
    m.group = r.group;
    m.term = r.term;
    m.log_term = r.log_term;
    m.index = r.index;
    m.commit = r.commit;
    m.reject_hint = 0;
    m.from = L.self;
    m.type = r.kind;
    m.reject = r.reject;
    m.flags = 0;
    m.ent_first = 0;
    m.n_ents = 0;
#pragma unroll
    for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
      if (((to >> p) & 1u) == 0) continue;
      uint64_t at = L.peer_off[p] + L.blk_off[(uint64_t)blockIdx.x * kMaxPeers + p] + in_wave[p];
      for (uint32_t w = 0; w < wave; ++w) at += wc[w][p];
      m.to = (uint8_t)p;
      enc[at] = m;
    }
  }
  // fillers: the encoder counts them as refused and writes nothing for them
  const uint64_t total = L.peer_off[L.n_peers];
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t k = total + i; k < n_max; k += stride) {
    WireMsg f{};
    f.to = 0xff;
    enc[k] = f;
  }
}

// ---- the layout with becomeLeader's broadcast in it (raftq_respond_set_lead) -------------------------------------------------------
// A twin of (3), over every slot (voters == nullptr) or over members; (1) and (2) are shared -- a win is kind == kMsgApp, which they
// count as a broadcast already.  What is new: a record with pad == 1 carries the empty entry of the new term.  Its header goes into
// the encoder's entry array in HBM at slot i, the result's own position (ent_first = i, n_ents = 1: no scan), and every frame of the
// broadcast names that one slot.  Slots of results that carry no entry are never read.  A kernel of its own with the new arguments
// behind the parents': those keep their kernarg offsets and their assembly.
static __global__ __launch_bounds__(kBlock) void resp_scatter_lead_kernel(RespLayout L, WireMsg* __restrict__ enc, uint64_t n_max,
                                                                          const uint16_t* __restrict__ voters, WireEnt* __restrict__ ents) {
  __shared__ uint32_t wc[kWaves][kMaxPeers];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  RespRec r{};
  if (i < L.n) r = L.resp[i];
  const bool valid = i < L.n && r.stamp == L.stamp && r.kind != 0;
  uint32_t to = 0;
  if (voters != nullptr) {
    to = resp_to_voters(r, valid, L, voters);
  } else {
#pragma unroll
    for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) to |= resp_to(r, valid, p, L) ? 1u << p : 0u;
  }
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint32_t in_wave[kMaxPeers];
#pragma unroll
  for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
    const uint64_t b = __ballot(((to >> p) & 1u) != 0);
    in_wave[p] = (uint32_t)__popcll(b & below);
    if (lane == 0) wc[wave][p] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (to != 0) {
    const bool lead = r.kind == kMsgApp && r.pad == 1;
    if (lead) {  // (i < L.n: the array has one slot per result)
      WireEnt e;
      e.term = r.term;
      e.index = r.index + 1;
      e.data_off = 0;
      e.data_len = 0;
      e.type = 0;
      ents[i] = e;
    }
    WireMsg m;
    m.group = r.group;
    m.term = r.term;
    m.log_term = r.log_term;
    m.index = r.index;
    m.commit = r.commit;
    m.reject_hint = 0;
    m.from = L.self;
    m.type = r.kind;
    m.reject = r.reject;
    m.flags = 0;
    m.ent_first = lead ? (uint32_t)i : 0u;
    m.n_ents = lead ? 1u : 0u;
#pragma unroll
    for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
      if (((to >> p) & 1u) == 0) continue;
      uint64_t at = L.peer_off[p] + L.blk_off[(uint64_t)blockIdx.x * kMaxPeers + p] + in_wave[p];
      for (uint32_t w = 0; w < wave; ++w) at += wc[w][p];
      m.to = (uint8_t)p;
      enc[at] = m;
    }
  }
  // fillers: the encoder counts them as refused and writes nothing for them
  const uint64_t total = L.peer_off[L.n_peers];
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t k = total + i; k < n_max; k += stride) {
    WireMsg f{};
    f.to = 0xff;
    enc[k] = f;
  }
}

}  // namespace raftqk
