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

// One text per step, one instantiation per entry point: a form's differences stand under `if constexpr`, and every __global__
// below instantiates exactly one body (a kernel that chose between two at run time would carry both bodies' LDS and registers).

// does result r send a frame to peer p?
__device__ __forceinline__ bool resp_to(const RespRec& r, bool valid, uint32_t p, const RespLayout& L) {
  return valid && p < L.n_peers && p != L.self && (r.kind == kMsgApp || r.to == p);
}

// MASKED: the layout over each group's own members (raftq_bcast_set_voters on a handle with voter masks loaded).  One rule changes:
// the commit broadcast (kind == kMsgApp) goes to slot p only if p's bit is set in voters[group] -- upstream's bcastAppend ranges
// over r.prs, which IS the membership.  A response to a sender goes to r.to as always, member or not: upstream answers whoever
// sent.  Everything else is the unmasked form's: peer-major, result order inside a slice, fillers only behind the total; a
// broadcast of a group with no member but self has no frame at all.
// The mask is a 2-byte gather of the dense `voters` array by the record's group, issued by broadcast records only.  (The walk lane
// holds the mask in a register and could have written it into the record's `to` / `pad` bytes, which a broadcast does not use;
// that would have changed NodeT<true>::respond and with it the masked walks, and the gather costs one 32-byte sector per broadcast.)

// the slots result r sends a frame to, as a bit mask (bit p: resp_to's verdict over members)
__device__ __forceinline__ uint32_t resp_to_voters(const RespRec& r, bool valid, const RespLayout& L, const uint16_t* __restrict__ voters) {
  if (!valid) return 0u;
  const uint32_t peers = ((1u << L.n_peers) - 1u) & ~(1u << L.self);
  const uint32_t want = r.kind == kMsgApp ? (uint32_t)voters[r.group] : (1u << r.to);
  return want & peers;
}

// the verdict per slot of either form (to: resp_to_voters' mask, MASKED only)
template <bool MASKED>
__device__ __forceinline__ bool resp_dest(const RespRec& r, bool valid, uint32_t p, const RespLayout& L, uint32_t to) {
  if constexpr (MASKED) return ((to >> p) & 1u) != 0;
  else return resp_to(r, valid, p, L);
}

// a record of the encoder's input but for its `to`
__device__ __forceinline__ WireMsg msg_head(uint64_t group, uint64_t term, uint64_t log_term, uint64_t index, uint64_t commit, uint32_t from, uint8_t type,
                                            uint8_t reject, uint32_t ent_first, uint32_t n_ents) {
  WireMsg m;
  m.group = group;
  m.term = term;
  m.log_term = log_term;
  m.index = index;
  m.commit = commit;
  m.reject_hint = 0;
  m.from = from;
  m.type = type;
  m.reject = reject;
  m.flags = 0;
  m.ent_first = ent_first;
  m.n_ents = n_ents;
  return m;
}

// fillers in enc[first .. end), by the whole grid: the encoder counts them as refused and writes nothing for them
__device__ __forceinline__ void fill_refused(WireMsg* enc, uint64_t first, uint64_t end) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t k = first + (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < end; k += stride) {
    WireMsg f{};
    f.to = 0xff;
    enc[k] = f;
  }
}

// (1) frames per peer of every workgroup's kBlock results
template <bool MASKED>
__device__ __forceinline__ void resp_count_body(RespLayout L, const uint16_t* __restrict__ voters) {
  __shared__ uint32_t wc[kWaves][kMaxPeers];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  RespRec r{};
  if (i < L.n) r = L.resp[i];
  const bool valid = i < L.n && r.stamp == L.stamp && r.kind != 0;
  uint32_t to = 0;
  if constexpr (MASKED) to = resp_to_voters(r, valid, L, voters);
#pragma unroll
  for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
    const uint64_t b = __ballot(resp_dest<MASKED>(r, valid, p, L, to));
    if (lane == 0) wc[wave][p] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)kMaxPeers) {
    uint32_t t = 0;
    for (int w = 0; w < kWaves; ++w) t += wc[w][threadIdx.x];
    L.blk_cnt[(uint64_t)blockIdx.x * kMaxPeers + threadIdx.x] = t;
  }
}
static __global__ __launch_bounds__(kBlock) void resp_count_kernel(RespLayout L) { resp_count_body<false>(L, nullptr); }
static __global__ __launch_bounds__(kBlock) void resp_count_voters_kernel(RespLayout L, const uint16_t* __restrict__ voters) {
  resp_count_body<true>(L, voters);
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
// LEAD: the layout with the broadcasts that carry entries in it (raftq_respond_set_lead, raftq_respond_set_props); (1) and (2) are
// shared -- such a result is kind == kMsgApp, which they count as a broadcast already.  The encoder's entry array in HBM has
// P.ent_base + n slots:
//   pad == 1, becomeLeader's: the empty entry of the new term goes to slot ent_base + i, behind every slot a proposal can name
//       (ent_first = ent_base + i, n_ents = 1: no scan), and every frame of the broadcast names that one slot;
//   pad == 2, a forwarded proposal's: the decoder has given the frame's entries the range ent_first .. ent_first + n_ents of an array
//       of at most ent_base headers (its device-side record of position i says which; the headers lie in the caller's page-locked
//       ents[]).  The stamped copy -- Term and Index overwritten, Type / data_off / data_len kept: the pool is the inbound stream --
//       goes to the SAME positions: no scan either.  The wave stamps: for every proposal of its 64 results in turn, lane k takes
//       header k, k + 64, ... (a 300-entry frame is five rounds of the wave, not 300 of one lane).
// Slots no frame names are never read.
struct RespProps {
  const WireMsg* dec;    // [n] the decoder's records in HBM (ent_first / n_ents), or nullptr: no proposal is answered
  const WireEnt* heads;  // the decoder's entry headers, as the device addresses the caller's array
  uint32_t ent_base;     // slots the proposals' entries take in front of the empty entries'
};
template <bool MASKED, bool LEAD>
__device__ __forceinline__ void resp_scatter_body(RespLayout L, WireMsg* __restrict__ enc, uint64_t n_max, const uint16_t* __restrict__ voters,
                                                  WireEnt* __restrict__ ents, RespProps P = RespProps{nullptr, nullptr, 0}) {
  __shared__ uint32_t wc[kWaves][kMaxPeers];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  RespRec r{};
  if (i < L.n) r = L.resp[i];
  const bool valid = i < L.n && r.stamp == L.stamp && r.kind != 0;
  uint32_t to = 0;
  if constexpr (MASKED) to = resp_to_voters(r, valid, L, voters);
  const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint32_t in_wave[kMaxPeers];
#pragma unroll
  for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
    const uint64_t b = __ballot(resp_dest<MASKED>(r, valid, p, L, to));
    in_wave[p] = (uint32_t)__popcll(b & below);
    if (lane == 0) wc[wave][p] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  uint32_t ent_first = 0, n_ents = 0;
  bool stamps = false;  // this result's frames carry the message's own entries
  if (MASKED ? to != 0 : valid) {
    if constexpr (LEAD) {
      if (r.kind == kMsgApp && r.pad == 1) {  // (i < L.n: the array has one slot per result behind ent_base)
        WireEnt e;
        e.term = r.term;
        e.index = r.index + 1;
        e.data_off = 0;
        e.data_len = 0;
        e.type = 0;
        ents[(uint64_t)P.ent_base + i] = e;
        ent_first = P.ent_base + (uint32_t)i;
        n_ents = 1;
      } else if (r.kind == kMsgApp && r.pad == 2 && P.dec != nullptr) {
        const WireMsg d = P.dec[i];
        // (a range the decoder could not store -- more entries than ents_cap: the call fails -- names no slot)
        if ((uint64_t)d.ent_first + d.n_ents <= P.ent_base) {
          ent_first = d.ent_first;
          n_ents = d.n_ents;
          stamps = n_ents != 0;
        }
      }
    }
    WireMsg m = msg_head(r.group, r.term, r.log_term, r.index, r.commit, L.self, r.kind, r.reject, ent_first, n_ents);
#pragma unroll
    for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
      if (!resp_dest<MASKED>(r, valid, p, L, to)) continue;
      uint64_t at = L.peer_off[p] + L.blk_off[(uint64_t)blockIdx.x * kMaxPeers + p] + in_wave[p];
      for (uint32_t w = 0; w < wave; ++w) at += wc[w][p];
      m.to = (uint8_t)p;
      enc[at] = m;
    }
  }
  if constexpr (LEAD) {
    // appendEntry's stamps, by the wave (every lane reaches this: the ballot and the broadcasts are wave-wide)
    uint64_t todo = __ballot(stamps);
    while (todo != 0) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint32_t first = __builtin_amdgcn_readlane(ent_first, src), cnt = __builtin_amdgcn_readlane(n_ents, src);
      const uint64_t term = wave_bcast_u64(r.term, src), index = wave_bcast_u64(r.index, src);
      for (uint32_t k = lane; k < cnt; k += 64) {
        WireEnt e = P.heads[first + k];
        e.term = term;
        e.index = index + 1 + k;
        ents[first + k] = e;
      }
    }
  }
  fill_refused(enc, L.peer_off[L.n_peers], n_max);
}
static __global__ __launch_bounds__(kBlock) void resp_scatter_kernel(RespLayout L, WireMsg* __restrict__ enc, uint64_t n_max) {
  resp_scatter_body<false, false>(L, enc, n_max, nullptr, nullptr);
}
static __global__ __launch_bounds__(kBlock) void resp_scatter_voters_kernel(RespLayout L, WireMsg* __restrict__ enc, uint64_t n_max,
                                                                            const uint16_t* __restrict__ voters) {
  resp_scatter_body<true, false>(L, enc, n_max, voters, nullptr);
}
// (the unmasked form keeps the parameter list it had when it served both forms: it reads no mask)
static __global__ __launch_bounds__(kBlock) void resp_scatter_lead_kernel(RespLayout L, WireMsg* __restrict__ enc, uint64_t n_max, const uint16_t*,
                                                                          WireEnt* __restrict__ ents, RespProps P) {
  resp_scatter_body<false, true>(L, enc, n_max, nullptr, ents, P);
}
static __global__ __launch_bounds__(kBlock) void resp_scatter_lead_voters_kernel(RespLayout L, WireMsg* __restrict__ enc, uint64_t n_max,
                                                                                 const uint16_t* __restrict__ voters, WireEnt* __restrict__ ents,
                                                                                 RespProps P) {
  resp_scatter_body<true, true>(L, enc, n_max, voters, ents, P);
}

}  // namespace raftqk
