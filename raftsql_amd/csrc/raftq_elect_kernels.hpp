// raftq_elect_kernels.hpp -- raftq_tick_elect_frames' election round (include/raftq_wire.h): Step(MsgHup) -> campaign() for the
// groups the Tick in front of it flagged MsgHup, applied to the device-resident state where the Tick has just flagged them, and
// the N - 1 MsgVotes of each written into the encoder's input in HBM behind the heartbeat records, peer-major -- for every peer
// slot p != self, ascending, one MsgVote per campaigned group in ascending group order.
//
// A campaign is a function of one 128-byte line, as a heartbeat is (raftq_beat_kernels.hpp): term + 1, vote = self, candidate,
// reset()'s match rows, the vote word with self's grant.  All of it is stated ONCE, in Node (raftq_step_kernels.hpp): a lane
// loads its group through Node, calls become_candidate() + poll(self, granted) -- the two calls step() makes for a local MsgHup
// -- and store(), which writes the record and, where they changed, the dense arrays the sweep, the tally and the Tick read.
// N >= 2 means a quorum of at least two: the candidate's own grant never wins, so becomeLeader is not reachable without masks.
//
// Order comes from the Tick's own per-wave counts and popcounts, beat_build_kernel's shape: a workgroup owns one 1,024-group
// block, ranks its MsgHup bits behind the sum of the earlier waves' counts (or the scan's offsets past 16K waves), compacts the
// ids in LDS, and one lane works per MsgHup group of rank < n_vb = min(MsgHup groups of this Tick, hup_cap).  No atomics, the
// same layout on every run.  Groups of rank >= hup_cap are the caller's: nothing of them is touched.
//
// The result record the host applies (the HardState to persist) is the 32-byte raftq_step_out_s_t whatever format the handle is
// set to: two 16-byte stores to page-locked host memory per campaign.  A vote record is four 16-byte stores (beat_store's
// pattern), neighbouring lanes to neighbouring records of a peer's slice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raftq_beat_kernels.hpp"
#include "raftq_step_kernels.hpp"
#include "raftq_wire_kernels.hpp"

namespace raftqk {

struct ElectArgs {
  const uint64_t* hup_bits;      // [gpad / 64] the Tick's MsgHup bits: word 4 w + k, bit l = group 256 w + 4 l + k
  const uint4* partials;         // [gpad / 256] the Tick's per-wave {MsgHup, MsgBeat} counts
  uint64_t n_chunks;             // gpad / 256
  const uint64_t* wave_off_hup;  // scan_partials_kernel's exclusive MsgHup offsets (handles of more than 16K waves), or nullptr
  const uint64_t* totals;        // [2] the lists kernel's totals: {MsgHup, MsgBeat} groups of this Tick
  NodeArrays a;                  // the handle's records and dense arrays (no response records, no at-tail bitmap)
  uint64_t hup_cap, beat_cap;    // groups campaigned / beaten at most; enc holds (beat_cap + hup_cap) * (n_peers - 1) records
  StepOutS* camp;                // [hup_cap] page-locked host memory: the result of hup id r of the list
  WireMsg* enc;                  // the encoder's input: the heartbeat records first (beat_build_kernel), the votes behind them
};

__device__ __forceinline__ void vote_store(WireMsg* dst, uint64_t group, uint64_t term, uint64_t log_term, uint64_t index, uint32_t from, uint32_t to) {
  uint4* q = reinterpret_cast<uint4*>(dst);
  q[0] = make_uint4((uint32_t)group, (uint32_t)(group >> 32), (uint32_t)term, (uint32_t)(term >> 32));
  q[1] = make_uint4((uint32_t)log_term, (uint32_t)(log_term >> 32), (uint32_t)index, (uint32_t)(index >> 32));
  q[2] = make_uint4(0u, 0u, 0u, 0u);                                   // commit, reject_hint
  q[3] = make_uint4(from, (uint32_t)kMsgVote | (to << 16), 0u, 0u);    // from | type, reject, to, flags | ent_first | n_ents
}

// One workgroup per 1,024-group block of the Tick (its four waves' 256-group chunks).
// MASKED -- over voters (raftq_tick_set_voters on a handle with voter masks loaded; raftq_beat_kernels.hpp says why the sections
// stay positional).  Every MsgHup group is promotable -- tick_voters_kernel flags no other -- and the lane runs the masked Node,
// the one step_voters_kernel uses: become_candidate(), poll(self, granted), then exactly the two arms of Node::step's MsgHup case.
//   granted == q_g: the group's only voter is self.  become_leader(), and camp[r] is Step's RAFTQ_OUT_BECAME_LEADER record for
//     that message: index = the empty entry's, commit = committed (a one-voter group commits its own append), RAFTQ_OUTF_HARDSTATE
//     (and _COMMITTED when the commit moved) and NOT RAFTQ_OUTF_ANSWERED -- the caller appends the empty entry, as after Step.
//     Nobody is asked: every vote slot of the group is a filler.
//   otherwise: RAFTQ_OUT_CAMPAIGN as in the unmasked form, a MsgVote to every member p != self, fillers in the other slots.
// ... of either election kind: type = kMsgVote or kMsgPreVote (the CQ entry points)
__device__ __forceinline__ void vote_store(WireMsg* dst, uint64_t group, uint64_t term, uint64_t log_term, uint64_t index, uint32_t from, uint32_t to,
                                           uint32_t type) {
  uint4* q = reinterpret_cast<uint4*>(dst);
  q[0] = make_uint4((uint32_t)group, (uint32_t)(group >> 32), (uint32_t)term, (uint32_t)(term >> 32));
  q[1] = make_uint4((uint32_t)log_term, (uint32_t)(log_term >> 32), (uint32_t)index, (uint32_t)(index >> 32));
  q[2] = make_uint4(0u, 0u, 0u, 0u);
  q[3] = make_uint4(from, type | (to << 16), 0u, 0u);
}

// One MsgHup group of the round under raftq_set_check_quorum (raftq_tick_set_checks; elect_build_cq_kernel, elect_build_cq_voters_kernel):
// the lane runs Node's CQ form and states no rule of its own -- it steps a local MsgHup through Node::step, the call the *_cq_* walks
// make for the caller's own MsgHup record, and packs step()'s result with put_result, as they do.  What step() gives decides the
// frames: RAFTQ_OUT_CAMPAIGN sends MsgVote at the new term; RAFTQ_OUT_PRE_CAMPAIGN (raftq_set_pre_vote: nothing but role, lead and
// the vote word moved) sends MsgPreVote at term + 1 to the same slots; RAFTQ_OUT_BECAME_LEADER (masked: the own grant was the quorum,
// with or without a pre-election in front) sends nothing.  The first two get RAFTQ_OUTF_ANSWERED.  -> member frames written
template <bool MASKED>
__device__ __forceinline__ uint32_t elect_group_cq(const ElectArgs& e, const uint16_t* __restrict__ voters, WireMsg* votes, uint64_t n_vb, uint64_t g,
                                                   uint64_t at) {
  uint64_t term = 0, last_index = 0, last_term = 0;
  uint32_t ask = 0;           // the slots a frame goes to
  uint32_t type = kMsgVote;   // ... a MsgVote or a MsgPreVote
  StepOutRec o;
  if (g < e.a.n_groups) {  // (the Tick flags no padding group)
    NodeT<MASKED, false, true> node(e.a, g, voters);
    const MsgRec m{g, 0, 0, 0, 0, 0, e.a.self, kMsgHup, 0, {0, 0}, 0};  // the local MsgHup a caller would have stepped
    node.step(m, o);
    node.store();
    if (o.type != kOutBecameLeader) {
      o.flags |= kFlagAnswered;
      if constexpr (MASKED) ask = node.vmask;
      else ask = ~0u;
    }
    const bool pre = o.type == kOutPreCampaign;
    type = pre ? kMsgPreVote : kMsgVote;
    term = pre ? node.term + 1 : node.term;
    last_index = node.last_index;
    last_term = o.log_term;
  } else {
    o = StepOutRec{g, 0, 0, 0, 0, 0, 0, 0, 0, kOutNone, 0, 0, 0};
  }
  put_result<true>(e.camp, at, o, kFmtS32);
  uint32_t wrote = 0;
#pragma unroll
  for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
    if (p >= e.a.n_peers || p == e.a.self) continue;
    const uint64_t slice = p < e.a.self ? p : p - 1;
    const bool member = ((ask >> p) & 1u) != 0;
    vote_store(votes + slice * n_vb + at, g, term, last_term, last_index, e.a.self, member ? p : 0xffu, type);
    wrote += member ? 1u : 0u;
  }
  return wrote;
}

// CQ: every group of the round is elect_group_cq's; ranking, sections and fillers are the same.
template <bool MASKED, bool CQ = false>
__device__ __forceinline__ void elect_build_body(ElectArgs e, const uint16_t* __restrict__ voters, unsigned long long* members) {
  __shared__ uint64_t red[kWaves];
  __shared__ uint32_t mine[kWaves];
  __shared__ uint32_t ids[kBlock * 4];
  const uint32_t tid = threadIdx.x;
  const uint64_t n_hup = e.totals[0], n_beat = e.totals[1];
  const uint64_t n_vb = n_hup < e.hup_cap ? n_hup : e.hup_cap;
  const uint64_t n_bb = n_beat < e.beat_cap ? n_beat : e.beat_cap;
  const uint64_t n_slices = e.a.n_peers - 1;
  uint64_t pos;  // rank of this block's first MsgHup group
  uint32_t tot;  // MsgHup groups of this block
  tick_rank<0>(e.hup_bits, e.partials, e.n_chunks, e.wave_off_hup, n_vb, red, mine, ids, pos, tot);
  [[maybe_unused]] uint32_t wrote = 0;
  if (pos < n_vb) {
    const uint64_t left = n_vb - pos;
    const uint32_t take = left < tot ? (uint32_t)left : tot;  // this block's groups of rank < n_vb
    WireMsg* const votes = e.enc + n_bb * n_slices;
    for (uint32_t r = tid; r < take; r += kBlock) {
      const uint64_t g = ids[r];
      const uint64_t at = pos + r;
      if constexpr (CQ) {
        wrote += elect_group_cq<MASKED>(e, voters, votes, n_vb, g, at);
        continue;
      }
      uint64_t term = 0, last_index = 0, last_term = 0;
      uint32_t ask = 0;  // the slots a MsgVote goes to
      u64x2 c0, c1;
      c0.x = c0.y = c1.x = c1.y = 0;
      if (g < e.a.n_groups) {  // (the Tick flags no padding group)
        NodeT<MASKED> node(e.a, g, voters);
        [[maybe_unused]] const uint64_t commit0 = node.committed;
        // Step(MsgHup) -> campaign(): the calls Node::step makes
        node.become_candidate();
        uint32_t granted, recorded;
        node.poll(e.a.self, true, granted, recorded);
        bool won = false;  // the own grant is a quorum: self is the group's only voter (unmasked, a quorum is at least two)
        if constexpr (MASKED) {
          won = granted == node.quorum();
          if (won) node.become_leader();
        }
        node.store();
        term = node.term; last_index = node.last_index; last_term = node.last_term;
        // == put_result(kFmtS32) of step()'s record: a campaign's commit carries the candidate's lastTerm
        c0.x = term; c0.y = last_index;
        if constexpr (MASKED) {
          uint32_t flags = kFlagHardState;  // (the term moved)
          if (won) flags |= node.committed != commit0 ? kFlagCommitted : 0u;
          else flags |= kFlagAnswered;
          c1.x = won ? node.committed : last_term;
          c1.y = (uint64_t)(uint8_t)node.vote | ((uint64_t)(uint8_t)node.lead << 8) | ((uint64_t)(won ? kOutBecameLeader : kOutCampaign) << 16) |
                 ((uint64_t)flags << 32) | ((uint64_t)node.role << 40);
          ask = won ? 0u : node.vmask;
        } else {
          c1.x = last_term;
          c1.y = (uint64_t)(uint8_t)node.vote | ((uint64_t)kOutCampaign << 16) | ((uint64_t)(kFlagHardState | kFlagAnswered) << 32) |
                 ((uint64_t)node.role << 40);
          ask = ~0u;
        }
      }
      u64x2* cq = reinterpret_cast<u64x2*>(e.camp + at);
      cq[0] = c0;
      cq[1] = c1;
#pragma unroll
      for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) {
        if (p >= e.a.n_peers || p == e.a.self) continue;
        const uint64_t slice = p < e.a.self ? p : p - 1;
        const bool member = ((ask >> p) & 1u) != 0;
        vote_store(votes + slice * n_vb + at, g, term, last_term, last_index, e.a.self, member ? p : 0xffu);
        if constexpr (MASKED) wrote += member ? 1u : 0u;
      }
    }
  }
  fill_refused(e.enc, (n_bb + n_vb) * n_slices, (e.beat_cap + e.hup_cap) * n_slices);  // behind both sections
  if constexpr (MASKED) members_add(wrote, red, members);
}
static __global__ __launch_bounds__(kBlock) void elect_build_kernel(ElectArgs e) { elect_build_body<false>(e, nullptr, nullptr); }
static __global__ __launch_bounds__(kBlock) void elect_build_voters_kernel(ElectArgs e, const uint16_t* __restrict__ voters, unsigned long long* members) {
  elect_build_body<true>(e, voters, members);
}
static __global__ __launch_bounds__(kBlock) void elect_build_cq_kernel(ElectArgs e) { elect_build_body<false, true>(e, nullptr, nullptr); }
static __global__ __launch_bounds__(kBlock) void elect_build_cq_voters_kernel(ElectArgs e, const uint16_t* __restrict__ voters,
                                                                              unsigned long long* members) {
  elect_build_body<true, true>(e, voters, members);
}

}  // namespace raftqk

