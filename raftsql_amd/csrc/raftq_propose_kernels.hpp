// raftq_propose_kernels.hpp -- device code of raftq_propose_frames (include/raftq_wire.h): the leader's appendEntry and
// bcastAppend for a batch of proposing groups (raft.go:211-215 -> etcd raft.stepLeader MsgProp: `r.appendEntry(m.Entries...);
// r.bcastAppend()`), one lane per group, written straight into the input of the streaming encoder that runs behind it.
//
// Round 5 did this on the host, per proposal: handle_proposal + bcast_append (raftq_node.cpp) built N - 1 64-byte message
// records and an entry header per proposal, copied them lane by lane into a page-locked array, and the encoder's readers pulled
// them back over the link -- 2.9 ms of a 4.0 ms turn on one core for 32K groups (profiles/r05/one_node_phases.txt).  The records
// are a pure function of the group's device-resident state (Term, lastIndex, lastTerm, committed) and of which entries were
// proposed: nothing the host has to compute, and nothing that has to cross the link.
//
// MASKED -- proposals over each group's own members (raftq_bcast_set_voters on a handle with voter masks loaded), the masks as a
// last argument.  One body per step, one instantiation per entry point (raftq_respond_kernels.hpp); propose_commit_kernel serves
// both forms.
//
// FWD -- a follower's proposals (raftq_propose_set_forward; etcd raft.stepFollower MsgProp: `m.To = r.lead; r.send(m)`): a record
// whose group this node does not lead is no refusal any more but ONE MsgProp frame to the group's leader, or -- no leader known --
// nothing ("no leader; dropping proposal").  A further instantiation of every body (*_fwd_kernel, *_fwd_voters_kernel,
// propose_commit_fwd_kernel): with the switch off the call launches the entry points it always did, compiled to what they were.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raftq_beat_kernels.hpp"
#include "raftq_step_kernels.hpp"
#include "raftq_wire_parse.hpp"

namespace raftqk {

struct PropRec {  // == raftq_prop_t
  uint64_t group;
  uint32_t ent_first, n_ents;
};
struct PropEnt {  // == raftq_prop_ent_t
  uint64_t data_off;
  uint32_t data_len, type;
};
static_assert(sizeof(PropRec) == 16 && sizeof(PropEnt) == 16, "record layout");

constexpr uint32_t kPropPayload = 1, kPropGroup = 2, kPropCount = 3, kPropRange = 4, kPropNotLeader = 5, kPropTwice = 6;
constexpr uint32_t kPropNoMember = 7, kPropCommits = 8;  // over members only
constexpr uint8_t kPropAppended = 0, kPropForwarded = 1, kPropDropped = 2;  // RAFTQ_PROP_*: what became of a record (FWD)
constexpr uint32_t kPropMaxEnts = 1024;  // raft.Config.MaxSizePerMsg's share of entries (raft.go:157): more go out as the caller's own sends

// Nothing is applied unless every record is sound: a group of this handle, led by this node, named once (the group's list
// count word doubles as the "seen" mark: propose_commit_kernel hands it back zero), 1 .. kPropMaxEnts entries inside prop_ents[],
// every entry's payload inside the pool.
// The records lie in page-locked HOST memory: this kernel reads them there ONCE, coalesced (16 bytes a lane: 1 KB a wave
// instruction over the link), and leaves a copy in device scratch for the kernel behind it -- round 6's first form had both
// kernels read the host arrays: 33 + 36 us for 32K groups, all of it link latency (profiles/r06/node_kernel_stats_first.csv).
// MASKED: two more reasons, both read off the masked Node loaded from the record line the check touches anyway (its lst_cnt is
// the "seen" mark):
//   kPropNoMember  self's bit is clear in voters[g].  Upstream v2.2's appendEntry would dereference a missing Progress
//                  (r.prs[r.id]); CHOICE: refuse.
//   kPropCommits   the commit kernel's sentence "maybeCommit cannot move anything with more than one peer" does not hold over members: a
//                  one-voter group commits on its own append, and under the 2015-era removeNode (which does not call
//                  maybeCommit) so does a group whose membership shrank since its last acknowledgement.  Evaluated exactly --
//                  Match[self] raised to last_index + n_ents as the commit will, then the masked maybe_commit() with its current-term
//                  gate -- on the lane's copy, which is never stored.  The call has no channel for a commit:
//                  raftq_apply_log_deltas has, and a tail report with the unchanged tail settles the commit first.
// Both after the six shared reasons, so a record sound by those is marked (lst_cnt) whatever the new ones say; a refused call's
// commit kernel takes every mark off again.
// FWD: kPropNotLeader is no reason any more, and the two masked reasons are judged for leader records only (a forward goes to
// `lead` whether or not lead or self is a member: upstream's send consults no prs).  Every record sound by the other reasons is
// marked, whatever its role.  The outcome bytes (RAFTQ_PROP_*) leave in this kernel, packed by the wave: two ballots hold the 64
// outcomes, eight lanes spread eight of them each into a 64-bit word -- one 8-byte store a lane, 64 bytes a wave over the link,
// where a byte a lane would be 64 separate writes.  `what`: the handle's outcome array as the device addresses it, a multiple of
// eight bytes long; the host believes it only when the call succeeded.
__device__ __forceinline__ uint8_t prop_outcome(uint8_t role, uint32_t lead, uint32_t self) {
  if (role == kLeader) return kPropAppended;
  // a candidate, a follower that knows no leader -- or one whose lead is itself, a loaded state upstream cannot reach (CHOICE: as
  // raftq_node's handle_proposal, dropped)
  return role == kFollower && lead != 0 && lead - 1 != self ? kPropForwarded : kPropDropped;
}
// byte k of the result = bit k of x
__device__ __forceinline__ uint64_t prop_spread8(uint64_t x) {
  const uint64_t v = ((x & 0xffull) * 0x0101010101010101ull) & 0x8040201008040201ull;
  return ((v + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;
}
template <bool MASKED, bool FWD = false>
__device__ __forceinline__ void propose_check_body(NodeArrays a, const PropRec* __restrict__ props, uint64_t n, const PropEnt* __restrict__ pe,
                                                   uint64_t n_pe, uint64_t pool_bytes, unsigned int* bad, unsigned int stamp, PropRec* __restrict__ props_d,
                                                   PropEnt* __restrict__ pe_d, unsigned long long* why, const uint16_t* __restrict__ voters,
                                                   uint64_t* __restrict__ what = nullptr) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  [[maybe_unused]] uint8_t outcome = kPropAppended;
  // the entry records, one per lane of the first ceil(n_pe / kBlock) workgroups ... (the grid covers max(n, n_pe) lanes)
  uint32_t reason = 0;  // kProp*: what is wrong with record i (the largest (reason, record) of the call goes into *why for the error text)
  if (i < n_pe) {
    const PropEnt e = pe[i];
    pe_d[i] = e;
    if (e.data_len != 0 && (e.data_off > pool_bytes || e.data_len > pool_bytes - e.data_off)) reason = kPropPayload;  // (an entry no record names is checked too: harmless)
  }
  if (i < n) {
    const PropRec p = props[i];
    props_d[i] = p;
    if (p.group >= a.n_groups) reason = kPropGroup;
    else if (p.n_ents == 0 || p.n_ents > kPropMaxEnts) reason = kPropCount;
    else if ((uint64_t)p.ent_first + p.n_ents > n_pe) reason = kPropRange;
    else {
      if constexpr (FWD) outcome = prop_outcome(a.role[p.group], a.rec[p.group].lead, a.self);
      if (!FWD && a.role[p.group] != kLeader) reason = kPropNotLeader;
      else if (atomicAdd(&a.rec[p.group].lst_cnt, 1u) != 0) reason = kPropTwice;
      else if constexpr (MASKED) {
        if (outcome == kPropAppended) {  // (FWD: the member refusals are the leader records')
          NodeT<true> node(a, p.group, voters);
          if (((node.vmask >> a.self) & 1u) == 0) reason = kPropNoMember;
          else {
            const uint64_t tail = node.last_index + p.n_ents;
            if (node.match(a.self) < tail) node.set_match(a.self, tail);
            if (node.maybe_commit()) reason = kPropCommits;
          }
        }
      }
    }
  }
  if constexpr (FWD) {
    const uint64_t b0 = __ballot((outcome & 1u) != 0), b1 = __ballot((outcome & 2u) != 0);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t first = i - lane + 8ull * lane;  // the record of this lane's first byte
    if (lane < 8 && first < n) what[first >> 3] = prop_spread8(b0 >> (8 * lane)) | (prop_spread8(b1 >> (8 * lane)) << 1);
  }
  if (reason) atomicMax(why, ((unsigned long long)(stamp & 0xffffffu) << 40) | ((unsigned long long)reason << 32) | (uint32_t)i);
  if (__ballot(reason != 0) != 0 && (threadIdx.x & 63) == 0) atomicExch(bad, stamp);  // (the word holds this call's stamp: refused)
}
static __global__ __launch_bounds__(kBlock) void propose_check_kernel(NodeArrays a, const PropRec* __restrict__ props, uint64_t n,
                                                                      const PropEnt* __restrict__ pe, uint64_t n_pe, uint64_t pool_bytes,
                                                                      unsigned int* bad, unsigned int stamp, PropRec* __restrict__ props_d,
                                                                      PropEnt* __restrict__ pe_d, unsigned long long* why) {
  propose_check_body<false>(a, props, n, pe, n_pe, pool_bytes, bad, stamp, props_d, pe_d, why, nullptr);
}
static __global__ __launch_bounds__(kBlock) void propose_check_voters_kernel(NodeArrays a, const PropRec* __restrict__ props, uint64_t n,
                                                                             const PropEnt* __restrict__ pe, uint64_t n_pe, uint64_t pool_bytes,
                                                                             unsigned int* bad, unsigned int stamp, PropRec* __restrict__ props_d,
                                                                             PropEnt* __restrict__ pe_d, unsigned long long* why,
                                                                             const uint16_t* __restrict__ voters) {
  propose_check_body<true>(a, props, n, pe, n_pe, pool_bytes, bad, stamp, props_d, pe_d, why, voters);
}
static __global__ __launch_bounds__(kBlock) void propose_check_fwd_kernel(NodeArrays a, const PropRec* __restrict__ props, uint64_t n,
                                                                          const PropEnt* __restrict__ pe, uint64_t n_pe, uint64_t pool_bytes,
                                                                          unsigned int* bad, unsigned int stamp, PropRec* __restrict__ props_d,
                                                                          PropEnt* __restrict__ pe_d, unsigned long long* why, uint64_t* __restrict__ what) {
  propose_check_body<false, true>(a, props, n, pe, n_pe, pool_bytes, bad, stamp, props_d, pe_d, why, nullptr, what);
}
static __global__ __launch_bounds__(kBlock) void propose_check_fwd_voters_kernel(NodeArrays a, const PropRec* __restrict__ props, uint64_t n,
                                                                                 const PropEnt* __restrict__ pe, uint64_t n_pe, uint64_t pool_bytes,
                                                                                 unsigned int* bad, unsigned int stamp, PropRec* __restrict__ props_d,
                                                                                 PropEnt* __restrict__ pe_d, unsigned long long* why,
                                                                                 const uint16_t* __restrict__ voters, uint64_t* __restrict__ what) {
  propose_check_body<true, true>(a, props, n, pe, n_pe, pool_bytes, bad, stamp, props_d, pe_d, why, voters, what);
}

// The call has TWO verdicts -- this check's, and the marshal's (a queued message it refuses, a stream that does not fit `out`) --
// and a failed call has applied nothing (include/raftq_wire.h), so appendEntry is split around the encoder: propose_build_kernel
// in front of it reads the state and writes what bcastAppend sends into the encoder's input, storing NOTHING to the node;
// propose_commit_kernel behind it stores the new tail once both verdicts are on the device.
//
// props / pe: the check kernel's copies in device memory.  msgs_out: the device part of the encoder's message array -- (N - 1) runs of n records, run r = the MsgApps for the r-th peer
// slot other than this node's; ents_out: the device part of its entry-header array, whose first element is entry `ent_base` of
// the whole array (a message's ent_first counts from the array's start).
// MASKED: every entry header is written; of the N - 1 MsgApps only those to a slot whose bit is set in voters[g] exist.  The
// encoder's input stays POSITIONAL, as the heartbeats' (raftq_beat_kernels.hpp): the slot of a peer that is no member of its
// group holds a filler (to = 0xff), which the encoder counts as refused and gives zero bytes.  The workgroup's member frames are
// summed and added once to *members (members_add): the host checks `refused == n_dev - member frames`.
// FWD: a forwarded record's N - 1 slots hold ONE frame, in the run of its leader's slot --
//   MsgProp{To: lead - 1, From: self, Group, Term: 0 (raft.send leaves a MsgProp's Term alone), Entries: {Type, Term: 0, Index: 0, Data}}
// -- and fillers; a dropped record's hold fillers only.  The entry headers are written for every record.  Fillers now exist in the
// unmasked form too, so both forms count the frames they built into *members.
template <bool MASKED, bool FWD = false>
__device__ __forceinline__ void propose_build_body(NodeArrays a, const PropRec* __restrict__ props, uint64_t n, const PropEnt* __restrict__ pe,
                                                   const unsigned int* __restrict__ bad, unsigned int stamp, WireMsg* __restrict__ msgs_out,
                                                   WireEnt* __restrict__ ents_out, uint32_t ent_base, const uint16_t* __restrict__ voters,
                                                   unsigned long long* members) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool refused = *bad == stamp;  // workgroup-uniform
  [[maybe_unused]] uint32_t wrote = 0;
  if (i < n && !refused) {  // (refused: nothing is built, no member frame counted -- the encoder counts every message as refused, the commit kernel takes the marks off)
    const PropRec p = props[i];
    const NodeT<MASKED> node(a, p.group, voters);
    const uint64_t old_last = node.last_index, old_term = node.last_term;
    [[maybe_unused]] uint8_t outcome = kPropAppended;
    if constexpr (FWD) outcome = prop_outcome(node.role, node.lead, a.self);
    // appendEntry's entries: `es[i].Term = r.Term; es[i].Index = li + 1 + i` (the append itself: propose_commit_kernel)
    for (uint32_t k = 0; k < p.n_ents; ++k) {
      const PropEnt e = pe[p.ent_first + k];
      WireEnt w;
      w.term = outcome == kPropAppended ? node.term : 0;  // (a client's entries as they reach stepFollower: neither stamped)
      w.index = outcome == kPropAppended ? old_last + 1 + k : 0;
      w.data_len = e.data_len;
      w.data_off = e.data_len ? e.data_off : 0;
      w.type = e.type;
      ents_out[p.ent_first + k] = w;
    }
    // bcastAppend (over r.prs) -> sendAppend(to) with Progress.Next at the tail: MsgApp{Index: next - 1, LogTerm: term(next - 1), Entries, Commit}
    WireMsg m = msg_head(p.group, node.term, old_term, old_last, node.committed, a.self, kMsgApp, 0, ent_base + p.ent_first, p.n_ents);
    if constexpr (FWD)
      if (outcome != kPropAppended) m = msg_head(p.group, 0, 0, 0, 0, a.self, kMsgProp, 0, ent_base + p.ent_first, p.n_ents);
    uint32_t run = 0;
    for (uint32_t to = 0; to < a.n_peers; ++to) {
      if (to == a.self) continue;
      bool member = true;
      if constexpr (MASKED) member = ((node.vmask >> to) & 1u) != 0;
      if constexpr (FWD)
        if (outcome != kPropAppended) member = outcome == kPropForwarded && to == node.lead - 1;
      if constexpr (MASKED || FWD) wrote += member ? 1u : 0u;
      m.to = member ? (uint8_t)to : (uint8_t)0xff;  // (a filler is any record addressed to 0xff, as beat_store's)
      msgs_out[(uint64_t)run * n + i] = m;
      ++run;
    }
  }
  if constexpr (MASKED || FWD) {
    __shared__ uint64_t red[kWaves];
    members_add(wrote, red, members);
  }
}
static __global__ __launch_bounds__(kBlock) void propose_build_kernel(NodeArrays a, const PropRec* __restrict__ props, uint64_t n,
                                                                      const PropEnt* __restrict__ pe, const unsigned int* __restrict__ bad,
                                                                      unsigned int stamp, WireMsg* __restrict__ msgs_out, WireEnt* __restrict__ ents_out, uint32_t ent_base) {
  propose_build_body<false>(a, props, n, pe, bad, stamp, msgs_out, ents_out, ent_base, nullptr, nullptr);
}
static __global__ __launch_bounds__(kBlock) void propose_build_voters_kernel(NodeArrays a, const PropRec* __restrict__ props, uint64_t n,
                                                                             const PropEnt* __restrict__ pe, const unsigned int* __restrict__ bad,
                                                                             unsigned int stamp, WireMsg* __restrict__ msgs_out, WireEnt* __restrict__ ents_out,
                                                                             uint32_t ent_base, const uint16_t* __restrict__ voters, unsigned long long* members) {
  propose_build_body<true>(a, props, n, pe, bad, stamp, msgs_out, ents_out, ent_base, voters, members);
}
static __global__ __launch_bounds__(kBlock) void propose_build_fwd_kernel(NodeArrays a, const PropRec* __restrict__ props, uint64_t n,
                                                                          const PropEnt* __restrict__ pe, const unsigned int* __restrict__ bad,
                                                                          unsigned int stamp, WireMsg* __restrict__ msgs_out, WireEnt* __restrict__ ents_out,
                                                                          uint32_t ent_base, unsigned long long* members) {
  propose_build_body<false, true>(a, props, n, pe, bad, stamp, msgs_out, ents_out, ent_base, nullptr, members);
}
static __global__ __launch_bounds__(kBlock) void propose_build_fwd_voters_kernel(NodeArrays a, const PropRec* __restrict__ props, uint64_t n,
                                                                                 const PropEnt* __restrict__ pe, const unsigned int* __restrict__ bad,
                                                                                 unsigned int stamp, WireMsg* __restrict__ msgs_out, WireEnt* __restrict__ ents_out,
                                                                                 uint32_t ent_base, const uint16_t* __restrict__ voters, unsigned long long* members) {
  propose_build_body<true, true>(a, props, n, pe, bad, stamp, msgs_out, ents_out, ent_base, voters, members);
}

// appendEntry's state change, behind the encoder on the same stream: `r.raftLog.append(es...); r.prs[r.id].maybeUpdate(lastIndex)`.
// (`r.maybeCommit()` cannot move anything with more than one peer: the leader's own Match is the largest, the quorum-th largest
// is somebody else's and did not change -- the host wrapper refuses a single-peer handle; over members the check refuses a
// record whose append would commit.)  One lane per record, for both forms: what is stored does not depend on the mask.
// Every lane reads the same four words, so every lane takes the same verdict BEFORE any lane stores:
//   *bad == stamp                 the check refused a record
//   pin[1] != fillers             the marshal refused a queued message (pin: the encoder's totals, raftq_wire_kernels.hpp; fillers:
//                                 the slots of non-members, n_dev - *members over members, none otherwise)
//   pin[0] > cap                  the stream does not fit `out`
//   pin[3] != 0                   a wait of the encoder gave up
// the conditions raftq_propose_frames fails on once the host has the same words.  Either way the check's marks come off.
// pin == nullptr: the encoder could not be launched -- the call fails, and this kernel only takes the marks off.
// FWD (`members` is never null: both build forms count): a forwarded or dropped record changes nothing of its group -- its mark
// comes off and that is all this kernel stores for it.
template <bool FWD>
__device__ __forceinline__ void propose_commit_body(NodeArrays a, const PropRec* __restrict__ props, uint64_t n, const unsigned int* __restrict__ bad,
                                                    unsigned int stamp, const uint64_t* __restrict__ pin, uint64_t cap, uint64_t n_dev,
                                                    const unsigned long long* __restrict__ members) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t fillers = members != nullptr ? n_dev - *members : 0;
  const bool whole = pin != nullptr && *bad != stamp && pin[1] == fillers && pin[0] <= cap && pin[3] == 0;
  const PropRec p = props[i];
  if (!whole) {
    if (p.group < a.n_groups) a.rec[p.group].lst_cnt = 0;
    return;
  }
  if constexpr (FWD) {
    if (a.role[p.group] != kLeader) {
      a.rec[p.group].lst_cnt = 0;
      return;
    }
  }
  Node node(a, p.group);
  node.last_index += p.n_ents;
  node.last_term = node.term;
  if (node.match(a.self) < node.last_index) node.set_match(a.self, node.last_index);
  node.store();  // (list words back to empty: the check's mark with them)
}
static __global__ __launch_bounds__(kBlock) void propose_commit_kernel(NodeArrays a, const PropRec* __restrict__ props, uint64_t n,
                                                                       const unsigned int* __restrict__ bad, unsigned int stamp,
                                                                       const uint64_t* __restrict__ pin, uint64_t cap, uint64_t n_dev,
                                                                       const unsigned long long* __restrict__ members) {
  propose_commit_body<false>(a, props, n, bad, stamp, pin, cap, n_dev, members);
}
static __global__ __launch_bounds__(kBlock) void propose_commit_fwd_kernel(NodeArrays a, const PropRec* __restrict__ props, uint64_t n,
                                                                           const unsigned int* __restrict__ bad, unsigned int stamp,
                                                                           const uint64_t* __restrict__ pin, uint64_t cap, uint64_t n_dev,
                                                                           const unsigned long long* __restrict__ members) {
  propose_commit_body<true>(a, props, n, bad, stamp, pin, cap, n_dev, members);
}

}  // namespace raftqk
