// raftq_step_kernels.hpp -- device code of the batched raft Step (include/raftq_step.h).
//
// etcd's raft.Step is a per-group sequential state machine; what is parallel is the G
// groups.  A batch is therefore grouped by raft group with the arrival order kept, and one
// lane per group gathers its group's scalar state into registers, applies the group's
// messages in order and scatters the state back.  Two ways to group (same bytes out):
//   list walk (default):  step_link_kernel threads every message onto its group's list with
//       three atomics, the lane of the group's first message orders and walks it (2b / 3b)
//   sorted walk (fallback for long runs): (1) keys, (2) stable radix sort of (group, position)
//       (raftq_sort_kernels.hpp), (3) step_kernel: one lane per run of equal keys
// Different lanes touch different groups, so there are no atomics on state and the result is
// identical to calling Step message by message (tests/test_step_gpu.py).
//
// Restates (2015-era etcd raft, reached from raft.go:268-270 / :223-224): Step, stepLeader,
// stepCandidate, stepFollower, reset, becomeFollower / becomeCandidate / becomeLeader,
// campaign, poll, maybeCommit, handleHeartbeat, raftLog.isUpToDate / commitTo,
// Progress.maybeUpdate.  Sparse, scattered access: bound by HBM latency / PCIe, not bandwidth.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raftq_kernels.hpp"

namespace raftqk {

struct MsgRec {  // == raftq_msg_t
  uint64_t group, term, log_term, index, commit, reject_hint;
  uint32_t from;
  uint8_t type, reject, pad[2];
  uint64_t resv;
};
struct StepOutRec {  // == raftq_step_out_t
  uint64_t group, term, index, log_term, commit, last_index;
  uint32_t to, vote, lead;
  uint8_t type, reject, flags, role;
};
struct LogDeltaRec {  // == raftq_log_delta_t
  uint64_t group, last_index, last_term, commit_to;
};
struct StepOutC {  // == raftq_step_out_c_t: the result record without what the caller's own batch already says
  uint64_t term, index, commit, aux;
  uint8_t vote, lead, type, reject, flags, role, pad[2];
};
struct StepOutS {  // == raftq_step_out_s_t: ... and without aux (include/raftq_step.h says what carried it)
  uint64_t term, index, commit;
  uint8_t vote, lead, type, reject, flags, role, pad[2];
};
static_assert(sizeof(MsgRec) == 64 && sizeof(StepOutRec) == 64 && sizeof(LogDeltaRec) == 32 && sizeof(StepOutC) == 40 && sizeof(StepOutS) == 32,
              "record layout");
constexpr uint8_t kFmtFull = 0, kFmtC40 = 1, kFmtS32 = 2;  // raftq_step_set_compact

// Everything Step's common paths need of a group, in ONE 128-byte line (round 6): the raft scalars, the words of the group's
// message list of the batch in flight (step_link_kernel / step_lists_kernel), and a copy of what the dense kernels own -- role,
// committed, the current-term gate and the N match words.  Round 3 kept each scalar in an array of its own (18 scattered lines
// per touched group); round 4 made the scalars one 64-byte record but still read role, committed, match[from] and -- for every
// acknowledgement -- all N match rows and the gate from their dense arrays: 33 MB read per 64K-message batch by the DRAM request
// counters, x2.3 of what the walk needs (profiles/r05/pmc_legs_summary.txt step_lists_kernel: 1.05 M 32-byte requests).  Now a
// touched group is one line in and one line out.
//
// What the dense kernels stream stays peer-major / group-major SoA and stays AUTHORITATIVE: match, committed (the sweep),
// first_idx (the gated sweep), role / elapsed (Tick), the vote words (the tally).  Step writes a word it changes to BOTH places.
// A call that changes the dense arrays without Step (raftq_load_*, a batching turn's ingest, an adopted sweep, a campaign list)
// marks the copies stale (raftq_t::node_mirror_fresh); the next Step-family call re-reads them (node_mirror_kernel) first.
// raftq_node -- Step, tail reports, proposals, Tick (which writes neither) -- never does.
struct __attribute__((aligned(128))) NodeRec {
  uint64_t term, last_index, last_term;
  uint32_t lst_head;  // batch position of the last-linked message of the group, kNil = none
  uint32_t lst_cnt;   // messages of the group in this batch
  uint32_t lst_min;   // smallest batch position of the group
  uint8_t vote, lead; // 0 = None, else slot + 1
  uint8_t role, pad;  // copy of role[g]
  uint64_t committed, first_idx;  // copies of committed[g], first_idx[g]
  uint64_t match[kMaxPeers];      // copies of match[p][g]
};
static_assert(sizeof(NodeRec) == 128, "one cache line");

struct NodeArrays {
  NodeRec* rec;     // [ld]
  uint8_t* role;
  uint32_t* elapsed;
  uint64_t* committed;
  uint64_t* first_idx;
  uint64_t* match;  // [N][ld]
  uint8_t* votes;   // [ld] packed vote words: 2 bits per peer, 16-bit words (N <= 8) or 32-bit (N = 9)
  uint64_t ld;
  uint32_t n_peers, self;
  bool msg_flags;   // the handle opted in to RAFTQ_MSGF_* (raftq_step_set_msg_flags): otherwise a record's pad bytes are padding
  uint8_t recs;     // whose records the batch holds: kRecsCaller, kRecsWire (raftq_step_submit_wire: the decoder's, strict) or
                    // kRecsFrames (raftq_step_frames: the decoder's, with RAFTQ_MSGF_* set by it)
  bool props = false;  // raftq_step_set_props: a MsgProp that says how many entries it carries is stepped (it is an unknown kind otherwise)
  // NodeT's LEAD form only (raftq_step_frames_respond): which broadcasts with entries respond() answers -- becomeLeader's
  // (raftq_respond_set_lead) and a forwarded proposal's (raftq_respond_set_props).  The form is launched when either is set.
  bool ans_lead = false, ans_props = false;
  uint64_t n_groups;
  uint32_t* self_max = nullptr;  // the handle's self-max word (raftq_kernels.hpp): a store that breaks the fact clears it
  // raftq_step_frames_respond only (nullptr otherwise): the walk writes resp[i] for every message it steps, stamped resp_stamp,
  // and reads the caller's at-tail bitmap (page-locked host memory, one word per 64 groups; nullptr = all clear)
  struct RespRec* resp = nullptr;
  const uint64_t* at_tail = nullptr;
  uint32_t resp_stamp = 0;
  uint32_t resp_ent_base = 0;  // ans_props: entry headers the decoder can hand back -- a proposal whose range ends beyond is the host's
  // raftq_set_check_quorum (nullptr otherwise; read by NodeT's CQ form alone, which is what the handle then launches): the dense word Tick's
  // tick_check_kernel streams -- activity bits (Progress.RecentActive, bit p) | lead_elapsed << 16 -- and the handle's election_tick,
  // which the lease compares the Tick-owned elapsed[g] with
  uint32_t* cq = nullptr;
  uint32_t election_tick = 0;
  // raftq_set_pre_vote (only ever true beside cq, and read by NodeT's CQ form alone): the five rules of include/raftq_step.h "PreVote"
  bool pv = false;
  // raftq_set_lead_transfer (likewise): the rules of include/raftq_step.h "Leadership transfer"; leadTransferee is bits 12..15 of the cq word
  bool lt = false;
  // raftq_set_read_index (likewise): 0 = off, kReadSafe, kReadLease -- the rules of include/raftq_step.h "ReadIndex in Step".  The read
  // records themselves are no member: a pointer here would move every kernel's arguments behind NodeArrays, so the *_cq_* walks take
  // them as a parameter of their own (RAFTQ_WALK_READS)
  uint8_t ri = 0;
};
static_assert(sizeof(NodeArrays) == 136, "a by-value argument of every Step-family kernel: its size moves their other arguments");
constexpr uint8_t kReadSafe = 1, kReadLease = 2;
// (ReadRec, raftq_set_read_index's record, is raftq_kernels.hpp's: the host's bulk calls speak it too)
constexpr uint8_t kRecsCaller = 0, kRecsWire = 1, kRecsFrames = 2;

constexpr uint8_t kMsgHup = 0, kMsgBeat = 1, kMsgProp = 2, kMsgApp = 3, kMsgAppResp = 4, kMsgVote = 5, kMsgVoteResp = 6,
                  kMsgHeartbeat = 8, kMsgHeartbeatResp = 9, kMsgCheckQuorum = 12, kMsgTransferLeader = 13, kMsgTimeoutNow = 14,
                  kMsgReadIndex = 15, kMsgReadIndexResp = 16, kMsgPreVote = 17, kMsgPreVoteResp = 18;
constexpr uint8_t kOutNone = 0, kOutVoteResp = 1, kOutHeartbeatResp = 2, kOutCampaign = 3, kOutBecameLeader = 4,
                  kOutProgress = 5, kOutBcastHeartbeat = 6, kOutAppend = 7, kOutAppended = 8, kOutDeferred = 9, kOutSkipped = 10,
                  kOutHeld = 11, kOutProposed = 12, kOutForward = 13, kOutPreCampaign = 14, kOutPreVoteResp = 15, kOutTermResp = 16,
                  kOutTransfer = 17, kOutReadIndex = 18, kOutReadState = 19;
constexpr uint8_t kMsgfEntries = 0x80, kMsgfBarrier = 0x40, kMsgfHold = 0x20, kMsgfSkip = 0x10;  // raftq_msg_t._pad[1]: RAFTQ_MSGF_*
constexpr uint8_t kFlagHardState = 1, kFlagCommitted = 2, kFlagUpdated = 4, kFlagSteppedDown = 8;
constexpr uint8_t kFlagTimeoutNow = 0x20;  // RAFTQ_OUTF_TIMEOUT_NOW: the transferee's Match is the tail -- send it MsgTimeoutNow
constexpr uint8_t kFlagReadReady = 0x40;   // RAFTQ_OUTF_READ_READY: a quorum has confirmed the read(s) -- release them
constexpr uint8_t kFlagAnswered = 0x10;  // RAFTQ_OUTF_ANSWERED: the messages the result calls for were built on the device

// What result i calls for, as the walk lane that stepped it saw the group (raftq_step_frames_respond; raftq_respond_kernels.hpp
// lays the frames out).  kind = the raftpb type of the message(s) to send, 0 = none built on the device; kMsgApp is the commit
// broadcast: one empty MsgApp to every peer but self; with pad = 1 (NodeT's LEAD form only) it is becomeLeader's broadcast and
// carries the empty entry {Term: term, Index: index + 1}; with pad = 2 (the same form) it is a forwarded proposal's bcastAppend and
// carries the message's own entries, stamped {Term: term, Index: index + 1 + k} (the layout finds them through the decoder's
// record of position i).  Valid only with this call's stamp (stale records read as "none").
struct RespRec {
  uint64_t group, term, index, log_term, commit;
  uint32_t stamp;
  uint8_t kind, reject, to, pad;
};
static_assert(sizeof(RespRec) == 48, "record layout");
constexpr uint8_t kFollower = 0, kCandidate = 1, kLeader = 2;
constexpr uint8_t kPreCandidate = 3;  // RAFTQ_ROLE_PRE_CANDIDATE: only under raftq_set_pre_vote; every other walk takes it for a follower without a leader

// result record i, in the handle's format.  Compact drops group and addressee (= msgs[i].group / .from) and folds
// log_term / last_index into one slot: log_term is only set by the two result types whose index IS last_index.
// PV: the *_cq_* walks' form, in which RAFTQ_OUT_PRE_CAMPAIGN (raftq_set_pre_vote) is packed as RAFTQ_OUT_CAMPAIGN is; the other
// walks never give that type and keep the form they had.  Likewise RAFTQ_OUT_READ_INDEX and a RAFTQ_OUT_PROGRESS with
// RAFTQ_OUTF_READ_READY (raftq_set_read_index): their log_term -- a read's sequence number -- rides the commit slot of both compact forms.
// RD: the *_cq_* walks' alone -- the one other user of the PV form, elect_build_cq_kernel, gives neither result and keeps its code.
template <bool RD>
__device__ __forceinline__ bool carries_read(const StepOutRec& o) {
  if constexpr (RD) return o.type == kOutReadIndex || (o.type == kOutProgress && (o.flags & kFlagReadReady) != 0);
  return false;
}
template <bool PV = false, bool RD = false>
__device__ __forceinline__ void put_result(void* out, uint64_t i, const StepOutRec& o, uint8_t fmt) {
  if (fmt == kFmtFull) {
    static_cast<StepOutRec*>(out)[i] = o;
    return;
  }
  if (fmt == kFmtS32) {
    StepOutS c;
    c.term = o.term;
    c.index = o.index;
    c.commit = (o.type == kOutCampaign || (PV && o.type == kOutPreCampaign) || carries_read<RD>(o)) ? o.log_term : o.commit;
    c.vote = (uint8_t)o.vote;
    c.lead = (uint8_t)o.lead;
    c.type = o.type;
    c.reject = o.reject;
    c.flags = o.flags;
    c.role = o.role;
    c.pad[0] = c.pad[1] = 0;
    static_cast<StepOutS*>(out)[i] = c;
    return;
  }
  StepOutC c;
  c.term = o.term;
  c.index = o.index;
  c.commit = carries_read<RD>(o) ? o.log_term : o.commit;
  c.aux = (o.type == kOutCampaign || o.type == kOutBecameLeader || (PV && o.type == kOutPreCampaign)) ? o.log_term : o.last_index;
  c.vote = (uint8_t)o.vote;
  c.lead = (uint8_t)o.lead;
  c.type = o.type;
  c.reject = o.reject;
  c.flags = o.flags;
  c.role = o.role;
  c.pad[0] = c.pad[1] = 0;
  static_cast<StepOutC*>(out)[i] = c;
}

// zero the batch's {touched-group count, bad flag} (a plain kernel: no runtime blit in the chain)
static __global__ void step_reset_kernel(unsigned long long* flags) {
  if (threadIdx.x < 2) flags[threadIdx.x] = 0;
}

// ---- (0) packed inbound records (raftq_msg40_t) -> the 64-byte records everything below reads.  In HBM: the
// widening costs a 3 us launch and no PCIe byte.
struct Msg40Rec {  // == raftq_msg40_t
  uint32_t group;
  uint8_t from, type, reject, pad;
  uint64_t term, index, aux, commit;
};
static_assert(sizeof(Msg40Rec) == 40, "ABI struct mismatch");

static __global__ __launch_bounds__(kBlock) void step_unpack40_kernel(const Msg40Rec* __restrict__ in, MsgRec* __restrict__ out,
                                                                      uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const Msg40Rec r = in[i];
  MsgRec m;
  m.group = r.group;
  m.term = r.term;
  m.index = r.index;
  m.commit = r.commit;
  const bool hint = r.type == kMsgAppResp;  // the one kind that carries a RejectHint (and no LogTerm)
  m.log_term = hint ? 0 : r.aux;
  m.reject_hint = hint ? r.aux : 0;
  m.from = r.from;
  m.type = r.type;
  m.reject = r.reject;
  m.pad[0] = m.pad[1] = 0;
  m.resv = 0;
  out[i] = m;
}

// What the two grouping kernels make of record i.  kSkip: RAFTQ_MSGF_SKIP, nobody's (answered on the spot, never grouped);
// kBad: fails the batch; kTake: goes to its group (a RAFTQ_MSGF_HOLD record too: only its group is looked at).
enum RecClass : int { kTake = 0, kSkip = 1, kBad = 2 };
// the number of entries a record says it carries under RAFTQ_MSGF_ENTRIES (the decoder's record keeps ent_first | n_ents << 32
// where the caller's keeps the count)
__device__ __forceinline__ uint64_t entry_count(const MsgRec& m, uint8_t recs) {
  return recs == kRecsFrames ? m.resv >> 32 : m.resv & 0xffffffffull;
}
// props (raftq_step_set_props): a MsgProp is a known kind when it says how many entries it carries and carries at least one
// (CHOICE: upstream's stepLeader panics on an empty one).  raftq_step_submit_wire's records carry no RAFTQ_MSGF_*: it stays
// malformed there.
// cq (raftq_set_check_quorum): RAFTQ_MSG_CHECK_QUORUM is a known, local kind in a caller's own records -- never in a record a
// decoder made of a peer's frame.
// pv (raftq_set_pre_vote): MsgPreVote and MsgPreVoteResp are known kinds, a peer's like MsgVote and MsgVoteResp, in every kind of record.
// lt (raftq_set_lead_transfer): MsgTransferLeader and MsgTimeoutNow likewise -- a MsgTransferLeader's `from` is the transferee's slot in
// its local form (term 0) too, so neither is a local kind: `from` >= N is malformed.
// ri (raftq_set_read_index, either mode): MsgReadIndex and MsgReadIndexResp likewise -- a MsgReadIndex's `from` is the requester's slot
// in its local form (term 0) too.
__device__ __forceinline__ RecClass classify(const MsgRec& m, uint64_t n_groups, uint32_t n_peers, bool msg_flags, uint8_t recs, bool props,
                                             bool cq = false, bool pv = false, bool lt = false, bool ri = false) {
  const uint8_t fl = msg_flags ? m.pad[1] : (uint8_t)0;
  if (fl & kMsgfSkip) return kSkip;
  if (m.group >= n_groups) return kBad;
  if (fl & kMsgfHold) return kTake;
  const uint8_t t = m.type;
  if (t == kMsgProp)
    return props && recs != kRecsWire && (fl & kMsgfEntries) != 0 && entry_count(m, recs) != 0 && m.from < n_peers ? kTake : kBad;
  const bool local = t == kMsgHup || t == kMsgBeat || (t == kMsgCheckQuorum && cq && recs == kRecsCaller);
  const bool known = local || t == kMsgApp || t == kMsgAppResp || t == kMsgVote || t == kMsgVoteResp ||
                     t == kMsgHeartbeat || t == kMsgHeartbeatResp || (pv && (t == kMsgPreVote || t == kMsgPreVoteResp)) ||
                     (lt && (t == kMsgTransferLeader || t == kMsgTimeoutNow)) || (ri && (t == kMsgReadIndex || t == kMsgReadIndexResp));
  if (!known || (!local && m.from >= n_peers)) return kBad;
  // records decoded on the device from stream frames (raftq_step_submit_wire) also carry the addressee's slot and the
  // decoder's flags in the two pad bytes: a frame that did not parse, or one addressed to no peer of this cluster, fails
  // the batch like any malformed message.  (raftq_step_frames' decoder has made those RAFTQ_MSGF_SKIP itself.)
  if (recs == kRecsWire && ((m.pad[1] & 1u) != 0 || m.pad[0] >= n_peers)) return kBad;
  return kTake;
}
__device__ __forceinline__ void put_skipped(void* out, uint64_t i, uint8_t compact) {
  StepOutRec o;
  __builtin_memset(&o, 0, sizeof o);
  o.type = kOutSkipped;
  put_result(out, i, o, compact);
}

// ---- (1) validate + sort keys.  The batch was DMA-copied from the pinned staging area into
// HBM; one lane per record reads its first 16 B (group, term) and the 16 B holding from/type.
// A malformed record raises *bad; step_kernel then applies nothing (the ABI's all-or-nothing rule).
static __global__ __launch_bounds__(kBlock) void step_keys_kernel(const MsgRec* __restrict__ msgs,
                                                                  uint64_t* __restrict__ keys,
                                                                  uint32_t* __restrict__ order, uint64_t n,
                                                                  uint64_t n_groups, uint32_t n_peers,
                                                                  unsigned int* bad, bool msg_flags, uint8_t recs,
                                                                  void* __restrict__ out, uint8_t compact, bool props, bool cq, bool pv, bool lt, bool ri) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool is_bad = false;
  if (i < n) {
    const RecClass c = classify(msgs[i], n_groups, n_peers, msg_flags, recs, props, cq, pv, lt, ri);
    is_bad = c == kBad;
    // a skipped record sorts behind every group (the key range has room for n_groups itself) and is answered here
    keys[i] = c == kTake ? msgs[i].group : c == kSkip ? n_groups : 0;  // (bad: keep the sort's key range valid)
    order[i] = (uint32_t)i;
    if (c == kSkip) put_skipped(out, i, compact);
  }
  if (__ballot(is_bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}

// ---- (3) one group's state in registers ------------------------------------------------------
constexpr uint32_t kMaxRun = 32;
constexpr uint32_t kNil = 0xffffffffu;

// MASKED (raftq_step_set_voters on a handle with voter masks loaded): quorum(), maybe_commit() and poll() run over the group's
// own voters -- include/raftq.h "per-group voter sets", the sweep's rules (sweep_voters_kernel) restated for Step.  The mask is
// ONE register, read from the dense `voters` array (authoritative; NodeRec has no room for nine bits and a copy would be one
// more thing to keep fresh) beside the record's loads: its address depends on g alone, so it adds a 32-byte sector per touched
// group and no dependent latency.  Everything else -- what is stored, reset()'s N slots, whose words are recorded -- is the
// unmasked form's: a non-voter's Match and vote are kept as always and merely do not count.
// `Node` stays the name of the unmasked form (elect_build_kernel, propose_build_kernel / propose_commit_kernel, the respond path).
// LEAD (raftq_respond_set_lead, raftq_step_frames_respond only): respond() answers RAFTQ_OUT_BECAME_LEADER too -- becomeLeader's
// broadcast, one MsgApp with the empty entry to every peer.  The frame's LogTerm is the lastTerm become_leader() overwrites, so
// that form keeps it (last_term_was).  Every `if constexpr (LEAD)` is empty in the other forms: they compile to what they were.
// The LEAD form is "the form that answers broadcasts with entries": under raftq_respond_set_props it also answers a
// RAFTQ_OUT_PROPOSED at the tail with the leader's bcastAppend -- the frame's Index / LogTerm are the tail appendEntry moved, so
// the MsgProp arm keeps that lastTerm in last_term_was too.  Which of the two it answers is NodeArrays::ans_lead / ans_props (run
// time: a third template axis would be four more walks).
// CQ (raftq_set_check_quorum): checkQuorum's four rules -- activity bits, reset(), the lease, RAFTQ_MSG_CHECK_QUORUM (include/raftq_step.h
// "CheckQuorum").  A template axis, not a run-time flag of NodeArrays: as a flag the rules cost every handle registers -- the sorted
// walk went from 158 to 169 VGPRs and from 3 waves per SIMD to 2, the list walk from 190 to 199, with the switch off
// (profiles/r24/README.md) -- and every `if constexpr (CQ)` is empty in the other forms: they compile to what they were.
// ---- raftq_set_read_index(h, RAFTQ_READ_SAFE): the rules that touch a group's read record, OUT OF LINE and on the record where it
// lies.  NodeT::step is inlined twice into the list walk; with the record held in NodeT (ten more registers, read lazily and written
// back when dirty, as the activity word is) and its rules inline, the inliner left maybe_commit(), respond() and become_follower()
// of those forms out of line instead, and a NodeT whose address is taken lives in scratch -- 400 to 528 bytes a lane
// (profiles/r30/README.md).  One call that takes what it needs by value costs the walks no register that lives across the role arms
// and no scratch; the record is in memory either way: a lane owns its group, so it reads what it wrote.  A batch with no read
// traffic and no reset() never gets here; a request stores two words, an acknowledgement that raises a word one, a reset() one
// zeroed record (NodeT::rd_zeroed spares the second of two in a row).
//   op kReadRequest   p = self: seq += 1, acked[p] = seq -> seq | (confirmed() >= seq) << 32; 0 = the counter is full, nothing moved
//      kReadAck       c = the context, p = its sender: acked[p] = max(acked[p], c) unless c > seq -> confirmed() if it moved, else 0
//      kReadBeat      -> seq if seq > confirmed(), else 0
//      kReadClear     the record zeroed
// confirmed(): the largest number >= q of the slots in `members` have acknowledged -- maybe_commit()'s counting form over the
// acknowledgement words; an empty `members` gives 0, a slot outside it is stored and does not count.
constexpr uint32_t kReadRequest = 0, kReadAck = 1, kReadBeat = 2, kReadClear = 3;
__device__ __forceinline__ uint32_t read_confirmed(const uint32_t (&ack)[kMaxPeers], uint32_t members, uint32_t q) {
  uint32_t best = 0;
#pragma unroll
  for (uint32_t c = 0; c < (uint32_t)kMaxPeers; ++c) {
    uint32_t ge = 0;
#pragma unroll
    for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) ge += (((members >> p) & 1u) != 0 && ack[p] >= ack[c]) ? 1u : 0u;
    if (((members >> c) & 1u) != 0 && ge >= q && ack[c] > best) best = ack[c];
  }
  return best;
}
static __device__ __noinline__ uint64_t read_rule(ReadRec* rec, uint32_t op, uint32_t p, uint32_t c, uint32_t members, uint32_t q) {
  if (op == kReadClear) {
    uint4* w = reinterpret_cast<uint4*>(rec);
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = uint4{0, 0, 0, 0};
    return 0;
  }
  uint32_t seq = rec->seq;
  uint32_t ack[kMaxPeers];
#pragma unroll
  for (int k = 0; k < kMaxPeers; ++k) ack[k] = rec->acked[k];
  if (op == kReadBeat) return seq > read_confirmed(ack, members, q) ? seq : 0;
  if (op == kReadRequest) {
    if (seq == 0xffffffffu) return 0;
    c = seq += 1;
    rec->seq = seq;
  } else if (c > seq) {
    return 0;
  }
  const uint32_t before = read_confirmed(ack, members, q);
  bool raised = false;
#pragma unroll
  for (uint32_t k = 0; k < (uint32_t)kMaxPeers; ++k)
    if (k == p && ack[k] < c) {
      ack[k] = c;
      raised = true;
    }
  if (raised) rec->acked[p] = c;
  const uint32_t after = read_confirmed(ack, members, q);
  if (op == kReadRequest) return (uint64_t)seq | ((uint64_t)(after >= seq ? 1u : 0u) << 32);
  return after > before ? after : 0;
}

// RI (raftq_set_read_index): the CQ form as the *_cq_* walks instantiate it, with the rules of include/raftq_step.h "ReadIndex in Step"
// behind the run-time NodeArrays::ri.  An axis of its own so that the one other user of the CQ form -- elect_build_cq_kernel, which
// has no read records to hand over -- compiles to what it was: every use of ri() folds to 0 there.
template <bool MASKED, bool LEAD = false, bool CQ = false, bool RI = false>
struct NodeT {
  static_assert(CQ || !RI, "the read rules live in the CQ form");
  const NodeArrays& a;
  uint64_t g;
  uint64_t term, last_index, last_term, committed, first_idx;
  uint64_t mt[kMaxPeers];  // Progress.Match of every peer, from the record
  uint32_t mt_dirty = 0;   // bit p: mt[p] differs from the dense match[p][g]
  uint32_t vote, lead;
  uint32_t vw = 0;  // the group's vote word (raft.votes as 2 bits per peer)
  uint32_t lst_head, lst_cnt, lst_min;  // the record's list words as loaded (the walk empties them when it stores)
  uint8_t role;
  bool held = false;  // this batch only: a MsgApp with RAFTQ_MSGF_BARRIER was left to the caller -- the group's later messages wait
  // raftq_step_frames_respond: the caller's at-tail bit as it still holds at this point of the batch, and whether an earlier
  // result of the group was left to the host (which ends the group's device-answered prefix)
  bool at_tail = false, host_owns = false;
  // what has to be written to the dense arrays besides the record (which always is, list words emptied)
  uint64_t committed0, first_idx0;
  uint8_t role0;
  bool vw_known = false, vw_dirty = false, elapsed_reset = false;
  uint32_t vmask = 0;  // MASKED only: voters[g], bit p = slot p votes in this group
  uint64_t last_term_was = 0;  // LEAD only: lastTerm as it stood before the latest become_leader() / the latest proposal's appendEntry
  // raftq_set_check_quorum only: the group's activity word (NodeArrays::cq), read lazily and written back when dirty, as the vote word
  uint32_t cqw = 0;
  bool cq_known = false, cq_dirty = false;
  // raftq_set_read_index(h, RAFTQ_READ_SAFE) only: the handle's read records (read_rule() below works on group g's in memory), and
  // whether this lane has zeroed the group's and nothing has touched it since (reset() may run twice for one message)
  ReadRec* reads = nullptr;
  bool rd_zeroed = false;

  __device__ NodeT(const NodeArrays& arr, uint64_t group, const uint16_t* voters = nullptr, ReadRec* read_recs = nullptr) : a(arr), g(group) {
    if constexpr (RI) reads = read_recs;
    if constexpr (MASKED) vmask = voters[g];
    const NodeRec r = a.rec[g];  // one line: eight 16-byte loads
    term = r.term; last_index = r.last_index; last_term = r.last_term;
    vote = r.vote; lead = r.lead;
    lst_head = r.lst_head; lst_cnt = r.lst_cnt; lst_min = r.lst_min;
    committed = committed0 = r.committed;
    first_idx = first_idx0 = r.first_idx;
    role = role0 = r.role;
#pragma unroll
    for (int p = 0; p < kMaxPeers; ++p) mt[p] = r.match[p];
    if (a.at_tail != nullptr) at_tail = ((a.at_tail[g >> 6] >> (g & 63)) & 1ull) != 0;
  }
  // list_reset: the walk hands the group's list back empty (log_deltas_kernel leaves the words as they are)
  __device__ void store(bool list_reset = true) const {
    NodeRec r;
    r.term = term; r.last_index = last_index; r.last_term = last_term;
    r.vote = (uint8_t)vote; r.lead = (uint8_t)lead;
    r.role = role; r.pad = 0;
    r.lst_head = list_reset ? kNil : lst_head;
    r.lst_cnt = list_reset ? 0u : lst_cnt;
    r.lst_min = list_reset ? kNil : lst_min;
    r.committed = committed;
    r.first_idx = first_idx;
#pragma unroll
    for (int p = 0; p < kMaxPeers; ++p) r.match[p] = mt[p];
    a.rec[g] = r;
    // ... and what changed, where the dense kernels read it
    if (committed != committed0) a.committed[g] = committed;
    if (role != role0) a.role[g] = role;
    if (first_idx != first_idx0) a.first_idx[g] = first_idx;
#pragma unroll
    for (int p = 0; p < kMaxPeers; ++p)
      if ((mt_dirty >> p) & 1u) a.match[(uint64_t)p * a.ld + g] = mt[p];
    // the group's rows as they now stand are all in mt[]: a peer above the word's slot breaks the self-max fact
    if (mt_dirty != 0 && a.self_max != nullptr) {
      const uint32_t w = *a.self_max;
      if ((w & kSelfMaxValid) != 0) {
        const uint64_t own = match(w & 0xffu);
        bool broken = false;
#pragma unroll
        for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) broken |= p < a.n_peers && mt[p] > own;
        if (broken) *a.self_max = 0u;
      }
    }
    // ... and Step does not keep the narrow mirror (the word behind the self-max word): a stored row ends it
    if (mt_dirty != 0 && a.self_max != nullptr && a.self_max[1] != 0u) a.self_max[1] = 0u;
    if (elapsed_reset) a.elapsed[g] = 0;
    if (vw_dirty) {
      if (a.n_peers <= 8) reinterpret_cast<uint16_t*>(a.votes)[g] = (uint16_t)vw;
      else reinterpret_cast<uint32_t*>(a.votes)[g] = vw;
      // ... nor the tally mirror (the word behind the narrow word): a stored vote word ends it
      if (a.self_max != nullptr && a.self_max[2] != 0u) a.self_max[2] = 0u;
    }
    if constexpr (CQ)
      if (cq_dirty) a.cq[g] = cqw;
  }
  __device__ void set_cq(uint32_t w) {
    cqw = w;
    cq_known = cq_dirty = true;
  }
  __device__ uint32_t get_cq() {
    if (!cq_known) {
      cqw = a.cq[g];
      cq_known = true;
    }
    return cqw;
  }
  // checkQuorum's lease (include/raftq_step.h): a leader always, a follower that has heard from its leader within election_tick
  // ticks.  elapsed[g] is the Tick's dense word, read here alone; a reset of this batch that store() has yet to write counts as 0
  __device__ bool in_lease() const {
    return role == kLeader || (lead != 0 && (elapsed_reset ? 0u : a.elapsed[g]) < a.election_tick);
  }
  __device__ void set_first_idx(uint64_t v) { first_idx = v; }
  __device__ uint64_t get_first_idx() const { return first_idx; }
  __device__ void set_votes(uint32_t w) {
    vw = w;
    vw_known = vw_dirty = true;
  }
  __device__ uint32_t get_votes() {
    if (!vw_known) {
      vw = a.n_peers <= 8 ? (uint32_t)reinterpret_cast<const uint16_t*>(a.votes)[g] : reinterpret_cast<const uint32_t*>(a.votes)[g];
      vw_known = true;
    }
    return vw;
  }
  // Progress.Match of peer p (a run-time index into registers: selects, not scratch)
  __device__ uint64_t match(uint32_t p) const {
    uint64_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxPeers; ++k) v = k == p ? mt[k] : v;
    return v;
  }
  __device__ void set_match(uint32_t p, uint64_t v) {
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxPeers; ++k) mt[k] = k == p ? v : mt[k];
    mt_dirty |= 1u << p;
  }
  __device__ __forceinline__ uint8_t ri() const {
    if constexpr (RI) return a.ri;
    else return 0;
  }
  // the slots confirmed() counts, and read_rule() on this group's record
  __device__ __forceinline__ uint32_t read_members() const {
    if constexpr (MASKED) return vmask;
    else return (1u << a.n_peers) - 1u;
  }
  __device__ __forceinline__ uint64_t read_op(uint32_t op, uint32_t p = 0, uint32_t c = 0) {
    rd_zeroed = op == kReadClear;
    return read_rule(reads + g, op, p, c, read_members(), quorum());
  }
  // CHOICE where upstream has no counterpart (its prs map IS the membership): q_g = popcount(voters[g]) / 2 + 1; an empty mask
  // gives 1, which nothing reaches (no candidate, no counted grant)
  __device__ uint32_t quorum() const {
    if constexpr (MASKED) return ((uint32_t)__popc(vmask) >> 1) + 1u;
    else return a.n_peers / 2 + 1;
  }
  // slot p counts: it is a peer and, in the masked form, a voter of this group (a mask names no slot >= N: raftq_load_voters)
  __device__ bool counts(uint32_t p, uint32_t n) const {
    if constexpr (MASKED) return ((vmask >> p) & 1u) != 0;
    else return p < n;
  }

  // raft.reset(term)
  __device__ void reset(uint64_t t) {
    if (term != t) { term = t; vote = 0; }
    lead = 0;
    elapsed_reset = true;
    set_votes(0);
    if constexpr (CQ) {
      set_cq(0);  // every Progress.RecentActive = false, electionElapsed = 0
      if (ri() == kReadSafe && !rd_zeroed) (void)read_op(kReadClear);  // readOnly = newReadOnly: no request of the old leadership is ever confirmed
    }
#pragma unroll
    for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p)
      if (p < a.n_peers) {
        const uint64_t v = p == a.self ? last_index : 0;
        if (mt[p] != v) mt_dirty |= 1u << p;
        mt[p] = v;
      }
  }
  __device__ void become_follower(uint64_t t, uint32_t new_lead) {
    reset(t);
    lead = new_lead;
    role = kFollower;
    set_first_idx(0);
  }
  __device__ void become_candidate() {
    reset(term + 1);
    vote = a.self + 1;
    role = kCandidate;
    set_first_idx(0);
  }
  // raft.maybeCommit + raftLog.maybeCommit: the largest index held by >= q peers (counting form),
  // then the compact current-term gate.  MASKED: by >= q_g VOTERS -- a non-voter neither counts nor is a candidate, so an
  // empty mask commits nothing and a one-voter group whose voter is the leader commits on its own append
  __device__ bool maybe_commit() {
    uint64_t m[kMaxPeers];
    const uint32_t n = a.n_peers, q = quorum();
#pragma unroll
    for (uint32_t p = 0; p < kMaxPeers; ++p) m[p] = counts(p, n) ? mt[p] : 0;
    uint64_t mci = 0;
#pragma unroll
    for (uint32_t c = 0; c < kMaxPeers; ++c) {
      uint32_t ge = 0;
#pragma unroll
      for (uint32_t p = 0; p < kMaxPeers; ++p) ge += (counts(p, n) && m[p] >= m[c]) ? 1u : 0u;
      if (counts(c, n) && ge >= q && m[c] > mci) mci = m[c];
    }
    if (mci > committed) {  // (the gate's word is only read when there is something to gate)
      const uint64_t fi = get_first_idx();
      if (fi != 0 && mci >= fi) {
        committed = mci;
        return true;
      }
    }
    return false;
  }
  // raft.becomeLeader incl. appendEntry(empty entry of the new term)
  __device__ void become_leader() {
    if constexpr (LEAD) last_term_was = last_term;
    reset(term);
    lead = a.self + 1;
    role = kLeader;
    last_index += 1;
    last_term = term;
    set_first_idx(last_index);
    set_match(a.self, last_index);
    (void)maybe_commit();
  }
  // raft.poll: the first response of a peer wins; returns {granted, recorded}.  MASKED: every sender's first response is
  // recorded as always; the two counts are over the voters' fields only (poll_word_voters' form)
  __device__ void poll(uint32_t from, bool granted, uint32_t& n_granted, uint32_t& n_recorded) {
    uint32_t w = get_votes();
    const uint32_t cur = (w >> (2 * from)) & 3u;
    if (cur != 1 && cur != 2) {
      w = (w & ~(3u << (2 * from))) | ((granted ? 1u : 2u) << (2 * from));
      set_votes(w);
    }
    uint32_t low;
    if constexpr (MASKED) low = spread_even(vmask);
    else low = 0x55555555u & ((1u << (2 * a.n_peers)) - 1u);
    const uint32_t g1 = w & ~(w >> 1) & low, r1 = (w >> 1) & ~w & low;
    n_granted = __popc(g1);
    n_recorded = __popc(g1 | r1);
  }
  __device__ void commit_to(uint64_t tocommit) {
    if (tocommit > last_index) tocommit = last_index;
    if (committed < tocommit) committed = tocommit;
  }

  // handleAppendEntries once the header is accepted.  A message that says what it carries (RAFTQ_MSGF_ENTRIES) and
  // appends at the log's tail needs nothing from the entries but their count and the last one's term:
  // raftLog.maybeAppend = matchTerm(tail) -> no conflict possible -> append -> commitTo(min(m.Commit, lastnewi)).
  __device__ void handle_append(const MsgRec& m, StepOutRec& o) {
    o.type = kOutAppend;
    if (a.msg_flags && (m.pad[1] & kMsgfEntries) && m.index == last_index && m.log_term == last_term) {
      const uint64_t k = entry_count(m, a.recs);
      if (k) {
        last_index = m.index + k;
        last_term = m.reject_hint;
      }
      commit_to(m.commit);  // clamps to last_index = lastnewi
      o.type = kOutAppended;
      o.index = last_index;
    }
  }

  // raftq_step_frames_respond: after step(m, o) for batch position i -- what the host's apply_result would send for this result
  // (raftq_node.cpp), when it is a message of the table in include/raftq_wire.h, as resp[i]; o gets RAFTQ_OUTF_ANSWERED.
  // The at-tail bit goes with every message that makes the host move some Next away from the tail (a rejection it backs off
  // for, a heartbeat response below lastIndex, a step-down); a result the host may answer itself ends the group's prefix.
  __device__ void respond(const MsgRec& m, StepOutRec& o, uint64_t i) {
    if (a.resp == nullptr) return;
    if (role != kLeader) at_tail = false;
    RespRec r;
    r.group = g; r.term = o.term; r.index = 0; r.log_term = 0; r.commit = 0;
    r.stamp = a.resp_stamp; r.kind = 0; r.reject = 0; r.to = (uint8_t)m.from; r.pad = 0;
    if (o.type == kOutProgress) {
      if (m.type == kMsgAppResp && m.reject) {
        if (m.index > o.index) at_tail = false;  // Progress.maybeDecrTo: the host backs Next off and resends
      } else if (m.type == kMsgHeartbeatResp) {
        if (o.index < last_index) at_tail = false;  // `if pr.Match < lastIndex { sendAppend }`
      }
    }
    // a forwarded proposal the leader took: until the host's bcastAppend no follower is at the new tail (a device-built commit
    // broadcast behind it would carry an index the followers do not have).  It and RAFTQ_OUT_FORWARD are the host's (default below).
    // LEAD under raftq_respond_set_props: inside the prefix and at the tail the proposal's bcastAppend is built below, which leaves
    // the followers (optimistically, as bcastAppend does) at the new tail -- the bit stays.
    if constexpr (LEAD) {
      // (the decoder's record: resv = ent_first | n_ents << 32; headers beyond ents_cap were not handed back)
      const bool prop_here = o.type == kOutProposed && a.ans_props && at_tail && !host_owns && (m.resv & 0xffffffffull) + (m.resv >> 32) <= a.resp_ent_base;
      if (o.type == kOutProposed && !prop_here) at_tail = false;
    } else {
      if (o.type == kOutProposed) at_tail = false;
    }
    if (!host_owns) {
      switch (o.type) {
        case kOutAppended: r.kind = kMsgAppResp; r.index = o.index; break;
        case kOutVoteResp: r.kind = kMsgVoteResp; r.reject = o.reject; break;
        case kOutHeartbeatResp:
          r.kind = kMsgHeartbeatResp;
          if constexpr (RI) r.index = o.index;  // raftq_set_read_index: the heartbeat's context, echoed (0 without the switch)
          break;
        case kOutProgress:
          if (m.type == kMsgAppResp && !m.reject) {
            if (!at_tail) host_owns = true;  // the host knows Next: it may send
            else if (o.flags & kFlagCommitted) {  // bcastAppend with every follower at the tail: N - 1 empty MsgApps
              r.kind = kMsgApp; r.index = last_index; r.log_term = last_term; r.commit = committed;
            }
          } else if (m.type == kMsgAppResp ? m.index > o.index : o.index < last_index) {
            host_owns = true;  // a resend
          }
          break;
        case kOutNone: case kOutSkipped: break;
        default:
          if constexpr (LEAD) {
            // becomeLeader's bcastAppend: reset() has put every Next at the empty entry's index, so every peer gets
            // MsgApp{Index: lastIndex - 1, LogTerm: the old lastTerm, Entries: [the empty entry]} (pad = 1: the layout writes the
            // entry header) -- which leaves every follower at the tail, whatever the caller's bitmap said
            if (o.type == kOutBecameLeader && a.ans_lead) {
              r.kind = kMsgApp; r.index = o.index - 1; r.log_term = last_term_was; r.commit = committed; r.pad = 1;
              at_tail = true;
              break;
            }
            // a forwarded proposal's bcastAppend with every Next at the old tail + 1: MsgApp{Index / LogTerm: the tail before
            // appendEntry (o.index is the first new index), Commit after, Entries: the message's own} (pad = 2: the layout stamps them)
            // (the bit is still set behind a proposal only where the test above found everything it asks for)
            if (o.type == kOutProposed && at_tail) {
              r.kind = kMsgApp; r.index = o.index - 1; r.log_term = last_term_was; r.commit = committed; r.pad = 2;
              break;
            }
          }
          host_owns = true;  // MsgApp left to the log's owner, a new leader's broadcast, held / deferred messages, a proposal taken or forwarded
      }
    }
    if (r.kind != 0) o.flags |= kFlagAnswered;
    a.resp[i] = r;
  }

  __device__ void step(const MsgRec& m, StepOutRec& o) {
    const uint64_t term0 = term, commit0 = committed;
    const uint32_t vote0 = vote;
    const uint8_t role0 = role;
    o.index = 0; o.log_term = 0; o.type = kOutNone; o.reject = 0; o.flags = 0;
    const bool hold = a.msg_flags && (m.pad[1] & kMsgfHold) != 0;  // RAFTQ_OUT_HELD: the caller's, where it stands; the rest waits
    if (held || hold) {  // RAFTQ_OUT_DEFERRED: nothing of this message is applied
      o.type = hold ? kOutHeld : kOutDeferred;
      held = true;
      o.group = g; o.term = term; o.commit = committed; o.last_index = last_index;
      o.to = m.from; o.vote = vote; o.lead = lead; o.role = role;
      return;
    }
    const uint32_t q = quorum();
    bool handled = false;
    bool campaigns = false, won = false;  // CQ form only: campaign() / becomeLeader are due (one copy of each, behind the role arms)
    bool transfer = false;                // ... and the campaign is a transfer's (MsgTimeoutNow): its MsgVotes go out marked
    if (m.type == kMsgHup) {
      handled = true;
      if (role != kLeader) {  // campaign()
        if constexpr (CQ) {
          // PreVote: becomePreCandidate -- no term, vote, Match, gate or activity word moves; the pre-election's grants use the vote
          // word.  An own grant that is the quorum already goes straight on to the campaign, which starts from reset() as always.
          // (The CQ form runs campaign() in ONE place, behind the role arms, for MsgHup and for a won pre-election.)
          campaigns = true;
          if (a.pv) {
            role = kPreCandidate;
            lead = 0;
            elapsed_reset = true;  // CHOICE: zeroed as Step's MsgHup always has
            set_votes(0);
            uint32_t gr, rec;
            poll(a.self, true, gr, rec);
            if (gr != q) {
              campaigns = false;
              o.type = kOutPreCampaign; o.index = last_index; o.log_term = last_term;
            }
          }
        } else {
          become_candidate();
          uint32_t gr, rec;
          poll(a.self, true, gr, rec);
          if (gr == q) { become_leader(); o.type = kOutBecameLeader; }
          else o.type = kOutCampaign;
          o.index = last_index;
          o.log_term = last_term;
        }
      }
    } else if (m.term != 0) {
      if (m.term > term) {
        // checkQuorum: a MsgVote inside the lease is ignored -- no term change, no answer (a partitioned node coming back)
        // PreVote: a MsgPreVote inside the lease likewise; outside it, and a granting MsgPreVoteResp, change no term and no role; a
        // rejecting MsgPreVoteResp makes a follower without a leader (CHOICE: its sender is no leader)
        if constexpr (CQ) {
          // Leadership transfer: a MsgVote marked as a transfer's (reject = 1) passes the lease
          const bool leased = ((m.type == kMsgVote && !(a.lt && m.reject)) || (a.pv && m.type == kMsgPreVote)) && in_lease();
          const bool keep = a.pv && (m.type == kMsgPreVote || (m.type == kMsgPreVoteResp && !m.reject));
          if (leased) handled = true;
          // ReadIndex: neither read kind is a leader's -- a MsgReadIndex's `from` is the requester, who leads nothing
          else if (!keep)
            become_follower(m.term, (m.type == kMsgVote || (a.pv && m.type == kMsgPreVoteResp) || (ri() != 0 && (m.type == kMsgReadIndex || m.type == kMsgReadIndexResp))) ? 0u : m.from + 1);
        } else {
          become_follower(m.term, m.type == kMsgVote ? 0u : m.from + 1);
        }
      } else if (m.term < term) {
        handled = true;  // stale: ignored
        // PreVote: ... but for a MsgPreVote, which is rejected with the own term, and a stale leader's MsgApp / MsgHeartbeat, which
        // is told the term it missed (nothing changes, no clock is reset, a barrier on it holds nobody up)
        if constexpr (CQ) {
          if (a.pv) {
            if (m.type == kMsgPreVote) { o.type = kOutPreVoteResp; o.reject = 1; o.index = term; }
            else if (m.type == kMsgApp || m.type == kMsgHeartbeat) o.type = kOutTermResp;
          }
        }
      }
    }
    // PreVote: a MsgPreVote that got this far is answered by one rule in every role, and changes nothing
    if constexpr (CQ) {
      if (!handled && a.pv && m.type == kMsgPreVote) {
        handled = true;
        const bool up_to_date = m.log_term > last_term || (m.log_term == last_term && m.index >= last_index);
        o.type = kOutPreVoteResp;
        if ((vote == 0 || m.term > term || vote == m.from + 1) && up_to_date) o.index = m.term;
        else { o.reject = 1; o.index = term; }
      }
    }
    if (!handled) {
      if (role == kLeader) {
        // Progress[from].RecentActive = true, in front of the reject branch; a non-voter's bit is stored and does not count
        if constexpr (CQ) {
          if (m.type == kMsgAppResp || m.type == kMsgHeartbeatResp) {
            const uint32_t w = get_cq();
            if (((w >> m.from) & 1u) == 0) set_cq(w | (1u << m.from));
          }
        }
        if (m.type == kMsgBeat) {
          o.type = kOutBcastHeartbeat;
          // ReadIndex: the round carries the last pending request's sequence number (upstream's lastPendingRequestCtx) -- the
          // resend of a round that was lost
          if constexpr (CQ) {
            if (ri() == kReadSafe) {
              o.index = read_op(kReadBeat);
            }
          }
        } else if (CQ && ri() != 0 && m.type == kMsgReadIndex) {
          // stepLeader MsgReadIndex: dropped until the leader has committed an entry of its term (the gate's own words), else the
          // read is good at `committed` once a quorum still takes this node for the leader -- the lease says so at once, the safe
          // mode numbers the request and waits for a heartbeat round that carries the number
          const uint64_t fi = get_first_idx();
          if (fi != 0 && committed >= fi) {
            if (ri() == kReadLease) {
              o.type = kOutReadIndex; o.index = committed; o.flags |= kFlagReadReady;
            } else {
              const uint64_t took = read_op(kReadRequest, a.self);
              if (took != 0) {
                o.type = kOutReadIndex; o.index = committed; o.log_term = took & 0xffffffffull;
                if (took >> 32) o.flags |= kFlagReadReady;
              }
            }
          }
        } else if (CQ && m.type == kMsgCheckQuorum) {
          // (classify() lets the kind through only under raftq_set_check_quorum)  The members that answered since the last check,
          // self included, against quorum(); the bits are cleared either way, and a leader without its quorum steps down
          const uint32_t w = get_cq();
          uint32_t members;
          if constexpr (MASKED) members = vmask;
          else members = (1u << a.n_peers) - 1u;
          const uint32_t act = (uint32_t)__popc(((w & kCqLowMask) | (1u << a.self)) & members);
          set_cq(w & ~kCqLowMask);
          if (act < q) become_follower(term, 0);
        } else if (CQ && a.lt && m.type == kMsgTransferLeader) {
          // stepLeader MsgTransferLeader: t = from.  A transfer to t already pending, or t no voter: ignored.  One to another slot is
          // aborted first, and t == self stops there (which is how a pending transfer is cancelled); else leadTransferee = t + 1 and
          // electionElapsed = 0, and the transferee gets MsgTimeoutNow if it is at the tail, sendAppend(t) -- the caller's -- if not
          const uint32_t t = m.from, w = get_cq();
          if (counts(t, a.n_peers) && (w & kCqTransfereeMask) >> kCqTransfereeShift != t + 1) {
            uint32_t nw = w & ~kCqTransfereeMask;
            if (t != a.self) {
              nw = (nw & kCqLowMask) | ((t + 1) << kCqTransfereeShift);
              o.type = kOutTransfer;
              o.index = match(t);
              if (o.index == last_index) o.flags |= kFlagTimeoutNow;
            }
            if (nw != w) set_cq(nw);
          }
        } else if (CQ && a.lt && m.type == kMsgProp && (get_cq() & kCqTransfereeMask) != 0) {
          // a transfer is pending: the proposal is dropped (ErrProposalDropped) -- RAFTQ_OUT_NONE, nothing moves
        } else if (m.type == kMsgVote) {
          o.type = kOutVoteResp; o.reject = 1;
        } else if (m.type == kMsgAppResp || m.type == kMsgProp) {
          // the two messages that move a Match: an acknowledgement the sender's, a forwarded proposal (stepLeader MsgProp:
          // appendEntry(m.Entries...) -- every entry stamped r.Term and the next index, whatever it carried -- then
          // prs[self].maybeUpdate(lastIndex)) the leader's own.  ONE maybeCommit behind both (classify() let a MsgProp through only
          // under raftq_step_set_props, with a count of at least one; the caller keeps last_index + n below 2^64).
          const bool prop = m.type == kMsgProp;
          uint32_t who = m.from;
          uint64_t idx = m.index > last_index ? last_index : m.index;
          bool moved = false;
          if (prop) {
            o.type = kOutProposed; o.index = last_index + 1; o.log_term = term;
            if constexpr (LEAD) last_term_was = last_term;
            last_index += entry_count(m, a.recs);
            last_term = term;
            who = a.self; idx = last_index;
            moved = true;
          } else {
            o.type = kOutProgress; o.reject = m.reject;
            if (!m.reject && match(who) < idx) {
              o.flags |= kFlagUpdated;
              moved = true;
            }
          }
          if (moved) {
            set_match(who, idx);
            (void)maybe_commit();
          }
          if (!prop) o.index = match(who);
          // Leadership transfer: the pending transferee's ack that updated its Match to the tail -- send it MsgTimeoutNow
          if constexpr (CQ) {
            if (a.lt && (o.flags & kFlagUpdated) != 0 && (get_cq() & kCqTransfereeMask) >> kCqTransfereeShift == who + 1 && o.index == last_index)
              o.flags |= kFlagTimeoutNow;
          }
        } else if (m.type == kMsgHeartbeatResp) {
          o.type = kOutProgress;
          o.index = match(m.from);
          // ReadIndex: the response echoes the round's context c; it counts for every request <= c.  0, or a number this leadership
          // has not handed out, is no context
          if constexpr (CQ) {
            if (ri() == kReadSafe && m.index != 0 && m.index <= 0xffffffffull) {  // (seq is 32 bits wide: a larger c is beyond it)
              const uint64_t after = read_op(kReadAck, m.from, (uint32_t)m.index);
              if (after != 0) {
                o.flags |= kFlagReadReady;
                o.log_term = after;
              }
            }
          }
        }
      } else if (role == kCandidate || (CQ && a.pv && role == kPreCandidate)) {
        if (m.type == kMsgApp) {
          become_follower(term, m.from + 1);
          handle_append(m, o);
        } else if (m.type == kMsgHeartbeat) {
          become_follower(term, m.from + 1);
          commit_to(m.commit);
          o.type = kOutHeartbeatResp;
          if constexpr (CQ)
            if (ri() != 0) o.index = m.index;  // ReadIndex: the round's context, echoed
        } else if (m.type == kMsgVote) {
          o.type = kOutVoteResp; o.reject = 1;
        } else if (m.type == kMsgVoteResp || (CQ && m.type == kMsgPreVoteResp)) {
          uint32_t gr, rec;
          // upstream's equality (`switch r.q()`), MASKED too: a mask that shrinks in the middle of an election can step over the
          // equal count -- upstream's behaviour, and the election timer's to repair
          if constexpr (CQ) {
            // PreVote: a pre-candidate polls MsgPreVoteResp and ignores MsgVoteResp, a candidate the other way round.  A won
            // pre-election is the campaign MsgHup runs without the switch (behind the role arms); a lost one is a lost election's
            // becomeFollower(term, None) -- Term and Vote are kept
            if ((m.type == kMsgPreVoteResp) == (role == kPreCandidate)) {
              poll(m.from, !m.reject, gr, rec);
              if (gr == q) {
                if (role == kPreCandidate) campaigns = true;
                else won = true;
              } else if (rec - gr == q) {
                become_follower(term, 0);
              }
            }
          } else {
            poll(m.from, !m.reject, gr, rec);
            if (gr == q) {
              become_leader();
              o.type = kOutBecameLeader; o.index = last_index; o.log_term = last_term;
            } else if (rec - gr == q) {
              become_follower(term, 0);
            }
          }
        }
      } else {
        if (m.type == kMsgApp) {
          elapsed_reset = true; lead = m.from + 1;
          handle_append(m, o);
        } else if (m.type == kMsgHeartbeat) {
          elapsed_reset = true; lead = m.from + 1;
          commit_to(m.commit);
          o.type = kOutHeartbeatResp;
          if constexpr (CQ)
            if (ri() != 0) o.index = m.index;  // ReadIndex: the round's context, echoed (either mode: the leader's may be the safe one)
        } else if (m.type == kMsgVote) {
          o.type = kOutVoteResp;
          const bool up_to_date = m.log_term > last_term || (m.log_term == last_term && m.index >= last_index);
          if ((vote == 0 || vote == m.from + 1) && up_to_date) { elapsed_reset = true; vote = m.from + 1; }
          else o.reject = 1;
        } else if ((m.type == kMsgProp || (CQ && a.lt && m.type == kMsgTransferLeader) || (CQ && ri() != 0 && m.type == kMsgReadIndex)) && lead != 0) {
          o.type = kOutForward;  // stepFollower MsgProp / MsgTransferLeader / MsgReadIndex: `m.To = r.lead; r.send(m)` -- the one result addressed to somebody else
        } else if (CQ && ri() != 0 && m.type == kMsgReadIndexResp) {
          o.type = kOutReadState;  // stepFollower MsgReadIndexResp: the leader's answer to a read this node forwarded -- readStates gets {Index}
          o.index = m.index;
        } else if (CQ && a.lt && m.type == kMsgTimeoutNow) {
          // stepFollower MsgTimeoutNow: campaign(campaignTransfer) at once if promotable() -- the real campaign under PreVote too
          campaigns = transfer = counts(a.self, a.n_peers);
        }
      }
    }
    if constexpr (CQ) {
      if (campaigns) {  // raft.campaign: becomeCandidate and the own grant, which may be the quorum
        become_candidate();
        uint32_t gr, rec;
        poll(a.self, true, gr, rec);
        won = gr == q;
        o.type = kOutCampaign;
        o.reject = transfer ? 1 : 0;
      }
      if (won) {
        become_leader();
        o.type = kOutBecameLeader;
        o.reject = 0;
      }
      if (campaigns || won) { o.index = last_index; o.log_term = last_term; }
    }
    if (a.msg_flags && o.type == kOutAppend && m.type == kMsgApp && (m.pad[1] & kMsgfBarrier)) held = true;
    o.group = g; o.term = term; o.commit = committed; o.last_index = last_index;
    o.to = o.type == kOutForward ? lead - 1 : m.from; o.vote = vote; o.lead = lead; o.role = role;
    if (term != term0 || vote != vote0 || committed != commit0) o.flags |= kFlagHardState;
    if (committed != commit0) o.flags |= kFlagCommitted;
    if (role0 != kFollower && role == kFollower) o.flags |= kFlagSteppedDown;
  }
};
using Node = NodeT<false>;

// ---- (2b, 3b) the same walk WITHOUT the sort.  Inbound traffic rarely brings more than a few messages
// of one group in one batch, so grouping by a full stable sort (4-12 launches, 40-60 us of a 95 us kernel
// chain at 64K messages) is the wrong tool.  step_link_kernel threads every message onto its group's list
// with three atomics on group-indexed arrays (exchange the list head, count, minimum batch position);
// the lane of a group's FIRST message then owns the group: it gathers the list (arbitrary order), sorts
// the <= kMaxRun positions in a private array, applies the messages in arrival order and empties the list -- the same
// sequence the sorted walk applies, so the result records are identical byte for byte
// (tests/test_step_gpu.py runs both paths).  A batch with a longer run sets the handle's `stall` word:
// nothing of it -- nor of any later batch already in flight -- is applied, and the host replays those
// batches, in order, through the sorted path (raftq_step.hip: replay_stalled).
// A slice [q0, q1) of the PREVIOUS batch's result records on its way to the host, carried by the first `blocks`
// workgroups of a kernel of THIS batch (step_d2h_kernel's loop).  As a kernel of its own that copy holds back this
// batch's kernels until it retires -- measured in round 1, profiles/r01/step_pipeline_trace.txt -- so a pipelined batch
// cost walk + copy; inside this batch's kernels the two overlap (the copy is PCIe-bound, the kernels HBM-latency-bound).
// The slice that ends the records also clears the device copy of the tail for the slot's next batch (zero_tail).
struct CopyRide {
  const u64x2* src;
  u64x2* dst;
  uint64_t q0, q1, q_last;  // q_last: index of the tail quad
  uint32_t blocks;
};

__device__ __forceinline__ void copy_ride(const CopyRide& c) {
  const uint64_t stride = (uint64_t)c.blocks * kBlock;
  for (uint64_t q = c.q0 + (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < c.q1; q += stride) {
    const u64x2 v = c.src[q];
    __builtin_nontemporal_store(v, c.dst + q);
    if (q == c.q_last) const_cast<u64x2*>(c.src)[q] = u64x2{0, 0};
  }
}

static __global__ __launch_bounds__(kBlock) void step_link_kernel(const MsgRec* __restrict__ msgs, uint64_t n,
                                                                  uint64_t n_groups, uint32_t n_peers, bool msg_flags, uint8_t recs,
                                                                  NodeRec* rec, uint32_t* __restrict__ next,
                                                                  unsigned int* bad, unsigned int* stall,
                                                                  void* __restrict__ out, uint8_t compact, CopyRide ride, bool props, bool cq, bool pv, bool lt, bool ri) {
  if (blockIdx.x < ride.blocks) {
    copy_ride(ride);
    return;
  }
  const uint64_t i = (uint64_t)(blockIdx.x - ride.blocks) * kBlock + threadIdx.x;
  bool is_bad = false, too_long = false;
  if (i < n) {
    const RecClass c = classify(msgs[i], n_groups, n_peers, msg_flags, recs, props, cq, pv, lt, ri);
    is_bad = c == kBad;
    if (c == kTake) {
      NodeRec* r = rec + msgs[i].group;  // three atomics on one line
      next[i] = atomicExch(&r->lst_head, (uint32_t)i);
      too_long = atomicAdd(&r->lst_cnt, 1u) + 1 > kMaxRun;
      atomicMin(&r->lst_min, (uint32_t)i);
    } else if (c == kSkip) {
      // nobody's: answered on the spot.  (A batch that turns out bad or stalled is not applied and its results are not
      // read -- a replay through the sorted walk writes this record again.)
      put_skipped(out, i, compact);
    }
  }
  if (__ballot(is_bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
  if (__ballot(too_long) != 0 && (threadIdx.x & 63) == 0) atomicOr(stall, 1u);
}

// ---- (3, 3b) the walks and the tail reports, each under its name over every slot and as *_voters_kernel over each group's own
// voters (raftq_step_set_voters): one text, expanded twice
#define RAFTQ_WALK_CQ false
#define RAFTQ_WALK_READS_PARAM
#define RAFTQ_WALK_READS
#define RAFTQ_WALK_KERNEL(stem) stem##_kernel
#define RAFTQ_WALK_MASKED false
#define RAFTQ_WALK_PARAM
#define RAFTQ_WALK_VOTERS
#include "raftq_step_walk_kernels.inc"
#undef RAFTQ_WALK_KERNEL
#undef RAFTQ_WALK_MASKED
#undef RAFTQ_WALK_PARAM
#undef RAFTQ_WALK_VOTERS
#define RAFTQ_WALK_KERNEL(stem) stem##_voters_kernel
#define RAFTQ_WALK_MASKED true
#define RAFTQ_WALK_PARAM , const uint16_t* __restrict__ voters
#define RAFTQ_WALK_VOTERS , voters
#include "raftq_step_walk_kernels.inc"
#undef RAFTQ_WALK_KERNEL
#undef RAFTQ_WALK_MASKED
#undef RAFTQ_WALK_PARAM
#undef RAFTQ_WALK_VOTERS
// ... and the two walks twice more as *_lead_kernel / *_lead_voters_kernel: NodeT's LEAD form (raftq_respond_set_lead), launched by
// raftq_step_frames_respond alone.  The tail reports answer nobody and have no such form.
#define RAFTQ_WALK_NO_DELTAS
#define RAFTQ_WALK_KERNEL(stem) stem##_lead_kernel
#define RAFTQ_WALK_MASKED false, true
#define RAFTQ_WALK_PARAM
#define RAFTQ_WALK_VOTERS
#include "raftq_step_walk_kernels.inc"
#undef RAFTQ_WALK_KERNEL
#undef RAFTQ_WALK_MASKED
#undef RAFTQ_WALK_PARAM
#undef RAFTQ_WALK_VOTERS
#define RAFTQ_WALK_KERNEL(stem) stem##_lead_voters_kernel
#define RAFTQ_WALK_MASKED true, true
#define RAFTQ_WALK_PARAM , const uint16_t* __restrict__ voters
#define RAFTQ_WALK_VOTERS , voters
#include "raftq_step_walk_kernels.inc"
#undef RAFTQ_WALK_KERNEL
#undef RAFTQ_WALK_MASKED
#undef RAFTQ_WALK_PARAM
#undef RAFTQ_WALK_VOTERS
// ... and all four walks once more as *_cq_* over NodeT's CQ form (raftq_set_check_quorum): what a handle with the switch on launches.
// The tail reports run none of the four rules and have no such form.
#undef RAFTQ_WALK_CQ
#undef RAFTQ_WALK_READS_PARAM
#undef RAFTQ_WALK_READS
#define RAFTQ_WALK_CQ true
#define RAFTQ_WALK_READS_PARAM , ReadRec* __restrict__ reads
#define RAFTQ_WALK_READS , nullptr, reads
#define RAFTQ_WALK_KERNEL(stem) stem##_cq_kernel
#define RAFTQ_WALK_MASKED false, false, true, true
#define RAFTQ_WALK_PARAM
#define RAFTQ_WALK_VOTERS
#include "raftq_step_walk_kernels.inc"
#undef RAFTQ_WALK_KERNEL
#undef RAFTQ_WALK_MASKED
#undef RAFTQ_WALK_PARAM
#undef RAFTQ_WALK_VOTERS
#undef RAFTQ_WALK_READS
#define RAFTQ_WALK_READS , reads
#define RAFTQ_WALK_KERNEL(stem) stem##_cq_voters_kernel
#define RAFTQ_WALK_MASKED true, false, true, true
#define RAFTQ_WALK_PARAM , const uint16_t* __restrict__ voters
#define RAFTQ_WALK_VOTERS , voters
#include "raftq_step_walk_kernels.inc"
#undef RAFTQ_WALK_KERNEL
#undef RAFTQ_WALK_MASKED
#undef RAFTQ_WALK_PARAM
#undef RAFTQ_WALK_VOTERS
#undef RAFTQ_WALK_READS
#define RAFTQ_WALK_READS , nullptr, reads
#define RAFTQ_WALK_KERNEL(stem) stem##_cq_lead_kernel
#define RAFTQ_WALK_MASKED false, true, true, true
#define RAFTQ_WALK_PARAM
#define RAFTQ_WALK_VOTERS
#include "raftq_step_walk_kernels.inc"
#undef RAFTQ_WALK_KERNEL
#undef RAFTQ_WALK_MASKED
#undef RAFTQ_WALK_PARAM
#undef RAFTQ_WALK_VOTERS
#undef RAFTQ_WALK_READS
#define RAFTQ_WALK_READS , reads
#define RAFTQ_WALK_KERNEL(stem) stem##_cq_lead_voters_kernel
#define RAFTQ_WALK_MASKED true, true, true, true
#define RAFTQ_WALK_PARAM , const uint16_t* __restrict__ voters
#define RAFTQ_WALK_VOTERS , voters
#include "raftq_step_walk_kernels.inc"
#undef RAFTQ_WALK_KERNEL
#undef RAFTQ_WALK_MASKED
#undef RAFTQ_WALK_PARAM
#undef RAFTQ_WALK_VOTERS
#undef RAFTQ_WALK_CQ
#undef RAFTQ_WALK_READS_PARAM
#undef RAFTQ_WALK_READS
#undef RAFTQ_WALK_NO_DELTAS

// ---- the record array's bulk paths (raftq_load_node / raftq_read_node: set-up and test traffic, not the hot path) ----------
static __global__ __launch_bounds__(kBlock) void node_init_kernel(NodeRec* rec, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  NodeRec r;
  __builtin_memset(&r, 0, sizeof r);
  r.lst_head = r.lst_min = kNil;
  rec[i] = r;
}
// the record's copies of what the dense kernels own, re-read (see NodeRec): one lane per group
static __global__ __launch_bounds__(kBlock) void node_mirror_kernel(NodeArrays a, uint64_t n) {
  const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= n) return;
  NodeRec* r = a.rec + g;
  r->role = a.role[g];
  r->committed = a.committed[g];
  r->first_idx = a.first_idx[g];
#pragma unroll
  for (uint32_t p = 0; p < (uint32_t)kMaxPeers; ++p) r->match[p] = p < a.n_peers ? a.match[(uint64_t)p * a.ld + g] : 0;
}
// field: 0 term, 1 vote, 2 lead, 3 last_index, 4 last_term.  `flat` is the ABI's array for groups [g0, g0 + n): u64 or u32.
template <bool PUT>
static __global__ __launch_bounds__(kBlock) void node_field_kernel(NodeRec* rec, uint64_t g0, uint64_t n, int field, void* flat) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  NodeRec* r = rec + g0 + i;
  uint64_t* f64 = static_cast<uint64_t*>(flat);
  uint32_t* f32 = static_cast<uint32_t*>(flat);
  if (PUT) {
    if (field == 0) r->term = f64[i];
    else if (field == 1) r->vote = (uint8_t)f32[i];
    else if (field == 2) r->lead = (uint8_t)f32[i];
    else if (field == 3) r->last_index = f64[i];
    else r->last_term = f64[i];
  } else {
    if (field == 0) f64[i] = r->term;
    else if (field == 1) f32[i] = r->vote;
    else if (field == 2) f32[i] = r->lead;
    else if (field == 3) f64[i] = r->last_index;
    else f64[i] = r->last_term;
  }
}

// ---- (4) results -> pinned, device-mapped host memory.  A small grid (grid-stride, 16 B per lane): the
// transfer is PCIe-bound and 64 workgroups keep the link full (77 us for 4 MB, the same as the
// runtime's own blit copy).
// zero_tail: the last quad is the batch's {touched count, bad, skipped} tail; once it is on its way to the host the
// device copy is cleared for the slot's next batch (saves that batch a reset launch).
static __global__ __launch_bounds__(kBlock) void step_d2h_kernel(const u64x2* __restrict__ src, u64x2* __restrict__ dst,
                                                                 uint64_t n_quads, bool zero_tail = false) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_quads; i += stride) {
    const u64x2 v = src[i];
    __builtin_nontemporal_store(v, dst + i);
    if (zero_tail && i == n_quads - 1) const_cast<u64x2*>(src)[i] = u64x2{0, 0};
  }
}

}  // namespace raftqk
