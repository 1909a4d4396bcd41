// raftq_internal.hpp -- the handle behind raftq_t, shared by the translation units
// that implement include/raftq.h (raftq_capi.hip) and include/raftq_step.h (raftq_step.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "raftq.h"
#include "raftq_wire.h"
#include "raftq_kernels.hpp"
#include "raftq_buffers.hpp"

struct raftq {
  int device = 0;
  uint64_t G = 0, gpad = 0, ld = 0;  // groups, groups padded to the tile granule, row stride
  uint32_t N = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  struct raftq_set* in_set = nullptr;  // member of a sweep set: the set owns the stream
  uint64_t* match = nullptr;
  uint64_t* committed[2] = {nullptr, nullptr};
  int cur = 0;
  uint64_t* first_idx = nullptr;
  uint8_t* votes = nullptr;
  // per-group voter masks (raftq_load_voters / raftq_apply_voter_deltas): u16 [ld], bit p = slot p votes in the group; nullptr =
  // none loaded: every slot votes in every group and the sweeps are the unmasked kernels
  uint16_t* voters = nullptr;
  uint8_t* outcome = nullptr;
  uint64_t* changed_bits = nullptr;
  uint4* partials = nullptr;
  uint4* h_partials = nullptr;  // pinned
  uint64_t n_partials = 0;      // of the most recent sweep
  uint64_t max_partials = 0;
  uint64_t* offsets = nullptr;  // [max_partials + 1]; last = total
  uint64_t* h_total = nullptr;  // pinned
  // The buffers below own their memory (raftq_buffers.hpp): members of the handle, released when it is deleted -- after
  // raftq_destroy's waits and before it destroys the handle's streams.
  // Delta staging the kernels access directly over PCIe (no staging memcpy launches); calls that read results back use it.
  raftq_buf::Buffer<> stage{raftq_buf::Kind::mapped};
  // The batching turn's ack buffer (raftq_stage*, raftq_cycle*, raftq_apply_[vote_]deltas).  Behind a large BAR it lives IN
  // HBM: posted PCIe writes land there as the acks arrive (45 GB/s measured from one core) and the ingest kernel reads HBM
  // instead of pulling the batch over PCIe in 64-byte requests (35 GB/s, 30 of a turn's 52 kernel-us).  The host only ever
  // WRITES it (reads over the BAR are uncached and slow).
  raftq_buf::HostWritable ingest;
  raftq_buf::BarRule bar;       // .staging decided at create: large BAR present and not disabled (RAFTQ_STAGE=host)
  // raftq_apply_log_deltas' host bookkeeping, kept across calls: per-group (epoch << 32 | records seen this call)
  std::vector<uint64_t> ld_mark, ld_start;
  // raftq_apply_log_deltas_nowait: two pinned staging areas taken in turn, an event each (the kernels that read it have run)
  struct LdNowait {
    raftq_buf::Buffer<> buf{raftq_buf::Kind::mapped};
    hipEvent_t ev = nullptr;
  };
  LdNowait ld_nowait[2];
  uint32_t ld_nowait_next = 0;
  std::vector<uint32_t> ld_round, ld_pos;
  uint32_t ld_epoch = 0;
  raftq_buf::Buffer<raftqk::Advance> adv{raftq_buf::Kind::mapped_coherent};  // compacted advance list
  uint64_t adv_listed = 0;     // entries of adv.h valid after the last collect / cycle
  bool adv_packed = false;     // ... in the 16-byte layout (raftq_cycle_packed)
  // RAFTQ_CYCLE_SEGMENTED: the last list lies in adv.h as one segment of seg_stride records per sweep tile, seg_h.h[t] of them valid
  bool adv_segmented = false;
  raftq_buf::Buffer<uint32_t> seg_h{raftq_buf::Kind::mapped_coherent};  // per-tile counts
  raftq_buf::Buffer<unsigned int> seg_d{raftq_buf::Kind::device};       // device copy (the flag kernel adds them up)
  uint32_t seg_tiles = 0, seg_stride = 0, seg_one = 0;  // seg_one: the count of a contiguous list presented as one segment
  uint64_t flag_mask = ~0ull;  // which bits of the completion word are the epoch the turn's wait compares (segmented: the top half)
  uint32_t* self_max = nullptr;  // device: the self-max word (raftq_kernels.hpp) -- which match row is every group's largest
  // The narrow mirror (raftq_kernels.hpp kNarrowValid): its word is self_max[1], always there and 0 until a build pass; the
  // arrays are allocated by the first build (both or neither: a handle that cannot have them simply has no mirror).
  uint64_t* anchor = nullptr;    // device u64 [ld]
  uint32_t* moff = nullptr;      // device u32 [N][ld]
  bool narrow_off = false;       // RAFTQ_NARROW=0 at raftq_create: never build the mirror
  uint32_t* narrow_word() const { return self_max + 1; }
  raftqk::NarrowMirror narrow_mirror() const { return raftqk::NarrowMirror{self_max + 1, anchor, moff}; }
  // The tally mirror (raftq_kernels.hpp kTallyValid): its word is self_max[2]; the bytes are allocated, zeroed, by raftq_create
  // with the word valid (all-zero vote words have an all-zero tally) -- or never, under RAFTQ_TALLY=0, and the word stays 0.
  uint8_t* tally = nullptr;      // device u8 [ld]: granted | rejected << 4 of votes[g]
  uint32_t* tally_word() const { return self_max + 2; }
  raftqk::TallyMirror tally_mirror() const { return raftqk::TallyMirror{self_max + 2, tally}; }
  uint64_t compact_epoch = 0;  // completion-flag values handed to hipStreamWriteValue64 (h_total[3])
  uint64_t compact_epoch_armed = 0;  // epoch the current turn's wait may poll for (0 = blocking wait)
  // wait_turn: consecutive waits whose flag did not land in time and waits sat out since -- per KIND of wait ([0] the batching
  // turn, [1] every other call that ends on the completion word: codecs, tick lists): a codec call under a profiler must not
  // switch the turn's wake-up off
  uint32_t flag_misses[2] = {0, 0}, flag_rested[2] = {0, 0};
  uint64_t flag_fallbacks = 0;                // turns that ended in the blocking wait although a flag was armed
  uint32_t* claim = nullptr;    // u32 [N][ld] vote-slot claims, lazily allocated
  // sparse ingest: device copy of the batch (validated on the way in) and the "bad batch" epoch words
  raftq_buf::Buffer<> delta_dev{raftq_buf::Kind::device};
  unsigned long long* delta_bad = nullptr;  // device: [0] match deltas, [1] vote deltas -- epoch of the last bad batch
  unsigned long long delta_epoch = 0;       // batches enqueued so far
  unsigned long long delta_check[2] = {0, 0};  // epochs whose host-visible flag (h_total[1], [2]) is still to be checked
  // batched Tick state, lazily allocated
  uint8_t* role = nullptr;      // [ld]
  uint32_t* elapsed = nullptr;  // [ld]
  uint8_t* action = nullptr;    // [ld]
  uint64_t* hup_bits = nullptr; // [gpad/64]
  uint64_t* beat_bits = nullptr; // [gpad/64]
  uint4* tick_partials = nullptr;  // [gpad/256]
  // raftq_tick_collect_lists: the two lists left in place (page-locked; 4-byte group ids; MsgBeat optionally as a bitmap)
  raftq_buf::Buffer<uint32_t> tl{raftq_buf::Kind::mapped_coherent};  // [tl_hup_cap] MsgHup ids | [tl_beat_cap] MsgBeat ids | beat bitmap (gpad / 64 words, 16-byte aligned)
  uint64_t tl_hup_cap = 0, tl_beat_cap = 0, tl_beat_at = 0, tl_map_off = 0;  // tl_beat_at: index of the first MsgBeat id; tl_map_off: byte offset of the bitmap
  uint64_t tl_n_hup = 0, tl_n_beat = 0;
  unsigned tl_flags = 0;
  bool tl_valid = false;
  uint64_t* tick_offsets2 = nullptr;  // [gpad/256 + 1]: the MsgBeat offsets of raftq_tick_collect on handles of more than 16K waves
  uint32_t election_tick = 10, heartbeat_tick = 1;  // reference raft.go:154-155
  uint64_t tick_seed = 0x1000, tick_no = 0;
  bool ticked = false;
  // raftq_set_check_quorum: both or neither (`cq` stands for the switch).  One dense word per group -- activity bits (bit p =
  // Progress[p].RecentActive) | lead_elapsed << 16 -- that tick_check_kernel streams and a Step lane reads lazily; the bitmap of the
  // groups the last raftq_tick gave action 3 (raftq_collect_checks)
  uint32_t* cq = nullptr;        // [ld]
  uint64_t* chk_bits = nullptr;  // [gpad/64]
  bool pre_vote = false;         // raftq_set_pre_vote: only ever true while cq is set
  bool lead_transfer = false;    // raftq_set_lead_transfer: likewise; leadTransferee is bits 12..15 of the cq word, which are 0 without it
  // raftq_set_read_index: 0 = off, RAFTQ_READ_SAFE, RAFTQ_READ_LEASE; only ever non-zero while cq is set.  reads: [ld] 64-byte records
  // {seq, acked[RAFTQ_MAX_PEERS], pad} (raftqk::ReadRec) that Step alone touches, allocated in the safe mode only
  uint8_t read_index = 0;
  void* reads = nullptr;
  // raftq_tick_set_checks (0 = off): with cq set, the fused Tick calls run instead of refusing and leave the groups whose check failed as
  // a third in-place list of at most this many ids behind the beat bitmap in `tl` (raftq_last_tick_checks).  A property of the handle,
  // as tick_voters is: raftq_clone_state leaves it alone
  uint64_t tick_chk_cap = 0;
  uint64_t tl_chk_cap = 0, tl_chk_off = 0, tl_n_chk = 0;  // of the last fused call: ids listed at most, their byte offset in tl, the total
  bool tl_chk_valid = false;     // the last call on the handle was a fused Tick call under the switch
  uint64_t* tick_offsets3 = nullptr;  // [gpad/256 + 1]: the failed checks' offsets on handles of more than 16K waves
  uint64_t* d_total = nullptr;  // device alias of h_total
  bool have_terms = false;
  unsigned last_flags = 0;
  int last_gpl = 0;
  const uint64_t* last_old = nullptr;
  const uint64_t* last_new = nullptr;
  // batched Step node state (raftq_step.hip), lazily allocated
  uint32_t self_peer = 0;
  bool self_set = false;  // raftq_set_self has been called: the handle is a node's (raftq_tick_frames asks)
  // the records' copies of the dense arrays (role, committed, first_idx, match) are what those arrays hold: false after anything but
  // Step / tail reports / proposals wrote them -- every such writer calls raftq_detail::dense_changed --; the next Step-family call
  // re-reads them first (raftq_step.hip ensure_mirror)
  bool node_mirror_fresh = false;
  uint64_t node_mirror_refreshes = 0;
  void* node_rec = nullptr;        // raftqk::NodeRec [ld]: term, vote, lead, last_index, last_term + the list words of the batch in flight
  unsigned int* step_stall = nullptr;  // device word: a batch needs the sorted path; later batches wait for the replay
  uint8_t step_compact = 0;        // result records: 0 = 64 bytes, 1 = 40, 2 = 32 (raftq_step_set_compact)
  bool step_msg_flags = false;     // raftq_msg_t._pad[1] / _resv carry RAFTQ_MSGF_* (raftq_step_set_msg_flags); padding otherwise
  bool step_voters = false;        // raftq_step_set_voters: with masks loaded the Step family runs the *_voters_kernel twins (a property of
                                   // the handle: raftq_clone_state and raftq_load_voters(h, NULL) leave it alone)
  bool step_props = false;         // raftq_step_set_props: Step takes a forwarded proposal (MsgProp, by its entry count) and the frames calls
                                   // flag one RAFTQ_MSGF_ENTRIES instead of RAFTQ_MSGF_HOLD (a property of the handle, as step_voters)
  bool tick_voters = false;        // raftq_tick_set_voters: with masks loaded Tick runs tick_voters_kernel (promotable()) and the two
                                   // device-built rounds go to each group's own members (the same kind of property as step_voters)
  bool bcast_voters = false;       // raftq_bcast_set_voters: with masks loaded raftq_step_frames_respond's commit broadcast and
                                   // raftq_propose_frames' bcastAppend go to each group's own members (the same kind of property)
  bool resp_lead = false;          // raftq_respond_set_lead: raftq_step_frames_respond answers RAFTQ_OUT_BECAME_LEADER too (the *_lead_kernel
                                   // walks, resp_scatter_lead[_voters]_kernel); the same kind of property
  bool resp_props = false;         // raftq_respond_set_props: raftq_step_frames_respond answers a RAFTQ_OUT_PROPOSED at the tail too (the same
                                   // walks and scatter kernels, NodeArrays::ans_props); the same kind of property
  bool prop_forward = false;       // raftq_propose_set_forward: raftq_propose_frames turns a follower's record into a MsgProp frame to its
                                   // leader (the *_fwd_kernel forms, raftq_propose_kernels.hpp); the same kind of property
  int step_walk_mode = 1;         // 1 = lists (default), 0 = always the sorted walk (RAFTQ_STEP_WALK=sort)
  uint32_t step_stalls_in_a_row = 0, step_sorted_left = 0;  // back-off from the list walk under hot-group traffic
  uint64_t step_replays = 0;       // batches that went through the sorted path after a stall
  // raftq_step_batch / _submit / _collect: two batches may be in flight, each in its own slot
  // (pinned staging in, device scratch, pinned results out), pipelined over two streams (DMA in | kernels +
  // result copy): the H2D of batch k+1 overlaps the kernels and the result copy of batch k
  // Batches of the pipelined Step in flight at most.  Three, because a batch's result copy rides in the walk kernel of
  // the batch behind it (see copy_pending): while the host waits for batch k it must be able to have batch k+1 on the
  // device AND be handing over batch k+2 -- with two slots that form lost to round 1's (profiles/r02/step_deferred_copy_ab.txt).
  static constexpr int kStepSlots = 3;
  struct StepSlot {
    raftq_buf::Buffer<> in_h{raftq_buf::Kind::pinned};  // staging: the copying forms (caller-owned arrays, received frames) go through it
    // what raftq_step_stage hands out behind a large BAR: fine-grained DEVICE memory the producer writes in place (posted PCIe
    // writes); the batch then never needs a DMA.  Device memory or empty: without a BAR the slot stages in in_h
    raftq_buf::HostWritable in_bar;
    raftq_buf::Buffer<> dev{raftq_buf::Kind::device};  // scratch: msgs, keys, order, outs, sort temp, flags
    raftq_buf::Buffer<> out{raftq_buf::Kind::mapped};  // result records + {touched-group count, bad flag}
    uint64_t n = 0;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    bool busy = false;
    bool lists = false;            // submitted through the sort-free walk
    bool replayed = false;         // already re-run through the sorted path (after a stall)
    // the batch's result copy has not been enqueued yet: it rides in the NEXT batch's walk kernel (a copy kernel of its
    // own keeps that batch's kernels from starting until it retires), or is launched by the batch's collect
    bool copy_pending = false;
    const void* w_off_in_place = nullptr;     // raftq_step_stage_wire: the decoder read the frame boundaries / the stream where
    const void* w_stream_in_place = nullptr;  // the producer wrote them (in_bar)
    size_t w_stage_stream_off = 0;            // where raftq_step_stage_wire put the stream within the slot's staging
    const void* msgs_in_place = nullptr;  // the walk read this batch's records where the producer wrote them (in_bar), not in `dev`
    const void* outs_d = nullptr;  // device result records of this batch (in `dev`)
    uint64_t out_quads = 0;        // ... in 16-byte units, tail included
    int end_bit = 0;
    uint32_t rec = 64;             // bytes per result record of this batch (64, or 40 compact)
    bool tail_zeroed = false;      // the device copy of the 16-byte result tail is known to be zero (for tail_n, tail_dev)
    uint64_t tail_n = 0;
    uint32_t tail_rec = 0;
    const void* tail_dev = nullptr;
    uint64_t w_nbytes = 0;
    // raftq_step_submit_wire: where this batch's decoded records sit in `dev`, and the pinned
    // copies raftq_step_wire_msgs / _entries hand out (fetched on demand)
    bool wire = false;
    uint8_t recs = 0;              // raftqk::kRecsCaller / kRecsWire / kRecsFrames: whose records the batch holds (replays need it)
    void* w_msgs_d = nullptr;      // raftq_wire_msg_t [n]
    void* w_ents_d = nullptr;      // raftq_wire_ent_t [w_ents_cap]
    const uint64_t* w_ent_total_d = nullptr;
    uint64_t w_ents_cap = 0;
    raftq_buf::Buffer<> w_pin{raftq_buf::Kind::pinned};  // msgs, then entries
    bool w_msgs_fetched = false, w_ents_fetched = false;
    uint64_t w_n_ents = 0;
  } step_slot[kStepSlots];
  int step_last_slot = -1;         // slot of the last collected batch
  uint64_t step_submitted = 0, step_collected = 0;  // slot of batch k = k % kStepSlots
  hipStream_t step_s_in = nullptr, step_s_out = nullptr;  // the inbound DMA; fetch_wire's copies (not behind the batch in flight)
  bool step_defer_copy = true;     // RAFTQ_STEP_DEFER_COPY=0: every batch launches its own result copy (round 1's form; for A/B)
  const void* step_last_out = nullptr;  // results of the last collected batch
  uint64_t step_last_n = 0;
  uint32_t step_last_rec = 64;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // raftq_sweep_many_async over handles that share one stream: every other launch goes to this auxiliary stream
  hipStream_t many_aux = nullptr;
  hipEvent_t many_fork = nullptr, many_join = nullptr;
  // wire / WAL codecs (raftq_wire.hip): growable device scratch (inputs + temporaries), device
  // output buffer, a small pinned block for totals / flags
  raftq_buf::Buffer<> wire_dev{raftq_buf::Kind::device};
  raftq_buf::Buffer<> wire_out{raftq_buf::Kind::device};
  uint64_t* wire_pin = nullptr;    // pinned, 256 bytes: four result words behind each of kPinCall / kPinWalPending / kPinRespond (raftq_wire.hip)
  uint64_t* wire_pin_d = nullptr;  // the same block as the device addresses it (the codecs' last kernel writes totals / flags there)
  unsigned long long* wire_flags = nullptr;  // device, 64 bytes, zero between calls: the codecs' malformed counters / bad flags
  // the streaming codec kernels (raftq_wire_kernels.hpp "the streaming form"): ticket word + per-tile look-back status
  raftq_buf::Buffer<unsigned long long> wire_lb{raftq_buf::Kind::device};  // kLbHead words {ticket, gave-up flag | landed waves | - | chunk ticket}, then kLbArrays status arrays of wire_lb_tiles words
  uint64_t wire_lb_tiles = 0;                // words per status array; 0: no block, or one that is not trusted any more
  uint32_t wire_ticket_base = 0, wire_epoch = 0;
  uint32_t wire_chunk_base = 0, wire_chunk_pending = 0;  // the readers' chunk tickets (the head's fourth word), accounted like the tiles'
  bool wire_chunk_unknown = false;           // the last launch had no reader workgroups: how far its chunk ticket got is not known
  unsigned int prop_stamp = 0;               // raftq_propose_frames: the call's stamp (its validation's verdict word holds it when a record was refused)
  // raftq_propose_set_forward: the outcome bytes of the last raftq_propose_frames call that succeeded with the switch on
  // (raftq_propose_outcomes) -- pinned and device-mapped, the check kernel stores them there by the wave
  raftq_buf::Buffer<uint8_t> prop_what{raftq_buf::Kind::mapped};
  uint64_t prop_what_n = 0;
  // raftq_step_frames_respond: the walk's response records + the layout's counts (device), and what the walk reads while the
  // call is on (resp_on): the call's stamp, the caller's at-tail bitmap as the device addresses it
  raftq_buf::Buffer<> resp_dev{raftq_buf::Kind::device};
  bool resp_on = false;
  uint32_t resp_stamp = 0;
  const uint64_t* resp_at_tail_d = nullptr;
  uint32_t resp_ent_base = 0;  // raftq_respond_set_props: entry headers the call's decoder can hand back (a proposal whose entries lie beyond is the host's)
  // raftq_wal_encode_begin .. _end: enqueued, its totals in wire_pin[kPinWalPending ..]; `done`: a later wait has covered it and what _end
  // will report is kept here
  bool wal_pending = false, wal_pending_done = false;
  bool wal_pending_waited = false;  // a wait on the handle's stream has come back since the begin: its kernel has run
  uint64_t wal_pending_n = 0, wal_pending_cap = 0;
  uint32_t wal_pending_prev = 0;
  int wal_pending_rc = 0;
  raftq_wal_counts_t wal_pending_counts{};
  std::string wal_pending_err;
  std::string err;
  // RAFTQ_PROFILE=1: host-side phase times of raftq_cycle, printed at destroy
  double prof[6] = {0, 0, 0, 0, 0, 0};
  uint64_t prof_n = 0;
};


// A set of handles of one shape on one GPU, swept by a single dispatch (raftq_set_*).
struct raftq_set {
  // the set's device and pinned memory: members, so `delete s` releases them (raftq_set_destroy: after its wait, before the stream goes)
  template <class T>
  struct Dev : raftq_buf::Buffer<T> {
    Dev() : raftq_buf::Buffer<T>(raftq_buf::Kind::device) {}
  };
  int device = 0;
  uint32_t N = 0;
  uint64_t gpad = 0;
  std::vector<raftq_t*> members;
  hipStream_t stream = nullptr;       // the set's stream; every member is re-homed onto it
  // device tables of the members' SweepArgs: [0] every member reads commit buffer 0, [1] buffer 1,
  // [2] rebuilt per launch when the members' buffers differ (someone swept a member on its own)
  Dev<raftqk::SweepArgs> tab[3];
  std::vector<raftqk::SweepArgs> tab_host;  // pageable on purpose: hipMemcpyAsync stages it before returning
  Dev<uint64_t> counts;               // [members][4] {changed, won, lost, 0}, reduced on the device
  Dev<uint64_t> np;                   // [members] number of per-wave partials of each member's last sweep
  std::vector<uint64_t> np_host;
  raftq_buf::Buffer<uint64_t> counts_h{raftq_buf::Kind::pinned};  // counts, copied out
  bool swept = false;
  bool broken = false;                // a member was destroyed under the set
  bool tab_stale = false;             // a member allocated its narrow mirror -- or, in a set that admits masks, its mask array came
                                      // or went -- since tab[0] / tab[1] (and vtab[0] / vtab[1]) were filled
  // raftq_set_create_voters: members may hold voter masks.  vtab[k] is tab[k] with every member's mask pointer beside its
  // SweepArgs (null: no masks loaded); a dispatch with at least one masked member reads it (sweep_set_voters_kernel), every
  // other dispatch reads tab[k] and launches what a plain set launches.  Empty in a set from raftq_set_create.
  bool allow_voters = false;
  Dev<raftqk::VoterSweepArgs> vtab[3];
  std::vector<raftqk::VoterSweepArgs> vtab_host;
  unsigned last_flags = 0;
  int mode = 0;                       // 0 = K-deep grid, 1 = persistent walk (raftq_set_mode)
  uint32_t persist_wgs = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // raftq_set_tick: device table of the members' TickArgs (as of tick_host), set ticks dispatched since it was built
  Dev<raftqk::TickArgs> tick_tab;
  std::vector<raftqk::TickArgs> tick_host;
  uint64_t tick_since = 0;
  // ... and of their TickVotersArgs, for the set ticks in which a member asks promotable() (tick_set_voters_kernel): a table and
  // a count of its own, so either dispatch finds the other's table stale by the tick numbers alone
  Dev<raftqk::TickVotersArgs> tick_vtab;
  std::vector<raftqk::TickVotersArgs> tick_vhost;
  uint64_t tick_vsince = 0;
  std::string err;
};


struct raftq_wire_counts;  // raftq_wire.h
namespace raftqk {
struct NodeArrays;  // raftq_step_kernels.hpp
}
namespace raftq_detail {
// raftq_step.hip, for raftq_propose_frames (raftq_wire.hip): Step's device state exists (allocated on first use) and *out views it
int node_arrays_of(raftq_t* h, raftqk::NodeArrays* out);
int fail(raftq_t* h, int code, const std::string& msg);
int use_device(raftq_t* h);
int use_device_idle(raftq_t* h, const char* who);  // + no Step batch in flight (RAFTQ_ESTATE otherwise)
// RAFTQ_ESTATE for a handle with voter masks loaded.  step_family (raftq_step_batch / _submit* / _frames / _frames_packed,
// raftq_apply_log_deltas*): let through once the handle opted in (raftq_step_set_voters) -- those calls then run over each group's
// own voters.  tick_rounds (raftq_tick_frames, raftq_tick_elect_frames): let through once the handle opted in to
// raftq_tick_set_voters -- their rounds then go to each group's own members.  bcast (raftq_step_frames_respond,
// raftq_propose_frames): let through once the handle opted in to raftq_bcast_set_voters -- their broadcasts then go to each group's
// own members.  Each of the three switches opens its own calls and no others.
int refuse_voters(raftq_t* h, const char* who, bool step_family = false, bool tick_rounds = false, bool bcast = false);
// Every writer of the dense arrays (role, committed, first_idx, match) outside Step calls this: the records' copies are stale
// (raftq_t::node_mirror_fresh), and the next Step-family call re-reads them first
inline void dense_changed(raftq_t* h) { h->node_mirror_fresh = false; }
// raftq_tick_set_voters on a handle with masks loaded: every Tick launch is tick_voters_kernel's, the rounds are beat_build_voters_kernel's and elect_build_voters_kernel's
inline bool masked_tick(const raftq_t* h) { return h->voters != nullptr && h->tick_voters; }
// raftq_bcast_set_voters on a handle with masks loaded: raftq_step_frames_respond walks with the masked Node and lays its answers
// out with the resp_*_voters_kernel entry points, raftq_propose_frames runs propose_check_voters_kernel / propose_build_voters_kernel
inline bool masked_bcast(const raftq_t* h) { return h->voters != nullptr && h->bcast_voters; }
// RAFTQ_ESTATE, "check quorum" in the text, on a handle with raftq_set_check_quorum on: the fused Tick calls and the device-built
// heartbeat / election rounds do not know a suppressed beat
// fused: the call is one raftq_tick_set_checks opens (let through once chk_cap > 0)
int refuse_check_quorum(raftq_t* h, const char* who, bool fused = false);
// RAFTQ_ESTATE, "pre vote" in the text, on a handle with raftq_set_pre_vote on: a call that turns a MsgHup into becomeCandidate on the device
int refuse_pre_vote(raftq_t* h, const char* who, bool fused = false);
// RAFTQ_ESTATE, "lead transfer" in the text, on a handle with raftq_set_lead_transfer on: a call whose kernels append a leader's own
// proposals without reading the word that says a transfer is pending
int refuse_lead_transfer(raftq_t* h, const char* who);
// RAFTQ_ESTATE, "read index" in the text, on a handle with raftq_set_read_index(h, RAFTQ_READ_SAFE): a call whose device-built
// heartbeat round would not carry the pending read's context
int refuse_read_index(raftq_t* h, const char* who);
// raftq_tick_set_checks on a handle with raftq_set_check_quorum on: the fused calls launch tick_check_kernel, list the failed checks and
// -- raftq_tick_elect_frames -- campaign through Node's CQ form (elect_build_cq_kernel / elect_build_cq_voters_kernel)
inline bool tick_checks(const raftq_t* h) { return h->cq != nullptr && h->tick_chk_cap != 0; }
int self_max_check(raftq_t* h);                 // the self-max word re-derived from the rows for h->self_peer (enqueued)
int narrow_build(raftq_t* h);                   // the narrow mirror and its word re-derived from the rows (enqueued)
int tally_build(raftq_t* h);                    // the tally bytes and their word re-derived from the vote words (enqueued)
int ensure_staging(raftq_t* h, size_t bytes);   // pinned, device-mapped staging (term deltas, campaign lists, log deltas)
int ensure_ingest(raftq_t* h, size_t bytes);    // the ack buffer of the batching turn: device memory behind a large BAR, else pinned
int ensure_tick_state(raftq_t* h);              // role / elapsed / action (+ hup bitmap)
void free_node_state(raftq_t* h);               // raftq_step.hip's allocations (called by raftq_destroy)
void free_wire_state(raftq_t* h);               // raftq_wire.hip's allocations (called by raftq_destroy)
// raftq_wire.hip, for raftq_step_frames (raftq_step.hip): the streaming decode with a node's checks, enqueued on the handle's
// stream and not waited for (the records also go to msgs_d, in HBM, for the Step kernels enqueued behind it); and what the
// decode has to say once the call's one wait is over.  RAFTQ_EINVAL when an array is not page-locked and 16-byte aligned.
// packed (raftq_step_frames_packed): `msgs` is the caller's array of narrow records of `form` bytes, wide[] gets the rest
// (to_slot = the handle's own); wire_frames_n_wide after the wait: how many wide records there were.
struct PackedDst {
  int form;  // RAFTQ_WIRE_FORM_40 | RAFTQ_WIRE_FORM_HEAD
  uint32_t head_types;
  void* wide;
  uint64_t wide_cap;
};
int wire_frames_enqueue(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off, uint64_t n, void* msgs, void* ents,
                        uint64_t ents_cap, void* msgs_d, int tail_appends, void* zero2 /* two device words left zero, or nullptr */,
                        const PackedDst* packed = nullptr);
uint64_t wire_frames_n_wide(raftq_t* h);
int wire_frames_finish(raftq_t* h, const uint64_t* frame_off, uint64_t n, bool have_ents, uint64_t ents_cap, ::raftq_wire_counts* counts);
// raftq_step_frames_respond (raftq_step.hip): the checks that come before anything is enqueued (every array page-locked and
// 16-byte aligned, the scratch allocated), then -- behind the Step chain, on the handle's stream -- the layout of the responses
// and their marshal; RespPlan carries the device views between them.  respond_finish reads the encoder's totals after the wait.
struct RespPlan {
  uint64_t n = 0, n_max = 0, cap = 0;  // results, frames the encoder is launched for (n * (N - 1)), out's size
  void* v_out = nullptr;
  uint64_t* v_resp_off = nullptr;
  uint64_t* peer_off = nullptr;        // the caller's (host) array, N + 1 words
  bool lead = false;                   // raftq_respond_set_lead: the encoder's input has an entry array, one slot per result
  // raftq_respond_set_props: ... and in front of those slots one per entry header the decoder can hand back (ent_base); the
  // encoder's pool is the decoder's copy of the inbound stream, which the marshal's scratch is laid out behind (keep)
  bool props = false;
  uint64_t ent_base = 0, nbytes = 0;
  const void* v_ents = nullptr;        // the caller's entry headers as the device addresses them
  const void* v_stream = nullptr;      // RAFTQ_RESPOND_PROPS_POOL=feed only: the caller's stream, which the encoder's readers bring in as the pool
  size_t keep = 0, pool_off = 0;       // bytes of the codecs' scratch the marshal leaves alone; where the stream's copy lies in them
};
int respond_prepare(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off, const void* msgs, const void* ents,
                    uint64_t ents_cap, const uint64_t* at_tail, void* out, uint64_t cap, uint64_t* resp_off, uint64_t* peer_off, uint64_t n,
                    RespPlan* p);
int respond_enqueue(raftq_t* h, const RespPlan& p);
int respond_finish(raftq_t* h, const RespPlan& p, ::raftq_wire_counts* resp_counts);
// raftq_tick_collect_lists in three steps (raftq_capi.hip), for raftq_tick_frames (raftq_wire.hip), which puts its kernels between
// the lists and the completion word: _prepare checks the flags and makes EVERY allocation of the Tick (a call that fails there has
// not ticked); _enqueue launches the tick kernel, the scans of a large handle and the lists kernel; _finish raises the completion
// word, waits for it and records what raftq_last_tick_lists hands out.  The caller has made sure no Step batch is in flight.
struct TickLists {
  unsigned flags;
  uint64_t cap_h, cap_b, beat_at, map_off;  // the in-place lists' layout (raftq_t::tl_*)
  const uint64_t* off_beat;                 // after _enqueue: scan_partials_kernel's MsgBeat offsets (more than 16K waves), or nullptr
  const uint64_t* off_h = nullptr;          // ... and its MsgHup offsets (raftq_tick_elect_frames)
  uint64_t cap_c = 0, chk_off = 0;          // raftq_tick_set_checks: ids of failed checks listed at most (0: the two-list form), their byte offset
};
int tick_lists_prepare(raftq_t* h, const char* who, unsigned flags, uint64_t hup_cap, uint64_t beat_cap, TickLists* tl);
int tick_lists_enqueue(raftq_t* h, TickLists* tl);
int tick_lists_finish(raftq_t* h, const char* who, const TickLists& tl, uint64_t* n_hup, uint64_t* n_beat);
// raftq_step.hip, for raftq_tick_frames: the handle's records exist and are fresh (ensure_mirror), voter masks refused --
// tick_rounds: unless the handle opted in to raftq_tick_set_voters (the two tick calls pass true); bcast: unless it opted in to
// raftq_bcast_set_voters (raftq_propose_frames passes true)
int node_records_of(raftq_t* h, const char* who, raftqk::NodeArrays* out, bool tick_rounds = false, bool bcast = false);
int respond_pass_ok(raftq_t* h);  // a pass of the marshal whose totals are about to be replaced (a stalled batch's first): it did not give up
// The wait that ends a call whose results the kernels wrote into page-locked memory themselves (the streaming codecs,
// raftq_step_frames): a one-thread kernel raises the handle's completion word behind everything enqueued so far and the host
// polls it (raftq_cycle's wait, raftq_capi.hip wait_turn) -- a stream synchronisation costs 15-20 us more than the word does.
// The blocking wait where the word cannot be had.
hipError_t wait_call(raftq_t* h);
}  // namespace raftq_detail

#define HIPCHK(h, expr)                                                                        \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      return raftq_detail::fail((h), _e == hipErrorOutOfMemory ? RAFTQ_ENOMEM : RAFTQ_EHIP,    \
                                std::string(#expr) + ": " + hipGetErrorString(_e));            \
    }                                                                                          \
  } while (0)
