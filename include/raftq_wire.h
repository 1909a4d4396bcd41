/*
 * raftq_wire.h -- C-ABI of the batched wire / WAL codecs: the
 * data formats either side of the quorum path.
 *
 * The reference moves two byte formats around its one raft group, both owned by
 * the un-vendored etcd dependency:
 *     rc.transport.Send(rd.Messages)        raft.go:230   raftpb.Message over rafthttp
 *     rc.wal.Save(rd.HardState, rd.Entries) raft.go:228   walpb.Record frames, CRC-32C chained
 *     w.ReadAll() in replayWAL              raft.go:122-134
 * With G groups per process those are per-message / per-record marshal calls in
 * G goroutines.  The entry points below do a whole batch on the GPU: protobuf
 * field encoding / parsing one lane per message, CRC-32C one lane per record
 * with the chain resolved by a parallel scan over (crc, x^(8 len)) pairs.
 *
 * FORMATS (restated from the published 2015-era etcd sources, v2.2-v2.3 line;
 * PARITY UNPINNED for the schema -- the .proto files are not on this machine --
 * but every byte produced is checked against the protobuf runtime on that schema
 * and against RFC 3720's CRC-32C vectors, see oracle/raftq_wire_oracle.c):
 *
 *   raftpb.Message   1 type  2 to  3 from  4 term  5 logTerm  6 index  7 entries*
 *                    8 commit  9 snapshot  10 reject  11 rejectHint  [12 group]
 *   raftpb.Entry     1 Type  2 Term  3 Index  4 Data  [5 group, WAL only]
 *   raftpb.HardState 1 term  2 vote  3 commit  [4 group]
 *   walpb.Record     1 type  2 crc  3 data       walpb.Snapshot  1 index  2 term
 *
 *   [n group] is this library's one extension: etcd runs a single group per
 *   process, so its messages carry none.  It is an ordinary varint field with an
 *   unused number, inside the CRC-covered bytes; a stock decoder skips it.
 *
 *   Encoding is canonical gogoproto (`nullable=false`): every scalar field is
 *   written, zero or not, in field order; Message.snapshot is always written
 *   (empty: 4a 08 12 06 0a 00 10 00 18 00); Entry.Data is omitted when empty.
 *   Decoding is ordinary protobuf: any field order, last scalar wins, unknown
 *   fields skipped, wrong wire type on a known field = malformed.
 *
 *   stream frame (rafthttp messageEncoder):  u64 BIG-endian length | Message
 *   WAL frame (wal/encoder.go, pre-3.0: no padding):  i64 LITTLE-endian length | Record
 *   Record.crc = crc32.Update(previous record's crc, castagnoli, Record.data)
 *   -- the running CRC of all Data bytes since the segment's crcType record.
 *
 * raft IDs on the wire are 1-based (raft.go:148-151); the structs carry peer
 * SLOTS (ID - 1) like the rest of this ABI.  An absent / zero ID decodes to
 * slot 0xFF (to) / 0xFFFFFFFF (from), which raftq_step_* rejects.
 *
 * No CPU path: all entry points need the handle's GPU.
 *
 * How a call moves its bytes.  When every array of a call is page-locked (hipHostMalloc /
 * hipHostRegister, or the handle's own staging areas) and 16-byte aligned, the call is ONE
 * kernel that reads the inputs and writes the outputs where they lie, both directions of
 * the link busy at once ("streaming form").  Otherwise (pageable memory, odd alignment, or
 * RAFTQ_WIRE_STREAMING=0 in the environment) inputs are copied in, outputs copied out
 * ("copying form").  Same results, byte for byte.  One difference a caller can see: a
 * streaming ENCODE that is refused (RAFTQ_EINVAL: cap too small, a range out of bounds, a
 * bad slot) has already been writing, so out[0 .. cap) and frame_off are unspecified after
 * it -- nothing at or behind out[cap] is ever touched; the copying form leaves out alone.
 * A streaming DECODE that finds more entries than ents_cap has likewise filled msgs and the
 * first ents_cap entry headers before it says so.
 */
#ifndef RAFTQ_WIRE_H
#define RAFTQ_WIRE_H

#include "raftq_step.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RAFTQ_MSG_SNAP 7 /* decoded, never accepted by Step */
/* (RAFTQ_MSG_PROP = 2, a follower forwarding a proposal to its leader: raftq_step.h -- held by raftq_step_frames, or stepped under raftq_step_set_props) */

/* raftq_wire_msg_t.flags */
#define RAFTQ_WIRE_F_MALFORMED 0x01u /* frame did not parse: every other field of the record is 0 */
#define RAFTQ_WIRE_F_SNAPSHOT 0x02u  /* a non-empty Message.snapshot was present (skipped) */
#define RAFTQ_WIRE_F_GROUP 0x04u     /* field 12 was present (absent = group 0, a stock etcd peer) */

/* One message header.  Same layout as raftq_msg_t (raftq_step.h) in the fields Step reads,
 * so a decoded array can be handed to raftq_step_submit unchanged. */
typedef struct raftq_wire_msg {
  uint64_t group;
  uint64_t term;
  uint64_t log_term;
  uint64_t index;
  uint64_t commit;
  uint64_t reject_hint;
  uint32_t from;      /* sender's peer slot */
  uint8_t type;       /* raftpb.MessageType; > 255 decodes to 255 */
  uint8_t reject;
  uint8_t to;         /* addressee's peer slot */
  uint8_t flags;      /* RAFTQ_WIRE_F_* (decode); raftq_step_frames adds RAFTQ_MSGF_* (0x10 .. 0x80) */
  uint32_t ent_first; /* this message's entries are ents[ent_first .. ent_first + n_ents) */
  uint32_t n_ents;
} raftq_wire_msg_t; /* 64 bytes */

/* One log entry.  data_off points into the payload pool (encode) or into the
 * decoded stream itself (decode: no payload byte is copied). */
typedef struct raftq_wire_ent {
  uint64_t term;
  uint64_t index;
  uint64_t data_off;
  uint32_t data_len;
  uint32_t type; /* raftpb.EntryType: 0 EntryNormal, 1 EntryConfChange */
} raftq_wire_ent_t; /* 32 bytes */

typedef struct raftq_wire_counts {
  uint64_t n_msgs;
  uint64_t n_ents;
  uint64_t n_malformed;
  uint64_t bytes; /* encoded / consumed */
} raftq_wire_counts_t;

/* Marshal n messages into rafthttp stream frames, in order.  frame_off (may be NULL) receives
 * n + 1 byte offsets into out; cap is out's size.  RAFTQ_EINVAL if cap is too small (counts->bytes
 * then says what is needed), if an entry range or payload range is out of bounds, or to/from >= 255. */
int raftq_wire_encode(raftq_t* h, const raftq_wire_msg_t* msgs, uint64_t n, const raftq_wire_ent_t* ents,
                      uint64_t n_ents, const void* pool, uint64_t pool_bytes, void* out, uint64_t cap,
                      uint64_t* frame_off /*[n+1]|NULL*/, raftq_wire_counts_t* counts /*|NULL*/);

/* Unmarshal n frames.  frame_off[i] .. frame_off[i+1] is frame i (its 8-byte length included) --
 * the receive loop knows the boundaries, it read the lengths to read the bodies.  A frame whose
 * length word disagrees with its extent, or whose body does not parse, is flagged MALFORMED and
 * counted; the call still succeeds.  ents receives the entry headers of all messages (message
 * order); RAFTQ_EINVAL if there are more than ents_cap (counts->n_ents says how many). */
int raftq_wire_decode(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off /*[n+1]*/, uint64_t n,
                      raftq_wire_msg_t* msgs /*[n]*/, raftq_wire_ent_t* ents /*[ents_cap]|NULL*/, uint64_t ents_cap,
                      raftq_wire_counts_t* counts /*|NULL*/);

/* ---- the narrow output forms of the streaming decoder ----------------------------------------------------------------
 * The 64-byte records are the largest block of bytes a decode sends over the link, and a node reads 7 of them from an
 * acknowledgement once Step has consumed the rest on the device.  The two calls below give EVERY frame a fixed-size narrow
 * record -- raftq_wire_msg40_t (RAFTQ_WIRE_FORM_40, lossless) or raftq_wire_head_t (RAFTQ_WIRE_FORM_HEAD, the routing word) --
 * and only a frame the narrow record cannot express exactly ("wide") ALSO its full raftq_wire_msg_t, compacted in frame
 * order into a second, short array wide[].
 *
 * A frame is NARROW when all of these hold:
 *   - it is malformed (the all-zero record plus RAFTQ_WIRE_F_MALFORMED: always narrow), or it parsed and
 *   - group < 2^32;
 *   - from <= 254, or from is absent (0xFFFFFFFF in the full record, written as 0xFF);
 *   - to == to_slot;
 *   - n_ents == 0;
 *   - the one of log_term / reject_hint its kind does not carry is 0: log_term for MsgAppResp, reject_hint for every other
 *     kind (evaluated after raftq_step_frames has overwritten a MsgApp's reject_hint);
 *   - RAFTQ_WIRE_FORM_HEAD only: the bit of its type is set in the caller's head_types mask (bit t = type t, t < 32) and
 *     reject == 0.  term, index, log_term, commit and reject_hint of such a frame are NOT delivered: the caller's declared
 *     choice, for the kinds whose fields it has had consumed on the device.
 * Every other frame is WIDE: its narrow record carries RAFTQ_WIRE_F_WIDE, its other fields are the full record's truncated
 * to their width, and in RAFTQ_WIRE_FORM_40 aux = k, the frame's position in wide[].  wide[] is in ascending frame order
 * in both forms, so k is also the number of WIDE records in front of this one.
 *
 * Expansion is exact: from the narrow array, wide[], to_slot and the form every 64-byte record raftq_wire_decode would have
 * written is recovered byte for byte (RAFTQ_WIRE_FORM_HEAD: in the delivered fields) -- a wide frame's from wide[k]; a narrow
 * one's as group, from (0xFF -> 0xFFFFFFFF), type, reject, flags, term, index, commit as they stand, to = to_slot,
 * ent_first = n_ents = 0, aux -> reject_hint (MsgAppResp) or log_term (every other kind), the other one 0; a malformed one's
 * as all-zero but the flags.  flags includes the SNAPSHOT and GROUP bits and Step's RAFTQ_MSGF_*; the bit RAFTQ_WIRE_F_WIDE
 * exists only in the narrow record. */
#define RAFTQ_WIRE_F_WIDE 0x08u /* narrow record: this frame's full record is in wide[] (the one flag bit that is free: 0x01-0x04 are RAFTQ_WIRE_F_*, 0x10-0x80 RAFTQ_MSGF_*) */
#define RAFTQ_WIRE_FORM_40 40   /* lossless */
#define RAFTQ_WIRE_FORM_HEAD 8  /* routing word only: for a caller that has had the fields consumed on the device */

typedef struct raftq_wire_msg40 { /* raftq_msg40_t's layout, flags in its pad byte */
  uint32_t group;
  uint8_t from; /* 0xFF = absent */
  uint8_t type;
  uint8_t reject;
  uint8_t flags; /* RAFTQ_WIRE_F_* | RAFTQ_MSGF_* */
  uint64_t term;
  uint64_t index;
  uint64_t aux; /* reject_hint on MsgAppResp, log_term on every other kind; WIDE: position in wide[] */
  uint64_t commit;
} raftq_wire_msg40_t; /* 40 bytes */
typedef struct raftq_wire_head {
  uint32_t group;
  uint8_t from;
  uint8_t type;
  uint8_t reject;
  uint8_t flags;
} raftq_wire_head_t; /* 8 bytes */

/* raftq_wire_decode with narrow records.  ents, counts and the preconditions are raftq_wire_decode's on the same input.
 * narrow: n records of `form` bytes; wide: room for wide_cap records (NULL with wide_cap = 0); *n_wide (may be NULL): how
 * many wide frames there are.  More of them than wide_cap: the narrow records and the first wide_cap wide records are
 * written, RAFTQ_EINVAL (the ents_cap rule) -- nothing at or behind wide[wide_cap] or narrow[n] is ever written.
 * Streaming form only: every array must be page-locked and 16-byte aligned, form one of the two, to_slot < 255 --
 * RAFTQ_EINVAL otherwise, before anything is enqueued.  RAFTQ_ESTATE while a Step batch is in flight on the handle (a
 * precondition plain raftq_wire_decode does not have: the call shares the in-flight batch's control words). */
int raftq_wire_decode_packed(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off /*[n+1]*/, uint64_t n,
                             int form, uint32_t head_types, uint32_t to_slot,
                             void* narrow /*[n] records of `form` bytes*/, raftq_wire_msg_t* wide /*[wide_cap]*/, uint64_t wide_cap,
                             raftq_wire_ent_t* ents /*|NULL*/, uint64_t ents_cap, raftq_wire_counts_t* counts /*|NULL*/, uint64_t* n_wide /*|NULL*/);

/* Walk the length words of a byte buffer (host side; pointer chasing, inherently serial):
 * off[0..n] for the n whole frames found.  big_endian = 1 for rafthttp streams, 0 for WAL files.
 * *n_frames = whole frames; *consumed = bytes they cover (a torn tail is left to the caller). */
int raftq_wire_scan_frames(const void* buf, uint64_t nbytes, int big_endian, uint64_t* off /*[cap+1]*/, uint64_t cap,
                           uint64_t* n_frames, uint64_t* consumed);

/* Step straight from the wire: decode on the device into the batch's message records (the 64-byte
 * records never cross PCIe), then exactly raftq_step_submit.  Frames that are malformed, or whose
 * type Step does not take, fail the batch at its collect like any malformed message.  Entry
 * headers of the batch (MsgApp) are available after the collect through raftq_step_wire_entries,
 * msgs[i].ent_first / n_ents through raftq_step_wire_msgs -- both in pinned memory, valid until
 * the next submit into that slot. */
int raftq_step_submit_wire(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off, uint64_t n);
/* Zero-copy form: the arrays the NEXT raftq_step_submit_wire will take, with room for n_cap frames and nbytes_cap stream
 * bytes -- fine-grained device memory behind a large BAR (the receive path's stores, or a NIC's, land in HBM and the
 * frames are decoded where they lie: no DMA, no copy), pinned host memory otherwise; write-only for the host either
 * way.  Fill frame_off[0..n] and the stream, pass the SAME two pointers to raftq_step_submit_wire.  The arrays belong to
 * the library from that submit until the batch is collected; asking for a slot's arrays again ends the validity of
 * raftq_step_wire_msgs / _entries for the batch that was decoded in them. */
int raftq_step_stage_wire(raftq_t* h, uint64_t n_cap, uint64_t nbytes_cap, uint64_t** frame_off, void** stream);
int raftq_step_wire_msgs(raftq_t* h, const raftq_wire_msg_t** msgs, uint64_t* n);
int raftq_step_wire_entries(raftq_t* h, const raftq_wire_ent_t** ents, uint64_t* n_ents);

/* A node's inbound half of a turn -- rafthttp's decoder, the checks a node makes on what it received, rc.node.Step for every
 * message (raft.go:268-270) -- as ONE submission with one wait: raftq_wire_decode into msgs / ents, then raftq_step_batch over
 * ALL n frames in arrival order, the decoder saying in every record's flag byte what Step is to make of it (RAFTQ_MSGF_*,
 * raftq_step.h; the handle must have opted in, raftq_step_set_msg_flags):
 *   - a frame that did not parse, is of a kind a peer never sends (anything but MsgProp, MsgApp, MsgAppResp, MsgVote,
 *     MsgVoteResp, MsgHeartbeat, MsgHeartbeatResp), names a group >= G or a sender >= N, or is addressed to a slot other than
 *     the handle's own (raftq_set_self): RAFTQ_MSGF_SKIP -> RAFTQ_OUT_SKIPPED.  rafthttp would log and drop the stream; a node
 *     has to survive whatever bytes a peer throws at it.
 *   - MsgProp (appending is the log owner's): RAFTQ_MSGF_HOLD -> RAFTQ_OUT_HELD, the group's later frames RAFTQ_OUT_DEFERRED.
 *     On a handle that opted in to raftq_step_set_props (raftq_step.h) instead: with entries RAFTQ_MSGF_ENTRIES -- Step takes it by
 *     its count, RAFTQ_OUT_PROPOSED / RAFTQ_OUT_FORWARD / RAFTQ_OUT_NONE, and holds nobody up -- and without entries
 *     RAFTQ_MSGF_SKIP, as a frame of a kind a peer never sends.
 *   - MsgTransferLeader, MsgTimeoutNow (types 13 and 14): on a handle that opted in to raftq_set_lead_transfer (raftq.h) kinds a
 *     peer sends, checked as the others are and flagged as little; without it they stay frames of a kind a peer never sends.
 *     (Likewise types 17 and 18 under raftq_set_pre_vote.)  raftq_step_frames_packed and raftq_step_submit_wire take them the same
 *     way.  No encoder builds the two kinds on the device.
 *   - MsgReadIndex, MsgReadIndexResp (types 15 and 16): on a handle that opted in to raftq_set_read_index (raftq.h, either mode)
 *     kinds a peer sends, in the same way; without it they stay frames of a kind a peer never sends.  A MsgReadIndex frame carries
 *     its context as an entry: it is a wide record in the packed form, like every frame with entries, and is flagged no differently
 *     from a MsgVote.  No encoder builds the two kinds on the device (the context bytes are host memory).
 *   - MsgApp: RAFTQ_MSGF_BARRIER, and with tail_appends != 0 RAFTQ_MSGF_ENTRIES (reject_hint, which a MsgApp does not use, is
 *     overwritten with the Term of its last entry) -- one that lands on the log's tail is RAFTQ_OUT_APPENDED.
 * Results: raftq_step_results (or _c), n records, out[i] answers frame i.  msgs / ents / counts as raftq_wire_decode, except
 * that more entries than ents_cap is NOT an error here -- the frames have been stepped; counts->n_ents says how many there
 * are, the first ents_cap are written, raftq_wire_decode fetches the rest.
 * Every array must be page-locked and 16-byte aligned (RAFTQ_EINVAL otherwise: make the two calls).  No batch may be in
 * flight.  raftq_node's turn is this call + one for what goes out. */
int raftq_step_frames(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off /*[n+1]*/, uint64_t n, int tail_appends,
                      raftq_wire_msg_t* msgs /*[n]*/, raftq_wire_ent_t* ents /*[ents_cap]|NULL*/, uint64_t ents_cap,
                      raftq_wire_counts_t* counts /*|NULL*/);

/* raftq_step_frames with narrow records (see raftq_wire_decode_packed): results, state afterwards, ents, counts and the
 * preconditions are exactly raftq_step_frames' on the same input; to_slot is the handle's own slot (raftq_set_self).  Step
 * still reads the full 64-byte records, from the decoder's copy in HBM -- what crosses the link is the narrow array and the
 * wide frames (MsgApp / MsgProp with entries, rejections in RAFTQ_WIRE_FORM_HEAD, anything odd).  More wide frames than
 * wide_cap is NOT an error here -- the frames have been stepped: *n_wide says how many there are, the first wide_cap are
 * written, raftq_wire_decode fetches the rest.  A refusal (an array not page-locked and 16-byte aligned, a bad form, an own
 * slot >= 255: RAFTQ_EINVAL; a batch in flight: RAFTQ_ESTATE) comes before anything is enqueued: nothing is applied. */
int raftq_step_frames_packed(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off /*[n+1]*/, uint64_t n, int tail_appends,
                             int form, uint32_t head_types,
                             void* narrow /*[n] records of `form` bytes*/, raftq_wire_msg_t* wide /*[wide_cap]*/, uint64_t wide_cap,
                             raftq_wire_ent_t* ents /*[ents_cap]|NULL*/, uint64_t ents_cap, raftq_wire_counts_t* counts /*|NULL*/, uint64_t* n_wide /*|NULL*/);

/* raftq_step_frames + the messages its results call for, built and marshalled on the device (raft.go:268-270 -> :227-230:
 * rc.node.Step's responses and the commit broadcast, then rc.transport.Send) -- ONE submission with one wait (a batch that stalls
 * into the sorted walk, > 32 frames of one group, waits three times: the call, the replay, the answers laid out again).  Everything the caller can see apart from `out` is what
 * raftq_step_frames gives on the same input -- records, entry headers, results, counts, the state after, the preconditions --
 * except that a result whose messages were built carries RAFTQ_OUTF_ANSWERED in its flags: the host sends nothing for it.
 * Built, for results 0 .. n-1 (every message From = self, Group = the result's; every other field zero):
 *   RAFTQ_OUT_APPENDED          MsgAppResp{Term, Index: lastnewi} to the sender
 *   RAFTQ_OUT_VOTE_RESP         MsgVoteResp{Term, Reject} to the sender
 *   RAFTQ_OUT_HEARTBEAT_RESP    MsgHeartbeatResp{Term} to the sender
 *   RAFTQ_OUT_PROGRESS + RAFTQ_OUTF_COMMITTED after a non-rejecting MsgAppResp, at_tail bit still set (bcastAppend with every
 *                               follower at the tail): N - 1 empty MsgApp{Term, Index: lastIndex, LogTerm: lastTerm, Commit},
 *                               lastIndex / lastTerm / Commit as they stand AT THAT MESSAGE
 * Everything else stays the caller's and is not flagged: RAFTQ_OUT_APPEND, RAFTQ_OUT_BECAME_LEADER (unless raftq_respond_set_lead,
 * below, opted the handle in), resends and reject backoff, HELD / DEFERRED / SKIPPED / NONE, and under raftq_step_set_props RAFTQ_OUT_PROPOSED
 * (which also clears the group's at_tail bit: no follower has the new entries before the host's bcastAppend -- unless
 * raftq_respond_set_props, below, opted the handle in) / RAFTQ_OUT_FORWARD.  A result the caller may have to answer itself (any of those that sends, a
 * MsgAppResp while the group's bit is clear) ends its group's device-answered prefix: the group's later results of the batch
 * are not answered either, so per (peer, group) the frames keep the order the host's own answers would have.
 * Under raftq_set_lead_transfer (raftq_step.h "Leadership transfer") RAFTQ_OUT_TRANSFER, a forwarded MsgTransferLeader
 * (RAFTQ_OUT_FORWARD) and a campaign from MsgTimeoutNow are the host's in the same way: no RAFTQ_OUTF_ANSWERED, and they end their
 * group's device-answered prefix.  RAFTQ_OUTF_TIMEOUT_NOW is always the host's to send; on a committing ack it does not stop the
 * commit broadcast from being built and flagged RAFTQ_OUTF_ANSWERED -- the result then carries both flags.
 * Under raftq_set_read_index (raftq_step.h "ReadIndex in Step") a device-built MsgHeartbeatResp carries Index = the heartbeat's
 * Index, the read context it echoes (with a zero context the bytes are what they were); RAFTQ_OUT_READ_INDEX,
 * RAFTQ_OUT_READ_STATE and a forwarded MsgReadIndex are the host's, as above; RAFTQ_OUTF_READ_READY on a progress result ends no
 * prefix.  In RAFTQ_READ_SAFE raftq_tick_frames and raftq_tick_elect_frames return RAFTQ_ESTATE ("read index"): their heartbeats
 * do not carry the pending context.
 * at_tail ([ceil(G / 64)] words, bit g = group g; NULL = all clear): the caller's word that it leads g and every follower's
 * Progress.Next is lastIndex + 1 now (Next is the caller's, raftq_step.h).  A wrong set bit is the caller's bug, a clear one
 * only costs speed.  The device clears g's bit from g's first message on that makes the host move a Next away from the tail:
 * a rejecting MsgAppResp with Index > Match, a MsgHeartbeatResp that leaves Match < lastIndex, a step-down.
 * out: rafthttp stream frames, peer-major -- for every peer slot p != self, ascending, the frames addressed to p in result order
 * (a broadcast puts one frame in every follower's slice).  peer_off[p] .. peer_off[p + 1] are frame indices (N + 1 words; self's
 * slice is empty, peer_off[N] = n_resp); resp_off (NULL, or room for n * (N - 1) + 1 words) gets byte offsets into out as
 * raftq_wire_encode's frame_off, entries n_resp .. n * (N - 1) all holding the total.  resp_counts: n_msgs = n_resp, bytes.
 * cap must be at least n * (N - 1) * RAFTQ_RESPOND_FRAME_MAX (the largest payload-free frame: 8-byte length, type / to / from of
 * one byte each, term / log_term / index / commit / group of ten, reject_hint 0, the empty snapshot): below it, or with any array
 * not page-locked and 16-byte aligned (at_tail, out, resp_off and peer_off included), or N < 2, RAFTQ_EINVAL before anything
 * is enqueued -- nothing is applied.  The response records are written into the encoder's input in HBM; they never exist in
 * host memory.
 *
 * Over each group's own members (raftq_bcast_set_voters(h, 1), below, on a handle with voter masks loaded): Step is the masked
 * Step's (raftq_step.h raftq_step_set_voters, whether or not that switch is on), and ONLY the commit broadcast changes -- it is
 * one empty MsgApp to every slot p != self whose bit is set in voters[g]: upstream's bcastAppend ranges over r.prs.  The
 * responses to a sender (MsgAppResp, MsgVoteResp, MsgHeartbeatResp) go to whoever sent, member or not, as upstream answers.
 * at_tail then reads "every MEMBER's Progress.Next is lastIndex + 1".  The layout stays COMPACT: peer-major, result order inside
 * a slice, fillers only behind the total; peer_off, resp_off and resp_counts keep their meaning.  A committing ack in a group
 * with no member other than self is flagged RAFTQ_OUTF_ANSWERED and builds ZERO frames -- the host would have sent to nobody
 * either.  The device-answered prefix, the clearing of at_tail bits, stalls and the replay are untouched.  With the switch on
 * and no masks loaded the call is what it always was.  RAFTQ_ESTATE, before anything is applied: voter masks loaded on a handle
 * that did not opt in with raftq_bcast_set_voters -- whatever raftq_step_set_voters and raftq_tick_set_voters say.
 *
 * becomeLeader's broadcast (raftq_respond_set_lead(h, 1), below): a RAFTQ_OUT_BECAME_LEADER inside its group's device-answered
 * prefix is answered too, with one frame for every slot p != self:
 *   MsgApp{Term, Index: lastIndex - 1, LogTerm: lastTerm as it stood BEFORE becomeLeader, Commit: committed after the message,
 *          Entries: [Entry{Type: 0, Term, Index: lastIndex, Data: nil}]}          (lastIndex = the empty entry's, the result's index)
 * -- byte for byte what raftq_wire_encode makes of the record bcastAppend builds after reset() put every Next at lastIndex.  The
 * result carries RAFTQ_OUTF_ANSWERED: the caller still appends the empty entry to its own log and WAL, sets every Next to
 * lastIndex + 1 and sends nothing.  Such a result does not end the prefix, and the broadcast leaves every follower at the tail: from
 * that message on the group counts as at the tail, whatever at_tail said and with at_tail == NULL too, until a later message clears
 * it as always (a rejection backed off for, a heartbeat response below the tail, a step-down) -- a committing ack later in the same
 * batch gets the usual empty MsgApps, behind the entry frame in every peer's slice.  A win behind a result that ended the prefix is
 * the caller's, like every other kind (the rule is stated for completeness: no sequence of frames reaches it through this call --
 * only MsgHup makes a candidate, frames carry none, and the one thing that ends a candidate's prefix, a held MsgProp, defers the
 * grant behind it).  Over members the broadcast goes to the slots of voters[g], a group with no member but self
 * is flagged and builds zero frames.  The entry headers are written into the encoder's input in HBM, one slot per result; they never
 * exist in host memory (a stalled batch's replay writes them again).  cap must then be at least n * (N - 1) *
 * RAFTQ_RESPOND_LEAD_FRAME_MAX: RAFTQ_RESPOND_FRAME_MAX plus the entries field of one empty entry at its largest -- field tag and
 * length (2), the tags of type, term and index (3), a one-byte type, term and index of ten bytes each.
 *
 * A forwarded proposal's MsgApps (raftq_respond_set_props(h, 1), below; it has an effect only where a RAFTQ_OUT_PROPOSED can arise,
 * that is under raftq_step_set_props): a RAFTQ_OUT_PROPOSED inside its group's device-answered prefix is answered on the device
 * when the group's at_tail bit is set at that message -- from the caller's bitmap, or from a device-answered becomeLeader earlier in
 * the batch.  The answer is one frame for every slot p != self:
 *   MsgApp{Term, Index: lastIndex BEFORE the proposal, LogTerm: lastTerm BEFORE the proposal, Commit: committed AFTER the message,
 *          Entries: the frame's n entries, entry k = {Type and Data as received, Term: Term, Index: old lastIndex + 1 + k}}
 * -- byte for byte what raftq_wire_encode makes of the records bcastAppend builds on the host with every Next at the old tail + 1,
 * the entries' headers the decoder's with term / index overwritten, the pool the inbound stream; an entry with data_len == 0 has no
 * Data field.  Over members the frames go to the slots of voters[g] only.  The result carries RAFTQ_OUTF_ANSWERED: the caller still
 * stores the entries in its own log and WAL, moves every Next to the new tail + 1 and sends nothing.  The at_tail bit STAYS set (the
 * optimistic state bcastAppend leaves, the assumption raftq_propose_frames states) and the prefix does not end: a second proposal of
 * the group later in the batch is answered against the new tail, a committing ack behind it gets the usual empty MsgApps with
 * Index = the new tail, behind the entry frames in every peer's slice.  A proposal that commits on its own append (a one-voter group
 * over members) carries the new commit and is answered like any other; a group with no member but self is flagged and builds zero
 * frames.  A RAFTQ_OUT_PROPOSED with the bit clear is the host's, as every proposal is without the switch: it ends the prefix and the
 * bit stays clear; so is one whose entry headers the decoder could not hand back (its range ends beyond ents_cap: the host has not got
 * them either).  RAFTQ_OUT_FORWARD stays the host's in every case.  Stalls keep their rules (the replay stamps the headers again).
 * The stamped headers and the MsgApp records are written into the encoder's input in HBM and never exist in host memory; the
 * payload bytes are gathered from the decoder's copy of the inbound stream in HBM and do not cross the link inbound a second time.
 * The call then requires, before anything is enqueued (RAFTQ_EINVAL, nothing applied): ents != NULL (the device stamps the
 * decoder's headers) and
 *   cap >= n * (N - 1) * FRAME + (N - 1) * (nbytes + ents_cap * RAFTQ_RESPOND_ENT_MAX)
 * with FRAME = RAFTQ_RESPOND_LEAD_FRAME_MAX under raftq_respond_set_lead and RAFTQ_RESPOND_FRAME_MAX otherwise (the bound must
 * stay within 2^31 bytes).  Every payload lies inside the stream, so the payloads of one peer's slice sum to at most nbytes;
 * RAFTQ_RESPOND_ENT_MAX is the most one entry adds beyond its payload, from the marshal's entry_size(): the entries field's tag and
 * length (1 + 5: the length of an entry whose data_len fits 32 bits takes five bytes at most), the tags of type / term / index /
 * data (4), a five-byte type (a 32-bit varint), term and index of ten bytes each, a five-byte data length: 6 + 4 + 5 + 20 + 5 = 40. */
#define RAFTQ_RESPOND_ENT_MAX 40u
#define RAFTQ_OUTF_ANSWERED 0x10u /* result flag: the messages this result calls for are in `out` (built on the device) */
#define RAFTQ_RESPOND_FRAME_MAX 83u
#define RAFTQ_RESPOND_LEAD_FRAME_MAX 109u /* = RAFTQ_RESPOND_FRAME_MAX + 26 */
int raftq_step_frames_respond(raftq_t* h, const void* stream, uint64_t nbytes, const uint64_t* frame_off /*[n+1]*/, uint64_t n, int tail_appends,
                              raftq_wire_msg_t* msgs /*[n]*/, raftq_wire_ent_t* ents /*[ents_cap]|NULL*/, uint64_t ents_cap,
                              const uint64_t* at_tail /*[ceil(G/64)] bitmap | NULL*/, void* out, uint64_t cap,
                              uint64_t* resp_off /*[n*(N-1)+1] | NULL*/, uint64_t* peer_off /*[N+1]*/,
                              raftq_wire_counts_t* counts /*inbound, as raftq_step_frames | NULL*/, raftq_wire_counts_t* resp_counts /*| NULL*/);

/* A node's OUTBOUND half of a turn for what it was asked to propose (round 6; raft.go:211-215 -> :227-230: rc.node.Propose ->
 * appendEntry -> bcastAppend -> rc.transport.Send) as ONE submission with one wait: for every record of props[] the leader's
 * appendEntry (lastIndex += n_ents, lastTerm = Term, its own Progress.Match) on the device-resident state, and bcastAppend --
 * the N - 1 MsgApp{Term, LogTerm: old lastTerm, Index: old lastIndex, Commit, Entries} headers and their entry headers are
 * written INTO THE ENCODER'S INPUT IN HBM (they never exist in host memory); then raftq_wire_encode over msgs[] (what the
 * caller queued itself this turn: responses, resends, heartbeats) followed by those MsgApps.  What the host keeps of a
 * proposal is its payload bytes (in `pool`, where data_off points) and its own log.
 *
 * props[i]: a group THIS handle's node leads (role == leader; anything else fails the call), at most once per call, with
 * every follower's Progress.Next at the log's tail -- the state bcastAppend leaves behind, i.e. every group outside a
 * catch-up; the caller, who owns Progress.Next (raftq_step.h), sends the others itself -- and 1 <= n_ents entries
 * prop_ents[ent_first .. ent_first + n_ents) in log order (every record of prop_ents[] must name a payload inside the pool).  The new entries get Term = the group's Term, Index = old lastIndex
 * + 1 + k.  The handle needs more than one peer (with one the append commits: raftq_apply_log_deltas reports that).
 *
 * The stream: the frames of msgs[0 .. n_msgs), then for every peer slot p != self, ascending, the n_props MsgApps addressed to
 * p in props[] order -- frame_off (may be NULL) gets n_msgs + (N - 1) * n_props + 1 offsets; peer p's MsgApps are ONE slice.
 * Byte for byte what raftq_wire_encode makes of the same messages built on the host (tests/test_wire_gpu.py::
 * test_propose_frames_*).  Every array must be page-locked and 16-byte aligned (RAFTQ_EINVAL otherwise), no Step batch may be
 * in flight.  A call that fails has applied nothing (a validation kernel runs first, and appendEntry's stores run behind the
 * marshal, once its verdict is in): a record refused, a message of msgs[] the marshal refuses (to / from >= 255, an entry range
 * outside ents[], a payload outside the pool) and an `out` that is too small all leave the handle as it was.  In the last case
 * counts->bytes is the size the stream needs, and the same call with cap >= counts->bytes appends once and succeeds -- cap ==
 * counts->bytes exactly included.  `out` and frame_off are unspecified after a refusal, as with the streaming raftq_wire_encode
 * (nothing is written at or behind out[cap], nor behind frame_off's n_msgs + (N - 1) * n_props + 1 words).  raftq_node's turn is
 * raftq_step_frames + this.
 *
 * Over each group's own members (raftq_bcast_set_voters(h, 1), below, on a handle with voter masks loaded): bcastAppend ranges
 * over r.prs -- of the N - 1 MsgApps of a record only those to a slot p whose bit is set in voters[g] exist.  The layout stays
 * POSITIONAL, as raftq_tick_frames': (N - 1) runs of n_props slots where they always were, frame_off keeps its n_msgs +
 * (N - 1) * n_props + 1 entries, and the slot of a peer that is no member of its group is a frame of ZERO length, frame_off[k + 1]
 * == frame_off[k].  The bytes are what raftq_wire_encode makes of msgs[] and the member MsgApps alone.  counts->n_msgs is n_msgs
 * plus the number of frames that have bytes; the entry headers are written for every record.  The state changes are what they
 * always were.  Two more records fail the call, nothing applied, as the others do:
 *   - this node is no member of its group: self's bit is clear in voters[g].  (Upstream v2.2 would dereference a missing
 *     Progress.  CHOICE: refuse.)
 *   - its append would move the commit index.  Without masks maybeCommit cannot move on an append -- the leader's own Match is the
 *     largest, the quorum-th largest is somebody else's.  Over members it can: a ONE-VOTER group commits on its own append, and
 *     under the 2015-era removeNode, which does not call maybeCommit, so does a group whose membership SHRANK since its last
 *     acknowledgement (N = 5, Match 10, 8, 5, 5, 5, committed 5, voters {0, 1, 2}: the append commits 8).  Evaluated exactly: with
 *     Match[self] raised to lastIndex + n_ents, the masked maybeCommit including the current-term gate would return true.  This
 *     call has no channel for a commit; raftq_apply_log_deltas has.  The recipe: a caller that loaded the masks knows its
 *     one-voter groups and appends for them with raftq_apply_log_deltas; after a voter delta that shrinks a led group, a tail
 *     report with the UNCHANGED tail runs maybeCommit over the new membership and reports the commit.  Once the commit is
 *     settled maybeCommit cannot move on an append -- self is a voter and holds the largest Match -- and the proposal passes.
 * RAFTQ_ESTATE, before anything is applied: voter masks loaded on a handle that did not opt in with raftq_bcast_set_voters --
 * whatever raftq_step_set_voters and raftq_tick_set_voters say.
 *
 * A follower's proposals (raftq_propose_set_forward(h, 1), below): the reference calls node.Propose on whatever node the client
 * reached (raft.go:211-215), and on a node that does not lead the group etcd's stepFollower turns the proposal into a MsgProp frame
 * to the leader -- `m.To = r.lead; r.send(m)`.  With the switch on, "anything else fails the call" above no longer holds: record i,
 * naming group g, is judged on the state as it stands at the call (nothing is in flight) --
 *   - role == leader: exactly the above -- appendEntry, the N - 1 MsgApps, the store behind the marshal.  RAFTQ_PROP_APPENDED.
 *   - role == follower, lead != 0 and lead - 1 != self: ONE frame,
 *       MsgProp{To: lead - 1, From: self, Group: g, Term: 0, Entries: the record's n_ents entries}
 *     (raft.send leaves a MsgProp's Term alone, so it is 0), entry k = {Type: prop_ents.type, Term: 0, Index: 0, Data}; an entry
 *     with data_len == 0 has no Data field; every other field is zero -- byte for byte what raftq_wire_encode makes of the record
 *     raftq_node's handle_proposal builds on the host.  Nothing of the group's state changes.  RAFTQ_PROP_FORWARDED.
 *   - a candidate, a follower with lead == 0, or a follower whose lead - 1 == self: no frame, no state change (upstream logs
 *     "no leader; dropping proposal").  The last is a loaded state upstream cannot reach; CHOICE: dropped, as handle_proposal
 *     does.  RAFTQ_PROP_DROPPED.
 * One call may mix all three.  Every other refusal stays and applies to every record whatever its role: a group out of range, 0
 * entries or more than 1024, an entry range outside prop_ents[], a payload outside the pool, a group named twice, N < 2, arrays not
 * page-locked and 16-byte aligned.  A refused call applies nothing, for forwarded and dropped records as for the leaders'.
 * The layout stays POSITIONAL, as it is over members: (N - 1) runs of n_props slots behind msgs[], frame_off keeps its n_msgs +
 * (N - 1) * n_props + 1 entries; a forwarded record has bytes only in the run of its leader's slot, its other slots and every slot
 * of a dropped record are frames of ZERO length.  The entry headers are written for every record.  counts->n_msgs is n_msgs plus
 * the frames that have bytes; counts->bytes and the "out is too small" retry keep their meaning.  A call whose records were all
 * dropped succeeds with no frame of its own.  Over members (raftq_bcast_set_voters with masks loaded) a forward goes to lead
 * whether or not lead or self is a member of the group -- upstream's send consults no prs -- and the two member refusals are judged
 * for leader records only.  What became of each record: raftq_propose_outcomes, below. */
typedef struct raftq_prop {
  uint64_t group;
  uint32_t ent_first; /* into prop_ents[] */
  uint32_t n_ents;    /* >= 1 */
} raftq_prop_t; /* 16 bytes */
typedef struct raftq_prop_ent {
  uint64_t data_off; /* byte offset of Entry.Data in pool; ignored when data_len == 0 */
  uint32_t data_len;
  uint32_t type; /* raftpb.EntryType */
} raftq_prop_ent_t; /* 16 bytes */
int raftq_propose_frames(raftq_t* h, const raftq_prop_t* props, uint64_t n_props, const raftq_prop_ent_t* prop_ents, uint64_t n_prop_ents,
                         const raftq_wire_msg_t* msgs, uint64_t n_msgs, const raftq_wire_ent_t* ents, uint64_t n_ents, const void* pool,
                         uint64_t pool_bytes, void* out, uint64_t cap, uint64_t* frame_off /*[n_msgs + (N-1) n_props + 1]|NULL*/,
                         raftq_wire_counts_t* counts /*|NULL*/);

/* The switch of the two calls above: raftq_step_frames_respond's commit broadcast and raftq_propose_frames' bcastAppend over each
 * group's own members ("per-group voter sets", raftq.h).  0, the default: both calls refuse a handle with voter masks loaded
 * (RAFTQ_ESTATE, "voter masks" in the text), whatever raftq_step_set_voters and raftq_tick_set_voters say.  1: both run over
 * voters[g], as their paragraphs "Over each group's own members" say.  Anything but 0 or 1 is RAFTQ_EINVAL; the handle must be
 * idle (RAFTQ_ESTATE with a Step batch in flight); a NULL handle returns an error without touching a device.  A property of the
 * handle, like the other two switches: raftq_clone_state does not copy it and raftq_load_voters(h, NULL) does not clear it; with
 * no masks loaded the handle launches exactly the kernels it always did, whatever the switch says.  Independent of
 * raftq_tick_set_voters and of raftq_step_set_voters: raftq_step_frames_respond with this switch on runs the masked Step on its
 * own authority, as raftq_tick_elect_frames does.  With all three switches on every frame a node builds on the device goes to a
 * group's members; what remains of conf changes is host work (ConfChange entries through raftq_node: not built). */
int raftq_bcast_set_voters(raftq_t* h, int on);

/* raftq_propose_frames for a node that does not lead every group it is asked about ("A follower's proposals" in that call's
 * paragraph).  0, the default: a record whose group this node does not lead fails the call ("this node does not lead its group") --
 * the call launches the kernels it launches without the switch, writes the same bytes and fails on the same records with the same
 * text.  1: such a record becomes a MsgProp frame to the group's leader, or is dropped where no leader is known.  Anything but 0 or
 * 1 is RAFTQ_EINVAL; the handle must be idle (RAFTQ_ESTATE with a Step batch in flight); a NULL handle returns an error without
 * touching a device.  A property of the handle, like the other switches: raftq_clone_state does not copy it.  Only
 * raftq_propose_frames reads it.  Independent of raftq_bcast_set_voters.  raftq_node does not turn it on: its handle_proposal still
 * builds a follower's MsgProp on the host.  (RAFTQ_OUT_FORWARD of raftq_step_frames_respond -- a follower handing on a MsgProp it
 * RECEIVED, after a change of leader -- stays the host's too.) */
int raftq_propose_set_forward(raftq_t* h, int on);

/* What became of every record of the last raftq_propose_frames call that SUCCEEDED with raftq_propose_set_forward on: *n =
 * n_props, (*what)[i] = RAFTQ_PROP_* of props[i].  The bytes live in page-locked memory the handle owns and are valid until the
 * next call on the handle; they leave the device in the call's own submission under its single wait, packed by the wave (eight
 * outcomes a store), not a byte a lane.  With the switch off, after a call that failed or was given no record, or before any such
 * call: *n = 0 and *what = NULL.  A NULL handle returns an error without touching a device. */
#define RAFTQ_PROP_APPENDED 0  /* this node leads the group: appended, N - 1 MsgApps (over members: one per member) */
#define RAFTQ_PROP_FORWARDED 1 /* a follower that knows its leader: one MsgProp frame in the leader's run */
#define RAFTQ_PROP_DROPPED 2   /* no leader known: no frame, nothing changed */
int raftq_propose_outcomes(raftq_t* h, const uint8_t** what, uint64_t* n);

/* raftq_step_frames_respond's fifth kind: becomeLeader's broadcast ("becomeLeader's broadcast" in that call's paragraph).  0, the
 * default: RAFTQ_OUT_BECAME_LEADER stays the caller's and ends its group's prefix -- the call launches the kernels it always did and
 * writes the bytes and flags it always did, under the cap rule it always had.  1: the win is answered on the device and cap must be
 * at least n * (N - 1) * RAFTQ_RESPOND_LEAD_FRAME_MAX (below it: RAFTQ_EINVAL before anything is enqueued, nothing applied).
 * Anything but 0 or 1 is RAFTQ_EINVAL; the handle must be idle (RAFTQ_ESTATE with a Step batch in flight); a NULL handle returns
 * an error without touching a device.  A property of the handle, like the other switches: raftq_clone_state does not copy it.  Only
 * raftq_step_frames_respond reads it: raftq_step_frames, raftq_tick_elect_frames (whose one-voter win has nobody to send to) and
 * raftq_node's turns are what they were.  Under raftq_set_check_quorum the answered win is a reset() like any other: the group's
 * activity word is 0 behind it, and an acknowledgement later in the batch sets its sender's bit alone. */
int raftq_respond_set_lead(raftq_t* h, int on);

/* raftq_step_frames_respond's sixth kind: a forwarded proposal's MsgApps ("A forwarded proposal's MsgApps" in that call's
 * paragraph).  0, the default: RAFTQ_OUT_PROPOSED stays the caller's, clears its group's at_tail bit and ends its prefix -- the call
 * launches the kernels it launches without the switch and writes the bytes and flags it writes without it, under the same cap rule.
 * 1: a proposal of a group at the tail is answered on the device; the call needs ents and the larger cap of its paragraph (RAFTQ_EINVAL
 * before anything is enqueued otherwise, nothing applied).  Anything but 0 or 1 is RAFTQ_EINVAL; the handle must be idle
 * (RAFTQ_ESTATE with a Step batch in flight); a NULL handle returns an error without touching a device.  A property of the handle,
 * like the other switches: raftq_clone_state does not copy it.  Only raftq_step_frames_respond reads it, and it has an effect only
 * with raftq_step_set_props on (no RAFTQ_OUT_PROPOSED arises otherwise).  Independent of raftq_respond_set_lead and
 * raftq_bcast_set_voters: all eight combinations work.  Under raftq_set_check_quorum a MsgVote that the lease ignores builds no
 * frame and does not end its group's prefix: the proposal and the committing acknowledgement behind it are still answered on the
 * device.  raftq_node does not turn it on. */
int raftq_respond_set_props(raftq_t* h, int on);

/* A node's heartbeat round (raft.go:223-224 -> :230: rc.node.Tick() -> tickHeartbeat -> Step(MsgBeat) -> bcastHeartbeat ->
 * rc.transport.Send) as ONE submission with one wait: the Tick, its lists, and the heartbeats the Tick calls for, built and
 * marshalled on the device.
 *
 * The Tick is exactly raftq_tick_collect_lists(h, flags, hup_cap, beat_cap, n_hup, n_beat) (raftq.h): the timers, the action bytes,
 * the counts -- *n_hup and *n_beat are the totals -- and what raftq_last_tick_lists hands out afterwards, the MsgHup ids and the
 * MsgBeat ids or, with RAFTQ_TICK_BEAT_BITMAP, the bitmap.
 *
 * The heartbeats: let n_built = min(*n_beat, beat_cap) -- beat_cap counts here with the bitmap flag too, as the bound on what
 * is built.  For each of the first n_built MsgBeat groups g, ascending, and every peer slot p != self (raftq_set_self), one frame
 *   MsgHeartbeat{to = p, from = self, group = g, term = Term(g), commit = min(match[p][g], committed(g))}, every other field zero
 * -- etcd's bcastHeartbeat / sendHeartbeat, `commit := min(r.prs[to].Match, r.raftLog.committed)` -- from the group's state as it
 * stands after this Tick (Step(MsgBeat) changes none of it).  Groups beyond beat_cap are the caller's: it finds them in the
 * bitmap or the list and sends for them itself.
 *
 * out: rafthttp stream frames, peer-major -- for every p != self, ascending, the n_built frames to p in ascending group order.
 * peer_off[p] .. peer_off[p + 1] are frame indices (N + 1 words; self's slice is empty, peer_off[N] = n_built * (N - 1));
 * frame_off (NULL, or room for beat_cap * (N - 1) + 1 words) gets byte offsets into out as raftq_wire_encode's, the entries past
 * the last frame all holding the total.  counts: n_msgs = n_built * (N - 1), bytes.  Byte for byte what raftq_wire_encode makes
 * of the same raftq_wire_msg_t records built on the host; the records are written into the encoder's input in HBM and never exist
 * in host memory.
 *
 * Over each group's own members (raftq_tick_set_voters(h, 1), raftq.h "batched Tick", on a handle with voter masks loaded): the
 * Tick applies promotable(), and of the frames above only those to a slot p whose bit is set in voters[g] exist -- upstream's
 * bcastHeartbeat ranges over r.prs.  The layout stays POSITIONAL: peer_off is exactly what it is without masks, n_built slots per
 * slice, frame_off keeps its beat_cap * (N - 1) + 1 entries, and the slot of a peer that is no member of its group is a frame of
 * ZERO length, frame_off[k + 1] == frame_off[k].  Peer p's bytes are out[frame_off[peer_off[p]] .. frame_off[peer_off[p + 1]]):
 * what raftq_wire_encode makes of the member records alone, in group order.  counts->n_msgs is the number of frames that have
 * bytes.  Whether self is a member is not asked: a leader whose own bit is clear still beats its members.  A built group with an
 * empty mask gives no frame.  With the switch on and no masks loaded the call is what it always was.
 *
 * Under raftq_set_check_quorum (raftq.h "CheckQuorum") the call is RAFTQ_ESTATE ("check quorum" in the text) unless
 * raftq_tick_set_checks(h, chk_cap > 0) opened it.  Then the Tick is the switch's: a leader group whose check failed has action 3, is
 * no MsgBeat group of this Tick -- not in *n_beat, the list or the bitmap -- and gets no frame; the groups whose check failed are
 * raftq_last_tick_checks' list, under the same wait.
 *
 * Refused before anything is enqueued -- a refused call has not ticked:
 *   RAFTQ_EINVAL  cap < beat_cap * (N - 1) * RAFTQ_RESPOND_FRAME_MAX (the largest payload-free frame, above);
 *                 out, frame_off or peer_off not page-locked and 16-byte aligned; N < 2; an unknown flag;
 *                 beat_cap * (N - 1) >= 2^31, or beat_cap * (N - 1) * RAFTQ_RESPOND_FRAME_MAX beyond 2^31 bytes
 *   RAFTQ_ESTATE  a Step batch in flight; no node state on the handle (neither raftq_set_self nor raftq_load_node was ever
 *                 called); voter masks loaded on a handle that did not opt in with raftq_tick_set_voters (the round would go to
 *                 every slot, not to the group's own membership -- whatever raftq_step_set_voters says: that switch opens
 *                 raftq_step_submit_wire, raftq_step_frames and raftq_step_frames_packed to a masked handle, not
 *                 raftq_step_frames_respond, raftq_propose_frames, raftq_tick_frames or raftq_tick_elect_frames)
 * Every allocation is made before the tick kernel is enqueued (the rule raftq_tick_collect_lists follows). */
int raftq_tick_frames(raftq_t* h, unsigned flags, uint64_t hup_cap, uint64_t beat_cap, uint64_t* n_hup, uint64_t* n_beat,
                      void* out, uint64_t cap, uint64_t* frame_off /*[beat_cap*(N-1)+1] | NULL*/, uint64_t* peer_off /*[N+1]*/,
                      raftq_wire_counts_t* counts /*| NULL*/);

/* raftq_tick_frames plus a node's election round (raft.go:223-224 -> :230: rc.node.Tick() -> tickElection -> Step(MsgHup) ->
 * campaign() -> N - 1 MsgVote -> rc.transport.Send), still ONE submission with one wait: the Tick, its lists, the heartbeats and
 * the campaigns the Tick calls for, applied, built and marshalled on the device.
 *
 * The Tick is exactly raftq_tick_collect_lists(h, flags, hup_cap, beat_cap, n_hup, n_beat): the timers, the action bytes, the
 * totals, and what raftq_last_tick_lists hands out afterwards.
 *
 * The heartbeats are exactly raftq_tick_frames' for the first n_bb = min(*n_beat, beat_cap) MsgBeat groups.
 *
 * The campaigns: let n_vb = min(*n_hup, hup_cap) -- hup_cap bounds the list and what is campaigned.  For each of the first n_vb
 * MsgHup groups, ascending, the device applies Step(MsgHup) to the device-resident state; the result is what raftq_step_batch
 * would leave had that local message been stepped at this point, in the record AND the dense arrays: term + 1, vote = self, role =
 * candidate, lead = None, first_idx = 0, elapsed = 0, reset()'s match rows (self = lastIndex, the others 0), the vote word cleared
 * and self's grant recorded, the self-max word cleared if the store breaks it.  camp[r] answers hup id r of the list: the 32-byte
 * record raftq_step_set_compact(h, 2) would give for that message -- type = RAFTQ_OUT_CAMPAIGN, index = lastIndex, commit = the
 * candidate's lastTerm, flags = RAFTQ_OUTF_HARDSTATE | RAFTQ_OUTF_ANSWERED -- whatever result format the handle is set to.  The
 * caller persists the HardState and sends nothing.  MsgHup groups of rank >= hup_cap are the caller's: nothing of them is
 * touched, and the caller steps their MsgHup itself.
 *
 * out: two sections of rafthttp stream frames, back to back.  The heartbeat section is exactly raftq_tick_frames'.  The vote
 * section follows: for every peer slot p != self, ascending, one frame per campaigned group in ascending group order,
 *   MsgVote{to = p, from = self, group, term = the new Term, index = lastIndex, log_term = lastTerm}, every other field zero.
 * Frames are numbered through both sections.  peer_off[0 .. N] are the heartbeat section's frame indices as raftq_tick_frames
 * gives them; peer_off[N + 1 .. 2 N + 1] are the vote section's, the first n_bb * (N - 1), the last (n_bb + n_vb) * (N - 1).
 * frame_off (NULL, or room for (beat_cap + hup_cap) * (N - 1) + 1 words) is as raftq_wire_encode's, the entries past the last
 * frame all holding the total.  counts: n_msgs = (n_bb + n_vb) * (N - 1), bytes.  Byte for byte what raftq_wire_encode makes of
 * the same raftq_wire_msg_t records built on the host.
 *
 * Over each group's own voters (raftq_tick_set_voters(h, 1) on a handle with voter masks loaded): the Tick applies promotable(),
 * so self votes in every MsgHup group; the heartbeat section is raftq_tick_frames' over members; and Step(MsgHup) is the masked
 * Step's (raftq_step.h raftq_step_set_voters, whether or not that switch is on), with its two arms:
 *   self is the group's ONLY voter (the own grant is the quorum): the group becomes leader at once.  camp[r] is Step's record
 *     for that message -- type = RAFTQ_OUT_BECAME_LEADER, index = the empty entry's, commit = the commit index (a one-voter
 *     group commits its own append: RAFTQ_OUTF_COMMITTED), RAFTQ_OUTF_HARDSTATE and NOT RAFTQ_OUTF_ANSWERED: the caller
 *     appends the empty entry as it does after Step.  Nobody is asked for a vote: every vote slot of the group has zero length.
 *   otherwise: RAFTQ_OUT_CAMPAIGN exactly as above, and a MsgVote to every member p != self -- upstream's campaign ranges over
 *     r.prs; the slots of the other peers have zero length.
 * Both sections stay positional, as raftq_tick_frames says: peer_off[0 .. 2 N + 1] is what it is without masks, frame_off keeps
 * (beat_cap + hup_cap) * (N - 1) + 1 entries, counts->n_msgs is the number of frames that have bytes.
 *
 * Under raftq_set_check_quorum and raftq_set_pre_vote (raftq.h) the call is RAFTQ_ESTATE ("pre vote", else "check quorum" in the text)
 * unless raftq_tick_set_checks(h, chk_cap > 0) opened it.  Then the Tick and the heartbeat section are raftq_tick_frames' under that
 * switch, and Step(MsgHup) is Step's with the switches on (raftq_step.h "CheckQuorum in Step", "PreVote in Step") -- the device calls
 * the arm the walks call:
 *   raftq_set_pre_vote off: the campaign above; its reset() also zeroes the group's activity word.  Over masks a one-voter group
 *     wins at once, as above.
 *   raftq_set_pre_vote on: becomePreCandidate -- role 3, lead = None, elapsed = 0, the vote word cleared and self's grant recorded;
 *     term, vote, the Match rows, the gate and the activity word do not move.  camp[r] is the 32-byte RAFTQ_OUT_PRE_CAMPAIGN record
 *     (index = lastIndex, commit = lastTerm, no RAFTQ_OUTF_HARDSTATE) with RAFTQ_OUTF_ANSWERED, and the vote section holds
 *     MsgPreVote{type 17, term = Term + 1, index = lastIndex, log_term = lastTerm} to every peer slot p != self, or to every member
 *     p != self over masks.  A group whose own grant is the quorum (one voter, over masks) goes straight on to the real campaign
 *     and the win: RAFTQ_OUT_BECAME_LEADER without RAFTQ_OUTF_ANSWERED and no frame, as above.
 *
 * Refused before anything is enqueued -- a refused call has neither ticked nor campaigned:
 *   RAFTQ_EINVAL  cap < (beat_cap + hup_cap) * (N - 1) * RAFTQ_RESPOND_FRAME_MAX; camp, out, frame_off or peer_off not page-locked
 *                 and 16-byte aligned (camp may be NULL only when hup_cap == 0); N < 2; an unknown flag;
 *                 (beat_cap + hup_cap) * (N - 1) >= 2^31, or that many frames beyond 2^31 bytes
 *   RAFTQ_ESTATE  a Step batch in flight; no node state on the handle; voter masks loaded on a handle that did not opt in with
 *                 raftq_tick_set_voters
 * Every allocation is made before the tick kernel is enqueued.  With hup_cap == 0 the call is raftq_tick_frames. */
int raftq_tick_elect_frames(raftq_t* h, unsigned flags, uint64_t hup_cap, uint64_t beat_cap, uint64_t* n_hup, uint64_t* n_beat,
                            raftq_step_out_s_t* camp /*[hup_cap]*/, void* out, uint64_t cap,
                            uint64_t* frame_off /*[(beat_cap + hup_cap)*(N-1)+1] | NULL*/, uint64_t* peer_off /*[2*(N+1)]*/,
                            raftq_wire_counts_t* counts /*| NULL*/);

/* ---- WAL ------------------------------------------------------------------------------------ */

/* walpb record types (wal/wal.go) */
#define RAFTQ_WAL_METADATA 1
#define RAFTQ_WAL_ENTRY 2
#define RAFTQ_WAL_STATE 3
#define RAFTQ_WAL_CRC 4
#define RAFTQ_WAL_SNAPSHOT 5

#define RAFTQ_WAL_F_MALFORMED 0x01u /* record or its Data did not parse */
#define RAFTQ_WAL_F_BADCRC 0x02u    /* Record.crc is not the running CRC (wal.ErrCRCMismatch) */
#define RAFTQ_WAL_F_GROUP 0x04u     /* the group extension field was present */

/* One WAL record:
 *   ENTRY     Data = Entry{Type: entry_type, Term: term, Index: index, Data: pool[data_off, +data_len), group}
 *   STATE     Data = HardState{term, vote (raft ID, 0 = None), commit = index, group}
 *   SNAPSHOT  Data = walpb.Snapshot{index, term}
 *   METADATA  Data = pool[data_off, +data_len) verbatim
 *   CRC       no Data; Record.crc = the running CRC (wal.saveCrc at the head of a segment) */
typedef struct raftq_wal_rec {
  uint64_t group;
  uint64_t term;
  uint64_t index;
  uint64_t data_off;
  uint32_t data_len;
  uint32_t vote;
  uint32_t crc;       /* decode: Record.crc as stored */
  uint8_t kind;       /* RAFTQ_WAL_* */
  uint8_t entry_type;
  uint8_t flags;      /* RAFTQ_WAL_F_* (decode) */
  uint8_t _pad;
} raftq_wal_rec_t; /* 48 bytes */

typedef struct raftq_wal_counts {
  uint64_t n_recs;
  uint64_t n_valid;  /* decode: records before the first malformed / CRC-mismatching one */
  uint64_t bytes;
  uint32_t last_crc; /* running CRC after the last (valid) record: prev_crc of the next batch */
  uint32_t _pad;
} raftq_wal_counts_t;

/* wal.Save for a batch: n records -> WAL frames appended to a segment whose running CRC is
 * prev_crc (0 for a new file, whose first record must then be a CRC record).  Records are
 * written in order; every record's crc continues the chain. */
int raftq_wal_encode(raftq_t* h, const raftq_wal_rec_t* recs, uint64_t n, const void* pool, uint64_t pool_bytes,
                     uint32_t prev_crc, void* out, uint64_t cap, uint64_t* frame_off /*[n+1]|NULL*/,
                     raftq_wal_counts_t* counts /*|NULL*/);

/* raftq_wal_encode in two halves, so that a turn's two encodes are ONE submission: _begin enqueues the encode on the handle's
 * stream and returns without waiting (page-locked buffers only: RAFTQ_EINVAL otherwise); the wait of whatever is called next
 * on the handle -- raftq_wire_encode in a node's turn -- covers it; _end reports what raftq_wal_encode would have (and waits
 * itself if nothing has).  out / frame_off are not to be read, nor recs / pool reused, before _end.  One at a time. */
int raftq_wal_encode_begin(raftq_t* h, const raftq_wal_rec_t* recs, uint64_t n, const void* pool, uint64_t pool_bytes,
                           uint32_t prev_crc, void* out, uint64_t cap, uint64_t* frame_off /*[n+1]|NULL*/);
int raftq_wal_encode_end(raftq_t* h, raftq_wal_counts_t* counts /*|NULL*/);

/* w.ReadAll for a batch of frames (boundaries from raftq_wire_scan_frames, big_endian = 0):
 * parse every record, recompute the CRC chain from prev_crc and compare.  As ReadAll, a CRC
 * record re-seeds the chain (and must equal the running value unless that is 0).
 * counts->n_valid = index of the first bad record (n if none); records from there on still
 * carry their parsed fields and flags, the caller decides (the reference log.Fatalf's, raft.go:126). */
int raftq_wal_decode(raftq_t* h, const void* bytes, uint64_t nbytes, const uint64_t* frame_off /*[n+1]*/, uint64_t n,
                     uint32_t prev_crc, raftq_wal_rec_t* recs /*[n]*/, raftq_wal_counts_t* counts /*|NULL*/);

#ifdef __cplusplus
}
#endif
#endif /* RAFTQ_WIRE_H */
