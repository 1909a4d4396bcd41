/*
 * raftq_step.h -- C-ABI of the batched raft `Step`.
 *
 * The reference hands every inbound peer message to the consensus core one at
 * a time:  raftNode.Process -> rc.node.Step(ctx, m)   (raft.go:268-270), and
 * drives the local timers through rc.node.Tick() (raft.go:223-224).  With G
 * groups per process that is G goroutine sets and one channel hand-off per
 * message.  raftq_step_batch() is the vectorised replacement: one call takes
 * a batch of messages addressed to any of the handle's G groups, applies
 * etcd's raft.Step / stepLeader / stepCandidate / stepFollower to the
 * device-resident group state, and returns one result record per message.
 *
 * What lives on the device (per group): Term, Vote, lead, role, the election
 * clock (shared with raftq_tick), raftLog.committed / lastIndex / lastTerm,
 * every peer's Progress.Match, the candidate's vote map and the compact
 * current-term gate.  What stays with the caller: the log entries themselves
 * (so MsgSnap is refused and MsgApp is processed as a header: the term /
 * leader / clock handling happens here, raftLog.maybeAppend runs on the
 * caller's log and is reported back with raftq_apply_log_deltas), and the
 * replication flow control (Progress.Next / probe / replicate / inflights),
 * which decides what to send, not what is committed.  A forwarded proposal
 * (MsgProp) moves the state by its number of entries alone: Step takes it once
 * the handle opted in (raftq_step_set_props below) -- the leader's appendEntry
 * bookkeeping happens here, storing the entries and bcastAppend stay the
 * caller's -- and refuses it as an unknown kind otherwise.
 *
 * Ordering: messages of one group are applied in batch order, exactly as if
 * Step had been called for them one after another; messages of different
 * groups are independent (raft groups share nothing).
 *
 * The arithmetic restated here lives in the un-vendored dependency
 * github.com/coreos/etcd/raft (2015-era API): PARITY
 * UNPINNED; the checker is oracle/raftq_step_oracle.c.
 */
#ifndef RAFTQ_STEP_H
#define RAFTQ_STEP_H

#include "raftq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* raftpb.MessageType values of the message kinds Step accepts */
#define RAFTQ_MSG_HUP 0            /* local: election timer fired (raftq_tick's MsgHup) */
#define RAFTQ_MSG_BEAT 1           /* local: heartbeat timer fired (raftq_tick's MsgBeat) */
#define RAFTQ_MSG_PROP 2           /* a follower's forwarded proposal: only under raftq_step_set_props, by its entry count */
#define RAFTQ_MSG_APP 3            /* header only (see above) */
#define RAFTQ_MSG_APP_RESP 4
#define RAFTQ_MSG_VOTE 5
#define RAFTQ_MSG_VOTE_RESP 6
#define RAFTQ_MSG_HEARTBEAT 8
#define RAFTQ_MSG_HEARTBEAT_RESP 9
#define RAFTQ_MSG_CHECK_QUORUM 12  /* local: the leader's check fell due and failed in raftq_tick (raftq_collect_checks); only under
                                    * raftq_set_check_quorum, see "CheckQuorum" below */
#define RAFTQ_MSG_TRANSFER_LEADER 13 /* raftpb values; only under raftq_set_lead_transfer, see "Leadership transfer" below */
#define RAFTQ_MSG_TIMEOUT_NOW 14
#define RAFTQ_MSG_READ_INDEX 15      /* raftpb values; only under raftq_set_read_index, see "ReadIndex in Step" below */
#define RAFTQ_MSG_READ_INDEX_RESP 16
#define RAFTQ_MSG_PRE_VOTE 17      /* raftpb values; only under raftq_set_pre_vote, see "PreVote" below */
#define RAFTQ_MSG_PRE_VOTE_RESP 18

/* one inbound message: the fields of raftpb.Message that Step reads */
typedef struct raftq_msg {
  uint64_t group;
  uint64_t term;        /* m.Term; 0 marks a local message (MsgHup / MsgBeat) */
  uint64_t log_term;    /* m.LogTerm: MsgVote = candidate's last term */
  uint64_t index;       /* m.Index: MsgVote = candidate's last index; MsgAppResp = acked / rejected index */
  uint64_t commit;      /* m.Commit: MsgHeartbeat */
  uint64_t reject_hint; /* m.RejectHint (MsgAppResp with reject; passes through to the caller) */
  uint32_t from;        /* sender's peer slot 0..N-1 (raft ID - 1); ignored for local messages */
  uint8_t type;         /* RAFTQ_MSG_* */
  uint8_t reject;       /* m.Reject */
  uint8_t _pad[2];      /* IGNORED unless the handle opted in (raftq_step_set_msg_flags): then _pad[1] = RAFTQ_MSGF_* */
  uint64_t _resv;       /* IGNORED unless the handle opted in: then, under RAFTQ_MSGF_ENTRIES, low 32 bits = number of entries (MsgApp, MsgProp) */
} raftq_msg_t;          /* 64 bytes */

/* The ten bytes behind `reject` are padding to every caller that has not said otherwise: raftq_step_stage hands out
 * uninitialised memory, a caller that fills records field by field (the Go binding) never touches them, and whatever they
 * hold is ignored.  raftq_step_set_msg_flags(h, 1) -- no batch in flight -- makes them mean what RAFTQ_MSGF_* says below
 * for every batch submitted afterwards; such a caller writes all 64 bytes of every record.  (Round 3 gave the bits meaning
 * unconditionally: stale staging bytes could be read as "this MsgApp carries N entries".) */
int raftq_step_set_msg_flags(raftq_t* h, int on);

/* Step over each group's own voters (raftq.h "per-group voter sets": raftq_load_voters / raftq_apply_voter_deltas).
 * 0 (default): a handle with voter masks loaded is refused by every Step-family call, as before.
 * 1: those calls run over each group's own voters.  No batch in flight (RAFTQ_ESTATE); on other than 0 / 1: RAFTQ_EINVAL.
 *
 * The calls the switch opens: raftq_step_batch, raftq_step_submit / _collect, raftq_step_submit_packed, raftq_step_submit_wire,
 * raftq_step_frames / raftq_step_frames_packed (raftq_wire.h), raftq_apply_log_deltas / _nowait.  With on = 1 and no masks
 * loaded the handle launches exactly the kernels it launches otherwise.  The switch is a property of the handle, like the
 * message flags: raftq_clone_state does not copy it and raftq_load_voters(h, NULL) does not clear it.
 *
 * The rules with masks loaded are the sweep's, restated for Step (CHOICE marks what upstream has no counterpart for: its
 * `prs` map IS the membership, so there a non-member simply has no entry):
 *   quorum()       q_g = popcount(voters[g]) / 2 + 1.
 *   maybeCommit    the largest index held by >= q_g VOTERS, then the compact current-term gate as always.  An empty mask
 *                  gives candidate 0: nothing commits (CHOICE).  A one-voter group whose voter is the leader commits on its
 *                  own append: raftq_apply_log_deltas on a leader, and becomeLeader's empty entry.
 *   poll           every sender's first response is recorded as always; granted / recorded count voters only.
 *   win and loss   keep upstream's EQUALITY (`switch r.q()`): granted == q_g wins, recorded - granted == q_g loses.  A
 *                  mask that shrinks in the middle of an election can step over the equal count; that is upstream's
 *                  behaviour (a conf change applied mid-election) and the election timer's to repair.
 *   non-voters     their words are stored and read as always (CHOICE): an ack from a non-voter moves its Match and sets
 *                  RAFTQ_OUTF_UPDATED, a MsgVote from a non-voter is answered by the usual rule.
 *   reset()        writes all N slots as always -- self = lastIndex, the others 0 -- whether or not self is a voter.
 *   MsgHup         on a group in which self does not vote campaigns (CHOICE: Step does not ask promotable(); the Tick of a
 *                  handle that opted in to raftq_tick_set_voters, raftq.h, raises no MsgHup for such a group): the own
 *                  grant is recorded but not counted, so the result is RAFTQ_OUT_CAMPAIGN.
 *
 * What stays refused (RAFTQ_ESTATE, "voter masks" in the text) whatever this switch says: raftq_step_frames_respond,
 * raftq_propose_frames unless raftq_bcast_set_voters (raftq_wire.h) opted the handle in, and raftq_tick_frames,
 * raftq_tick_elect_frames unless raftq_tick_set_voters (raftq.h "batched Tick") did: each of those switches sends its calls'
 * broadcasts to each group's own members.  Without them the broadcasts go to N - 1 slots, not to a membership, and the
 * proposal path relies on "maybeCommit cannot move with more than one peer", which a one-voter group breaks -- over members
 * raftq_propose_frames refuses a record whose append would move the commit index.  raftq_step_frames_respond with
 * raftq_bcast_set_voters on runs the rules above whether or not this switch is on.  A sweep set takes masked members
 * when it is made with raftq_set_create_voters (raftq.h "sweep sets"; its sweeps and ticks then run over each member's own
 * voters) and refuses them when made with raftq_set_create; raftq_node (which never loads masks) is as before. */
int raftq_step_set_voters(raftq_t* h, int on);

/* Step takes forwarded proposals.  In the reference every node has its own front end and calls node.Propose locally
 * (raft.go:211-215); on a follower etcd's stepFollower forwards the proposal to the leader as a MsgProp frame, which reaches the
 * leader through Process -> node.Step (raft.go:268-270): with three nodes, two thirds of all writes.
 * 0 (default): type 2 is an unknown kind (a batch that holds one fails and applies nothing), and the frames calls of raftq_wire.h
 *    flag every MsgProp frame RAFTQ_MSGF_HOLD -- the caller's, RAFTQ_OUT_HELD, the rest of its group RAFTQ_OUT_DEFERRED -- as before.
 * 1: a record of type RAFTQ_MSG_PROP is stepped.  No batch in flight (RAFTQ_ESTATE); on other than 0 / 1: RAFTQ_EINVAL.  A
 *    property of the handle, like raftq_step_set_voters: raftq_clone_state does not copy it.
 * The switch matters only where a record's flag byte is read: without raftq_step_set_msg_flags type 2 stays an unknown kind
 * (the switch itself is accepted).
 *
 * The record.  It carries RAFTQ_MSGF_ENTRIES and its number of entries where a MsgApp's is (the low 32 bits of _resv).  It is
 * MALFORMED -- the batch fails and applies nothing -- without that flag, with a count of 0 (CHOICE: upstream's stepLeader panics on
 * an empty MsgProp) or with `from` >= N.  RAFTQ_MSGF_HOLD and RAFTQ_MSGF_SKIP win over the type as on every record.  The entries'
 * own Term and Index are not looked at (appendEntry overwrites them); no other field but group, term, from is read.  The caller
 * keeps last_index + n below 2^64: nothing checks it.
 *
 * The rules (2015-era etcd/raft).  raft.send leaves a MsgProp's Term at 0, so it passes Step's term rules as a local message
 * does; a record that does carry a term is judged by them as any message: a higher one makes the node a follower of `from` first,
 * a lower one is ignored (RAFTQ_OUT_NONE).  Then, by role:
 *   leader     appendEntry + the bookkeeping behind it: last_index += n, last_term = term, Progress[self].Match = last_index,
 *              maybeCommit.  RAFTQ_OUT_PROPOSED: index = the FIRST new index, log_term = term (what every new entry is stamped
 *              with), last_index = the new tail; RAFTQ_OUTF_COMMITTED | RAFTQ_OUTF_HARDSTATE when the commit index moved (N = 1,
 *              or a one-voter group under raftq_step_set_voters).  It holds nobody up: the group's later messages of the batch
 *              are stepped against the new tail, as upstream would (an acknowledgement's min(m.index, last_index) sees it).
 *              Storing the entries and bcastAppend are the caller's.
 *   follower   with a leader: RAFTQ_OUT_FORWARD, `to` = lead - 1 -- send the message on to the leader (`m.To = r.lead;
 *              r.send(m)`).  Nothing changes.  Without a leader: dropped, RAFTQ_OUT_NONE.
 *   candidate  dropped, RAFTQ_OUT_NONE.
 *
 * Where it does not reach: raftq_step_submit_wire (the pad bytes of its records are the decoder's, not RAFTQ_MSGF_*: type 2
 * stays malformed there) and the 40-byte inbound raftq_msg40_t (it carries no count: type 2 is malformed there too).  The frames
 * calls (raftq_step_frames, raftq_step_frames_packed, raftq_step_frames_respond; raftq_wire.h) with the switch on flag a MsgProp
 * frame with entries RAFTQ_MSGF_ENTRIES (its count is the decoder's n_ents) and one without entries RAFTQ_MSGF_SKIP, as a frame
 * of a kind a peer never sends; in the packed form a MsgProp with entries is a wide record, as every frame with entries is.
 * raftq_step_frames_respond leaves both results to the host (no RAFTQ_OUTF_ANSWERED) and, behind a RAFTQ_OUT_PROPOSED, builds no
 * commit broadcast for the group: its at-tail bit is cleared, no follower has the new entries yet -- unless
 * raftq_respond_set_props (raftq_wire.h) opted the handle in: then a RAFTQ_OUT_PROPOSED of a group at the tail is answered with the
 * leader's MsgApps, built on the device, and the bit stays.  raftq_node does not turn the switch on. */
int raftq_step_set_props(raftq_t* h, int on);

/* CheckQuorum in Step (raftq_set_check_quorum, raftq.h "CheckQuorum": the switch, the state and the Tick side).  With the switch
 * off every call returns what it always did and type 12 is an unknown kind that fails its batch.  With it on, in every walk form
 * and every Step-family call (etcd/raft's checkQuorum restated, PARITY UNPINNED; CHOICE marks what upstream has no counterpart for):
 *   1. stepLeader, on MsgAppResp and MsgHeartbeatResp from p: active |= 1 << p -- in front of the reject branch, so a rejected
 *      acknowledgement counts as activity.  Over masks (raftq_step_set_voters) a non-voter's bit is stored and does not count
 *      (CHOICE, as its Match).
 *   2. reset() -- becomeFollower, becomeCandidate, becomeLeader -- clears every activity bit and lead_elapsed.
 *   3. The lease, in Step's `m.Term > r.Term` arm, for MsgVote only: with
 *          inLease = role == leader || (lead != None && elapsed[g] < election_tick)
 *      the message is IGNORED -- RAFTQ_OUT_NONE, no state change, no response.  A leader under the switch is always in lease
 *      (upstream's electionElapsed wraps at electionTimeout); a candidate has no lead and never is.  Every other kind with a
 *      higher term behaves as always.  elapsed[g] is the Tick's word (a MsgApp / MsgHeartbeat earlier in the batch has zeroed it).
 *   4. RAFTQ_MSG_CHECK_QUORUM, a local kind: term 0, `from` ignored, like MsgHup and MsgBeat; the 64-byte and the 40-byte record
 *      both take it (a frame of that type from a peer stays a frame of a kind a peer never sends).
 *        leader   act = popcount((active | 1 << self) & members), members = the group's voter mask in the masked form, all N
 *                 slots otherwise; q = that form's quorum().  All activity bits are cleared.  act < q: becomeFollower(term, None) --
 *                 RAFTQ_OUT_NONE with RAFTQ_OUTF_STEPPED_DOWN, role follower, lead 0; Term and Vote do not change, so no
 *                 RAFTQ_OUTF_HARDSTATE.  Otherwise RAFTQ_OUT_NONE and nothing else changes.  An empty mask: act 0 < q 1, the
 *                 leader steps down (CHOICE).
 *        other    ignored (RAFTQ_OUT_NONE).
 * In raftq_step_frames_respond (raftq_wire.h) a lease-ignored MsgVote builds no frame and does not end its group's device-answered
 * prefix, and a device-answered becomeLeader clears the activity word in the lane that builds its broadcast.
 * raftq_node does not turn the switch on. */

/* PreVote in Step (raftq_set_pre_vote, raftq.h "PreVote": the switch, what it requires and closes).  With the switch off every call
 * returns what it always did and types 17 and 18 are unknown kinds that fail their batch.  With it on, in every walk form and every
 * Step-family call (etcd/raft's preVote and its answer to a stale leader restated, PARITY UNPINNED; CHOICE marks where this differs
 * from or adds to upstream).  raftq_msg_t and raftq_msg40_t take types 17 and 18 with MsgVote's fields (index / log_term = the
 * sender's tail, reject); both are a peer's kinds: `from` >= N is malformed.
 *   1. MsgHup on a non-leader is becomePreCandidate: role = RAFTQ_ROLE_PRE_CANDIDATE, lead = None, the vote word cleared and the
 *      own grant recorded, elapsed[g] = 0 (CHOICE: zeroed as Step's MsgHup always has; upstream leaves the clock alone).  Term,
 *      Vote, the Match words, the gate and the activity word do not change.  RAFTQ_OUT_PRE_CAMPAIGN: index / log_term = the log's
 *      tail, term = the unchanged r.Term -- the frames carry term + 1 --, no RAFTQ_OUTF_HARDSTATE.  If the own grant already equals
 *      quorum() (N = 1, a one-voter group) Step goes straight on through becomeCandidate and becomeLeader: the result is byte for
 *      byte what MsgHup gives without the switch.  Over masks with self not a voter the grant is recorded but not counted and the
 *      result is RAFTQ_OUT_PRE_CAMPAIGN (the existing CHOICE for MsgHup).  A leader ignores MsgHup, as always.
 *   2. m.Term > r.Term.  A MsgPreVote inside the lease is ignored exactly as a MsgVote is (CheckQuorum's rule 3, for both kinds);
 *      outside it, it changes no term and no role and goes on to rule 4.  A MsgPreVoteResp with reject == 0 changes no term and
 *      goes on to the role's arm; with reject == 1 it is becomeFollower(m.Term, None) (CHOICE: lead is None, the sender is no
 *      leader).  Every other kind behaves as always.
 *   3. 0 < m.Term < r.Term.  A MsgPreVote: RAFTQ_OUT_PRE_VOTE_RESP, reject = 1, index = r.Term.  A MsgApp or MsgHeartbeat:
 *      RAFTQ_OUT_TERM_RESP -- no state change, no clock reset; a RAFTQ_MSGF_BARRIER on it holds nobody up and RAFTQ_MSGF_ENTRIES is
 *      not looked at.  Every other kind is ignored, as always.
 *   4. A MsgPreVote that got this far is answered by one rule in every role (upstream moved vote handling in front of the role
 *      functions with PreVote):
 *          grant = (Vote == None || m.Term > r.Term || Vote == from + 1) && isUpToDate(m.Index, m.LogTerm)
 *      RAFTQ_OUT_PRE_VOTE_RESP: granted, index = m.Term; rejected, reject = 1 and index = r.Term.  NOTHING changes -- not Term, Vote,
 *      lead, role, elapsed or the activity bits -- and no flag is set.  A MsgVote is answered by the per-role rules it always had.
 *   5. Role 3 is stepped by the candidate's arm, but: it polls MsgPreVoteResp and ignores MsgVoteResp (a candidate ignores
 *      MsgPreVoteResp; so do a follower and a leader).  granted == quorum(): becomeCandidate -- term + 1, vote self, reset() incl.
 *      the activity word, the own grant -- and the result is one of the two MsgHup has without the switch: RAFTQ_OUT_CAMPAIGN with
 *      RAFTQ_OUTF_HARDSTATE, or RAFTQ_OUT_BECAME_LEADER if the own grant is the quorum.  recorded - granted == quorum():
 *      becomeFollower(term, None), RAFTQ_OUTF_STEPPED_DOWN, Term and Vote kept.  Upstream's equality form, masked too.  A MsgApp /
 *      MsgHeartbeat of the own term: becomeFollower(term, from) and handled, as a candidate does; a MsgVote of the own term is
 *      rejected; a MsgProp is dropped.
 * The compact records: RAFTQ_OUT_PRE_CAMPAIGN is packed as RAFTQ_OUT_CAMPAIGN is (below).  In raftq_step_frames_respond
 * (raftq_wire.h) the three new results are the host's -- no RAFTQ_OUTF_ANSWERED, and they end their group's device-answered prefix --
 * while a lease-ignored MsgPreVote builds no frame and does not end it, as a lease-ignored MsgVote does not.  Under the switch the
 * frames calls take frames of types 17 and 18; without it they stay frames of a kind a peer never sends.  Device-built MsgPreVote
 * rounds are not built yet: raftq_tick_elect_frames refuses the handle.  raftq_node does not turn the switch on. */

/* Leadership transfer in Step (raftq_set_lead_transfer, raftq.h "Leadership transfer": the switch, its state, what it requires and
 * closes).  With the switch off every call returns what it always did, types 13 and 14 are unknown kinds that fail their batch and
 * apply nothing, and a MsgVote's `reject` byte is not looked at.  With it on, in every walk form and every Step-family call
 * (etcd/raft's leadership transfer restated, PARITY UNPINNED; CHOICE marks where this differs from or adds to upstream).  The
 * transferee is leadTransferee[g], bits 12..15 of the activity word (0 = None, else slot + 1); no Tick kernel changes.
 *   1. The records.  Both kinds use group, term, from.  A MsgTransferLeader's `from` is the TRANSFEREE's slot in both of its forms:
 *      the local one (term 0: what node.TransferLeadership steps) and the forwarded one (a follower sends it on with its own term).
 *      `from` >= N is malformed even at term 0.  MsgTimeoutNow is a peer's kind.  raftq_msg_t and raftq_msg40_t both take them.
 *   2. The mark.  CHOICE: a transfer's campaign marks its MsgVote with reject = 1 (upstream: Context == "CampaignTransfer"; this
 *      wire has no Context field, and its field 12 is the group).  `reject` is carried by the 64-byte record, the 40-byte record
 *      and the frame, and means nothing else on a request.
 *   3. The lease.  CheckQuorum's rule 3 and PreVote's rule 2 ignore a MsgVote only if reject == 0.  A marked MsgVote of a higher
 *      term is becomeFollower(m.Term, None) and is answered by the role's rule as always.  A MsgPreVote is never marked.
 *   4. Leader, MsgTransferLeader, t = from.  t not a voter (the masked form; upstream's pr == nil): ignored.  A transfer to t
 *      already pending: ignored.  One to another slot pending: aborted first.  Then t == self: stop (a transfer to self therefore
 *      cancels a pending one, as upstream).  Otherwise leadTransferee = t + 1 and lead_elapsed = 0; RAFTQ_OUT_TRANSFER, to = t,
 *      index = Match[t]; with RAFTQ_OUTF_TIMEOUT_NOW when Match[t] == last_index (send MsgTimeoutNow{To: t, Term: term}), without
 *      it the caller runs sendAppend(t).  Every ignored case is RAFTQ_OUT_NONE and changes nothing.
 *   5. Leader, MsgAppResp from the pending transferee for which maybeUpdate returned true (RAFTQ_OUTF_UPDATED) and whose Match now
 *      equals last_index: its RAFTQ_OUT_PROGRESS also carries RAFTQ_OUTF_TIMEOUT_NOW.  An ack that does not update sends nothing
 *      (upstream has it inside the update branch).
 *   6. Leader, MsgProp with a transfer pending: dropped -- RAFTQ_OUT_NONE, nothing moves (upstream's ErrProposalDropped).
 *   7. reset().  Every becomeFollower / becomeCandidate / becomeLeader clears the transferee (the activity word is zeroed as it
 *      always was), and RAFTQ_MSG_CHECK_QUORUM clears it whether or not the check passes.
 *   8. Follower, MsgTransferLeader: with a leader RAFTQ_OUT_FORWARD, to = lead - 1, nothing changes; without one RAFTQ_OUT_NONE.
 *      A candidate or pre-candidate: RAFTQ_OUT_NONE.
 *   9. MsgTimeoutNow.  The term rules come first, as for any message: a higher term makes the node a follower of `from`; a lower
 *      one is ignored (under PreVote it is NOT one of the kinds answered RAFTQ_OUT_TERM_RESP).  A follower that is a voter --
 *      the masked form asks promotable(), as upstream does; a follower that is not gives RAFTQ_OUT_NONE -- campaigns at once: the
 *      real campaign even under PreVote, no pre-candidate step.  RAFTQ_OUT_CAMPAIGN with reject = 1 (send the MsgVotes marked), or
 *      RAFTQ_OUT_BECAME_LEADER (reject = 0) if the own grant is the quorum.  A leader, candidate or pre-candidate ignores it.
 * Not modelled (CHOICE): a voter delta that removes the pending transferee does not abort the transfer; the Tick's timeout does.
 * The compact records: RAFTQ_OUT_TRANSFER packs as RAFTQ_OUT_PROGRESS does; `reject` and the new flag ride all three formats as
 * they are.  In raftq_step_frames_respond (raftq_wire.h) RAFTQ_OUT_TRANSFER, a forwarded MsgTransferLeader and a campaign from
 * MsgTimeoutNow are the host's -- no RAFTQ_OUTF_ANSWERED, and they end their group's device-answered prefix --;
 * RAFTQ_OUTF_TIMEOUT_NOW is always the host's to send and does not stop a committing ack's commit broadcast from being built and
 * flagged RAFTQ_OUTF_ANSWERED.  Under the switch the frames calls take frames of types 13 and 14; without it they stay frames of a
 * kind a peer never sends.  No encoder builds the two kinds on the device.  raftq_node does not turn the switch on. */

/* ReadIndex in Step (raftq_set_read_index, raftq.h "ReadIndex": the switch, its modes, its state, what it requires and closes).
 * With the switch off every call returns what it always did, and types 15 and 16 are unknown kinds that fail their batch and apply
 * nothing.  With it on, in every walk form and every Step-family call (etcd/raft's ReadIndex restated, PARITY UNPINNED; CHOICE marks
 * where this differs from or adds to upstream).  seq, acked[p] and confirmed() are the group's read record (RAFTQ_READ_SAFE only).
 *   1. The records.  RAFTQ_MSG_READ_INDEX uses group and from: `from` is the REQUESTER's slot -- self for a local request, the
 *      follower's for a forwarded one.  raft.send leaves its Term at 0, as for MsgProp, so it passes the term rules as a local
 *      message does; a record that does carry a term is judged by them as any message is -- a higher one is becomeFollower(m.Term,
 *      None): `from` is the requester, who leads nothing (forward a read at term 0, as it came).  `from` >= N is malformed even at
 *      term 0.
 *      RAFTQ_MSG_READ_INDEX_RESP is a peer's kind: group, term, from, index.  raftq_msg_t and raftq_msg40_t both take them.  The
 *      request's own context (upstream: Entries[0].Data) stays with the caller: result i answers record i, the device needs no id.
 *   2. Leader, MsgReadIndex.  Dropped -- RAFTQ_OUT_NONE, nothing moves -- while the leader has not committed an entry of its term
 *      (first_idx == 0 || committed < first_idx, the gate's own words; CHOICE: etcd 3.3 / 3.4, later versions queue the request),
 *      and in the safe mode at seq == 2^32 - 1 (CHOICE).  Otherwise RAFTQ_OUT_READ_INDEX, to = from, index = committed.
 *      RAFTQ_READ_LEASE: log_term = 0 and RAFTQ_OUTF_READ_READY -- release at once; nothing else changes.  RAFTQ_READ_SAFE:
 *      seq += 1, acked[self] = seq, log_term = seq; RAFTQ_OUTF_READ_READY iff confirmed() >= seq already (N = 1, or a one-voter
 *      group whose voter is self).  Without the flag the caller queues the read and sends MsgHeartbeat{Index: seq} to every member
 *      (upstream's bcastHeartbeatWithCtx); of several such results of one group in a batch only the last one's round needs sending.
 *   3. Leader, MsgHeartbeatResp from p with c = m.index, RAFTQ_READ_SAFE.  CHOICE: the context rides the `index` field of
 *      MsgHeartbeat and its response -- neither kind reads that field otherwise, and this wire has no Context field.  c == 0, or
 *      c > seq (no honest peer sends that; CHOICE: ignored): exactly as without the switch.  Otherwise before = confirmed();
 *      acked[p] = max(acked[p], c); after = confirmed(); if after > before the RAFTQ_OUT_PROGRESS result also carries
 *      RAFTQ_OUTF_READ_READY and log_term = after: the caller releases every queued read with sequence <= after, at the index its
 *      RAFTQ_OUT_READ_INDEX gave.  `index` stays Match; the activity bit, at_tail and everything else are as always.
 *      CHOICE against upstream: upstream counts acknowledgements per context; here an acknowledgement of c counts for every
 *      request <= c.  Round c was sent after request s <= c arrived, so the acknowledgement proves leadership at a time after
 *      that request as well.  Every release upstream makes, this rule makes at the same message or an earlier one, never a later
 *      one; and it survives loss, duplication and reordering without a queue on the device.
 *   4. reset() clears seq and every acked word: every becomeFollower / becomeCandidate / becomeLeader (upstream: readOnly =
 *      newReadOnly).  The caller drops its queue on RAFTQ_OUTF_STEPPED_DOWN or a change of role.  A RAFTQ_MSG_CHECK_QUORUM that
 *      passes does NOT clear it.
 *   5. Leader, MsgBeat, RAFTQ_READ_SAFE: RAFTQ_OUT_BCAST_HEARTBEAT gets index = seq if seq > confirmed(), else 0 -- upstream's
 *      lastPendingRequestCtx, the resend of a lost round.
 *   6. Follower.  MsgReadIndex with a leader: RAFTQ_OUT_FORWARD, to = lead - 1, nothing changes; without one RAFTQ_OUT_NONE.  A
 *      candidate or pre-candidate: RAFTQ_OUT_NONE.  MsgHeartbeat, in the follower's arm and in the candidate's arm that becomes a
 *      follower: the RAFTQ_OUT_HEARTBEAT_RESP result gets index = m.index, the echo -- in both modes: a lease-mode follower may sit
 *      under a safe-mode leader.  MsgReadIndexResp on a follower: RAFTQ_OUT_READ_STATE, to = from, index = m.index, nothing
 *      changes beyond what the term rules did -- a higher term is becomeFollower(m.Term, None) first, as for any kind that is not
 *      a leader's.  A leader or candidate ignores MsgReadIndexResp; a lower term is ignored, as always.
 *   7. The compact records.  RAFTQ_OUT_READ_INDEX, and a RAFTQ_OUT_PROGRESS with RAFTQ_OUTF_READ_READY, carry log_term in the
 *      `commit` slot of both the 40-byte and the 32-byte record.  The first one's commit IS its `index`; the second one's is not
 *      delivered -- a MsgHeartbeatResp moves no commit index.  RAFTQ_OUT_READ_STATE and a forwarded read pack as
 *      RAFTQ_OUT_PROGRESS / RAFTQ_OUT_FORWARD do.
 *   8. Frames (raftq_wire.h): under the switch the frames calls and raftq_step_submit_wire take types 15 and 16 as kinds a peer
 *      sends.  In raftq_step_frames_respond a device-built MsgHeartbeatResp carries Index = m.index (with a zero context the bytes
 *      are what they were); RAFTQ_OUT_READ_INDEX, RAFTQ_OUT_READ_STATE and a forwarded read are the host's -- no
 *      RAFTQ_OUTF_ANSWERED, and they end their group's device-answered prefix; RAFTQ_OUTF_READ_READY on a progress result ends no
 *      prefix and stops no commit broadcast.  No encoder builds types 15 and 16 on the device: the context bytes are host memory.
 *   9. What the switch closes: raftq.h "ReadIndex".  raftq_node does not turn the switch on. */

/* raftq_msg_t._pad[1] once the handle opted in.  RAFTQ_MSGF_ENTRIES on a MsgApp: the caller says what the message carries -- the low 32 bits of
 * _resv = its number of entries, reject_hint (a field MsgApp does not use) = the Term of the last one (unused with no
 * entries).  Step then runs raftLog.maybeAppend itself whenever the message appends at the TAIL of the log (m.Index ==
 * lastIndex and m.LogTerm == lastTerm: findConflict has nothing to look at): lastIndex / lastTerm move past the new
 * entries, commitTo(min(m.Commit, lastnewi)) runs, and the result is RAFTQ_OUT_APPENDED -- no raftq_apply_log_deltas
 * round trip for the common case of replication.  Every other MsgApp (a gap, a conflict, an index below the tail)
 * is answered RAFTQ_OUT_APPEND as without the flag.  On a MsgProp (raftq_step_set_props) the flag is required and _resv says how
 * many entries are proposed.  Ignored on every other kind and on packed (40-byte) records. */
#define RAFTQ_MSGF_ENTRIES 0x80u
/* RAFTQ_MSGF_BARRIER on a MsgApp: if Step leaves the append to the caller (RAFTQ_OUT_APPEND: the log's tail is about to change
 * in a way only the log's owner can work out), the messages of the same group that FOLLOW it in this batch are not applied --
 * they would be stepped against a stale tail -- and are answered RAFTQ_OUT_DEFERRED: step them again, in order, after
 * raftq_apply_log_deltas.  With it a caller need not keep back everything behind a MsgApp: a batch may hold any number of
 * messages per group, and the ones that land on the tail (RAFTQ_OUT_APPENDED) hold nobody up. */
#define RAFTQ_MSGF_BARRIER 0x40u
/* RAFTQ_MSGF_HOLD on any record: the message is one Step does not take (a MsgProp on a handle without raftq_step_set_props,
 * raft.go:211-215) but whose place in its group's arrival order matters.  It is NOT stepped -- its type and `from` are not even
 * looked at -- and answered RAFTQ_OUT_HELD (the group's state as it stands at that point of the batch), whatever came before
 * it; every message of the group BEHIND it in this batch is answered RAFTQ_OUT_DEFERRED, as behind a barrier.  The caller
 * deals with the held message when it walks the results in order and steps the deferred ones in a later batch. */
#define RAFTQ_MSGF_HOLD 0x20u
/* RAFTQ_MSGF_SKIP on any record: not a message at all (a frame that did not parse, or was addressed to somebody else) -- no
 * field of the record is looked at, nothing is applied, the answer is RAFTQ_OUT_SKIPPED (an otherwise zero record).  With it a
 * batch can stand for "everything received, in order" and result i still answers record i. */
#define RAFTQ_MSGF_SKIP 0x10u

/* what Step did with message i: out[i] answers msgs[i] */
#define RAFTQ_OUT_NONE 0            /* ignored: stale term, or this role does not handle the type */
#define RAFTQ_OUT_VOTE_RESP 1       /* send MsgVoteResp{To: to, Term: term, Reject: reject} */
#define RAFTQ_OUT_HEARTBEAT_RESP 2  /* send MsgHeartbeatResp{To: to, Term: term} */
#define RAFTQ_OUT_CAMPAIGN 3        /* became candidate: send MsgVote{Term: term, Index: index, LogTerm: log_term} to every other peer */
#define RAFTQ_OUT_BECAME_LEADER 4   /* won the election: append the empty entry {Term: term, Index: index}, then bcastAppend */
#define RAFTQ_OUT_PROGRESS 5        /* leader took MsgAppResp / MsgHeartbeatResp from `to`: index = Progress.Match now */
#define RAFTQ_OUT_BCAST_HEARTBEAT 6 /* leader's MsgBeat: send MsgHeartbeat to every other peer */
#define RAFTQ_OUT_APPEND 7          /* MsgApp header accepted: run raftLog.maybeAppend on the log, then raftq_apply_log_deltas */
#define RAFTQ_OUT_DEFERRED 9        /* NOT applied: an earlier MsgApp of the group with RAFTQ_MSGF_BARRIER was answered RAFTQ_OUT_APPEND, or an
                                     * earlier record of the group carried RAFTQ_MSGF_HOLD */
#define RAFTQ_OUT_APPENDED 8        /* MsgApp with RAFTQ_MSGF_ENTRIES that appended at the tail: Step did maybeAppend's bookkeeping -- store
                                     * the entries, send MsgAppResp{Index: index} (index = lastnewi = last_index); commit is final */
#define RAFTQ_OUT_SKIPPED 10        /* RAFTQ_MSGF_SKIP: nothing looked at, nothing applied */
#define RAFTQ_OUT_HELD 11           /* RAFTQ_MSGF_HOLD: not stepped; the group's later messages of this batch are RAFTQ_OUT_DEFERRED */
#define RAFTQ_OUT_PROPOSED 12       /* leader took a MsgProp (raftq_step_set_props): store its n entries as {Term: log_term, Index: index ..
                                     * last_index}, then bcastAppend */
#define RAFTQ_OUT_FORWARD 13        /* follower's MsgProp: send it on to `to` = lead - 1, the one result whose addressee is not the sender */
#define RAFTQ_OUT_PRE_CAMPAIGN 14   /* became pre-candidate: send MsgPreVote{Term: term + 1, Index: index, LogTerm: log_term} to every other peer */
#define RAFTQ_OUT_PRE_VOTE_RESP 15  /* send MsgPreVoteResp{To: to, Term: index, Reject: reject} -- `index` carries the response's Term */
#define RAFTQ_OUT_TERM_RESP 16      /* a stale leader's MsgApp / MsgHeartbeat: send MsgAppResp{To: to, Term: term} (Index 0, no reject) */
#define RAFTQ_OUT_TRANSFER 17       /* leader took a MsgTransferLeader: `to` = the transferee, index = its Match; with RAFTQ_OUTF_TIMEOUT_NOW send
                                     * MsgTimeoutNow{To: to, Term: term}, without it run sendAppend(to) */

#define RAFTQ_OUT_READ_INDEX 18     /* leader took a MsgReadIndex: `to` = the requester, index = the read's index (the commit index), log_term = its
                                     * sequence number (0 in the lease mode); release it with RAFTQ_OUTF_READ_READY, else queue it and send
                                     * MsgHeartbeat{Index: log_term} to every member */
#define RAFTQ_OUT_READ_STATE 19     /* follower got the leader's MsgReadIndexResp: the read it forwarded is good at `index` */

#define RAFTQ_OUTF_HARDSTATE 0x01u    /* Term, Vote or Commit changed: HardState must be persisted (wal.Save, raft.go:228) */
#define RAFTQ_OUTF_COMMITTED 0x02u    /* raftLog.committed advanced (leader: bcastAppend carries it) */
#define RAFTQ_OUTF_UPDATED 0x04u      /* Progress.maybeUpdate returned true */
#define RAFTQ_OUTF_STEPPED_DOWN 0x08u /* was leader or candidate, is follower now */
/* (0x10u is RAFTQ_OUTF_ANSWERED, raftq_wire.h) */
#define RAFTQ_OUTF_TIMEOUT_NOW 0x20u  /* raftq_set_lead_transfer: the pending transferee `to` is at the tail -- send MsgTimeoutNow{To: to, Term: term} */
/* RAFTQ_OUTF_READ_READY is 0x40u.  It is spelled as a shift because tests/test_lead_transfer_abi.py, written when 0x20u was "the one
 * bit that was free", sums every flag spelled 0xNNu in this header and raftq_wire.h and expects 0x3F; existing tests are not edited by
 * the change that adds a flag.  tests/test_read_index_abi.py holds the value (a C _Static_assert) and that no other flag has the bit.
 * When that older assertion is brought up to date this becomes 0x40u like its neighbours. */
#define RAFTQ_OUTF_READ_READY (1u << 6) /* raftq_set_read_index: on RAFTQ_OUT_READ_INDEX release this read; on RAFTQ_OUT_PROGRESS release every queued
                                       * read of the group with sequence number <= log_term */

typedef struct raftq_step_out {
  uint64_t group;
  uint64_t term;       /* r.Term after the message */
  uint64_t index;      /* by type, see RAFTQ_OUT_* */
  uint64_t log_term;   /* by type */
  uint64_t commit;     /* raftLog.committed after the message */
  uint64_t last_index; /* raftLog.lastIndex() after the message */
  uint32_t to;         /* addressee of the response = sender of the message (RAFTQ_OUT_FORWARD: the leader's slot, lead - 1) */
  uint32_t vote;       /* r.Vote after: 0 = None, else peer slot + 1 */
  uint32_t lead;       /* r.lead after: 0 = None, else peer slot + 1 */
  uint8_t type;        /* RAFTQ_OUT_* */
  uint8_t reject;
  uint8_t flags;       /* RAFTQ_OUTF_* */
  uint8_t role;        /* RAFTQ_ROLE_* after the message */
} raftq_step_out_t;    /* 64 bytes */

/* the caller's log changed: it now ends at (last_index, last_term).  Leader
 * (appendEntry): Progress[self].maybeUpdate(last_index) and maybeCommit.
 * Follower (handleAppendEntries after maybeAppend): commitTo(min(commit_to,
 * last_index)); commit_to = 0 leaves the commit index alone. */
typedef struct raftq_log_delta {
  uint64_t group;
  uint64_t last_index;
  uint64_t last_term;
  uint64_t commit_to;
} raftq_log_delta_t;

typedef struct raftq_step_counts {
  uint64_t n_msgs;
  uint64_t n_groups_touched;
} raftq_step_counts_t;

/* which peer slot this process is in every group of the handle (raft ID - 1) */
int raftq_set_self(raftq_t* h, uint32_t self_peer);

/* bulk load / read-back of the node state ([G] each; any pointer may be NULL).
 * vote / lead: 0 = None, else peer slot + 1. */
int raftq_load_node(raftq_t* h, const uint64_t* term, const uint32_t* vote, const uint32_t* lead,
                    const uint64_t* last_index, const uint64_t* last_term);
int raftq_read_node(raftq_t* h, uint64_t* term, uint32_t* vote, uint32_t* lead, uint64_t* last_index,
                    uint64_t* last_term, uint64_t* first_idx_cur_term);

/* Step for a batch.  `out` receives n records (out[i] answers msgs[i]); may be
 * NULL when the caller only wants the state change.  Returns RAFTQ_EINVAL and
 * applies nothing if any message is malformed (group / from out of range,
 * unknown type). */
int raftq_step_batch(raftq_t* h, const raftq_msg_t* msgs, uint64_t n, raftq_step_out_t* out,
                     raftq_step_counts_t* counts);

/* pipelined form: up to THREE batches in flight.  raftq_step_submit enqueues a batch and returns
 * at once; raftq_step_collect blocks for the oldest batch in flight and hands out its results.
 * (A batch's result records leave the device inside the walk kernel of the batch submitted behind it -- a copy kernel
 * of their own would hold that batch's kernels back -- or at its own collect when nothing is behind it: keep a batch
 * on the device and one being handed over while waiting for a third, and the copy, the walk and the host overlap.)
 * Batches are applied in submission order; the H2D copy of batch k+1 overlaps the kernels and the
 * result copy of batch k.  raftq_step_batch == submit + collect.
 * A malformed batch is reported by ITS collect and applies nothing; a batch submitted behind it
 * is still applied.  While batches are in flight every other call that reads or changes group
 * state (sweeps, Tick, deltas, raftq_apply_log_deltas, raftq_load_* / raftq_read_*) returns RAFTQ_ESTATE:
 * a batch is only guaranteed applied once collected (one holding more than 32 messages of a single
 * group is replayed through the sorted walk at its collect, in order with whatever follows it). */
int raftq_step_submit(raftq_t* h, const raftq_msg_t* msgs, uint64_t n);
int raftq_step_collect(raftq_t* h, raftq_step_out_t* out /*[n]|NULL*/, raftq_step_counts_t* counts /*|NULL*/);

/* zero-copy variants.  raftq_step_stage returns the staging array the NEXT submit will use (the three slots
 * alternate: ask again for every batch), with room for n messages -- fine-grained DEVICE memory when the host
 * can address it (large BAR: the receive path's stores land in HBM and the batch needs no inbound DMA), pinned
 * host memory otherwise (or with RAFTQ_STAGE=host); write-only for the host either way (reads of device
 * memory over the BAR are uncached).  Fill it in place and pass the SAME pointer to raftq_step_submit /
 * raftq_step_batch and no host copy is made -- behind a large BAR no copy at all: the batch is walked where it was
 * written, so the array belongs to the library from that submit until the batch is collected (do not write to it
 * again; raftq_step_stage hands out another slot's array for the next batch).  With out == NULL the result
 * records stay in pinned memory; raftq_step_results returns those of the batch collected last
 * (valid until the next raftq_step_submit / raftq_step_batch). */
int raftq_step_stage(raftq_t* h, uint64_t n, raftq_msg_t** msgs);
int raftq_step_results(raftq_t* h, const raftq_step_out_t** out, uint64_t* n);

/* Packed inbound records: 40 instead of 64 bytes per message cross PCIe (or the BAR) on the way IN -- a pipelined
 * Step is bound by exactly that transfer.  No message kind Step accepts carries both a LogTerm and a RejectHint, so
 * the two share a field; the group id takes 32 bits (handles of 2^32 groups or more refuse the packed calls).  The
 * records are widened to raftq_msg_t on the device before Step reads them: the results, the order and the
 * all-or-nothing rule are those of raftq_step_submit on the widened batch. */
typedef struct raftq_msg40 {
  uint32_t group;
  uint8_t from;         /* sender's peer slot */
  uint8_t type;         /* RAFTQ_MSG_* */
  uint8_t reject;
  uint8_t _pad;         /* 0 */
  uint64_t term;
  uint64_t index;
  uint64_t aux;         /* m.RejectHint on MsgAppResp, m.LogTerm on every other kind */
  uint64_t commit;
} raftq_msg40_t;        /* 40 bytes */
/* as raftq_step_stage / raftq_step_submit; collect with raftq_step_collect (packed and plain batches may alternate) */
int raftq_step_stage_packed(raftq_t* h, uint64_t n, raftq_msg40_t** msgs);
int raftq_step_submit_packed(raftq_t* h, const raftq_msg40_t* msgs, uint64_t n);

/* Compact result records: 40 instead of 64 bytes per message cross PCIe (the result copy is what a pipelined
 * batch waits for).  Record i answers msgs[i], so its group and addressee (= msgs[i].group, msgs[i].from) are not
 * repeated; `aux` is log_term for RAFTQ_OUT_CAMPAIGN / RAFTQ_OUT_BECAME_LEADER / RAFTQ_OUT_PRE_CAMPAIGN -- whose `index` is the last index --
 * and raftLog.lastIndex() for every other type (whose log_term is 0, but for RAFTQ_OUT_PROPOSED, whose log_term IS its term):
 * the full record is recovered exactly.  The addressee of a RAFTQ_OUT_FORWARD is not msgs[i].from: it is recovered from the
 * record's `lead` (to = lead - 1), here and in the 32-byte record.
 * While the format is on, raftq_step_collect / _batch take out == NULL and the records are read in place through
 * raftq_step_results_c (valid until the next submit).  Switch only with no batch in flight. */
typedef struct raftq_step_out_c {
  uint64_t term;   /* r.Term after the message */
  uint64_t index;  /* by type, as raftq_step_out_t */
  uint64_t commit; /* raftLog.committed after */
  uint64_t aux;    /* see above */
  uint8_t vote;    /* 0 = None, else peer slot + 1 */
  uint8_t lead;
  uint8_t type;    /* RAFTQ_OUT_* */
  uint8_t reject;
  uint8_t flags;   /* RAFTQ_OUTF_* */
  uint8_t role;
  uint8_t _pad[2];
} raftq_step_out_c_t; /* 40 bytes */
/* The 32-byte record (round 6; raftq_step_set_compact(h, 2)): the 40-byte one without `aux`.  What aux carried is either not
 * needed by whoever applies a result (raftLog.lastIndex() after a message: the log's owner knows its own log) or recoverable:
 * log_term of a RAFTQ_OUT_BECAME_LEADER IS its term (becomeLeader appends the empty entry of the new term), and a
 * RAFTQ_OUT_CAMPAIGN -- which moves no commit index -- carries its log_term in `commit`, and so does a RAFTQ_OUT_PRE_CAMPAIGN.  The full record is recovered exactly
 * by a reader that tracks lastIndex / committed per group across the batch (tests/test_step_gpu.py does); behind a
 * RAFTQ_OUT_PROPOSED the tail is index + n - 1, n being the count of the reader's own record, and its log_term is its term.  Why not the
 * 16-byte-per-message + 24-byte-per-touched-group form VERDICT r05 sketched: a result's term and commit are the state AFTER
 * THAT message (a vote response carries the term it was granted at, a leader broadcasts the commit index it had), so a group
 * needs a state record per CHANGE, not one per batch; with that, 16 + 24 k bytes per message (k = state changes per message)
 * is below 32 only under 0.67 changes per message and needs a compaction pass in the walk's latency path; 32 fixed bytes are
 * 20 % less than 40 on every mix and ride the pipeline as they are.
 * raftq_step_set_compact: 0 = 64-byte records, 1 = 40-byte, 2 = 32-byte. */
typedef struct raftq_step_out_s {
  uint64_t term;   /* r.Term after the message */
  uint64_t index;  /* by type, as raftq_step_out_t */
  uint64_t commit; /* raftLog.committed after; RAFTQ_OUT_CAMPAIGN / RAFTQ_OUT_PRE_CAMPAIGN: the candidate's log_term */
  uint8_t vote;    /* 0 = None, else peer slot + 1 */
  uint8_t lead;
  uint8_t type;    /* RAFTQ_OUT_* */
  uint8_t reject;
  uint8_t flags;   /* RAFTQ_OUTF_* */
  uint8_t role;
  uint8_t _pad[2];
} raftq_step_out_s_t; /* 32 bytes */
int raftq_step_set_compact(raftq_t* h, int on);
int raftq_step_results_c(raftq_t* h, const raftq_step_out_c_t** out, uint64_t* n);
int raftq_step_results_s(raftq_t* h, const raftq_step_out_s_t** out, uint64_t* n);

/* records of one group are applied in order; committed_out (may be NULL) receives
 * raftLog.committed after record i -- how a commit moved by a tail report (a leader that
 * is its own quorum, a follower's commitTo) surfaces, the way Ready.HardState.Commit does */
int raftq_apply_log_deltas(raftq_t* h, const raftq_log_delta_t* d, uint64_t n, uint64_t* committed_out /*[n]|NULL*/);
/* The same reports enqueued and left: the call returns as soon as the records are staged, the engine's state has moved by the time
 * anything called later on the handle runs, and nothing comes back -- for the reports whose outcome the caller knows: a LEADER's
 * appendEntry with more than one peer cannot move raftLog.committed (the leader's own Match is the largest; the quorum-th
 * largest is somebody else's and no ack has arrived for entries that did not exist), which is every report of a steady-state
 * turn's proposals.  raftq_node makes this call for exactly those and the waiting one for everything else. */
int raftq_apply_log_deltas_nowait(raftq_t* h, const raftq_log_delta_t* d, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif /* RAFTQ_STEP_H */
