/*
 * raftq.h -- C-ABI of the MI355X batched multi-raft quorum engine.
 *
 * This is the drop-in boundary for ONE hot path of chzchzchz/raftsql: the
 * per-group quorum arithmetic that the reference reaches through
 *     rc.node.Step     (raft.go:268-270, inbound MsgAppResp / MsgVoteResp)
 *     rc.node.Propose  (raft.go:211-215, leader-local append)
 *     rc.node.Tick     (raft.go:223-224)
 * and whose result the reference consumes from rc.node.Ready() (raft.go:227,
 * HardState.Commit / CommittedEntries).  The arithmetic itself lives in the
 * un-vendored dependency github.com/coreos/etcd/raft (SURVEY.md section 0,
 * F1/F2): raft.maybeCommit, raftLog.maybeCommit, raft.q and raft.poll.  The
 * reference has no FFI for it, so the entry points below are what a cgo shim
 * in a G-group raftsql would bind (see INTEGRATION.md for that shim).
 *
 * Conventions
 *   - every function returns RAFTQ_OK (0) or a negative RAFTQ_E* code; none
 *     throws, aborts or calls exit().  raftq_last_error() gives the text.
 *   - a handle owns device-resident SoA state for G groups x N peers on one
 *     GPU.  One handle is NOT thread-safe (the caller serialises, mirroring
 *     the one-goroutine rule of raft.Node); different handles are independent.
 *   - host buffers are caller-owned and are only read/written during the
 *     call; no pointer is retained after return (cgo pointer rule).
 *   - host-side matrices are peer-major and dense:  x[p * G + g].
 *   - vote encoding (uint8): 0 = no response yet, 1 = granted, 2 = rejected.
 *     Any other byte value counts as "no response".
 *   - outcome encoding (uint8): 0 = pending, 1 = won, 2 = lost.
 *   - log indices and terms are uint64, as raftpb's.  Index 0 is the dummy
 *     entry: it carries term 0 and never commits.
 */
#ifndef RAFTQ_H
#define RAFTQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAFTQ_ABI_VERSION 1
#define RAFTQ_MAX_PEERS 9 /* north_star: selection network for N <= 9 */

/* return codes */
#define RAFTQ_OK 0
#define RAFTQ_EINVAL (-1)  /* bad argument (NULL, N out of range, G == 0 ...) */
#define RAFTQ_ENOMEM (-2)  /* device or pinned-host allocation failed */
#define RAFTQ_EHIP (-3)    /* a HIP runtime call failed; see raftq_last_error */
#define RAFTQ_ESTATE (-4)  /* call sequence error (e.g. gated sweep, no terms) */
#define RAFTQ_ENODEV (-5)  /* no usable GPU / device index out of range */

/* sweep flags (raftq_step_async) */
#define RAFTQ_SWEEP_COMMIT 0x01u /* commit-advance: etcd raft.maybeCommit */
#define RAFTQ_SWEEP_GATED 0x02u  /* + raftLog.maybeCommit's current-term gate */
#define RAFTQ_SWEEP_VOTES 0x04u  /* RequestVote tally: etcd raft.poll */
#define RAFTQ_SWEEP_NO_ADOPT 0x08u /* evaluate into the shadow commit buffer
                                      but do not make it current ("what-if") */
#define RAFTQ_SWEEP_LDS 0x10u /* A/B variant: LDS-staged odd-even transposition
                                 sort instead of the in-register network */
#define RAFTQ_SWEEP_CHANGED 0x20u /* also emit the changed-groups bitmap that
                                     raftq_collect_changed() compacts */
/* cache policy of the sweep's loads/stores.  Default (neither bit): chosen by
 * the handle's footprint -- state that fits the 256 MiB Infinity Cache is
 * swept with normal (cached) accesses so the next sweep hits on-die, larger
 * state is streamed non-temporally.  A caller that knows better (e.g. many
 * handles swept round-robin, so none stays cached) forces one. */
#define RAFTQ_SWEEP_STREAM 0x40u /* force non-temporal streaming accesses */
#define RAFTQ_SWEEP_CACHED 0x80u /* force normal cached accesses */

/* raftq_cycle / raftq_cycle_packed only: the caller vouches for the ranges of its records (a driver that built them
 * itself), so the library validates and scatters the match deltas in ONE pass straight from the batch.  A record of
 * EITHER kind that is out of range after all is dropped on its own -- what a trusted turn applies never depends on
 * another record of the batch: every other match and vote record is applied, the sweep is adopted, every output is
 * filled in, and the call returns RAFTQ_EINVAL with "that record was dropped, every other record ... was applied" in
 * raftq_last_error().  Without the flag a turn is all-or-nothing. */
#define RAFTQ_CYCLE_TRUSTED 0x100u

typedef struct raftq raftq_t;

/* per-sweep tallies (reduced from per-wave partials when waited for) */
typedef struct raftq_counts {
  uint64_t n_changed; /* groups whose commit index advanced   */
  uint64_t n_won;     /* groups whose candidate reached quorum */
  uint64_t n_lost;    /* groups whose candidate was rejected by a quorum */
} raftq_counts_t;

/* one MsgAppResp-shaped update: peer `peer` of group `group` now matches
 * `match` (raft.go:268-270 -> Step -> Progress.maybeUpdate: only increases) */
typedef struct raftq_delta {
  uint64_t group;
  uint64_t match;
  uint32_t peer;
  uint32_t _pad;
} raftq_delta_t;

/* one MsgVoteResp-shaped update (first response from a peer wins, as poll) */
typedef struct raftq_vote_delta {
  uint64_t group;
  uint32_t peer;
  uint8_t vote; /* 1 granted, 2 rejected */
  uint8_t _pad[3];
} raftq_vote_delta_t;

/* one group whose leader entered a new term (or appended the first entry of
 * its term): updates the gate of raftLog.maybeCommit for that group */
typedef struct raftq_term_delta {
  uint64_t group;
  uint64_t cur_term;
  uint64_t first_idx_cur_term; /* 0 = no entry of cur_term in the log yet */
} raftq_term_delta_t;

/* one advanced group: what would surface in Ready.HardState.Commit */
typedef struct raftq_advance {
  uint64_t group;
  uint64_t old_commit;
  uint64_t new_commit;
} raftq_advance_t;

/* the same two records in 16 bytes, for handles of at most 2^32 groups (raftq_cycle_packed): the batching turn
 * is bound by PCIe both ways, and these are a third fewer bytes each way */
typedef struct raftq_delta16 {
  uint64_t match;
  uint32_t group;
  uint32_t peer;
} raftq_delta16_t;
typedef struct raftq_advance16 {
  uint64_t new_commit;
  uint32_t group;
  uint32_t advanced_by; /* new_commit - old_commit, saturated at 2^32 - 1 (then old_commit is not recoverable) */
} raftq_advance16_t;

/* ---- library / device ------------------------------------------------- */
int raftq_abi_version(void);
int raftq_device_count(int* n);
/* quorum size q = floor(N/2)+1  (etcd raft.q) -- host-side helper */
uint32_t raftq_quorum(uint32_t n_peers);

/* ---- handle lifetime --------------------------------------------------- */
/* allocates the padded SoA state for G groups x N peers in HBM on `device`;
 * everything starts zeroed (match 0, committed 0, no votes, no terms).
 * 1 <= n_groups <= RAFTQ_MAX_GROUPS (RAFTQ_EINVAL above): the bound is what the
 * parity suite has compared against the oracle on one handle (2^29 + 70001 groups,
 * tests/test_envelope_gpu.py), rounded up to the next power of two -- a larger
 * population is several handles (one sweep set), which is also how it shards. */
#define RAFTQ_MAX_GROUPS (1ull << 30)
int raftq_create(int device, uint64_t n_groups, uint32_t n_peers, raftq_t** out);
void raftq_destroy(raftq_t* h);
uint64_t raftq_groups(const raftq_t* h);
uint32_t raftq_peers(const raftq_t* h);
const char* raftq_last_error(const raftq_t* h); /* h may be NULL: global */

/* all handles default to their own non-blocking stream.  A caller that owns
 * streams (torch, a Go batching goroutine with one stream per device) can
 * install one; `stream` is a hipStream_t passed as void*. */
int raftq_set_stream(raftq_t* h, void* stream);
void* raftq_get_stream(const raftq_t* h);

/* ---- bulk load of resident state (host -> HBM) ------------------------- */
int raftq_load_match(raftq_t* h, const uint64_t* match /*[N][G]*/,
                     const uint64_t* committed /*[G]*/);
/* first_idx_cur_term[g] = first log index whose entry has term cur_term[g],
 * or 0 when the leader's log holds no entry of its current term yet. */
int raftq_load_terms(raftq_t* h, const uint64_t* cur_term /*[G]*/,
                     const uint64_t* first_idx_cur_term /*[G]*/);
int raftq_load_votes(raftq_t* h, const uint8_t* votes /*[N][G]*/);

/* ---- sparse ingest ----------------------------------- */
int raftq_apply_deltas(raftq_t* h, const raftq_delta_t* d, uint64_t n);
int raftq_apply_vote_deltas(raftq_t* h, const raftq_vote_delta_t* d, uint64_t n);
/* later records of the same group win (applied in order on the host side) */
int raftq_apply_term_deltas(raftq_t* h, const raftq_term_delta_t* d, uint64_t n);

/* ---- per-group voter sets ------------------------------------------------
 * A handle has N peer SLOTS; which of them vote is a property of each group.  etcd's q() is len(r.prs)/2 + 1 over the
 * group's own r.prs, which changes whenever a conf change is applied.  voters[g] is a 16-bit mask: bit p set = slot p is a
 * voting member of group g (a bit at or above N: RAFTQ_EINVAL).  With n_g = popcount(voters[g]) and q_g = n_g/2 + 1:
 *   - the commit candidate is the q_g-th largest match[p][g] over the voters only; raftLog.maybeCommit then runs as
 *     always (gated or not), and the commit index never decreases;
 *   - the tally counts granted and rejected over the voters only: won if granted >= q_g, else lost if rejected >= q_g,
 *     else pending.
 * Match and vote words of non-voters are stored, ingested and read back as always; the decisions ignore them.  An EMPTY
 * mask marks an unused group slot: its candidate is 0, so nothing commits, and its outcome stays pending (upstream has no
 * such state: a raft with no peers does not exist there).
 * With masks loaded, raftq_step_async / raftq_commit_advance / raftq_vote_tally / raftq_collect_changed / raftq_cycle /
 * raftq_cycle_packed run the masked sweep under every flag but RAFTQ_SWEEP_LDS (RAFTQ_EINVAL: the A/B variant has no masked
 * form).  Step (raftq_step.h / raftq_wire.h) runs over each group's own voters on a handle that opted in with
 * raftq_step_set_voters(h, 1) -- raftq_step_batch, raftq_step_submit / _collect, raftq_step_submit_packed, raftq_step_submit_wire,
 * raftq_step_frames / _frames_packed, raftq_apply_log_deltas / _nowait; raftq_step.h restates these rules for quorum(),
 * maybeCommit and poll -- and refuses a masked handle that did not (RAFTQ_ESTATE, the default).  Tick and the two rounds it
 * starts on the device have a switch of their own, raftq_tick_set_voters(h, 1) ("batched Tick" below): promotable() in
 * raftq_tick / raftq_tick_collect / raftq_tick_collect_lists, and raftq_tick_frames / raftq_tick_elect_frames (raftq_wire.h)
 * over each group's own members; without it Tick reads no mask and those two calls refuse a masked handle (RAFTQ_ESTATE, the
 * default).  The other two calls that build a broadcast on the device, raftq_step_frames_respond (the commit broadcast) and
 * raftq_propose_frames (bcastAppend), have the third switch, raftq_bcast_set_voters(h, 1) (raftq_wire.h): their MsgApps then go
 * to each group's own members, and a proposal whose append would move the commit index -- a one-voter group, a membership that
 * shrank -- is refused and pointed to raftq_apply_log_deltas; without it both refuse a masked handle (RAFTQ_ESTATE, the
 * default).  Sweep sets ("sweep sets" below) have a constructor of their own for this: a set from raftq_set_create_voters takes
 * masked members, lets raftq_load_voters / raftq_apply_voter_deltas change them while it lives, and sweeps and ticks every member
 * over its own voters; a set from raftq_set_create refuses a masked handle, and those two calls on one of its members, with
 * RAFTQ_ESTATE and a message that says so, whatever the switches say.  A handle with no masks loaded is exactly the handle it
 * always was, kernels included. */
typedef struct raftq_voter_delta {
  uint64_t group;
  uint16_t voters; /* the group's new mask */
  uint16_t reset;  /* slots whose Match is zeroed and whose vote is cleared: a slot reused for a new replica */
  uint32_t _pad;
} raftq_voter_delta_t;
/* The first membership of every group: the rpeers of raft.go:148-164 (StartNode(c, rpeers), itself a run of
 * ConfChangeAddNode entries).  voters[G]; NULL drops the masks: every slot votes again, the unmasked kernels. */
int raftq_load_voters(raftq_t* h, const uint16_t* voters);
/* Conf changes applied: the entries publishEntries passes by at raft.go:84-86, where upstream raftexample calls
 * ApplyConfChange.  Per record: the group's mask is replaced and, for every bit of `reset`, match[p][group] is zeroed and
 * peer p's vote cleared (deltas only ever raise Match: a reused slot must not inherit its predecessor's).  The last record
 * of a group wins.  All-or-nothing: one record with group >= G or a bit >= N and nothing is applied, RAFTQ_EINVAL.  On a
 * handle with no masks loaded the records change "every slot votes". */
int raftq_apply_voter_deltas(raftq_t* h, const raftq_voter_delta_t* d, uint64_t n);
/* the masks as the device holds them (r.prs of every group, raft.go:84-86 / 148-164); (1 << N) - 1 everywhere when none are
 * loaded.  voters_out[G]. */
int raftq_read_voters(raftq_t* h, uint16_t* voters_out);

/* ---- the sweep ---------------------------------------------------------- */
/* enqueue one pass over all G groups on the handle's stream. */
int raftq_step_async(raftq_t* h, unsigned flags);
/* block until everything enqueued on the handle has finished; if `counts` is
 * not NULL, fill it with the tallies of the most recent sweep. */
int raftq_wait(raftq_t* h, raftq_counts_t* counts);

/* synchronous conveniences = step_async + wait + optional read-back */
int raftq_commit_advance(raftq_t* h, int gated, uint64_t* committed_out /*[G]|NULL*/,
                         uint64_t* n_changed /*|NULL*/);
int raftq_vote_tally(raftq_t* h, uint8_t* outcome_out /*[G]|NULL*/,
                     raftq_counts_t* counts /*|NULL*/);

/* ---- read-back ---------------------------------------------------------- */
int raftq_read_committed(raftq_t* h, uint64_t* committed_out /*[G]*/);
int raftq_read_outcome(raftq_t* h, uint8_t* outcome_out /*[G]*/);
int raftq_read_match(raftq_t* h, uint64_t* match_out /*[N][G]*/);
/* the peer slot whose match row the device knows to be the largest of every
 * group (the sweep then does not read that row), or -1 when none is known. */
int raftq_self_max(raftq_t* h, int32_t* slot_out);
/* The narrow mirror: a per-group anchor (u64) and one 32-bit offset per match row, match[p][g] == anchor[g] + offset[p][g]
 * for every row of every group.  While the device knows that to hold, a commit sweep of 3 or more peers reads the mirror
 * (8 + 4N bytes a group) instead of the rows (8N).  raftq_load_match builds it; the batching turn's ingest keeps it true;
 * Step, a voter delta that resets a slot and an ack 2^32 or more above its group's anchor end it until the next build.
 * Costs 8 + 4N bytes a group; RAFTQ_NARROW=0 in the environment at raftq_create keeps a handle from ever having one.
 * raftq_narrow: *valid_out = 1 while the mirror holds, 0 otherwise.  raftq_narrow_rebuild: the build pass on demand (the
 * word stays 0 where a group's values spread over 2^32 or more, no memory can be had, or the handle was created without). */
int raftq_narrow(raftq_t* h, int32_t* valid_out);
int raftq_narrow_rebuild(raftq_t* h);
/* The tally mirror: one byte per group, tally[g] == granted | rejected << 4, the two counts poll() takes over the group's vote
 * word.  While the device knows that to hold, a sweep with RAFTQ_SWEEP_VOTES reads the byte (1 B a group) instead of the word
 * (2 B, 4 B at 9 peers) and compares the counts with the quorum itself.  Valid from raftq_create; raftq_load_votes rebuilds it,
 * the batching turn's vote ingest and raftq_campaign keep it true; Step and a voter delta that resets a slot end it until the
 * next build.  Costs 1 byte a group; RAFTQ_TALLY=0 in the environment at raftq_create keeps a handle from ever having one.
 * Sweeps of a handle with voter masks read the words either way.  Results never depend on it.
 * raftq_tally: *valid_out = 1 while the mirror holds, 0 otherwise.  raftq_tally_rebuild: the build pass on demand, then the
 * same answer in *valid_out (may be NULL; 0 where the handle was created without, or Step batches are in flight). */
int raftq_tally(raftq_t* h, int32_t* valid_out);
int raftq_tally_rebuild(raftq_t* h, int32_t* valid_out);
int raftq_read_votes(raftq_t* h, uint8_t* votes_out /*[N][G]*/);
/* compacted list of the groups the last RAFTQ_SWEEP_CHANGED sweep advanced,
 * in ascending group order; returns the count in *n (<= cap entries stored). */
int raftq_collect_changed(raftq_t* h, raftq_advance_t* out, uint64_t cap, uint64_t* n);

/* ---- batched Tick --------------------------------------
 * rc.node.Tick() (raft.go:223-224) for every group at once: etcd's
 * tickHeartbeat for leaders, tickElection + isElectionTimeout for the rest.
 * role: 0 follower, 1 candidate, 2 leader; action: 0 none, 1 MsgHup, 2 MsgBeat (3: a leader's failed check, only under
 * raftq_set_check_quorum, "CheckQuorum" below).
 * Timers default to the reference's ElectionTick 10 / HeartbeatTick 1
 * (raft.go:154-155).  The randomised election timeout draws from a
 * counter-based stream, not Go's math/rand (which cannot be reproduced
 * without the Go runtime).  The stream, exactly (round 6):
 *   key = fin64((seed ^ tick_no * 0xD1B54A32D192ED03) + 0x9E3779B97F4A7C15)   once per tick,
 *         fin64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
 *   rnd = fin32(lo32(group) ^ hi32(group) ^ lo32(key)) ^ hi32(key)             per group,
 *         fin32(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^ x >> 16
 * and a timer fires when elapsed - election_tick > rnd % election_tick
 * (etcd's isElectionTimeout with its rand.Int() replaced by rnd).
 *
 * promotable().  Upstream's tickElection begins `if !r.promotable() { r.elapsed = 0; return }`: a node that is not in a
 * group's r.prs never campaigns for it.  By default Tick reads no voter mask ("per-group voter sets" above) and a removed node
 * keeps raising MsgHup.  raftq_tick_set_voters(h, 1) opts the handle in: with masks loaded, raftq_tick, raftq_tick_collect,
 * raftq_tick_collect_lists and the Tick inside raftq_tick_frames / raftq_tick_elect_frames (raftq_wire.h) apply, with
 * mine = bit `self` (raftq_set_self, raftq_step.h) of voters[g]:
 *   a leader                    unchanged -- tickHeartbeat does not ask
 *   a non-leader, mine set      unchanged -- the same elapsed + 1, the same draw from the same stream, the same MsgHup
 *   a non-leader, mine clear    elapsed = 0, action 0, never flagged (an empty mask, an unused slot, is this case)
 * The masked Tick needs to know `self`: RAFTQ_ESTATE on a handle with neither raftq_set_self nor raftq_load_node.  The switch
 * also opens raftq_tick_frames and raftq_tick_elect_frames to a masked handle -- their rounds then go to each group's own
 * members.  0 is the default (Tick asks nobody, the two calls refuse a masked handle); anything but 0 or 1 is RAFTQ_EINVAL; the
 * handle must be idle (RAFTQ_ESTATE with a Step batch in flight).  A property of the handle: raftq_clone_state does not copy it
 * and raftq_load_voters(h, NULL) does not clear it; with no masks loaded the handle launches what it always did, whatever the
 * switch says.  Independent of raftq_step_set_voters.  raftq_set_tick applies the same rule member by member in a set from
 * raftq_set_create_voters ("sweep sets" below); in a set from raftq_set_create no member holds masks and nothing changes. */
#define RAFTQ_ROLE_FOLLOWER 0
#define RAFTQ_ROLE_CANDIDATE 1
#define RAFTQ_ROLE_LEADER 2
#define RAFTQ_ROLE_PRE_CANDIDATE 3 /* only under raftq_set_pre_vote ("PreVote" below) */
typedef struct raftq_tick_counts {
  uint64_t n_hup;  /* groups whose election timer fired: they campaign */
  uint64_t n_beat; /* leader groups due a heartbeat */
} raftq_tick_counts_t;
int raftq_set_timers(raftq_t* h, uint32_t election_tick, uint32_t heartbeat_tick, uint64_t seed);
int raftq_load_roles(raftq_t* h, const uint8_t* role /*[G]*/, const uint32_t* elapsed /*[G]|NULL = 0*/);
int raftq_tick_set_voters(raftq_t* h, int on);
/* one Tick for every group; synchronous when counts != NULL, else enqueued */
int raftq_tick(raftq_t* h, raftq_tick_counts_t* counts);
/* any of the outputs may be NULL */
int raftq_read_tick(raftq_t* h, uint8_t* action /*[G]*/, uint32_t* elapsed /*[G]*/, uint8_t* role /*[G]*/);
/* ascending list of the groups the last raftq_tick sent MsgHup to */
int raftq_collect_hups(raftq_t* h, uint64_t* groups, uint64_t cap, uint64_t* n);
/* ascending list of the leader groups the last raftq_tick sent MsgBeat to: they owe their followers a heartbeat
 * round (etcd tickHeartbeat -> Step(MsgBeat) -> bcastHeartbeat, reached from rc.node.Tick(), raft.go:223-224) */
int raftq_collect_beats(raftq_t* h, uint64_t* groups, uint64_t cap, uint64_t* n);
/* raftq_tick + both lists in one call: two launches and ONE wait (tick, then one kernel that ranks the MsgHup and the
 * MsgBeat bitmaps into two ascending lists), where raftq_tick + raftq_collect_hups + raftq_collect_beats are five
 * launches and two waits.  *n_hup / *n_beat receive the full counts even when they exceed the caps. */
int raftq_tick_collect(raftq_t* h, uint64_t* hups, uint64_t hup_cap, uint64_t* n_hup, uint64_t* beats, uint64_t beat_cap,
                       uint64_t* n_beat);

/* The same Tick + lists as they are meant to be read by a batching host: 4-byte group ids (a handle holds at most 2^30
 * groups) LEFT IN PLACE in page-locked memory -- nothing is copied into caller arrays -- and, with RAFTQ_TICK_BEAT_BITMAP,
 * the MsgBeat groups as a bitmap in group order (bit g % 64 of word g / 64) instead of a list: with HeartbeatTick 1
 * (raft.go:155) every leader owes a heartbeat on every tick, so the beat list IS the leader set, tick after tick.
 * n_hup / n_beat are the totals; at most hup_cap / beat_cap ids are listed (beat_cap is ignored with the bitmap).  Three
 * launches and one wait on the turn's completion word.  Stands in for rc.node.Tick() of every group (raft.go:223-224). */
#define RAFTQ_TICK_BEAT_BITMAP 1u
int raftq_tick_collect_lists(raftq_t* h, unsigned flags, uint64_t hup_cap, uint64_t beat_cap, uint64_t* n_hup, uint64_t* n_beat);
/* what the last raftq_tick_collect_lists left: ascending ids (valid until the next call of either on this handle); any
 * pointer argument may be NULL.  With the bitmap: *beats = NULL, *n_beats = 0, *bitmap_words = ceil(G / 64). */
int raftq_last_tick_lists(raftq_t* h, const uint32_t** hups, uint64_t* n_hups, const uint32_t** beats, uint64_t* n_beats,
                          const uint64_t** beat_bitmap, uint64_t* bitmap_words);
/* ---- CheckQuorum: the leader's lease (etcd/raft's checkQuorum, restated; PARITY UNPINNED) -------------------------------------
 * Upstream added checkQuorum after the 2015 API the reference vendors; what follows is the specification (CHOICE marks what
 * upstream has no counterpart for).  raftq_set_check_quorum(h, 1) opts the handle in: a leader that hears from less than a quorum
 * of its group for election_tick ticks steps down, and (raftq_step.h "CheckQuorum") a node under a live leader ignores a MsgVote
 * of a higher term.  0 is the default; anything but 0 or 1 is RAFTQ_EINVAL; the handle must be idle (RAFTQ_ESTATE with a Step
 * batch in flight).  A property of the handle: raftq_clone_state does not copy it.  Turning it on allocates the state below,
 * zeroed; turning it off frees it.
 *
 * The state, per group, on a handle that opted in: active[g], bit p set = Progress[p].RecentActive, and lead_elapsed[g], a
 * leader's electionElapsed (elapsed[g] is a leader's heartbeat counter).  The device keeps both in ONE 32-bit word, lead_elapsed in
 * 16 bits: with the switch on, raftq_set_check_quorum and raftq_set_timers refuse an election_tick above 65535 and
 * raftq_load_activity a lead_elapsed above it (RAFTQ_EINVAL).
 *
 * Tick.  With the switch on only raftq_tick runs, and like the masked Tick it needs to know `self` (RAFTQ_ESTATE on a handle with
 * neither raftq_set_self nor raftq_load_node).  For a leader group:
 *   1. the heartbeat side as always: v = elapsed + 1, a beat is due when v >= heartbeat_tick;
 *   2. le = lead_elapsed + 1; if le < election_tick, lead_elapsed = le and nothing more;
 *   3. otherwise lead_elapsed = 0 and act = popcount((active | 1 << self) & members) is held against q = popcount(members) / 2 + 1,
 *      members = voters[g] when raftq_tick_set_voters is on and masks are loaded, else all N slots (an empty mask: act 0 < q 1,
 *      the check fails -- CHOICE; a non-voter's bit is stored and does not count -- CHOICE, as its Match):
 *        pass   active = 0; the beat and the action byte are as always.  This is upstream's Step(MsgCheckQuorum) on a leader that
 *               keeps its quorum -- nothing changes but the bits -- done on the device: no message for a healthy group.
 *        fail   active stays; action 3, the group is listed by raftq_collect_checks, and NO beat is raised this tick: elapsed = v,
 *               the group is absent from the beat list and from n_beat.  The caller steps it with a RAFTQ_MSG_CHECK_QUORUM record
 *               (raftq_step.h), and Step applies the rule in full: an acknowledgement that lands in between saves the leader, as
 *               it would upstream.  Such a leader misses exactly one heartbeat (CHOICE); a check that is not stepped leaves the
 *               beat to the next tick.
 * A non-leader group ticks bit for bit as without the switch (promotable() included); its active and lead_elapsed do not change.
 * raftq_read_tick's action byte may be 3.  raftq_tick_counts_t keeps its two fields.
 *
 * What the switch closes (RAFTQ_ESTATE, "check quorum" in the text): raftq_tick_collect, raftq_tick_collect_lists,
 * raftq_tick_frames, raftq_tick_elect_frames (raftq_wire.h) and raftq_set_tick on a set holding such a member -- their beat lists
 * and device-built rounds do not know a suppressed beat.  raftq_campaign and raftq_load_roles do not touch the activity state.
 *
 * What raftq_tick_set_checks opens again.  raftq_tick_set_checks(h, chk_cap) with chk_cap > 0 opts a handle with the switch on back
 * in to four of them: raftq_tick_collect, raftq_tick_collect_lists, raftq_tick_frames and raftq_tick_elect_frames run the Tick above
 * (the same kernel raftq_tick launches) and leave the hup and beat results they always left.  A group whose check failed has action
 * 3 and NO beat: it is absent from the beat list, from the RAFTQ_TICK_BEAT_BITMAP bitmap, from *n_beat and from the heartbeat round.
 * The three in-place forms also leave the groups whose check failed as a THIRD list, raftq_last_tick_checks: the first
 * min(total, chk_cap) ids, ascending, 4 bytes each, in the same page-locked buffer as the hup and beat ids, valid until the next
 * call on the handle and covered by the one wait the call makes anyway.  Groups beyond chk_cap -- and every group after
 * raftq_tick_collect, the copying form, which has no slot for them -- come from raftq_collect_checks, which reads the bitmap of the
 * last Tick whichever call made it.  Every allocation of the third list is made before the Tick is enqueued: a call that fails has
 * not ticked.  raftq_tick_elect_frames' election round is then Step's own MsgHup arm under the switch (raftq_wire.h): a campaign's
 * reset() clears the activity word too.  chk_cap == 0 is the default: every call is as described above, refusal texts included.  No
 * effect while raftq_set_check_quorum is off.  The handle must be idle (RAFTQ_ESTATE with a Step batch in flight).  A property of
 * the handle: raftq_clone_state does not copy it.  raftq_set_tick keeps refusing a set that holds a member with the switch on. */
int raftq_set_check_quorum(raftq_t* h, int on);
int raftq_tick_set_checks(raftq_t* h, uint64_t chk_cap);
/* the third list of the last raftq_tick_collect_lists / raftq_tick_frames / raftq_tick_elect_frames under raftq_tick_set_checks:
 * *checks = the ids, *n_listed = min(*n_total, chk_cap), *n_total = the groups whose check failed in that Tick; any pointer argument
 * may be NULL.  RAFTQ_ESTATE when the last Tick call on the handle left no third list: none yet; a raftq_tick or raftq_tick_collect
 * since; a fused call made while the switch or raftq_set_check_quorum was off; raftq_tick_set_checks itself since. */
int raftq_last_tick_checks(raftq_t* h, const uint32_t** checks, uint64_t* n_listed, uint64_t* n_total);
/* bulk load / read-back ([G] each; either pointer may be NULL: that half is left alone / not read).  RAFTQ_ESTATE without the
 * switch; a bit at or above N, or a lead_elapsed above 65535: RAFTQ_EINVAL, nothing loaded.  raftq_clone_state copies the arrays
 * when both handles hold them. */
int raftq_load_activity(raftq_t* h, const uint16_t* active /*[G]|NULL*/, const uint32_t* lead_elapsed /*[G]|NULL*/);
int raftq_read_activity(raftq_t* h, uint16_t* active /*[G]|NULL*/, uint32_t* lead_elapsed /*[G]|NULL*/);
/* ascending list of the leader groups whose check the last raftq_tick found failing (action 3); raftq_collect_hups's contract.
 * *n = 0 with the switch off. */
int raftq_collect_checks(raftq_t* h, uint64_t* groups, uint64_t cap, uint64_t* n);

/* ---- PreVote: pre-elections, and an answer for a stale leader (etcd/raft's preVote, restated; PARITY UNPINNED) -----------------
 * CheckQuorum alone locks a node out for good: cut off, it campaigns and inflates its term; back again, its MsgVote of the higher
 * term is ignored under the lease and the leader's MsgApp / MsgHeartbeat of the lower term are dropped without an answer, so its
 * timer never resets and it campaigns again.  Upstream closed this with PreVote -- a pre-election at term + 1 that moves no term
 * until a quorum would grant -- and, under `checkQuorum || preVote`, a MsgAppResp that tells a stale leader the term it missed.
 * raftq_set_pre_vote(h, 1) opts the handle in to both; the rules are Step's (raftq_step.h "PreVote").  0 is the default; anything but
 * 0 or 1 is RAFTQ_EINVAL; the handle must be idle (RAFTQ_ESTATE with a Step batch in flight); a NULL handle is an error and no
 * device is touched.  A property of the handle: raftq_clone_state does not copy it.  It holds no state of its own.
 *
 * CHOICE: it requires CheckQuorum.  raftq_set_pre_vote(h, 1) on a handle without raftq_set_check_quorum is RAFTQ_ESTATE ("check
 * quorum" in the text), and raftq_set_check_quorum(h, 0) while it is on is RAFTQ_ESTATE ("pre vote").  Upstream's two options are
 * independent; here the hole PreVote closes exists only under the lease, the pair is what upstream recommends, and the rules stay
 * inside the walks a handle with the lease launches -- no new family of kernels.
 *
 * Roles.  raftq_load_roles accepts RAFTQ_ROLE_PRE_CANDIDATE with the switch on, and refuses it as any role above 2 otherwise.  The
 * Tick needs no change: every Tick kernel tests role == 2 alone, so a pre-candidate's election timer runs as a follower's does.
 * Turning the switch off leaves a role-3 group as it is: a Step without the switch takes it for a follower without a leader
 * (the last arm of its role test) until a message gives it another role.
 *
 * What the switch closes (RAFTQ_ESTATE, "pre vote" in the text): raftq_tick_elect_frames (raftq_wire.h), whose device-built round
 * makes a MsgHup a becomeCandidate and sends MsgVote (it is closed to CheckQuorum already).  raftq_campaign stays the real
 * becomeCandidate.  raftq_node does not turn the switch on.
 *
 * raftq_tick_set_checks(h, chk_cap > 0) ("CheckQuorum" above) opens raftq_tick_elect_frames under this switch as well: its round is
 * then Step's MsgHup arm with the switch on -- a pre-election: role 3, no term moves, camp[r] is RAFTQ_OUT_PRE_CAMPAIGN and the frames
 * are MsgPreVote at term + 1 (raftq_wire.h). */
int raftq_set_pre_vote(raftq_t* h, int on);

/* ---- Leadership transfer: MsgTransferLeader, MsgTimeoutNow (etcd/raft's leadTransferee, restated; PARITY UNPINNED) ----------------
 * Under the lease (raftq_set_check_quorum) a node under a live leader ignores a MsgVote of a higher term, so leadership cannot be
 * moved off a node on purpose: the only route is to kill it and wait out an election timeout.  Upstream's transfer avoids that: the
 * leader brings the transferee up to its tail and sends it MsgTimeoutNow; the transferee campaigns at once, with a MsgVote that is
 * marked as a transfer's and passes the lease.  raftq_set_lead_transfer(h, 1) opts the handle in; the rules are Step's (raftq_step.h
 * "Leadership transfer").  0 is the default; anything but 0 or 1 is RAFTQ_EINVAL; the handle must be idle (RAFTQ_ESTATE with a Step
 * batch in flight); a NULL handle is an error and no device is touched.  A property of the handle: raftq_clone_state does not copy it.
 *
 * CHOICE: it requires CheckQuorum.  raftq_set_lead_transfer(h, 1) on a handle without raftq_set_check_quorum is RAFTQ_ESTATE ("check
 * quorum" in the text), and raftq_set_check_quorum(h, 0) while it is on is RAFTQ_ESTATE ("lead transfer").  It is independent of
 * raftq_set_pre_vote.
 *
 * State.  leadTransferee[g] -- 0 = None, else peer slot + 1 -- is bits 12..15 of the activity word raftq_set_check_quorum allocated:
 * the activity bits stay in 0..8 (at most 9 peers, so a transferee of 9 fits in four bits), lead_elapsed in 16..31.  NO TICK KERNEL
 * CHANGES: tick_check_kernel already does what upstream's tickHeartbeat does.  A check that falls due and passes writes the whole word
 * 0 -- abortLeaderTransfer() at the election timeout; one that fails keeps the low half, and Step's RAFTQ_MSG_CHECK_QUORUM then clears
 * the low 16 bits whether the leader steps down or not; a check that is not due, and a non-leader, leave the low half alone; and the
 * check's popcount is over the members, at most 9 bits.  With the switch off no code path sets bits 12..15.
 *   raftq_read_activity never shows bits 12..15 in `active`; raftq_load_activity with `active` given keeps them as they are (a word
 *   that names a slot >= n_peers is refused as always).  raftq_set_lead_transfer(h, 0) clears them in every group.
 *   raftq_load_transfer / raftq_read_transfer: the transferees as one byte per group.  RAFTQ_ESTATE without the switch; a value
 *   above n_peers is RAFTQ_EINVAL and nothing is loaded.
 *   raftq_clone_state copies the word as it always has: the transferee travels with it.
 *
 * What the switch closes (RAFTQ_ESTATE, "lead transfer" in the text): raftq_propose_frames (raftq_wire.h) -- a leader must drop its
 * own proposals while a transfer is pending, and the proposal kernels do not read the word (a follow-up).  raftq_apply_log_deltas
 * stays the caller's responsibility: the caller knows of the transfer from RAFTQ_OUT_TRANSFER and can ask raftq_read_transfer.
 * Not modelled (CHOICE): a voter delta that removes the pending transferee does not abort the transfer; the Tick's timeout does.
 * raftq_node does not turn the switch on. */
int raftq_set_lead_transfer(raftq_t* h, int on);
int raftq_load_transfer(raftq_t* h, const uint8_t* transferee /*[G]*/);
int raftq_read_transfer(raftq_t* h, uint8_t* transferee /*[G]*/);

/* ---- ReadIndex: linearizable reads by a quorum of heartbeats (etcd/raft's ReadIndex, restated; PARITY UNPINNED) --------------------
 * A read that is linearizable without being written to the log: the leader notes its commit index, proves that it is still the
 * leader, and releases the read at that index.  The proof is a quorum of heartbeat acknowledgements that carry the request's
 * context (RAFTQ_READ_SAFE, upstream's ReadOnlySafe) or the CheckQuorum lease alone (RAFTQ_READ_LEASE, upstream's
 * ReadOnlyLeaseBased: no round trip, and only as safe as the clocks behind the lease).  raftq_set_read_index(h, mode) opts the handle
 * in; the rules are Step's (raftq_step.h "ReadIndex in Step").  0 is off, the default; anything but 0, 1 or 2 is RAFTQ_EINVAL; the
 * handle must be idle (RAFTQ_ESTATE with a Step batch in flight); a NULL handle is an error and no device is touched.  A property
 * of the handle: raftq_clone_state does not copy the switch.  Every change of mode zeroes the state below; mode 0 frees it.
 *
 * CHOICE, as for the last two switches: both modes require CheckQuorum.  raftq_set_read_index(h, 1 or 2) on a handle without
 * raftq_set_check_quorum is RAFTQ_ESTATE ("check quorum" in the text), and raftq_set_check_quorum(h, 0) while it is on is
 * RAFTQ_ESTATE ("read index").  The lease mode needs CheckQuorum as it does upstream; the safe mode requires it so that its rules
 * stay in the walks a handle with the lease launches.  Independent of raftq_set_pre_vote, raftq_set_lead_transfer,
 * raftq_step_set_props and the voter switches.
 *
 * State, RAFTQ_READ_SAFE only (RAFTQ_READ_LEASE holds none).  seq[g]: a 32-bit count of the read requests this leadership has
 * taken.  acked[p][g]: the largest of those numbers peer p has acknowledged.  Only Step touches it: one 64-byte record per group
 * {seq, acked[RAFTQ_MAX_PEERS], pad}, read only by a message that asks (a request, an acknowledgement with a context, a MsgBeat) and
 * written only where a word changed -- a batch with no read traffic and no reset() moves no byte of it, a reset() writes one zeroed
 * record.  confirmed(g) is not stored: it is the q-th largest of acked[p][g] over the group's members -- all N slots, or
 * voters[g] where Step runs over each group's own voters (raftq_step_set_voters; q_g = popcount / 2 + 1, an empty mask gives 0, a
 * non-voter's word is stored and does not count).
 *   raftq_load_reads: seq [G] and / or acked [N][G], NULL leaves that half alone.  RAFTQ_ESTATE unless the mode is RAFTQ_READ_SAFE;
 *   an acked word above its group's seq (the loaded one, or the one that stands) is RAFTQ_EINVAL and nothing is loaded.
 *   raftq_read_reads: seq [G], acked [N][G], confirmed [G], each optional.  confirmed is over the form Step launches on the handle:
 *   the masks under raftq_step_set_voters or raftq_bcast_set_voters, every slot otherwise.
 *   Both are set-up and test calls, not a hot path: the records cross the link in slices of 2^20 groups through 64 MB of pageable
 *   staging, whatever G is, and raftq_load_reads walks them twice (every slice is validated before the first is written).
 *   raftq_clone_state copies the records when both handles hold them.
 *
 * What the switch closes (RAFTQ_ESTATE, "read index" in the text), RAFTQ_READ_SAFE only: raftq_tick_frames and
 * raftq_tick_elect_frames (raftq_wire.h) -- their device-built heartbeats do not carry the pending read's context (a follow-up).
 * RAFTQ_READ_LEASE closes nothing.  raftq_node does not turn the switch on. */
#define RAFTQ_READ_SAFE 1
#define RAFTQ_READ_LEASE 2
int raftq_set_read_index(raftq_t* h, int mode);
int raftq_load_reads(raftq_t* h, const uint32_t* seq /*[G]|NULL*/, const uint32_t* acked /*[N][G]|NULL*/);
int raftq_read_reads(raftq_t* h, uint32_t* seq, uint32_t* acked, uint32_t* confirmed /*[G], each |NULL*/);

/* becomeCandidate for `n` distinct groups: role = candidate, elapsed = 0, votes
 * cleared, the candidate's own slot (`self_peer`) granted.  Term bookkeeping is
 * the caller's (raftq_apply_term_deltas). */
int raftq_campaign(raftq_t* h, const uint64_t* groups, uint64_t n, uint32_t self_peer);

/* ---- one batching iteration ----------------------------
 * What the single batching goroutine does per turn, fused into one call with
 * ONE host/device sync: scatter the MsgAppResp / MsgVoteResp deltas, sweep all
 * groups with `flags`, and return the compacted list of advanced groups (the
 * batched Ready.HardState.Commit).  Any of the arrays may be NULL with length 0;
 * `n_advanced` receives the full count even when it exceeds `cap`. */
int raftq_cycle(raftq_t* h, const raftq_delta_t* deltas, uint64_t n_deltas,
                const raftq_vote_delta_t* vote_deltas, uint64_t n_vote_deltas, unsigned flags,
                raftq_advance_t* advances_out, uint64_t cap, uint64_t* n_advanced,
                raftq_counts_t* counts);

/* zero-copy variants: raftq_stage returns the handle's ack buffer with room for the
 * given counts -- fine-grained DEVICE memory when the host can address it (large BAR:
 * the handlers' stores land in HBM as the acks arrive and the turn never pulls them
 * over PCIe), pinned device-visible host memory otherwise (or with RAFTQ_STAGE=host).
 * WRITE-ONLY for the host: reads of device memory over the BAR are uncached and slow.
 * Fill it and pass the SAME pointers to raftq_cycle and no staging copy is made.  They stay valid until the next
 * raftq_stage / raftq_apply_* / raftq_destroy on the handle.  With
 * advances_out == NULL and cap > 0, raftq_cycle leaves the advance list in
 * pinned memory; raftq_last_advances returns it (valid until the next
 * raftq_cycle / raftq_collect_changed). */
int raftq_stage(raftq_t* h, uint64_t n_deltas, uint64_t n_vote_deltas, raftq_delta_t** deltas,
                raftq_vote_delta_t** vote_deltas);
int raftq_last_advances(raftq_t* h, const raftq_advance_t** list, uint64_t* n_listed);

/* The batching turn -- one iteration of the Ready loop (raft.go:227-235) for every group -- with the 16-byte
 * records (handles of at most 2^32 groups).  Same semantics as raftq_cycle /
 * raftq_stage / raftq_last_advances; match deltas arrive as raftq_delta16_t, the advance list leaves as
 * raftq_advance16_t.  Without RAFTQ_CYCLE_TRUSTED a turn is all-or-nothing in either layout: one out-of-range record
 * of either kind and no record of the call is applied, the sweep it ran is not adopted, RAFTQ_EINVAL (with the flag:
 * see RAFTQ_CYCLE_TRUSTED above).  Arrays passed from the handle's ack buffer must have been staged with THIS call's
 * counts and layout (raftq_stage* with the same n_deltas / n_vote_deltas): RAFTQ_EINVAL otherwise. */
int raftq_cycle_packed(raftq_t* h, const raftq_delta16_t* deltas, uint64_t n_deltas,
                       const raftq_vote_delta_t* vote_deltas, uint64_t n_vote_deltas, unsigned flags,
                       raftq_advance16_t* advances_out, uint64_t cap, uint64_t* n_advanced,
                       raftq_counts_t* counts);
int raftq_stage_packed(raftq_t* h, uint64_t n_deltas, uint64_t n_vote_deltas, raftq_delta16_t** deltas,
                       raftq_vote_delta_t** vote_deltas);
int raftq_last_advances_packed(raftq_t* h, const raftq_advance16_t** list, uint64_t* n_listed);

/* RAFTQ_CYCLE_SEGMENTED on raftq_cycle_packed (advances_out == NULL, counts == NULL): the advance list may be left in SEGMENTS --
 * the turn's sweep writes the records of every tile of 1,024 groups itself, ascending, into that tile's own stretch of the
 * pinned list, and the compaction pass (a kernel, a boundary, 13 us of a 47 us turn) does not run: two kernels and the
 * completion word per turn instead of four.  Read them with raftq_last_advance_segments: segment s holds counts[s] records
 * at recs + s * stride, and walking the segments in order IS the ascending list raftq_last_advances_packed would have
 * returned (n_advanced is the same total).  A turn that cannot take that form (a vote tally or counts asked for, the list
 * copied out, the A/B sweep, a handle with voter masks loaded, a handle of more than 4M groups -- the pinned list has a slot per group) produces the contiguous
 * list as always, `cap` records of it at most, and raftq_last_advance_segments presents it as ONE segment: a consumer that
 * passes the flag reads segments, whatever happened (and compares counts[0] with n_advanced when there is one).  Valid until the next raftq_cycle* /
 * raftq_collect_changed on the handle. */
#define RAFTQ_CYCLE_SEGMENTED 0x200u
int raftq_last_advance_segments(raftq_t* h, const raftq_advance16_t** recs, const uint32_t** counts, uint32_t* n_segments,
                                uint64_t* stride);

/* ---- sweep sets: many handles, one dispatch --------------------------------
 * A host that runs more groups than it wants in one handle (several tenants, several
 * shards of one keyspace, 1M-group batches of a larger population) sweeps them together:
 * the G-fold Ready loop of raft.go:220-245 once more over K handles.  A set takes K
 * handles of one shape (same device, peer count and padded group count) and evaluates
 * them in ONE kernel launch (grid = tiles x K, the members' array pointers come from a
 * device-resident table), so the fixed cost of a launch boundary -- about a tenth of a
 * 1M x 5 sweep on MI355X -- is paid once per set instead of once per member.  Results
 * are exactly those of raftq_step_async on every member, and every per-handle call
 * (raftq_wait counts, raftq_read_*, raftq_collect_changed, raftq_apply_*) keeps working
 * on a member between set sweeps.
 *   - raftq_set_create re-homes every member onto the set's own stream (so member calls
 *     and set sweeps stay ordered); raftq_set_stream on a member is refused meanwhile;
 *     raftq_set_destroy gives every member a fresh stream back.  Destroy the set before
 *     its members (a member destroyed under a set makes the set refuse further calls).
 *   - flags are raftq_step_async's (RAFTQ_SWEEP_LDS excepted), applied to every member;
 *     a gated sweep needs terms loaded on every member.
 *   - like a handle, a set is not thread-safe, and its members must not be used from
 *     another thread while the set is.
 *   - voter masks ("per-group voter sets" above).  raftq_set_create refuses a handle with masks loaded, and its members
 *     refuse raftq_load_voters / raftq_apply_voter_deltas / raftq_clone_state from a masked source (RAFTQ_ESTATE).
 *     raftq_set_create_voters is raftq_set_create in every other respect -- the same shape rules, the same re-homing, the same
 *     refusals of null, duplicate, already-in-a-set and Step-in-flight members -- and admits them: members with and without
 *     masks may be mixed, and raftq_load_voters (NULL included), raftq_apply_voter_deltas and raftq_clone_state from a masked
 *     source are allowed on a member while the set lives.  raftq_set_sweep_async then leaves every member exactly as
 *     raftq_step_async(member, flags) would -- a masked member decides over its voters, an unmasked one over every slot:
 *     commit buffers, outcomes, the changed bitmap / raftq_collect_changed, the counts of raftq_set_wait and of raftq_wait.
 *     A dispatch in which no member holds masks launches exactly what a plain set launches (persistent mode, the narrow and
 *     the self-row bodies included); a dispatch with at least one masked member is one K-deep grid of the masked kernel, and
 *     RAFTQ_SET_PERSISTENT then runs that grid form too (there is no persistent masked walk).  RAFTQ_SWEEP_LDS stays refused.
 *     raftq_set_tick: a member with masks loaded and raftq_tick_set_voters on gets promotable() ("batched Tick" above) exactly
 *     as raftq_tick applies it, every other member -- no masks, or the switch off -- ticks as it always did, all in one
 *     dispatch; RAFTQ_TICK_SHAPE does not apply to a dispatch with such a member.  A switched-on masked member that does not
 *     know its self slot makes the call fail with RAFTQ_ESTATE before anything is launched: no member has ticked. */
typedef struct raftq_set raftq_set_t;
#define RAFTQ_SET_GRID 0       /* one K-deep grid: blockIdx.y = member (default) */
#define RAFTQ_SET_PERSISTENT 1 /* resident workgroups walk all K x tiles, next tile's loads in flight */
int raftq_set_create(raftq_t* const* handles, uint32_t n, raftq_set_t** out);
int raftq_set_create_voters(raftq_t* const* handles, uint32_t n, raftq_set_t** out);
void raftq_set_destroy(raftq_set_t* s);
uint32_t raftq_set_size(const raftq_set_t* s);
const char* raftq_set_last_error(const raftq_set_t* s); /* s may be NULL: global */
void* raftq_set_get_stream(const raftq_set_t* s);
/* launch shape of the set's sweeps; persist_workgroups 0 keeps the current / default count.  A dispatch with a masked member
 * (raftq_set_create_voters) runs the grid form whatever the mode. */
int raftq_set_mode(raftq_set_t* s, int mode, uint32_t persist_workgroups);
/* enqueue one pass over every member on the set's stream */
int raftq_set_sweep_async(raftq_set_t* s, unsigned flags);
/* one Tick of every group of every member as ONE dispatch, enqueued on the set's stream; each member is left exactly as
 * raftq_tick(member, NULL) would leave it (raftq_collect_hups / _beats / raftq_read_tick per member afterwards) */
int raftq_set_tick(raftq_set_t* s);
/* block until the set's stream is idle; tallies of each member's most recent sweep into
 * per_member[raftq_set_size] and / or their sum into *total (either may be NULL) */
int raftq_set_wait(raftq_set_t* s, raftq_counts_t* per_member, raftq_counts_t* total);
int raftq_set_timer_begin(raftq_set_t* s);
int raftq_set_timer_end(raftq_set_t* s, float* elapsed_ms);
/* the same K sweeps as K launches (raftq_step_async on every handle in turn, each on its
 * own stream): the host loop of a caller without a set, in one call.  Distinct handles that
 * share ONE stream (members of a set) are alternated between that stream and an auxiliary
 * one, forked and joined inside the call, so that consecutive launches overlap their
 * boundaries; everything is ordered behind / in front of the shared stream as before. */
int raftq_sweep_many_async(raftq_t* const* handles, uint32_t n, unsigned flags);
/* device-to-device copy of the quorum state (match, commit index, term gate, votes, voter masks)
 * of `src` into `dst` (same device, groups and peers): fork a population without a host
 * round trip.  `dst` ends with src's masks, or with none when src has none.  Tick / Step node
 * state is not copied. */
int raftq_clone_state(raftq_t* dst, raftq_t* src);

/* ---- measurement hooks (bench harness) --------------------------------- */
/* HIP events recorded on the handle's own stream, so the elapsed time covers
 * exactly the kernels enqueued between begin and end. */
int raftq_timer_begin(raftq_t* h);
int raftq_timer_end(raftq_t* h, float* elapsed_ms);

/* ---- page-locked host memory for the caller's bulk buffers ------------- */
/* Every entry point that takes or fills a caller-owned host buffer accepts any
 * memory; given a buffer from raftq_host_alloc the transfer is a direct DMA at
 * PCIe speed instead of a staged pageable copy (bulk loads, read-backs, the
 * wire / WAL codecs of raftq_wire.h).  Needs a GPU runtime: RAFTQ_ENODEV /
 * RAFTQ_ENOMEM otherwise.  A cgo caller wraps the pointer with unsafe.Slice;
 * the memory is not Go-managed, so the cgo pointer rules do not apply to it. */
int raftq_host_alloc(void** p, uint64_t bytes);
void raftq_host_free(void* p);

#ifdef __cplusplus
}
#endif
#endif /* RAFTQ_H */
