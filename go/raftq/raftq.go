// Package raftq is the cgo binding of libraftq.so (include/raftq.h): the
// MI355X batched quorum engine that stands in for the per-group
// maybeCommit / poll arithmetic raftsql reaches through raft.Node
// (reference raft.go:214, 224, 269).
//
// STATUS: SOURCE ONLY.  The build image has no Go toolchain, so this file has
// never been compiled or run; it documents the binding a maintainer would add
// (see INTEGRATION.md).  The tested host mirror is raftsql_amd/engine.py.
package raftq

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../raftsql_amd -lraftq -Wl,-rpath,${SRCDIR}/../../raftsql_amd
#include <stdlib.h>
#include <string.h>
#include "raftq.h"

// The handle-less error text (raftq_last_error(NULL), raftq_set_last_error(NULL)) is thread-local in the
// library, and a goroutine may change OS thread between two cgo calls.  These helpers make the failing call
// and the fetch of its text ONE cgo call, so the text always belongs to the call (ADVICE r01).
static int raftq_create_msg(int device, uint64_t groups, uint32_t peers, raftq_t** out, char* msg, size_t cap) {
  int rc = raftq_create(device, groups, peers, out);
  if (rc != RAFTQ_OK && cap) { strncpy(msg, raftq_last_error(NULL), cap - 1); msg[cap - 1] = 0; }
  return rc;
}
static int raftq_device_count_msg(int* n, char* msg, size_t cap) {
  int rc = raftq_device_count(n);
  if (rc != RAFTQ_OK && cap) { strncpy(msg, raftq_last_error(NULL), cap - 1); msg[cap - 1] = 0; }
  return rc;
}
static int raftq_set_create_msg(raftq_t* const* hs, uint32_t n, raftq_set_t** out, int voters, char* msg, size_t cap) {
  int rc = voters ? raftq_set_create_voters(hs, n, out) : raftq_set_create(hs, n, out);
  if (rc != RAFTQ_OK && cap) { strncpy(msg, raftq_set_last_error(NULL), cap - 1); msg[cap - 1] = 0; }
  return rc;
}
*/
import "C"

import (
	"errors"
	"fmt"
	"unsafe"
)

// Sweep flags (mirror RAFTQ_SWEEP_*).
const (
	SweepCommit  = 0x01
	SweepGated   = 0x02
	SweepVotes   = 0x04
	SweepNoAdopt = 0x08
	SweepLDS     = 0x10
	SweepChanged = 0x20
	SweepStream  = 0x40
	SweepCached  = 0x80
)

// Vote slot / outcome encodings.
const (
	VoteNone, VoteGranted, VoteRejected     = 0, 1, 2
	OutcomePending, OutcomeWon, OutcomeLost = 0, 1, 2
)

// Counts are the tallies of one sweep.
type Counts struct{ Changed, Won, Lost uint64 }

// Delta is one MsgAppResp-shaped update; layout-identical to raftq_delta_t.
type Delta struct {
	Group, Match uint64
	Peer, _      uint32
}

// VoteDelta is one MsgVoteResp-shaped update; layout-identical to raftq_vote_delta_t.
type VoteDelta struct {
	Group uint64
	Peer  uint32
	Vote  uint8
	_     [3]uint8
}

// Advance is one group whose commit index moved; layout-identical to raftq_advance_t.
type Advance struct{ Group, Old, New uint64 }

// Engine owns the resident quorum state of G groups x N peers on one GPU.
// Like raft.Node it must be driven from ONE goroutine.
type Engine struct {
	h      *C.raftq_t
	Groups uint64
	Peers  uint32
	// walBegun: a WalSaveBegin that enqueued something is waiting for its WalSaveEnd; walPrevCrc: what an End answers when the
	// Begin before it had no records (nothing was enqueued, the chain's CRC is where it was)
	walBegun   bool
	walPrevCrc uint32
}

func (e *Engine) err(rc C.int) error {
	if rc == C.RAFTQ_OK {
		return nil
	}
	return fmt.Errorf("raftq: %d: %s", int(rc), C.GoString(C.raftq_last_error(e.h)))
}

// DeviceCount reports the GPUs libraftq can see.
func DeviceCount() (int, error) {
	var n C.int
	var msg [256]C.char
	if rc := C.raftq_device_count_msg(&n, &msg[0], 256); rc != C.RAFTQ_OK {
		return 0, errors.New(C.GoString(&msg[0]))
	}
	return int(n), nil
}

// New allocates zeroed state for groups x peers on `device`.
func New(device int, groups uint64, peers uint32) (*Engine, error) {
	var h *C.raftq_t
	var msg [256]C.char
	if rc := C.raftq_create_msg(C.int(device), C.uint64_t(groups), C.uint32_t(peers), &h, &msg[0], 256); rc != C.RAFTQ_OK {
		return nil, fmt.Errorf("raftq: %d: %s", int(rc), C.GoString(&msg[0]))
	}
	return &Engine{h: h, Groups: groups, Peers: peers}, nil
}

// Close frees the device state.
func (e *Engine) Close() { C.raftq_destroy(e.h); e.h = nil }

// LoadMatch bulk-loads match[p*G+g] and committed[g]; either may be nil.
// The slices are only read during the call (cgo pointer rule).
func (e *Engine) LoadMatch(match, committed []uint64) error {
	var m, c *C.uint64_t
	if match != nil {
		m = (*C.uint64_t)(unsafe.Pointer(&match[0]))
	}
	if committed != nil {
		c = (*C.uint64_t)(unsafe.Pointer(&committed[0]))
	}
	return e.err(C.raftq_load_match(e.h, m, c))
}

// LoadTerms loads cur_term[g] and the first log index of that term (0 = none).
func (e *Engine) LoadTerms(curTerm, firstIdxCurTerm []uint64) error {
	return e.err(C.raftq_load_terms(e.h, (*C.uint64_t)(unsafe.Pointer(&curTerm[0])),
		(*C.uint64_t)(unsafe.Pointer(&firstIdxCurTerm[0]))))
}

// LoadVotes loads votes[p*G+g].
func (e *Engine) LoadVotes(votes []uint8) error {
	return e.err(C.raftq_load_votes(e.h, (*C.uint8_t)(unsafe.Pointer(&votes[0]))))
}

// ApplyDeltas scatters MsgAppResp updates (Progress.maybeUpdate: max).
func (e *Engine) ApplyDeltas(d []Delta) error {
	if len(d) == 0 {
		return nil
	}
	return e.err(C.raftq_apply_deltas(e.h, (*C.raftq_delta_t)(unsafe.Pointer(&d[0])), C.uint64_t(len(d))))
}

// ApplyVoteDeltas records MsgVoteResp answers (poll: first response wins).
func (e *Engine) ApplyVoteDeltas(d []VoteDelta) error {
	if len(d) == 0 {
		return nil
	}
	return e.err(C.raftq_apply_vote_deltas(e.h, (*C.raftq_vote_delta_t)(unsafe.Pointer(&d[0])), C.uint64_t(len(d))))
}

// StepAsync enqueues one sweep over all groups.
func (e *Engine) StepAsync(flags uint) error { return e.err(C.raftq_step_async(e.h, C.uint(flags))) }

// Wait blocks until the sweep is done and returns its tallies.
func (e *Engine) Wait() (Counts, error) {
	var c C.raftq_counts_t
	if err := e.err(C.raftq_wait(e.h, &c)); err != nil {
		return Counts{}, err
	}
	return Counts{uint64(c.n_changed), uint64(c.n_won), uint64(c.n_lost)}, nil
}

// CollectChanged returns the groups the last SweepChanged sweep advanced,
// ascending by group: the batched equivalent of Ready.HardState.Commit.
func (e *Engine) CollectChanged(buf []Advance) ([]Advance, uint64, error) {
	var n C.uint64_t
	var p *C.raftq_advance_t
	if len(buf) > 0 {
		p = (*C.raftq_advance_t)(unsafe.Pointer(&buf[0]))
	}
	if err := e.err(C.raftq_collect_changed(e.h, p, C.uint64_t(len(buf)), &n)); err != nil {
		return nil, 0, err
	}
	k := uint64(n)
	if k > uint64(len(buf)) {
		k = uint64(len(buf))
	}
	return buf[:k], uint64(n), nil
}

// ReadCommitted copies the current commit index of every group.
func (e *Engine) ReadCommitted(out []uint64) error {
	return e.err(C.raftq_read_committed(e.h, (*C.uint64_t)(unsafe.Pointer(&out[0]))))
}

// ReadOutcome copies the vote outcome of every group.
func (e *Engine) ReadOutcome(out []uint8) error {
	return e.err(C.raftq_read_outcome(e.h, (*C.uint8_t)(unsafe.Pointer(&out[0]))))
}

// ---- sweep sets (include/raftq.h "sweep sets"): K engines of one shape, ONE dispatch per sweep -------------

// Set launch shapes (mirror RAFTQ_SET_*).
const (
	SetGrid       = 0
	SetPersistent = 1
)

// Set sweeps its member engines with a single kernel launch.  Close the Set before its members.
type Set struct {
	s       *C.raftq_set_t
	Members []*Engine
}

// NewSet re-homes every member onto the set's stream (raftq_set_create).  No member may hold voter masks.
func NewSet(members []*Engine) (*Set, error) { return newSet(members, 0) }

// NewSetVoters is NewSet for members that may hold voter masks (raftq_set_create_voters): masked and unmasked members may be
// mixed, LoadVoters / ApplyVoterDeltas stay allowed on a member while the set lives, and SweepAsync and Tick treat every member
// as StepAsync and Tick on it alone would.
func NewSetVoters(members []*Engine) (*Set, error) { return newSet(members, 1) }

func newSet(members []*Engine, voters C.int) (*Set, error) {
	if len(members) == 0 {
		return nil, errors.New("raftq: empty set")
	}
	// the handle array lives in C memory: Go pointers to Go pointers must not cross cgo
	arr := (*[1 << 28]*C.raftq_t)(C.malloc(C.size_t(len(members)) * C.size_t(unsafe.Sizeof(uintptr(0)))))
	defer C.free(unsafe.Pointer(arr))
	for i, e := range members {
		arr[i] = e.h
	}
	var s *C.raftq_set_t
	var msg [256]C.char
	if rc := C.raftq_set_create_msg((**C.raftq_t)(unsafe.Pointer(arr)), C.uint32_t(len(members)), &s, voters, &msg[0], 256); rc != C.RAFTQ_OK {
		return nil, fmt.Errorf("raftq: %d: %s", int(rc), C.GoString(&msg[0]))
	}
	return &Set{s: s, Members: members}, nil
}

func (s *Set) err(rc C.int) error {
	if rc == C.RAFTQ_OK {
		return nil
	}
	return fmt.Errorf("raftq: %d: %s", int(rc), C.GoString(C.raftq_set_last_error(s.s)))
}

// Close gives every member a stream of its own back (raftq_set_destroy).
func (s *Set) Close() { C.raftq_set_destroy(s.s); s.s = nil }

// Mode selects the launch shape; workgroups 0 keeps the default residency of the persistent walk.
func (s *Set) Mode(mode int, workgroups uint32) error {
	return s.err(C.raftq_set_mode(s.s, C.int(mode), C.uint32_t(workgroups)))
}

// SweepAsync enqueues one pass over every member: the G-fold Ready loop of raft.go:220-245, K-fold.
func (s *Set) SweepAsync(flags uint) error { return s.err(C.raftq_set_sweep_async(s.s, C.uint(flags))) }

// Wait blocks until the set's stream is idle; perMember (len == members, or nil) and total receive the tallies.
func (s *Set) Wait(perMember []Counts, total *Counts) error {
	var pm *C.raftq_counts_t
	if perMember != nil {
		pm = (*C.raftq_counts_t)(unsafe.Pointer(&perMember[0]))
	}
	return s.err(C.raftq_set_wait(s.s, pm, (*C.raftq_counts_t)(unsafe.Pointer(total))))
}

// SweepMany is the same K sweeps as K launches (raftq_sweep_many_async): for callers without a Set.
func SweepMany(engines []*Engine, flags uint) error {
	for _, e := range engines {
		if err := e.StepAsync(flags); err != nil {
			return err
		}
	}
	return nil
}

// CloneStateFrom copies src's quorum state device-to-device (raftq_clone_state).
func (e *Engine) CloneStateFrom(src *Engine) error { return e.err(C.raftq_clone_state(e.h, src.h)) }

// CollectBeats lists the leader groups the last Tick sent MsgBeat to (raftq_collect_beats).
func (e *Engine) CollectBeats(out []uint64) (uint64, error) {
	var n C.uint64_t
	var p *C.uint64_t
	if len(out) > 0 {
		p = (*C.uint64_t)(unsafe.Pointer(&out[0]))
	}
	rc := C.raftq_collect_beats(e.h, p, C.uint64_t(len(out)), &n)
	return uint64(n), e.err(rc)
}

// SetCheckQuorum opts the engine in to (or out of) upstream's checkQuorum (raftq_set_check_quorum; include/raftq.h "CheckQuorum"):
// Tick then runs the leader's periodic check -- a group that fails it gets action 3, raises no beat that tick and is listed by
// CollectChecks; step it with a Msg of type MsgCheckQuorum and Step decides (OutNone with OutfSteppedDown when the leader has
// heard from less than a quorum) -- Step records which peers answered, and a node under a live leader ignores a MsgVote of a
// higher term.  TickCollect, TickCollectLists, TickFrames, TickElectFrames and Set.Tick return ErrState while it is on.  Needs
// SetSelf; election_tick must fit 16 bits.  A property of the engine; no batch may be in flight.
func (e *Engine) SetCheckQuorum(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	return e.err(C.raftq_set_check_quorum(e.h, v))
}

// SetPreVote opts the engine in to (or out of) upstream's preVote (raftq_set_pre_vote; include/raftq.h "PreVote"): Step's MsgHup
// then starts a pre-election -- role RolePreCandidate, OutPreCampaign, no term moves until a quorum of MsgPreVoteResp grants --, Msgs
// of type MsgPreVote / MsgPreVoteResp are stepped, and a stale leader's MsgApp / MsgHeartbeat is answered OutTermResp.  Requires
// SetCheckQuorum(true) (ErrState otherwise, and SetCheckQuorum(false) returns ErrState while it is on); TickElectFrames returns
// ErrState meanwhile.  A property of the engine; no batch may be in flight.
func (e *Engine) SetPreVote(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	return e.err(C.raftq_set_pre_vote(e.h, v))
}

// SetLeadTransfer opts the engine in to (or out of) upstream's leadership transfer (raftq_set_lead_transfer; include/raftq.h
// "Leadership transfer"): Msgs of type MsgTransferLeader / MsgTimeoutNow are stepped, a MsgVote with Reject = 1 is a transfer's and
// passes the lease, a leader with a transfer pending drops MsgProp.  Requires SetCheckQuorum(true) (ErrState otherwise, and
// SetCheckQuorum(false) returns ErrState while it is on); ProposeFrames returns ErrState meanwhile.  A property of the engine; no
// batch may be in flight.  Turning it off clears every pending transferee.
func (e *Engine) SetLeadTransfer(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	return e.err(C.raftq_set_lead_transfer(e.h, v))
}

// LoadTransfer sets every group's leadTransferee: 0 = None, else peer slot + 1 (raftq_load_transfer).
func (e *Engine) LoadTransfer(transferee []uint8) error {
	if uint64(len(transferee)) != e.Groups || e.Groups == 0 {
		return errors.New("raftq: LoadTransfer: transferee must hold G bytes")
	}
	return e.err(C.raftq_load_transfer(e.h, (*C.uint8_t)(unsafe.Pointer(&transferee[0]))))
}

// ReadTransfer reads every group's leadTransferee (raftq_read_transfer).
func (e *Engine) ReadTransfer(transferee []uint8) error {
	if uint64(len(transferee)) != e.Groups || e.Groups == 0 {
		return errors.New("raftq: ReadTransfer: transferee must hold G bytes")
	}
	return e.err(C.raftq_read_transfer(e.h, (*C.uint8_t)(unsafe.Pointer(&transferee[0]))))
}

// Read modes of SetReadIndex (raftq_set_read_index; include/raftq.h "ReadIndex").
const (
	ReadOff   = 0
	ReadSafe  = C.RAFTQ_READ_SAFE  // a read waits for a quorum of heartbeat acknowledgements that carry its sequence number
	ReadLease = C.RAFTQ_READ_LEASE // the CheckQuorum lease releases it at once
)

// SetReadIndex opts the engine in to (or, with ReadOff, out of) upstream's ReadIndex: Msgs of type MsgReadIndex / MsgReadIndexResp
// are stepped, a leader answers OutReadIndex, a heartbeat's Index carries a read's context and is echoed.  Requires
// SetCheckQuorum(true) (ErrState otherwise, and SetCheckQuorum(false) returns ErrState while it is on); with ReadSafe TickFrames and
// TickElectFrames return ErrState meanwhile.  A property of the engine; no batch may be in flight.  Every change of mode zeroes the
// read records.
func (e *Engine) SetReadIndex(mode int) error {
	v := C.int(mode)
	return e.err(C.raftq_set_read_index(e.h, v))
}

// LoadReads sets every group's read record: seq [G], acked [N][G]; nil leaves that half alone (raftq_load_reads, ReadSafe only).
func (e *Engine) LoadReads(seq []uint32, acked []uint32) error {
	var s *C.uint32_t
	var a *C.uint32_t
	if seq != nil {
		s = (*C.uint32_t)(unsafe.Pointer(&seq[0]))
	}
	if acked != nil {
		a = (*C.uint32_t)(unsafe.Pointer(&acked[0]))
	}
	return e.err(C.raftq_load_reads(e.h, s, a))
}

// ReadReads copies them back with confirmed [G], the q-th largest acknowledgement over each group's members; any slice may be nil
// (raftq_read_reads).
func (e *Engine) ReadReads(seq []uint32, acked []uint32, confirmed []uint32) error {
	var s *C.uint32_t
	var a *C.uint32_t
	var c *C.uint32_t
	if seq != nil {
		s = (*C.uint32_t)(unsafe.Pointer(&seq[0]))
	}
	if acked != nil {
		a = (*C.uint32_t)(unsafe.Pointer(&acked[0]))
	}
	if confirmed != nil {
		c = (*C.uint32_t)(unsafe.Pointer(&confirmed[0]))
	}
	return e.err(C.raftq_read_reads(e.h, s, a, c))
}

// LoadActivity sets every group's activity word (bit p = peer slot p answered since the last check) and / or every leader's
// electionElapsed; nil leaves that half alone (raftq_load_activity).
func (e *Engine) LoadActivity(active []uint16, leadElapsed []uint32) error {
	var a *C.uint16_t
	var l *C.uint32_t
	if active != nil {
		a = (*C.uint16_t)(unsafe.Pointer(&active[0]))
	}
	if leadElapsed != nil {
		l = (*C.uint32_t)(unsafe.Pointer(&leadElapsed[0]))
	}
	return e.err(C.raftq_load_activity(e.h, a, l))
}

// ReadActivity copies them back; either slice may be nil (raftq_read_activity).
func (e *Engine) ReadActivity(active []uint16, leadElapsed []uint32) error {
	var a *C.uint16_t
	var l *C.uint32_t
	if active != nil {
		a = (*C.uint16_t)(unsafe.Pointer(&active[0]))
	}
	if leadElapsed != nil {
		l = (*C.uint32_t)(unsafe.Pointer(&leadElapsed[0]))
	}
	return e.err(C.raftq_read_activity(e.h, a, l))
}

// CollectChecks lists the leader groups whose check the last Tick found failing (raftq_collect_checks); 0 with the switch off.
func (e *Engine) CollectChecks(out []uint64) (uint64, error) {
	var n C.uint64_t
	var p *C.uint64_t
	if len(out) > 0 {
		p = (*C.uint64_t)(unsafe.Pointer(&out[0]))
	}
	rc := C.raftq_collect_checks(e.h, p, C.uint64_t(len(out)), &n)
	return uint64(n), e.err(rc)
}

// VoterDelta is one applied conf change of one group (raftq_voter_delta_t: group, the new voter mask, the slots to reset).
// Voters bit p set = peer slot p votes in the group; Reset bit p set = the slot's Match is zeroed and its vote cleared.
type VoterDelta struct {
	Group  uint64
	Voters uint16
	Reset  uint16
	_      uint32
}

// LoadVoters sets every group's voter mask: the rpeers StartNode is given (raft.go:148-164).  nil drops the masks, and
// every slot votes in every group again (raftq_load_voters).
func (e *Engine) LoadVoters(voters []uint16) error {
	var p *C.uint16_t
	if voters != nil {
		p = (*C.uint16_t)(unsafe.Pointer(&voters[0]))
	}
	return e.err(C.raftq_load_voters(e.h, p))
}

// ApplyVoterDeltas applies conf changes: what ApplyConfChange does for the entries publishEntries passes by (raft.go:84-86).
// The last record of a group wins; one bad record and nothing is applied (raftq_apply_voter_deltas).
func (e *Engine) ApplyVoterDeltas(d []VoterDelta) error {
	if len(d) == 0 {
		return nil
	}
	return e.err(C.raftq_apply_voter_deltas(e.h, (*C.raftq_voter_delta_t)(unsafe.Pointer(&d[0])), C.uint64_t(len(d))))
}

// ReadVoters copies every group's voter mask; all N bits everywhere when none are loaded (raftq_read_voters).
func (e *Engine) ReadVoters(out []uint16) error {
	return e.err(C.raftq_read_voters(e.h, (*C.uint16_t)(unsafe.Pointer(&out[0]))))
}
