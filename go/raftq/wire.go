// wire.go -- cgo binding of include/raftq_wire.h: batched raftpb.Message stream frames and
// walpb.Record WAL frames, and Step fed straight from received frames.
//
// SOURCE ONLY: never compiled or run (no Go toolchain in the build image; see README.md).
// It is the binding INTEGRATION.md section 4 describes: where a G-group raftsql would call
// it instead of G x rc.transport.Send / rc.wal.Save / w.ReadAll (raft.go:230, :228, :124).
package raftq

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../raftsql_amd -lraftq -Wl,-rpath,${SRCDIR}/../../raftsql_amd
#include "raftq_wire.h"
*/
import "C"

import (
	"fmt"
	"unsafe"
)

// WireMsg is layout-identical to raftq_wire_msg_t (64 bytes); its first fields are Msg's, so a
// decoded slice can be reinterpreted as []Msg for StepBatch.
type WireMsg struct {
	Group, Term, LogTerm, Index, Commit, RejectHint uint64
	From                                            uint32 // peer slot = raft ID - 1
	Type, Reject, To, Flags                         uint8
	EntFirst, NEnts                                 uint32
}

// WireEnt is layout-identical to raftq_wire_ent_t (32 bytes).
type WireEnt struct {
	Term, Index, DataOff uint64
	DataLen, Type        uint32
}

// WalRec is layout-identical to raftq_wal_rec_t (48 bytes).
type WalRec struct {
	Group, Term, Index, DataOff uint64
	DataLen, Vote, Crc          uint32
	Kind, EntryType, Flags, _   uint8
}

const (
	WireMalformed = C.RAFTQ_WIRE_F_MALFORMED
	WireSnapshot  = C.RAFTQ_WIRE_F_SNAPSHOT
	WireGroup     = C.RAFTQ_WIRE_F_GROUP

	WalMetadata = C.RAFTQ_WAL_METADATA
	WalEntry    = C.RAFTQ_WAL_ENTRY
	WalState    = C.RAFTQ_WAL_STATE
	WalCrc      = C.RAFTQ_WAL_CRC
	WalSnapshot = C.RAFTQ_WAL_SNAPSHOT

	WalFMalformed = C.RAFTQ_WAL_F_MALFORMED
	WalFBadCRC    = C.RAFTQ_WAL_F_BADCRC // wal.ErrCRCMismatch
)

func bytesPtr(b []byte) unsafe.Pointer {
	if len(b) == 0 {
		return nil
	}
	return unsafe.Pointer(&b[0])
}

// HostAlloc returns page-locked memory (raftq_host_alloc): buffers handed to the calls below
// from it move by direct DMA.  Not Go-managed memory: free it with HostFree.
func HostAlloc(n int) ([]byte, error) {
	var p unsafe.Pointer
	if rc := C.raftq_host_alloc(&p, C.uint64_t(n)); rc != C.RAFTQ_OK {
		return nil, fmt.Errorf("raftq: %d: %s", int(rc), C.GoString(C.raftq_last_error(nil)))
	}
	return unsafe.Slice((*byte)(p), n), nil
}

func HostFree(b []byte) {
	if len(b) != 0 {
		C.raftq_host_free(unsafe.Pointer(&b[0]))
	}
}

// EncodeMessages marshals msgs (entries in ents, payloads in pool) into rafthttp stream frames in
// out -- what messageEncoder.encode does per message behind rc.transport.Send(rd.Messages)
// (raft.go:230).  frameOff (len(msgs)+1, or nil) receives the frame boundaries.  If out is too
// small the error is returned and `need` says how many bytes are required.
func (e *Engine) EncodeMessages(msgs []WireMsg, ents []WireEnt, pool, out []byte, frameOff []uint64) (need uint64, err error) {
	if len(msgs) == 0 {
		return 0, nil
	}
	var c C.raftq_wire_counts_t
	var pe *C.raftq_wire_ent_t
	if len(ents) > 0 {
		pe = (*C.raftq_wire_ent_t)(unsafe.Pointer(&ents[0]))
	}
	var po *C.uint64_t
	if len(frameOff) > len(msgs) {
		po = (*C.uint64_t)(unsafe.Pointer(&frameOff[0]))
	}
	rc := C.raftq_wire_encode(e.h, (*C.raftq_wire_msg_t)(unsafe.Pointer(&msgs[0])), C.uint64_t(len(msgs)), pe,
		C.uint64_t(len(ents)), bytesPtr(pool), C.uint64_t(len(pool)), bytesPtr(out), C.uint64_t(len(out)), po, &c)
	return uint64(c.bytes), e.err(rc)
}

// ScanFrames walks the length words of buf (bigEndian: rafthttp streams; little: WAL files) and
// returns the boundaries of the whole frames and the bytes they cover; a torn tail stays with the caller.
func ScanFrames(buf []byte, bigEndian bool, off []uint64) (frames int, consumed uint64) {
	if len(off) < 2 {
		return 0, 0
	}
	be := C.int(0)
	if bigEndian {
		be = 1
	}
	var n, used C.uint64_t
	C.raftq_wire_scan_frames(bytesPtr(buf), C.uint64_t(len(buf)), be, (*C.uint64_t)(unsafe.Pointer(&off[0])),
		C.uint64_t(len(off)-1), &n, &used)
	return int(n), uint64(used)
}

// DecodeMessages unmarshals the frames of stream delimited by frameOff into msgs (len(frameOff)-1)
// and their entry headers into ents; Entry.Data stays in stream (WireEnt.DataOff points into it).
func (e *Engine) DecodeMessages(stream []byte, frameOff []uint64, msgs []WireMsg, ents []WireEnt) (nEnts, nMalformed uint64, err error) {
	n := len(frameOff) - 1
	if n <= 0 {
		return 0, 0, nil
	}
	var c C.raftq_wire_counts_t
	var pe *C.raftq_wire_ent_t
	if len(ents) > 0 {
		pe = (*C.raftq_wire_ent_t)(unsafe.Pointer(&ents[0]))
	}
	rc := C.raftq_wire_decode(e.h, bytesPtr(stream), C.uint64_t(len(stream)), (*C.uint64_t)(unsafe.Pointer(&frameOff[0])),
		C.uint64_t(n), (*C.raftq_wire_msg_t)(unsafe.Pointer(&msgs[0])), pe, C.uint64_t(len(ents)), &c)
	return uint64(c.n_ents), uint64(c.n_malformed), e.err(rc)
}

// StepSubmitWire is raftNode.Process (raft.go:268-270) for a whole receive buffer: the frames are
// unmarshalled on the GPU and stepped there; collect with StepCollect as for StepSubmit.
func (e *Engine) StepSubmitWire(stream []byte, frameOff []uint64) error {
	n := len(frameOff) - 1
	if n <= 0 {
		return nil
	}
	return e.err(C.raftq_step_submit_wire(e.h, bytesPtr(stream), C.uint64_t(len(stream)),
		(*C.uint64_t)(unsafe.Pointer(&frameOff[0])), C.uint64_t(n)))
}

// StepWireMsgs / StepWireEntries: the decoded records of the batch just collected (MsgApp entry
// ranges for the log's owner); valid until the next submit into that slot.
func (e *Engine) StepWireMsgs() ([]WireMsg, error) {
	var p *C.raftq_wire_msg_t
	var n C.uint64_t
	if rc := C.raftq_step_wire_msgs(e.h, &p, &n); rc != C.RAFTQ_OK {
		return nil, e.err(rc)
	}
	return unsafe.Slice((*WireMsg)(unsafe.Pointer(p)), int(n)), nil
}

func (e *Engine) StepWireEntries() ([]WireEnt, error) {
	var p *C.raftq_wire_ent_t
	var n C.uint64_t
	if rc := C.raftq_step_wire_entries(e.h, &p, &n); rc != C.RAFTQ_OK {
		return nil, e.err(rc)
	}
	return unsafe.Slice((*WireEnt)(unsafe.Pointer(p)), int(n)), nil
}

// WalSave is rc.wal.Save(rd.HardState, rd.Entries) (raft.go:228) for every group's Ready at once:
// recs in order (a STATE record per dirty HardState, an ENTRY record per entry), appended to a
// segment whose running CRC is prevCrc.  Returns the bytes to write and the CRC to carry on.
func (e *Engine) WalSave(recs []WalRec, pool []byte, prevCrc uint32, out []byte) (n uint64, lastCrc uint32, err error) {
	if len(recs) == 0 {
		return 0, prevCrc, nil
	}
	var c C.raftq_wal_counts_t
	rc := C.raftq_wal_encode(e.h, (*C.raftq_wal_rec_t)(unsafe.Pointer(&recs[0])), C.uint64_t(len(recs)), bytesPtr(pool),
		C.uint64_t(len(pool)), C.uint32_t(prevCrc), bytesPtr(out), C.uint64_t(len(out)), nil, &c)
	return uint64(c.bytes), uint32(c.last_crc), e.err(rc)
}

// WalReadAll is w.ReadAll() (raft.go:124) for the frames of a segment: records parsed, the CRC
// chain recomputed and compared.  valid < len(recs) is where the reference would log.Fatalf
// (raft.go:126): recs[valid].Flags says whether it did not parse or its CRC mismatched.
func (e *Engine) WalReadAll(data []byte, frameOff []uint64, prevCrc uint32, recs []WalRec) (valid uint64, lastCrc uint32, err error) {
	n := len(frameOff) - 1
	if n <= 0 {
		return 0, prevCrc, nil
	}
	var c C.raftq_wal_counts_t
	rc := C.raftq_wal_decode(e.h, bytesPtr(data), C.uint64_t(len(data)), (*C.uint64_t)(unsafe.Pointer(&frameOff[0])),
		C.uint64_t(n), C.uint32_t(prevCrc), (*C.raftq_wal_rec_t)(unsafe.Pointer(&recs[0])), &c)
	return uint64(c.n_valid), uint32(c.last_crc), e.err(rc)
}

// StepStageWire returns the arrays the next StepSubmitWire will take, with room for nCap frames and nbytesCap stream
// bytes (raftq_step_stage_wire): device memory behind a large BAR -- fill them in place and submit slices of them.
func (e *Engine) StepStageWire(nCap, nbytesCap int) (frameOff []uint64, stream []byte, err error) {
	var po *C.uint64_t
	var ps unsafe.Pointer
	if rc := C.raftq_step_stage_wire(e.h, C.uint64_t(nCap), C.uint64_t(nbytesCap), &po, &ps); rc != C.RAFTQ_OK {
		return nil, nil, e.err(rc)
	}
	return unsafe.Slice((*uint64)(unsafe.Pointer(po)), nCap+1), unsafe.Slice((*byte)(ps), nbytesCap), nil
}

// StepFrames is a node's inbound half of a turn as ONE submission and one wait (raftq_step_frames): rafthttp's decoder, the
// checks a node makes on what it received and rc.node.Step (raft.go:268-270) for every frame, in arrival order.  The decoder
// says in every record's flag byte what Step made of it: a frame that is nobody's is skipped (OutSkipped), a MsgProp is
// held for the log's owner (OutHeld, the rest of its group OutDeferred), a MsgApp is a barrier that says what it carries.
// msgs / ents / stream / frameOff must be page-locked (HostAlloc).  Results: StepResults(), one per frame.  nEnts may exceed
// len(ents): the frames have been stepped all the same, WireDecode fetches the remaining headers.
func (e *Engine) StepFrames(stream []byte, frameOff []uint64, tailAppends bool, msgs []WireMsg, ents []WireEnt) (nEnts, nMalformed uint64, err error) {
	n := len(frameOff) - 1
	if n <= 0 {
		return 0, 0, nil
	}
	if len(msgs) < n {
		return 0, 0, fmt.Errorf("raftq: StepFrames: %d frames, room for %d records", n, len(msgs))
	}
	var pe *C.raftq_wire_ent_t
	if len(ents) > 0 {
		pe = (*C.raftq_wire_ent_t)(unsafe.Pointer(&ents[0]))
	}
	ta := C.int(0)
	if tailAppends {
		ta = 1
	}
	var c C.raftq_wire_counts_t
	rc := C.raftq_step_frames(e.h, bytesPtr(stream), C.uint64_t(len(stream)), (*C.uint64_t)(unsafe.Pointer(&frameOff[0])), C.uint64_t(n), ta,
		(*C.raftq_wire_msg_t)(unsafe.Pointer(&msgs[0])), pe, C.uint64_t(len(ents)), &c)
	return uint64(c.n_ents), uint64(c.n_malformed), e.err(rc)
}

// WireMsg40 / WireHead: the decoder's narrow records (raftq_wire_msg40_t -- Msg40's layout with the flags in its pad byte --
// and raftq_wire_head_t, include/raftq_wire.h).  A record whose Flags carry WireWide stands for a frame whose full WireMsg is
// in wide[]; in WireMsg40 its Aux is the position there.
type WireMsg40 struct {
	Group  uint32
	From   uint8 // 0xFF = absent
	Type   uint8
	Reject uint8
	Flags  uint8
	Term   uint64
	Index  uint64
	Aux    uint64 // RejectHint on MsgAppResp, LogTerm on every other kind, the position in wide[] under WireWide
	Commit uint64
}

type WireHead struct {
	Group  uint32
	From   uint8
	Type   uint8
	Reject uint8
	Flags  uint8
}

// WireWide / WireForm40 / WireFormHead: RAFTQ_WIRE_F_WIDE, RAFTQ_WIRE_FORM_40, RAFTQ_WIRE_FORM_HEAD
const (
	WireWide     = 0x08
	WireForm40   = 40
	WireFormHead = 8
)

// narrowPtr: the narrow array of a packed call (exactly one of n40 / heads is used, by form) and the check that it holds n records
func narrowPtr(who string, form, n int, n40 []WireMsg40, heads []WireHead) (unsafe.Pointer, error) {
	switch form {
	case WireForm40:
		if len(n40) < n {
			return nil, fmt.Errorf("raftq: %s: %d frames, room for %d 40-byte records", who, n, len(n40))
		}
		return unsafe.Pointer(&n40[0]), nil
	case WireFormHead:
		if len(heads) < n {
			return nil, fmt.Errorf("raftq: %s: %d frames, room for %d heads", who, n, len(heads))
		}
		return unsafe.Pointer(&heads[0]), nil
	}
	return nil, fmt.Errorf("raftq: %s: form %d is neither WireForm40 nor WireFormHead", who, form)
}

// DecodePacked is DecodeMessages with narrow records (raftq_wire_decode_packed): every frame gets a WireMsg40 (form
// WireForm40, in n40) or a WireHead (WireFormHead, in heads; headTypes: bit t = frames of type t may travel as heads), and
// only a frame the narrow record cannot express exactly -- addressed to another slot than toSlot, carrying entries, ... --
// also its full WireMsg, in frame order, in wide.  nWide may exceed len(wide): the call then fails, the first len(wide) are
// written.  Every slice must be page-locked (HostAlloc); no Step batch may be in flight.
func (e *Engine) DecodePacked(stream []byte, frameOff []uint64, form int, headTypes uint32, toSlot uint32, n40 []WireMsg40, heads []WireHead,
	wide []WireMsg, ents []WireEnt) (nEnts, nMalformed, nWide uint64, err error) {
	n := len(frameOff) - 1
	if n <= 0 {
		return 0, 0, 0, nil
	}
	pn, err := narrowPtr("DecodePacked", form, n, n40, heads)
	if err != nil {
		return 0, 0, 0, err
	}
	var pw *C.raftq_wire_msg_t
	if len(wide) > 0 {
		pw = (*C.raftq_wire_msg_t)(unsafe.Pointer(&wide[0]))
	}
	var pe *C.raftq_wire_ent_t
	if len(ents) > 0 {
		pe = (*C.raftq_wire_ent_t)(unsafe.Pointer(&ents[0]))
	}
	var c C.raftq_wire_counts_t
	var nw C.uint64_t
	rc := C.raftq_wire_decode_packed(e.h, bytesPtr(stream), C.uint64_t(len(stream)), (*C.uint64_t)(unsafe.Pointer(&frameOff[0])), C.uint64_t(n),
		C.int(form), C.uint32_t(headTypes), C.uint32_t(toSlot), pn, pw, C.uint64_t(len(wide)), pe, C.uint64_t(len(ents)), &c, &nw)
	return uint64(c.n_ents), uint64(c.n_malformed), uint64(nw), e.err(rc)
}

// StepFramesPacked is StepFrames with narrow records (raftq_step_frames_packed; toSlot is the engine's own slot): results,
// state and ents as StepFrames gives them, the link carries the narrow array and the wide frames only.  nWide may exceed
// len(wide): the frames have been stepped all the same, DecodeMessages fetches the rest.
func (e *Engine) StepFramesPacked(stream []byte, frameOff []uint64, tailAppends bool, form int, headTypes uint32, n40 []WireMsg40, heads []WireHead,
	wide []WireMsg, ents []WireEnt) (nEnts, nMalformed, nWide uint64, err error) {
	n := len(frameOff) - 1
	if n <= 0 {
		return 0, 0, 0, nil
	}
	pn, err := narrowPtr("StepFramesPacked", form, n, n40, heads)
	if err != nil {
		return 0, 0, 0, err
	}
	var pw *C.raftq_wire_msg_t
	if len(wide) > 0 {
		pw = (*C.raftq_wire_msg_t)(unsafe.Pointer(&wide[0]))
	}
	var pe *C.raftq_wire_ent_t
	if len(ents) > 0 {
		pe = (*C.raftq_wire_ent_t)(unsafe.Pointer(&ents[0]))
	}
	ta := C.int(0)
	if tailAppends {
		ta = 1
	}
	var c C.raftq_wire_counts_t
	var nw C.uint64_t
	rc := C.raftq_step_frames_packed(e.h, bytesPtr(stream), C.uint64_t(len(stream)), (*C.uint64_t)(unsafe.Pointer(&frameOff[0])), C.uint64_t(n), ta,
		C.int(form), C.uint32_t(headTypes), pn, pw, C.uint64_t(len(wide)), pe, C.uint64_t(len(ents)), &c, &nw)
	return uint64(c.n_ents), uint64(c.n_malformed), uint64(nw), e.err(rc)
}

// SetBcastVoters opts the engine in to (or out of) the two device-built broadcasts over each group's own members: with voter masks
// loaded, StepFramesRespond's commit broadcast and ProposeFrames' MsgApps then go to the group's members only instead of the calls
// returning ErrState (include/raftq_wire.h: StepFramesRespond stays compact; ProposeFrames stays positional, a non-member's slot is a
// frame of zero length, and a record whose append would move the commit index is refused).  Independent of SetStepVoters and
// SetTickVoters; no batch may be in flight.
func (e *Engine) SetBcastVoters(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	return e.err(C.raftq_bcast_set_voters(e.h, v))
}

// SetRespondLead opts the engine in to (or out of) StepFramesRespond's answer to a won election (raftq_respond_set_lead): an
// OutBecameLeader result inside its group's device-answered prefix is then flagged OutfAnswered and becomeLeader's broadcast --
// one MsgApp{Index: lastIndex-1, LogTerm: the old lastTerm, Entries: [the empty entry]} per peer -- is in out; the caller still
// appends the empty entry to its own log and WAL, sets every Next to lastIndex+1 and sends nothing.  len(out) must then be at
// least n*(N-1)*RespondLeadFrameMax.  Off by default; no batch may be in flight.
func (e *Engine) SetRespondLead(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	return e.err(C.raftq_respond_set_lead(e.h, v))
}

// SetRespondProps opts the engine in to (or out of) StepFramesRespond's answer to a forwarded proposal (raftq_respond_set_props;
// an effect only after SetStepProps(true)): an OutProposed result inside its group's device-answered prefix whose group is at the
// tail is then flagged OutfAnswered and the leader's MsgApps -- one per peer, Index / LogTerm the tail before the proposal, the
// frame's own entries stamped with the term and the next indices, their payloads gathered from the inbound stream on the device --
// are in out; the caller still stores the entries in its own log and WAL, moves every Next to the new tail + 1 and sends nothing.
// ents must then be non-nil and len(out) at least n*(N-1)*FRAME + (N-1)*(len(stream) + len(ents)*RespondEntMax), FRAME =
// RespondLeadFrameMax after SetRespondLead(true), RespondFrameMax otherwise.  Off by default; no batch may be in flight.
func (e *Engine) SetRespondProps(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	return e.err(C.raftq_respond_set_props(e.h, v))
}

// SetProposeForward opts the engine in to (or out of) ProposeFrames for a node that does not lead every group it is asked about
// (raftq_propose_set_forward; etcd stepFollower's MsgProp: m.To = r.lead; r.send(m)): a Prop whose group this node follows is then
// ONE MsgProp{To: lead, From: self, Term: 0, Entries} frame in the run of its leader's slot (its other slots are frames of zero
// length), one whose group knows no leader is dropped, and ProposeFrames returns what became of every Prop.  Off by default: such a
// Prop fails the call.  No batch may be in flight.
func (e *Engine) SetProposeForward(on bool) error {
	v := C.int(0)
	if on {
		v = 1
	}
	return e.err(C.raftq_propose_set_forward(e.h, v))
}

// PropAppended / PropForwarded / PropDropped: RAFTQ_PROP_* (include/raftq_wire.h), ProposeFrames' outcome bytes
const (
	PropAppended  = 0
	PropForwarded = 1
	PropDropped   = 2
)

// StepFramesRespond is StepFrames plus the messages its results call for, built and marshalled on the device
// (raftq_step_frames_respond; raft.go:268-270 -> :227-230): MsgAppResp / MsgVoteResp / MsgHeartbeatResp to the senders and the
// commit broadcast of a group whose at-tail bit is set (atTail: one bit per group, nil = none).  out receives rafthttp frames,
// peer-major: peerOff[p] .. peerOff[p+1] (len N + 1) are peer p's frames, respOff (nil, or len >= n*(N-1)+1) their byte
// offsets.  A result flagged OutfAnswered is answered: send nothing for it.  len(out) must be at least
// n*(N-1)*RespondFrameMax (RespondLeadFrameMax after SetRespondLead(true)).  Every slice must be page-locked (HostAlloc).
func (e *Engine) StepFramesRespond(stream []byte, frameOff []uint64, tailAppends bool, msgs []WireMsg, ents []WireEnt, atTail []uint64,
	out []byte, respOff, peerOff []uint64) (nEnts, nResp, respBytes uint64, err error) {
	n := len(frameOff) - 1
	if n <= 0 {
		return 0, 0, 0, nil
	}
	if len(msgs) < n {
		return 0, 0, 0, fmt.Errorf("raftq: StepFramesRespond: %d frames, room for %d records", n, len(msgs))
	}
	// the library writes peerOff and respOff and the walk reads atTail where they lie: a short slice would be overrun
	if uint64(len(peerOff)) < uint64(e.Peers)+1 {
		return 0, 0, 0, fmt.Errorf("raftq: StepFramesRespond: peerOff has %d words, needs Peers + 1 = %d", len(peerOff), e.Peers+1)
	}
	if atTail != nil && uint64(len(atTail)) < (e.Groups+63)/64 {
		return 0, 0, 0, fmt.Errorf("raftq: StepFramesRespond: atTail has %d words, needs ceil(Groups / 64) = %d", len(atTail), (e.Groups+63)/64)
	}
	if respOff != nil && uint64(len(respOff)) < uint64(n)*uint64(e.Peers-1)+1 {
		return 0, 0, 0, fmt.Errorf("raftq: StepFramesRespond: respOff has %d words, needs n * (Peers - 1) + 1 = %d", len(respOff),
			uint64(n)*uint64(e.Peers-1)+1)
	}
	var pe *C.raftq_wire_ent_t
	if len(ents) > 0 {
		pe = (*C.raftq_wire_ent_t)(unsafe.Pointer(&ents[0]))
	}
	var pt, pr *C.uint64_t
	if len(atTail) > 0 {
		pt = (*C.uint64_t)(unsafe.Pointer(&atTail[0]))
	}
	if len(respOff) > 0 {
		pr = (*C.uint64_t)(unsafe.Pointer(&respOff[0]))
	}
	ta := C.int(0)
	if tailAppends {
		ta = 1
	}
	var c, rcnt C.raftq_wire_counts_t
	rc := C.raftq_step_frames_respond(e.h, bytesPtr(stream), C.uint64_t(len(stream)), (*C.uint64_t)(unsafe.Pointer(&frameOff[0])), C.uint64_t(n), ta,
		(*C.raftq_wire_msg_t)(unsafe.Pointer(&msgs[0])), pe, C.uint64_t(len(ents)), pt, bytesPtr(out), C.uint64_t(len(out)), pr,
		(*C.uint64_t)(unsafe.Pointer(&peerOff[0])), &c, &rcnt)
	return uint64(c.n_ents), uint64(rcnt.n_msgs), uint64(rcnt.bytes), e.err(rc)
}

// TickFrames is TickCollectLists plus the heartbeat round the Tick calls for, built and marshalled on the device
// (raftq_tick_frames; raft.go:223-224 -> :230: rc.node.Tick -> tickHeartbeat -> Step(MsgBeat) -> bcastHeartbeat ->
// rc.transport.Send): for each of the first min(NBeat, beatCap) MsgBeat groups, ascending, and every peer slot p != self one
// MsgHeartbeat{Term, Commit: min(Match[p], committed)}.  out receives rafthttp frames, peer-major: peerOff[p] .. peerOff[p+1]
// (len Peers + 1) are peer p's frames in ascending group order, frameOff (nil, or len >= beatCap*(Peers-1)+1) their byte offsets.
// Groups beyond beatCap are the caller's (they are in the bitmap or the list).  len(out) must be at least
// beatCap*(Peers-1)*RespondFrameMax; out, frameOff and peerOff must be page-locked (HostAlloc).  A refused call has not ticked.
func (e *Engine) TickFrames(flags uint, hupCap, beatCap uint64, out []byte, frameOff, peerOff []uint64) (t TickLists, nFrames, nBytes uint64, err error) {
	if uint64(len(peerOff)) < uint64(e.Peers)+1 {
		return TickLists{}, 0, 0, fmt.Errorf("raftq: TickFrames: peerOff has %d words, needs Peers + 1 = %d", len(peerOff), e.Peers+1)
	}
	if frameOff != nil && uint64(len(frameOff)) < beatCap*uint64(e.Peers-1)+1 {
		return TickLists{}, 0, 0, fmt.Errorf("raftq: TickFrames: frameOff has %d words, needs beatCap * (Peers - 1) + 1 = %d", len(frameOff),
			beatCap*uint64(e.Peers-1)+1)
	}
	var pf *C.uint64_t
	if len(frameOff) > 0 {
		pf = (*C.uint64_t)(unsafe.Pointer(&frameOff[0]))
	}
	var nh, nb C.uint64_t
	var c C.raftq_wire_counts_t
	rc := C.raftq_tick_frames(e.h, C.uint(flags), C.uint64_t(hupCap), C.uint64_t(beatCap), &nh, &nb, bytesPtr(out), C.uint64_t(len(out)), pf,
		(*C.uint64_t)(unsafe.Pointer(&peerOff[0])), &c)
	if err := e.err(rc); err != nil {
		return TickLists{}, 0, 0, err
	}
	var ph, pb *C.uint32_t
	var pm *C.uint64_t
	var lh, lb, lm C.uint64_t
	if err := e.err(C.raftq_last_tick_lists(e.h, &ph, &lh, &pb, &lb, &pm, &lm)); err != nil {
		return TickLists{}, 0, 0, err
	}
	t = TickLists{NHup: uint64(nh), NBeat: uint64(nb)}
	if lh > 0 {
		t.Hups = unsafe.Slice((*uint32)(unsafe.Pointer(ph)), int(lh))
	}
	if lb > 0 {
		t.Beats = unsafe.Slice((*uint32)(unsafe.Pointer(pb)), int(lb))
	}
	if lm > 0 {
		t.BeatBitmap = unsafe.Slice((*uint64)(unsafe.Pointer(pm)), int(lm))
	}
	return t, uint64(c.n_msgs), uint64(c.bytes), nil
}

// TickElectFrames is TickFrames plus the election round the Tick calls for (raftq_tick_elect_frames; raft.go:223-224 -> :230:
// rc.node.Tick -> tickElection -> Step(MsgHup) -> campaign -> Peers-1 MsgVote -> rc.transport.Send): Step(MsgHup) is applied on
// the device to the first min(NHup, hupCap) MsgHup groups, camp[r] (len >= hupCap) is the compact result of hup id r -- the
// HardState to persist; the caller sends nothing for it -- and out receives the heartbeat section as TickFrames lays it out,
// then the vote section: for every peer slot p != self, ascending, one MsgVote{Term, Index: lastIndex, LogTerm: lastTerm} per
// campaigned group in ascending group order.  peerOff (len 2*(Peers+1)): the heartbeat section's frame indices, then the vote
// section's; frameOff (nil, or len >= (beatCap+hupCap)*(Peers-1)+1) the byte offsets.  MsgHup groups beyond hupCap are the
// caller's.  len(out) must be at least (beatCap+hupCap)*(Peers-1)*RespondFrameMax; camp, out, frameOff and peerOff must be
// page-locked (HostAlloc).  A refused call has neither ticked nor campaigned.
func (e *Engine) TickElectFrames(flags uint, hupCap, beatCap uint64, camp []StepOutS, out []byte, frameOff, peerOff []uint64) (t TickLists, nFrames, nBytes uint64, err error) {
	if uint64(len(peerOff)) < 2*(uint64(e.Peers)+1) {
		return TickLists{}, 0, 0, fmt.Errorf("raftq: TickElectFrames: peerOff has %d words, needs 2 * (Peers + 1) = %d", len(peerOff), 2*(e.Peers+1))
	}
	nMax := (beatCap + hupCap) * uint64(e.Peers-1)
	if frameOff != nil && uint64(len(frameOff)) < nMax+1 {
		return TickLists{}, 0, 0, fmt.Errorf("raftq: TickElectFrames: frameOff has %d words, needs (beatCap + hupCap) * (Peers - 1) + 1 = %d", len(frameOff), nMax+1)
	}
	if uint64(len(camp)) < hupCap {
		return TickLists{}, 0, 0, fmt.Errorf("raftq: TickElectFrames: camp has %d records, needs hupCap = %d", len(camp), hupCap)
	}
	var pf *C.uint64_t
	if len(frameOff) > 0 {
		pf = (*C.uint64_t)(unsafe.Pointer(&frameOff[0]))
	}
	var pc *C.raftq_step_out_s_t
	if len(camp) > 0 {
		pc = (*C.raftq_step_out_s_t)(unsafe.Pointer(&camp[0]))
	}
	var nh, nb C.uint64_t
	var c C.raftq_wire_counts_t
	rc := C.raftq_tick_elect_frames(e.h, C.uint(flags), C.uint64_t(hupCap), C.uint64_t(beatCap), &nh, &nb, pc, bytesPtr(out), C.uint64_t(len(out)), pf,
		(*C.uint64_t)(unsafe.Pointer(&peerOff[0])), &c)
	if err := e.err(rc); err != nil {
		return TickLists{}, 0, 0, err
	}
	var ph, pb *C.uint32_t
	var pm *C.uint64_t
	var lh, lb, lm C.uint64_t
	if err := e.err(C.raftq_last_tick_lists(e.h, &ph, &lh, &pb, &lb, &pm, &lm)); err != nil {
		return TickLists{}, 0, 0, err
	}
	t = TickLists{NHup: uint64(nh), NBeat: uint64(nb)}
	if lh > 0 {
		t.Hups = unsafe.Slice((*uint32)(unsafe.Pointer(ph)), int(lh))
	}
	if lb > 0 {
		t.Beats = unsafe.Slice((*uint32)(unsafe.Pointer(pb)), int(lb))
	}
	if lm > 0 {
		t.BeatBitmap = unsafe.Slice((*uint64)(unsafe.Pointer(pm)), int(lm))
	}
	return t, uint64(c.n_msgs), uint64(c.bytes), nil
}

// OutfAnswered / RespondFrameMax / RespondLeadFrameMax / RespondEntMax: RAFTQ_OUTF_ANSWERED, RAFTQ_RESPOND_FRAME_MAX,
// RAFTQ_RESPOND_LEAD_FRAME_MAX, RAFTQ_RESPOND_ENT_MAX (include/raftq_wire.h)
const (
	OutfAnswered        = 0x10
	RespondFrameMax     = 83
	RespondLeadFrameMax = 109
	RespondEntMax       = 40
)

// WalSaveBegin / WalSaveEnd: rc.wal.Save (raft.go:228) in two halves, so that a turn's WAL encode and its outbound marshal
// are one submission: Begin enqueues (raftq_wal_encode_begin; page-locked buffers), the wait of the WireEncode called next
// covers it, End reports what WalSave would have.  out is not to be read, nor recs / pool reused, before End.
func (e *Engine) WalSaveBegin(recs []WalRec, pool []byte, prevCrc uint32, out []byte) error {
	e.walPrevCrc = prevCrc
	if len(recs) == 0 { // a turn with nothing to persist: the End paired with it answers (0, prevCrc, nil)
		e.walBegun = false
		return nil
	}
	err := e.err(C.raftq_wal_encode_begin(e.h, (*C.raftq_wal_rec_t)(unsafe.Pointer(&recs[0])), C.uint64_t(len(recs)), bytesPtr(pool),
		C.uint64_t(len(pool)), C.uint32_t(prevCrc), bytesPtr(out), C.uint64_t(len(out)), nil))
	e.walBegun = err == nil
	return err
}

func (e *Engine) WalSaveEnd() (n uint64, lastCrc uint32, err error) {
	if !e.walBegun {
		return 0, e.walPrevCrc, nil
	}
	e.walBegun = false
	var c C.raftq_wal_counts_t
	rc := C.raftq_wal_encode_end(e.h, &c)
	return uint64(c.bytes), uint32(c.last_crc), e.err(rc)
}

// Prop is layout-identical to raftq_prop_t (16 bytes): a group this node leads, and which of propEnts are its new entries.
type Prop struct {
	Group    uint64
	EntFirst uint32 // into propEnts
	NEnts    uint32 // >= 1
}

// PropEnt is layout-identical to raftq_prop_ent_t (16 bytes): where one proposed Entry's Data lies in the pool.
type PropEnt struct {
	DataOff uint64
	DataLen uint32
	Type    uint32 // raftpb.EntryType
}

// ProposeFrames is a node's outbound half of a turn for what it was asked to propose (raftq_propose_frames; raft.go:211-215 ->
// :227-230) as ONE submission and one wait: for every Prop the leader's appendEntry on the device-resident state and the N - 1
// MsgApps of bcastAppend, written into the encoder's input in HBM -- they never exist in host memory --, then the marshal of
// msgs (what the caller queued itself this turn) followed by those MsgApps, one run per peer slot != self, ascending.  The
// caller still owns the log (it appends the entries itself) and Progress.Next (it names only groups whose followers are all at
// the tail, and moves Next past the new entries).  Every slice must be page-locked (HostAlloc).  A call that fails has appended
// nothing: when out is too small, need is the size the stream takes and the same call with len(out) >= need is safe -- it appends
// once.  After SetProposeForward(true) outcomes holds one Prop* byte per Prop (raftq_propose_outcomes: a copy of the handle's own
// bytes); it is nil otherwise and after a call that failed.  SOURCE ONLY (round 6).
func (e *Engine) ProposeFrames(props []Prop, propEnts []PropEnt, msgs []WireMsg, ents []WireEnt, pool, out []byte, frameOff []uint64) (need uint64, outcomes []byte, err error) {
	var pp *C.raftq_prop_t
	var ppe *C.raftq_prop_ent_t
	var pm *C.raftq_wire_msg_t
	var pe *C.raftq_wire_ent_t
	var po *C.uint64_t
	if len(props) > 0 {
		pp = (*C.raftq_prop_t)(unsafe.Pointer(&props[0]))
	}
	if len(propEnts) > 0 {
		ppe = (*C.raftq_prop_ent_t)(unsafe.Pointer(&propEnts[0]))
	}
	if len(msgs) > 0 {
		pm = (*C.raftq_wire_msg_t)(unsafe.Pointer(&msgs[0]))
	}
	if len(ents) > 0 {
		pe = (*C.raftq_wire_ent_t)(unsafe.Pointer(&ents[0]))
	}
	if len(frameOff) > 0 {
		po = (*C.uint64_t)(unsafe.Pointer(&frameOff[0]))
	}
	var c C.raftq_wire_counts_t
	rc := C.raftq_propose_frames(e.h, pp, C.uint64_t(len(props)), ppe, C.uint64_t(len(propEnts)), pm, C.uint64_t(len(msgs)), pe, C.uint64_t(len(ents)),
		bytesPtr(pool), C.uint64_t(len(pool)), bytesPtr(out), C.uint64_t(len(out)), po, &c)
	if rc != 0 {
		return uint64(c.bytes), nil, e.err(rc)
	}
	var what *C.uint8_t
	var nWhat C.uint64_t
	if rc := C.raftq_propose_outcomes(e.h, &what, &nWhat); rc != 0 {
		return uint64(c.bytes), nil, e.err(rc)
	}
	if nWhat != 0 {
		outcomes = C.GoBytes(unsafe.Pointer(what), C.int(nWhat))
	}
	return uint64(c.bytes), outcomes, nil
}
