//go:build etcd

// respond_props_pin_test.go -- the MsgApps raftq_step_frames_respond builds for a forwarded proposal under SetRespondProps
// (include/raftq_wire.h "A forwarded proposal's MsgApps") beside the ones a real github.com/coreos/etcd/raft leader sends for the
// same MsgProp: stepLeader's appendEntry + bcastAppend with every follower at the tail.  Build as etcd_pin_test.go says.
//
// SOURCE ONLY: the module is not on the build machine and there is no Go toolchain.
package raftq

import (
	"testing"
	"unsafe"

	"github.com/coreos/etcd/raft"
	pb "github.com/coreos/etcd/raft/raftpb"
)

// TestRespondPropsAgainstEtcd: node 1 of three wins an election and has its empty entry acknowledged by both followers (every
// Next at the tail); then follower 2 forwards a proposal of two entries, one of them with no Data.  etcd's Ready holds the two
// MsgApps; the engine, loaded with the state before the proposal and the group's at-tail bit set, must build the same two
// messages from the MsgProp's own frame.
func TestRespondPropsAgainstEtcd(t *testing.T) {
	const n = 3
	peers := []raft.Peer{{ID: 1}, {ID: 2}, {ID: 3}}
	st := raft.NewMemoryStorage()
	c := &raft.Config{ID: 1, ElectionTick: 10, HeartbeatTick: 1, Storage: st, MaxSizePerMsg: 1 << 20, MaxInflightMsgs: 256}
	rn, err := raft.NewRawNode(c, peers)
	if err != nil {
		t.Fatal(err)
	}
	var sent []pb.Message
	drain := func() {
		for rn.HasReady() {
			rd := rn.Ready()
			st.Append(rd.Entries)
			if !raft.IsEmptyHardState(rd.HardState) {
				st.SetHardState(rd.HardState)
			}
			sent = append(sent, rd.Messages...)
			rn.Advance(rd)
		}
	}
	drain()
	rn.Campaign()
	drain()
	term := rn.Status().Term
	for _, from := range []uint64{2, 3} {
		rn.Step(pb.Message{Type: pb.MsgVoteResp, From: from, To: 1, Term: term})
		drain()
	}
	tail, _ := st.LastIndex()
	for _, from := range []uint64{2, 3} {
		rn.Step(pb.Message{Type: pb.MsgAppResp, From: from, To: 1, Term: term, Index: tail})
		drain()
	}
	if rn.Status().RaftState != raft.StateLeader {
		t.Fatal("node 1 does not lead")
	}
	tailTerm, _ := st.Term(tail)
	commit := rn.Status().Commit

	e, err := New(0, 1, n)
	if err != nil {
		t.Skip(err) // no GPU here
	}
	defer e.Close()
	for _, err := range []error{e.SetMsgFlags(true), e.SetStepProps(true), e.SetRespondProps(true)} {
		if err != nil {
			t.Fatal(err)
		}
	}
	// the leader's state before the proposal (the loaders of etcd_pin_test.go's TestStepAgainstEtcd)
	if err := e.LoadNode([]uint64{term}, []uint32{1}, []uint32{1}, []uint64{tail}, []uint64{tailTerm}); err != nil {
		t.Fatal(err)
	}
	if err := e.LoadRoles([]uint8{2}, []uint32{0}); err != nil {
		t.Fatal(err)
	}
	if err := e.LoadMatch([]uint64{tail, tail, tail}, []uint64{commit}); err != nil {
		t.Fatal(err)
	}
	if err := e.LoadTerms([]uint64{term}, []uint64{tail}); err != nil {
		t.Fatal(err)
	}

	prop := pb.Message{Type: pb.MsgProp, From: 2, To: 1, Entries: []pb.Entry{{Data: []byte("put k v")}, {Type: pb.EntryConfChange}}}
	sent = nil
	rn.Step(prop)
	drain()
	var want []pb.Message
	for _, m := range sent {
		if m.Type == pb.MsgApp {
			want = append(want, m)
		}
	}
	if len(want) != n-1 {
		t.Fatalf("etcd sent %d MsgApps for the proposal", len(want))
	}

	alloc := func(bytes int) []byte {
		b, err := HostAlloc(bytes)
		if err != nil {
			t.Fatal(err)
		}
		return b
	}
	body, err := prop.Marshal()
	if err != nil {
		t.Fatal(err)
	}
	stream := alloc(8 + len(body))
	for k := 0; k < 8; k++ {
		stream[k] = byte(uint64(len(body)) >> (56 - 8*k))
	}
	copy(stream[8:], body)
	words := func(k int) []uint64 { return unsafe.Slice((*uint64)(unsafe.Pointer(&alloc(8 * k)[0])), k) }
	off := words(2)
	off[0], off[1] = 0, uint64(len(stream))
	msgs := unsafe.Slice((*WireMsg)(unsafe.Pointer(&alloc(64)[0])), 1)
	const entsCap = 4
	ents := unsafe.Slice((*WireEnt)(unsafe.Pointer(&alloc(32 * entsCap)[0])), entsCap)
	atTail := words(1)
	atTail[0] = 1
	out := alloc(1*(n-1)*RespondFrameMax + (n-1)*(len(stream)+entsCap*RespondEntMax))
	respOff, peerOff := words(1*(n-1)+1), words(n+1)
	_, nResp, _, err := e.StepFramesRespond(stream, off, true, msgs, ents, atTail, out, respOff, peerOff)
	if err != nil {
		t.Fatal(err)
	}
	if nResp != n-1 || peerOff[0] != 0 || peerOff[1] != 0 || peerOff[2] != 1 || peerOff[3] != 2 {
		t.Fatalf("%d frames, slices %v", nResp, peerOff)
	}
	for k := 0; k < n-1; k++ {
		var got pb.Message
		if err := got.Unmarshal(out[respOff[k]+8 : respOff[k+1]]); err != nil { // (a stock Unmarshal skips the group field)
			t.Fatal(err)
		}
		var w *pb.Message
		for i := range want {
			if want[i].To == got.To {
				w = &want[i]
			}
		}
		if w == nil {
			t.Fatalf("frame %d goes to %d: etcd sent nothing there", k, got.To)
		}
		a, _ := got.Marshal()
		b, _ := w.Marshal()
		if string(a) != string(b) {
			t.Fatalf("the MsgApp to %d\n device %x\n etcd   %x", got.To, a, b)
		}
	}
}
