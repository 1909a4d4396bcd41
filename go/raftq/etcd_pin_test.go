//go:build etcd

// etcd_pin_test.go -- the check that would PIN parity (SURVEY.md F1/F2, 8c): drive the real
// github.com/coreos/etcd/raft (the module raft.go:27-34 imports; v2.2-v2.3 line) and this repo's
// restatement with the same acknowledgements and compare the commit index after every message.
// Build with `go test -tags etcd ./go/raftq` in a GOPATH that holds that etcd checkout.
//
// SOURCE ONLY: the module is not on the build machine and there is no Go toolchain.
package raftq

import (
	"math/rand"
	"testing"
	"unsafe"

	"github.com/coreos/etcd/raft"
	pb "github.com/coreos/etcd/raft/raftpb"
)

func TestCommitIndexAgainstEtcd(t *testing.T) {
	for _, n := range []int{1, 2, 3, 4, 5, 7, 9} {
		rng := rand.New(rand.NewSource(int64(0xC0FFEE00 + n)))
		peers := make([]raft.Peer, n)
		for i := range peers {
			peers[i] = raft.Peer{ID: uint64(i + 1)}
		}
		st := raft.NewMemoryStorage()
		c := &raft.Config{ID: 1, ElectionTick: 10, HeartbeatTick: 1, Storage: st, MaxSizePerMsg: 1 << 20, MaxInflightMsgs: 256}
		rn, err := raft.NewRawNode(c, peers)
		if err != nil {
			t.Fatal(err)
		}
		drain := func() pb.HardState { // apply a Ready the way raft.go:227-235 does
			var hs pb.HardState
			for rn.HasReady() {
				rd := rn.Ready()
				st.Append(rd.Entries)
				if !raft.IsEmptyHardState(rd.HardState) {
					hs = rd.HardState
					st.SetHardState(hs)
				}
				rn.Advance(rd)
			}
			return hs
		}
		drain()
		rn.Campaign()
		drain()
		for p := 2; p <= n; p++ { // win the election
			rn.Step(pb.Message{Type: pb.MsgVoteResp, From: uint64(p), To: 1, Term: 1})
		}
		drain()
		for i := 0; i < 40; i++ {
			rn.Propose([]byte{byte(i)})
		}
		drain()
		last, _ := st.LastIndex()
		first, _ := st.FirstIndex()
		_ = first
		match := make([]uint64, n)
		match[0] = last
		committed := rn.Status().Commit
		firstIdxCurTerm := uint64(0)
		for i := uint64(1); i <= last; i++ { // the compact gate: first index of the leader's term
			if tm, _ := st.Term(i); tm == 1 {
				firstIdxCurTerm = i
				break
			}
		}
		for step := 0; step < 400 && n > 1; step++ {
			p := 1 + rng.Intn(n-1)
			idx := uint64(rng.Int63n(int64(last) + 1))
			rn.Step(pb.Message{Type: pb.MsgAppResp, From: uint64(p + 1), To: 1, Term: 1, Index: idx})
			drain()
			if idx > match[p] { // Progress.maybeUpdate
				match[p] = idx
			}
			committed = commitLikeEtcd(match, committed, firstIdxCurTerm, true)
			if got := rn.Status().Commit; got != committed {
				t.Fatalf("N=%d step %d: etcd commit %d, restatement %d (match %v)", n, step, got, committed, match)
			}
		}
	}
}

// ---- round 6 (VERDICT r05 item 9): the pin, one command away, for Step and the byte formats too ------------------------------
//
// TestStepAgainstEtcd drives one real raft (RawNode, peer 1 of N) and one group of this repo's batched Step with the same
// message sequence -- an election, acknowledgements, heartbeats, a higher-term vote that deposes the leader -- and compares
// {term, vote, commit, lead, role} after every message.  What the restatement calls role / lead / vote is rn.Status().
func TestStepAgainstEtcd(t *testing.T) {
	for _, n := range []int{1, 3, 5, 7} {
		rng := rand.New(rand.NewSource(int64(0x57E9 + n)))
		peers := make([]raft.Peer, n)
		for i := range peers {
			peers[i] = raft.Peer{ID: uint64(i + 1)}
		}
		st := raft.NewMemoryStorage()
		c := &raft.Config{ID: 1, ElectionTick: 10, HeartbeatTick: 1, Storage: st, MaxSizePerMsg: 1 << 20, MaxInflightMsgs: 256}
		rn, err := raft.NewRawNode(c, peers)
		if err != nil {
			t.Fatal(err)
		}
		drain := func() {
			for rn.HasReady() {
				rd := rn.Ready()
				st.Append(rd.Entries)
				if !raft.IsEmptyHardState(rd.HardState) {
					st.SetHardState(rd.HardState)
				}
				for _, m := range rd.Messages { // the rule raftq_tick_frames restates: a heartbeat's Commit is min(Progress[to].Match, committed)
					if m.Type == pb.MsgVote { // the round raftq_tick_elect_frames restates: campaign()'s MsgVote{Term: the new term, Index: lastIndex, LogTerm: lastTerm}
						li, _ := st.LastIndex()
						ltm, _ := st.Term(li)
						if s := rn.Status(); m.Term != s.Term || m.Index != li || m.LogTerm != ltm || m.Commit != 0 || m.Reject || len(m.Entries) != 0 ||
							s.RaftState != raft.StateCandidate || s.Vote != 1 {
							t.Fatalf("N=%d: MsgVote to %d carries {Term %d Index %d LogTerm %d}, want {%d %d %d} from a candidate that voted for itself (state %v, vote %d)",
								n, m.To, m.Term, m.Index, m.LogTerm, s.Term, li, ltm, s.RaftState, s.Vote)
						}
					}
					if m.Type != pb.MsgHeartbeat {
						continue
					}
					s := rn.Status()
					want := s.Commit
					if mt := s.Progress[m.To].Match; mt < want {
						want = mt
					}
					if m.Commit != want {
						t.Fatalf("N=%d: MsgHeartbeat to %d carries Commit %d, want min(Match %d, committed %d)", n, m.To, m.Commit, s.Progress[m.To].Match, s.Commit)
					}
				}
				rn.Advance(rd)
			}
		}
		drain()
		e, err := New(0, 1, uint32(n))
		if err != nil {
			t.Skip(err) // no GPU here
		}
		defer e.Close()
		// the bootstrap ConfChange entries of StartNode / NewRawNode: the restatement's log starts where etcd's does
		last, _ := st.LastIndex()
		lt, _ := st.Term(last)
		if err := e.LoadNode([]uint64{rn.Status().Term}, []uint32{0}, []uint32{0}, []uint64{last}, []uint64{lt}); err != nil {
			t.Fatal(err)
		}
		check := func(what string) {
			s := rn.Status()
			ns, err := e.ReadNode()
			if err != nil {
				t.Fatal(err)
			}
			role := map[raft.StateType]uint8{raft.StateFollower: 0, raft.StateCandidate: 1, raft.StateLeader: 2}[s.RaftState]
			if ns.Term[0] != s.Term || uint64(ns.Vote[0]) != s.Vote || ns.Committed[0] != s.Commit || uint64(ns.Lead[0]) != s.Lead || ns.Role[0] != role {
				t.Fatalf("N=%d after %s: etcd {term %d vote %d commit %d lead %d state %v}, restatement {term %d vote %d commit %d lead %d role %d}",
					n, what, s.Term, s.Vote, s.Commit, s.Lead, s.RaftState, ns.Term[0], ns.Vote[0], ns.Committed[0], ns.Lead[0], ns.Role[0])
			}
		}
		step := func(m pb.Message, what string) {
			rn.Step(m)
			drain()
			out := make([]StepOut, 1)
			rec := Msg{Group: 0, Term: m.Term, LogTerm: m.LogTerm, Index: m.Index, Commit: m.Commit, RejectHint: m.RejectHint,
				From: uint32(m.From - 1), Type: uint8(m.Type)}
			if m.Reject {
				rec.Reject = 1
			}
			if _, err := e.StepBatch([]Msg{rec}, out); err != nil {
				t.Fatal(err)
			}
			check(what)
		}
		rn.Campaign()
		drain()
		if _, err := e.StepBatch([]Msg{{Group: 0, Type: uint8(pb.MsgHup)}}, make([]StepOut, 1)); err != nil {
			t.Fatal(err)
		}
		check("MsgHup")
		term := rn.Status().Term
		for p := 2; p <= n; p++ {
			step(pb.Message{Type: pb.MsgVoteResp, From: uint64(p), To: 1, Term: term, Reject: p == n && n > 3}, "MsgVoteResp")
		}
		last, _ = st.LastIndex()
		for i := 0; i < 200 && n > 1; i++ {
			p := uint64(2 + rng.Intn(n-1))
			switch rng.Intn(4) {
			case 0:
				step(pb.Message{Type: pb.MsgHeartbeatResp, From: p, To: 1, Term: term}, "MsgHeartbeatResp")
			case 1:
				step(pb.Message{Type: pb.MsgAppResp, From: p, To: 1, Term: term, Index: uint64(rng.Int63n(int64(last) + 1)), Reject: true, RejectHint: 0}, "MsgAppResp(reject)")
			default:
				step(pb.Message{Type: pb.MsgAppResp, From: p, To: 1, Term: term, Index: uint64(rng.Int63n(int64(last) + 1))}, "MsgAppResp")
			}
			rn.Tick() // HeartbeatTick 1: the leader's bcastHeartbeat, checked in drain
			drain()
		}
		if n > 1 { // a candidate of a higher term with an up-to-date log deposes the leader and gets the vote
			step(pb.Message{Type: pb.MsgVote, From: 2, To: 1, Term: term + 5, LogTerm: term + 1, Index: last + 10}, "MsgVote(higher term)")
			step(pb.Message{Type: pb.MsgHeartbeat, From: 2, To: 1, Term: term + 5, Commit: rn.Status().Commit}, "MsgHeartbeat")
		}
	}
}

// TestFramesAgainstGogoProto: the stream frames raftq_wire_encode writes are rafthttp's messageEncoder frames -- an 8-byte
// big-endian length and pb.Message.Marshal() (the generated gogo-proto code of the pinned etcd) -- byte for byte, and what
// raftq_wire_decode reads back from etcd's own bytes is the message.  (The `group` extension field is 0 here: omitted... the
// encoder writes it always, as field 12, which a stock Unmarshal skips: the comparison strips it.)
func TestFramesAgainstGogoProto(t *testing.T) {
	e, err := New(0, 4, 3)
	if err != nil {
		t.Skip(err)
	}
	defer e.Close()
	rng := rand.New(rand.NewSource(0xF4A3E5))
	for round := 0; round < 50; round++ {
		var msgs []WireMsg
		var ents []WireEnt
		var pool []byte
		var want [][]byte
		for i := 0; i < 64; i++ {
			m := pb.Message{Type: pb.MessageType(rng.Intn(10)), To: uint64(1 + rng.Intn(3)), From: uint64(1 + rng.Intn(3)), Term: uint64(rng.Int63n(1 << 40)),
				LogTerm: uint64(rng.Int63n(1 << 20)), Index: uint64(rng.Int63n(1 << 50)), Commit: uint64(rng.Int63n(1 << 30)), Reject: rng.Intn(2) == 1,
				RejectHint: uint64(rng.Int63n(1 << 10))}
			w := WireMsg{Term: m.Term, LogTerm: m.LogTerm, Index: m.Index, Commit: m.Commit, RejectHint: m.RejectHint, From: uint32(m.From - 1), To: uint8(m.To - 1),
				Type: uint8(m.Type), EntFirst: uint32(len(ents))}
			if m.Reject {
				w.Reject = 1
			}
			if m.Type == pb.MsgApp {
				for k := 0; k < 1+rng.Intn(3); k++ {
					d := make([]byte, rng.Intn(200))
					rng.Read(d)
					m.Entries = append(m.Entries, pb.Entry{Term: m.Term, Index: m.Index + uint64(k) + 1, Data: d})
					ents = append(ents, WireEnt{Term: m.Term, Index: m.Index + uint64(k) + 1, DataOff: uint64(len(pool)), DataLen: uint32(len(d))})
					pool = append(pool, d...)
					w.NEnts++
				}
			}
			b, err := m.Marshal()
			if err != nil {
				t.Fatal(err)
			}
			want = append(want, b)
			msgs = append(msgs, w)
		}
		out := make([]byte, 1<<20)
		off := make([]uint64, len(msgs)+1)
		if _, err := e.EncodeMessages(msgs, ents, pool, out, off); err != nil {
			t.Fatal(err)
		}
		for i, b := range want {
			frame := out[off[i]:off[i+1]]
			var back pb.Message
			if err := back.Unmarshal(frame[8:]); err != nil { // etcd reads what the device wrote
				t.Fatalf("round %d msg %d: etcd cannot unmarshal the device's frame: %v", round, i, err)
			}
			again, _ := back.Marshal()
			if string(again) != string(b) {
				t.Fatalf("round %d msg %d: the device's frame is not etcd's message\n got  %x\n want %x", round, i, again, b)
			}
		}
		// etcd's own bytes through the device's decoder
		var stream []byte
		offs := []uint64{0}
		for _, b := range want {
			var l [8]byte
			for k := 0; k < 8; k++ {
				l[k] = byte(uint64(len(b)) >> (56 - 8*k))
			}
			stream = append(append(stream, l[:]...), b...)
			offs = append(offs, uint64(len(stream)))
		}
		gm := make([]WireMsg, len(want))
		ge := make([]WireEnt, len(ents)+1)
		if _, bad, err := e.DecodeMessages(stream, offs, gm, ge); err != nil || bad != 0 {
			t.Fatal(err, bad)
		}
		for i := range gm {
			a, b := gm[i], msgs[i]
			if a.Term != b.Term || a.LogTerm != b.LogTerm || a.Index != b.Index || a.Commit != b.Commit || a.From != b.From || a.To != b.To || a.Type != b.Type ||
				a.Reject != b.Reject || a.RejectHint != b.RejectHint || a.NEnts != b.NEnts {
				t.Fatalf("round %d msg %d: decoded %+v, sent %+v", round, i, a, b)
			}
		}
	}
}

// TestWalAgainstEtcdWal: raftq_wal_encode's bytes are a WAL the pinned etcd's `wal` package reads back -- records, running
// CRC and all -- when they are written behind the head wal.Create leaves (metadata + crc record), and raftq_wal_decode reads
// the file wal.Save wrote.  Needs "github.com/coreos/etcd/wal" beside the raft module; see PIN.md for the file-level steps
// (segment header, 64 MB preallocation: the library writes frames, the file is the caller's -- raft.go:98-116).
//
// (Left as the procedure in PIN.md rather than code: wal.Create's on-disk head differs between v2.2 and v2.3 -- the range PIN.md
// says to try -- and a test that cannot be compiled here should not guess which.)

// TestDecodePackedAgainstDecode: etcd's own bytes through the decoder's narrow forms (DecodePacked) give what DecodeMessages
// gives -- a narrow frame field by field (WireMsg40: all of them; WireHead: the routing word), a wide one as wide[k].
func TestDecodePackedAgainstDecode(t *testing.T) {
	e, err := New(0, 4, 3)
	if err != nil {
		t.Skip(err)
	}
	defer e.Close()
	rng := rand.New(rand.NewSource(0x9AC4ED))
	const n = 300
	var raw []byte
	offs := []uint64{0}
	for i := 0; i < n; i++ {
		m := pb.Message{Type: pb.MessageType(rng.Intn(10)), To: uint64(1 + rng.Intn(2)), From: uint64(1 + rng.Intn(3)), Term: uint64(rng.Int63n(1 << 40)),
			Index: uint64(rng.Int63n(1 << 50)), Commit: uint64(rng.Int63n(1 << 30)), Reject: rng.Intn(4) == 0}
		if m.Type == pb.MsgAppResp {
			m.RejectHint = uint64(rng.Int63n(1 << 10))
		} else {
			m.LogTerm = uint64(rng.Int63n(1 << 20))
		}
		if m.Type == pb.MsgApp && rng.Intn(2) == 0 {
			m.Entries = []pb.Entry{{Term: m.Term, Index: m.Index + 1, Data: []byte{byte(i)}}}
		}
		b, err := m.Marshal()
		if err != nil {
			t.Fatal(err)
		}
		var l [8]byte
		for k := 0; k < 8; k++ {
			l[k] = byte(uint64(len(b)) >> (56 - 8*k))
		}
		raw = append(append(raw, l[:]...), b...)
		offs = append(offs, uint64(len(raw)))
	}
	// page-locked copies: the narrow forms exist in the streaming form only
	alloc := func(bytes int) []byte {
		b, err := HostAlloc(bytes)
		if err != nil {
			t.Fatal(err)
		}
		return b
	}
	stream := alloc(len(raw))
	copy(stream, raw)
	offB := alloc(8 * len(offs))
	off := unsafe.Slice((*uint64)(unsafe.Pointer(&offB[0])), len(offs))
	copy(off, offs)
	full := unsafe.Slice((*WireMsg)(unsafe.Pointer(&alloc(64 * n)[0])), n)
	wide := unsafe.Slice((*WireMsg)(unsafe.Pointer(&alloc(64 * n)[0])), n)
	n40 := unsafe.Slice((*WireMsg40)(unsafe.Pointer(&alloc(40 * n)[0])), n)
	heads := unsafe.Slice((*WireHead)(unsafe.Pointer(&alloc(8 * n)[0])), n)
	ents := unsafe.Slice((*WireEnt)(unsafe.Pointer(&alloc(32 * n)[0])), n)
	if _, bad, err := e.DecodeMessages(stream, off, full, ents); err != nil || bad != 0 {
		t.Fatal(err, bad)
	}
	const toSlot = 0
	const respKinds = 1<<uint(pb.MsgAppResp) | 1<<uint(pb.MsgVoteResp) | 1<<uint(pb.MsgHeartbeatResp)
	for _, form := range []int{WireForm40, WireFormHead} {
		_, _, nWide, err := e.DecodePacked(stream, off, form, respKinds, toSlot, n40, heads, wide, ents)
		if err != nil {
			t.Fatal(err)
		}
		k := uint64(0)
		for i := 0; i < n; i++ {
			h := WireHead{n40[i].Group, n40[i].From, n40[i].Type, n40[i].Reject, n40[i].Flags}
			if form == WireFormHead {
				h = heads[i]
			}
			f := full[i]
			if h.Flags&WireWide != 0 {
				if wide[k] != f || (form == WireForm40 && n40[i].Aux != k) {
					t.Fatalf("form %d frame %d: wide[%d] = %+v, decoded %+v", form, i, k, wide[k], f)
				}
				k++
				continue
			}
			if uint64(h.Group) != f.Group || uint32(h.From) != f.From || h.Type != f.Type || h.Reject != f.Reject || h.Flags != f.Flags || f.To != toSlot || f.NEnts != 0 {
				t.Fatalf("form %d frame %d: head %+v, decoded %+v", form, i, h, f)
			}
			if form == WireForm40 {
				aux := f.LogTerm
				if f.Type == uint8(pb.MsgAppResp) {
					aux = f.RejectHint
				}
				if m := n40[i]; m.Term != f.Term || m.Index != f.Index || m.Commit != f.Commit || m.Aux != aux {
					t.Fatalf("frame %d: narrow %+v, decoded %+v", i, m, f)
				}
			}
		}
		if k != nWide {
			t.Fatalf("form %d: %d wide records met, %d reported", form, k, nWide)
		}
	}
}

// TestStepVotersAgainstEtcd: the masked rules of raftq_step_set_voters (include/raftq_step.h) beside a real raft whose `prs` map IS
// the mask.  The engine has N = 5 peer slots; the group's members are the raft IDs in `members` (slot = ID - 1), so etcd's q() is
// len(prs)/2 + 1 = popcount(mask)/2 + 1.  Same messages to both; {term, vote, commit, lead, role} compared after every one.  A
// message from a slot that is no member goes to the engine only where etcd would ignore it as well (an ack of a peer without
// Progress is dropped upstream; the engine stores its Match and does not count it -- the commit index must not move).
func TestStepVotersAgainstEtcd(t *testing.T) {
	const n = 5
	for _, members := range [][]uint64{{1}, {1, 2}, {1, 2, 4}, {1, 3, 4, 5}, {1, 2, 3, 4, 5}} {
		rng := rand.New(rand.NewSource(int64(0x707E25 + len(members))))
		mask := uint16(0)
		peers := make([]raft.Peer, len(members))
		for i, id := range members {
			peers[i] = raft.Peer{ID: id}
			mask |= 1 << (id - 1)
		}
		st := raft.NewMemoryStorage()
		c := &raft.Config{ID: 1, ElectionTick: 10, HeartbeatTick: 1, Storage: st, MaxSizePerMsg: 1 << 20, MaxInflightMsgs: 256}
		rn, err := raft.NewRawNode(c, peers)
		if err != nil {
			t.Fatal(err)
		}
		drain := func() {
			for rn.HasReady() {
				rd := rn.Ready()
				st.Append(rd.Entries)
				if !raft.IsEmptyHardState(rd.HardState) {
					st.SetHardState(rd.HardState)
				}
				rn.Advance(rd)
			}
		}
		drain()
		e, err := New(0, 1, n)
		if err != nil {
			t.Skip(err) // no GPU here
		}
		defer e.Close()
		if err := e.LoadVoters([]uint16{mask}); err != nil {
			t.Fatal(err)
		}
		if err := e.SetStepVoters(true); err != nil {
			t.Fatal(err)
		}
		last, _ := st.LastIndex()
		lt, _ := st.Term(last)
		if err := e.LoadNode([]uint64{rn.Status().Term}, []uint32{0}, []uint32{0}, []uint64{last}, []uint64{lt}); err != nil {
			t.Fatal(err)
		}
		check := func(what string) {
			s := rn.Status()
			ns, err := e.ReadNode()
			if err != nil {
				t.Fatal(err)
			}
			role := map[raft.StateType]uint8{raft.StateFollower: 0, raft.StateCandidate: 1, raft.StateLeader: 2}[s.RaftState]
			if ns.Term[0] != s.Term || uint64(ns.Vote[0]) != s.Vote || ns.Committed[0] != s.Commit || uint64(ns.Lead[0]) != s.Lead || ns.Role[0] != role {
				t.Fatalf("members %v after %s: etcd {term %d vote %d commit %d lead %d state %v}, restatement {term %d vote %d commit %d lead %d role %d}",
					members, what, s.Term, s.Vote, s.Commit, s.Lead, s.RaftState, ns.Term[0], ns.Vote[0], ns.Committed[0], ns.Lead[0], ns.Role[0])
			}
		}
		step := func(m pb.Message, toEtcd bool, what string) {
			if toEtcd {
				rn.Step(m)
				drain()
			}
			rec := Msg{Group: 0, Term: m.Term, LogTerm: m.LogTerm, Index: m.Index, Commit: m.Commit, From: uint32(m.From - 1), Type: uint8(m.Type)}
			if m.Reject {
				rec.Reject = 1
			}
			if _, err := e.StepBatch([]Msg{rec}, make([]StepOut, 1)); err != nil {
				t.Fatal(err)
			}
			check(what)
		}
		rn.Campaign()
		drain()
		if _, err := e.StepBatch([]Msg{{Group: 0, Type: uint8(pb.MsgHup)}}, make([]StepOut, 1)); err != nil {
			t.Fatal(err)
		}
		check("MsgHup") // a one-voter group {self} is leader already: q_g = 1
		term := rn.Status().Term
		isMember := func(id uint64) bool { return mask&(1<<(id-1)) != 0 }
		for id := uint64(2); id <= n; id++ { // a non-member's grant is recorded by the engine and counts nowhere
			step(pb.Message{Type: pb.MsgVoteResp, From: id, To: 1, Term: term}, isMember(id), "MsgVoteResp")
		}
		last, _ = st.LastIndex()
		for i := 0; i < 200; i++ {
			id := uint64(2 + rng.Intn(n-1))
			step(pb.Message{Type: pb.MsgAppResp, From: id, To: 1, Term: term, Index: uint64(rng.Int63n(int64(last) + 1))}, isMember(id), "MsgAppResp")
		}
	}
}

// TestStepPropsAgainstEtcd: forwarded proposals (raftq_step_set_props) beside a real raft.  A one-node group and a three-node
// group are campaigned into leadership, then stepped with MsgProps of one to four entries between acknowledgements: after every
// message the engine's term, commit index, leader and role are etcd's, and so is the log's tail.  Then the same on a follower
// (the proposal is forwarded: nothing moves) and on a candidate (dropped).
func TestStepPropsAgainstEtcd(t *testing.T) {
	for _, n := range []int{1, 3} {
		rng := rand.New(rand.NewSource(int64(0x9809 + n)))
		peers := make([]raft.Peer, n)
		for i := range peers {
			peers[i] = raft.Peer{ID: uint64(i + 1)}
		}
		st := raft.NewMemoryStorage()
		c := &raft.Config{ID: 1, ElectionTick: 10, HeartbeatTick: 1, Storage: st, MaxSizePerMsg: 1 << 20, MaxInflightMsgs: 256}
		rn, err := raft.NewRawNode(c, peers)
		if err != nil {
			t.Fatal(err)
		}
		drain := func() {
			for rn.HasReady() {
				rd := rn.Ready()
				st.Append(rd.Entries)
				if !raft.IsEmptyHardState(rd.HardState) {
					st.SetHardState(rd.HardState)
				}
				rn.Advance(rd)
			}
		}
		drain()
		e, err := New(0, 1, uint32(n))
		if err != nil {
			t.Skip(err) // no GPU here
		}
		defer e.Close()
		for _, err := range []error{e.SetMsgFlags(true), e.SetStepProps(true)} {
			if err != nil {
				t.Fatal(err)
			}
		}
		last, _ := st.LastIndex()
		lt, _ := st.Term(last)
		if err := e.LoadNode([]uint64{rn.Status().Term}, []uint32{0}, []uint32{0}, []uint64{last}, []uint64{lt}); err != nil {
			t.Fatal(err)
		}
		check := func(what string) {
			s := rn.Status()
			ns, err := e.ReadNode()
			if err != nil {
				t.Fatal(err)
			}
			tail, _ := st.LastIndex()
			role := map[raft.StateType]uint8{raft.StateFollower: 0, raft.StateCandidate: 1, raft.StateLeader: 2}[s.RaftState]
			if ns.Term[0] != s.Term || ns.Committed[0] != s.Commit || uint64(ns.Lead[0]) != s.Lead || ns.Role[0] != role || ns.LastIndex[0] != tail {
				t.Fatalf("n = %d after %s: etcd {term %d commit %d lead %d state %v tail %d}, restatement {term %d commit %d lead %d role %d tail %d}",
					n, what, s.Term, s.Commit, s.Lead, s.RaftState, tail, ns.Term[0], ns.Committed[0], ns.Lead[0], ns.Role[0], ns.LastIndex[0])
			}
		}
		step := func(m pb.Message, what string) StepOut {
			rn.Step(m)
			drain()
			rec := Msg{Term: m.Term, LogTerm: m.LogTerm, Index: m.Index, Commit: m.Commit, From: uint32(m.From - 1), Type: uint8(m.Type)}
			if m.Type == pb.MsgProp {
				rec.Flags, rec.Resv = MsgfEntries, uint64(len(m.Entries))
			}
			out := make([]StepOut, 1)
			if _, err := e.StepBatch([]Msg{rec}, out); err != nil {
				t.Fatal(err)
			}
			check(what)
			return out[0]
		}
		from := uint64(1) // (N = 1: the only possible sender is the node itself)
		if n > 1 {
			from = 2
		}
		prop := func(k int) pb.Message {
			ents := make([]pb.Entry, k)
			for i := range ents {
				ents[i] = pb.Entry{Data: []byte{byte(i)}, Term: 77, Index: 99} // (appendEntry overwrites Term and Index)
			}
			return pb.Message{Type: pb.MsgProp, From: from, To: 1, Entries: ents}
		}
		// a follower without a leader drops it
		if o := step(prop(1), "MsgProp on a leaderless follower"); o.Type != OutNone {
			t.Fatalf("leaderless follower: type %d", o.Type)
		}
		rn.Campaign()
		drain()
		if _, err := e.StepBatch([]Msg{{Type: uint8(pb.MsgHup)}}, make([]StepOut, 1)); err != nil {
			t.Fatal(err)
		}
		check("MsgHup")
		term := rn.Status().Term
		if n > 1 { // a candidate drops it, then wins
			if o := step(prop(2), "MsgProp on a candidate"); o.Type != OutNone {
				t.Fatalf("candidate: type %d", o.Type)
			}
			step(pb.Message{Type: pb.MsgVoteResp, From: 2, To: 1, Term: term}, "MsgVoteResp")
		}
		for i := 0; i < 100; i++ {
			k := 1 + rng.Intn(4)
			before, _ := st.LastIndex()
			o := step(prop(k), "MsgProp on the leader")
			if o.Type != OutProposed || o.Index != before+1 || o.LastIndex != before+uint64(k) || o.LogTerm != term {
				t.Fatalf("leader: %+v, tail before %d, %d entries", o, before, k)
			}
			if n > 1 && rng.Intn(2) == 0 { // an acknowledgement somewhere at or below the new tail
				tail, _ := st.LastIndex()
				step(pb.Message{Type: pb.MsgAppResp, From: 2, To: 1, Term: term, Index: uint64(rng.Int63n(int64(tail) + 1))}, "MsgAppResp")
			}
		}
		if n > 1 { // a heartbeat of a newer leader, then the proposal is forwarded to it
			step(pb.Message{Type: pb.MsgHeartbeat, From: 3, To: 1, Term: term + 1}, "MsgHeartbeat of a newer term")
			if o := step(prop(1), "MsgProp on a follower"); o.Type != OutForward || o.To != 2 {
				t.Fatalf("follower: %+v", o)
			}
		}
	}
}
