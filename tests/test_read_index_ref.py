"""CPU: the ReadIndex reference (tests/ref_read_index.py) held to the header's rules by hand, shown to say what ref_lead_transfer says
with the switch off, shown to discriminate on every input the GPU tests step (tests/test_read_index_gpu.py compares the kernels with
it, so an input on which a rule never fires would pass for lack of traffic), held against an independent model of upstream's readOnly
on lossy traces, and run as three nodes: a forwarded read, a cut-off leader in both modes, a lost round."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import _widegen as WG
from tests import ref_lead_transfer as T
from tests import ref_raft_py as R
from tests import ref_read_index as RI
from tests import ref_step_props as P
from tests import ref_step_voters as V

CASES = RI.case_list()
READY = RI.FlagReadReady


def _state(n=3, me=0, g=8):
    """g groups at term 4 with a log of 9 entries of which 7 are committed; nobody leads"""
    s = pyoracle.NodeState(g, n, me)
    s.term[:], s.last_index[:], s.last_term[:], s.committed[:] = 4, 9, 4, 7
    s.match[me] = 9
    return s


def _lead(s, groups, first_idx=1):
    s.role[groups], s.lead[groups], s.vote[groups], s.first_idx[groups] = 2, s.self_peer + 1, s.self_peer + 1, first_idx


def _batch(recs):
    m = np.zeros(len(recs), pyoracle.STEP_MSG_DT)
    for i, kw in enumerate(recs):
        RI._rec(m, i, **kw)
    return m


def _got(out):
    return [(int(o["type"]), int(o["index"]), int(o["log_term"]), int(o["flags"]) & READY, int(o["to"])) for o in out]


# ---- the nine rules, by hand -------------------------------------------------------------------------------------------------------
def test_rules_2_3_5_the_leader_numbers_confirms_and_resends():
    """N = 3, self 0 leads group 0 with the gate open: two requests, the acknowledgement of round 2 (both released), a duplicate, a
    late one, a number never handed out, a beat with nothing pending, a third request and the beat that resends its round"""
    s, x = _state(), RI.zero_extra(8, 3)
    _lead(s, [0])
    m = _batch([dict(group=0, type=RI.MsgReadIndex, frm=0),                                # 0  local
                dict(group=0, type=RI.MsgReadIndex, term=4, frm=2),                        # 1  forwarded by peer 2
                dict(group=0, type=R.MsgHeartbeatResp, term=4, frm=1, index=2),            # 2  round 2: self + 1 = the quorum
                dict(group=0, type=R.MsgHeartbeatResp, term=4, frm=1, index=2),            # 3  duplicate
                dict(group=0, type=R.MsgHeartbeatResp, term=4, frm=2, index=1),            # 4  late, of round 1
                dict(group=0, type=R.MsgHeartbeatResp, term=4, frm=2, index=9),            # 5  c > seq
                dict(group=0, type=R.MsgBeat),                                             # 6  nothing pending
                dict(group=0, type=RI.MsgReadIndex, frm=0),                                # 7
                dict(group=0, type=R.MsgBeat),                                             # 8  round 3 again
                dict(group=0, type=R.MsgHeartbeatResp, term=4, frm=2, index=3)])           # 9
    out = RI.step_batch(s, None, x, m)
    assert _got(out) == [(RI.OutReadIndex, 7, 1, 0, 0), (RI.OutReadIndex, 7, 2, 0, 2), (R.OutProgress, 0, 2, READY, 1), (R.OutProgress, 0, 0, 0, 1),
                         (R.OutProgress, 0, 0, 0, 2), (R.OutProgress, 0, 0, 0, 2), (R.OutBcastHeartbeat, 0, 0, 0, 0), (RI.OutReadIndex, 7, 3, 0, 0),
                         (R.OutBcastHeartbeat, 3, 0, 0, 0), (R.OutProgress, 0, 3, READY, 2)]
    assert int(x.seq[0]) == 3 and x.acked[:, 0].tolist() == [3, 2, 3]
    assert int(x.active[0]) == 0b110 and (x.seq[1:] == 0).all() and (x.acked[:, 1:] == 0).all()  # the activity bit as always; no other group moved
    assert RI.confirmed_of(x, None, 3)[0] == 3


def test_rule_2_the_gate_the_counter_and_the_lease_mode():
    s, x = _state(), RI.zero_extra(8, 3)
    _lead(s, [0, 1, 2, 3])
    s.first_idx[0] = 0                     # no entry of the term yet
    s.first_idx[1] = 8                     # ... or not committed (committed = 7)
    x.seq[2] = RI.SEQ_MAX - 1
    x.seq[3], x.acked[:, 3] = RI.SEQ_MAX, RI.SEQ_MAX
    m = _batch([dict(group=grp, type=RI.MsgReadIndex, frm=0) for grp in (0, 1, 2, 2, 3)])
    out = RI.step_batch(s, None, x, m)
    assert _got(out) == [(R.OutNone, 0, 0, 0, 0), (R.OutNone, 0, 0, 0, 0), (RI.OutReadIndex, 7, RI.SEQ_MAX, 0, 0), (R.OutNone, 0, 0, 0, 0),
                         (R.OutNone, 0, 0, 0, 0)]
    assert x.seq[:4].tolist() == [0, 0, RI.SEQ_MAX, RI.SEQ_MAX] and int(x.acked[0, 2]) == RI.SEQ_MAX
    # RAFTQ_READ_LEASE: released at once, no number, no state; the gate holds there too
    s, x = _state(), RI.zero_extra(8, 3)
    _lead(s, [0, 1])
    s.first_idx[0] = 0
    m = _batch([dict(group=0, type=RI.MsgReadIndex, frm=0), dict(group=1, type=RI.MsgReadIndex, term=4, frm=1), dict(group=1, type=R.MsgBeat),
                dict(group=1, type=R.MsgHeartbeatResp, term=4, frm=1, index=1)])
    out = RI.step_batch(s, None, x, m, mode=RI.LEASE)
    assert _got(out) == [(R.OutNone, 0, 0, 0, 0), (RI.OutReadIndex, 7, 0, READY, 1), (R.OutBcastHeartbeat, 0, 0, 0, 0), (R.OutProgress, 0, 0, 0, 1)]
    assert (x.seq == 0).all() and (x.acked == 0).all()


def test_rule_2_masks_one_voter_is_ready_at_once_and_a_non_voter_does_not_count():
    s, x = _state(n=5, me=1), RI.zero_extra(8, 5)
    _lead(s, [0, 1, 2])
    voters = np.full(8, 0b11111, np.uint16)
    voters[0], voters[1], voters[2] = 0b00010, 0b01111, 0  # self alone | slot 4 is no voter | nobody
    m = _batch([dict(group=0, type=RI.MsgReadIndex, frm=1),
                dict(group=1, type=RI.MsgReadIndex, frm=1),
                dict(group=1, type=R.MsgHeartbeatResp, term=4, frm=4, index=1),   # stored, not counted
                dict(group=1, type=R.MsgHeartbeatResp, term=4, frm=0, index=1),   # 2 of 4 voters: q = 3
                dict(group=1, type=R.MsgHeartbeatResp, term=4, frm=3, index=1),   # the quorum
                dict(group=2, type=RI.MsgReadIndex, frm=1)])                      # an empty mask confirms nothing
    out = RI.step_batch(s, voters, x, m)
    assert _got(out) == [(RI.OutReadIndex, 7, 1, READY, 1), (RI.OutReadIndex, 7, 1, 0, 1), (R.OutProgress, 0, 0, 0, 4), (R.OutProgress, 0, 0, 0, 0),
                         (R.OutProgress, 0, 1, READY, 3), (RI.OutReadIndex, 7, 1, 0, 1)]
    assert x.acked[:, 1].tolist() == [1, 1, 0, 1, 1] and RI.confirmed_of(x, voters, 5)[:3].tolist() == [1, 1, 0]


def test_rule_4_reset_clears_and_a_passing_check_does_not():
    s, x = _state(), RI.zero_extra(8, 3)
    _lead(s, [0, 1, 2])
    x.seq[:3], x.acked[0, :3], x.acked[1, :3] = 5, 5, 4
    x.active[1], x.active[2] = 0b111, 0
    m = _batch([dict(group=0, type=R.MsgApp, term=5, frm=1, index=9, log_term=4),  # a higher term: becomeFollower
                dict(group=0, type=R.MsgHeartbeatResp, term=4, frm=2, index=5),     # stale
                dict(group=1, type=12),                                             # the check passes
                dict(group=2, type=12)])                                            # the check fails: step-down
    out = RI.step_batch(s, None, x, m)
    assert x.seq[:3].tolist() == [0, 5, 0] and x.acked[:, :3].T.tolist() == [[0, 0, 0], [5, 4, 0], [0, 0, 0]]
    assert s.role[:3].tolist() == [0, 2, 0] and int(out[3]["flags"]) & R.FlagSteppedDown


def test_rule_6_followers_candidates_and_the_term_rules():
    s, x = _state(g=8), RI.zero_extra(8, 3)
    s.lead[0], s.lead[1], s.lead[3] = 2, 0, 3  # follows slot 1 | nobody | slot 2
    s.role[2] = 1                              # a candidate
    _lead(s, [4])
    m = _batch([dict(group=0, type=RI.MsgReadIndex, frm=0),                                   # 0  forwarded to slot 1
                dict(group=0, type=RI.MsgReadIndex, term=4, frm=2),                           # 1  a forwarded one is forwarded again
                dict(group=0, type=R.MsgHeartbeat, term=4, frm=1, index=6, ),                 # 2  echoed
                dict(group=0, type=RI.MsgReadIndexResp, term=4, frm=1, index=7),              # 3  the read state
                dict(group=0, type=RI.MsgReadIndexResp, term=3, frm=1, index=8),              # 4  a lower term: ignored
                dict(group=1, type=RI.MsgReadIndex, frm=0),                                   # 5  no leader
                dict(group=2, type=RI.MsgReadIndex, frm=0),                                   # 6  a candidate
                dict(group=2, type=RI.MsgReadIndexResp, term=4, frm=1, index=7),              # 7
                dict(group=2, type=R.MsgHeartbeat, term=4, frm=1, index=11),                  # 8  becomes a follower and echoes
                dict(group=3, type=RI.MsgReadIndexResp, term=6, frm=1, index=7),              # 9  a higher term: follows nobody, then the state
                dict(group=4, type=RI.MsgReadIndexResp, term=4, frm=1, index=7),              # 10 a leader ignores it
                dict(group=4, type=RI.MsgReadIndex, term=9, frm=1)])                          # 11 a higher term on a request: follows nobody, so nothing to forward to
    out = RI.step_batch(s, None, x, m)
    assert _got(out) == [(P.OutForward, 0, 0, 0, 1), (P.OutForward, 0, 0, 0, 1), (R.OutHeartbeatResp, 6, 0, 0, 1), (RI.OutReadState, 7, 0, 0, 1),
                         (R.OutNone, 0, 0, 0, 1), (R.OutNone, 0, 0, 0, 0), (R.OutNone, 0, 0, 0, 0), (R.OutNone, 0, 0, 0, 1),
                         (R.OutHeartbeatResp, 11, 0, 0, 1), (RI.OutReadState, 7, 0, 0, 1), (R.OutNone, 0, 0, 0, 1), (R.OutNone, 0, 0, 0, 1)]
    assert (int(s.term[3]), int(s.lead[3]), int(s.role[3])) == (6, 0, 0) and (int(s.term[4]), int(s.lead[4]), int(s.role[4])) == (9, 0, 0)
    assert int(s.role[2]) == 0 and int(s.lead[2]) == 2 and (x.seq == 0).all()


# ---- the switch off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [c for c in T.case_list() if not c.get("hot")][::3], ids=T.case_id)
def test_switch_off_is_ref_lead_transfer(kw):
    """mode 0 on inputs without the new kinds: the bytes and the state ref_lead_transfer gives, whatever the heartbeats' index says"""
    start, voters, m, want, after = T.step_case(**kw)
    s, x = V.copy_state(start[0]), RI.Extra(start[1].copy(), start[2].copy(), start[3].copy(), np.zeros(s_g := start[0].G, np.uint32),
                                             np.zeros((start[0].N, s_g), np.uint32))
    got = RI.step_batch(s, voters, x, np.array(m), mode=0, pre_vote=kw.get("pre_vote", True))
    assert got.tobytes() == np.array(want).tobytes()
    assert np.array_equal(x.active, after[1]) and np.array_equal(x.lead_elapsed, after[2]) and np.array_equal(x.transferee, after[3])
    assert (x.seq == 0).all() and (x.acked == 0).all()
    for name, _ in pyoracle.NodeState.FIELDS:
        assert np.array_equal(getattr(s, name), getattr(after[0], name)), name


# ---- every GPU input discriminates -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CASES, ids=RI.case_id)
def test_every_gpu_input_discriminates(kw):
    start, voters, m, want, after = RI.step_case(**kw)
    sw = RI.case_switches(kw)
    assert len(m) == RI.N_MSGS and start[0].G == RI.G
    for rule in RI.case_rules(kw):
        assert len(RI.changed_records(start, voters, m, want, after, rule, **sw)) >= RI.ARM_FLOOR, (rule, RI.RULE_NAMES[rule])
    a = RI.arms(start, voters, m, **sw)
    for arm in RI.arm_floors(kw):
        assert a[arm] >= RI.ARM_FLOOR, (arm, dict(a))
    x0, x1 = start[1], after[1]
    if sw["mode"] == RI.SAFE:
        assert (x0.seq == RI.SEQ_MAX - 1).sum() >= RI.PLANT and (x1.seq == RI.SEQ_MAX).sum() >= RI.PLANT  # one request taken, the next dropped
        if kw["n"] == 9 and not kw.get("hot"):  # nine distinct acknowledgement words: every selection slot live
            assert (np.sort(x0.acked, axis=0)[1:] != np.sort(x0.acked, axis=0)[:-1]).all(axis=0).sum() >= RI.PLANT
    else:
        assert (x1.seq == 0).all() and (x1.acked == 0).all()
        ready = want["type"] == RI.OutReadIndex
        assert ready.sum() >= RI.ARM_FLOOR and ((want["flags"][ready] & READY) != 0).all() and (want["log_term"][ready] == 0).all()
    if kw.get("hot"):
        grp = np.bincount(m["group"].astype(np.int64)).argmax()
        mine = m["group"] == grp
        assert mine.sum() > 32 and (m["type"][mine] == RI.MsgReadIndex).sum() == 3
        acks = m[mine][m["type"][mine] == R.MsgHeartbeatResp]
        ctx = acks["index"].astype(np.int64)
        assert (np.diff(ctx) < 0).any() and any((acks[i]["from"], ctx[i]) == (acks[i + 1]["from"], ctx[i + 1]) for i in range(len(acks) - 1))  # out of order, a duplicate
        assert ((want["flags"][mine] & READY) != 0).any()


def test_the_cases_cover_the_switches():
    seen = {(c.get("masks", False), c.get("pre_vote", True), c.get("lead_transfer", True)) for c in CASES if c.get("mode", RI.SAFE) == RI.SAFE}
    assert len(seen) == 8
    assert {(c["n"], c["self_peer"]) for c in CASES} >= set(RI.SHAPES)


# ---- against upstream's readOnly, on lossy traces ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mask,seed", [(3, None, 1), (5, None, 2), (9, None, 3), (5, 0b01111, 4), (9, 0b101010101, 5), (5, 0b00001, 6), (3, 0b110, 7)])
def test_traces_with_loss_duplication_and_reordering(n, mask, seed):
    """one led group, self 0; requests arrive, every request's round goes to every peer, and the acknowledgements are lost, doubled
    and reordered.  After every message: what upstream's readOnly has released is a subset of what this rule has, and every read
    this rule has released has at least q members -- self included -- whose acknowledged round is >= its number."""
    rng = np.random.default_rng(seed)
    s, x = _state(n=n, me=0, g=1), RI.zero_extra(1, n)
    _lead(s, [0])
    voters = None if mask is None else np.array([mask], np.uint16)
    members = [p for p in range(n) if mask is None or (mask >> p) & 1]
    q = len(members) // 2 + 1
    ro = RI.ReadOnly()
    mine, theirs = set(), set()
    truly = {p: 0 for p in range(n)}  # the largest round each peer has really acknowledged to the leader
    truly_self = 0
    wire = []                         # acknowledgements in flight: (peer, context)
    asked = 0
    for step in range(400):
        if rng.random() < 0.25 or not wire:
            out = RI.step_batch(s, voters, x, _batch([dict(group=0, type=RI.MsgReadIndex, frm=0)]))[0]
            assert int(out["type"]) == RI.OutReadIndex
            asked += 1
            sq = int(out["log_term"])
            assert sq == asked
            truly_self = sq
            ro.add_request(7, sq, 0)
            if 0 in members and q == 1:  # upstream's single-voter shortcut
                theirs |= {c for c, _ in ro.advance(sq)}
            if int(out["flags"]) & READY:
                mine |= set(range(1, sq + 1))
            for p in range(1, n):
                for _ in range(int(rng.choice([0, 1, 1, 2]))):  # lost, delivered, doubled
                    wire.insert(int(rng.integers(0, len(wire) + 1)), (p, sq))  # ... and reordered
        else:
            p, c = wire.pop(int(rng.integers(0, len(wire))))
            truly[p] = max(truly[p], c)
            out = RI.step_batch(s, voters, x, _batch([dict(group=0, type=R.MsgHeartbeatResp, term=4, frm=p, index=c)]))[0]
            if int(out["flags"]) & READY:
                mine |= set(range(1, int(out["log_term"]) + 1))
            acks = ro.recv_ack(p, c)
            if acks is not None and len(acks & set(members)) >= q:
                theirs |= {ctx for ctx, _ in ro.advance(c)}
        assert theirs <= mine, (step, sorted(theirs - mine))
        for sq in mine:
            have = sum(1 for p in members if (truly_self if p == 0 else truly[p]) >= sq)
            assert have >= q, (step, sq, have)
        assert mine == set(range(1, int(RI.confirmed_of(x, voters, n)[0]) + 1))
    assert asked > 50 and (len(mine) > 20 or 0 not in members or q > len(members))
    if mask is None:
        assert len(theirs) > 10 and len(mine) > len(theirs) - 1


# ---- three nodes -------------------------------------------------------------------------------------------------------------------
G_SCENARIO = 6
CLUSTER_KW = dict(election_tick=5, heartbeat_tick=2)


def forwarded_read(c):
    """node 1 asks: its MsgReadIndex is forwarded to node 0, numbered, confirmed by a round, answered with MsgReadIndexResp, and
    arrives as RAFTQ_OUT_READ_STATE with an index >= every commit that preceded the request"""
    commit_before = c.s[0].committed.copy()
    c.inject(1, RI.read_msgs(range(c.g), frm=1))
    c.run(4)
    got = dict(c.released[1])
    assert sorted(got) == list(range(c.g)), c.released
    assert all(got[grp] >= int(commit_before[grp]) for grp in got)
    kinds = [int(t) for k, _, outs in c.log if k == 1 for t in outs["type"]]
    assert P.OutForward in kinds and RI.OutReadState in kinds
    if c.mode == RI.SAFE:
        lead = [o for k, _, outs in c.log if k == 0 for o in outs]
        assert any(int(o["type"]) == RI.OutReadIndex and not int(o["flags"]) & READY for o in lead)
        assert any(int(o["type"]) == R.OutProgress and int(o["flags"]) & READY for o in lead)
        assert (c.x[0].seq == 1).all() and (RI.confirmed_of(c.x[0], None, 3) == 1).all()
    assert c.converged() and (c.leaders()[1] == 0).all()


def cut_off_leader(c):
    """node 0 is cut off from its followers and asked for reads every round.  RAFTQ_READ_SAFE: never one RAFTQ_OUTF_READ_READY.
    RAFTQ_READ_LEASE: it releases until its CheckQuorum fires -- the documented difference between the modes."""
    c.cut = {0}
    stale = 0
    for _ in range(2 * c.et + 2):
        led = np.flatnonzero(c.s[0].role == 2)
        c.inject(0, RI.read_msgs(led, frm=0))
        before = len(c.released[0])
        c.round()
        stale += len(c.released[0]) - before
    assert (c.s[0].role != 2).all()  # the check fired
    if c.mode == RI.SAFE:
        assert stale == 0 and not any(int(o["flags"]) & READY for k, _, outs in c.log if k == 0 for o in outs)
        assert (c.x[0].seq == 0).all() and all(not v for v in c.queue[0].values())  # the step-down cleared the record, the host its queue
    else:
        assert stale >= c.g


def lost_round(c):
    """the round of a read is lost on the wire; rule 5's heartbeat carries the number again and the read is released"""
    drop = {"on": True, "n": 0}

    def lose(k, p, one):
        if drop["on"] and k == 0 and int(one["type"]) == R.MsgHeartbeat and int(one["index"]) != 0:
            drop["n"] += 1
            return True
        return False

    c.lose = lose
    c.inject(0, RI.read_msgs(range(c.g), frm=0))
    c.turn(0)
    assert drop["n"] == 2 * c.g and not c.released[0]
    drop["on"] = False
    c.run(c.ht + 2)
    assert sorted(grp for grp, _ in c.released[0]) == list(range(c.g))
    beats = [o for k, b, outs in c.log if k == 0 for o in outs if int(o["type"]) == R.OutBcastHeartbeat]
    assert any(int(o["index"]) == 1 for o in beats)


SCENARIOS = {forwarded_read: (RI.SAFE, RI.LEASE), cut_off_leader: (RI.SAFE, RI.LEASE), lost_round: (RI.SAFE,)}


@pytest.mark.parametrize("pre_vote", [False, True])
@pytest.mark.parametrize("scenario,mode", [(f, md) for f, modes in SCENARIOS.items() for md in modes], ids=lambda v: getattr(v, "__name__", str(v)))
def test_three_nodes(scenario, mode, pre_vote):
    scenario(RI.Cluster(G_SCENARIO, pre_vote, mode=mode, **CLUSTER_KW))


def test_lost_round_needs_rule_5():
    c = RI.Cluster(G_SCENARIO, True, ri_leave_out={5}, **CLUSTER_KW)
    with pytest.raises(AssertionError):
        lost_round(c)


# ---- the band cases: 64-bit terms, indices and contexts --------------------------------------------------------------------------------
BAND_CASES = [kw for kw in CASES if kw.get("band")]
B32 = [kw for kw in BAND_CASES if kw["band"] == "b32"]
B63 = [kw for kw in BAND_CASES if kw["band"] == "b63"]


def test_the_band_cases_are_the_issue_s():
    per_band = [(kw["band"], kw["n"], bool(kw.get("masks"))) for kw in BAND_CASES[:6]]
    assert per_band == [(b, n, mk) for b in WG.BAND_NAMES for n, mk in ((3, False), (9, True))]
    assert [(kw["band"], kw.get("mode", RI.SAFE), bool(kw.get("hot"))) for kw in BAND_CASES[6:]] == [("b63", RI.LEASE, False), ("b32", RI.SAFE, True)]
    assert CASES[-len(BAND_CASES):] == BAND_CASES and len({RI.case_id(kw) for kw in CASES}) == len(CASES)  # appended, ids of their own
    assert {kw.get("pre_vote", True) for kw in BAND_CASES} == {kw.get("lead_transfer", True) for kw in BAND_CASES} == {False, True}


@pytest.mark.parametrize("kw", BAND_CASES, ids=RI.case_id)
def test_band_cases_are_where_they_say(kw):
    _, _, m, want, after = RI.step_case(**kw)
    WG.check_in_band(kw["band"], want, kw)
    WG.guard_case(after[0], m)
    beats = np.isin(m["type"], (R.MsgHeartbeat, R.MsgHeartbeatResp))
    assert (m["index"][beats] >= 2**32).sum() >= RI.ARM_FLOOR  # contexts the 32-bit record cannot hold


@pytest.mark.parametrize("kw", B32, ids=RI.case_id)
def test_a_32_bit_reading_of_the_b32_case_decides_differently(kw):
    """the reference over the same start and batch with every 64-bit word reduced mod 2^32 (a context of 2^32 + 1 then reads as round
    1): measured 32.8 % / 28.1 % / 22.3 % (the hot case) of the 512 records differ in (type, reject, flags, role), 23 / 22 / 16 of them
    of types 12..18; the floors are 10 % and 8"""
    start, voters, m, want, _ = RI.step_case(**kw)
    s32, m32 = WG.low32(start[0], m)
    want32 = RI.step_batch(s32, voters, start[1].copy(), m32, **RI.case_switches(kw))
    WG.check_narrow_reading(m, want, want32, WG.OWN_KINDS, kw)


@pytest.mark.parametrize("kw", B63, ids=RI.case_id)
def test_the_b63_case_compares_across_the_sign_bit(kw):
    """measured: 37.5 % / 33.8 % / 36.9 % (the lease case) of the records have m.term : term or m.index : last_index on opposite sides
    of 2^63, 23 / 19 / 16 of them of types 12..18; the floors are 5 % and PLANT"""
    start, _, m, _, _ = RI.step_case(**kw)
    WG.check_straddles(start[0], m, WG.OWN_KINDS, RI.PLANT, kw)


@pytest.mark.parametrize("kw", BAND_CASES, ids=RI.case_id)
def test_the_gate_the_contexts_and_the_read_states_by_hand(kw):
    """the band-only plants: per record (type, index, log_term, READ_READY), and the read record after, written out"""
    band, safe = kw["band"], kw.get("mode", RI.SAFE) == RI.SAFE
    plants = {}
    start, _, m, want, after = RI.step_case(**kw, plants=plants)
    s0, x1 = start[0], after[1]
    H = RI.PLANT // 2

    def got(grp):
        at = np.flatnonzero(m["group"] == grp)
        return _got(want[at]), m[at]

    # the gate: committed >= first_idx, as 64-bit words
    assert len(plants["same"]) == len(plants["apart"]) == 2 * H
    for name in ("same", "apart"):
        for grp in plants[name]:
            recs, sent = got(grp)
            c, f = int(s0.committed[grp]), int(s0.first_idx[grp])
            assert c >= (WG.band_floor(band)[1] - 1 if name == "same" else 2**32 + 1) and c == int(s0.last_index[grp]) - 1
            assert f == (c if name == "same" else c - 2**32) and f >= 1
            assert int(sent["type"][0]) == RI.MsgReadIndex
            assert recs[0][:4] == ((RI.OutReadIndex, c, 1, 0) if safe else (RI.OutReadIndex, c, 0, READY)), (name, recs[0])  # open: the index whole
    closed = plants["closed"]
    assert [int(s0.first_idx[grp]) for grp in closed[::2]] == [0] * H and int(s0.first_idx[closed[1]]) == int(s0.committed[closed[1]]) + 1
    if band != "top":
        assert int(s0.first_idx[closed[-1]]) == int(s0.committed[closed[-1]]) + 2**32
    for grp in closed:
        recs, _ = got(grp)
        assert [r[:4] for r in recs] == [(R.OutNone, 0, 0, 0)], recs  # closed: dropped
    # contexts at and above 2^32 are beyond every seq: nothing stored, nothing released
    for grp in plants["beyond"]:
        recs, sent = got(grp)
        assert [int(c) for c in sent["index"]] == [5, 0, 2**32 + 1, 2**32, 2**63 + 2] and (sent["type"] == R.MsgHeartbeatResp).all()
        assert [r[:4] for r in recs] == [(R.OutProgress, int(s0.match[p, grp]), 0, 0) for p in sent["from"]]  # (the sender's Match, as always)
        if safe:
            assert int(start[1].seq[grp]) == int(x1.seq[grp]) == 3 and x1.acked[:, grp].tolist() == [3 if p == s0.self_peer else 0 for p in range(s0.N)]
    # a heartbeat's context is echoed whole, by a follower and by a candidate (which follows the sender first)
    for name in ("fwd", "cnd"):
        for grp in plants[name]:
            recs, sent = got(grp)
            assert int(sent["type"][-1]) == R.MsgHeartbeat and int(sent["index"][-1]) == 2**32 + 7
            assert recs[-1][:4] == (R.OutHeartbeatResp, 2**32 + 7, 0, 0) and int(after[0].role[grp]) == 0
    # a MsgReadIndexResp's index -- the lifted committed -- arrives whole
    for grp in plants["rstate"]:
        recs, sent = got(grp)
        idx = plants["read_at"][int(grp)]
        assert idx >= 2**32 and idx in (int(s0.committed[grp]), WG.band_edge(band) + list(plants["rstate"]).index(grp))
        assert int(sent["type"][1]) == RI.MsgReadIndexResp and int(sent["index"][1]) == idx
        assert recs[0][:4] == (R.OutNone, 0, 0, 0) and recs[1][:4] == (RI.OutReadState, idx, 0, 0)
