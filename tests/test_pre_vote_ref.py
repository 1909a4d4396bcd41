"""tests/ref_pre_vote.py held to a hand table and to the references below it (CPU): the Step reference gives what include/raftq_step.h
"PreVote" says row by row, every input the GPU tests step tells each of the five rules from its absence (the floors are asserted
here), and the three-node scenario shows the reason for the feature on the reference alone."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import _widegen as WG
from tests import ref_check_quorum as Q
from tests import ref_pre_vote as PV
from tests import ref_raft_py as R
from tests import ref_step_voters as V

F, C, L, P = 0, 1, 2, 3  # roles
HS, CM, DOWN = R.FlagHardState, R.FlagCommitted, R.FlagSteppedDown
PRE_VOTE, PRE_RESP = PV.MsgPreVote, PV.MsgPreVoteResp
CAMPAIGN, LEADER, PRE_CAMPAIGN, PV_RESP, TERM_RESP = R.OutCampaign, R.OutBecameLeader, PV.OutPreCampaign, PV.OutPreVoteResp, PV.OutTermResp


def _group(n, me, role, term=5, lead=None, elapsed=0, vote=None, last_index=7, votes=None):
    s = pyoracle.NodeState(1, n, me)
    s.role[0], s.term[0], s.elapsed[0], s.last_index[0], s.last_term[0] = role, term, elapsed, last_index, term
    s.lead[0] = (me + 1 if role == L else 0) if lead is None else lead
    s.vote[0] = (me + 1 if role != F else 0) if vote is None else vote
    s.first_idx[0] = 1 if role == L else 0
    s.match[me, 0] = last_index
    if role in (C, P):
        s.votes[me, 0] = 1
    for p, v in (votes or {}).items():
        s.votes[p, 0] = v
    return s


def _msg(type, frm=0, term=0, index=0, log_term=0, reject=0, flags=0):
    m = np.zeros(1, pyoracle.STEP_MSG_DT)
    m["type"], m["from"], m["term"], m["index"], m["log_term"], m["reject"] = type, frm, term, index, log_term, reject
    m["_pad"][0] = (0, flags)
    return m


# Every group: term 5, the log ends at (7, 5), election_tick 10.  `frm` is a slot; vote and lead are slot + 1.
# (what, n, self, role, kwargs of the group, voters | None, message, -> type, reject, index, flags, role, lead, term, vote, more)
TABLE = [
    # rule 1
    ("MsgHup on a follower: pre-candidate, nothing to persist", 3, 0, F, dict(lead=2, elapsed=3, vote=3), None, _msg(R.MsgHup), PRE_CAMPAIGN, 0, 7, 0, P, 0, 5, 3, dict(log_term=5, elapsed=0, votes=[1, 0, 0])),
    ("MsgHup on a candidate: no STEPPED_DOWN", 3, 0, C, dict(votes={1: 2}), None, _msg(R.MsgHup), PRE_CAMPAIGN, 0, 7, 0, P, 0, 5, 1, dict(votes=[1, 0, 0])),
    ("MsgHup on a pre-candidate: the pre-election starts over", 3, 0, P, dict(votes={2: 2}), None, _msg(R.MsgHup), PRE_CAMPAIGN, 0, 7, 0, P, 0, 5, 1, dict(votes=[1, 0, 0])),
    ("MsgHup on a leader is ignored", 3, 0, L, {}, None, _msg(R.MsgHup), R.OutNone, 0, 0, 0, L, 1, 5, 1, {}),
    ("N = 1: MsgHup is the whole election, as without the switch", 1, 0, F, {}, None, _msg(R.MsgHup), LEADER, 0, 8, HS | CM, L, 1, 6, 1, dict(log_term=6)),
    ("masked, self is no voter: the grant is recorded, not counted", 3, 0, F, {}, 0b110, _msg(R.MsgHup), PRE_CAMPAIGN, 0, 7, 0, P, 0, 5, 0, dict(votes=[1, 0, 0])),
    ("masked, self is the one voter: straight on", 3, 0, F, {}, 0b001, _msg(R.MsgHup), LEADER, 0, 8, HS | CM, L, 1, 6, 1, {}),
    # rule 2
    ("MsgPreVote of a higher term to a leader: in lease, ignored", 3, 0, L, {}, None, _msg(PRE_VOTE, 2, 6, 9, 6), R.OutNone, 0, 0, 0, L, 1, 5, 1, {}),
    ("... to a follower in lease: ignored", 3, 0, F, dict(lead=2, elapsed=9), None, _msg(PRE_VOTE, 2, 6, 9, 6), R.OutNone, 0, 0, 0, F, 2, 5, 0, dict(elapsed=9)),
    ("... out of lease: granted with the message's term, nothing changes", 3, 0, F, dict(lead=2, elapsed=10), None, _msg(PRE_VOTE, 2, 6, 9, 6), PV_RESP, 0, 6, 0, F, 2, 5, 0, dict(elapsed=10)),
    ("MsgVote of a higher term in lease is still ignored", 3, 0, L, {}, None, _msg(R.MsgVote, 2, 6, 9, 6), R.OutNone, 0, 0, 0, L, 1, 5, 1, {}),
    ("a granting MsgPreVoteResp of a higher term to a follower: no term moves", 3, 0, F, dict(lead=2), None, _msg(PRE_RESP, 1, 6), R.OutNone, 0, 0, 0, F, 2, 5, 0, {}),
    ("a rejecting one: becomeFollower(m.term, None)", 3, 0, P, {}, None, _msg(PRE_RESP, 1, 8, reject=1), R.OutNone, 0, 0, HS | DOWN, F, 0, 8, 0, dict(votes=[0, 0, 0])),
    ("... to a leader too, and its lead is None", 3, 0, L, {}, None, _msg(PRE_RESP, 1, 8, reject=1), R.OutNone, 0, 0, HS | DOWN, F, 0, 8, 0, {}),
    ("a MsgHeartbeat of a higher term keeps its 2015 rule", 3, 0, P, {}, None, _msg(R.MsgHeartbeat, 1, 6), R.OutHeartbeatResp, 0, 0, HS | DOWN, F, 2, 6, 0, {}),
    # rule 3
    ("MsgPreVote of a lower term: rejected with the own term", 3, 0, F, dict(lead=2, elapsed=11), None, _msg(PRE_VOTE, 2, 4, 9, 4), PV_RESP, 1, 5, 0, F, 2, 5, 0, dict(elapsed=11)),
    ("a stale MsgHeartbeat: TERM_RESP, no clock reset", 3, 0, F, dict(lead=2, elapsed=6), None, _msg(R.MsgHeartbeat, 2, 4), TERM_RESP, 0, 0, 0, F, 2, 5, 0, dict(elapsed=6)),
    ("a stale MsgApp to a leader, flags and all", 3, 0, L, {}, None, _msg(R.MsgApp, 2, 4, 7, 5, flags=V.MSGF_BARRIER | V.MSGF_ENTRIES), TERM_RESP, 0, 0, 0, L, 1, 5, 1, {}),
    ("a stale MsgVote is ignored as always", 3, 0, F, {}, None, _msg(R.MsgVote, 2, 4, 9, 4), R.OutNone, 0, 0, 0, F, 0, 5, 0, {}),
    ("a stale MsgPreVoteResp is ignored", 3, 0, P, {}, None, _msg(PRE_RESP, 1, 4, reject=1), R.OutNone, 0, 0, 0, P, 0, 5, 1, dict(votes=[1, 0, 0])),
    # rule 4
    ("a higher term grants whoever the vote went to", 3, 0, F, dict(vote=2), None, _msg(PRE_VOTE, 2, 6, 9, 6), PV_RESP, 0, 6, 0, F, 0, 5, 2, {}),
    ("... but not a log that is behind", 3, 0, F, {}, None, _msg(PRE_VOTE, 2, 6, 3, 5), PV_RESP, 1, 5, 0, F, 0, 5, 0, {}),
    ("the own term, voted for another: rejected", 3, 0, F, dict(vote=2), None, _msg(PRE_VOTE, 2, 5, 9, 5), PV_RESP, 1, 5, 0, F, 0, 5, 2, {}),
    ("the own term, voted for the sender: granted", 3, 0, F, dict(vote=3), None, _msg(PRE_VOTE, 2, 5, 7, 5), PV_RESP, 0, 5, 0, F, 0, 5, 3, {}),
    ("the own term, no vote: granted, and no vote is recorded", 3, 0, F, {}, None, _msg(PRE_VOTE, 2, 5, 7, 5), PV_RESP, 0, 5, 0, F, 0, 5, 0, {}),
    ("a candidate of the own term has voted for itself", 3, 0, C, {}, None, _msg(PRE_VOTE, 2, 5, 9, 5), PV_RESP, 1, 5, 0, C, 0, 5, 1, {}),
    ("a leader of the own term rejects", 3, 0, L, {}, None, _msg(PRE_VOTE, 2, 5, 9, 5), PV_RESP, 1, 5, 0, L, 1, 5, 1, {}),
    # rule 5
    ("a grant at term + 1 that makes the quorum: the campaign", 3, 0, P, {}, None, _msg(PRE_RESP, 1, 6), CAMPAIGN, 0, 7, HS, C, 0, 6, 1, dict(log_term=5, votes=[1, 0, 0], elapsed=0)),
    ("one grant of five is not enough", 5, 4, P, {}, None, _msg(PRE_RESP, 0, 6), R.OutNone, 0, 0, 0, P, 0, 5, 5, dict(votes=[1, 0, 0, 0, 1])),
    ("a duplicate grant counts once", 5, 4, P, dict(votes={0: 1}), None, _msg(PRE_RESP, 0, 6), R.OutNone, 0, 0, 0, P, 0, 5, 5, {}),
    ("one rejection of three is not the quorum", 3, 0, P, {}, None, _msg(PRE_RESP, 1, 5, reject=1), R.OutNone, 0, 0, 0, P, 0, 5, 1, dict(votes=[1, 2, 0])),
    ("the second is: follows nobody, Term and Vote kept", 3, 0, P, dict(votes={1: 2}), None, _msg(PRE_RESP, 2, 5, reject=1), R.OutNone, 0, 0, DOWN, F, 0, 5, 1, dict(votes=[0, 0, 0])),
    ("a pre-candidate ignores MsgVoteResp", 3, 0, P, {}, None, _msg(R.MsgVoteResp, 1, 5), R.OutNone, 0, 0, 0, P, 0, 5, 1, dict(votes=[1, 0, 0])),
    ("a candidate ignores MsgPreVoteResp", 3, 0, C, {}, None, _msg(PRE_RESP, 1, 5), R.OutNone, 0, 0, 0, C, 0, 5, 1, dict(votes=[1, 0, 0])),
    ("a leader ignores it", 3, 0, L, {}, None, _msg(PRE_RESP, 1, 5), R.OutNone, 0, 0, 0, L, 1, 5, 1, {}),
    ("a MsgHeartbeat of the own term: follows the sender", 3, 0, P, {}, None, _msg(R.MsgHeartbeat, 1, 5), R.OutHeartbeatResp, 0, 0, DOWN, F, 2, 5, 1, {}),
    ("a MsgApp of the own term likewise", 3, 0, P, {}, None, _msg(R.MsgApp, 1, 5, 7, 5), R.OutAppend, 0, 0, DOWN, F, 2, 5, 1, {}),
    ("a MsgVote of the own term is rejected", 3, 0, P, {}, None, _msg(R.MsgVote, 1, 5, 9, 5), R.OutVoteResp, 1, 0, 0, P, 0, 5, 1, {}),
    ("a MsgVote of a higher term: follower first, then the vote", 3, 0, P, {}, None, _msg(R.MsgVote, 1, 6, 9, 6), R.OutVoteResp, 0, 0, HS | DOWN, F, 0, 6, 2, {}),
    ("masked: a non-voter's grant is recorded and does not count", 3, 0, P, {}, 0b101, _msg(PRE_RESP, 1, 6), R.OutNone, 0, 0, 0, P, 0, 5, 1, dict(votes=[1, 1, 0])),
    ("masked: the voter's does", 3, 0, P, {}, 0b101, _msg(PRE_RESP, 2, 6), CAMPAIGN, 0, 7, HS, C, 0, 6, 1, {}),
]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_step_reference_against_the_hand_table(row):
    what, n, me, role, kw, voters, m, typ, reject, index, flags, role2, lead2, term2, vote2, more = row
    s = _group(n, me, role, **kw)
    elapsed0 = int(s.elapsed[0])
    vt = None if voters is None else np.array([voters], np.uint16)
    ac, le = np.array([0b010 if n > 1 else 0], np.uint16), np.array([4], np.uint32)
    o = PV.step_batch(s, vt, ac, le, m)[0]
    got = tuple(int(o[k]) for k in ("type", "reject", "index", "flags", "role", "lead", "term", "vote"))
    assert got == (typ, reject, index, flags, role2, lead2, term2, vote2), what
    assert (int(s.role[0]), int(s.lead[0]), int(s.term[0]), int(s.vote[0])) == (role2, lead2, term2, vote2), what
    if "log_term" in more:
        assert int(o["log_term"]) == more["log_term"], what
    if "elapsed" in more:
        assert int(s.elapsed[0]) == more["elapsed"], what
    if "votes" in more:
        assert s.votes[:, 0].tolist() == more["votes"], what
    if typ in (PV_RESP, TERM_RESP, PRE_CAMPAIGN) or (typ == R.OutNone and flags == 0):
        # nothing a reset() would touch has moved: the activity word, the Match row, the gate -- and, but for becomePreCandidate, the clock
        assert (int(ac[0]), int(le[0])) == (0b010 if n > 1 else 0, 4) and int(s.match[me, 0]) == 7 and int(s.committed[0]) == 0, what
        if typ != PRE_CAMPAIGN:
            assert int(s.elapsed[0]) == elapsed0, what


def test_without_its_five_rules_the_reference_is_check_quorum_s():
    """the mixin restates Step's head and overrides nothing below it: with every rule left out, traffic without the two kinds and
    without role 3 is stepped as tests/ref_check_quorum.py steps it"""
    for kw in (Q.case_list()[2], Q.case_list()[5]):
        start, voters, m, want, after = Q.step_case(**kw)
        st = (V.copy_state(start[0]), start[1].copy(), start[2].copy())
        got = PV.step_batch(st[0], voters, st[1], st[2], np.array(m), leave_out={1, 2, 3, 4, 5})
        assert got.tobytes() == want.tobytes() and not Q.state_differs(st, after), kw


CASES = PV.case_list()
FLOOR = 16  # records, per rule, over all the cases (the issue's)


def test_every_rule_discriminates_on_the_gpu_inputs():
    total = {rule: 0 for rule in (1, 2, 3, 4, 5)}
    for kw in CASES:
        start, voters, m, want, after = PV.step_case(**kw)
        new = np.isin(m["type"], (PRE_VOTE, PRE_RESP))
        assert new.sum() >= 40 and np.isin((PRE_CAMPAIGN, PV_RESP, TERM_RESP), want["type"]).all() or kw["n"] == 1, kw
        for rule in total:
            k = len(PV.changed_records(start, voters, m, want, after, rule))
            total[rule] += k
            if kw["n"] >= 3:
                assert k >= 1, ("rule %d makes no difference on this input" % rule, kw)
    for rule, k in total.items():
        assert k >= FLOOR, (rule, k)


def test_the_hot_cases_hold_a_run_the_list_walk_does_not_take():
    for kw in CASES:
        if kw.get("hot"):
            _, _, m, want, _ = PV.step_case(**kw)
            grp = np.bincount(m["group"].astype(np.int64))
            assert grp.max() >= 40
            hot = want[m["group"] == grp.argmax()]
            assert {PRE_CAMPAIGN, CAMPAIGN} <= set(hot["type"].tolist()), kw  # pre-elections are won inside the run


# ---- the reason for the feature ----------------------------------------------------------------------------------------------------
G_SCENARIO = 96
HEAL_ROUNDS = 4       # rounds from the heal to "node 2 follows node 0 everywhere": a property of the reference and the seed
INFLATED_ROUNDS = 24  # rounds until every group of the inflated-term run has one leader that the other two follow


def _cut_off(pre_vote, g=G_SCENARIO):
    c = PV.Cluster(g, pre_vote)
    c.run(2)
    c.cut = {2}
    c.run(3 * 2 * c.et)  # three election timeouts of at most 2 * election_tick ticks
    c.cut = set()
    return c


def test_check_quorum_alone_locks_the_node_out():
    c = _cut_off(False)
    assert (c.s[2].term > 1).all()
    c.run(10 * 2 * c.et)
    assert (c.s[2].term > c.s[0].term).all() and (c.s[0].role == L).all() and (c.s[0].term == 1).all()
    assert ((c.s[2].lead == 0) & (c.s[2].role != F)).all()  # it follows nobody, ten election timeouts on
    assert not c.converged()


def test_pre_vote_lets_it_back_in():
    c = _cut_off(True)
    assert (c.s[2].term == 1).all() and (c.s[2].role == P).all()  # it pre-campaigned alone and its term never moved
    c.run(HEAL_ROUNDS - 1)
    assert not c.converged()
    c.round()
    assert c.converged()
    assert (c.s[2].role == F).all() and (c.s[2].lead == 1).all() and (c.s[2].term == 1).all()
    assert (c.s[0].role == L).all() and (c.s[0].term == 1).all()  # the old leader never stepped down
    c.run(2 * 2 * c.et)
    assert c.converged() and (c.s[0].role == L).all() and (c.s[0].term == 1).all()


def test_an_inflated_term_brings_the_leader_down_and_the_group_converges():
    c = PV.Cluster(G_SCENARIO, True)
    c.s[2].term[:], c.s[2].lead[:], c.s[2].vote[:] = 7, 0, 0
    seen = []
    c.on_step = lambda k, batch, outs: seen.append((k, outs))
    c.run(2)  # (heartbeat_tick is 2: the first beat falls on the second tick)
    # node 2 answered node 0's heartbeat with RAFTQ_OUT_TERM_RESP, group by group ...
    assert sum(int((outs["type"] == TERM_RESP).sum()) for k, outs in seen if k == 2) == G_SCENARIO
    assert (c.s[2].term == 7).all() and (c.s[2].role == F).all() and (c.s[2].lead == 0).all()
    c.round()
    assert (c.s[0].role == F).all() and (c.s[0].term == 7).all()  # ... and the MsgAppResp made of it brought the leader down
    c.run(INFLATED_ROUNDS - 4)
    assert not c.converged()
    c.round()
    assert c.converged()
    assert (np.stack([s.term for s in c.s]).min(axis=0) >= 8).all()
    c.run(2 * 2 * c.et)
    assert c.converged()


# ---- the band cases: 64-bit terms and indices ----------------------------------------------------------------------------------------
BAND_CASES = [kw for kw in CASES if kw.get("band")]
B32 = [kw for kw in BAND_CASES if kw["band"] == "b32"]
B63 = [kw for kw in BAND_CASES if kw["band"] == "b63"]


def test_the_band_cases_are_the_issue_s():
    assert [(kw["band"], kw["n"], bool(kw.get("masks"))) for kw in BAND_CASES] == [(b, n, mk) for b in WG.BAND_NAMES for n, mk in ((3, False), (9, True))]
    assert CASES[-len(BAND_CASES):] == BAND_CASES and len({PV.case_id(kw) for kw in CASES}) == len(CASES)  # appended, ids of their own


@pytest.mark.parametrize("kw", BAND_CASES, ids=PV.case_id)
def test_band_cases_are_where_they_say(kw):
    _, _, m, want, after = PV.step_case(**kw)
    WG.check_in_band(kw["band"], want, kw)
    WG.guard_case(after[0], m)
    new = np.isin(m["type"], (PRE_VOTE, PRE_RESP))  # what test_every_rule_discriminates_on_the_gpu_inputs asks of every case
    assert new.sum() >= 40 and np.isin((PRE_CAMPAIGN, PV_RESP, TERM_RESP), want["type"]).all()


@pytest.mark.parametrize("kw", B32, ids=PV.case_id)
def test_a_32_bit_reading_of_the_b32_case_decides_differently(kw):
    """the reference over the same start and batch with every 64-bit word reduced mod 2^32: measured 46.9 % / 43.4 % of the 512
    records differ in (type, reject, flags, role), 55 / 54 of them of types 12..18; the floors are 10 % and 8"""
    start, voters, m, want, _ = PV.step_case(**kw)
    s32, m32 = WG.low32(start[0], m)
    want32 = PV.step_batch(s32, voters, start[1].copy(), start[2].copy(), m32)
    WG.check_narrow_reading(m, want, want32, WG.OWN_KINDS, kw)


@pytest.mark.parametrize("kw", B63, ids=PV.case_id)
def test_the_b63_case_compares_across_the_sign_bit(kw):
    """measured: 58.8 % / 58.2 % of the records have m.term : term or m.index : last_index on opposite sides of 2^63, 81 / 85 of them
    of types 12..18; the floors are 5 % and PLANT"""
    start, _, m, _, _ = PV.step_case(**kw)
    WG.check_straddles(start[0], m, WG.OWN_KINDS, PV.PLANT, kw)


@pytest.mark.parametrize("kw", B32 + B63, ids=PV.case_id)
def test_the_pre_elections_around_B_by_hand(kw):
    """the planted groups of term B - 1 (and the stale ones of term B): per record (type, reject, index, flags, term, role), and the
    term and role after, written out"""
    B, q = WG.BANDS[kw["band"]], kw["n"] // 2 + 1
    plants = {}
    start, _, m, want, after = PV.step_case(**kw, plants=plants)
    s0, s1 = start[0], after[0]

    def got(grp):
        at = np.flatnonzero(m["group"] == grp)
        return [tuple(int(want[i][k]) for k in ("type", "reject", "index", "flags", "term", "role")) for i in at], [int(t) for t in m["term"][at]]

    for name, groups in plants.items():
        assert len(groups) == PV.PLANT
        for grp in groups:
            recs, terms = got(grp)
            tail = int(s0.last_index[grp])
            assert int(s0.term[grp]) == (B if name == "stale" else B - 1)
            if name == "win":  # MsgHup, q - 2 grants that are not yet the quorum, the one that is: the campaign at term B
                assert terms == [0] + [B] * (q - 1)
                assert recs == [(PRE_CAMPAIGN, 0, tail, 0, B - 1, P)] + [(R.OutNone, 0, 0, 0, B - 1, P)] * (q - 2) + [(CAMPAIGN, 0, tail, HS, B, C)]
                end = (B, C)
            elif name == "bump":  # one rejection from two terms up: becomeFollower(B + 1, None)
                assert terms == [0, B + 1]
                assert recs == [(PRE_CAMPAIGN, 0, tail, 0, B - 1, P), (R.OutNone, 0, 0, HS | DOWN, B + 1, F)]
                end = (B + 1, F)
            elif name == "in_lease":
                assert terms == [B] and recs == [(R.OutNone, 0, 0, 0, B - 1, F)]
                end = (B - 1, F)
            elif name == "out_lease":  # granted with the message's term; nothing changes
                assert terms == [B] and recs == [(PV_RESP, 0, B, 0, B - 1, F)]
                end = (B - 1, F)
            elif name == "stale":  # the term before, from across the boundary: TERM_RESP twice, a rejection with the own term
                assert terms == [B - 1] * 3 and recs == [(TERM_RESP, 0, 0, 0, B, F)] * 2 + [(PV_RESP, 1, B, 0, B, F)]
                end = (B, F)
            else:  # led: the next term's is ignored in the lease, the own term's rejected with the own term
                assert terms == [B, B - 1] and recs == [(R.OutNone, 0, 0, 0, B - 1, L), (PV_RESP, 1, B - 1, 0, B - 1, L)]
                end = (B - 1, L)
            assert (int(s1.term[grp]), int(s1.role[grp])) == end, name
