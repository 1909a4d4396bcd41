"""tests/ref_lead_transfer.py held to a hand table and to the references below it (CPU): the Step reference gives what
include/raftq_step.h "Leadership transfer" says row by row, every input the GPU tests step tells each of the rules 3..9 from its
absence and holds every arm of rules 4 and 9 (the floors are asserted here), and three scenarios on three reference nodes show the
reason for the feature: a transfer to a follower that is behind completes, the same without rule 3 does not, and one to a node that
is cut off is aborted by the Tick."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import _widegen as WG
from tests import ref_check_quorum as Q
from tests import ref_lead_transfer as T
from tests import ref_pre_vote as PV
from tests import ref_raft_py as R
from tests import ref_step_props as P
from tests import ref_step_voters as V

F, C, L, PC = 0, 1, 2, 3  # roles
HS, CM, UP, DOWN, TN = R.FlagHardState, R.FlagCommitted, R.FlagUpdated, R.FlagSteppedDown, T.FlagTimeoutNow
XFER, TNOW = T.MsgTransferLeader, T.MsgTimeoutNow
NONE, TRANSFER, FORWARD, CAMPAIGN, LEADER, PROGRESS, PROPOSED, VOTE_RESP = (R.OutNone, T.OutTransfer, P.OutForward, R.OutCampaign, R.OutBecameLeader,
                                                                           R.OutProgress, P.OutProposed, R.OutVoteResp)
DISCRIMINATION_FLOOR = 4


def _group(n, me, role, term=5, lead=None, elapsed=0, vote=None, last_index=7, match=None):
    s = pyoracle.NodeState(1, n, me)
    s.role[0], s.term[0], s.elapsed[0], s.last_index[0], s.last_term[0] = role, term, elapsed, last_index, term
    s.lead[0] = (me + 1 if role == L else 0) if lead is None else lead
    s.vote[0] = (me + 1 if role != F else 0) if vote is None else vote
    s.first_idx[0] = 1 if role == L else 0
    s.match[me, 0] = last_index
    if role in (C, PC):
        s.votes[me, 0] = 1
    for p, v in (match or {}).items():
        s.match[p, 0] = v
    return s


def _msg(type, frm=0, term=0, index=0, log_term=0, reject=0, ents=0):
    m = np.zeros(1, pyoracle.STEP_MSG_DT)
    m["type"], m["from"], m["term"], m["index"], m["log_term"], m["reject"] = type, frm, term, index, log_term, reject
    if ents:
        m["_pad"][0] = (0, V.MSGF_ENTRIES)
        m["_resv"][0] = ents
    return m


# Every group: 3 peers unless said, term 5, the log ends at (7, 5), election_tick 10, activity word 0b010, lead_elapsed 4.  `frm` is a
# slot; vote, lead and the transferee are slot + 1.  A led group has committed nothing (first_idx 1): an ack that a quorum now holds commits.
# (what, pre_vote, n, self, role, kwargs of the group, voters | None, transferee before, message,
#  -> type, reject, index, flags, `to`, role, lead, term, transferee after, lead_elapsed after)
TABLE = [
    # rule 3
    ("a marked MsgVote of a higher term passes a leader's lease", True, 3, 0, L, {}, None, 0, _msg(R.MsgVote, 2, 6, 9, 6, reject=1), VOTE_RESP, 0, 0, HS | DOWN, 2, F, 0, 6, 0, 0),
    ("... and takes a pending transfer with it", False, 3, 0, L, {}, None, 3, _msg(R.MsgVote, 2, 6, 9, 6, reject=1), VOTE_RESP, 0, 0, HS | DOWN, 2, F, 0, 6, 0, 0),
    ("an unmarked one is ignored", True, 3, 0, L, {}, None, 3, _msg(R.MsgVote, 2, 6, 9, 6), NONE, 0, 0, 0, 2, L, 1, 5, 3, 4),
    ("a marked one passes a follower's lease", True, 3, 0, F, dict(lead=2, elapsed=2), None, 0, _msg(R.MsgVote, 2, 6, 9, 6, reject=1), VOTE_RESP, 0, 0, HS, 2, F, 0, 6, 0, 0),
    ("an unmarked one does not", False, 3, 0, F, dict(lead=2, elapsed=2), None, 0, _msg(R.MsgVote, 2, 6, 9, 6), NONE, 0, 0, 0, 2, F, 2, 5, 0, 4),
    ("a marked one with a log that is behind is rejected, the term moves", True, 3, 0, F, dict(lead=2, elapsed=2), None, 0, _msg(R.MsgVote, 2, 6, 3, 5, reject=1), VOTE_RESP, 1, 0, HS, 2, F, 0, 6, 0, 0),
    ("a marked MsgVote of the own term is no higher term: the role's rule", True, 3, 0, L, {}, None, 0, _msg(R.MsgVote, 2, 5, 9, 5, reject=1), VOTE_RESP, 1, 0, 0, 2, L, 1, 5, 0, 4),
    ("a MsgPreVote is never marked: in lease, ignored", True, 3, 0, L, {}, None, 0, _msg(PV.MsgPreVote, 2, 6, 9, 6, reject=1), NONE, 0, 0, 0, 2, L, 1, 5, 0, 4),
    # rule 4
    ("a transferee behind the tail: sendAppend is the caller's", True, 3, 0, L, dict(match={2: 4}), None, 0, _msg(XFER, 2), TRANSFER, 0, 4, 0, 2, L, 1, 5, 3, 0),
    ("at the tail: MsgTimeoutNow", False, 3, 0, L, dict(match={2: 7}), None, 0, _msg(XFER, 2), TRANSFER, 0, 7, TN, 2, L, 1, 5, 3, 0),
    ("the forwarded form, at the leader's term", True, 3, 0, L, dict(match={1: 7}), None, 0, _msg(XFER, 1, 5), TRANSFER, 0, 7, TN, 1, L, 1, 5, 2, 0),
    ("a Match beyond the tail is not the tail", True, 3, 0, L, dict(match={2: 9}), None, 0, _msg(XFER, 2), TRANSFER, 0, 9, 0, 2, L, 1, 5, 3, 0),
    ("the same transferee again: ignored, the clock runs on", True, 3, 0, L, dict(match={2: 7}), None, 3, _msg(XFER, 2), NONE, 0, 0, 0, 2, L, 1, 5, 3, 4),
    ("another one: aborted and replaced", True, 3, 0, L, dict(match={1: 2}), None, 3, _msg(XFER, 1), TRANSFER, 0, 2, 0, 1, L, 1, 5, 2, 0),
    ("to self: a pending transfer is cancelled", True, 3, 0, L, {}, None, 3, _msg(XFER, 0), NONE, 0, 0, 0, 0, L, 1, 5, 0, 4),
    ("to self with none pending: nothing", True, 3, 0, L, {}, None, 0, _msg(XFER, 0), NONE, 0, 0, 0, 0, L, 1, 5, 0, 4),
    ("masked: a transferee that is no voter is ignored", True, 3, 0, L, {}, 0b011, 2, _msg(XFER, 2), NONE, 0, 0, 0, 2, L, 1, 5, 2, 4),
    ("N = 9, self 0, slot 8: nibble 9", False, 9, 0, L, dict(match={8: 7}), None, 0, _msg(XFER, 8), TRANSFER, 0, 7, TN, 8, L, 1, 5, 9, 0),
    ("a stale forwarded one is ignored", True, 3, 0, L, {}, None, 0, _msg(XFER, 2, 4), NONE, 0, 0, 0, 2, L, 1, 5, 0, 4),
    ("one of a higher term deposes as any message does", True, 3, 0, L, {}, None, 3, _msg(XFER, 2, 6), FORWARD, 0, 0, HS | DOWN, 2, F, 3, 6, 0, 0),
    # rule 5
    ("the transferee's ack reaches the tail: MsgTimeoutNow", True, 3, 0, L, dict(match={2: 4}), None, 3, _msg(R.MsgAppResp, 2, 5, 7), PROGRESS, 0, 7, UP | TN | HS | CM, 2, L, 1, 5, 3, 4),
    ("... an ack beyond the tail is clamped to it", False, 3, 0, L, dict(match={2: 4}), None, 3, _msg(R.MsgAppResp, 2, 5, 11), PROGRESS, 0, 7, UP | TN | HS | CM, 2, L, 1, 5, 3, 4),
    ("it stops short of the tail: nothing yet", True, 3, 0, L, dict(match={2: 4}), None, 3, _msg(R.MsgAppResp, 2, 5, 6), PROGRESS, 0, 6, UP | HS | CM, 2, L, 1, 5, 3, 4),
    ("an ack that does not update sends nothing", True, 3, 0, L, dict(match={2: 7}), None, 3, _msg(R.MsgAppResp, 2, 5, 7), PROGRESS, 0, 7, 0, 2, L, 1, 5, 3, 4),
    ("another peer's ack at the tail is not the transferee's", True, 3, 0, L, dict(match={1: 4}), None, 3, _msg(R.MsgAppResp, 1, 5, 7), PROGRESS, 0, 7, UP | HS | CM, 1, L, 1, 5, 3, 4),
    ("a rejection is no ack", True, 3, 0, L, dict(match={2: 4}), None, 3, _msg(R.MsgAppResp, 2, 5, 7, reject=1), PROGRESS, 1, 4, 0, 2, L, 1, 5, 3, 4),
    # rule 6
    ("a proposal while a transfer is pending is dropped", True, 3, 0, L, {}, None, 3, _msg(P.MsgProp, 1, ents=2), NONE, 0, 0, 0, 1, L, 1, 5, 3, 4),
    ("with none pending it is taken", True, 3, 0, L, {}, None, 0, _msg(P.MsgProp, 1, ents=2), PROPOSED, 0, 8, 0, 1, L, 1, 5, 0, 4),
    # rule 7
    ("a MsgHeartbeat of a higher term: reset() clears the transferee", True, 3, 0, L, {}, None, 3, _msg(R.MsgHeartbeat, 1, 6), R.OutHeartbeatResp, 0, 0, HS | DOWN, 1, F, 2, 6, 0, 0),
    ("a check that passes clears it", True, 3, 0, L, {}, None, 3, _msg(Q.MsgCheckQuorum), NONE, 0, 0, 0, 0, L, 1, 5, 0, 4),
    ("a check that fails clears it on the way down", True, 5, 0, L, {}, None, 3, _msg(Q.MsgCheckQuorum), NONE, 0, 0, DOWN, 0, F, 0, 5, 0, 0),
    # rule 8
    ("a follower forwards it to its leader", True, 3, 0, F, dict(lead=2), None, 0, _msg(XFER, 2), FORWARD, 0, 0, 0, 1, F, 2, 5, 0, 4),
    ("... the forwarded form too", False, 3, 0, F, dict(lead=3), None, 0, _msg(XFER, 1, 5), FORWARD, 0, 0, 0, 2, F, 3, 5, 0, 4),
    ("without a leader it is dropped", True, 3, 0, F, {}, None, 0, _msg(XFER, 2), NONE, 0, 0, 0, 2, F, 0, 5, 0, 4),
    ("a candidate drops it", True, 3, 0, C, {}, None, 0, _msg(XFER, 2), NONE, 0, 0, 0, 2, C, 0, 5, 0, 4),
    ("a pre-candidate drops it", True, 3, 0, PC, {}, None, 0, _msg(XFER, 2), NONE, 0, 0, 0, 2, PC, 0, 5, 0, 4),
    # rule 9
    ("MsgTimeoutNow: the campaign, at once and marked, PreVote or not", True, 3, 0, F, dict(lead=2, elapsed=1), None, 0, _msg(TNOW, 1, 5), CAMPAIGN, 1, 7, HS, 1, C, 0, 6, 0, 0),
    ("... without PreVote", False, 3, 0, F, dict(lead=2, elapsed=1), None, 0, _msg(TNOW, 1, 5), CAMPAIGN, 1, 7, HS, 1, C, 0, 6, 0, 0),
    ("of a higher term: a follower of `from` first", True, 3, 0, F, dict(lead=2), None, 0, _msg(TNOW, 2, 7), CAMPAIGN, 1, 7, HS, 2, C, 0, 8, 0, 0),
    ("of a lower term: ignored, and no RAFTQ_OUT_TERM_RESP", True, 3, 0, F, dict(lead=2), None, 0, _msg(TNOW, 1, 4), NONE, 0, 0, 0, 1, F, 2, 5, 0, 4),
    ("masked, self is no voter: not promotable", True, 3, 0, F, dict(lead=2), 0b110, 0, _msg(TNOW, 1, 5), NONE, 0, 0, 0, 1, F, 2, 5, 0, 4),
    ("masked, self is the one voter: leader at once, unmarked", True, 3, 0, F, dict(lead=2), 0b001, 0, _msg(TNOW, 1, 5), LEADER, 0, 8, HS | CM, 1, L, 1, 6, 0, 0),
    ("a leader ignores it", True, 3, 0, L, {}, None, 3, _msg(TNOW, 1, 5), NONE, 0, 0, 0, 1, L, 1, 5, 3, 4),
    ("a candidate ignores it", True, 3, 0, C, {}, None, 0, _msg(TNOW, 1, 5), NONE, 0, 0, 0, 1, C, 0, 5, 0, 4),
    ("a pre-candidate ignores it", True, 3, 0, PC, {}, None, 0, _msg(TNOW, 1, 5), NONE, 0, 0, 0, 1, PC, 0, 5, 0, 4),
]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_step_reference_against_the_hand_table(row):
    what, pv, n, me, role, kw, voters, tr0, m, typ, reject, index, flags, to, role2, lead2, term2, tr2, le2 = row
    s = _group(n, me, role, **kw)
    vt = None if voters is None else np.array([voters], np.uint16)
    ac, le, tr = np.array([0b010], np.uint16), np.array([4], np.uint32), np.array([tr0], np.uint8)
    out, tr_back = T.step_batch(s, vt, ac, le, tr, m, pv)
    o = out[0]
    got = tuple(int(o[k]) for k in ("type", "reject", "index", "flags", "to", "role", "lead", "term"))
    assert got == (typ, reject, index, flags, to, role2, lead2, term2), what
    assert (int(s.role[0]), int(s.lead[0]), int(s.term[0])) == (role2, lead2, term2), what
    assert tr_back is tr and (int(tr[0]), int(le[0])) == (tr2, le2), what
    if typ == NONE and flags == 0 and int(m["type"][0]) != Q.MsgCheckQuorum:  # every ignored case changes nothing but, at most, the transferee
        assert int(ac[0]) == 0b010 and int(s.match[me, 0]) == 7 and int(s.last_index[0]) == 7 and int(s.committed[0]) == 0, what


def test_without_its_rules_the_reference_is_pre_vote_s():
    """the mixin overrides nothing it does not name: with every rule left out, PreVote's own inputs -- no record of the two kinds, no
    transferee -- are stepped as tests/ref_pre_vote.py steps them"""
    for kw in (PV.case_list()[2], PV.case_list()[5]):
        start, voters, m, want, after = PV.step_case(**kw)
        st = (V.copy_state(start[0]), start[1].copy(), start[2].copy(), np.zeros(start[0].G, np.uint8))
        out, tr = T.step_batch(st[0], voters, st[1], st[2], st[3], np.array(m), True, leave_out=T.RULES)
        assert out.tobytes() == np.array(want).tobytes() and not Q.state_differs(st[:3], after) and (tr == 0).all()
        st = (V.copy_state(start[0]), start[1].copy(), start[2].copy(), np.zeros(start[0].G, np.uint8))
        unmarked = np.array(m)
        unmarked["reject"][unmarked["type"] == R.MsgVote] = 0  # (with its rules on, only a mark tells the two apart)
        want_u = PV.step_batch(V.copy_state(start[0]), voters, start[1].copy(), start[2].copy(), unmarked)
        out, _ = T.step_batch(st[0], voters, st[1], st[2], st[3], unmarked, True)
        assert out.tobytes() == want_u.tobytes()


def test_leave_out_takes_names():
    assert T.rules(("lease", 9, "forward")) == {3, 8, 9} and sorted(T.RULE_NAMES) == list(T.RULES)


CASES = T.case_list()


@pytest.mark.parametrize("kw", CASES, ids=T.case_id)
def test_every_gpu_input_discriminates_and_holds_every_arm(kw):
    start, voters, m, want, after = T.step_case(**kw)
    for rule in T.case_rules(kw):
        n = len(T.changed_records(start, voters, m, want, after, rule, kw.get("pre_vote", True)))
        assert n >= DISCRIMINATION_FLOOR, (T.RULE_NAMES[rule], n)
    for arm, n in T.arms(start, voters, m, want).items():
        assert n >= T.ARM_FLOOR, (arm, n)
    # the states hold what the issue asks for
    s0, tr0 = start[0], start[3]
    led = s0.role == 2
    assert (tr0[led] != 0).sum() >= 8 and (tr0[~led] == 0).all()
    t = np.where(tr0 != 0, tr0, 1).astype(np.int64) - 1
    mt = s0.match[t, np.arange(s0.G)]
    pend = tr0 != 0
    assert (mt[pend] == s0.last_index[pend]).any() and (mt[pend] < s0.last_index[pend]).any()
    assert (s0.match[:, led] > s0.last_index[led][None, :]).any()  # a Match beyond the tail
    votes = (m["type"] == R.MsgVote) & (m["term"] > s0.term[m["group"].astype(np.int64)])
    for mark in (0, 1):
        took = votes & (m["reject"] == mark)
        assert (took & (want["type"] == R.OutNone)).sum() >= (4 if mark == 0 else 0) and (took & (want["type"] == R.OutVoteResp)).sum() >= 4, mark
    assert ((start[2] == 65535) & pend).sum() >= 4


def test_the_tick_composes_check_quorum_s():
    """over words without a transferee ref_lead_transfer.tick IS ref_check_quorum.tick_array; with one, a check that falls due and
    passes clears it and nothing else touches it"""
    g, n, me, et = 600, 5, 4, 6
    role, elapsed, active, lead_elapsed, transferee, voters = T.tick_input(g, n, me, et, 77, masks=True)
    el, ac, le, tr = elapsed, active, lead_elapsed, transferee
    cleared = 0
    for t in range(2 * et):
        want = Q.tick_array(pyoracle, role, el, ac, le, voters, me, n, et, 2, 99, t)
        got = T.tick(pyoracle, role, el, ac, le, tr, voters, me, n, et, 2, 99, t)
        for a, b in zip(want[:4], got[:4]):
            assert np.array_equal(a, b), t
        assert want[4:] == got[5:]
        passed = (role == 2) & (le + 1 >= et) & (got[1] != 3)
        assert np.array_equal(got[4], np.where(passed, 0, tr)), t
        cleared += int((passed & (tr != 0)).sum())
        el, ac, le, tr = got[0], got[2], got[3], got[4]
    assert cleared >= 50


# ---- three nodes -------------------------------------------------------------------------------------------------------------------
G_SCENARIO = 12
BEHIND = 2
CLUSTER_KW = {"completing": dict(behind=BEHIND), "aborted": dict(behind=BEHIND)}


def _flat_log(c, since=0):
    return [(k, b[i], o[i]) for k, b, o in c.log[since:] for i in range(len(b))]


def completing(c, rounds=4):
    """node 0 leads, node 2 is BEHIND entries back.  One MsgTransferLeader per group on the leader -> MsgApp, ack,
    RAFTQ_OUTF_TIMEOUT_NOW, marked votes granted inside the lease, the old leader a follower: the term rises by exactly 1 and no
    pre-election is run.  -> the flat log of the transfer's rounds"""
    g = c.g
    c.run(2)
    assert (c.s[0].role == 2).all() and (c.s[1].elapsed < c.et).all()
    since = len(c.log)
    c.inject(0, T.transfer_msgs(g, 2))
    c.run(rounds)
    log = _flat_log(c, since)
    kinds = lambda k, f: [(int(b["type"]), int(o["type"])) for kk, b, o in log if kk == k and f(b, o)]  # noqa: E731
    xfer = [o for k, b, o in log if k == 0 and int(b["type"]) == T.MsgTransferLeader]
    assert len(xfer) == g and all(int(o["type"]) == T.OutTransfer and int(o["flags"]) == 0 and int(o["index"]) == 5 - BEHIND for o in xfer)
    assert len(kinds(2, lambda b, o: int(b["type"]) == R.MsgApp and int(o["type"]) == R.OutAppended and int(o["index"]) == 5)) == g
    acks = [o for k, b, o in log if k == 0 and int(b["type"]) == R.MsgAppResp and int(o["flags"]) & T.FlagTimeoutNow]
    assert len(acks) == g
    camp = [o for k, b, o in log if k == 2 and int(b["type"]) == T.MsgTimeoutNow]
    assert len(camp) == g and all(int(o["type"]) == R.OutCampaign and int(o["reject"]) == 1 and int(o["term"]) == 2 for o in camp)
    grants = [(k, o) for k, b, o in log if k != 2 and int(b["type"]) == R.MsgVote and int(b["reject"]) == 1]
    assert len(grants) == 2 * g and all(int(o["type"]) == R.OutVoteResp and int(o["reject"]) == 0 for _, o in grants)
    assert all(int(b["type"]) != PV.MsgPreVote and int(o["type"]) != PV.OutPreCampaign for _, b, o in log)  # no pre-election
    assert (c.s[2].role == 2).all() and (c.s[0].role == 0).all() and (c.s[1].role == 0).all()
    assert all((s.term == 2).all() for s in c.s) and all((t == 0).all() for t in c.transferee)
    c.run(2)
    assert c.converged() and (c.leaders()[1] == 2).all() and all((s.term == 2).all() for s in c.s)
    return log


def not_completing(c, rounds=4):
    """the same with rule 3 left out on every node: the marked votes are ignored under the lease like any other"""
    g = c.g
    c.run(2)
    since = len(c.log)
    c.inject(0, T.transfer_msgs(g, 2))
    c.run(rounds)
    log = _flat_log(c, since)
    votes = [o for k, b, o in log if k != 2 and int(b["type"]) == R.MsgVote and int(b["term"]) == 2]
    assert len(votes) == 2 * g and all(int(o["type"]) == R.OutNone and int(o["term"]) == 1 for o in votes)
    assert (c.s[2].role == 1).all() and (c.s[2].term == 2).all() and not (c.s[2].role == 2).any()
    assert (c.s[1].term == 1).all() and (c.s[1].vote != 3).all() and (c.s[0].vote != 3).all()


def aborted(c):
    """node 2 is cut off.  The transfer to it stays pending -- a MsgProp is dropped meanwhile --; election_tick Ticks after it was
    taken the leader's check falls due, passes on node 1's heartbeat responses and clears the transferee: a MsgProp is accepted again"""
    g = c.g
    c.run(2)
    c.cut = {2}
    c.inject(0, T.transfer_msgs(g, 2))
    c.run(1)  # (the Tick of this round comes first: lead_elapsed is 0 behind it)
    assert (c.transferee[0] == 3).all() and (c.lead_elapsed[0] == 0).all() and (c.s[0].role == 2).all()
    c.inject(0, T.prop_msgs(g, 1))
    c.run(1)
    k, b, o = c.log[-1] if c.log[-1][0] == 0 else next(x for x in reversed(c.log) if x[0] == 0)
    prop = b["type"] == P.MsgProp
    assert prop.sum() == g and (o["type"][prop] == R.OutNone).all() and (c.s[0].last_index == 5).all()
    c.run(c.et - 2)
    assert (c.transferee[0] == 3).all()  # election_tick - 1 Ticks: still pending
    c.run(1)
    assert (c.transferee[0] == 0).all() and (c.s[0].role == 2).all() and (c.s[0].term == 1).all()
    c.inject(0, T.prop_msgs(g, 1))
    c.run(1)
    k, b, o = next(x for x in reversed(c.log) if x[0] == 0)
    prop = b["type"] == P.MsgProp
    assert prop.sum() == g and (o["type"][prop] == P.OutProposed).all() and (c.s[0].last_index == 6).all()


@pytest.mark.parametrize("pre_vote", [False, True])
def test_a_transfer_to_a_follower_that_is_behind_completes(pre_vote):
    completing(T.Cluster(G_SCENARIO, pre_vote, **CLUSTER_KW["completing"]))


@pytest.mark.parametrize("pre_vote", [False, True])
def test_without_rule_3_it_does_not_complete(pre_vote):
    not_completing(T.Cluster(G_SCENARIO, pre_vote, behind=BEHIND, leave_out={"lease"}))


@pytest.mark.parametrize("pre_vote", [False, True])
def test_a_transfer_to_a_cut_off_node_is_aborted(pre_vote):
    aborted(T.Cluster(G_SCENARIO, pre_vote, **CLUSTER_KW["aborted"]))


# ---- the band cases: 64-bit terms and indices ----------------------------------------------------------------------------------------
BAND_CASES = [kw for kw in CASES if kw.get("band")]
B32 = [kw for kw in BAND_CASES if kw["band"] == "b32"]
B63 = [kw for kw in BAND_CASES if kw["band"] == "b63"]


def test_the_band_cases_are_the_issue_s():
    assert [(kw["band"], kw["n"], bool(kw.get("masks"))) for kw in BAND_CASES] == [(b, n, mk) for b in WG.BAND_NAMES for n, mk in ((3, False), (9, True))]
    assert CASES[-len(BAND_CASES):] == BAND_CASES and len({T.case_id(kw) for kw in CASES}) == len(CASES)  # appended, ids of their own
    assert {(bool(kw.get("masks")), kw["pre_vote"]) for kw in BAND_CASES} == {(a, b) for a in (False, True) for b in (False, True)}


@pytest.mark.parametrize("kw", BAND_CASES, ids=T.case_id)
def test_band_cases_are_where_they_say(kw):
    _, _, m, want, after = T.step_case(**kw)
    WG.check_in_band(kw["band"], want, kw)
    WG.guard_case(after[0], m)


@pytest.mark.parametrize("kw", B32, ids=T.case_id)
def test_a_32_bit_reading_of_the_b32_case_decides_differently(kw):
    """the reference over the same start and batch with every 64-bit word reduced mod 2^32: measured 29.9 % / 31.2 % of the 512
    records differ in (type, reject, flags, role), 14 / 28 of them of types 12..18; the floors are 10 % and 8"""
    start, voters, m, want, _ = T.step_case(**kw)
    s32, m32 = WG.low32(start[0], m)
    want32, _ = T.step_batch(s32, voters, start[1].copy(), start[2].copy(), start[3].copy(), m32, kw["pre_vote"])
    WG.check_narrow_reading(m, want, want32, WG.OWN_KINDS, kw)


@pytest.mark.parametrize("kw", B63, ids=T.case_id)
def test_the_b63_case_compares_across_the_sign_bit(kw):
    """measured: 31.8 % / 29.7 % of the records have m.term : term or m.index : last_index on opposite sides of 2^63, 11 / 13 of them
    of types 12..18 (the eight MsgTimeoutNow of term B to followers of term B - 1 among them); the floors are 5 % and PLANT"""
    start, _, m, _, _ = T.step_case(**kw)
    WG.check_straddles(start[0], m, WG.OWN_KINDS, T.PLANT, kw)


@pytest.mark.parametrize("kw", BAND_CASES, ids=T.case_id)
def test_the_transfers_at_the_tail_by_hand(kw):
    """the band-only plants: per record (type, reject, index, flags, role), the transferee, the Match and the term after, written out"""
    band = kw["band"]
    B = WG.BANDS[band]
    plants = {}
    start, _, m, want, after = T.step_case(**kw, plants=plants)
    s0, s1, last = start[0], after[0], plants["last"]

    def got(grp):
        at = np.flatnonzero(m["group"] == grp)
        return [tuple(int(want[i][k]) for k in ("type", "reject", "index", "flags", "role")) for i in at], m[at]

    assert (len(plants["at_tail"]), len(plants["far"]), len(plants["by_ack"]), len(plants["tn_up"])) == (1, 2, 2, T.PLANT)
    for name in ("at_tail", "far", "by_ack"):
        for grp in plants[name]:
            recs, sent = got(grp)
            tail = int(s0.last_index[grp])
            assert (tail == B if B else tail >= WG.TOP_LO) and int(start[3][grp]) == 0 and int(s1.last_index[grp]) == tail
            assert int(sent["type"][0]) == XFER and int(sent["from"][0]) == last
            if name == "at_tail":  # Match == tail: MsgTimeoutNow at once
                assert int(s0.match[last, grp]) == tail and recs == [(TRANSFER, 0, tail, TN, L)]
            elif name == "far":  # 2^32 away, the low words equal: no flag
                away = int(s0.match[last, grp])
                assert abs(away - tail) == 2**32 and away & 0xFFFFFFFF == tail & 0xFFFFFFFF and recs == [(TRANSFER, 0, away, 0, L)]
            else:  # the acknowledgement that moves the Match from tail - 1 to the tail carries the flag
                assert int(s0.match[last, grp]) == tail - 1 and int(sent["type"][1]) == R.MsgAppResp and int(sent["index"][1]) == tail
                assert recs[0] == (TRANSFER, 0, tail - 1, 0, L) and len(recs) == 2
                assert recs[1][:3] == (PROGRESS, 0, tail) and recs[1][3] & (UP | TN) == UP | TN and recs[1][4] == L
                assert int(s1.match[last, grp]) == tail
            assert int(after[3][grp]) == last + 1 and int(after[2][grp]) == 0  # pending, the transfer's clock started
    if B:
        for grp in plants["tn_up"]:  # MsgTimeoutNow of term B to a follower of term B - 1: a follower at B first, then the campaign at B + 1
            recs, sent = got(grp)
            tail = int(s0.last_index[grp])
            assert int(s0.term[grp]) == B - 1 and int(sent["type"][0]) == TNOW and int(sent["term"][0]) == B
            assert recs == [(CAMPAIGN, 1, tail, HS, C)] and (int(s1.term[grp]), int(s1.role[grp])) == (B + 1, C)
