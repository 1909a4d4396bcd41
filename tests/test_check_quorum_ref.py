"""tests/ref_check_quorum.py held to itself and to a hand table (CPU): the two statements of the Tick agree, the Step reference
gives what include/raftq_step.h "CheckQuorum" says row by row, and every input the GPU tests step tells the feature -- each of its
four rules -- from its absence."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import _widegen as WG
from tests import ref_check_quorum as Q
from tests import ref_raft_py as R
from tests import ref_step_voters as V

CQ = Q.MsgCheckQuorum
F, C, L = 0, 1, 2  # roles
DOWN = R.FlagSteppedDown


def _group(n, me, role, term=5, lead=None, elapsed=0, vote=None, last_index=7):
    s = pyoracle.NodeState(1, n, me)
    s.role[0], s.term[0], s.elapsed[0], s.last_index[0], s.last_term[0] = role, term, elapsed, last_index, term
    s.lead[0] = (me + 1 if role == L else 0) if lead is None else lead
    s.vote[0] = (me + 1 if role != F else 0) if vote is None else vote
    s.first_idx[0] = 1 if role == L else 0
    s.match[me, 0] = last_index
    if role == C:
        s.votes[me, 0] = 1
    return s


def _msg(type, frm=0, term=0, index=0, log_term=0, reject=0):
    m = np.zeros(1, pyoracle.STEP_MSG_DT)
    m["type"], m["from"], m["term"], m["index"], m["log_term"], m["reject"] = type, frm, term, index, log_term, reject
    return m


# (what, n, self, role, kwargs of the group, voters | None, active before, message, -> type, reject, flags, role, lead, term, active after)
TABLE = [
    ("an ack sets the bit", 3, 0, L, {}, None, 0b000, _msg(R.MsgAppResp, 1, 5, 7), R.OutProgress, 0, R.FlagUpdated | R.FlagHardState | R.FlagCommitted, L, 1, 5, 0b010),
    ("a heartbeat response sets the bit", 3, 0, L, {}, None, 0b000, _msg(R.MsgHeartbeatResp, 2, 5), R.OutProgress, 0, 0, L, 1, 5, 0b100),
    ("a rejected ack sets it", 3, 0, L, {}, None, 0b000, _msg(R.MsgAppResp, 2, 5, 7, reject=1), R.OutProgress, 1, 0, L, 1, 5, 0b100),
    ("a passing check clears the bits", 3, 0, L, {}, None, 0b110, _msg(CQ), R.OutNone, 0, 0, L, 1, 5, 0),
    ("one peer beside self is a quorum of three", 3, 0, L, {}, None, 0b100, _msg(CQ), R.OutNone, 0, 0, L, 1, 5, 0),
    ("a failing check steps down: STEPPED_DOWN alone", 3, 0, L, {}, None, 0b000, _msg(CQ), R.OutNone, 0, DOWN, F, 0, 5, 0),
    ("two of five beside self are not needed: one is too few", 5, 4, L, {}, None, 0b00001, _msg(CQ), R.OutNone, 0, DOWN, F, 0, 5, 0),
    ("self's own bit does not count twice", 5, 4, L, {}, None, 0b10001, _msg(CQ), R.OutNone, 0, DOWN, F, 0, 5, 0),
    ("a check on a follower is ignored", 3, 0, F, dict(lead=2), None, 0b110, _msg(CQ), R.OutNone, 0, 0, F, 2, 5, 0b110),
    ("a check on a candidate is ignored", 3, 0, C, {}, None, 0b010, _msg(CQ), R.OutNone, 0, 0, C, 0, 5, 0b010),
    ("MsgVote at a higher term to a leader is ignored", 3, 0, L, {}, None, 0b010, _msg(R.MsgVote, 2, 6, 9, 6), R.OutNone, 0, 0, L, 1, 5, 0b010),
    ("... to a follower with a leader, in lease", 3, 0, F, dict(lead=2, elapsed=9), None, 0, _msg(R.MsgVote, 2, 6, 9, 6), R.OutNone, 0, 0, F, 2, 5, 0),
    ("... out of lease: answered as always", 3, 0, F, dict(lead=2, elapsed=10), None, 0, _msg(R.MsgVote, 2, 6, 9, 6), R.OutVoteResp, 0, R.FlagHardState, F, 0, 6, 0),
    ("... to a follower without a leader: answered", 3, 0, F, dict(lead=0, elapsed=0), None, 0, _msg(R.MsgVote, 2, 6, 9, 6), R.OutVoteResp, 0, R.FlagHardState, F, 0, 6, 0),
    ("... to a candidate: answered as always", 3, 0, C, {}, None, 0b001, _msg(R.MsgVote, 2, 6, 9, 6), R.OutVoteResp, 0, R.FlagHardState | DOWN, F, 0, 6, 0),
    ("MsgVote at the SAME term to a leader: rejected as always", 3, 0, L, {}, None, 0, _msg(R.MsgVote, 2, 5, 9, 6), R.OutVoteResp, 1, 0, L, 1, 5, 0),
    ("MsgApp at a higher term in lease is still obeyed", 3, 0, F, dict(lead=2, elapsed=0), None, 0, _msg(R.MsgApp, 1, 6, 7, 5), R.OutAppend, 0, R.FlagHardState, F, 2, 6, 0),
    ("MsgHeartbeat at a higher term deposes a leader and clears the bits", 3, 0, L, {}, None, 0b110, _msg(R.MsgHeartbeat, 1, 6), R.OutHeartbeatResp, 0, R.FlagHardState | DOWN, F, 2, 6, 0),
    ("masked: a non-voter's bit is stored ...", 3, 0, L, {}, 0b101, 0b000, _msg(R.MsgHeartbeatResp, 1, 5), R.OutProgress, 0, 0, L, 1, 5, 0b010),
    ("... and does not count", 3, 0, L, {}, 0b101, 0b010, _msg(CQ), R.OutNone, 0, DOWN, F, 0, 5, 0),
    ("masked: the voter's bit does", 3, 0, L, {}, 0b101, 0b100, _msg(CQ), R.OutNone, 0, 0, L, 1, 5, 0),
    ("masked: self does not vote and is not counted", 3, 0, L, {}, 0b110, 0b010, _msg(CQ), R.OutNone, 0, DOWN, F, 0, 5, 0),
    ("masked: an empty mask steps down", 3, 0, L, {}, 0b000, 0b111, _msg(CQ), R.OutNone, 0, DOWN, F, 0, 5, 0),
    ("N = 1: a lone leader always passes", 1, 0, L, {}, None, 0, _msg(CQ), R.OutNone, 0, 0, L, 1, 5, 0),
    ("N = 1, masked, its one voter", 1, 0, L, {}, 0b1, 0, _msg(CQ), R.OutNone, 0, 0, L, 1, 5, 0),
]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_step_reference_against_the_hand_table(row):
    what, n, me, role, kw, voters, active, m, typ, reject, flags, role2, lead2, term2, active2 = row
    s = _group(n, me, role, **kw)
    vt = None if voters is None else np.array([voters], np.uint16)
    ac, le = np.array([active], np.uint16), np.array([4], np.uint32)
    o = Q.step_batch(s, vt, ac, le, m)[0]
    assert (int(o["type"]), int(o["reject"]), int(o["flags"]), int(o["role"]), int(o["lead"]), int(o["term"])) == (typ, reject, flags, role2, lead2, term2), what
    assert int(ac[0]) == active2, what
    assert int(le[0]) == (4 if int(o["role"]) == role and int(o["term"]) == 5 else 0), what  # reset() alone clears it: a new role or term
    if flags & DOWN and typ == R.OutNone:  # becomeFollower(term, None): Term and Vote as they were
        assert int(o["vote"]) == me + 1 and int(s.elapsed[0]) == 0


def test_without_its_four_rules_the_reference_is_the_oracle():
    """the mixin overrides the four rules and nothing else: with all of them left out it steps a batch as the C oracle does"""
    from tests import _stepgen
    rng = np.random.default_rng(9400)
    s = _stepgen.random_state(rng, 64, 3, 1)
    m = _stepgen.random_batch(rng, s, 400)
    a = V.copy_state(s)
    want = a.step_batch(m)
    ac, le = np.full(64, 0b101, np.uint16), np.full(64, 3, np.uint32)
    got = Q.step_batch(s, None, ac, le, m, leave_out={1, 2, 3, 4})
    assert got.tobytes() == want.tobytes() and not Q.state_differs((s, ac, le), (a, np.full(64, 0b101, np.uint16), np.full(64, 3, np.uint32)))


@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("n,me", [(1, 0), (3, 0), (3, 2), (5, 4), (9, 8)])
@pytest.mark.parametrize("et,ht", [(1, 1), (3, 1), (3, 2), (10, 2)])
def test_the_two_tick_statements_agree(n, me, et, ht, masks):
    g = 300
    role, el, ac, le, voters = Q.tick_input(g, n, me, et, seed=9410 + 10 * n + et + ht, masks=masks)
    seen = set()
    for t in range(2 * et + 1):
        a = Q.tick_array(pyoracle, role, el, ac, le, voters, me, n, et, ht, 0x77, t)
        b = Q.tick_scalar(pyoracle, role, el, ac, le, voters, me, n, et, ht, 0x77, t)
        for x, y, k in zip(a, b, ("elapsed", "action", "active", "lead_elapsed", "n_hup", "n_beat")):
            assert np.array_equal(x, y), (k, t)
        el, act, ac, le = a[:4]
        seen |= set(np.unique(act).tolist())
        lost = act == 3
        assert not lost.any() or (np.all(role[lost] == 2) and np.all(le[lost] == 0))
    assert seen >= ({0, 2} if n == 1 and not masks else {0, 1, 2, 3}), seen  # (a lone leader over every slot never fails)


CASES = Q.case_list()


@pytest.mark.parametrize("kw", CASES, ids=[str(sorted(k.items())) for k in CASES])
def test_every_gpu_input_discriminates(kw):
    """the band cases too, held to the same floors"""
    start, voters, m, want, after = Q.step_case(**kw)
    got = Q.outcomes(start, voters, m, want)
    can_fail = kw["n"] > 1 or kw.get("masks")  # N = 1 over every slot: the lone leader always passes (the rule itself)
    for k in ("passing checks", "checks on a non-leader", "lease-ignored votes", "acks that set a bit"):
        assert got[k] >= 1, (k, got)
    assert got["failing checks"] >= (1 if can_fail else 0), got
    for rule in (1, 2, 3, 4):
        st = (V.copy_state(start[0]), start[1].copy(), start[2].copy())
        without = Q.step_batch(st[0], voters, st[1], st[2], m, leave_out={rule})
        assert without.tobytes() != want.tobytes() or Q.state_differs(st, after), ("rule %d makes no difference on this input" % rule, kw)


# ---- the band cases: 64-bit terms and indices ----------------------------------------------------------------------------------------
BAND_CASES = [kw for kw in CASES if kw.get("band")]
B32 = [kw for kw in BAND_CASES if kw["band"] == "b32"]
B63 = [kw for kw in BAND_CASES if kw["band"] == "b63"]


def test_the_band_cases_are_the_issue_s():
    assert [(kw["band"], kw["n"], bool(kw.get("masks"))) for kw in BAND_CASES] == [(b, n, mk) for b in WG.BAND_NAMES for n, mk in ((3, False), (9, True))]
    assert CASES[-len(BAND_CASES):] == BAND_CASES and len({Q.case_id(kw) for kw in CASES}) == len(CASES)  # appended, ids of their own


@pytest.mark.parametrize("kw", BAND_CASES, ids=Q.case_id)
def test_band_cases_are_where_they_say(kw):
    _, _, m, want, after = Q.step_case(**kw)
    WG.check_in_band(kw["band"], want, kw)
    WG.guard_case(after[0], m)


@pytest.mark.parametrize("kw", B32, ids=Q.case_id)
def test_a_32_bit_reading_of_the_b32_case_decides_differently(kw):
    """the reference over the same start and batch with every 64-bit word reduced mod 2^32: measured 44.3 % / 43.2 % of the 512
    records differ in (type, reject, flags, role), 48 / 50 of them MsgCheckQuorum or MsgVote records (7 / 12 MsgCheckQuorum alone: a
    check carries no 64-bit word of its own and differs only where the group's role already did); the floors are 10 % and 8."""
    start, voters, m, want, _ = Q.step_case(**kw)
    s32, m32 = WG.low32(start[0], m)
    want32 = Q.step_batch(s32, voters, start[1].copy(), start[2].copy(), m32)
    WG.check_narrow_reading(m, want, want32, Q.OWN_KINDS, kw)


@pytest.mark.parametrize("kw", B63, ids=Q.case_id)
def test_the_b63_case_compares_across_the_sign_bit(kw):
    """measured: 52.1 % / 53.3 % of the records have m.term : term or m.index : last_index on opposite sides of 2^63, 55 / 49 of them
    MsgVote records (a MsgCheckQuorum carries no term); the floors are 5 % and PLANT"""
    start, _, m, _, _ = Q.step_case(**kw)
    WG.check_straddles(start[0], m, Q.OWN_KINDS, Q.PLANT, kw)


@pytest.mark.parametrize("kw", B32 + B63, ids=Q.case_id)
def test_the_vote_of_term_B_by_hand(kw):
    """a MsgVote of term B to a leader and to followers of term B - 1: inside the lease it is ignored and the term stays B - 1, past
    the lease it is granted and the term becomes B"""
    B = WG.BANDS[kw["band"]]
    plants = {}
    start, _, m, want, after = Q.step_case(**kw, plants=plants)
    s0, s1 = start[0], after[0]
    for name, groups in plants.items():
        assert len(groups) == Q.PLANT
        for grp in groups:
            at = np.flatnonzero(m["group"] == grp)
            assert len(at) == 1 and int(m["type"][at[0]]) == R.MsgVote and int(m["term"][at[0]]) == B and int(s0.term[grp]) == B - 1
            o = want[at[0]]
            got = tuple(int(o[k]) for k in ("type", "reject", "index", "flags", "term", "role"))
            if name == "out_lease":
                assert got == (R.OutVoteResp, 0, 0, R.FlagHardState, B, F), (name, got)
                assert (int(s1.term[grp]), int(s1.vote[grp]), int(s1.lead[grp])) == (B, int(m["from"][at[0]]) + 1, 0)
            else:
                assert got == (R.OutNone, 0, 0, 0, B - 1, L if name == "led" else F), (name, got)
                assert (int(s1.term[grp]), int(s1.vote[grp]), int(s1.lead[grp])) == (B - 1, int(s0.vote[grp]), int(s0.lead[grp]))
