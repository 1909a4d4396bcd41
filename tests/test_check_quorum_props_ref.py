"""tests/ref_check_quorum_props.py held to the two references it composes and to itself (CPU): with the four CheckQuorum rules left
out it is ref_step_props' Step, without a MsgProp it is ref_check_quorum's; every input the GPU tests hand to the device tells each
rule from its absence and the switch from its absence, and shows what its test is about (the floors) -- so the GPU tests cannot pass
on inputs that show nothing."""
import functools

import numpy as np
import pytest

from tests import ref_check_quorum as Q
from tests import ref_check_quorum_props as CP
from tests import ref_raft_py as R
from tests import ref_respond_props as RP
from tests import ref_step_props as P
from tests import ref_step_voters as V

ALL = frozenset({1, 2, 3, 4})
RESPOND = CP.respond_case_list()
PROPS = CP.props_case_list()


@functools.lru_cache(maxsize=None)
def _respond(name):
    start, voters, s, off, at, plan = CP.respond_case(**RESPOND[name])
    st = CP.copy_triple(start)
    return start, voters, s, off, at, plan, CP.want(st[0], st[1], st[2], s, off, at, voters, trace=True), st


@functools.lru_cache(maxsize=None)
def _lock(name):
    return CP.lockstep(**CP.LOCK_SHAPES[name])


def _differs(start, voters, m, want, after, rule, **kw):
    st = CP.copy_triple(start)
    without = CP.step_batch(st[0], voters, st[1], st[2], m, leave_out={rule}, **kw)
    return without.tobytes() != want.tobytes() or Q.state_differs(st, after)


# ---- the composition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RESPOND))
def test_without_the_four_rules_it_is_step_props_on_the_frames_inputs(name):
    start, voters, s, off, at, plan, w, _ = _respond(name)
    rec = w["rec"]
    assert not (rec["type"] == CP.MsgCheckQuorum).any() and (rec["type"] == P.MsgProp).sum() >= 8
    a, b = CP.copy_triple(start), V.copy_state(start[0])
    got = CP.step_batch(a[0], voters, a[1], a[2], rec, leave_out=ALL)
    assert got.tobytes() == P.step_batch(b, voters, rec).tobytes()
    assert not Q.state_differs(a, (b, start[1], start[2]))  # and the activity words were not touched


@pytest.mark.parametrize("k", range(0, len(P.case_list()[0]), 3))
def test_without_the_four_rules_it_is_step_props_on_caller_records(k):
    start, voters, m, want, after = P.case(**P.case_list()[0][k])
    ac, le = np.full(start.G, 0b1, np.uint16), np.full(start.G, 2, np.uint32)
    a = V.copy_state(start)
    assert CP.step_batch(a, voters, ac, le, m, leave_out=ALL).tobytes() == want.tobytes()
    assert not Q.state_differs((a, ac, le), (after, np.full(start.G, 0b1, np.uint16), np.full(start.G, 2, np.uint32)))


@pytest.mark.parametrize("kw", Q.case_list(), ids=[str(sorted(k.items())) for k in Q.case_list()])
def test_without_a_proposal_it_is_the_check_quorum_reference(kw):
    start, voters, m, want, after = Q.step_case(**kw)
    assert not (m["type"] == P.MsgProp).any()
    a = CP.copy_triple(start)
    assert CP.step_batch(a[0], voters, a[1], a[2], m).tobytes() == want.tobytes() and not Q.state_differs(a, after)
    for rule in (1, 2, 3, 4):
        a, b = CP.copy_triple(start), CP.copy_triple(start)
        assert CP.step_batch(a[0], voters, a[1], a[2], m, leave_out={rule}).tobytes() == Q.step_batch(b[0], voters, b[1], b[2], m, leave_out={rule}).tobytes()
        assert not Q.state_differs(a, b)


def test_a_malformed_batch_moves_nothing():
    start, voters, m, want, after, plan = CP.props_case(**PROPS[0])
    a = CP.copy_triple(start)
    with pytest.raises(ValueError):
        CP.step_batch(a[0], voters, a[1], a[2], CP.malformed_beside_a_check(m))
    assert not Q.state_differs(a, start)


def test_frames_records_carry_their_count_in_the_high_half():
    """the decoder's form of a record (frames=True): the entry count is _resv's high half, and an empty one there is malformed"""
    start, voters, m, want, after, plan = CP.props_case(**PROPS[0])
    f = np.array(m)
    f["_resv"] = (f["_resv"] & np.uint64(0xFFFFFFFF)) << np.uint64(32)
    a = CP.copy_triple(start)
    assert CP.step_batch(a[0], voters, a[1], a[2], f, frames=True).tobytes() == want.tobytes() and not Q.state_differs(a, after)
    with pytest.raises(ValueError):
        CP.step_batch(a[0], voters, a[1], a[2], np.array(m), frames=True)  # (the low half alone says nothing there)


# ---- raftq_step_frames_respond --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RESPOND))
def test_respond_inputs_show_the_switch_in_the_lead_forms(name):
    start, voters, s, off, at, plan, w, after = _respond(name)
    kw = RESPOND[name]
    got = CP.respond_shows(start, w)
    for k, floor in CP.RESPOND_FLOORS.items():
        assert got[k] >= floor, (k, got)
    CP.assert_planted(start, w, plan)
    if kw.get("hot"):
        assert np.bincount(w["rec"]["group"][w["outs"]["type"] != V.OutSkipped].astype(np.int64)).max() > 32
    # each rule but the fourth (no frame carries type 12) makes a difference
    for rule in (1, 2, 3):
        assert _differs(start, voters, w["rec"], w["outs"], after, rule), ("rule %d makes no difference" % rule, name)
    assert not _differs(start, voters, w["rec"], w["outs"], after, 4)
    # the switch matters: result records and outbound stream
    off_w = RP.want(V.copy_state(start[0]), s, off, at, voters, lead=True)
    assert off_w["outs"].tobytes() != w["outs"].tobytes() and bytes(off_w["stream"]) != bytes(w["stream"])
    assert int((off_w["outs"].view(np.uint8).reshape(-1, 64) != w["outs"].view(np.uint8).reshape(-1, 64)).any(axis=1).sum()) >= 10


def test_respond_band_cases_are_where_they_say():
    for name, lo in (("top", 2**64 - 2**12), ("b32", 2**32 - 6)):
        w = _respond(name)[6]
        assert int(w["sent_ents"]["index"].max()) >= lo and int(w["sent"]["term"].max()) >= lo - 3, name


# ---- proposals through raftq_step_batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", PROPS, ids=[str(sorted(k.items())) for k in PROPS])
def test_props_inputs_discriminate(kw):
    start, voters, m, want, after, plan = CP.props_case(**kw)
    CP.assert_props_planted(start, m, want, plan, kw["n"])
    got = Q.outcomes(start, voters, m, want)
    assert got["passing checks"] >= CP.PLANT and got["failing checks"] >= 2 * CP.PLANT and got["lease-ignored votes"] >= 1, got
    assert got["checks on a non-leader"] >= 1 and got["acks that set a bit"] >= 1, got
    prop = m["type"] == P.MsgProp
    assert (want["type"][prop] == P.OutProposed).sum() >= 8 and (want["type"][prop] == P.OutForward).sum() >= 8
    assert (m["type"] == CP.MsgCheckQuorum).sum() >= 2 * CP.PLANT + 30
    if kw.get("hot"):
        assert np.bincount(m["group"].astype(np.int64)).max() > 32
    for rule in (1, 2, 3, 4):
        assert _differs(start, voters, m, want, after, rule), ("rule %d makes no difference" % rule, kw)
    # the switch matters to the proposals: with the rules left out the deposed leaders take theirs
    st = CP.copy_triple(start)
    without = CP.step_batch(st[0], voters, st[1], st[2], m, leave_out=ALL)
    assert ((without["type"] == P.OutProposed) & (want["type"] != P.OutProposed)).sum() >= CP.PLANT


# ---- Tick and Step in lockstep --------------------------------------------------------------------------------------------------
def _acts_in(r):
    """which of the four rules certainly act in a round, read off the reference's records and the words either side of the batch:
      1  some group ends with an activity bit it did not start with: nothing but rule 1 sets a bit
      2  some group's lead_elapsed was non-zero and ends 0: nothing in Step but reset() clears it
      3  a MsgVote of a higher term came back RAFTQ_OUT_NONE with the term unmoved: without the lease it is answered
      4  a MsgCheckQuorum record carries RAFTQ_OUTF_STEPPED_DOWN: without the rule the record carries no flag
    (a rule may act in other rounds too -- a bit set and cleared again by a later reset, say -- and leave no trace: not claimed)"""
    m, o = r["m"], r["want"]
    (_, ac0, le0), (_, ac1, le1) = r["before"], r["after"]
    return {1: bool((ac1 & ~ac0).any()), 2: bool(((le0 != 0) & (le1 == 0)).any()), 3: bool(CP.lease_ignored(m, o).any()),
            4: bool(((m["type"] == CP.MsgCheckQuorum) & ((o["flags"] & R.FlagSteppedDown) != 0)).any())}


@pytest.mark.parametrize("name", list(CP.LOCK_SHAPES))
def test_lockstep_inputs_discriminate(name):
    start, voters, rounds = _lock(name)
    assert len(rounds) == 4 * CP.LOCK_ET
    got = CP.lockstep_shows(rounds)
    for k, floor in CP.LOCK_FLOORS.items():
        assert got[k] >= floor, (k, got)
    seen = set()
    for r in rounds:
        seen |= set(np.unique(r["tick"][1]).tolist())
    assert seen >= {0, 1, 2, 3}, seen
    # a round's batch is an input of its own.  In EVERY round that holds the traffic a rule acts on, leaving the rule out changes the
    # records or the state behind the batch -- and the second half of the rounds holds such traffic for every rule
    relevant = dict.fromkeys((1, 2, 3, 4), 0)
    for t, r in enumerate(rounds):
        on = _acts_in(r)
        for rule in (1, 2, 3, 4):
            hit = _differs(r["before"], voters, r["m"], r["want"], r["after"], rule, election_tick=CP.LOCK_ET)
            assert hit or not on[rule], ("rule %d makes no difference in round %d" % (rule, t), name)
            relevant[rule] += on[rule] and t >= len(rounds) // 2
    assert all(relevant[rule] >= (3 if rule in (1, 3) else 2) for rule in relevant), relevant
    # what the Step reads is the Tick's word: with the elapsed of the round's start instead, some lease decision falls the other way
    flipped = 0
    prev = start
    for r in rounds:
        st = CP.copy_triple(r["before"])
        st[0].elapsed[:] = prev[0].elapsed
        flipped += CP.step_batch(st[0], voters, st[1], st[2], r["m"], election_tick=CP.LOCK_ET).tobytes() != r["want"].tobytes()
        prev = r["after"]
    assert flipped >= 3, flipped


@pytest.mark.parametrize("long_runs", [False, True], ids=["short-runs", "long-runs"])
def test_lease_case_is_what_it_says(long_runs):
    start, (b1, b2), sets = CP.lease_case(long_runs)
    st = CP.copy_triple(start)
    w1 = CP.step_batch(st[0], None, st[1], st[2], b1)
    w2 = CP.step_batch(st[0], None, st[1], st[2], b2)

    def votes(m, o, groups):
        k = (m["type"] == R.MsgVote) & np.isin(m["group"], groups)
        assert k.sum() == len(groups)
        return o[k]

    for o in (votes(b1, w1, sets["one batch"]), votes(b2, w2, sets["two batches"])):
        assert (o["type"] == R.OutNone).all() and (o["term"] == 4).all() and (o["lead"] == 2).all()
    for key in ("control", "no leader", "candidate"):
        o = votes(b1, w1, sets[key])
        assert (o["type"] == R.OutVoteResp).all() and (o["term"] == 5).all() and (o["reject"] == 0).all(), key
    runs = [int(np.bincount(b["group"].astype(np.int64)).max()) for b in (b1, b2)]
    if long_runs:  # more than kMaxRun = 32: the list walk stalls, both batches go through the sorted walk's replay
        for key in ("one batch", "control"):
            assert (b1["group"] == sets[key][0]).sum() > 32
        assert (b2["group"] == sets["two batches"][0]).sum() > 32
    else:  # no run the list walk cannot take: both batches stay on it
        assert max(runs) <= 2, runs
    # rule 3 alone decides the first two sets: without it every one of their votes is answered
    a = CP.copy_triple(start)
    x1 = CP.step_batch(a[0], None, a[1], a[2], b1, leave_out={3})
    x2 = CP.step_batch(a[0], None, a[1], a[2], b2, leave_out={3})
    assert (votes(b1, x1, sets["one batch"])["type"] == R.OutVoteResp).all() and (votes(b2, x2, sets["two batches"])["type"] == R.OutVoteResp).all()
    # the other three rules have nothing to act on here, and leaving them out changes nothing: no group is led (rules 1 and 4 are
    # the leader's), and every activity word and lead_elapsed is 0 from the start, so the resets behind the answered votes clear nothing
    assert not (start[0].role == 2).any() and not start[1].any() and not start[2].any()
    a = CP.copy_triple(start)
    y1 = CP.step_batch(a[0], None, a[1], a[2], b1, leave_out={1, 2, 4})
    y2 = CP.step_batch(a[0], None, a[1], a[2], b2, leave_out={1, 2, 4})
    assert y1.tobytes() == w1.tobytes() and y2.tobytes() == w2.tobytes() and not Q.state_differs(a, st)
