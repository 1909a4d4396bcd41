"""GPU: CheckQuorum beside the other Step switches, against tests/ref_check_quorum_props.py, byte for byte.

raftq_step_frames_respond with raftq_set_check_quorum AND raftq_respond_set_lead / raftq_respond_set_props on launches the four
walks no other suite reaches (raftq_step.hip launch_walk: h->cq picks the *_cq_* family, lead_step(h) the *_lead form,
masked_step(h) the *_voters form):
  step_lists_cq_lead_kernel          test_frames_respond_under_the_switch, unmasked cases, the default walk
  step_lists_cq_lead_voters_kernel   the masked cases, the default walk
  step_cq_lead_kernel                the unmasked cases under RAFTQ_STEP_WALK=sort, and the replay of the "hot" case's stalled batch
  step_cq_lead_voters_kernel         the masked cases under RAFTQ_STEP_WALK=sort, and the replay of "hot-masked"
Then raftq_step_batch with raftq_step_set_props under the switch (MsgProp and type 12 in one batch), Tick and Step alternating over
one handle with nothing re-loaded, and the lease behind a reset of the same batch or of a batch still in flight.  What each input
shows is asserted on the reference alone by tests/test_check_quorum_props_ref.py."""
import functools

import numpy as np
import pytest

from oracle import pywire as W
from raftsql_amd._lib import RAFTQ_EINVAL
from tests import _stepgen
from tests import ref_check_quorum as Q
from tests import ref_check_quorum_props as CP
from tests import ref_respond_props as RP
from tests import ref_step_voters as V
from tests.test_check_quorum_gpu import _code, _same_after, _same_records
from tests.test_respond_props_gpu import _call, _held_to

pytestmark = pytest.mark.gpu

RESPOND = CP.respond_case_list()
PROPS = CP.props_case_list()


@pytest.fixture(scope="module")
def S(gpu_engine_cls):
    from raftsql_amd import step

    return step


# ---- raftq_step_frames_respond: the four *_cq_lead* walks -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _respond(name):
    start, voters, s, off, at, plan = CP.respond_case(**RESPOND[name])
    st = CP.copy_triple(start)
    return start, voters, s, off, at, CP.want(st[0], st[1], st[2], s, off, at, voters), st


def _wire_engine(start, voters, on=True, lead=True, props=True):
    from raftsql_amd.wire import WireEngine

    s, active, lead_elapsed = start
    e = WireEngine(s.G, s.N, s.self_peer)
    _stepgen.load_engine(e, s)
    e.set_timers(Q.ELECTION_TICK, 1, CP.TICK_SEED)
    if on:
        e.set_check_quorum(True)
        e.load_activity(active, lead_elapsed)
    e.set_step_props(True)
    if props:
        e.set_respond_props(True)
    if lead:
        e.set_respond_lead(True)
    if voters is not None:
        e.load_voters(voters)
        e.set_step_voters(True)
        e.set_bcast_voters(True)
    return e


def _walk(monkeypatch, walk):
    if walk == "sort":
        monkeypatch.setenv("RAFTQ_STEP_WALK", "sort")
    else:
        monkeypatch.delenv("RAFTQ_STEP_WALK", raising=False)


@pytest.mark.parametrize("walk", ["lists", "sort"])
@pytest.mark.parametrize("name", list(RESPOND))
def test_frames_respond_under_the_switch(oracle, S, monkeypatch, name, walk):
    """the result records, the outbound stream, the frame offsets, peer_off, the counts, every word of state, the activity arrays"""
    _walk(monkeypatch, walk)
    start, voters, s, off, at, w, after = _respond(name)
    n_e = len(W.wire_decode(s, off)[1])
    with _wire_engine(start, voters) as e:
        _held_to(e, w, _call(e, s, off, n_e + 1, at), s, off, (name, walk))
        _same_after(e, after, (name, walk))


@pytest.mark.parametrize("lead,props", [(True, False), (False, True)], ids=["lead-alone", "props-alone"])
def test_frames_respond_with_one_of_the_two_switches(oracle, S, lead, props):
    """either switch alone launches the lead forms too (lead_step): the other kind is left to the host and ends its prefix"""
    name = "n5-masked"
    start, voters, s, off, at, _, _ = _respond(name)
    st = CP.copy_triple(start)
    w = CP.want(st[0], st[1], st[2], s, off, at, voters, lead=lead, props=props)
    assert (len(w["wins"]) > 0) == lead and (len(w["taken"]) > 0) == props
    n_e = len(W.wire_decode(s, off)[1])
    with _wire_engine(start, voters, lead=lead, props=props) as e:
        _held_to(e, w, _call(e, s, off, n_e + 1, at), s, off, (name, lead, props))
        _same_after(e, st, (name, lead, props))


@pytest.mark.parametrize("name", ["n3", "hot-masked"])
def test_frames_respond_switch_off_twin(oracle, S, name):
    """the same input on a handle without raftq_set_check_quorum: ref_respond_props.want's bytes, as before"""
    start, voters, s, off, at, w_on, _ = _respond(name)
    st = V.copy_state(start[0])
    w = RP.want(st, s, off, at, voters, lead=True)
    assert bytes(w["stream"]) != bytes(w_on["stream"])
    n_e = len(W.wire_decode(s, off)[1])
    with _wire_engine(start, voters, on=False) as e:
        _held_to(e, w, _call(e, s, off, n_e + 1, at), s, off, ("switch off", name))
        _stepgen.assert_same_state(e, st)


# ---- raftq_step_batch: MsgProp and type 12 in one batch --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _props(k):
    return CP.props_case(**PROPS[k])


def _node_engine(S, start, voters, et=Q.ELECTION_TICK, ht=1, tick_voters=False):
    s, active, lead_elapsed = start
    e = S.NodeEngine(s.G, s.N, s.self_peer)
    _stepgen.load_engine(e, s)
    e.set_timers(et, ht, CP.TICK_SEED)
    if voters is not None:
        e.load_voters(voters)
        e.set_step_voters(True)
        if tick_voters:
            e.set_tick_voters(True)
    e.set_step_props(True)
    e.set_check_quorum(True)
    e.load_activity(active, lead_elapsed)
    return e


@pytest.mark.parametrize("k", range(len(PROPS)), ids=["-".join(str(v) for v in kw.values()) for kw in PROPS])
def test_step_batch_with_proposals_under_the_switch(S, k):
    start, voters, m, want, after, _ = _props(k)
    with _node_engine(S, start, voters) as e:
        got, _ = e.step_batch(np.array(m))
        _same_records(got, want, m, PROPS[k])
        _same_after(e, after, PROPS[k])


@pytest.mark.parametrize("walk", ["lists", "sort"])
def test_step_batch_with_proposals_both_walks(S, monkeypatch, walk):
    _walk(monkeypatch, walk)
    k = len(PROPS) - 1
    start, voters, m, want, after, _ = _props(k)
    assert PROPS[k].get("hot") and np.bincount(m["group"].astype(np.int64)).max() > 32
    with _node_engine(S, start, voters) as e:
        got, _ = e.step_batch(np.array(m))
        _same_records(got, want, m, walk)
        _same_after(e, after, walk)


@pytest.mark.parametrize("k", [0, 3], ids=["all-slots", "masks"])
def test_a_malformed_proposal_beside_a_check_applies_nothing(S, k):
    """the one atomicity case the switch adds: the check kernel refuses the batch before any walk runs -- no word of state moves,
    the activity words included; the whole batch then steps as if nothing had been tried"""
    start, voters, m, want, after, _ = _props(k)
    bad = CP.malformed_beside_a_check(m)
    with _node_engine(S, start, voters) as e:
        code, _ = _code(e.step_batch, bad)
        assert code == RAFTQ_EINVAL
        _same_after(e, start, "behind the refused batch")
        got, _ = e.step_batch(np.array(m))
        _same_records(got, want, m, "behind the refusal")
        _same_after(e, after, "behind the refusal")


# ---- Tick and Step in lockstep --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lock(name):
    return CP.lockstep(**CP.LOCK_SHAPES[name])


@pytest.mark.parametrize("name", list(CP.LOCK_SHAPES))
def test_tick_and_step_in_lockstep(S, name):
    """one handle, one reference, 4 * election_tick rounds; nothing is loaded into the handle after round 0: what the Tick leaves in
    elapsed and lead_elapsed is what Step reads, what Step leaves is what the next Tick reads"""
    start, voters, rounds = _lock(name)
    with _node_engine(S, start, voters, et=CP.LOCK_ET, ht=CP.LOCK_HT, tick_voters=True) as e:
        for t, r in enumerate(rounds):
            el, act, ac, le, n_hup, n_beat = r["tick"]
            assert e.tick() == (n_hup, n_beat), (name, t)
            g_act, g_el, g_role = e.read_tick()
            assert np.array_equal(g_act, act) and np.array_equal(g_el, el) and np.array_equal(g_role, r["before"][0].role), (name, t)
            g_ac, g_le = e.read_activity()
            assert np.array_equal(g_ac, ac) and np.array_equal(g_le, le), (name, t)
            lists = {}
            for k, collect in ((1, e.collect_hups), (2, e.collect_beats), (3, e.collect_checks)):
                ids, cnt = collect()
                assert cnt == int((act == k).sum()) and np.array_equal(ids, np.flatnonzero(act == k)), (name, t, k)
                lists[k] = ids
            m = r["m"]
            # the batch holds one check for every id the device listed, and a MsgHup for every listed id (the random traffic has more)
            assert np.array_equal(np.sort(m["group"][m["type"] == S.MSG_CHECK_QUORUM]), lists[3]), (name, t)
            assert np.isin(lists[1], m["group"][m["type"] == S.MSG_HUP]).all(), (name, t)
            got, _ = e.step_batch(np.array(m))
            _same_records(got, r["want"], m, (name, t))
            _same_after(e, r["after"], (name, t))


@pytest.mark.parametrize("form", ["short-lists", "short-sort", "long"])
def test_the_lease_behind_a_reset_of_this_batch_and_of_one_in_flight(S, monkeypatch, form):
    """a heartbeat zeroes elapsed; the higher-term MsgVote behind it -- in the same batch, or in a second batch submitted before the
    first is collected -- finds the follower in lease; alone it is answered.
      short-lists   no group has more than two records in a batch: both batches go through step_lists_cq_kernel, and the two
                    submitted back to back are two list walks in flight -- the second reads the reset the first has not stored yet
      short-sort    the same batches under RAFTQ_STEP_WALK=sort: step_cq_kernel, two sorted walks in flight
      long          one group of each set has a run longer than kMaxRun = 32: the list walk stalls and applies nothing, the stalled
                    batch and the one in flight behind it are replayed through the sorted walk one after the other"""
    _walk(monkeypatch, "sort" if form == "short-sort" else "lists")
    start, (b1, b2), _ = CP.lease_case(long_runs=form == "long")
    assert (max(np.bincount(b["group"].astype(np.int64)).max() for b in (b1, b2)) > 32) == (form == "long")
    st = CP.copy_triple(start)
    w1 = CP.step_batch(st[0], None, st[1], st[2], b1)
    w2 = CP.step_batch(st[0], None, st[1], st[2], b2)
    with _node_engine(S, start, None) as e:
        e.step_submit(b1)
        e.step_submit(b2)
        g1, _ = e.step_collect()
        g2, _ = e.step_collect()
        _same_records(g1, w1, b1, ("first batch", form))
        _same_records(g2, w2, b2, ("second batch", form))
        _same_after(e, st, ("both batches", form))
    with _node_engine(S, start, None) as e:  # and one call at a time
        for b, w in ((b1, w1), (b2, w2)):
            got, _ = e.step_batch(b)
            _same_records(got, w, b, ("one call at a time", form))
        _same_after(e, st, ("one call at a time", form))
