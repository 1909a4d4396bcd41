"""GPU: the tally word and its bytes (raftq_kernels.hpp kTallyValid).  While the device knows
tally[g] == granted | rejected << 4 of every group's vote word, a sweep with votes reads the byte instead of the word.  One
case per writer of the vote words: each sets the word, keeps it or ends it, and reads it back with raftq_tally -- that shows
which branch the sweeps took.  After every move every dispatch is held equal to the oracle, outcomes and the won / lost
tallies: one handle (votes alone, votes with commit, plain and gated), and a set in its grid and persistent forms that mixes
the handle with a companion whose word is the other way round.  The outcome array is overwritten in front of every dispatch.

G = 4,099 (tests/ref_tally.py): two full 2,048-group tiles and a ragged third.  tests/test_tally_ref.py shows that the inputs
hold all three outcomes before and after the batch, and groups whose byte would disagree with its word had a duplicate
record been counted twice.  Every input is in range unless the case says otherwise."""
import os

import numpy as np
import pytest

from raftsql_amd._lib import (CYCLE_TRUSTED, SET_GRID, SET_PERSISTENT, SWEEP_COMMIT, SWEEP_GATED, SWEEP_NO_ADOPT, SWEEP_VOTES)
from raftsql_amd.engine import SweepSet
from tests import ref_tally as T

pytestmark = pytest.mark.gpu

G = T.G
PEERS = (1, 2, 3, 5, 7, 9)
FORMS = (SWEEP_VOTES, SWEEP_VOTES | SWEEP_COMMIT, SWEEP_VOTES | SWEEP_COMMIT | SWEEP_GATED)


def _loaded(E, st):
    e = E(st.n_groups, st.n_peers)
    e.load_state(st)
    return e


def _ref(st):
    return [st.match.copy(), st.committed.copy(), st.first_idx_cur_term.copy(), st.votes.copy()]


def _scribble(e):
    """leave something else in the handle's outcome array, so that the next dispatch's stores are what is read back: a masked
    sweep in which no slot votes finds every group pending (the masks go again at once; neither touches the words, the bytes or
    the tally word)"""
    e.load_voters(np.zeros(G, np.uint16))
    e.sweep(SWEEP_VOTES | SWEEP_NO_ADOPT)
    e.load_voters(None)
    assert not e.read_outcome().any()


def _check(oracle, es, refs):
    """refs[k] = [match, committed, first_idx, votes] of member k as it stands; every dispatch leaves it so (NO_ADOPT).  The
    outcome array is scribbled over in front of every dispatch: each has to store its own outcomes."""
    want = [{g: oracle.commit_advance(m, c, g, f) for g in (False, True)} for m, c, f, _ in refs]
    tally = [oracle.vote_tally(v) for _, _, _, v in refs]
    for e, w, t in zip(es, want, tally):
        for form in FORMS:
            _scribble(e)
            c = e.sweep(form | SWEEP_NO_ADOPT)
            assert np.array_equal(e.read_outcome(), t[0]), form
            assert (c.n_won, c.n_lost) == (t[1], t[2]), form
            if form & SWEEP_COMMIT:
                gated = bool(form & SWEEP_GATED)
                assert np.array_equal(e.read_committed(), w[gated][0]) and c.n_changed == w[gated][1], form
    for mode, wgs in ((SET_GRID, 0), (SET_PERSISTENT, 3)):
        for form in FORMS:
            for e in es:  # (a set of this kind refuses masks on its members: scribble first, then form the set)
                _scribble(e)
            with SweepSet(es) as s:
                s.set_mode(mode, wgs)
                per, _ = s.sweep(form | SWEEP_NO_ADOPT)
                for e, w, t, c in zip(es, want, tally, per):
                    assert np.array_equal(e.read_outcome(), t[0]), (mode, form)
                    assert (c.n_won, c.n_lost) == (t[1], t[2]), (mode, form)
                    if form & SWEEP_COMMIT:
                        gated = bool(form & SWEEP_GATED)
                        assert np.array_equal(e.read_committed(), w[gated][0]) and c.n_changed == w[gated][1], (mode, form)


def _cleared(E, st):
    """a handle that holds `st` with its tally word ended (a voter delta that resets a slot whose field is empty already: the
    words stand, the word goes), every slot voting again"""
    e = _loaded(E, st)
    g = int(np.nonzero(st.votes[st.n_peers - 1] == 0)[0][0])
    e.apply_voter_deltas(e.pack_voter_deltas([g], [(1 << st.n_peers) - 1], [1 << (st.n_peers - 1)]))
    e.load_voters(None)
    assert not e.tally()
    return e, g


def _pair(E, oracle, e, ref, n, seed):
    """`e` with a companion whose word is the other way round: the set then mixes members with and without a valid word"""
    other = T.gpu_state(n, seed)
    if e.tally():
        o, g = _cleared(E, other)
        oref = _ref(other)
        oref[0][n - 1, g] = 0  # (the reset slot's Match)
    else:
        o, oref = _loaded(E, other), _ref(other)
    with o:
        assert o.tally() != e.tally()
        _check(oracle, [e, o], [ref, oref])
        assert o.tally() != e.tally()  # sweeps write neither word


@pytest.mark.parametrize("n", PEERS)
def test_create_is_valid_and_load_builds(gpu_engine_cls, oracle, n):
    st = T.gpu_state(n, 32000 + n)
    with gpu_engine_cls(G, n) as e:
        assert e.tally()  # raftq_create: zero words, zero bytes
        e.load_match(st.match, st.committed)
        e.load_terms(st.cur_term, st.first_idx_cur_term)
        ref = _ref(st)
        ref[3][:] = 0
        _pair(gpu_engine_cls, oracle, e, ref, n, 32010 + n)  # nobody has voted: every group pending, from the zero bytes
        e.load_votes(st.votes)
        assert e.tally()
        _pair(gpu_engine_cls, oracle, e, _ref(st), n, 32020 + n)


@pytest.mark.parametrize("trusted", [False, True], ids=["validated", "trusted"])
@pytest.mark.parametrize("n", PEERS)
def test_vote_ingest_keeps_the_bytes(gpu_engine_cls, oracle, n, trusted):
    """a batch with duplicates per (group, peer) and both answers for one slot: the first in batch position wins and the byte
    counts it once; then the same batch again -- every slot it names is answered, no byte moves"""
    st = T.gpu_state(n, 32000 + n)
    g, p, v = T.gpu_vote_batch(n, 32050 + n)

    def ingest(e):
        if trusted:
            _, vd = e.stage_packed(0, len(g))
            vd[:] = e.pack_vote_deltas(g, p, v)
            e.cycle_packed(SWEEP_COMMIT | SWEEP_VOTES | SWEEP_NO_ADOPT | CYCLE_TRUSTED, None, vd, cap=G, inplace=True, want_counts=False)
        else:
            e.apply_vote_deltas(g, p, v)

    with _loaded(gpu_engine_cls, st) as e:
        ref = _ref(st)
        for _ in range(2):
            ingest(e)
            ref[3] = oracle.apply_vote_deltas(ref[3], g, p, v)
            assert e.tally()
            assert np.array_equal(e.read_votes(), ref[3])
            _pair(gpu_engine_cls, oracle, e, ref, n, 32060 + n)
        assert e.tally_rebuild()  # the build pass over the words the ingest left: the same bytes
        _check(oracle, [e], [ref])


@pytest.mark.parametrize("n", PEERS)
def test_refused_turn_leaves_word_and_bytes(gpu_engine_cls, oracle, n):
    """an untrusted batch with one record out of range applies nothing"""
    st = T.gpu_state(n, 32100 + n)
    g, p, v = T.gpu_vote_batch(n, 32150 + n)
    g = g.copy()
    g[1500] = G  # one group past the end
    with _loaded(gpu_engine_cls, st) as e:
        with pytest.raises(Exception):
            e.apply_vote_deltas(g, p, v)
        assert e.tally() and np.array_equal(e.read_votes(), st.votes)
        _pair(gpu_engine_cls, oracle, e, _ref(st), n, 32160 + n)


@pytest.mark.parametrize("n", PEERS)
def test_campaign_keeps_the_bytes(gpu_engine_cls, oracle, n):
    st = T.gpu_state(n, 32200 + n)
    groups = np.array([0, 2, 3, 7, 2047, 2048, G - 1], np.uint64)
    with _loaded(gpu_engine_cls, st) as e:
        ref = _ref(st)
        e.load_roles(np.zeros(G, np.uint8))
        e.campaign(groups, self_peer=n - 1)
        _, _, ref[3] = oracle.campaign(np.zeros(G, np.uint8), np.zeros(G, np.uint32), ref[3], groups, n - 1)
        assert e.tally() and np.array_equal(e.read_votes(), ref[3])
        _pair(gpu_engine_cls, oracle, e, ref, n, 32210 + n)
        # the election goes on: the other peers answer the candidates, the bytes follow
        others = np.arange(n - 1, dtype=np.uint32)
        g, p = np.repeat(groups, n - 1), np.tile(others, len(groups))
        v = np.where((g + p) % 3 == 0, 2, 1).astype(np.uint8)
        if len(g):
            e.apply_vote_deltas(g, p, v)
            ref[3] = oracle.apply_vote_deltas(ref[3], g, p, v)
        assert e.tally() and np.array_equal(e.read_votes(), ref[3])
        _pair(gpu_engine_cls, oracle, e, ref, n, 32220 + n)


@pytest.mark.parametrize("n", PEERS)
def test_voter_delta_with_a_reset_ends_it_and_rebuild_restores(gpu_engine_cls, oracle, n):
    st = T.gpu_state(n, 32300 + n)
    full = (1 << n) - 1
    with _loaded(gpu_engine_cls, st) as e:
        ref = _ref(st)
        e.apply_voter_deltas(e.pack_voter_deltas([3], [full], [0]))  # a new mask, no slot reset: the words stand
        assert e.tally()
        e.apply_voter_deltas(e.pack_voter_deltas([2], [full], [1]))  # group 2 is won by its first q slots: slot 0's grant goes
        assert not e.tally()
        ref[0][0, 2] = 0
        ref[3][0, 2] = 0
        assert np.array_equal(e.read_votes(), ref[3])
        e.load_voters(None)  # every slot votes again: the unmasked dispatches, over the words
        _pair(gpu_engine_cls, oracle, e, ref, n, 32310 + n)
        assert oracle.vote_tally(ref[3])[0][2] == 0  # (a stale byte would still say won)
        assert e.tally_rebuild()
        _pair(gpu_engine_cls, oracle, e, ref, n, 32320 + n)


@pytest.mark.parametrize("n", PEERS)
def test_masked_handle_answers_from_its_words(gpu_engine_cls, oracle, n):
    from tests import ref_voters as RV

    st = T.gpu_state(n, 32400 + n)
    rng = np.random.default_rng(32400 + n)
    voters = (rng.integers(0, 1 << n, G) | 1).astype(np.uint16)
    with _loaded(gpu_engine_cls, st) as e:
        e.load_voters(voters)
        assert e.tally()  # the word stands; the masked kernels do not ask it
        want, won, lost = RV.vote_tally(st.votes, voters)
        for form in FORMS:
            c = e.sweep(form | SWEEP_NO_ADOPT)
            assert np.array_equal(e.read_outcome(), want) and (c.n_won, c.n_lost) == (won, lost), form
        e.load_voters(None)
        _pair(gpu_engine_cls, oracle, e, _ref(st), n, 32410 + n)


@pytest.mark.parametrize("n", PEERS)
def test_step_that_stores_a_vote_word_ends_it(gpu_engine_cls, oracle, n):
    from raftsql_amd.step import MSG_APP_RESP, MSG_HUP, ROLE_FOLLOWER, ROLE_LEADER, NodeEngine, pack_msgs

    st = T.gpu_state(n, 32500 + n)
    st.match[:] = np.minimum(st.match, np.uint64(10))
    st.match[0] = 10
    st.committed[:] = 0
    term, first = np.full(G, 3, np.uint64), np.full(G, 1, np.uint64)
    role = np.full(G, ROLE_LEADER, np.uint8)
    role[5] = ROLE_FOLLOWER
    with NodeEngine(G, n) as e:
        e.load_match(st.match, st.committed)
        e.load_votes(st.votes)
        e.load_terms(term, first)
        e.load_roles(role)
        e.load_node(term=term, last_index=np.full(G, 100, np.uint64), last_term=term)
        assert e.tally()
        if n >= 2:
            e.step_batch(pack_msgs(np.array([9], np.uint64), MSG_APP_RESP, term=3, frm=1, index=50))  # stores no vote word
            assert e.tally()
        e.step_batch(pack_msgs(np.array([5], np.uint64), MSG_HUP))  # becomeCandidate: group 5's word is reset to the own grant
        assert not e.tally()
        votes = e.read_votes()
        if n >= 2:  # (a group of one wins at once: becomeLeader empties the word again)
            assert (votes[:, 5] == np.eye(n, dtype=np.uint8)[0]).all() and not np.array_equal(votes, st.votes)
        node = e.read_node()
        ref = [e.read_match(), node["committed"], node["first_idx"], votes]
        _pair(gpu_engine_cls, oracle, e, ref, n, 32510 + n)
        assert e.tally_rebuild()
        _pair(gpu_engine_cls, oracle, e, ref, n, 32520 + n)


@pytest.mark.parametrize("n", (2, 3, 5, 7, 9))
def test_step_from_wire_frames_ends_it(gpu_engine_cls, oracle, n):
    """the same write-back reached through raftq_step_submit_wire: a MsgVote frame of a higher term makes three leaders
    followers, which empties their vote words"""
    from oracle import pywire as W
    from raftsql_amd.step import MSG_VOTE, ROLE_LEADER
    from raftsql_amd.wire import WireEngine

    st = T.gpu_state(n, 32800 + n)
    st.match[:] = np.minimum(st.match, np.uint64(10))
    st.match[0] = 10
    st.committed[:] = 0
    term, first = np.full(G, 3, np.uint64), np.full(G, 1, np.uint64)
    groups = np.array([2, 2048, G - 1])
    assert st.votes[:, groups].any(axis=0).all()
    with WireEngine(G, n, 0) as e:
        e.load_match(st.match, st.committed)
        e.load_votes(st.votes)
        e.load_terms(term, first)
        e.load_roles(np.full(G, ROLE_LEADER, np.uint8))
        e.load_node(term=term, last_index=np.full(G, 100, np.uint64), last_term=term)
        assert e.tally()
        m = np.zeros(len(groups), W.WIRE_MSG_DT)
        m["group"], m["type"], m["term"], m["from"], m["to"] = groups, MSG_VOTE, 4, 1, 0
        m["index"], m["log_term"] = 200, 3
        s, off = W.wire_encode(m)
        e.step_submit_wire(s, off)
        e.step_collect()
        assert not e.tally()
        votes = e.read_votes()
        assert not votes[:, groups].any() and not np.array_equal(votes, st.votes)
        node = e.read_node()
        ref = [e.read_match(), node["committed"], node["first_idx"], votes]
        _pair(gpu_engine_cls, oracle, e, ref, n, 32810 + n)
        assert e.tally_rebuild()
        _pair(gpu_engine_cls, oracle, e, ref, n, 32820 + n)


@pytest.mark.parametrize("n", (2, 3, 5, 9))
def test_device_built_election_round_ends_it(oracle, n):
    """raftq_tick_elect_frames: Step(MsgHup) applied on the device to the groups whose timers fired (raftq_elect_kernels.hpp),
    driven and held to the oracle by tests/test_tick_elect_gpu.py's own check"""
    from tests import test_tick_elect_gpu as TE

    hb, me = 1, n - 1
    rng = np.random.default_rng(32900 + n)
    st = TE.make_state(rng, G, n, me, hb)
    e, twin = TE._pair(G, n, me, st, hb)
    with e, twin:
        assert e.tally()  # loaded: built
        nh, _, _, _ = TE.check_tick(oracle, e, twin, st, 0, hb, G, G, True, f"N={n}")  # (sweeps, and holds the outcomes to the oracle)
        assert nh > 0 and not e.tally()
        want = oracle.vote_tally(st.votes)
        assert e.tally_rebuild()
        for form in FORMS[:2]:
            _scribble(e)
            c = e.sweep(form | SWEEP_NO_ADOPT)
            assert np.array_equal(e.read_outcome(), want[0]) and (c.n_won, c.n_lost) == (want[1], want[2]), form


@pytest.mark.parametrize("n", PEERS)
def test_clone_carries_bytes_and_word(gpu_engine_cls, oracle, n, monkeypatch):
    a_st, b_st = T.gpu_state(n, 32600 + n), T.gpu_state(n, 32650 + n)
    monkeypatch.setenv("RAFTQ_TALLY", "0")
    with gpu_engine_cls(G, n) as bare_dst, _loaded(gpu_engine_cls, b_st) as bare_src:
        monkeypatch.delenv("RAFTQ_TALLY")  # read once, at raftq_create
        b_ended, g = _cleared(gpu_engine_cls, b_st)
        b_ref = _ref(b_st)
        b_ref[0][n - 1, g] = 0
        with _loaded(gpu_engine_cls, a_st) as a, b_ended as b, gpu_engine_cls(G, n) as d1, gpu_engine_cls(G, n) as d2, \
                gpu_engine_cls(G, n) as d3:
            assert (a.tally(), b.tally(), bare_src.tally(), bare_dst.tally()) == (True, False, False, False)
            d1.clone_state_from(a)  # valid source, fresh destination: the bytes and the word
            assert d1.tally()
            d2.load_state(a_st)
            d2.clone_state_from(b)  # a destination that had its own takes the source's ended word
            assert not d2.tally()
            _check(oracle, [d1, d2], [_ref(a_st), b_ref])
            d3.clone_state_from(bare_src)  # a source without the mirror: the destination's bytes are not the new words'
            assert not d3.tally()
            bare_dst.clone_state_from(a)  # a destination without: nowhere to put them
            assert not bare_dst.tally() and not bare_dst.tally_rebuild()
            _check(oracle, [d3, bare_dst], [_ref(b_st), _ref(a_st)])
            assert d3.tally_rebuild()
            _check(oracle, [d3, bare_dst], [_ref(b_st), _ref(a_st)])
    assert "RAFTQ_TALLY" not in os.environ


@pytest.mark.parametrize("n", PEERS)
def test_raftq_tally_0_is_never_valid(gpu_engine_cls, oracle, n, monkeypatch):
    st = T.gpu_state(n, 32700 + n)
    g, p, v = T.gpu_vote_batch(n, 32750 + n)
    monkeypatch.setenv("RAFTQ_TALLY", "0")
    with gpu_engine_cls(G, n) as e:
        monkeypatch.delenv("RAFTQ_TALLY")  # read once, at raftq_create: the companion has the mirror, the same moves keep it
        with gpu_engine_cls(G, n) as o:
            _tally_0_body(oracle, n, st, g, p, v, e, o)
    assert "RAFTQ_TALLY" not in os.environ


def _tally_0_body(oracle, n, st, g, p, v, e, o):
    assert not e.tally() and o.tally()
    e.load_state(st)
    o.load_state(st)
    assert not e.tally() and not e.tally_rebuild()
    e.apply_vote_deltas(g, p, v)
    o.apply_vote_deltas(g, p, v)
    ref = _ref(st)
    ref[3] = oracle.apply_vote_deltas(ref[3], g, p, v)
    e.load_roles(np.zeros(G, np.uint8))
    e.campaign(np.array([6], np.uint64), self_peer=0)
    o.load_roles(np.zeros(G, np.uint8))
    o.campaign(np.array([6], np.uint64), self_peer=0)
    _, _, ref[3] = oracle.campaign(np.zeros(G, np.uint8), np.zeros(G, np.uint32), ref[3], np.array([6], np.uint64), 0)
    assert not e.tally() and o.tally()
    _check(oracle, [e, o], [ref, [r.copy() for r in ref]])
