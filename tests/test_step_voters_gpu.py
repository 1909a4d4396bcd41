"""GPU: Step over each group's own voters (raftq_step_set_voters; step_voters_kernel, step_lists_voters_kernel,
log_deltas_voters_kernel) against the masked statement tests/ref_step_voters.py: every result byte and every word of state --
node fields, match, votes, first_idx, role, elapsed, committed.

Shapes: N = 8 is the widest 16-bit vote word, N = 9 the 32-bit one; 3149 groups = several blocks and a ragged last one, 129 =
across one block's wave boundary, 1 = a single group."""
import functools

import numpy as np
import pytest

from raftsql_amd import _lib
from raftsql_amd._lib import RAFTQ_EINVAL, RAFTQ_ESTATE, SWEEP_COMMIT, SWEEP_GATED, SWEEP_VOTES
from raftsql_amd.engine import RaftqError
from tests import _stepgen
from tests import ref_step_voters as V
from tests import ref_voters as RV

pytestmark = pytest.mark.gpu

SHAPES = ((1, 0), (2, 1), (3, 0), (5, 4), (8, 2), (9, 8))
GROUPS = (3149, 129, 1)
G0 = GROUPS[0]


@pytest.fixture(scope="module")
def S(gpu_engine_cls):
    from raftsql_amd import step

    return step


def _engine(S, s, voters, on=True, cls=None):
    e = (cls or S.NodeEngine)(s.G, s.N, s.self_peer)
    _stepgen.load_engine(e, s)
    if voters is not None:
        e.load_voters(voters)
    if on:
        e.set_step_voters(True)
    return e


def _same_records(got, want, msgs, what=""):
    assert got.dtype.itemsize == want.dtype.itemsize == 64 and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, 64) != want.view(np.uint8).reshape(-1, 64)).any(axis=1))
        assert False, (what, len(bad), int(bad[0]), msgs[bad[0]], got[bad[0]], want[bad[0]])


def _code(f, *args, **kw):
    with pytest.raises(RaftqError) as ei:
        f(*args, **kw)
    return ei.value.code, str(ei.value)


# ---- the directed inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["commit", "election"])
@pytest.mark.parametrize("n,self_peer", SHAPES)
def test_directed_inputs(S, n, self_peer, kind):
    make = V.commit_input if kind == "commit" else V.election_input
    # the inputs discriminate (tests/test_step_voters_ref.py says how each share is read), asserted before anything runs
    s, voters, m = make(n, self_peer, G0, 8500 + n)
    a = V.copy_state(s)
    V.step_batch(a, voters, m)
    if kind == "commit":
        full = RV.commit_advance(a.match, s.committed, V.full_masks(n, G0), True, s.first_idx)[0]
        share = float((RV.commit_advance(a.match, s.committed, voters, True, s.first_idx)[0] != full).mean())
    else:
        b = V.copy_state(s)
        V.step_batch(b, V.full_masks(n, G0), m)
        share = float((a.role != b.role).mean())
    print("%s input, N = %d: the masks change the outcome in %.3f of the groups" % (kind, n, share))
    assert share >= V.floor_for(kind, n), (kind, n, share)
    for k, g in enumerate(GROUPS):
        s, voters, m = make(n, self_peer, g, 8500 + n + 100 * k)
        with _engine(S, s, voters) as e:
            want = V.step_batch(s, voters, m)
            got, touched = e.step_batch(m)
            assert touched == g
            _same_records(got, want, m, (kind, n, g))
            _stepgen.assert_same_state(e, s)
            assert np.array_equal(e.read_voters(), voters)


# ---- random traffic: in-batch ordering, both walks, both result formats ---------------------------------------------------------
def _leaky_state(rng, g, n, self_peer):
    """_stepgen.random_state + masks with the edge cases planted + tests/test_voters_gpu.State's leak: whatever a non-voter
    holds must not count -- in the led groups its Match is the log's tail (the largest value a Match takes there), and among
    the candidates it has granted in the even groups and rejected in the odd ones"""
    s = _stepgen.random_state(rng, g, n, self_peer)
    voters = rng.integers(0, 1 << n, g).astype(np.uint16)
    me = 1 << self_peer
    other = 1 << ((self_peer + 1) % n)
    full = (1 << n) - 1
    edge = np.array([0, full, me, other, full & ~me, 0, full, me, other, full & ~me], np.uint16)  # empty, full, self only, a single
    at = rng.permutation(g)[:min(g, edge.size)]                                                   # non-self voter, self not a voter
    voters[at] = edge[:at.size]
    bits = RV.member_bits(voters, n)
    led, cand = s.role == 2, s.role == 1
    s.match[:] = np.where(~bits & led[None, :], s.last_index[None, :], s.match)
    s.votes[:] = np.where(~bits & cand[None, :], np.where(np.arange(g) % 2 == 0, 1, 2)[None, :], s.votes).astype(np.uint8)
    s.votes[self_peer, cand] = 1
    return s, voters


def _tail_reports(rng, s, k=300):
    g = np.sort(rng.integers(0, s.G, k)).astype(np.uint64)
    first = np.concatenate([[True], g[1:] != g[:-1]])
    r = np.arange(k) - np.maximum.accumulate(np.where(first, np.arange(k), 0))  # 0, 1, 2 .. within a group
    li = s.last_index[g] + r.astype(np.uint64) + rng.integers(0, 2, k).astype(np.uint64) * first
    lt = np.maximum(s.last_term[g], s.term[g] * (s.role[g] == 2))
    ct = np.where(rng.random(k) < 0.5, 0, s.committed[g] + rng.integers(0, 4, k).astype(np.uint64))
    return g, li, lt, ct


@functools.lru_cache(maxsize=None)
def _traffic(n, self_peer):
    """the reference, once per shape and never changed: start state, masks, and per round (msgs, records, tail reports, their
    answers, last_index / committed before the batch, state after)"""
    rng = np.random.default_rng(8600 + 10 * n + self_peer)
    g = 777
    s, voters = _leaky_state(rng, g, n, self_peer)
    start = V.copy_state(s)
    hot = rng.choice(g, 40, replace=False)
    rounds = []
    for rnd in range(6):
        m = _stepgen.random_batch(rng, s, 4000, hot_groups=hot if rnd % 2 == 0 else None)
        before = (s.last_index.copy(), s.committed.copy())
        want = V.step_batch(s, voters, m)
        mid = V.copy_state(s)
        rep = _tail_reports(rng, s)
        ans = V.apply_log_deltas(s, voters, *rep)
        rounds.append((m, want, rep, ans, before, mid, V.copy_state(s)))
    assert max(np.unique(rounds[0][0]["group"], return_counts=True)[1]) > 32  # the hot rounds stall into the sorted walk
    return start, voters, rounds


@pytest.mark.parametrize("compact", [0, 2], ids=["64-byte-results", "32-byte-results"])
@pytest.mark.parametrize("walk", ["lists", "sort"])
@pytest.mark.parametrize("n,self_peer", SHAPES)
def test_random_traffic(S, n, self_peer, walk, compact, monkeypatch):
    if walk == "sort":
        monkeypatch.setenv("RAFTQ_STEP_WALK", "sort")
    else:
        monkeypatch.delenv("RAFTQ_STEP_WALK", raising=False)
    start, voters, rounds = _traffic(n, self_peer)
    with _engine(S, V.copy_state(start), voters) as e:
        e.set_compact(compact)
        for rnd, (m, want, rep, ans, before, mid, after) in enumerate(rounds):
            if compact:
                e.step_submit(m)
                recs, touched = e.step_collect()
                got = S.expand_short(m, recs, *before)
            else:
                got, touched = e.step_batch(m)
            assert touched == len(np.unique(m["group"]))
            _same_records(got, want, m, (n, walk, compact, rnd))
            _stepgen.assert_same_state(e, mid)
            assert np.array_equal(e.apply_log_deltas(*rep), ans), rnd
            _stepgen.assert_same_state(e, after)


def test_three_batches_in_flight_with_a_stalled_one(S):
    """three deep, the batch with a run longer than 32 second of three: nothing of it nor of the third is applied by the list
    walk; the collect replays both, in order, through step_voters_kernel"""
    n, me, g = 5, 4, 777
    rng = np.random.default_rng(8700)
    s, voters = _leaky_state(rng, g, n, me)
    with _engine(S, V.copy_state(s), voters) as e:
        for trip in range(3):
            batches = [_stepgen.random_batch(rng, s, 600) for _ in range(3)]
            batches[1]["group"][:40] = 21 + trip
            want = []
            for m in batches:
                want.append(V.step_batch(s, voters, m))
            for m in batches:
                e.step_submit(m)
            assert _code(e.set_step_voters, False)[0] == RAFTQ_ESTATE  # a batch in flight
            for m, w in zip(batches, want):
                got, touched = e.step_collect()
                _same_records(got, w, m, trip)
                assert touched == len(np.unique(m["group"]))
            _stepgen.assert_same_state(e, s)


def test_a_conf_change_between_batches(S):
    n, me, g = 5, 0, 777
    rng = np.random.default_rng(8800)
    s, voters = _leaky_state(rng, g, n, me)
    with _engine(S, V.copy_state(s), voters) as e:
        for rnd in range(3):
            m = _stepgen.random_batch(rng, s, 3000)
            _same_records(e.step_batch(m)[0], V.step_batch(s, voters, m), m, rnd)
            # a replica leaves some groups; in others a slot is reused (added as a voter, its Match and vote reset) -- on led and
            # on campaigning groups among them
            led, cand = np.flatnonzero(s.role == 2), np.flatnonzero(s.role == 1)
            assert len(led) > 20 and len(cand) > 20
            grp = np.concatenate([led[:60], cand[:60], rng.integers(0, g, 60)]).astype(np.uint64)
            slot = rng.integers(0, n, len(grp))
            gone = rng.random(len(grp)) < 0.5
            new = np.where(gone, voters[grp] & ~(1 << slot), voters[grp] | (1 << slot)).astype(np.uint16)
            reset = np.where(gone, 0, 1 << slot).astype(np.uint16)
            e.apply_voter_deltas(e.pack_voter_deltas(grp, new, reset))
            s.match[:], s.votes[:], voters = RV.apply_voter_deltas(s.match, s.votes, voters, grp, new, reset)
            assert np.array_equal(e.read_voters(), voters)
            _stepgen.assert_same_state(e, s)
        for rnd in range(2):
            m = _stepgen.random_batch(rng, s, 3000)
            _same_records(e.step_batch(m)[0], V.step_batch(s, voters, m), m, rnd)
            _stepgen.assert_same_state(e, s)


@pytest.mark.parametrize("n,self_peer", [(1, 0), (3, 1), (9, 8)])
def test_one_voter_groups(S, n, self_peer):
    g = 129
    rng = np.random.default_rng(8900 + n)
    s = _stepgen.random_state(rng, g, n, self_peer)
    voters = np.full(g, 1 << self_peer, np.uint16)
    led, fol = np.flatnonzero(s.role == 2), np.flatnonzero(s.role == 0)
    assert len(led) > 10 and len(fol) > 10
    with _engine(S, V.copy_state(s), voters) as e:
        # a leader that is its group's only voter commits on its own append: the tail report alone
        tail = s.last_index[led] + 3
        want = V.apply_log_deltas(s, voters, led, tail, s.term[led])
        assert np.array_equal(want, tail)  # (first_idx <= the tail: random_state's leaders hold an entry of their term)
        assert np.array_equal(e.apply_log_deltas(led, tail, s.term[led]), want)
        _stepgen.assert_same_state(e, s)
        # a follower's MsgHup: its own grant is the quorum, and becomeLeader's empty entry commits at once
        m = S.pack_msgs(fol.astype(np.uint64), S.MSG_HUP)
        want = V.step_batch(s, voters, m)
        assert (want["type"] == S.OUT_BECAME_LEADER).all() and np.array_equal(want["commit"], want["last_index"])
        _same_records(e.step_batch(m)[0], want, m)
        _stepgen.assert_same_state(e, s)


def test_step_and_sweep_are_one_function(S):
    """after a masked batch the masked sweep -- the other statement of maybeCommit / poll over the voters -- finds nothing left to
    advance; from a state swept once, as tests/test_step_gpu.py::test_step_then_dense_sweep_agree"""
    n, me = 5, 0
    rng = np.random.default_rng(9000)
    s, voters = _leaky_state(rng, G0, n, me)
    with _engine(S, V.copy_state(s), voters) as e:
        e.sweep(SWEEP_COMMIT | SWEEP_GATED)
        s.committed[:] = RV.commit_advance(s.match, s.committed, voters, True, s.first_idx)[0]
        for rnd in range(3):
            m = _stepgen.random_batch(rng, s, 12000)
            _same_records(e.step_batch(m)[0], V.step_batch(s, voters, m), m, rnd)
            c = e.sweep(SWEEP_COMMIT | SWEEP_GATED | SWEEP_VOTES)
            assert c.n_changed == 0, rnd
            _stepgen.assert_same_state(e, s)
            assert np.array_equal(e.read_outcome(), RV.vote_tally(s.votes, voters)[0])
            rep = _tail_reports(rng, s)
            assert np.array_equal(e.apply_log_deltas(*rep), V.apply_log_deltas(s, voters, *rep))
            assert e.sweep(SWEEP_COMMIT | SWEEP_GATED).n_changed == 0


# ---- frames ------------------------------------------------------------------------------------------------------------------
def _payload_free_frames(rng, e, s, k):
    """k payload-free messages addressed to this node, marshalled by the library's own encoder -> (wire records, stream, offsets)"""
    from oracle import pywire as W

    w = np.zeros(k, W.WIRE_MSG_DT)
    g = rng.integers(0, s.G, k)
    w["group"], w["type"] = g, rng.choice([4, 5, 6, 8, 9], k)
    w["term"] = np.maximum(1, s.term[g].astype(np.int64) + rng.choice([-1, 0, 0, 0, 1], k)).astype(np.uint64)
    w["from"], w["to"] = (s.self_peer + 1 + rng.integers(0, s.N - 1, k)) % s.N, s.self_peer
    li = s.last_index[g].astype(np.int64)
    w["index"] = np.maximum(0, li + rng.integers(-2, 3, k)).astype(np.uint64)
    w["commit"] = np.maximum(0, li + rng.integers(-3, 3, k)).astype(np.uint64)
    w["reject"] = rng.random(k) < 0.2
    resp = w["type"] == 4
    w["log_term"] = np.where(resp, 0, np.maximum(0, s.last_term[g].astype(np.int64) + rng.integers(-1, 2, k))).astype(np.uint64)
    w["reject_hint"] = np.where(resp, w["index"], 0)
    stream, off = e.wire_encode(w)
    return w, stream, off


def test_step_frames_on_a_masked_handle(S):
    from oracle import pywire as W
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from raftsql_amd.wire import WireEngine

    n, me, g = 5, 2, 129
    rng = np.random.default_rng(9100)
    s, voters = _leaky_state(rng, g, n, me)
    with _engine(S, V.copy_state(s), voters, cls=WireEngine) as a, _engine(S, V.copy_state(s), voters) as b:
        for rnd in range(3):
            w, stream, off = _payload_free_frames(rng, a, s, 700)
            m = np.zeros(len(w), S.MSG_DT)
            for k in ("group", "term", "log_term", "index", "commit", "reject_hint", "from", "type", "reject"):
                m[k] = w[k]
            m["_pad"][:, 0] = w["to"]
            msgs = pinned_empty(len(w), W.WIRE_MSG_DT)
            _, _, outs, c = a.step_frames(pinned_copy(np.ascontiguousarray(stream)), pinned_copy(np.ascontiguousarray(off, np.uint64)), msgs)
            assert (c.n_msgs, c.n_malformed) == (len(w), 0)
            got_b, _ = b.step_batch(m)
            _same_records(outs, got_b, m, rnd)
            _same_records(outs, V.step_batch(s, voters, m), m, rnd)
            _stepgen.assert_same_state(a, s)
            _stepgen.assert_same_state(b, s)


# ---- the switch ----------------------------------------------------------------------------------------------------------------
def test_switch_semantics(S, oracle):
    from oracle import pywire as W
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from raftsql_amd.wire import PROP_DT, PROP_ENT_DT, WireEngine

    n, me, g = 5, 1, 700
    rng = np.random.default_rng(9200)
    s, voters = _leaky_state(rng, g, n, me)
    m = _stepgen.random_batch(rng, s, 500)
    with _engine(S, V.copy_state(s), voters, on=False, cls=WireEngine) as e:
        # masks loaded, switch off: refused as ever, texts included
        rc, msg = _code(e.step_batch, m)
        assert rc == RAFTQ_ESTATE and "voter masks" in msg
        rc, msg = _code(e.step_submit, m)
        assert rc == RAFTQ_ESTATE and "voter masks" in msg
        rc, msg = _code(e.apply_log_deltas, [0], [1], [1])
        assert rc == RAFTQ_ESTATE and "voter masks" in msg
        assert _code(e.apply_log_deltas_nowait, [0], [1], [1])[0] == RAFTQ_ESTATE
        assert _code(e.set_step_voters, 2)[0] == RAFTQ_EINVAL
        assert _code(e.set_step_voters, -1)[0] == RAFTQ_EINVAL
        _stepgen.assert_same_state(e, s)  # nothing was applied
        # switch on: through, over the voters
        e.set_step_voters(True)
        _same_records(e.step_batch(m)[0], V.step_batch(s, voters, m), m)
        e.step_submit(m)
        assert _code(e.set_step_voters, True)[0] == RAFTQ_ESTATE  # a batch in flight
        _same_records(e.step_collect()[0], V.step_batch(s, voters, m), m)
        # the calls that build a broadcast on the device stay refused
        cap = e.respond_cap(g)
        out, off, po = pinned_empty(cap + 16, np.uint8), pinned_empty(g * (n - 1) + 1, np.uint64), pinned_empty(2 * (n + 1), np.uint64)
        rc, msg = _code(e.tick_frames, out, off, po, g)
        assert rc == RAFTQ_ESTATE and "voter masks" in msg
        camp = pinned_empty(4, S.OUT_S_DT)
        rc, msg = _code(e.tick_elect_frames, camp, out, None, po, 4, 4)
        assert rc == RAFTQ_ESTATE and "voter masks" in msg
        w, stream, foff = _payload_free_frames(rng, e, s, 50)
        ps, pf = pinned_copy(np.ascontiguousarray(stream)), pinned_copy(np.ascontiguousarray(foff, np.uint64))
        rc, msg = _code(e.step_frames_respond, ps, pf, pinned_empty(50, W.WIRE_MSG_DT), None, None, out, None, po)
        assert rc == RAFTQ_ESTATE and "voter masks" in msg
        props, pents = pinned_empty(1, PROP_DT), pinned_empty(1, PROP_ENT_DT)
        props[0], pents[0] = (int(np.flatnonzero(s.role == 2)[0]), 0, 1), (0, 4, 0)
        rc, msg = _code(e.propose_frames, props, pents, np.zeros(0, W.WIRE_MSG_DT), np.zeros(0, W.WIRE_ENT_DT), pinned_copy(np.zeros(16, np.uint8)), out)
        assert rc == RAFTQ_ESTATE and "voter masks" in msg
        _stepgen.assert_same_state(e, s)  # none of them ticked, campaigned, stepped or appended
        # switch on and the masks dropped: exactly the unmasked handle -- the C oracle's records -- and the switch is still on
        e.load_voters(None)
        m2 = _stepgen.random_batch(rng, s, 500)
        _same_records(e.step_batch(m2)[0], s.step_batch(m2), m2)
        _stepgen.assert_same_state(e, s)
        e.load_voters(voters)
        m3 = _stepgen.random_batch(rng, s, 500)
        _same_records(e.step_batch(m3)[0], V.step_batch(s, voters, m3), m3)
        # clone_state_from carries the masks and leaves the destination's switch as it was
        with S.NodeEngine(g, n, me) as off_dst, S.NodeEngine(g, n, me) as on_dst:
            on_dst.set_step_voters(True)
            for d in (off_dst, on_dst):
                _stepgen.load_engine(d, s)  # (the node fields are not part of the quorum state a clone copies)
                d.clone_state_from(e)
                assert np.array_equal(d.read_voters(), voters)
            rc, msg = _code(off_dst.step_batch, m3)
            assert rc == RAFTQ_ESTATE and "voter masks" in msg
            ref = V.copy_state(s)
            _same_records(on_dst.step_batch(m3)[0], V.step_batch(ref, voters, m3), m3)
