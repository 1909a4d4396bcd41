"""GPU: the narrow word and its mirror (raftq_kernels.hpp kNarrowValid).  While the device knows
match[p][g] == anchor[g] + offset[p][g] everywhere, a commit sweep of three or more peers reads the 32-bit mirror instead
of the rows.  One case per writer: each sets the word, keeps it or ends it, and reads it back with raftq_narrow -- that
shows which body the sweeps took.  Then every dispatch is held equal to the oracle, whole arrays: one handle plain and
gated, a set (grid and persistent walk) that mixes a member with a valid word and one without, and a segmented
raftq_cycle_packed turn; commit indices, the changed bitmap, the tallies and the vote outcomes.

G = 4,099: two full 2,048-group tiles and a ragged third (three full 1,024-group tiles, a fourth and a ragged fifth for the
one-handle and segmented shapes).  N = 1 and 2 have no narrow body (the word is built all the same); 3, 5, 7, 9 run the
networks of every size class and both sides of the self-row-skip rule.  Every input is in range."""
import os

import numpy as np
import pytest

from raftsql_amd import synth
from raftsql_amd._lib import (CYCLE_SEGMENTED, CYCLE_TRUSTED, SET_GRID, SET_PERSISTENT, SWEEP_CHANGED, SWEEP_COMMIT, SWEEP_GATED,
                              SWEEP_NO_ADOPT, SWEEP_VOTES)
from raftsql_amd.engine import SweepSet

pytestmark = pytest.mark.gpu

G = 4099
PEERS = (1, 2, 3, 5, 7, 9)
SPAN = 1 << 32


def _state(n, seed):
    return synth.make_groups(G, n, seed=seed, with_terms=True)


def _wide(n, seed):
    """a state one of whose groups spreads over 2^32 (from two peers on): no mirror can stand for it"""
    st = _state(n, seed)
    if n >= 2:
        st.match[0, 2049] = st.match[n - 1, 2049] + np.uint64(SPAN)
    return st


def _loaded(E, st):
    e = E(st.n_groups, st.n_peers)
    e.load_state(st)
    return e


def _ref(st):
    return [st.match.copy(), st.committed.copy(), st.first_idx_cur_term.copy(), st.votes.copy()]


def _check(oracle, es, refs):
    """refs[k] = [match, committed, first_idx, votes] of member k as it stands.  Every dispatch leaves that state as it was
    (NO_ADOPT) except the segmented turn at the end, which adopts; refs are updated to match."""
    want = [{g: oracle.commit_advance(m, c, g, f) for g in (False, True)} for m, c, f, _ in refs]
    tally = [oracle.vote_tally(v) for _, _, _, v in refs]
    for e, w, t, r in zip(es, want, tally, refs):
        for gated in (False, True):
            c = e.sweep(SWEEP_COMMIT | SWEEP_VOTES | SWEEP_CHANGED | (SWEEP_GATED if gated else 0) | SWEEP_NO_ADOPT)
            assert np.array_equal(e.read_committed(), w[gated][0])
            assert (c.n_changed, c.n_won, c.n_lost) == (w[gated][1], t[1], t[2])
            assert np.array_equal(e.read_outcome(), t[0])
            adv, n_adv = e.collect_changed()
            moved = np.nonzero(w[gated][0] != r[1])[0]
            assert n_adv == len(moved) and np.array_equal(adv["group"], moved.astype(np.uint64))
            assert np.array_equal(adv["old_commit"], r[1][moved]) and np.array_equal(adv["new_commit"], w[gated][0][moved])
    with SweepSet(es) as s:
        for mode, wgs in ((SET_GRID, 0), (SET_PERSISTENT, 3)):
            s.set_mode(mode, wgs)
            for gated in (False, True):
                per, _ = s.sweep(SWEEP_COMMIT | SWEEP_VOTES | SWEEP_CHANGED | (SWEEP_GATED if gated else 0) | SWEEP_NO_ADOPT)
                for e, w, t, r, c in zip(es, want, tally, refs, per):
                    assert np.array_equal(e.read_committed(), w[gated][0]), (mode, gated)
                    assert (c.n_changed, c.n_won, c.n_lost) == (w[gated][1], t[1], t[2]), (mode, gated)
                    assert np.array_equal(e.read_outcome(), t[0])
                    adv, n_adv = e.collect_changed()
                    moved = np.nonzero(w[gated][0] != r[1])[0]
                    assert n_adv == len(moved) and np.array_equal(adv["group"], moved.astype(np.uint64)), (mode, gated)
    for k, (e, w) in enumerate(zip(es, want)):
        gated = k % 2 == 1
        m, c, f, v = refs[k]
        d, _ = e.stage_packed(1, 0)
        d[:] = e.pack_deltas16(np.array([0], np.uint64), np.array([0], np.uint32), m[0, :1])  # a record that moves nothing
        _, total, _ = e.cycle_packed(SWEEP_COMMIT | (SWEEP_GATED if gated else 0) | CYCLE_SEGMENTED, d, None, cap=G, inplace=True,
                                     want_counts=False)
        _, counts, _ = e.last_advance_segments()
        assert len(counts) > 1, "the turn did not take the segmented form"
        assert total == w[gated][1] == int(counts.sum())
        assert np.array_equal(e.read_committed(), w[gated][0])
        listed = e.advance_list_from_segments()
        moved = np.nonzero(w[gated][0] != c)[0]
        assert np.array_equal(listed["group"].astype(np.int64), moved) and np.array_equal(listed["new_commit"], w[gated][0][moved])
        refs[k][1] = w[gated][0]


def _pair(E, oracle, e, ref, n, seed):
    """`e` with a companion whose word is the other way round: the set then mixes members with and without a valid word"""
    other = _state(n, seed) if not e.narrow() else _wide(n, seed)
    with _loaded(E, other) as o:
        if n >= 2:
            assert o.narrow() != e.narrow()
        _check(oracle, [e, o], [ref, _ref(other)])


@pytest.mark.parametrize("n", PEERS)
def test_load_builds_the_mirror(gpu_engine_cls, oracle, n):
    st = _state(n, 11000 + n)
    with gpu_engine_cls(G, n) as e:
        assert not e.narrow()  # raftq_create: no mirror yet
        e.load_state(st)
        assert e.narrow() and e.self_max() == 0
        ref = _ref(st)
        _pair(gpu_engine_cls, oracle, e, ref, n, 11050 + n)
        assert e.narrow()  # sweeps and a turn whose record moves nothing keep it
        if n >= 2:  # loaded again with one group too wide: no mirror; and restored: a mirror again
            e.load_state(_wide(n, 11000 + n))
            assert not e.narrow()
            e.load_state(st)
            assert e.narrow()


@pytest.mark.parametrize("n", PEERS)
def test_adversarial_block_has_no_mirror(gpu_engine_cls, oracle, n):
    st = synth.concat(synth.make_groups(G - synth.adversarial_block(n).n_groups, n, seed=11100 + n, with_terms=True),
                      synth.adversarial_block(n))
    assert st.n_groups == G
    with _loaded(gpu_engine_cls, st) as e:
        assert e.narrow() == (n == 1)  # its 0-and-UINT64_MAX groups
        _pair(gpu_engine_cls, oracle, e, _ref(st), n, 11150 + n)


@pytest.mark.parametrize("n", PEERS)
def test_rebuild(gpu_engine_cls, oracle, n):
    """the build pass on demand, after a writer that ended the mirror: an ack far above its group, then one that closes the gap"""
    st = _state(n, 11200 + n)
    with _loaded(gpu_engine_cls, st) as e:
        ref = _ref(st)
        g, p = np.array([4098], np.uint64), np.array([n - 1], np.uint32)
        far = st.match.max(axis=0)[4098] + np.uint64(SPAN + 5)  # 2^32 above every other value of the group
        e.apply_deltas(g, p, np.array([far], np.uint64))
        ref[0] = oracle.apply_deltas(ref[0], g, p, np.array([far], np.uint64))
        assert not e.narrow()
        assert e.narrow_rebuild() == (n == 1)  # the group is still too wide (one peer: never)
        if n >= 2:
            allp = np.arange(n, dtype=np.uint32)
            e.apply_deltas(np.full(n, 4098, np.uint64), allp, np.full(n, far, np.uint64))
            ref[0] = oracle.apply_deltas(ref[0], np.full(n, 4098, np.uint64), allp, np.full(n, far, np.uint64))
            assert not e.narrow()  # nothing but a build pass sets the word
        assert e.narrow_rebuild()
        assert np.array_equal(e.read_match(), ref[0])
        _pair(gpu_engine_cls, oracle, e, ref, n, 11250 + n)


@pytest.mark.parametrize("n", PEERS)
def test_clone_carries_the_mirror(gpu_engine_cls, oracle, n):
    good, bad = _state(n, 11300 + n), _wide(n, 11350 + n)
    with _loaded(gpu_engine_cls, good) as a, _loaded(gpu_engine_cls, bad) as b, gpu_engine_cls(G, n) as d1, gpu_engine_cls(G, n) as d2:
        assert (a.narrow(), b.narrow(), d1.narrow(), d2.narrow()) == (True, n == 1, False, False)
        d1.clone_state_from(a)  # a destination that never had a mirror gets the source's
        assert d1.narrow()
        d2.load_state(good)
        d2.clone_state_from(b)  # one that had its own loses it with the rows
        assert d2.narrow() == (n == 1)
        _check(oracle, [d1, d2], [_ref(good), _ref(bad)])


@pytest.mark.parametrize("trusted", [False, True], ids=["validated", "trusted"])
@pytest.mark.parametrize("n", PEERS)
def test_ingest_follows_the_mirror(gpu_engine_cls, oracle, n, trusted):
    """four records, one group each: below the anchor, equal to the current value, at anchor + 2^32 - 1 (the largest offset:
    the word stays), and -- in a second batch -- at anchor + 2^32 (the word is cleared)"""
    st = _state(n, 11400 + n)
    anchor = st.match.min(axis=0)

    def ingest(e, g, p, v):
        if trusted:
            d, _ = e.stage_packed(len(g), 0)
            d[:] = e.pack_deltas16(g, p, v)
            e.cycle_packed(SWEEP_COMMIT | SWEEP_NO_ADOPT | CYCLE_TRUSTED, d, None, cap=G, inplace=True, want_counts=False)
        else:
            e.apply_deltas(g, p, v)

    with _loaded(gpu_engine_cls, st) as e:
        ref = _ref(st)
        g = np.array([5, 2047, 2048], np.uint64)
        p = np.array([0, n - 1, n // 2], np.uint32)
        v = np.array([anchor[5] - np.uint64(1), st.match[n - 1, 2047], anchor[2048] + np.uint64(SPAN - 1)], np.uint64)
        ingest(e, g, p, v)
        ref[0] = oracle.apply_deltas(ref[0], g, p, v)
        assert e.narrow()
        assert np.array_equal(e.read_match(), ref[0])
        _pair(gpu_engine_cls, oracle, e, ref, n, 11450 + n)
        assert e.narrow()
        g, p, v = np.array([4098], np.uint64), np.array([0], np.uint32), np.array([anchor[4098] + np.uint64(SPAN)], np.uint64)
        ingest(e, g, p, v)
        ref[0] = oracle.apply_deltas(ref[0], g, p, v)
        assert not e.narrow()
        assert np.array_equal(e.read_match(), ref[0])
        _pair(gpu_engine_cls, oracle, e, ref, n, 11460 + n)


@pytest.mark.parametrize("n", PEERS)
def test_ingest_keeps_a_busy_mirror_true(gpu_engine_cls, oracle, n):
    """a batch with many records per slot (the 32-bit maximum must land where the 64-bit one does), then the narrow sweeps"""
    st = _state(n, 11500 + n)
    rng = np.random.default_rng(11500 + n)
    with _loaded(gpu_engine_cls, st) as e:
        ref = _ref(st)
        g = rng.integers(0, G, 6000).astype(np.uint64)
        g[:600] = 4098
        p = rng.integers(0, n, 6000).astype(np.uint32)
        v = np.maximum(st.match[p, g].astype(np.int64) + rng.integers(-2500, 2500, 6000), 0).astype(np.uint64)
        e.apply_deltas(g, p, v)
        ref[0] = oracle.apply_deltas(ref[0], g, p, v)
        assert e.narrow() and np.array_equal(e.read_match(), ref[0])
        _pair(gpu_engine_cls, oracle, e, ref, n, 11550 + n)


@pytest.mark.parametrize("n", PEERS)
def test_step_that_stores_a_match_row_ends_the_mirror(gpu_engine_cls, oracle, n):
    from raftsql_amd.step import MSG_APP_RESP, ROLE_LEADER, NodeEngine, pack_msgs

    st = _state(n, 11600 + n)
    st.match[:] = np.minimum(st.match, np.uint64(10))
    st.match[0] = 10
    st.committed[:] = 0
    term, first = np.full(G, 3, np.uint64), np.full(G, 1, np.uint64)
    with NodeEngine(G, n) as e:
        e.load_match(st.match, st.committed)
        e.load_votes(st.votes)
        e.load_terms(term, first)
        e.load_roles(np.full(G, ROLE_LEADER, np.uint8))
        e.load_node(term=term, last_index=np.full(G, 100, np.uint64), last_term=term)
        assert e.narrow()
        if n >= 2:
            e.step_batch(pack_msgs(np.array([9], np.uint64), MSG_APP_RESP, term=3, frm=1, index=int(st.match[1, 9])))  # stores no row
            assert e.narrow()
            e.step_batch(pack_msgs(np.array([7], np.uint64), MSG_APP_RESP, term=3, frm=1, index=50))
            assert not e.narrow()
            assert e.read_match()[1, 7] == 50
        node = e.read_node()
        ref = [e.read_match(), node["committed"], node["first_idx"], st.votes.copy()]
        _pair(gpu_engine_cls, oracle, e, ref, n, 11650 + n)
        assert e.narrow_rebuild()
        _pair(gpu_engine_cls, oracle, e, ref, n, 11660 + n)


@pytest.mark.parametrize("n", PEERS)
def test_voter_delta_with_a_reset_ends_the_mirror(gpu_engine_cls, oracle, n):
    st = _state(n, 11700 + n)
    full = (1 << n) - 1
    with _loaded(gpu_engine_cls, st) as e:
        ref = _ref(st)
        e.apply_voter_deltas(e.pack_voter_deltas([3], [full], [0]))  # a new mask, no slot reset: the rows stand
        assert e.narrow()
        e.apply_voter_deltas(e.pack_voter_deltas([2050], [full], [1 << (n - 1)]))
        assert not e.narrow()
        ref[0][n - 1, 2050] = 0
        ref[3][n - 1, 2050] = 0
        assert np.array_equal(e.read_match(), ref[0])
        e.load_voters(None)  # every slot votes again: the unmasked dispatches, over the rows
        _pair(gpu_engine_cls, oracle, e, ref, n, 11750 + n)


@pytest.mark.parametrize("n", PEERS)
def test_raftq_narrow_0_never_builds(gpu_engine_cls, oracle, n, monkeypatch):
    st = _state(n, 11800 + n)
    monkeypatch.setenv("RAFTQ_NARROW", "0")
    with gpu_engine_cls(G, n) as e, gpu_engine_cls(G, n) as d:
        monkeypatch.delenv("RAFTQ_NARROW")  # read once, at raftq_create
        e.load_state(st)
        assert not e.narrow() and not e.narrow_rebuild()
        with _loaded(gpu_engine_cls, st) as src:
            assert src.narrow()
            d.clone_state_from(src)
            assert not d.narrow()
        _check(oracle, [e, d], [_ref(st), _ref(st)])
    assert "RAFTQ_NARROW" not in os.environ


@pytest.mark.parametrize("n", PEERS)
def test_self_max_clear_and_narrow_valid_and_the_reverse(gpu_engine_cls, oracle, n):
    """the two words are independent: a follower one above its leader ends the self-row skip and leaves the mirror, a group
    2^32 wide whose leader holds the maximum does the reverse"""
    a_st = _state(n, 11900 + n)
    if n >= 2:
        a_st.match[n - 1, 1000] = a_st.match[0, 1000] + np.uint64(1)
    b_st = _wide(n, 11950 + n)  # (_wide raises slot 0, the self row)
    with _loaded(gpu_engine_cls, a_st) as a, _loaded(gpu_engine_cls, b_st) as b:
        assert (a.self_max(), a.narrow()) == (-1 if n >= 2 else 0, True)
        assert (b.self_max(), b.narrow()) == (0, n == 1)
        _check(oracle, [a, b], [_ref(a_st), _ref(b_st)])
        assert (a.self_max(), a.narrow()) == (-1 if n >= 2 else 0, True)
        assert (b.self_max(), b.narrow()) == (0, n == 1)


@pytest.mark.parametrize("n", (3, 5))
def test_mirror_built_under_a_set(gpu_engine_cls, oracle, n):
    """members that get their mirror only after the set was created: the set's tables name the new arrays"""
    sts = [_state(n, 12000 + 10 * n + k) for k in range(3)]
    es = [gpu_engine_cls(G, n) for _ in sts]
    try:
        with SweepSet(es) as s:
            for e, st in zip(es, sts):
                e.load_state(st)
            assert all(e.narrow() for e in es)
            per, _ = s.sweep(SWEEP_COMMIT | SWEEP_VOTES | SWEEP_NO_ADOPT)
            for e, st, c in zip(es, sts, per):
                w, nw = oracle.commit_advance(st.match, st.committed, False, st.first_idx_cur_term)
                assert np.array_equal(e.read_committed(), w) and c.n_changed == nw
    finally:
        for e in es:
            e.close()
