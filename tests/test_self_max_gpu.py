"""GPU: the self-max word (raftq_kernels.hpp).  While the device knows the self row to be every group's
largest, the commit sweep does not read it.  Each case sets the word, or breaks the fact, through a different writer
and checks the word with raftq_self_max: that shows which path the sweeps took.  Then every dispatch is held equal to
the oracle, whole arrays: one handle, a set as a K-deep grid, a set as a persistent walk, and the batching turn's
segmented sweep.  Each runs gated and ungated, for N = 1..9."""
import numpy as np
import pytest

from raftsql_amd import synth
from raftsql_amd._lib import CYCLE_SEGMENTED, SET_GRID, SET_PERSISTENT, SWEEP_COMMIT, SWEEP_GATED, SWEEP_NO_ADOPT, SWEEP_VOTES
from raftsql_amd.engine import SweepSet

pytestmark = pytest.mark.gpu

G = 5000  # > one 2048-group tile: several tiles per member, and the segmented turn has several segments
MULTI = range(2, 10)  # q >= 2: the peer counts whose sweep can leave a row out


def _state(n, seed):
    return synth.make_groups(G, n, seed=seed, with_terms=True)


def _loaded(E, st):
    e = E(st.n_groups, st.n_peers)
    e.load_state(st)
    return e


def _check(oracle, es, refs):
    """refs[k] = (match, committed, first_idx) of member k as it stands.  Every dispatch leaves that state as it was
    (NO_ADOPT) except the segmented turn at the end, which adopts; refs are updated to match."""
    want = [{g: oracle.commit_advance(m, c, g, f) for g in (False, True)} for m, c, f in refs]
    for e, w in zip(es, want):
        for gated in (False, True):
            c = e.sweep(SWEEP_COMMIT | (SWEEP_GATED if gated else 0) | SWEEP_NO_ADOPT)
            assert np.array_equal(e.read_committed(), w[gated][0]) and c.n_changed == w[gated][1]
    with SweepSet(es) as s:
        for mode, wgs in ((SET_GRID, 0), (SET_PERSISTENT, 3)):
            s.set_mode(mode, wgs)
            for gated in (False, True):
                per, _ = s.sweep(SWEEP_COMMIT | SWEEP_VOTES | (SWEEP_GATED if gated else 0) | SWEEP_NO_ADOPT)
                for e, w, c in zip(es, want, per):
                    assert np.array_equal(e.read_committed(), w[gated][0]) and c.n_changed == w[gated][1], (mode, gated)
    for k, (e, w) in enumerate(zip(es, want)):
        gated = k % 2 == 1
        m, c, f = refs[k]
        d, _ = e.stage_packed(1, 0)
        d[:] = e.pack_deltas16(np.array([0], np.uint64), np.array([0], np.uint32), m[0, :1])  # a record that moves nothing
        _, total, _ = e.cycle_packed(SWEEP_COMMIT | (SWEEP_GATED if gated else 0) | CYCLE_SEGMENTED, d, None, cap=G, inplace=True,
                                     want_counts=False)
        recs, counts, _ = e.last_advance_segments()
        assert len(counts) > 1, "the turn did not take the segmented form"
        assert total == w[gated][1] == int(counts.sum())
        assert np.array_equal(e.read_committed(), w[gated][0])
        refs[k] = (m, w[gated][0], f)


def _ref(st):
    return (st.match.copy(), st.committed.copy(), st.first_idx_cur_term.copy())


@pytest.mark.parametrize("n", range(1, 10))
def test_flag_is_set_on_synth_state(gpu_engine_cls, oracle, n):
    st = _state(n, 9500 + n)
    assert (st.match[0] == st.match.max(axis=0)).all()  # slot 0 is the leader's: the row maximum
    with _loaded(gpu_engine_cls, st) as e:
        assert e.self_max() == 0
        refs = [_ref(st)]
        _check(oracle, [e], refs)
        assert e.self_max() == 0


@pytest.mark.parametrize("n", MULTI)
def test_one_group_against_the_fact_keeps_the_flag_clear(gpu_engine_cls, oracle, n):
    st = _state(n, 9600 + n)
    st.match[n - 1, 4321] = st.match[0, 4321] + 1
    with _loaded(gpu_engine_cls, st) as e:
        assert e.self_max() == -1
        _check(oracle, [e], [_ref(st)])
        # loaded again with the fact restored: set again
        st.match[n - 1, 4321] = st.match[0, 4321]
        e.load_state(st)
        assert e.self_max() == 0
        _check(oracle, [e], [_ref(st)])


@pytest.mark.parametrize("n", MULTI)
def test_ingested_follower_delta_above_self_clears(gpu_engine_cls, oracle, n):
    """raftq_apply_deltas (staged, validated) and a trusted packed turn (validated and applied in one kernel)"""
    from raftsql_amd._lib import CYCLE_TRUSTED

    st = _state(n, 9700 + n)
    with _loaded(gpu_engine_cls, st) as a, _loaded(gpu_engine_cls, st) as b:
        ref = _ref(st)
        g = np.array([17, 2222, 4999], np.uint64)
        p = np.array([1, n - 1, 1], np.uint32)
        v = st.match[0, g] + np.array([0, 0, 3], np.uint64)  # only the last record goes above its group's self row
        a.apply_deltas(g, p, v)
        assert a.self_max() == -1
        d, _ = b.stage_packed(3, 0)
        d[:] = b.pack_deltas16(g, p, v)
        b.cycle_packed(SWEEP_COMMIT | SWEEP_NO_ADOPT | CYCLE_TRUSTED, d, None, cap=G, inplace=True, want_counts=False)
        assert b.self_max() == -1
        m = oracle.apply_deltas(ref[0], g, p, v)
        assert np.array_equal(a.read_match(), m) and np.array_equal(b.read_match(), m)
        _check(oracle, [a, b], [(m, ref[1], ref[2]), (m.copy(), ref[1].copy(), ref[2])])


@pytest.mark.parametrize("n", MULTI)
def test_follower_delta_equal_to_self_keeps_the_flag(gpu_engine_cls, oracle, n):
    from raftsql_amd._lib import CYCLE_TRUSTED

    st = _state(n, 9800 + n)
    rng = np.random.default_rng(9800 + n)
    with _loaded(gpu_engine_cls, st) as a, _loaded(gpu_engine_cls, st) as b:
        ref = _ref(st)
        g = rng.integers(0, G, 3000).astype(np.uint64)
        p = rng.integers(1, n, 3000).astype(np.uint32)
        # followers catch up to their leader (equal, never above), leaders move on in the same batch
        g2 = rng.integers(0, G, 500).astype(np.uint64)
        gs = np.concatenate([g, g2])
        ps = np.concatenate([p, np.zeros(500, np.uint32)])
        vs = np.concatenate([st.match[0, g], st.match[0, g2] + np.uint64(7)])
        a.apply_deltas(gs, ps, vs)
        d, _ = b.stage_packed(len(gs), 0)
        d[:] = b.pack_deltas16(gs, ps, vs)
        b.cycle_packed(SWEEP_COMMIT | SWEEP_NO_ADOPT | CYCLE_TRUSTED, d, None, cap=G, inplace=True, want_counts=False)
        assert a.self_max() == 0 and b.self_max() == 0
        m = oracle.apply_deltas(ref[0], gs, ps, vs)
        assert np.array_equal(a.read_match(), m)
        _check(oracle, [a, b], [(m, ref[1], ref[2]), (m.copy(), ref[1].copy(), ref[2])])
        assert a.self_max() == 0 and b.self_max() == 0


@pytest.mark.parametrize("n", MULTI)
def test_set_self_to_a_slot_that_is_not_the_max(gpu_engine_cls, oracle, n):
    st = _state(n, 9900 + n)
    assert (st.match[1] < st.match.max(axis=0)).any()
    with _loaded(gpu_engine_cls, st) as e:
        e._chk(e._lib.raftq_set_self(e._h, 1))
        assert e.self_max() == -1
        _check(oracle, [e], [_ref(st)])
        e._chk(e._lib.raftq_set_self(e._h, 0))
        assert e.self_max() == 0
        # a slot that IS every group's max, other than 0
        st2 = _state(n, 9950 + n)
        st2.match[[0, n - 1]] = st2.match[[n - 1, 0]]
        e.load_state(st2)
        assert e.self_max() == (0 if (st2.match[0] == st2.match.max(axis=0)).all() else -1)  # the handle's self is slot 0
        e._chk(e._lib.raftq_set_self(e._h, n - 1))
        assert e.self_max() == n - 1
        _check(oracle, [e], [_ref(st2)])


@pytest.mark.parametrize("n", MULTI)
def test_clone_carries_the_flag(gpu_engine_cls, oracle, n):
    good = _state(n, 10000 + n)
    bad = _state(n, 10050 + n)
    bad.match[1, 99] = bad.match[0, 99] + 5
    with _loaded(gpu_engine_cls, good) as g, _loaded(gpu_engine_cls, bad) as b, \
            gpu_engine_cls(G, n) as d1, gpu_engine_cls(G, n) as d2:
        assert (g.self_max(), b.self_max(), d1.self_max(), d2.self_max()) == (0, -1, 0, 0)
        d1.clone_state_from(b)
        assert d1.self_max() == -1
        d2.load_state(bad)
        assert d2.self_max() == -1
        d2.clone_state_from(g)
        assert d2.self_max() == 0
        _check(oracle, [d1, d2], [_ref(bad), _ref(good)])


@pytest.mark.parametrize("n", MULTI)
def test_step_raising_a_follower_above_self_clears(gpu_engine_cls, oracle, n):
    """Step's write-back: a leader whose own Match trails its log (loaded that way) takes a MsgAppResp that puts a follower
    above it.  Another group's ack that stays at or below its leader's Match keeps the flag."""
    from raftsql_amd.step import MSG_APP_RESP, ROLE_LEADER, NodeEngine, pack_msgs

    st = _state(n, 10100 + n)
    st.match[:] = np.minimum(st.match, np.uint64(10))
    st.match[0] = 10
    st.committed[:] = 0
    term = np.full(G, 3, np.uint64)
    first = np.full(G, 1, np.uint64)
    with NodeEngine(G, n) as e:
        e.load_match(st.match, st.committed)
        e.load_terms(term, first)
        e.load_roles(np.full(G, ROLE_LEADER, np.uint8))
        e.load_node(term=term, last_index=np.full(G, 100, np.uint64), last_term=term)
        assert e.self_max() == 0
        keep = pack_msgs(np.array([9], np.uint64), MSG_APP_RESP, term=3, frm=1, index=10)
        e.step_batch(keep)
        assert e.self_max() == 0
        m = e.read_match()
        assert m[1, 9] == 10
        e.step_batch(pack_msgs(np.array([7], np.uint64), MSG_APP_RESP, term=3, frm=1, index=50))
        assert e.self_max() == -1
        m = e.read_match()
        assert m[1, 7] == 50 and m[0, 7] == 10
        node = e.read_node()
        _check(oracle, [e], [(m, node["committed"], node["first_idx"])])


@pytest.mark.parametrize("n", MULTI)
def test_set_mixing_flagged_and_unflagged_members(gpu_engine_cls, oracle, n):
    sts = [_state(n, 10200 + 10 * n + k) for k in range(4)]
    for k in (1, 3):
        sts[k].match[n - 1, 100 * k] = sts[k].match[0, 100 * k] + 1
    es = [_loaded(gpu_engine_cls, st) for st in sts]
    try:
        assert [e.self_max() for e in es] == [0, -1, 0, -1]
        _check(oracle, es, [_ref(st) for st in sts])
    finally:
        for e in es:
            e.close()
