"""GPU: raftq_tick_frames (include/raftq_wire.h) -- raftq_tick_collect_lists plus the heartbeat round the Tick calls for, built on
the device and marshalled by the streaming encoder.

Nothing expected comes from the code under test: the MsgBeat / MsgHup groups are oracle.pyoracle.tick's; that Step(MsgBeat) of
such a group answers RAFTQ_OUT_BCAST_HEARTBEAT, and the term it sends at, are NodeState.step_batch's; the commit rule (etcd's
sendHeartbeat: min(Progress.Match, committed)) is restated below; the bytes are oracle.pywire.wire_encode's.  The Tick half is also
compared with a twin handle driven through raftq_tick_collect_lists."""
import copy
import ctypes as C

import numpy as np
import pytest

from oracle import pywire as W

pytestmark = pytest.mark.gpu

MSG_BEAT, MSG_HEARTBEAT, OUT_BCAST_HEARTBEAT = 1, 8, 6
CANARY = 0xA5
CANARY64 = np.uint64(0xA5A5A5A5A5A5A5A5)
ET, SEED = 10, 0x7157


def _spread(rng, n, lo_bytes=1, hi_bytes=6):
    """values whose varints take lo_bytes .. hi_bytes bytes, every length present"""
    nb = rng.integers(lo_bytes, hi_bytes + 1, n)
    lo = np.where(nb == 1, 1, 2.0 ** (7 * (nb - 1))).astype(np.uint64)
    hi = (2.0 ** (7 * nb)).astype(np.uint64)
    return lo + (rng.random(n) * (hi - lo)).astype(np.uint64)


def make_state(rng, G, N, me, hb, wide64=False):
    """roles of every kind in every 1,024-group block, terms and indices over 1- to 6-byte varints (wide64: 2^62 .. 2^64 - 1),
    match[p] below and above committed; hb > 1: leaders at random points of their heartbeat interval"""
    from oracle import pyoracle

    s = pyoracle.NodeState(G, N, me)
    s.role[:] = rng.choice([0, 1, 2, 2], G)
    for b in range(0, G, 1024):  # every block holds every role (where it has three groups)
        k = min(3, G - b)
        s.role[b:b + k] = [2, 0, 1][:k]
    lead, cand = s.role == 2, s.role == 1
    top = np.uint64(2**64 - 1)
    if wide64:
        big = lambda: np.uint64(2**62) + rng.integers(0, 2**64 - 2**62, G, dtype=np.uint64)  # noqa: E731
        s.term[:], s.committed[:] = big(), big()
        s.term[0], s.committed[0] = top, top - np.uint64(1)
    else:
        s.term[:], s.committed[:] = _spread(rng, G), _spread(rng, G)
    for p in range(N):  # both arms of the min: half of the words below committed, half at or above it
        if wide64:
            below = np.maximum(np.uint64(2**62), s.committed - rng.integers(1, 2**61, G, dtype=np.uint64))
        else:
            below = (s.committed * rng.random(G)).astype(np.uint64)
        above = s.committed + np.minimum(top - s.committed, rng.integers(0, 1000, G).astype(np.uint64))
        s.match[p] = np.where(rng.random(G) < 0.5, below, above)
    s.last_index[:] = np.maximum(s.committed, s.match.max(axis=0))
    s.match[me] = s.last_index
    s.last_term[:] = s.term
    s.first_idx[lead] = 1
    s.vote[:] = np.where(lead | cand, me + 1, rng.integers(0, N + 1, G))
    s.lead[:] = np.where(lead, me + 1, 0)
    s.votes[me, cand] = 1
    s.elapsed[:] = np.where(lead, rng.integers(0, hb, G), rng.integers(0, ET, G))
    return s


def want_frames(st, beats, beat_cap):
    """the heartbeat round of the first beat_cap MsgBeat groups: (wire records peer-major, peer_off)"""
    from raftsql_amd import step as S

    N, me = st.N, st.self_peer
    built = np.asarray(beats[:beat_cap], np.int64)
    # Step(MsgBeat) on each: a leader's bcastHeartbeat, at the group's term (a copy: the oracle's state is not to move)
    outs = copy.deepcopy(st).step_batch(S.pack_msgs(built.astype(np.uint64), MSG_BEAT)) if len(built) else np.zeros(0, S.OUT_DT)
    assert (outs["type"] == OUT_BCAST_HEARTBEAT).all(), "the oracle does not broadcast for a group the Tick flagged MsgBeat"
    recs = []
    for p in range(N):
        if p == me:
            continue
        w = np.zeros(len(built), W.WIRE_MSG_DT)
        w["group"], w["type"], w["to"], w["from"], w["term"] = built, MSG_HEARTBEAT, p, me, outs["term"]
        w["commit"] = np.minimum(st.match[p][built], st.committed[built])  # sendHeartbeat: min(r.prs[to].Match, r.raftLog.committed)
        recs.append(w)
    peer_off = np.zeros(N + 1, np.uint64)
    peer_off[1:] = np.cumsum([0 if p == me else len(built) for p in range(N)])
    return (np.concatenate(recs) if recs else np.zeros(0, W.WIRE_MSG_DT)), peer_off


class Bufs:
    """page-locked out / frame_off / peer_off for one beat_cap, canaries behind what the call may write"""

    def __init__(self, e, beat_cap, frame_off=True):
        from raftsql_amd.engine import pinned_empty

        self.n_max = beat_cap * (e.n_peers - 1)
        self.cap = e.respond_cap(beat_cap)
        self.out = pinned_empty(self.cap + 64, np.uint8)
        self.off = pinned_empty(self.n_max + 1 + 8, np.uint64) if frame_off else None
        self.po = pinned_empty(e.n_peers + 1, np.uint64)
        self.reset()

    def reset(self):
        self.out[:] = CANARY
        self.po[:] = CANARY64
        if self.off is not None:
            self.off[:] = CANARY64

    def canaries_ok(self):
        return bool((self.out[self.cap:] == CANARY).all()) and (self.off is None or bool((self.off[self.n_max + 1:] == CANARY64).all()))


def check_tick(oracle, e, twin, st, tick_no, hb, beat_cap, bitmap, what, frame_off=True):
    """one raftq_tick_frames against the oracle (st.elapsed moves with it) and, when given, the twin's raftq_tick_collect_lists"""
    G, N = st.G, st.N
    el, act, rh, rb = oracle.tick(st.role, st.elapsed, ET, hb, SEED, tick_no)
    st.elapsed[:] = el
    hups, beats = np.nonzero(act == 1)[0].astype(np.uint32), np.nonzero(act == 2)[0].astype(np.uint32)
    want_w, want_po = want_frames(st, beats, beat_cap)
    want_s, want_off = W.wire_encode(want_w) if len(want_w) else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    b = Bufs(e, beat_cap, frame_off)
    got_s, got_off, got_po, c, got_h, nh, second, nb = e.tick_frames(b.out, b.off[: b.n_max + 1] if frame_off else None, b.po, beat_cap,
                                                                     beat_bitmap=bitmap, cap=b.cap)
    assert (nh, nb) == (rh, rb), what
    assert (c.n_msgs, c.n_ents, c.n_malformed, c.bytes) == (len(want_w), 0, 0, len(want_s)), what
    assert np.array_equal(got_po, want_po), (what, got_po, want_po)
    assert bytes(got_s) == bytes(want_s), what
    if frame_off:
        full = np.full(b.n_max + 1, len(want_s), np.uint64)  # entries past the last frame all hold the total
        full[: len(want_off)] = want_off
        assert np.array_equal(b.off[: b.n_max + 1], full), what
    assert b.canaries_ok(), what
    assert np.array_equal(got_h, hups), what
    if bitmap:
        bits = np.unpackbits(second.view(np.uint8), bitorder="little")
        assert len(second) == (G + 63) // 64 and np.array_equal(bits[:G], (act == 2).astype(np.uint8)) and not bits[G:].any(), what
    else:
        assert np.array_equal(second, beats[: min(beat_cap, G)]), what
    got_act, got_el, got_role = e.read_tick()
    assert np.array_equal(got_act, act) and np.array_equal(got_el, el) and np.array_equal(got_role, st.role), what
    if twin is not None:
        t_h, t_nh, t_second, t_nb = twin.tick_collect_lists(None, beat_cap, beat_bitmap=bitmap)
        assert (t_nh, t_nb) == (nh, nb) and np.array_equal(t_h, got_h) and np.array_equal(t_second, second), what
        for a, w in zip(twin.read_tick(), (got_act, got_el, got_role)):
            assert np.array_equal(a, w), what
    return len(beats), len(want_w)


def _pair(G, N, me, st, hb):
    """the engine under test with st loaded, and a twin that only ticks"""
    from raftsql_amd.engine import QuorumEngine
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    e, twin = WireEngine(G, N, me), QuorumEngine(G, N)
    for x in (e, twin):
        x.set_timers(ET, hb, SEED)
    _stepgen.load_engine(e, st)
    twin.load_roles(st.role, st.elapsed)
    return e, twin


@pytest.mark.parametrize("N", [2, 3, 5, 9])
@pytest.mark.parametrize("G", [3149, 129, 1])
def test_heartbeats_match_the_oracle(oracle, N, G):
    """three ticks in a row, heartbeat_tick 1 and 3, both flags values, with and without frame_off"""
    for hb in (1, 3):
        rng = np.random.default_rng(9100 + 16 * N + hb + G)
        me = int(rng.integers(0, N))
        st = make_state(rng, G, N, me, hb)
        e, twin = _pair(G, N, me, st, hb)
        with e, twin:
            seen_beats, seen_partial = 0, False
            for t in range(3):
                nb, nf = check_tick(oracle, e, twin, st, t, hb, G, bitmap=(t + hb) % 2 == 0, what=f"N={N} G={G} hb={hb} tick {t}", frame_off=t != 1)
                assert nf == nb * (N - 1)
                seen_beats += nb
                seen_partial |= 0 < nb < int((st.role == 2).sum())
            assert seen_beats > 0
            assert hb == 1 or G < 100 or seen_partial, "heartbeat_tick 3 was meant to make only some leaders beat"
            # both arms of the min were taken among the leaders
            lead = st.role == 2
            others = [p for p in range(N) if p != me]
            if G > 100:
                assert any((st.match[p][lead] < st.committed[lead]).any() for p in others) and any((st.match[p][lead] > st.committed[lead]).any() for p in others)


def test_sixty_four_bit_terms_and_indices(oracle):
    """terms, match and commit at 2^62 .. 2^64 - 1 (10-byte varints).  If this fails, marshal want_frames' records through
    raftq_wire_encode: that separates the new kernel from the encoder."""
    G, N, me, hb = 300, 3, 1, 1
    rng = np.random.default_rng(9200)
    st = make_state(rng, G, N, me, hb, wide64=True)
    assert int(st.term.min()) >= 2**62 and int(st.term.max()) == 2**64 - 1
    e, twin = _pair(G, N, me, st, hb)
    with e, twin:
        for t in range(2):
            nb, nf = check_tick(oracle, e, twin, st, t, hb, G, bitmap=t == 0, what=f"64-bit tick {t}")
            assert nb > 50


@pytest.mark.parametrize("bitmap", [True, False])
def test_beat_cap_below_the_beat_count(oracle, bitmap):
    """only the first beat_cap groups are built, n_beat is still the total, nothing behind cap or frame_off's end is touched;
    beat_cap = 0 builds nothing"""
    G, N, me, hb = 2500, 3, 2, 1
    rng = np.random.default_rng(9300 + bitmap)
    st = make_state(rng, G, N, me, hb)
    e, twin = _pair(G, N, me, st, hb)
    with e, twin:
        n_lead = int((st.role == 2).sum())
        for t, cap in enumerate([n_lead // 3, 1, 0, n_lead - 1, n_lead, n_lead + 7]):
            nb, nf = check_tick(oracle, e, twin, st, t, hb, cap, bitmap, f"beat_cap {cap}")
            assert nb == n_lead and nf == min(cap, n_lead) * (N - 1)


def test_a_handle_with_no_leader_builds_nothing(oracle):
    from raftsql_amd.engine import pinned_empty
    from raftsql_amd.wire import WireEngine

    G, N, me = 1500, 5, 0
    with WireEngine(G, N, me) as e:  # fresh: every group a follower
        e.set_timers(ET, 1, SEED)
        out, off, po = pinned_empty(e.respond_cap(40), np.uint8), pinned_empty(40 * (N - 1) + 1, np.uint64), pinned_empty(N + 1, np.uint64)
        po[:], off[:] = CANARY64, CANARY64
        s, got_off, got_po, c, hups, nh, second, nb = e.tick_frames(out, off, po, 40, beat_bitmap=True)
        assert nb == 0 and len(s) == 0 and c.n_msgs == 0 and c.bytes == 0 and not got_po.any() and not off.any() and not second.any()
        _, act, rh, _ = oracle.tick(np.zeros(G, np.uint8), np.zeros(G, np.uint32), ET, 1, SEED, 0)
        assert nh == rh and np.array_equal(hups, np.nonzero(act == 1)[0].astype(np.uint32))


def test_frames_follow_whatever_writes_the_state(oracle):
    """the frames come from the device's CURRENT state: after raftq_load_match, after an adopted sweep, after acks through the
    batching turn's ingest, and after Step batches that elect groups and step leaders down (the pattern of tests/test_step_gpu.py::
    test_records_follow_whatever_else_writes_the_dense_arrays)"""
    from raftsql_amd import _lib
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    G, N, me, hb = 3000, 5, 2, 1
    rng = np.random.default_rng(9400)
    st = _stepgen.random_state(rng, G, N, me)
    moved = 0
    with WireEngine(G, N, me) as e:
        e.set_timers(ET, hb, SEED)
        _stepgen.load_engine(e, st)
        for t, move in enumerate(["none", "load_match", "sweep", "step", "deltas", "step", "sweep", "step"]):
            role0 = st.role.copy()
            if move == "load_match":
                lead = st.role == 2
                for p in range(N):
                    if p != me:
                        st.match[p] = np.where(lead, (st.last_index * rng.random(G)).astype(np.uint64), st.match[p])
                e.load_match(st.match, st.committed)
            elif move == "sweep":
                e.sweep(_lib.SWEEP_COMMIT | _lib.SWEEP_GATED)
                st.committed[:] = oracle.commit_advance(st.match, st.committed, True, st.first_idx)[0]
            elif move == "deltas":
                k = 800
                g, p = rng.integers(0, G, k).astype(np.uint64), rng.integers(0, N, k).astype(np.uint32)
                v = (st.last_index[g.astype(np.int64)] * rng.random(k)).astype(np.uint64)
                e.apply_deltas(g, p, v)
                np.maximum.at(st.match, (p.astype(np.int64), g.astype(np.int64)), v)
            elif move == "step":
                m = _stepgen.random_batch(rng, st, 4000)
                want = st.step_batch(m)
                got, _ = e.step_batch(m)
                assert np.array_equal(got, want)
                moved += int(((role0 == 2) != (st.role == 2)).sum())
            check_tick(oracle, e, None, st, t, hb, G, bitmap=t % 2 == 0, what=f"after {move} (tick {t})")
        _stepgen.assert_same_state(e, st)
    assert moved > 20, "the Step batches were meant to elect groups and step leaders down"


def test_refusals_have_not_ticked(oracle):
    """every refusal of the header's table returns its code before anything is enqueued: the next accepted call is the oracle's
    FIRST tick"""
    from raftsql_amd import _lib
    from raftsql_amd.engine import QuorumEngine, RaftqError, pinned_empty
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    G, N, me, hb = 700, 3, 0, 1
    rng = np.random.default_rng(9500)
    st = make_state(rng, G, N, me, hb)
    lib = _lib.load()

    def raw(h, flags, beat_cap, out, cap, off, po):
        nh, nb, c = C.c_uint64(0), C.c_uint64(0), _lib.WireCounts()
        return lib.raftq_tick_frames(h, flags, G, beat_cap, C.byref(nh), C.byref(nb), out.ctypes.data if out is not None else None, cap,
                                     off.ctypes.data if off is not None else None, po.ctypes.data, C.byref(c))

    e, twin = _pair(G, N, me, st, hb)
    with e, twin:
        cap = e.respond_cap(G)
        out, off, po = pinned_empty(cap + 16, np.uint8), pinned_empty(G * (N - 1) + 1, np.uint64), pinned_empty(N + 1, np.uint64)
        assert raw(e._h, 0, G, out, cap - 1, off, po) == _lib.RAFTQ_EINVAL  # cap one byte under the bound
        assert raw(e._h, 0, G, np.zeros(cap, np.uint8), cap, off, po) == _lib.RAFTQ_EINVAL  # pageable out
        assert raw(e._h, 0, G, out, cap, np.zeros(G * (N - 1) + 1, np.uint64), po) == _lib.RAFTQ_EINVAL  # pageable frame_off
        assert raw(e._h, 0, G, out, cap, off, np.zeros(N + 1, np.uint64)) == _lib.RAFTQ_EINVAL  # pageable peer_off
        assert raw(e._h, 0, G, out[8:], cap, off, po) == _lib.RAFTQ_EINVAL  # page-locked, but not 16-byte aligned
        assert raw(e._h, 0, G, out, cap, off[1:], po) == _lib.RAFTQ_EINVAL
        assert raw(e._h, 2, G, out, cap, off, po) == _lib.RAFTQ_EINVAL  # unknown flag
        assert raw(e._h, 0, 2**31, out, 2**62, None, po) == _lib.RAFTQ_EINVAL  # beat_cap * (N - 1) >= 2^31
        assert raw(e._h, 0, 2**30, out, 2**62, None, po) == _lib.RAFTQ_EINVAL
        # a Step batch in flight
        m = _stepgen.random_batch(rng, st, 300)
        e.step_submit(m)
        assert raw(e._h, 0, G, out, cap, off, po) == _lib.RAFTQ_ESTATE
        got, _ = e.step_collect()
        assert np.array_equal(got, st.step_batch(m))
        twin.load_roles(st.role, st.elapsed)
        # voter masks loaded
        e.load_voters(np.full(G, (1 << N) - 1, np.uint16))
        assert raw(e._h, 0, G, out, cap, off, po) == _lib.RAFTQ_ESTATE
        e.load_voters(None)
        with pytest.raises(RaftqError) as ei:  # the binding raises what the library returns
            e.tick_frames(out, off, po, G, cap=cap - 1)
        assert ei.value.code == _lib.RAFTQ_EINVAL
        # none of them ticked: the first accepted call is tick 0
        check_tick(oracle, e, twin, st, 0, hb, G, True, "after the refusals")
        check_tick(oracle, e, twin, st, 1, hb, G, False, "after the refusals, tick 1")
    # a single-peer handle; a handle that was never a node's
    with WireEngine(G, 1, 0) as one:
        po1 = pinned_empty(2, np.uint64)
        assert raw(one._h, 0, G, out, cap, None, po1) == _lib.RAFTQ_EINVAL
    with QuorumEngine(G, N) as q:
        assert raw(q._h, 0, G, out, cap, off, po) == _lib.RAFTQ_ESTATE
