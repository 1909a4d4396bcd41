"""GPU: the two device-built broadcasts over each group's own members (raftq_bcast_set_voters; resp_count_voters_kernel,
resp_scatter_voters_kernel, propose_check_voters_kernel, propose_build_voters_kernel) against tests/ref_bcast_members.py, whose
inputs tests/test_bcast_members_ref.py checks on the CPU.

Masks are ref_bcast_members.masks(): uniform in [1, 2^N) with a few groups forced empty and a few forced to one voter; the respond
inputs plant {self} alone and the full mask among the led groups (ref_bcast_members._respond_start says why), the propose inputs
make self and one other slot vote in the proposed groups; a test that deviates further says so."""
import functools

import numpy as np
import pytest

from oracle import pywire as W
from raftsql_amd import _lib
from raftsql_amd.engine import RaftqError
from tests import _stepgen
from tests import ref_bcast_members as B
from tests import ref_step_voters as V
from tests.test_respond_gpu import _call, _frames, _leader_state
from tests.test_wire_gpu import _same

pytestmark = pytest.mark.gpu

ANSWERED = B.ANSWERED
MSG_APP, MSG_APP_RESP = B.MSG_APP, B.MSG_APP_RESP


@pytest.fixture(scope="module")
def WireEngine(gpu_engine_cls):
    from raftsql_amd.wire import WireEngine

    return WireEngine


def _engine(WireEngine, st, voters, bcast=True):
    e = WireEngine(st.G, st.N, st.self_peer)
    _stepgen.load_engine(e, st)
    if voters is not None:
        e.load_voters(voters)
    if bcast:
        e.set_bcast_voters(True)
    return e


def _code(f, *args, **kw):
    with pytest.raises(RaftqError) as ei:
        f(*args, **kw)
    return ei.value.code, str(ei.value)


def _check_call(e, c, what, resp_off=True):
    """one call against the restatement: everything tests/test_respond_gpu.py::_check compares"""
    want_m, we, want_o, want_w, want_po, want_ans, _ = c["want"]
    s, off = c["s"], c["off"]
    want_s, want_off = W.wire_encode(want_w) if len(want_w) else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    gm, ge, go, got_s, got_off, got_po, cnt, rc = _call(e, s, off, len(we), c["at_tail"], c["tail_appends"], resp_off=resp_off)
    n = len(off) - 1
    assert (cnt.n_msgs, cnt.n_ents, cnt.bytes) == (n, len(we), len(s)), what
    _same(gm, want_m, f"records, {what}")
    _same(ge, we, f"entry headers, {what}")
    ans = (go["flags"] & ANSWERED) != 0
    assert np.array_equal(ans, want_ans), (what, np.nonzero(ans != want_ans)[0][:10])
    go = go.copy()
    go["flags"] &= np.uint8(~ANSWERED & 0xFF)
    _same(go, want_o, f"results, {what}")
    assert np.array_equal(got_po, want_po), (what, got_po, want_po)
    assert rc.n_msgs == len(want_w) and rc.bytes == len(want_s), what
    assert bytes(got_s) == bytes(want_s), what
    if resp_off:
        assert np.array_equal(got_off, want_off), what
    _stepgen.assert_same_state(e, c["after"])


@functools.lru_cache(maxsize=None)
def _run(case, tail_appends=(True, False)):
    """the reference of one case, computed once and never changed"""
    seed, G, N, me, sizes = case
    return B.respond_run(seed, G, N, me, sizes, tail_appends)


# ---- 1. the switch -------------------------------------------------------------------------------------------------------------
def _propose_args(props, pe, pool, hm, he, N):
    from raftsql_amd.engine import pinned_copy, pinned_empty

    out = pinned_empty(len(pool) + 128 * (len(hm) + len(props) * (N - 1)) + 4096, np.uint8)
    off = pinned_empty(len(hm) + len(props) * (N - 1) + 1, np.uint64)
    return [pinned_copy(props), pinned_copy(pe), pinned_copy(hm), pinned_copy(he), pinned_copy(pool), out, off]


def test_the_switch(WireEngine):
    N, me, G = 3, 1, 4096
    s, voters, props, pe, pool, hm, he = B.propose_input(17000, G, N, me, 200, 20)
    start = V.copy_state(s)
    stream, off = _frames([dict(group=int(props["group"][0]), type=MSG_APP_RESP, term=int(s.term[int(props["group"][0])]),
                                index=int(s.last_index[int(props["group"][0])]), **{"from": (me + 1) % N})], me)
    args = _propose_args(props, pe, pool, hm, he, N)
    with _engine(WireEngine, s, voters, bcast=False) as e:
        e.set_step_voters(True)
        e.set_tick_voters(True)

        def refused():
            rc, msg = _code(e.propose_frames, *args)
            assert rc == _lib.RAFTQ_ESTATE and "voter masks" in msg
            rc, msg = _code(_call, e, stream, off, 0, None)
            assert rc == _lib.RAFTQ_ESTATE and "voter masks" in msg
            _stepgen.assert_same_state(e, start)

        refused()
        for bad in (-1, 2):
            assert _code(e.set_bcast_voters, bad)[0] == _lib.RAFTQ_EINVAL
        refused()  # (a refused setting leaves the switch where it was)
        from raftsql_amd import step as S_

        m = S_.pack_msgs(np.array([0], np.uint64), S_.MSG_HEARTBEAT_RESP, term=s.term[:1], frm=(me + 1) % N)
        e.step_submit(m)
        assert _code(e.set_bcast_voters, True)[0] == _lib.RAFTQ_ESTATE  # a batch in flight
        e.step_collect()
        V.step_batch(s, voters, m)
        _stepgen.assert_same_state(e, s)
        e.set_bcast_voters(True)
        *_, rc = _call(e, stream, off, 0, None)  # goes through (no bitmap: nothing to broadcast)
        assert rc.n_msgs == 0
        V.step_batch(s, voters, _rec_of(stream, off, s))
        got, goff, c = e.propose_frames(*args)
        msgs, keep, ents = B.propose_expect(s, voters, props, pe, hm, he)
        want, want_off = B.encode_positional(msgs, keep, ents, pool)
        assert bytes(got) == bytes(want) and np.array_equal(goff, want_off) and c.n_msgs == keep.sum()
        _stepgen.assert_same_state(e, s)
        e.set_bcast_voters(False)
        start = V.copy_state(s)
        refused()


def _rec_of(stream, off, st, tail_appends=True):
    from tests.test_wire_gpu import _node_filter

    wm, we, _ = W.wire_decode(stream, off)
    return _node_filter(wm, we, st.G, st.N, st.self_peer, tail_appends)[1]


# ---- 2. respond against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["lists", "sort"])
def test_respond_matches_the_restatement(WireEngine, walk, monkeypatch):
    if walk == "sort":
        monkeypatch.setenv("RAFTQ_STEP_WALK", "sort")
    start, voters, calls = _run(B.RESPOND_BIG)
    with _engine(WireEngine, start, voters) as e:
        for it, c in enumerate(calls):
            _check_call(e, c, f"call {it}", resp_off=it != 1)
        assert np.array_equal(e.read_voters(), voters)


@pytest.mark.parametrize("N", [2, 3, 4, 5, 6, 7, 8, 9])
def test_respond_for_every_cluster_size_and_slot(WireEngine, N):
    for me in range(N):
        start, voters, calls = B.respond_run(*B.respond_slot_case(N, me), (True, False))
        with _engine(WireEngine, start, voters) as e:
            for it, c in enumerate(calls):
                _check_call(e, c, f"N={N} me={me} call {it}")


def test_respond_with_long_runs_goes_through_the_sorted_walk(WireEngine):
    """> 32 frames of one group: the list walk stalls, the collect replays the batch through the sorted (masked) walk, and the
    answers are laid out over members again"""
    start, voters, calls = _run(B.RESPOND_LONG, (True,))
    assert max(np.unique(_rec_of(calls[0]["s"], calls[0]["off"], start)["group"], return_counts=True)[1]) > 32
    with _engine(WireEngine, start, voters) as e:
        for it, c in enumerate(calls):
            _check_call(e, c, f"call {it}")


# ---- 3. directed respond cases: N = 3, G = 4, self 0, every group led at (10, 3), committed 8, the followers at 8 ------------------
def _directed(WireEngine, rows, voters, bits=(0, 1, 2, 3)):
    G, N, me = 4, 3, 0
    voters = np.asarray(voters, np.uint16)
    st = _leader_state(G, N, me)
    with _engine(WireEngine, st, voters) as e:
        s, off = _frames(rows, me)
        at = B.bitmap(G, bits) if bits is not None else None
        gm, ge, go, got_s, got_off, got_po, c, rc = _call(e, s, off, 0, at)
        want_m, we, want_o, want_w, want_po, want_ans, _ = B.respond_want(st, voters, s, off, at)
        assert np.array_equal((go["flags"] & ANSWERED) != 0, want_ans)
        want_s = W.wire_encode(want_w)[0] if len(want_w) else np.zeros(0, np.uint8)
        assert bytes(got_s) == bytes(want_s) and np.array_equal(got_po, want_po) and rc.n_msgs == len(want_w)
        _stepgen.assert_same_state(e, st)
        return go, W.wire_decode(got_s, got_off)[0] if len(got_s) else np.zeros(0, W.WIRE_MSG_DT), got_po, st


def test_a_committing_ack_broadcasts_to_members_only(WireEngine):
    """group 1 votes {0, 2}: the ack of 2 is a quorum of two, and the broadcast goes to 2 alone; group 2 votes {0, 1, 2}: both"""
    go, sent, po, st = _directed(WireEngine, [dict(group=1, type=MSG_APP_RESP, term=3, index=10, **{"from": 2}),
                                              dict(group=2, type=MSG_APP_RESP, term=3, index=10, **{"from": 1})], [7, 0b101, 7, 7])
    assert (go["flags"] & ANSWERED).all() and list(po) == [0, 0, 1, 3]
    assert list(zip(sent["to"], sent["group"])) == [(1, 2), (2, 1), (2, 2)]
    assert (sent["type"] == MSG_APP).all() and (sent["index"] == 10).all() and (sent["commit"] == 10).all() and (sent["log_term"] == 3).all()
    assert int(st.committed[1]) == 10 and int(st.committed[2]) == 10


def test_a_leader_with_no_other_member_is_answered_with_no_frame(WireEngine):
    """group 3 votes {0}: the ack of a non-voter moves its Match, the one-voter quorum commits the tail, the result is flagged
    RAFTQ_OUTF_ANSWERED and there is nobody to send to"""
    from raftsql_amd import step as S_

    go, sent, po, st = _directed(WireEngine, [dict(group=3, type=MSG_APP_RESP, term=3, index=9, **{"from": 2})], [7, 7, 7, 0b001])
    assert go["flags"][0] & ANSWERED and go["flags"][0] & S_.OUTF_COMMITTED and len(sent) == 0 and list(po) == [0, 0, 0, 0]
    assert int(st.committed[3]) == 10 and int(st.match[2, 3]) == 9


def test_a_clear_at_tail_bit_gives_no_broadcast(WireEngine):
    go, sent, po, st = _directed(WireEngine, [dict(group=1, type=MSG_APP_RESP, term=3, index=10, **{"from": 2})], [7, 0b101, 7, 7], bits=(0, 2, 3))
    assert not go["flags"][0] & ANSWERED and len(sent) == 0 and int(st.committed[1]) == 10


# ---- 4. respond parity ---------------------------------------------------------------------------------------------------------
def test_full_masks_and_no_masks_are_the_unmasked_call(WireEngine, oracle):
    """full masks with the switch on: out, peer_off and resp_off byte for byte those of a second handle without masks; then the
    masks are dropped with the switch still on and the call is the unmasked one (tests/test_respond_gpu.py::_check, the C oracle)"""
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from tests.test_respond_gpu import _check, _leaders_bitmap
    from tests.test_wire_gpu import _node_frames

    G, N, me = 2000, 5, 3
    rng = np.random.default_rng(17400)
    st = _stepgen.random_state(rng, G, N, self_peer=me)
    with _engine(WireEngine, st, V.full_masks(N, G)) as a, _engine(WireEngine, st, None, bcast=False) as b:
        for it, n in enumerate([300, 6000]):
            s, off = _node_frames(rng, n, st, me)
            at = _leaders_bitmap(rng, st, 1.0)
            ps, po = pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, np.uint64))
            got = []
            for e in (a, b):
                out = pinned_empty(e.respond_cap(n), np.uint8)
                out[:] = 0xEE
                r = e.step_frames_respond(ps, po, pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(8 * n, W.WIRE_ENT_DT), pinned_copy(at), out,
                                          pinned_empty(n * (N - 1) + 1, np.uint64), pinned_empty(N + 1, np.uint64))
                got.append((bytes(out), r[4].tobytes(), r[5].tobytes(), r[2].tobytes(), r[7].n_msgs, r[7].bytes))
            assert got[0] == got[1], f"call {it}"
            assert got[0][4] > 0
            st.step_batch(_rec_of(s, off, st))
        for e in (a, b):
            _stepgen.assert_same_state(e, st)
        a.load_voters(None)  # the switch stays on: the handle launches what it always did
        s, off = _node_frames(rng, 3000, st, me)
        answered, frames = _check(a, st, s, off, _leaders_bitmap(rng, st, 1.0), True, "masks dropped")
        assert answered > 0 and frames > answered
        _stepgen.assert_same_state(a, st)


# ---- 5. propose against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,me,n_props,n_host", B.PROPOSE_SHAPES)
def test_propose_matches_the_restatement(WireEngine, N, me, n_props, n_host):
    G = 8192
    _check_propose_members(WireEngine, *B.propose_input(B.propose_seed(N, n_props), G, N, me, n_props, n_host))


def _check_propose_members(WireEngine, s, voters, props, pe, pool, hm, he):
    """one raftq_propose_frames call over members against the restatement (s moves): the stream, the positional offsets, the
    counts, the 0xEE behind the stream, the state after; then every other voter's ack commits the new tail"""
    from raftsql_amd import step as S_
    from raftsql_amd.engine import pinned_copy, pinned_empty

    N, me = s.N, s.self_peer
    with _engine(WireEngine, s, voters) as e:
        committed0 = s.committed.copy()
        msgs, keep, ents = B.propose_expect(s, voters, props, pe, hm, he)  # (s moves)
        want, want_off = B.encode_positional(msgs, keep, ents, pool)
        out, off = pinned_empty(len(want) + 64, np.uint8), pinned_empty(len(msgs) + 1, np.uint64)
        out[:] = 0xEE
        got, goff, c = e.propose_frames(pinned_copy(props), pinned_copy(pe), pinned_copy(hm), pinned_copy(he), pinned_copy(pool), out, off)
        assert np.array_equal(goff, want_off)
        assert got.tobytes() == want.tobytes() and bytes(out[len(want):]) == b"\xee" * 64
        assert (c.n_msgs, c.n_ents, c.bytes) == (int(keep.sum()), len(ents), len(want))
        _stepgen.assert_same_state(e, s)
        assert np.array_equal(s.committed, committed0)
        # and Step goes on from the new tail: the acks of every other voter are a masked quorum and commit it
        e.set_step_voters(True)
        g = props["group"].astype(np.int64)
        for p in range(N):
            if p == me:
                continue
            of = g[((voters[g].astype(np.uint32) >> p) & 1).astype(bool)]
            if not len(of):
                continue
            m = S_.pack_msgs(of.astype(np.uint64), S_.MSG_APP_RESP, term=s.term[of], frm=p, index=s.last_index[of])
            want_o = V.step_batch(s, voters, m)
            got_o, _ = e.step_batch(m)
            assert got_o.tobytes() == want_o.tobytes(), p
        assert np.array_equal(s.committed[g], s.last_index[g])
        _stepgen.assert_same_state(e, s)


# ---- 6. propose refusals -------------------------------------------------------------------------------------------------------
def test_propose_refusals_apply_nothing_and_the_next_call_is_whole(WireEngine):
    """reason 7 (self's bit cleared in one proposed group), reason 8 ({self} alone in one), the six old reasons with masks loaded:
    RAFTQ_EINVAL with the reason's text, the state untouched; then the whole call"""
    from raftsql_amd.engine import pinned_copy, pinned_empty

    N, me, G = 3, 1, 4096
    s, voters, props, pe, pool, hm, he = B.propose_input(16100, G, N, me, 600, 50)
    follower = V.copy_state(s)
    follower.role[int(props["group"][17])] = 0
    dup = props.copy()
    dup["group"][5] = dup["group"][400]
    none = props.copy()
    none["n_ents"][9] = 0
    outside = props.copy()
    outside["ent_first"][599] = len(pe)
    beyond = props.copy()
    beyond["group"][3] = G
    far = pe.copy()
    far["data_off"][3], far["data_len"][3] = len(pool), 8
    v7, v8 = voters.copy(), voters.copy()
    v7[int(props["group"][17])] &= ~np.uint16(1 << me)
    v8[int(props["group"][400])] = 1 << me
    ph, pee, ppool = pinned_copy(hm), pinned_copy(he), pinned_copy(pool)
    out, off = pinned_empty(1 << 20, np.uint8), pinned_empty(len(hm) + 600 * (N - 1) + 1, np.uint64)
    with _engine(WireEngine, s, voters) as e:
        for what, words, (pr, ents_, vm, role) in [
                ("no member", "record 17: this node is no member of its group", (props, pe, v7, s.role)),
                ("commits", "record 400: its append would move the commit index", (props, pe, v8, s.role)),
                ("follower", "record 17: this node does not lead its group", (props, pe, voters, follower.role)),
                ("twice", "its group is named twice", (dup, pe, voters, s.role)),
                ("empty", "record 9: it carries no entries", (none, pe, voters, s.role)),
                ("range", "record 599: its entries lie outside prop_ents[]", (outside, pe, voters, s.role)),
                ("group", "record 3: its group is out of range", (beyond, pe, voters, s.role)),
                ("payload", "record 3: an entry's payload lies outside the pool", (props, far, voters, s.role))]:
            e.load_voters(vm)
            e.load_roles(role, s.elapsed)
            rc, msg = _code(e.propose_frames, pinned_copy(pr), pinned_copy(ents_), ph, pee, ppool, out, off)
            assert rc == _lib.RAFTQ_EINVAL and words in msg and "nothing was appended" in msg, (what, msg)
            e.load_roles(s.role, s.elapsed)
            _stepgen.assert_same_state(e, s)
        e.load_voters(voters)
        msgs, keep, ents = B.propose_expect(s, voters, props, pe, hm, he)
        want, want_off = B.encode_positional(msgs, keep, ents, pool)
        got, goff, c = e.propose_frames(pinned_copy(props), pinned_copy(pe), ph, pee, ppool, out, off)
        assert got.tobytes() == want.tobytes() and np.array_equal(goff[: len(want_off)], want_off) and c.n_msgs == keep.sum()
        _stepgen.assert_same_state(e, s)


def test_the_mask_shrink_example(WireEngine):
    """N = 5, self 0, Match 10, 8, 5, 5, 5, committed 5, voters {0, 1, 2}: refused for reason 8; raftq_apply_log_deltas with the
    unchanged tail reports the commit of 8; then the proposal passes, to the two members, carrying Commit 8"""
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from raftsql_amd.wire import PROP_DT, PROP_ENT_DT

    s, voters = B.shrink_example()
    props, pe = np.zeros(1, PROP_DT), np.zeros(1, PROP_ENT_DT)
    props["group"], props["n_ents"] = 2, 1
    pe["data_len"] = 5
    pool = np.arange(5, dtype=np.uint8)
    hm, he = np.zeros(0, W.WIRE_MSG_DT), np.zeros(0, W.WIRE_ENT_DT)
    out, off = pinned_empty(4096, np.uint8), pinned_empty(5, np.uint64)
    args = [pinned_copy(props), pinned_copy(pe), hm, he, pinned_copy(pool), out, off]
    with _engine(WireEngine, s, voters) as e:
        rc, msg = _code(e.propose_frames, *args)
        assert rc == _lib.RAFTQ_EINVAL and "record 0: its append would move the commit index" in msg and "raftq_apply_log_deltas" in msg
        _stepgen.assert_same_state(e, s)
        e.set_step_voters(True)
        got = e.apply_log_deltas(np.array([2], np.uint64), 10, 3)
        assert list(got) == [8] and list(V.apply_log_deltas(s, voters, [2], 10, 3)) == [8]
        _stepgen.assert_same_state(e, s)
        msgs, keep, ents = B.propose_expect(s, voters, props, pe, hm, he)
        want, want_off = B.encode_positional(msgs, keep, ents, pool)
        got, goff, c = e.propose_frames(*args)
        assert list(keep) == [True, True, False, False] and c.n_msgs == 2
        assert got.tobytes() == want.tobytes() and np.array_equal(goff, want_off)
        sent = W.wire_decode(np.asarray(got), goff[:3])[0]
        assert list(sent["to"]) == [1, 2] and (sent["commit"] == 8).all() and (sent["index"] == 10).all()
        _stepgen.assert_same_state(e, s)
        assert int(s.committed[2]) == 8 and int(s.last_index[2]) == 11


# ---- 7. propose parity ---------------------------------------------------------------------------------------------------------
def test_full_masks_are_the_unmasked_proposals_three_calls_in_a_row(WireEngine):
    """full masks with the switch on: the bytes and offsets of a handle without masks (and the oracle's), three calls in a row on
    each, so that the control block and the members word carry over"""
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from tests.test_wire_gpu import _propose_expect, _propose_setup

    G, N, me = 8192, 3, 0
    rng = np.random.default_rng(17700)
    d, props, pe, pool, hm, he = _propose_setup(rng, G, N, me, 3000, 500, max_per_group=2)
    s = B.propose_state(d, N, me)
    with _engine(WireEngine, s, V.full_masks(N, G)) as a, _engine(WireEngine, s, None, bcast=False) as b:
        pp, ppe, ph, phe, ppool = pinned_copy(props), pinned_copy(pe), pinned_copy(hm), pinned_copy(he), pinned_copy(pool)
        for rep in range(3):
            want_m, want_e, new_last, new_lt = _propose_expect(d, N, me, props, pe, hm, he)
            want, want_off = W.wire_encode(want_m, want_e, pool)
            for e in (a, b):
                out, off = pinned_empty(len(want) + 64, np.uint8), pinned_empty(len(want_m) + 1, np.uint64)
                got, goff, c = e.propose_frames(pp, ppe, ph, phe, ppool, out, off)
                assert np.array_equal(goff, want_off) and got.tobytes() == want.tobytes(), rep
                assert (c.n_msgs, c.n_ents, c.bytes) == (len(want_m), len(want_e), len(want))
            d["last"], d["last_term"] = new_last, new_lt
        na, nb = a.read_node(), b.read_node()
        for k in na:
            assert np.array_equal(na[k], nb[k]), k
        assert np.array_equal(a.read_match(), b.read_match())
