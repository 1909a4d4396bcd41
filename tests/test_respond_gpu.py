"""GPU: raftq_step_frames_respond (include/raftq_wire.h) -- raftq_step_frames plus the responses and commit broadcasts its
results call for, built on the device and marshalled by the streaming encoder.

The expected frames come from a restatement of the header's table and at-tail rule (below) run over the oracle's full
64-byte results, marshalled by oracle/pywire; the inbound records, entry headers, results (RAFTQ_OUTF_ANSWERED aside) and
the state after are checked against the oracle exactly as tests/test_wire_gpu.py checks raftq_step_frames."""
import numpy as np
import pytest

from oracle import pywire as W
from tests.test_wire_gpu import _node_filter, _node_frames, _same

pytestmark = pytest.mark.gpu

ANSWERED = 0x10
MSG_APP, MSG_APP_RESP, MSG_VOTE_RESP, MSG_HB_RESP = 3, 4, 6, 9


def expected(rec, outs, last_term0, at_tail, N, me):
    """the messages results 0..n-1 call for (the table + the at-tail rule + the device-answered prefix), restated.
    rec: the records Step read (pyoracle STEP_MSG_DT); outs: the oracle's full results; last_term0: every group's lastTerm
    before the batch; at_tail: the caller's bitmap or None.  -> (wire records, peer-major; peer_off; answered mask)"""
    from raftsql_amd import step as S

    n = len(rec)
    per_peer = [[] for _ in range(N)]
    answered = np.zeros(n, bool)
    st = {}  # group -> [at-tail bit, host owns the rest, lastTerm]
    for i in range(n):
        o, m = outs[i], rec[i]
        t = int(o["type"])
        if t == S.OUT_SKIPPED:
            continue
        g = int(m["group"])
        if g not in st:
            bit = at_tail is not None and (int(at_tail[g >> 6]) >> (g & 63)) & 1
            st[g] = [bool(bit), False, int(last_term0[g])]
        s = st[g]
        if t == S.OUT_APPENDED and int(m["_resv"]) & 0xFFFFFFFF:
            s[2] = int(m["reject_hint"])
        if t == S.OUT_BECAME_LEADER:
            s[2] = int(o["term"])
        if int(o["role"]) != S.ROLE_LEADER:
            s[0] = False
        mt, rej, idx = int(m["type"]), int(m["reject"]), int(o["index"])
        if t == S.OUT_PROGRESS:
            if mt == MSG_APP_RESP and rej and int(m["index"]) > idx:
                s[0] = False
            elif mt == MSG_HB_RESP and idx < int(o["last_index"]):
                s[0] = False
        kind, to, fields = 0, int(m["from"]), {}
        if not s[1]:
            if t == S.OUT_APPENDED:
                kind, fields = MSG_APP_RESP, {"index": idx}
            elif t == S.OUT_VOTE_RESP:
                kind, fields = MSG_VOTE_RESP, {"reject": int(o["reject"])}
            elif t == S.OUT_HEARTBEAT_RESP:
                kind = MSG_HB_RESP
            elif t == S.OUT_PROGRESS:
                if mt == MSG_APP_RESP and not rej:
                    if not s[0]:
                        s[1] = True
                    elif int(o["flags"]) & S.OUTF_COMMITTED:
                        kind, to = MSG_APP, None
                        fields = {"index": int(o["last_index"]), "log_term": s[2], "commit": int(o["commit"])}
                elif (int(m["index"]) > idx) if mt == MSG_APP_RESP else (idx < int(o["last_index"])):
                    s[1] = True
            elif t != S.OUT_NONE:
                s[1] = True
        if not kind:
            continue
        answered[i] = True
        for p in range(N):
            if p == me or (to is not None and p != to):
                continue
            per_peer[p].append(dict(group=g, term=int(o["term"]), type=kind, to=p, **fields))
    recs = [r for p in range(N) for r in per_peer[p]]
    w = np.zeros(len(recs), W.WIRE_MSG_DT)
    for k, r in enumerate(recs):
        for f, v in r.items():
            w[k][f] = v
    w["from"] = me
    peer_off = np.zeros(N + 1, np.uint64)
    peer_off[1:] = np.cumsum([len(per_peer[p]) for p in range(N)])
    return w, peer_off, answered


def _bitmap(G, groups):
    b = np.zeros((G + 63) // 64, np.uint64)
    for g in np.asarray(groups, np.int64):
        b[g >> 6] |= np.uint64(1) << np.uint64(g & 63)
    return b


def _call(e, s, off, n_ents, at_tail, tail_appends=True, cap=None, resp_off=True):
    from raftsql_amd.engine import pinned_copy, pinned_empty

    n = len(off) - 1
    msgs, ents = pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(n_ents + 1, W.WIRE_ENT_DT)
    out = pinned_empty(e.respond_cap(n) if cap is None else cap, np.uint8)
    ro = pinned_empty(n * (e.n_peers - 1) + 1, np.uint64) if resp_off else None
    po = pinned_empty(e.n_peers + 1, np.uint64)
    at = pinned_copy(at_tail) if at_tail is not None else None
    return e.step_frames_respond(pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, np.uint64)), msgs, ents, at,
                                 out, ro, po, tail_appends=tail_appends)


def _check(e, st, s, off, at_tail, tail_appends, what, resp_off=True):
    """one call against the oracle + the restatement; st (the oracle state) moves with it"""
    from raftsql_amd import step as S

    N, me, G = st.N, st.self_peer, st.G
    wm, we, _ = W.wire_decode(s, off)
    want_m, rec = _node_filter(wm, we, G, N, me, tail_appends)
    last_term0 = st.last_term.copy()
    want_o = st.step_batch(rec)
    want_w, want_po, want_ans = expected(rec, want_o, last_term0, at_tail, N, me)
    want_s, want_off = W.wire_encode(want_w) if len(want_w) else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    gm, ge, go, got_s, got_off, got_po, c, rc = _call(e, s, off, len(we), at_tail, tail_appends, resp_off=resp_off)
    n = len(off) - 1
    assert (c.n_msgs, c.n_ents, c.bytes) == (n, len(we), len(s)), what
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
    return want_ans.sum(), len(want_w)


def _leaders_bitmap(rng, st, frac=0.7):
    lead = np.nonzero(st.role == 2)[0]
    return _bitmap(st.G, lead[rng.random(len(lead)) < frac])


@pytest.mark.parametrize("walk", ["lists", "sort"])
@pytest.mark.parametrize("tail_appends", [True, False])
def test_respond_matches_the_restated_table(oracle, walk, tail_appends, monkeypatch):
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    if walk == "sort":
        monkeypatch.setenv("RAFTQ_STEP_WALK", "sort")
    G, N, me = 3000, 5, 2
    rng = np.random.default_rng(4100 + tail_appends)
    st = _stepgen.random_state(rng, G, N, self_peer=me)
    answered = frames = 0
    with WireEngine(G, N, me) as e:
        _stepgen.load_engine(e, st)
        for it, n in enumerate([1, 255, 257, 9000]):
            s, off = _node_frames(rng, n, st, me)
            a, f = _check(e, st, s, off, _leaders_bitmap(rng, st), tail_appends, f"call {it}", resp_off=it != 1)
            answered, frames = answered + a, frames + f
        _stepgen.assert_same_state(e, st)
    assert answered > 100 and frames > answered


@pytest.mark.parametrize("N", [2, 3, 4, 5, 6, 7, 8, 9])
def test_respond_for_every_cluster_size_and_slot(oracle, N):
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    G = 1500
    rng = np.random.default_rng(4200 + N)
    for me in range(N):
        st = _stepgen.random_state(rng, G, N, self_peer=me)
        with WireEngine(G, N, me) as e:
            _stepgen.load_engine(e, st)
            for it, n in enumerate([257, 2000]):
                s, off = _node_frames(rng, n, st, me)
                _check(e, st, s, off, _leaders_bitmap(rng, st) if it else None, it == 0, f"N={N} me={me} call {it}")
            _stepgen.assert_same_state(e, st)


def test_respond_with_long_runs_goes_through_the_sorted_walk(oracle):
    """> 32 frames of one group: the list walk stalls, the collect replays the batch through the sorted walk, and the
    responses are laid out and marshalled again from what the replay answered"""
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    G, N, me = 40, 3, 1
    rng = np.random.default_rng(4300)
    st = _stepgen.random_state(rng, G, N, self_peer=me)
    with WireEngine(G, N, me) as e:
        _stepgen.load_engine(e, st)
        for it, n in enumerate([6000, 300, 50]):
            s, off = _node_frames(rng, n, st, me)
            _check(e, st, s, off, _leaders_bitmap(rng, st, 1.0), True, f"call {it}")
        _stepgen.assert_same_state(e, st)


# ---- targeted cases: one leader, hand-made frames -----------------------------------------------------------------------

def _leader_state(G, N, me, last=10, term=3):
    from oracle import pyoracle

    st = pyoracle.NodeState(G, N, me)
    st.term[:] = term
    st.last_index[:] = last
    st.last_term[:] = term
    st.committed[:] = last - 2
    st.role[:] = 2
    st.vote[:] = me + 1
    st.lead[:] = me + 1
    st.first_idx[:] = 1
    for p in range(N):
        st.match[p] = last - 2
    st.match[me] = last
    return st


def _frames(rows, me):
    """rows: message fields; `ents`: that many empty entries of the message's term behind its index"""
    m = np.zeros(len(rows), W.WIRE_MSG_DT)
    ents = []
    for k, r in enumerate(rows):
        r = dict(r)
        ne = r.pop("ents", 0)
        for f, v in r.items():
            m[k][f] = v
        m[k]["ent_first"], m[k]["n_ents"] = len(ents), ne
        ents += [(int(m[k]["term"]), int(m[k]["index"]) + 1 + j) for j in range(ne)]
    m["to"] = me
    e = np.zeros(len(ents), W.WIRE_ENT_DT)
    for j, (t, i) in enumerate(ents):
        e[j]["term"], e[j]["index"] = t, i
    s, off = W.wire_encode(m, e, np.zeros(1, np.uint8))
    return s.copy(), off


def _one_leader_case(oracle, rows, G=4, N=3, me=0, bits=(0, 1, 2, 3)):
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    st = _leader_state(G, N, me)
    with WireEngine(G, N, me) as e:
        _stepgen.load_engine(e, st)
        s, off = _frames(rows, me)
        at = _bitmap(G, bits) if bits is not None else None
        wm, we, _ = W.wire_decode(s, off)
        gm, ge, go, got_s, got_off, got_po, c, rc = _call(e, s, off, len(we), at)
        st2 = _leader_state(G, N, me)
        _, rec = _node_filter(wm, we, G, N, me, True)
        lt0 = st2.last_term.copy()
        want_o = st2.step_batch(rec)
        want_w, want_po, want_ans = expected(rec, want_o, lt0, at, N, me)
        assert np.array_equal((go["flags"] & ANSWERED) != 0, want_ans)
        want_s = W.wire_encode(want_w)[0] if len(want_w) else np.zeros(0, np.uint8)
        assert bytes(got_s) == bytes(want_s) and np.array_equal(got_po, want_po)
        _stepgen.assert_same_state(e, st2)
        return go, W.wire_decode(got_s, got_off)[0] if len(got_s) else np.zeros(0, W.WIRE_MSG_DT), got_po


def test_a_committing_ack_broadcasts_to_every_follower(oracle):
    go, sent, po = _one_leader_case(oracle, [dict(group=1, type=MSG_APP_RESP, term=3, index=10, **{"from": 2})])
    assert go["flags"][0] & ANSWERED and list(po) == [0, 0, 1, 2]
    assert list(sent["to"]) == [1, 2] and (sent["type"] == MSG_APP).all() and (sent["index"] == 10).all()
    assert (sent["log_term"] == 3).all() and (sent["commit"] == 10).all() and (sent["from"] == 0).all() and (sent["group"] == 1).all()


def test_a_reject_before_a_committing_ack_leaves_the_broadcast_to_the_host(oracle):
    go, sent, po = _one_leader_case(oracle, [dict(group=1, type=MSG_APP_RESP, term=3, index=10, reject=1, reject_hint=7, **{"from": 1}),
                                             dict(group=1, type=MSG_APP_RESP, term=3, index=10, **{"from": 2})])
    assert not (go["flags"] & ANSWERED).any() and len(sent) == 0 and po[-1] == 0


def test_a_heartbeat_response_below_the_tail_clears_the_bit(oracle):
    go, sent, po = _one_leader_case(oracle, [dict(group=2, type=MSG_HB_RESP, term=3, **{"from": 1}),
                                             dict(group=2, type=MSG_APP_RESP, term=3, index=10, **{"from": 2})])
    assert not (go["flags"] & ANSWERED).any() and len(sent) == 0


def test_commit_then_step_down_and_append_broadcasts_the_earlier_tail(oracle):
    """the leader commits (broadcast at lastIndex 10 / lastTerm 3), then a higher-term MsgApp makes it a follower that
    appends at its tail: the broadcast carries the tail it had, the MsgAppResp the new one"""
    go, sent, po = _one_leader_case(oracle, [dict(group=3, type=MSG_APP_RESP, term=3, index=10, **{"from": 1}),
                                             dict(group=3, type=MSG_APP, term=5, index=10, log_term=3, commit=10, ents=2, **{"from": 2})])
    assert (go["flags"] & ANSWERED).all()
    app = sent[sent["type"] == MSG_APP]
    assert len(app) == 2 and (app["index"] == 10).all() and (app["log_term"] == 3).all() and (app["term"] == 3).all()
    resp = sent[sent["type"] == MSG_APP_RESP]
    assert len(resp) == 1 and resp["to"][0] == 2 and resp["term"][0] == 5 and resp["index"][0] == 12


def test_no_bitmap_means_no_broadcast(oracle):
    go, sent, po = _one_leader_case(oracle, [dict(group=1, type=MSG_APP_RESP, term=3, index=10, **{"from": 2}),
                                             dict(group=0, type=5, term=3, index=10, log_term=3, **{"from": 1})], bits=None)
    assert not go["flags"][0] & ANSWERED and go["flags"][1] & ANSWERED
    assert len(sent) == 1 and sent["type"][0] == MSG_VOTE_RESP and sent["reject"][0] == 1 and sent["to"][0] == 1


# ---- refusals ---------------------------------------------------------------------------------------------------------

def test_refusals_apply_nothing_and_the_next_call_is_whole(oracle):
    from raftsql_amd import _lib
    from raftsql_amd.engine import RaftqError, pinned_copy, pinned_empty
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    G, N, me = 500, 3, 0
    rng = np.random.default_rng(4400)
    st = _stepgen.random_state(rng, G, N, self_peer=me)
    with WireEngine(G, N, me) as e:
        _stepgen.load_engine(e, st)
        s, off = _node_frames(rng, 300, st, me)
        n = len(off) - 1
        wm, we, _ = W.wire_decode(s, off)
        at = _leaders_bitmap(rng, st, 1.0)
        # a cap one byte under the bound
        with pytest.raises(RaftqError) as ei:
            _call(e, s, off, len(we), at, cap=e.respond_cap(n) - 1)
        assert ei.value.code == _lib.RAFTQ_EINVAL
        _stepgen.assert_same_state(e, st)
        # pageable arrays: the output, the bitmap, the boundaries
        ps, po = pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, np.uint64))
        msgs, ents = pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT)
        pin_out, pin_po = pinned_empty(e.respond_cap(n), np.uint8), pinned_empty(N + 1, np.uint64)
        for kw in (dict(out=np.zeros(e.respond_cap(n), np.uint8)), dict(at_tail=at.copy()), dict(peer_off=np.zeros(N + 1, np.uint64)),
                   dict(frame_off=np.ascontiguousarray(off, np.uint64).copy())):
            args = dict(stream=ps, frame_off=po, msgs=msgs, ents=ents, at_tail=pinned_copy(at), out=pin_out, resp_off=None, peer_off=pin_po)
            args.update(kw)
            with pytest.raises(RaftqError) as ei:
                e.step_frames_respond(**args)
            assert ei.value.code == _lib.RAFTQ_EINVAL, kw.keys()
            _stepgen.assert_same_state(e, st)
        _check(e, st, s, off, at, True, "after the refusals")
        _stepgen.assert_same_state(e, st)


# ---- the bench's shape ----------------------------------------------------------------------------------------------------

def _bench_acks(G, N, me, rng):
    """every group led here at term 3 with every follower at lastIndex - 1 (entries just proposed), and an ack from every
    follower: the first commits (one commit broadcast each), the second does not -- 65,536 acks for 32,768 groups x 3"""
    from tests import _stepgen  # noqa: F401

    st = _leader_state(G, N, me, last=20, term=3)
    for p in range(N):
        if p != me:
            st.match[p] = 19
    st.committed[:] = 19
    fol = [p for p in range(N) if p != me]
    order = np.stack([rng.permutation(fol) for _ in range(G)])  # per group, which follower acks first
    m = np.zeros(G * len(fol), W.WIRE_MSG_DT)
    m["group"] = np.repeat(np.arange(G), len(fol))
    m["from"] = order.reshape(-1)
    m["type"], m["term"], m["index"], m["to"] = MSG_APP_RESP, 3, 20, me
    m = m[rng.permutation(len(m))]
    # keep each group's two acks in some order: the permutation already shuffles, the oracle follows the same order
    s, off = W.wire_encode(m)
    return st, s.copy(), off


def test_respond_at_bench_size(oracle):
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    G, N, me = 32768, 3, 0
    rng = np.random.default_rng(4500)
    st, s, off = _bench_acks(G, N, me, rng)
    with WireEngine(G, N, me) as e:
        _stepgen.load_engine(e, st)
        a, f = _check(e, st, s, off, _bitmap(G, np.arange(G)), True, "bench size")
        assert a == G and f == G * (N - 1)
        _stepgen.assert_same_state(e, st)


@pytest.mark.parametrize("compact", [2, 0])
def test_everything_but_the_flag_is_raftq_step_frames(oracle, compact):
    """the same frames into two engines in the same state, one through raftq_step_frames, one through the new call: records,
    entry headers, counts, every result byte but RAFTQ_OUTF_ANSWERED (in the 32-byte form the node reads, and the full one) and
    the state after are the same"""
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    G, N, me = 2000, 3, 1
    rng = np.random.default_rng(4600 + compact)
    st = _stepgen.random_state(rng, G, N, self_peer=me)
    with WireEngine(G, N, me) as a, WireEngine(G, N, me) as b:
        for e in (a, b):
            _stepgen.load_engine(e, st)
            e.set_compact(compact)
        for it, n in enumerate([300, 6000]):
            s, off = _node_frames(rng, n, st, me)
            wm, we, _ = W.wire_decode(s, off)
            ps, po = pinned_copy(np.ascontiguousarray(s)), pinned_copy(np.ascontiguousarray(off, np.uint64))
            ma, ea = pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT)
            mb, eb = pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT)
            ra = a.step_frames(ps, po, ma, ea)
            rb = b.step_frames_respond(ps, po, mb, eb, pinned_copy(_leaders_bitmap(rng, st, 1.0)), pinned_empty(b.respond_cap(n), np.uint8),
                                       None, pinned_empty(N + 1, np.uint64))
            _same(rb[0], ra[0], f"records, call {it}")
            _same(rb[1], ra[1], f"entry headers, call {it}")
            ca, cb = ra[3], rb[6]
            assert (ca.n_msgs, ca.n_ents, ca.n_malformed, ca.bytes) == (cb.n_msgs, cb.n_ents, cb.n_malformed, cb.bytes)
            got = rb[2].copy()
            assert ((got["flags"] & ANSWERED) != 0).sum() > 0
            got["flags"] &= np.uint8(~ANSWERED & 0xFF)
            _same(got, ra[2], f"results, call {it}")
            st.step_batch(_node_filter(wm, we, G, N, me, True)[1])
        ra_, rb_ = a.read_node(), b.read_node()
        for k in ra_:
            assert np.array_equal(ra_[k], rb_[k]), k
        assert np.array_equal(a.read_match(), b.read_match()) and np.array_equal(a.read_votes(), b.read_votes())
