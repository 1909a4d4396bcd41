"""GPU: raftq_propose_set_forward (include/raftq_wire.h "A follower's proposals") -- raftq_propose_frames turns a record whose group
this node follows into ONE MsgProp frame to the group's leader, drops one whose group knows no leader, and says what became of every
record (raftq_propose_outcomes): the *_fwd_kernel forms of raftq_propose_kernels.hpp and the streaming encoder behind them.

Every case compares the stream, every frame offset, the counts, the 0xEE guard behind the stream, the outcomes and the device state
after with tests/ref_propose_forward.py, byte for byte (the reference and every case's inputs are checked on the CPU by
tests/test_propose_forward_ref.py).  Every test fails on a tree without the switch (the symbol does not exist)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pywire as W
from tests import ref_propose_forward as PF
from tests import ref_respond_props as RP
from tests import ref_step_voters as V

pytestmark = pytest.mark.gpu


def _engine(s, voters=None, forward=True):
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    e = WireEngine(s.G, s.N, s.self_peer)
    _stepgen.load_engine(e, s)
    if voters is not None:
        e.load_voters(voters)
        e.set_bcast_voters(True)
    if forward:
        e.set_propose_forward(True)
    return e


def _call(e, props, pe, pool, hm, he, n_want, cap=None, counts=None):
    """-> (propose_frames' tuple, the whole `out` array)"""
    from raftsql_amd.engine import pinned_copy, pinned_empty

    out = pinned_empty(n_want + 64 if cap is None else max(cap, 1), np.uint8)
    out[:] = 0xEE
    off = pinned_empty(len(hm) + len(props) * (e.n_peers - 1) + 1, np.uint64)
    got = e.propose_frames(pinned_copy(props), pinned_copy(pe), pinned_copy(hm), pinned_copy(he), pinned_copy(pool), out[: len(out) if cap is None else cap],
                           off, counts)
    return got, out


def _held_to(got, out, w, n_hm, n_he, n_pe, what):
    stream, off, c, outcomes = got
    assert np.array_equal(off, w["off"]), (what, np.flatnonzero(off != w["off"])[:10])
    assert bytes(stream) == bytes(w["stream"]), what
    assert bytes(out[len(w["stream"]):len(w["stream"]) + 64]) == b"\xee" * 64, what
    assert (c.n_msgs, c.n_ents, c.bytes) == (n_hm + w["n_frames"], n_he + n_pe, len(w["stream"])), (what, c.n_msgs, c.n_ents, c.bytes)
    assert outcomes.dtype == np.uint8 and np.array_equal(outcomes, w["what"]), (what, np.flatnonzero(outcomes != w["what"])[:10])


def _check(c, what):
    """the case's call against the reference; then the marks: the same call over the records of the groups this node does not lead
    succeeds a second time (a mark left behind would read "named twice") and is the reference's again"""
    from tests import _stepgen

    w = c["want"]
    with _engine(c["s0"], c["voters"]) as e:
        assert len(e.propose_outcomes()) == 0  # before any call
        got, out = _call(e, c["props"], c["pe"], c["pool"], c["hm"], c["he"], len(w["stream"]))
        _held_to(got, out, w, len(c["hm"]), len(c["he"]), len(c["pe"]), what)
        _stepgen.assert_same_state(e, c["after"])  # the leaders' tails and own Match moved, nothing else
        rest = c["props"][w["what"] != PF.APPENDED]
        if len(rest):
            st = V.copy_state(c["after"])
            w2 = PF.want(st, c["voters"], rest, c["pe"], c["pool"], c["hm"], c["he"])
            got2, out2 = _call(e, rest, c["pe"], c["pool"], c["hm"], c["he"], len(w2["stream"]))
            _held_to(got2, out2, w2, len(c["hm"]), len(c["he"]), len(c["pe"]), f"{what}, the followers' records again")
            _stepgen.assert_same_state(e, c["after"])


@functools.lru_cache(maxsize=None)
def _parity(k):
    return PF.parity_case(k)


@functools.lru_cache(maxsize=None)
def _masked(k):
    return PF.masked_case(k)


@pytest.mark.parametrize("k", range(len(PF.PARITY)), ids=["N%d-self%d-%d-props-%d-queued-%s" % (c[0], c[1], c[2], c[3], c[4].replace(" ", "-")) for c in PF.PARITY])
def test_parity(oracle, k):
    _check(_parity(k), PF.PARITY[k])


@pytest.mark.parametrize("k", range(len(PF.MASKED)), ids=["N%d-self%d-%d-props-%d-queued-%s" % (c[0], c[1], c[2], c[3], c[4].replace(" ", "-")) for c in PF.MASKED])
def test_masked(oracle, k):
    """raftq_bcast_set_voters with masks loaded: a forward goes to lead whether or not lead or self is a member; the leaders'
    MsgApps go to members only, in the same call"""
    _check(_masked(k), PF.MASKED[k])


def test_all_dropped_succeeds_with_no_frame(oracle):
    """candidates, followers without a leader and followers whose lead is themselves: the call succeeds, the stream is the caller's
    own messages, every slot of the device's has zero length"""
    c = PF.case(3, 1, 300, 0, "dropped", seed=23900, G=512)
    assert c["want"]["n_frames"] == 0 and len(c["want"]["stream"]) == 0 and (c["want"]["what"] == PF.DROPPED).all()
    _check(c, "all dropped")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _spoil(c, reason, i):
    """record i of the case made unsound by `reason` -> (props, prop_ents)"""
    props, pe = c["props"].copy(), c["pe"].copy()
    f = int(props["ent_first"][i])
    if reason == "group":
        props["group"][i] = c["G"]
    elif reason == "empty":
        props["n_ents"][i] = 0
    elif reason == "count":
        props["n_ents"][i] = 1025
    elif reason == "range":
        props["ent_first"][i] = len(pe)
    elif reason == "payload":
        pe["data_len"][f], pe["data_off"][f] = 8, len(c["pool"]) - 3
    elif reason == "twice":
        j = (i + 7) % len(props)
        props["group"][j] = props["group"][i]
    return props, pe


TEXT = {"group": "out of range", "empty": "no entries", "count": "no entries", "range": "outside prop_ents", "payload": "outside the pool", "twice": "named twice"}


def _assert_refused(e, c, props, pe, text, what, **kw):
    from tests import _stepgen

    with pytest.raises(Exception) as ei:
        _call(e, props, pe, c["pool"], c["hm"], c["he"], len(c["want"]["stream"]), **kw)
    assert "propose_frames" in str(ei.value) and text in str(ei.value), (what, ei.value)
    _stepgen.assert_same_state(e, c["s0"])
    assert len(e.propose_outcomes()) == 0, what


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_refusals_apply_nothing(oracle, masked):
    """each existing reason, on a forwarded record and on a leader record of a mixed call; an `out` that is too small; pageable
    arrays: the state untouched after each, no outcomes, and the whole call right behind them is correct -- it names every group,
    so a mark left behind by any refusal would fail it"""
    from raftsql_amd import _lib
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from tests import _stepgen

    c = PF.case(5, 2, 600, 50, "mixed", seed=23700 + masked, masked=masked, G=2048)
    w = c["want"]
    fwd, led, drop = (int(np.flatnonzero(w["what"] == o)[3]) for o in (PF.FORWARDED, PF.APPENDED, PF.DROPPED))
    with _engine(c["s0"], c["voters"]) as e:
        for reason in TEXT:
            for kind, i in (("forwarded", fwd), ("leader", led), ("dropped", drop)):
                props, pe = _spoil(c, reason, i)
                _assert_refused(e, c, props, pe, TEXT[reason], (reason, kind))
        if masked:  # the member refusals are the leader records': self's bit cleared in a led group
            v = c["voters"].copy()
            v[int(c["props"]["group"][led])] &= np.uint16(~(1 << c["me"]) & 0xFFFF)
            e.load_voters(v)
            _assert_refused(e, c, c["props"], c["pe"], "no member", "self is no member of a led group")
            e.load_voters(c["voters"])
        # out is too small: counts->bytes is the size needed, and exactly that cap succeeds once
        cnt = _lib.WireCounts()
        _assert_refused(e, c, c["props"], c["pe"], "out is too small", "cap one byte short", cap=len(w["stream"]) - 1, counts=cnt)
        assert cnt.bytes == len(w["stream"])
        # pageable arrays: refused before anything is enqueued
        out, cc = pinned_empty(len(w["stream"]) + 64, np.uint8), _lib.WireCounts()
        props, pe, ppool = c["props"].copy(), c["pe"].copy(), pinned_copy(c["pool"])
        rc = e._lib.raftq_propose_frames(e._h, props.ctypes.data, len(props), pe.ctypes.data, len(pe), None, 0, None, 0, ppool.ctypes.data, len(ppool),
                                         out.ctypes.data, len(out), None, C.byref(cc))
        assert rc == _lib.RAFTQ_EINVAL
        _stepgen.assert_same_state(e, c["s0"])
        got, out = _call(e, c["props"], c["pe"], c["pool"], c["hm"], c["he"], len(w["stream"]), cap=len(w["stream"]))
        assert np.array_equal(got[1], w["off"]) and bytes(got[0]) == bytes(w["stream"]) and np.array_equal(got[3], w["what"])
        assert (got[2].n_msgs, got[2].bytes) == (len(c["hm"]) + w["n_frames"], len(w["stream"]))
        _stepgen.assert_same_state(e, c["after"])


def test_a_single_peer_handle_is_refused_whatever_the_switch(oracle):
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from raftsql_amd.wire import WireEngine

    props, pe, pool, hm, he = PF.records(np.random.default_rng(5), 64, 4, 0)
    with WireEngine(64, 1, self_peer=0) as e1:
        e1.set_propose_forward(True)
        with pytest.raises(Exception) as ei:
            e1.propose_frames(pinned_copy(props), pinned_copy(pe), pinned_copy(hm), pinned_copy(he), pinned_copy(pool), pinned_empty(4096, np.uint8), None)
        assert "single-peer" in str(ei.value)


def test_the_switch_itself(oracle):
    """0 / 1 only; off by default; not copied by raftq_clone_state"""
    c = PF.case(3, 1, 40, 0, "mixed", seed=23800, G=128)
    with _engine(c["s0"], forward=False) as e, _engine(c["s0"], forward=False) as d:
        with pytest.raises(Exception):
            e.set_propose_forward(2)
        e.set_propose_forward(True)
        d.clone_state_from(e)
        with pytest.raises(Exception) as ei:  # (the clone's own switch is still off)
            d.propose_frames(*_pinned(c), *_outs(c, d))
        assert "does not lead its group" in str(ei.value)
        got = e.propose_frames(*_pinned(c), *_outs(c, e))
        assert len(got) == 4 and np.array_equal(got[3], c["want"]["what"])
        e.set_propose_forward(False)
        assert len(e.propose_outcomes()) == 0


def _pinned(c):
    from raftsql_amd.engine import pinned_copy

    return tuple(pinned_copy(c[k]) for k in ("props", "pe", "hm", "he", "pool"))


def _outs(c, e):
    from raftsql_amd.engine import pinned_empty

    return pinned_empty(len(c["want"]["stream"]) + 4096, np.uint8), pinned_empty(len(c["hm"]) + len(c["props"]) * (e.n_peers - 1) + 1, np.uint64)


# ---- the switch-off twin ---------------------------------------------------------------------------------------------------------------
def test_switch_off_twin(oracle):
    """the same mixed inputs with the switch off: "does not lead its group", nothing applied, no outcomes; an all-leader input gives
    the bytes of the switch-on call"""
    from tests import _stepgen

    c = PF.case(5, 1, 700, 300, "mixed", seed=23600, G=2048)
    with _engine(c["s0"], forward=False) as t:
        with pytest.raises(Exception) as ei:
            t.propose_frames(*_pinned(c), *_outs(c, t))
        assert "does not lead its group" in str(ei.value) and "nothing was appended" in str(ei.value)
        _stepgen.assert_same_state(t, c["s0"])
        assert len(t.propose_outcomes()) == 0
    led = PF.case(5, 1, 700, 300, "led", seed=23601, G=2048)
    w = led["want"]
    with _engine(led["s0"], forward=True) as e, _engine(led["s0"], forward=False) as t:
        on = e.propose_frames(*_pinned(led), *_outs(led, e))
        off = t.propose_frames(*_pinned(led), *_outs(led, t))
        assert len(on) == 4 and len(off) == 3  # (the package hands the outcomes back only under the switch)
        assert bytes(on[0]) == bytes(off[0]) == bytes(w["stream"]) and np.array_equal(on[1], off[1]) and np.array_equal(on[1], w["off"])
        assert (on[2].n_msgs, on[2].n_ents, on[2].bytes) == (off[2].n_msgs, off[2].n_ents, off[2].bytes)
        assert np.array_equal(on[3], w["what"]) and (on[3] == PF.APPENDED).all()
        p, n = C.c_void_p(None), C.c_uint64(9)
        assert t._lib.raftq_propose_outcomes(t._h, C.byref(p), C.byref(n)) == 0 and n.value == 0
        _stepgen.assert_same_state(e, led["after"])
        _stepgen.assert_same_state(t, led["after"])


# ---- the round trip: a follower's front end to the leader's MsgApps, no frame header built on a host ---------------------------------------
def test_round_trip_from_a_followers_proposal_to_the_leaders_msgapps(oracle):
    """handle F (self 1, follows slot 0 in every group) forwards; the slice of slot 0's run, located by frame_off, is handle L's
    inbound stream (self 0, leads every group, every group at the tail; raftq_step_set_msg_flags, raftq_step_set_props and
    raftq_respond_set_props on): every result RAFTQ_OUT_PROPOSED and answered, L's tails moved by each record's count, L's output
    tests/ref_respond_props.py's byte for byte, and the MsgApps decoded carry the payloads F was given"""
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen
    from tests.test_respond_props_gpu import _call as respond_call
    from tests.test_respond_props_gpu import _held_to as respond_held_to

    G, N, n_props = 512, 3, 300
    rng = np.random.default_rng(23950)
    sf = PF.state(rng, G, N, 1, np.full(G, PF.K_FOLLOW + 0))  # the 0-th slot other than self: slot 0
    props, pe, pool, hm, he = PF.records(rng, G, n_props, 0)
    wf = PF.want(V.copy_state(sf), None, props, pe, pool, hm, he)
    assert (wf["what"] == PF.FORWARDED).all() and (wf["to"] == 0).all()
    with _engine(sf) as f:
        got, out = _call(f, props, pe, pool, hm, he, len(wf["stream"]))
        _held_to(got, out, wf, 0, 0, len(pe), "the follower's call")
        stream, off = got[0], got[1]
    # slot 0's run: the first of the N - 1 = 2 runs behind the (empty) host part; slot 2's run has no byte
    assert int(off[2 * n_props]) == int(off[n_props]) == len(stream)
    inbound = np.asarray(stream[int(off[0]):int(off[n_props])]).copy()
    in_off = (off[: n_props + 1] - off[0]).astype(np.uint64)

    sl = RP.leader_state(G, N, 0)
    old_tail = sl.last_index.copy()
    at_tail = RP.bitmap(G, range(G))
    with WireEngine(G, N, 0) as l:  # (the package turns raftq_step_set_msg_flags on at create)
        _stepgen.load_engine(l, sl)
        l.set_step_props(True)
        l.set_respond_props(True)
        n_e = len(pe)
        w = RP.want(sl, inbound, in_off, at_tail, lead=False)  # sl MOVES
        res = respond_call(l, inbound, in_off, n_e + 1, at_tail)
        go = respond_held_to(l, w, res, inbound, in_off, "the leader's call")
        _stepgen.assert_same_state(l, sl)
    assert (go["type"] == 12).all() and w["answered"].all()  # RAFTQ_OUT_PROPOSED, RAFTQ_OUTF_ANSWERED (respond_held_to compared the flag)
    g = props["group"].astype(np.int64)
    want_tail = old_tail.copy()
    want_tail[g] += props["n_ents"]
    assert np.array_equal(sl.last_index, want_tail)
    raw = res[3]
    sent, ents, bad = W.wire_decode(raw, res[4])
    assert bad == 0 and len(sent) == 2 * n_props and list(res[5]) == [0, 0, n_props, 2 * n_props]
    for k, m in enumerate(sent):
        i = k % n_props  # per peer the frames keep the records' order
        assert (int(m["to"]), int(m["from"]), int(m["type"]), int(m["group"]), int(m["term"])) == (1 + k // n_props, 0, 3, int(g[i]), 5)
        assert int(m["index"]) == int(old_tail[g[i]]) and int(m["n_ents"]) == int(props["n_ents"][i])
        for j in range(int(m["n_ents"])):
            en, src = ents[int(m["ent_first"]) + j], pe[int(props["ent_first"][i]) + j]
            assert (int(en["term"]), int(en["index"]), int(en["type"]), int(en["data_len"])) == (5, int(old_tail[g[i]]) + 1 + j, int(src["type"]), int(src["data_len"]))
            a, b = int(en["data_off"]), int(src["data_off"])
            assert bytes(raw[a:a + int(en["data_len"])]) == bytes(pool[b:b + int(src["data_len"])])
