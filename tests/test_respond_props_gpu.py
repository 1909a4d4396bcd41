"""GPU: raftq_respond_set_props (include/raftq_wire.h "A forwarded proposal's MsgApps") -- raftq_step_frames_respond answers a
RAFTQ_OUT_PROPOSED of a group at the tail with the leader's MsgApps, built on the device: the lead-form walks, the scatter kernels'
wave-stamped entry headers, and the streaming encoder gathering the payloads from the decoder's copy of the inbound stream.

Every case compares out, resp_off, peer_off, resp_counts, the result flags, the records and entry headers handed back and the device
state after with tests/ref_respond_props.py, byte for byte; and with a twin handle that ran the switch off, whose frames are the
reference's without the rule and which marshals the reference's records through raftq_wire_encode with the inbound stream as the pool.
Every test fails on a tree without the switch (the symbol does not exist)."""
import functools

import numpy as np
import pytest

from oracle import pywire as W
from tests import ref_respond_props as RP
from tests import ref_step_voters as V
from tests.test_wire_gpu import _same

pytestmark = pytest.mark.gpu

ANSWERED = RP.ANSWERED
PROPOSED, FORWARD, PROGRESS, BECAME_LEADER = 12, 13, 5, 4


def _engine(st, props=True, lead=False, voters=None):
    from raftsql_amd.wire import WireEngine
    from tests import _stepgen

    e = WireEngine(st.G, st.N, st.self_peer)
    _stepgen.load_engine(e, st)
    e.set_step_props(True)
    if voters is not None:
        e.load_voters(voters)
        e.set_bcast_voters(True)
    if lead:
        e.set_respond_lead(True)
    if props:
        e.set_respond_props(True)
    return e


def _call(e, s, off, ents_cap, at_tail, cap=None, resp_off=True, ents=True, pin_stream=True):
    from raftsql_amd.engine import pinned_copy, pinned_empty

    n = len(off) - 1
    msgs = pinned_empty(n, W.WIRE_MSG_DT)
    ent_arr = pinned_empty(ents_cap, W.WIRE_ENT_DT) if ents else None
    out = pinned_empty(e.respond_cap(n, len(s), ents_cap) if cap is None else cap, np.uint8)
    ro = pinned_empty(n * (e.n_peers - 1) + 1, np.uint64) if resp_off else None
    po = pinned_empty(e.n_peers + 1, np.uint64)
    at = pinned_copy(at_tail) if at_tail is not None else None
    stream = np.ascontiguousarray(s)
    return e.step_frames_respond(pinned_copy(stream) if pin_stream else stream.copy(), pinned_copy(np.ascontiguousarray(off, np.uint64)), msgs,
                                 ent_arr, at, out, ro, po)


def _held_to(e, w, got, s, off, what, resp_off=True):
    gm, ge, go, got_s, got_off, got_po, c, rc = got
    assert (c.n_msgs, c.n_ents, c.bytes) == (len(off) - 1, len(w["ents"]), len(s)), what
    _same(gm, w["m"], f"records, {what}")
    _same(ge, w["ents"][: len(ge)], f"entry headers, {what}")
    ans = (go["flags"] & ANSWERED) != 0
    assert np.array_equal(ans, w["answered"]), (what, np.nonzero(ans != w["answered"])[0][:10])
    go = go.copy()
    go["flags"] &= np.uint8(~ANSWERED & 0xFF)
    _same(go, w["outs"], f"results, {what}")
    assert np.array_equal(got_po, w["peer_off"]), (what, got_po, w["peer_off"])
    assert rc.n_msgs == w["n_frames"] and rc.bytes == len(w["stream"]), (what, rc.n_msgs, w["n_frames"], rc.bytes, len(w["stream"]))
    assert bytes(got_s) == bytes(w["stream"]), what
    if resp_off:
        assert np.array_equal(got_off, w["off"]), what
    return go


def _check(e, t, st, s, off, at_tail, what, voters=None, lead=False, ents_cap=None, resp_off=True, slack=1):
    """one call on the handle e (switch on) and on its twin t (switch off; None: no twin) against the reference; st, the reference's
    state, moves with it -> the reference's dict (+ "got": the handle's results and its frames decoded by the oracle)"""
    from tests import _stepgen

    st_t = V.copy_state(st)
    n_e = len(W.wire_decode(s, off)[1])
    cap_e = n_e + slack if ents_cap is None else ents_cap
    w = RP.want(st, s, off, at_tail, voters, lead=lead, ents_cap=None if ents_cap is None else ents_cap)
    got = _call(e, s, off, cap_e, at_tail, resp_off=resp_off)
    go = _held_to(e, w, got, s, off, what, resp_off)
    _stepgen.assert_same_state(e, st)
    if t is not None:
        w_off = RP.want(st_t, s, off, at_tail, voters, lead=lead, props=False)
        tg = _call(t, s, off, cap_e, at_tail)
        _held_to(t, w_off, tg, s, off, f"the twin, {what}")
        _stepgen.assert_same_state(t, st)
        _same(tg[0], got[0], f"twin records, {what}")
        _same(tg[1], got[1], f"twin entry headers, {what}")
        if len(w["sent"]):  # the MsgApps (and everything else) built by the test, marshalled by the twin's raftq_wire_encode
            ts, toff = t.wire_encode(w["sent"], w["sent_ents"], np.ascontiguousarray(s))
            assert bytes(ts) == bytes(got[3]), f"twin marshal, {what}"
            if resp_off:
                assert np.array_equal(np.asarray(toff, np.uint64), got[4]), f"twin offsets, {what}"
    w["got"] = (go, W.wire_decode(got[3], got[4]) if resp_off and len(got[3]) else None, got[5], got[3])
    return w


def _pair(st, **kw):
    return _engine(st, **kw), _engine(st, **dict(kw, props=False))


# ---- directed ----------------------------------------------------------------------------------------------------------------------
def test_one_proposal_builds_the_leaders_msgapps(oracle):
    """N = 3, term 5, the log ends at (10, term 3), committed 8: two frames, Index 10, LogTerm 3, Commit 8, the entry stamped (5, 11)"""
    G, N, me = 4, 3, 0
    st = RP.leader_state(G, N, me)
    e, t = _pair(st)
    with e, t:
        s, off = RP.frames([RP.prop(1, 2, [(0, b"hello")])], me)
        w = _check(e, t, st, s, off, RP.bitmap(G, [1]), "one proposal")
        go, (sent, ents, _), po, raw = w["got"]
    assert go["type"][0] == PROPOSED and w["answered"][0] and w["taken"] == [0]
    assert list(po) == [0, 0, 1, 2] and list(sent["to"]) == [1, 2] and (sent["type"] == 3).all() and (sent["term"] == 5).all()
    assert (sent["index"] == 10).all() and (sent["log_term"] == 3).all() and (sent["commit"] == 8).all() and (sent["n_ents"] == 1).all()
    for k in range(2):
        en = ents[int(sent["ent_first"][k])]
        assert (int(en["term"]), int(en["index"]), int(en["data_len"]), int(en["type"])) == (5, 11, 5, 0)
        assert bytes(raw[int(en["data_off"]):int(en["data_off"]) + 5]) == b"hello"
    assert int(st.last_index[1]) == 11 and int(st.last_term[1]) == 5


@pytest.mark.parametrize("bitmap", ["clear", "none"])
def test_a_proposal_with_the_bit_clear_is_the_hosts(oracle, bitmap):
    """not answered, the prefix ends: the committing ack behind it builds nothing either"""
    G, N, me = 4, 3, 0
    st = RP.leader_state(G, N, me)
    e, t = _pair(st)
    with e, t:
        s, off = RP.frames([RP.prop(1, 2, [(0, b"hello")]), RP.ack(1, 2, 5, 11), RP.ack(2, 1, 5, 10)], me)
        w = _check(e, t, st, s, off, RP.bitmap(G, [2]) if bitmap == "clear" else None, bitmap)
        go, _, po, _ = w["got"]
    assert list(go["type"]) == [PROPOSED, PROGRESS, PROGRESS] and not w["answered"][:2].any() and w["taken"] == []
    assert w["answered"][2] == (bitmap == "clear") and int(st.committed[1]) == 11


def test_switch_off_is_the_call_as_it_was(oracle):
    """a handle that never saw the switch and one that had it on and off again: the parent's frames, flags and cap rule"""
    kw = RP.case_list()[10]
    start, voters, s, off, at = RP.random_case(**kw)
    a, b = _engine(start, props=False), _engine(start, props=False)
    with a, b:
        b.set_respond_props(True)
        assert b.respond_cap(10, 100, 7) == 10 * (kw["N"] - 1) * 83 + (kw["N"] - 1) * (100 + 7 * 40)
        b.set_respond_props(False)
        n = len(off) - 1
        assert a.respond_cap(n, len(s), 99) == b.respond_cap(n, len(s), 99) == n * (kw["N"] - 1) * 83
        n_e = len(W.wire_decode(s, off)[1])
        for x in (a, b):
            w = RP.want(V.copy_state(start), s, off, at, lead=False, props=False)
            assert w["taken"] == [] and (w["outs"]["type"] == PROPOSED).sum() >= 8
            _held_to(x, w, _call(x, s, off, n_e + 1, at, cap=n * (kw["N"] - 1) * 83), s, off, "switch off")
        # ... and ents == NULL is still allowed there
        x = _engine(start, props=False)
        with x:
            _held_to(x, w, _call(x, s, off, 0, at, ents=False), s, off, "switch off, no ents")


def test_a_committing_ack_and_a_second_proposal_behind_a_proposal(oracle):
    """the bit stays: the ack gets the empty MsgApps with Index = the new tail behind the entry frames in every slice, the second
    proposal is answered against the new tail and carries the new commit"""
    G, N, me = 4, 3, 1
    st = RP.leader_state(G, N, me, committed=9, match=10)
    e, t = _pair(st)
    with e, t:
        s, off = RP.frames([RP.prop(2, 0, [(0, b"a"), (0, b"bc")]), RP.ack(2, 0, 5, 12), RP.prop(2, 2, [(1, b"conf")])], me)
        w = _check(e, t, st, s, off, RP.bitmap(G, [2]), "ack + second proposal")
        go, (sent, ents, _), po, _ = w["got"]
    assert w["answered"].all() and w["taken"] == [0, 2] and list(po) == [0, 3, 3, 6]
    assert list(sent["index"][:3]) == [10, 12, 12] and list(sent["log_term"][:3]) == [3, 5, 5] and list(sent["commit"][:3]) == [10, 12, 12]
    assert list(sent["n_ents"][:3]) == [2, 0, 1]
    last = ents[int(sent["ent_first"][2])]
    assert (int(last["term"]), int(last["index"]), int(last["type"])) == (5, 13, 1)  # EntryConfChange kept


@pytest.mark.parametrize("lead", [False, True])
def test_behind_a_device_answered_win(oracle, lead):
    """raftq_respond_set_lead on: the win puts the group at the tail with no bitmap at all, the proposal behind it is answered -- the
    empty entry's slot and the proposal's side by side.  Off: the win ends the prefix, the proposal is the host's"""
    from tests import ref_respond_lead as L

    G, N, me = 4, 3, 0
    st = L.candidate_state(G, N, me)
    e, t = _pair(st, lead=lead)
    with e, t:
        s, off = RP.frames([dict(group=1, type=6, term=7, **{"from": 2}), RP.prop(1, 1, [(0, b"x" * 20), (0, b"")]),
                            dict(group=3, type=6, term=7, **{"from": 1})], me)
        w = _check(e, t, st, s, off, None, f"win, lead={lead}", lead=lead)
        go, dec, po, _ = w["got"]
    assert list(go["type"]) == [BECAME_LEADER, PROPOSED, BECAME_LEADER]
    assert list(w["answered"]) == [lead] * 3 and w["taken"] == ([1] if lead else [])
    if lead:
        sent = dec[0]
        assert list(sent["n_ents"][:3]) == [1, 2, 1] and list(sent["index"][:3]) == [10, 11, 10] and list(sent["log_term"][:3]) == [2, 7, 2]


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 127, 128, 300, 16384])
def test_payload_lengths_at_unaligned_offsets(oracle, length):
    """the 16-byte copy boundaries and the varint boundaries of the data and entry lengths; the payloads start at odd offsets"""
    G, N, me = 8, 3, 2
    st = RP.leader_state(G, N, me)
    rng = np.random.default_rng(9900 + length)
    data = bytes(rng.integers(0, 256, length, dtype=np.uint8))
    rows = [RP.prop(g, g % 2, [(0, data[k:] + data[:k]) for k in range(1 + g % 3)] + [(0, b"q" * g)]) for g in range(1, 8)]
    e, t = _pair(st)
    with e, t:
        s, off = RP.frames(rows, me, pad=3)
        w = _check(e, t, st, s, off, RP.bitmap(G, range(G)), f"length {length}")
    assert w["taken"] == list(range(7))


@pytest.mark.parametrize("count", [1, 2, 3, 64, 65, 300])
def test_entry_counts_in_one_frame(oracle, count):
    """one frame with `count` entries (more than the decoder's lanes keep, one wave, one wave and a lane, five rounds of the wave)
    between two small ones"""
    G, N, me = 4, 4, 1
    st = RP.leader_state(G, N, me)
    many = [(k % 2, bytes([k % 251]) * (k % 7)) for k in range(count)]
    e, t = _pair(st)
    with e, t:
        s, off = RP.frames([RP.prop(0, 0, [(0, b"first")]), RP.prop(1, 2, many), RP.prop(2, 3, [(0, b"last")])], me)
        w = _check(e, t, st, s, off, RP.bitmap(G, range(G)), f"{count} entries")
        go, (sent, ents, _), po, _ = w["got"]
    assert w["taken"] == [0, 1, 2] and int(st.last_index[1]) == 10 + count
    k = int(np.flatnonzero(sent["n_ents"] == count)[0]) if count > 1 else 1
    got = ents[int(sent["ent_first"][k]):int(sent["ent_first"][k]) + count]
    assert list(got["index"]) == list(range(11, 11 + count)) and (got["term"] == 5).all() and list(got["type"]) == [k % 2 for k in range(count)]


def test_proposals_at_the_workgroup_boundaries(oracle):
    """513 frames -- two workgroups of the layout and a lone lane -- with the proposals at 0, 63, 64, 255, 256, 257, 511, 512; every
    other frame a heartbeat response that builds nothing"""
    G, N, me, n = 600, 5, 3, 513
    positions = (0, 63, 64, 255, 256, 257, 511, 512)
    st = RP.leader_state(G, N, me, match=10)
    rows, k = [], 0
    for i in range(n):
        if i in positions:
            j = positions.index(i)
            rows.append(RP.prop(j, (me + 1 + j) % N if (me + 1 + j) % N != me else (me + 2) % N, [(0, bytes([j]) * (j + 1))] * (1 + j % 3)))
        else:
            rows.append(dict(group=8 + k, type=9, term=5, **{"from": (me + 1) % N}))
            k += 1
    e, t = _pair(st)
    with e, t:
        s, off = RP.frames(rows, me)
        w = _check(e, t, st, s, off, RP.bitmap(G, range(8)), "boundaries")
    assert w["taken"] == list(positions) and w["n_frames"] == 8 * (N - 1)


def test_a_long_run_with_proposals_goes_through_the_replay(oracle):
    """more than 32 frames of one group: the list walk stalls, the replay answers through the sorted lead walk and the layout --
    with the stamped headers -- is made again: the same bytes as the reference's"""
    G, N, me = 8, 3, 1
    st = RP.leader_state(G, N, me, match=10)
    rows = [RP.prop(5, 0, [(0, b"one")])]
    rows += [RP.ack(5, 2 * (k % 2), 5, 11) for k in range(34)]
    rows += [RP.prop(5, 2, [(0, b"two"), (0, b"")]), RP.prop(3, 0, [(0, b"other")])]
    e, t = _pair(st)
    with e, t:
        s, off = RP.frames(rows, me)
        w = _check(e, t, st, s, off, RP.bitmap(G, [3, 5]), "long run")
    assert w["taken"] == [0, 35, 36] and w["answered"][[0, 1, 35, 36]].all() and int(st.committed[5]) == 11  # (the first ack commits)


def test_payloads_fed_from_the_callers_stream(oracle, monkeypatch):
    """RAFTQ_RESPOND_PROPS_POOL=feed, the measured alternative: the encoder's readers bring the pool in from the caller's
    stream instead of the decoder's copy being kept -- the same bytes"""
    monkeypatch.setenv("RAFTQ_RESPOND_PROPS_POOL", "feed")
    _run(len(_CASES) - 7)
    test_payload_lengths_at_unaligned_offsets(oracle, 300)


# ---- over members ---------------------------------------------------------------------------------------------------------------------
def test_over_members(oracle):
    """N = 5: a non-member gets no frame; a one-voter group commits on the append and its proposal carries the new commit with zero
    frames (no member but self); a group whose other member is slot 2 sends one frame"""
    G, N, me = 4, 5, 0
    st = RP.leader_state(G, N, me)
    voters = np.array([0b00111, 0b00111, 0b00001, 0b00101], np.uint16)
    e, t = _pair(st, voters=voters)
    with e, t:
        s, off = RP.frames([RP.prop(1, 3, [(0, b"abc")]), RP.prop(2, 4, [(0, b"solo")]), RP.prop(3, 1, [(0, b"pair")])], me)
        w = _check(e, t, st, s, off, RP.bitmap(G, range(G)), "members", voters)
        go, (sent, _, _), po, _ = w["got"]
    assert w["answered"].all() and w["taken"] == [0, 1, 2] and list(po) == [0, 0, 1, 3, 3, 3]
    assert list(sent["to"]) == [1, 2, 2] and list(sent["group"]) == [1, 1, 3]
    assert int(go["commit"][1]) == 11 and int(st.committed[2]) == 11  # the one-voter group committed its own append


# ---- random ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(k):
    return RP.random_case(**RP.case_list()[k])


def _run(k, lead=False, twin=True):
    start, voters, s, off, at = _case(k)
    st = V.copy_state(start)
    e = _engine(st, lead=lead, voters=voters)
    t = _engine(st, lead=lead, voters=voters, props=False) if twin else None
    with e:
        w = _check(e, t, st, s, off, at, f"case {k}", voters, lead=lead)
    if t is not None:
        t.close()
    assert len(w["taken"]) >= RP.FLOORS["answered proposals"]
    return w


_CASES = RP.case_list()
_BY_N = {N: [k for k, c in enumerate(_CASES) if c["N"] == N and c["n_frames"] == 300] for N in range(2, 10)}


@pytest.mark.parametrize("N", range(2, 10))
def test_every_cluster_size_and_slot(oracle, N):
    assert len(_BY_N[N]) == N
    for k in _BY_N[N]:
        _run(k, twin=False)


@pytest.mark.parametrize("walk", ["lists", "sort"])
@pytest.mark.parametrize("which", ["plain 0", "plain 1", "masked", "hot"])
def test_random_batches(oracle, walk, which, monkeypatch):
    if walk == "sort":
        monkeypatch.setenv("RAFTQ_STEP_WALK", "sort")
    k = len(_CASES) - 7 + ["plain 0", "plain 1", "masked", "hot"].index(which)
    assert ("masked" in _CASES[k]) == (which == "masked") and ("hot" in _CASES[k]) == (which == "hot")
    _run(k, lead=which == "plain 1")


def test_all_three_switches_together(oracle):
    """raftq_respond_set_props with raftq_respond_set_lead and raftq_bcast_set_voters (the other combinations are above: alone,
    with lead, with members; and each with the switch off in the twins)"""
    _run(len(_CASES) - 5, lead=True)


@pytest.mark.parametrize("band", ["b32", "b63", "top"])
def test_wide_values_with_cap_exactly_at_the_bound(oracle, band):
    """tails within 6 of 2^32 and of 2^63 and in [2^64 - 2^12, 2^64 - 2^11): the stamped term and index take up to ten bytes; out is
    exactly the header's bound"""
    from tests import _widegen as WG

    k = len(_CASES) - 3 + WG.BAND_NAMES.index(band)
    assert _CASES[k]["band"] == band
    w = _run(k)
    assert int(w["sent_ents"]["index"].max()) >= {"b32": 2**32 - 6, "b63": 2**63 - 6, "top": 2**64 - 2**12}[band]
    start, voters, s, off, at = _case(k)
    n, N = len(off) - 1, start.N
    n_e = len(w["ents"])
    with _engine(start) as e:
        bound = RP.cap_bound(n, N, len(s), n_e, False)
        assert e.respond_cap(n, len(s), n_e) == bound
        _held_to(e, w, _call(e, s, off, n_e, at, cap=bound), s, off, f"cap at the bound, {band}")


def test_headers_beyond_ents_cap_leave_the_proposal_to_the_host(oracle):
    """more entries than ents_cap is no error of the frames calls: a proposal whose headers the decoder could not hand back is not
    answered and ends its group's prefix; the ones in front of it are"""
    G, N, me = 4, 3, 0
    st = RP.leader_state(G, N, me)
    with _engine(st) as e:
        s, off = RP.frames([RP.prop(0, 1, [(0, b"aa")] * 3), RP.prop(1, 2, [(0, b"bb")] * 3), RP.prop(2, 1, [(0, b"cc")])], me)
        w = _check(e, None, st, s, off, RP.bitmap(G, range(G)), "beyond ents_cap", ents_cap=5)
    assert w["taken"] == [0] and list(w["answered"]) == [True, False, False]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_its_twin(oracle):
    """cap one byte below the bound, ents == NULL, an unpinned stream, on = 2, the switch with a batch in flight: each is refused before
    anything is applied and leaves everything that can be read of the handle equal to a twin's that saw no refusal; then both take a
    whole call"""
    from raftsql_amd import _lib
    from raftsql_amd import step as S
    from raftsql_amd.engine import RaftqError
    from tests import _refusals as R

    k = len(_CASES) - 6
    start, voters, s, off, at = _case(k)
    st = V.copy_state(start)
    n, N, me = len(off) - 1, start.N, start.self_peer
    n_e = len(W.wire_decode(s, off)[1])

    def code(f, *a, **kw):
        with pytest.raises(RaftqError) as ei:
            f(*a, **kw)
        return ei.value.code

    with _engine(st) as e, _engine(st) as t:
        bound = RP.cap_bound(n, N, len(s), n_e + 1, False)
        assert e.respond_cap(n, len(s), n_e + 1) == bound
        assert code(_call, e, s, off, n_e + 1, at, cap=bound - 1) == _lib.RAFTQ_EINVAL
        R.same_snapshot(R.snapshot(e), R.snapshot(t), "cap one below the bound")
        assert code(_call, e, s, off, n_e + 1, at, ents=False, cap=bound) == _lib.RAFTQ_EINVAL
        R.same_snapshot(R.snapshot(e), R.snapshot(t), "ents == NULL")
        assert code(_call, e, s, off, n_e + 1, at, pin_stream=False) == _lib.RAFTQ_EINVAL
        R.same_snapshot(R.snapshot(e), R.snapshot(t), "an unpinned stream")
        assert code(e.set_respond_props, 2) == _lib.RAFTQ_EINVAL
        m = S.pack_msgs(np.array([0], np.uint64), S.MSG_HEARTBEAT_RESP, term=st.term[:1], frm=(me + 1) % N)
        for x in (e, t):
            x.step_submit(m)
        assert code(e.set_respond_props, False) == _lib.RAFTQ_ESTATE  # a batch in flight
        for x in (e, t):
            x.step_collect()
        from tests import ref_step_props as P

        P.step_batch(st, None, m)
        R.same_snapshot(R.snapshot(e), R.snapshot(t), "the switch with a batch in flight")
        w = _check(e, None, V.copy_state(st), s, off, at, "after the refusals")
        assert len(w["taken"]) >= 8
        _check(t, None, st, s, off, at, "the twin")
        R.same_snapshot(R.snapshot(e), R.snapshot(t), "behind the whole call")
