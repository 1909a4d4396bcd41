"""CPU: tests/ref_respond_props.py, the reference of the GPU suite, is held to a hand table of frame bytes written out literally;
with the new rule switched off it is tests/ref_respond_lead.expected on every random case; and every random case the GPU tests run
contains what tells the feature from its absence (tests/ref_respond_props.FLOORS)."""
import functools

import numpy as np
import pytest

from tests import ref_respond_lead as L
from tests import ref_respond_props as RP
from tests import ref_step_voters as V

G, N, ME = 4, 3, 0
# a frame: 8-byte big-endian length | 08 type | 10 to+1 | 18 from+1 | 20 term | 28 logTerm | 30 index | 3a len entry ... | 40 commit |
# 4a 08 12 06 0a 00 10 00 18 00 (the empty snapshot) | 50 reject | 58 rejectHint | 60 group;  an entry: 08 type | 10 term | 18 index |
# 22 len data (left out when the data is empty)
TAIL = "4a0812060a0010001800" "5000" "5800" "6001"


def _app(to, term, log_term, index, ents, commit):
    body = "0803" + "10%02x" % (to + 1) + "1801" + "20%02x" % term + "28%02x" % log_term + "30%02x" % index + ents + "40%02x" % commit + TAIL
    return "%016x" % (len(body) // 2) + body


HELLO = "3a0d" "0800" "1005" "180b" "2205" "68656c6c6f"  # {EntryNormal, Term 5, Index 11, "hello"}
HI = "3a0a" "0800" "1005" "180b" "2202" "6869"          # {EntryNormal, Term 5, Index 11, "hi"}
CONF_EMPTY = "3a06" "0801" "1005" "180c"                # {EntryConfChange, Term 5, Index 12, no Data field}
EMPTY_7_11 = "3a06" "0800" "1007" "180b"                # becomeLeader's empty entry {Term 7, Index 11}
X_7_12 = "3a09" "0800" "1007" "180c" "2201" "78"        # {EntryNormal, Term 7, Index 12, "x"}

TABLE = {
    # the leader at term 5, log (10, term 3), committed 8, followers' Match 8: Index 10, LogTerm 3, Commit 8
    "one proposal of one entry": (
        "leader", [RP.prop(1, 2, [(0, b"hello")])], [1], False,
        [_app(1, 5, 3, 10, HELLO, 8), _app(2, 5, 3, 10, HELLO, 8)], [0, 0, 1, 2], [True]),
    "two entries, one with empty Data": (
        "leader", [RP.prop(1, 2, [(0, b"hi"), (1, b"")])], [1], False,
        [_app(1, 5, 3, 10, HI + CONF_EMPTY, 8), _app(2, 5, 3, 10, HI + CONF_EMPTY, 8)], [0, 0, 1, 2], [True]),
    # a candidate at term 7, log (10, term 2), committed 8: the win's frame, then the proposal's against the tail (11, term 7)
    "a proposal behind a win": (
        "candidate", [dict(group=1, type=6, term=7, **{"from": 2}), RP.prop(1, 1, [(0, b"x")])], None, True,
        [_app(1, 7, 2, 10, EMPTY_7_11, 8), _app(1, 7, 7, 11, X_7_12, 8), _app(2, 7, 2, 10, EMPTY_7_11, 8), _app(2, 7, 7, 11, X_7_12, 8)],
        [0, 0, 2, 4], [True, True]),
    "a proposal with the bit clear": (
        "leader", [RP.prop(1, 2, [(0, b"hello")])], [2], False, [], [0, 0, 0, 0], [False]),
}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_hand_table(oracle, name):
    state, rows, bits, lead, frames, peer_off, answered = TABLE[name]
    st = RP.leader_state(G, N, ME) if state == "leader" else L.candidate_state(G, N, ME)
    s, off = RP.frames(rows, ME)
    w = RP.want(st, s, off, None if bits is None else RP.bitmap(G, bits), lead=lead)
    got = [bytes(w["stream"][int(w["off"][k]):int(w["off"][k + 1])]).hex() for k in range(w["n_frames"])]
    assert got == frames, name
    assert list(w["peer_off"]) == peer_off and list(w["answered"]) == answered


def test_the_literal_frames_are_what_they_say():
    """(the table's own spelling: the first row's first frame, byte for byte)"""
    assert _app(1, 5, 3, 10, HELLO, 8) == ("000000000000002d" "0803" "1002" "1801" "2005" "2803" "300a" "3a0d" "0800" "1005" "180b" "2205"
                                           "68656c6c6f" "4008" "4a0812060a0010001800" "5000" "5800" "6001")


@functools.lru_cache(maxsize=None)
def _case(k):
    return RP.random_case(**RP.case_list()[k])


@pytest.mark.parametrize("k", range(len(RP.case_list())))
def test_every_gpu_case_tells_the_feature_from_its_absence(oracle, k):
    start, voters, s, off, at = _case(k)
    w = RP.want(V.copy_state(start), s, off, at, voters)
    got = RP.shows(w, w["rec"])
    for what, floor in RP.FLOORS.items():
        assert got[what] >= floor, (RP.case_list()[k], what, got)
    # ... and the bytes differ from the ones without the rule
    w_off = RP.want(V.copy_state(start), s, off, at, voters, props=False)
    assert w_off["taken"] == [] and bytes(w_off["stream"]) != bytes(w["stream"]) and w_off["answered"].sum() < w["answered"].sum()


@pytest.mark.parametrize("k", [0, 10, 30, len(RP.case_list()) - 7, len(RP.case_list()) - 5, len(RP.case_list()) - 4])
@pytest.mark.parametrize("lead", [False, True])
def test_with_the_rule_off_it_is_the_lead_reference(oracle, k, lead):
    """props = False: records, entry headers, slices and flags are ref_respond_lead.expected's (lead on), or -- with both off --
    tests/test_respond_gpu.expected's, which is ref_respond_lead's with no win answered"""
    from oracle import pywire as W
    from tests import ref_step_props as P

    start, voters, s, off, at = _case(k)
    st = V.copy_state(start)
    wm, we, _ = W.wire_decode(s, off)
    want_m, rec = P.node_filter(wm, we, st.G, st.N, st.self_peer, True, True)
    lt0 = st.last_term.copy()
    outs = P.step_batch(st, voters, rec)
    w, e, po, ans, wins, taken = RP.expected(rec, want_m, we, outs, lt0, at, st.N, st.self_peer, voters, lead=lead, props=False)
    assert taken == []
    if lead:
        w2, e2, po2, ans2, wins2 = L.expected(rec, outs, lt0, at, st.N, st.self_peer, voters)
        assert wins == wins2 and np.array_equal(e[["term", "index"]], e2[["term", "index"]])
    else:
        from tests.ref_bcast_members import expected as expected_members
        from tests.test_respond_gpu import expected as expected_off

        if voters is None:
            w2, po2, ans2 = expected_off(rec, outs, lt0, at, st.N, st.self_peer)
        else:
            w2, po2, ans2 = expected_members(rec, outs, lt0, at, st.N, st.self_peer, voters)[:3]
        assert wins == [] and len(e) == 0
    assert np.array_equal(w, w2) and np.array_equal(po, po2) and np.array_equal(ans, ans2)


def test_the_bound_holds_for_every_case_and_is_tight_for_an_entry(oracle):
    """RAFTQ_RESPOND_ENT_MAX from the marshal: an entry with every varint at its widest adds exactly 40 bytes beyond its payload; and
    no case's stream exceeds the header's bound"""
    from oracle import pywire as W

    big = np.uint64(2**64 - 1)
    m = np.zeros(1, W.WIRE_MSG_DT)
    m["type"], m["to"], m["from"], m["n_ents"] = 3, 1, 0, 1
    e = np.zeros(1, W.WIRE_ENT_DT)
    m0 = m.copy()
    m0["n_ents"] = 0
    bare = len(W.wire_encode(m0)[0])
    length = 1 << 21  # a three-byte data length is not the widest, a 2^28-byte payload is not a test: the length's varint grows by
    e["term"], e["index"], e["type"], e["data_len"] = big, big, 0xFFFFFFFF, length  # one byte per 7 bits, 5 bytes at 2^28 .. 2^32 - 1
    s, _ = W.wire_encode(m, e, np.zeros(length, np.uint8))
    # tag + entry length (4 bytes here, 5 from 2^28 on) + 4 tags + type 5 + term 10 + index 10 + data length (4 here, 5 from 2^28 on)
    assert len(s) - bare - length == RP.ENT_MAX - 2
    for k in (0, 10, len(RP.case_list()) - 1):
        start, voters, st_s, off, at = _case(k)
        w = RP.want(V.copy_state(start), st_s, off, at, voters)
        assert len(w["stream"]) <= RP.cap_bound(len(off) - 1, start.N, len(st_s), len(w["ents"]), False)
