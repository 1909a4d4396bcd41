"""CPU: tests/ref_propose_forward.py, the reference of the GPU suite of raftq_propose_set_forward, is anchored three ways -- (a) a
hand table of frame bytes written out literally, (b) its outcome rule against what tests/ref_step_props.py's Step makes of the same
MsgProp from self at term 0, (c) its leader records against the rule of tests/test_wire_gpu.py::_propose_expect restated here -- and
every random case the GPU suite runs is checked to show what it is meant to (ref_propose_forward.assert_shows)."""
import functools
import types

import numpy as np
import pytest

from oracle import pyoracle
from oracle import pywire as W
from tests import ref_bcast_members as B
from tests import ref_propose_forward as PF
from tests import ref_step_props as P
from tests import ref_step_voters as V

# a frame: 8-byte big-endian length | 08 type | 10 to+1 | 18 from+1 | 20 term | 28 logTerm | 30 index | 3a len entry ... | 40 commit |
# 4a 08 12 06 0a 00 10 00 18 00 (the empty snapshot) | 50 reject | 58 rejectHint | 60 group;  an entry: 08 type | 10 term | 18 index |
# 22 len data (left out when the data is empty)
SNAP = "4a0812060a0010001800"


def _prop(to, frm, ents, group):
    body = "0802" + "10%02x" % (to + 1) + "18%02x" % (frm + 1) + "2000" + "2800" + "3000" + ents + "4000" + SNAP + "5000" + "5800" + "60" + group
    return "%016x" % (len(body) // 2) + body


ABC = "3a0b" "0800" "1000" "1800" "2203" "616263"  # {EntryNormal, Term 0, Index 0, "abc"}
NO_DATA = "3a06" "0800" "1000" "1800"              # {EntryNormal, Term 0, Index 0, no Data field}
CONF_HI = "3a0a" "0801" "1000" "1800" "2202" "6869"  # {EntryConfChange, Term 0, Index 0, "hi"}
BIG = (1 << 32) + 5  # a group id above 2^32: the varint 85 80 80 80 10

# name -> (self, the group, its leader's slot, the entries as (type, payload), the frame, the run it lies in)
TABLE = {
    "self 1 forwards one 3-byte entry to slot 0": (1, 1, 0, [(0, b"abc")], _prop(0, 1, ABC, "01"), 0),
    "self 1 forwards to slot 2": (1, 1, 2, [(0, b"abc")], _prop(2, 1, ABC, "01"), 1),
    "self 2 forwards two entries, one with no Data and one of type 1": (2, 3, 1, [(0, b""), (1, b"hi")], _prop(1, 2, NO_DATA + CONF_HI, "03"), 1),
    "self 2, a group id above 2^32": (2, BIG, 0, [(0, b"abc")], _prop(0, 2, ABC, "8580808010"), 0),
    "self 1, a group id above 2^32, two entries": (1, BIG, 2, [(1, b"hi"), (0, b"")], _prop(2, 1, CONF_HI + NO_DATA, "8580808010"), 1),
}


def test_the_literal_frames_are_what_they_say():
    """(the table's own spelling: the first row's frame, byte for byte)"""
    assert TABLE["self 1 forwards one 3-byte entry to slot 0"][4] == (
        "000000000000002b" "0802" "1001" "1802" "2000" "2800" "3000" "3a0b" "0800" "1000" "1800" "2203" "616263" "4000"
        "4a0812060a0010001800" "5000" "5800" "6001")


def _sparse(me, g, lead):
    """one follower group of an N = 3 node, as the dicts expect() indexes (a group id above 2^32 fits no array)"""
    return types.SimpleNamespace(N=3, self_peer=me, role={g: PF.FOLLOWER}, lead={g: lead + 1}, term={g: 7}, last_index={g: 10}, last_term={g: 6},
                                 committed={g: 9})


@pytest.mark.parametrize("name", sorted(TABLE))
def test_hand_table(oracle, name):
    me, g, lead, entries, frame, run = TABLE[name]
    props = np.zeros(1, PF.PROP_DT)
    props["group"], props["n_ents"] = g, len(entries)
    pe = np.zeros(len(entries), PF.PROP_ENT_DT)
    pool = bytearray(b"\xee" * 5)
    for k, (typ, data) in enumerate(entries):
        pe[k]["data_off"], pe[k]["data_len"], pe[k]["type"] = len(pool), len(data), typ
        pool += data
    s = _sparse(me, g, lead)
    w = PF.want(s, None, props, pe, np.frombuffer(bytes(pool), np.uint8), np.zeros(0, W.WIRE_MSG_DT), np.zeros(0, W.WIRE_ENT_DT))
    assert list(w["what"]) == [PF.FORWARDED] and list(w["to"]) == [lead] and w["n_frames"] == 1
    # N - 1 = 2 runs of one slot: the frame in its leader's run, the other slot of zero length
    assert list(w["off"]) == ([0, len(frame) // 2, len(frame) // 2] if run == 0 else [0, 0, len(frame) // 2])
    assert bytes(w["stream"]).hex() == frame, name
    assert (s.last_index[g], s.last_term[g], s.committed[g]) == (10, 6, 9)  # nothing of the group's state moves


def test_hand_table_drops(oracle):
    """a candidate, a follower without a leader and a follower whose lead is itself: no frame, every slot of zero length"""
    for role, lead in ((PF.CANDIDATE, 0), (PF.FOLLOWER, 0), (PF.FOLLOWER, 2), (PF.CANDIDATE, 1)):
        s = _sparse(1, 4, lead - 1)
        s.role[4] = role
        props = np.zeros(1, PF.PROP_DT)
        props["group"], props["n_ents"] = 4, 1
        pe = np.zeros(1, PF.PROP_ENT_DT)
        pe["data_len"] = 3
        w = PF.want(s, None, props, pe, np.frombuffer(b"abc", np.uint8), np.zeros(0, W.WIRE_MSG_DT), np.zeros(0, W.WIRE_ENT_DT))
        assert list(w["what"]) == [PF.DROPPED] and list(w["off"]) == [0, 0, 0] and len(w["stream"]) == 0 and w["n_frames"] == 0


# ---- the random cases of the GPU suite ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(kind, k):
    return PF.parity_case(k) if kind == "parity" else PF.masked_case(k)


CASES = [("parity", k) for k in range(len(PF.PARITY))] + [("masked", k) for k in range(len(PF.MASKED))]


@pytest.mark.parametrize("kind,k", CASES)
def test_every_gpu_case_shows_what_it_is_meant_to(oracle, kind, k):
    c = _case(kind, k)
    PF.assert_shows(c, (kind, k))
    if kind == "masked":
        got = PF.masked_shows(c)
        assert got["forwards to a non-member leader"] >= 1 and got["forwards from a non-member self"] >= 1, got
        # (the two member refusals are not what these cases are about: no leader record meets one)
        led = c["props"][c["want"]["what"] == PF.APPENDED]
        assert (B.propose_verdict(c["s0"], c["voters"], led) == 0).all()
        if c["mix"] == "mixed":  # ... and a leader record with a non-member slot in the same call
            assert got["leader records with a non-member slot"] >= 1 and PF.shows(c)["member fillers among the leaders' slots"] >= 1, got
    w = c["want"]
    # the layout: one offset per slot and one more, fillers of zero length, the frames that have bytes counted
    n_slots = len(c["hm"]) + len(c["props"]) * (c["N"] - 1)
    assert len(w["off"]) == n_slots + 1 and int(w["off"][-1]) == len(w["stream"])
    assert ((np.diff(w["off"].astype(np.int64)) > 0) == w["keep"]).all()
    # a forwarded record has bytes in exactly one run, a dropped one in none, a leader's in every member's
    per_rec = w["keep"][len(c["hm"]):].reshape(c["N"] - 1, len(c["props"])).sum(axis=0)
    assert (per_rec[w["what"] == PF.FORWARDED] == 1).all() and (per_rec[w["what"] == PF.DROPPED] == 0).all()
    if c["voters"] is None:
        assert (per_rec[w["what"] == PF.APPENDED] == c["N"] - 1).all()


@pytest.mark.parametrize("kind,k", CASES)
def test_outcomes_are_what_step_makes_of_the_same_msgprop(oracle, kind, k):
    """(b) every group of the case, not only the proposed ones: a MsgProp from self at term 0 through tests/ref_step_props.py --
    PROPOSED <-> APPENDED, FORWARD <-> FORWARDED with the same `to`, NONE <-> DROPPED.  The one stated exception: a follower whose lead
    is itself, which Step hands on to itself and the rule drops (the header's CHOICE)."""
    c = _case(kind, k)
    s0, me = c["s0"], c["me"]
    G = s0.G
    m = np.zeros(G, pyoracle.STEP_MSG_DT)
    for g in range(G):
        P._prop(m, g, g, 1, term=0, frm=me)
    if c["voters"] is not None:  # (the masked Step of a group self leads needs self among its voters, as the call does: the others only)
        ok = (s0.role != PF.LEADER) | (((c["voters"] >> np.uint16(me)) & 1) == 1)
        m = m[ok]
    outs = P.step_batch(V.copy_state(s0), c["voters"], m)
    n_exc = 0
    for o, g in zip(outs, m["group"].astype(np.int64)):
        got, to = PF.outcome(int(s0.role[g]), int(s0.lead[g]), me)
        t = int(o["type"])
        if s0.role[g] == PF.FOLLOWER and s0.lead[g] == me + 1:
            assert t == P.OutForward and int(o["to"]) == me and got == PF.DROPPED
            n_exc += 1
        elif t == P.OutProposed:
            assert got == PF.APPENDED
        elif t == P.OutForward:
            assert got == PF.FORWARDED and int(o["to"]) == to
        else:
            assert t == 0 and got == PF.DROPPED  # RAFTQ_OUT_NONE
    if c["mix"] in ("dropped", "mixed"):
        assert n_exc >= 1


def _leader_rule(st, N, me, props, pe, n_hm, n_he):
    """tests/test_wire_gpu.py::_propose_expect restated for the records of led groups: -> {(record, run): the MsgApp's fields},
    {entry: (term, index, data_len, data_off, type)}, the new tails"""
    msgs, ents, tails = {}, {}, {}
    for i, p in enumerate(props):
        g, k, f = int(p["group"]), int(p["n_ents"]), int(p["ent_first"])
        if st.role[g] != 2:
            continue
        for j in range(k):
            ents[n_he + f + j] = (int(st.term[g]), int(st.last_index[g]) + 1 + j, int(pe["data_len"][f + j]),
                                  int(pe["data_off"][f + j]) if pe["data_len"][f + j] else 0, int(pe["type"][f + j]))
        run = 0
        for to in range(N):
            if to == me:
                continue
            msgs[(i, run)] = dict(group=g, term=int(st.term[g]), log_term=int(st.last_term[g]), index=int(st.last_index[g]), commit=int(st.committed[g]),
                                  to=to, type=3, ent_first=n_he + f, n_ents=k, **{"from": me})
            run += 1
        tails[g] = (int(st.last_index[g]) + k, int(st.term[g]))
    return msgs, ents, tails


@pytest.mark.parametrize("kind,k", CASES)
def test_leader_records_are_the_existing_rule(oracle, kind, k):
    """(c) ... and everything that is no leader's record is a MsgProp with nothing but group, from, to and its entries; the state
    after: the leaders' tails and own Match, nothing else"""
    c = _case(kind, k)
    w, s0, after, N, me = c["want"], c["s0"], c["after"], c["N"], c["me"]
    n_props, n_hm, n_he = len(c["props"]), len(c["hm"]), len(c["he"])
    msgs, ents, tails = _leader_rule(s0, N, me, c["props"], c["pe"], n_hm, n_he)
    for (i, run), f in msgs.items():
        got = w["msgs"][n_hm + run * n_props + i]
        assert {k_: int(got[k_]) for k_ in f} == f and int(got["reject"]) == 0 and int(got["reject_hint"]) == 0
    for at, f in ents.items():
        e = w["ents"][at]
        assert (int(e["term"]), int(e["index"]), int(e["data_len"]), int(e["data_off"]), int(e["type"])) == f
    led = np.repeat(w["what"] == PF.APPENDED, c["props"]["n_ents"])
    rest = w["ents"][n_he:][~led]
    assert (rest["term"] == 0).all() and (rest["index"] == 0).all()
    others = w["msgs"][n_hm:][~np.tile(w["what"] == PF.APPENDED, N - 1)]
    for f in ("term", "log_term", "index", "commit", "reject", "reject_hint"):
        assert (others[f] == 0).all(), f
    assert (others["type"] == 2).all() and (others["from"] == me).all()
    assert np.array_equal(w["msgs"][:n_hm], c["hm"]) and np.array_equal(w["ents"][:n_he], c["he"])
    want_last, want_lt, want_match = s0.last_index.copy(), s0.last_term.copy(), s0.match.copy()
    for g, (last, term) in tails.items():
        want_last[g], want_lt[g] = last, term
        want_match[me, g] = max(int(want_match[me, g]), last)
    assert np.array_equal(after.last_index, want_last) and np.array_equal(after.last_term, want_lt) and np.array_equal(after.match, want_match)
    for f in ("term", "vote", "lead", "role", "committed", "first_idx", "elapsed", "votes"):
        assert np.array_equal(getattr(after, f), getattr(s0, f)), f
    assert set(tails) == set(int(g) for g in c["props"]["group"][w["what"] == PF.APPENDED])
