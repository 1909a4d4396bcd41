"""CPU: tests/ref_tick_checks.py, the composed reference of tests/test_tick_checks_gpu.py, is itself checked: it equals each reference
it composes on that reference's own ground, and test_tick_elect_gpu.want_round with both switches off; a hand table of frame bytes
written out from the raftpb field numbers holds one MsgPreVote and one MsgVote frame against it (and shows that oracle.pywire
marshals type 17); every GPU case's inputs contain what tells the feature from its absence; and the header and the built library
carry the two new symbols."""
import os
import re

import numpy as np
import pytest

from oracle import pyoracle
from oracle import pywire as W
from tests import ref_check_quorum as Q
from tests import ref_pre_vote as PV
from tests import ref_step_voters as V
from tests import ref_tick_checks as R
from tests import ref_tick_members as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ET, SEED = R.ET, R.SEED
CASES = R.case_list()
_ids = lambda c: "-".join(str(v) for v in c)  # noqa: E731


def _state_equal(a, b):
    return not Q.state_differs(a, b)


# ---- 1. the composed reference against what it composes ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
def test_the_tick_is_ref_check_quorums(oracle, mode):
    """R.tick against ref_check_quorum.tick_scalar, the per-group statement, over the three ticks of a case's scenes"""
    for scene in R.scenes(mode, 129, 3):
        st, active, le = R.copy_case(scene["st"], scene["active"], scene["lead_elapsed"])
        for t in range(R.TICKS):
            want = Q.tick_scalar(oracle, st.role, st.elapsed, active, le, scene["voters"], st.self_peer, st.N, ET, scene["hb"], SEED, t)
            act = R.tick(st, active, le, scene["voters"], scene["hb"], t)
            assert np.array_equal(act, want[1]) and np.array_equal(st.elapsed, want[0])
            assert np.array_equal(active, want[2]) and np.array_equal(le, want[3])


@pytest.mark.parametrize("mode", R.MODES)
def test_the_campaigns_are_the_step_references(oracle, mode):
    """R.campaigns' results and state are ref_check_quorum.step_batch's / ref_pre_vote.step_batch's on the same MsgHup records"""
    from raftsql_amd import step as S

    scene = R.scenes(mode, 129, 5)[0]
    a, b = (R.copy_case(scene["st"], scene["active"], scene["lead_elapsed"]) for _ in range(2))
    act = R.tick(*a, scene["voters"], scene["hb"], 0)
    R.tick(*b, scene["voters"], scene["hb"], 0)
    hups = np.flatnonzero(act == 1)
    assert len(hups) >= 2
    _, _, camp, built, outs = R.campaigns(*a, scene["voters"], hups, len(hups) - 1, scene["pre_vote"])
    msgs = S.pack_msgs(hups[:-1].astype(np.uint64), R.MSG_HUP)
    step = PV.step_batch if scene["pre_vote"] else Q.step_batch
    want = step(b[0], scene["voters"], b[1], b[2], msgs, ET)
    assert outs.tobytes() == want.tobytes() and _state_equal(a, b) and np.array_equal(built, hups[:-1])
    assert np.array_equal(camp["type"], want["type"]) and np.array_equal(camp["term"], want["term"])
    # the last MsgHup group, beyond the cap, was not touched
    g = int(hups[-1])
    assert a[0].term[g] == scene["st"].term[g] and a[0].role[g] == scene["st"].role[g]


@pytest.mark.parametrize("n", [2, 3, 5])
def test_check_quorum_alone_campaigns_as_the_masked_step_does(oracle, n):
    """a MsgHup under CheckQuorum alone is Step's campaign plus a cleared activity word: the records, the slots and the state are
    ref_tick_members.member_campaigns' (ref_step_voters.step_batch) on the same input"""
    scene = R.scenes("cq_masks", 129, n)[0]
    a = R.copy_case(scene["st"], scene["active"], scene["lead_elapsed"])
    act = R.tick(*a, scene["voters"], scene["hb"], 0)
    b = V.copy_state(a[0])
    hups = np.flatnonzero(act == 1)
    w, keep, camp, built, outs = R.campaigns(*a, scene["voters"], hups, len(hups), False)
    w2, keep2, camp2, built2, outs2 = M.member_campaigns(b, scene["voters"], hups, len(hups))
    assert len(hups) > 0 and (outs["type"] == R.OUT_BECAME_LEADER).any() and (outs["type"] == R.OUT_CAMPAIGN).any()
    assert w.tobytes() == w2.tobytes() and np.array_equal(keep, keep2) and camp.tobytes() == camp2.tobytes() and outs.tobytes() == outs2.tobytes()
    assert _state_equal((a[0], a[1], a[2]), (b, a[1], a[2]))
    assert not a[1][built].any()  # reset() cleared the campaigned groups' activity words


@pytest.mark.parametrize("n,g", [(2, 129), (3, 3149), (5, 129)])
def test_switches_off_it_is_want_round(oracle, n, g):
    """with both switches off the composed round is test_tick_elect_gpu.want_round: records, peer_off, camp, state, bytes"""
    from tests import test_tick_elect_gpu as TE

    for hb in (1, 3):
        rng = np.random.default_rng(28500 + n + hb)
        st = TE.make_state(rng, g, n, int(rng.integers(0, n)), hb)
        a, b = V.copy_state(st), V.copy_state(st)
        for t in range(R.TICKS):
            hup_cap, beat_cap = (g, g) if t != 1 else (3, 2)
            r = R.round_(a, None, None, None, hb, t, hup_cap, beat_cap, False)
            el, act, _, _ = oracle.tick(b.role, b.elapsed, ET, hb, SEED, t)
            b.elapsed[:] = el
            want_w, want_po, want_camp, built, _ = TE.want_round(b, np.flatnonzero(act == 1), np.flatnonzero(act == 2), hup_cap, beat_cap)
            assert np.array_equal(r["act"], act) and r["w"].tobytes() == want_w.tobytes() and r["keep"].all()
            assert np.array_equal(r["po"], want_po) and r["camp"].tobytes() == want_camp.tobytes() and np.array_equal(r["built"], built)
            want_s, want_off = W.wire_encode(want_w) if len(want_w) else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
            assert bytes(r["stream"]) == bytes(want_s) and np.array_equal(r["off"][: len(want_off)], want_off)
            assert _state_equal((a, a.elapsed, a.elapsed), (b, b.elapsed, b.elapsed))


def test_no_check_due_and_no_pre_vote_is_want_round_too(oracle):
    """CheckQuorum on, but no check due within the ticks: what the switch adds to a tick and to a MsgHup shows nowhere in the round"""
    from tests import test_tick_elect_gpu as TE

    g, n, hb = 129, 3, 1
    rng = np.random.default_rng(28600)
    st = TE.make_state(rng, g, n, 1, hb)
    a, b = V.copy_state(st), V.copy_state(st)
    active, le = np.zeros(g, np.uint16), np.zeros(g, np.uint32)
    for t in range(R.TICKS):
        r = R.round_(a, active, le, None, hb, t, g, g, False)
        el, act, _, _ = oracle.tick(b.role, b.elapsed, ET, hb, SEED, t)
        b.elapsed[:] = el
        want_w, want_po, want_camp, _, _ = TE.want_round(b, np.flatnonzero(act == 1), np.flatnonzero(act == 2), g, g)
        assert len(r["checks"]) == 0 and r["w"].tobytes() == want_w.tobytes() and r["camp"].tobytes() == want_camp.tobytes()
        assert np.array_equal(r["po"], want_po)


# ---- 2. a hand table of frame bytes ------------------------------------------------------------------------------------------------
# a frame: 8-byte big-endian length | 08 type | 10 to+1 | 18 from+1 | 20 term | 28 logTerm | 30 index | 40 commit |
# 4a 08 12 06 0a 00 10 00 18 00 (the empty snapshot) | 50 reject | 58 rejectHint | 60 group
def _frame(type_, to, frm, term, log_term, index, group):
    body = ("08%02x" % type_ + "10%02x" % (to + 1) + "18%02x" % (frm + 1) + "20%02x" % term + "28%02x" % log_term + "30%02x" % index + "4000" +
            "4a0812060a0010001800" + "5000" + "5800" + "60%02x" % group)
    return "%016x" % (len(body) // 2) + body


# one follower of nobody (group 2 of three, N = 3, self = 0) at term 5 with its log at (9, term 4), its election timer about to fire
HAND = {
    # PreVote on: MsgPreVote (type 17 = 0x11) at term 6 = Term + 1; the term stays 5
    True: ([_frame(0x11, 1, 0, 6, 4, 9, 2), _frame(0x11, 2, 0, 6, 4, 9, 2)], 5, PV.PRE, R.OUT_PRE_CAMPAIGN),
    # PreVote off: MsgVote (type 5) at the new term 6
    False: ([_frame(0x05, 1, 0, 6, 4, 9, 2), _frame(0x05, 2, 0, 6, 4, 9, 2)], 6, 1, R.OUT_CAMPAIGN),
}


def _hand_state():
    st = pyoracle.NodeState(3, 3, 0)
    st.term[:], st.last_index[:], st.last_term[:] = 5, 9, 4
    st.match[0] = 9
    st.elapsed[2] = 2 * ET - 1
    return st, np.zeros(3, np.uint16), np.zeros(3, np.uint32)


@pytest.mark.parametrize("pre_vote", [True, False])
def test_hand_table(oracle, pre_vote):
    frames, term_after, role_after, out_type = HAND[pre_vote]
    st, active, le = _hand_state()
    r = R.round_(st, active, le, None, 1, 0, 3, 3, pre_vote)
    assert list(r["hups"]) == [2] and len(r["beats"]) == 0
    got = [bytes(r["stream"][int(r["off"][k]):int(r["off"][k + 1])]).hex() for k in range(r["frames"])]
    assert got == frames
    assert list(r["po"]) == [0, 0, 0, 0, 0, 0, 1, 2]
    c = r["camp"][0]
    assert (int(c["type"]), int(c["term"]), int(c["index"]), int(c["commit"]), int(c["role"])) == (out_type, term_after, 9, 4, role_after)
    assert int(c["flags"]) == R.OUTF_ANSWERED | (0 if pre_vote else R.OUTF_HARDSTATE)
    assert (int(st.term[2]), int(st.role[2])) == (term_after, role_after)
    # the records the frames were marshalled from say the same, and decode to themselves (type 17 through oracle.pywire both ways)
    w = r["w"]
    assert list(w["type"]) == [17 if pre_vote else 5] * 2 and list(w["term"]) == [6, 6] and list(w["to"]) == [1, 2]
    back, _, bad = W.wire_decode(r["stream"], r["off"][:3])
    assert bad == 0 and list(back["type"]) == list(w["type"]) and list(back["term"]) == [6, 6] and list(back["index"]) == [9, 9]


def test_the_literal_frames_are_what_they_say():
    """the table's own bytes, read back field by field with nothing but the varint rule"""
    raw = bytes.fromhex(HAND[True][0][0])
    assert int.from_bytes(raw[:8], "big") == len(raw) - 8
    body = raw[8:]
    fields, i = {}, 0
    while i < len(body):
        key = body[i]
        i += 1
        if key & 7 == 2:
            n = body[i]
            fields[key >> 3] = body[i + 1:i + 1 + n]
            i += 1 + n
        else:
            assert body[i] < 0x80
            fields[key >> 3] = body[i]
            i += 1
    assert (fields[1], fields[2], fields[3], fields[4], fields[5], fields[6], fields[8], fields[12]) == (17, 2, 1, 6, 4, 9, 0, 2)


# ---- 3. every GPU case discriminates -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_every_case_discriminates(oracle, case):
    mode, g, n = case[:3]
    c = R.shows(case)
    assert c["passed"] >= 1, c        # a check that is due and passes, its bits cleared
    assert c["failed"] >= 1, c        # one that fails: action 3 ...
    assert c["failed_beats"] == 0, c  # ... no beat and no heartbeat frame
    assert c["hups"] >= 1 and c["beats"] >= 1, c
    if "pv" in mode:
        assert c["pre_kept_term"] >= 1 and c["cand_to_pre"] >= 1, c
    else:
        assert c["campaigns"] >= 1, c
    if "masks" in mode:
        assert c["solo_wins"] >= 1 and c["empty_slots"] >= 1, c


@pytest.mark.parametrize("case", [c for c in CASES if len(c) == 4], ids=_ids)
def test_the_wide_cases_ask_above_2_63(oracle, case):
    """a wide64 case: device-built MsgPreVote frames -- asked at term + 1 -- with a term above 2^63, over tails and last terms above 2^62"""
    assert case[3] == "wide64" and "pv" in case[0] and CASES[-2:] == [c for c in CASES if len(c) == 4]
    high = asked = 0
    for scene in R.scenes(*case):
        st = scene["st"]
        assert int(st.term[0]) == 2**64 - 1 and int(st.role[0]) == 2 and int(st.term.min()) >= 2**62 and int(st.last_index.min()) >= 2**62
        for r in R.play(scene):
            w = r["w"][r["keep"]]
            pre = w[w["type"] == R.MSG_PRE_VOTE]
            high += int((pre["term"] > 2**63).sum())
            asked += int(((pre["index"] >= 2**62) & (pre["log_term"] >= 2**62)).sum())  # (under PreVote a Tick's MsgHup never asks by MsgVote)
            assert 0 not in r["built"]  # nobody campaigns from the top term
            before = r["before"][0].term[r["built"]]
            assert np.array_equal(r["outs"]["term"] + (r["outs"]["type"] == R.OUT_PRE_CAMPAIGN), before + np.uint64(1))  # every round asks at term + 1
    assert high >= 1 and asked >= 1, (high, asked)


# ---- 4. the switch's effect left out -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if "pv" in c[0]], ids=_ids)
def test_a_plain_campaign_would_differ(oracle, case):
    """a PreVote case whose MsgHup is stepped as a plain campaign gives other bytes and another state"""
    stream = camp = state = 0
    for scene in R.scenes(*case):  # (a G = 1 scene may hold a leader, or a one-voter group, whose pre-election IS the campaign)
        on, off = R.play(scene), R.play(scene, plain_hup=True)
        stream += any(bytes(a["stream"]) != bytes(b["stream"]) for a, b in zip(on, off))
        camp += any(a["camp"].tobytes() != b["camp"].tobytes() for a, b in zip(on, off))
        state += Q.state_differs(on[-1]["after"], off[-1]["after"])
    assert stream >= 1 and camp >= 1 and state >= 1, (stream, camp, state)


# ---- 5. the ABI --------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_both_symbols():
    from raftsql_amd import _lib

    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raftq.h")).read())
    assert "int raftq_tick_set_checks(raftq_t* h, uint64_t chk_cap);" in hdr
    assert "int raftq_last_tick_checks(raftq_t* h, const uint32_t** checks, uint64_t* n_listed, uint64_t* n_total);" in hdr
    lib = _lib.load()
    for name in ("raftq_tick_set_checks", "raftq_last_tick_checks"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.raftq_tick_set_checks(None, 1) != 0 and b"null handle" in lib.raftq_last_error(None)
    assert lib.raftq_last_tick_checks(None, None, None, None) != 0
