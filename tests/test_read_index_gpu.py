"""GPU: ReadIndex (raftq_set_read_index; the rules in NodeT::step of every *_cq_* walk and in read_rule(), the two kinds in classify()
and in the frames calls' filter, the echo in respond(), the read records) against tests/ref_read_index.py: every result byte, every
word of state, the activity arrays, the transferees, seq / acked / confirmed.

Step shapes (the issue's): G = 194 groups -- a partial wave --, batches of 512 records, N in {3, 5, 9}, self in the first and in the
last slot, over every slot and over voter masks, PreVote and leadership transfer on and off, both modes.  N = 9 with nine distinct
acknowledgement words; seq loaded at 2^32 - 2; a batch with 40 records of one group (more than kMaxRun = 32: the sorted walk) with
three requests and their acknowledgements out of order; a one-voter masked group released at once; a closed gate; a higher-term
MsgApp in the middle of a batch; a non-voter's acknowledgement.  What each Step input shows of the feature is asserted on the
reference alone by tests/test_read_index_ref.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle
from raftsql_amd._lib import RAFTQ_EINVAL, RAFTQ_ESTATE, READ_LEASE, READ_SAFE
from raftsql_amd.engine import RaftqError
from tests import _stepgen
from tests import ref_check_quorum as Q
from tests import ref_lead_transfer as T
from tests import ref_raft_py as R
from tests import ref_read_index as RI
from tests import ref_step_props as P
from tests import ref_step_voters as V

pytestmark = pytest.mark.gpu

CASES = RI.case_list()
HOT = [c for c in CASES if c.get("hot")]
SEED = 0x5EED
ANSWERED = 0x10
NEW_KINDS = (RI.MsgReadIndex, RI.MsgReadIndexResp)
assert (READ_SAFE, READ_LEASE) == (RI.SAFE, RI.LEASE)


def _pick(**kw):
    """the first case of the list with these arguments"""
    return next(c for c in CASES if all(c.get(k, d) == v for k, (v, d) in kw.items()))


@pytest.fixture(scope="module")
def S(gpu_engine_cls):
    from raftsql_amd import step

    return step


@functools.lru_cache(maxsize=None)
def _case(key):
    return RI.step_case(**dict(key))


def _key(kw):
    return tuple(sorted(kw.items()))


def _engine(S, s, voters, x, mode=RI.SAFE, pre_vote=True, lead_transfer=True, cls=None, election_tick=Q.ELECTION_TICK, heartbeat_tick=1, seed=SEED):
    e = (cls or S.NodeEngine)(s.G, s.N, s.self_peer)
    e.set_timers(election_tick, heartbeat_tick, seed)
    e.set_check_quorum(True)
    e.set_step_props(True)
    if pre_vote:
        e.set_pre_vote(True)
    if lead_transfer:
        e.set_lead_transfer(True)
    e.set_read_index(mode)
    _stepgen.load_engine(e, s)
    if voters is not None:
        e.load_voters(voters)
        e.set_step_voters(True)
    e.load_activity(x.active, x.lead_elapsed)
    if lead_transfer:
        e.load_transfer(x.transferee)
    if mode == RI.SAFE:
        e.load_reads(x.seq, x.acked)
    return e


def _same_records(got, want, msgs, what=""):
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        k = got.dtype.itemsize
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, k) != want.view(np.uint8).reshape(-1, k)).any(axis=1))
        assert False, (what, len(bad), int(bad[0]), None if msgs is None else msgs[bad[0]], got[bad[0]], want[bad[0]])


def _same_after(e, after, voters, mode=RI.SAFE, lead_transfer=True, what=""):
    s, x = after
    _stepgen.assert_same_state(e, s)
    a, le = e.read_activity()
    assert np.array_equal(a, x.active), (what, "active")
    assert np.array_equal(le, x.lead_elapsed), (what, "lead_elapsed")
    if lead_transfer:
        assert np.array_equal(e.read_transfer(), x.transferee), (what, "transferee")
    if mode == RI.SAFE:
        seq, acked, conf = e.read_reads()
        assert np.array_equal(seq, x.seq), (what, "seq", np.flatnonzero(seq != x.seq)[:8])
        assert np.array_equal(acked, x.acked), (what, "acked")
        assert np.array_equal(conf, RI.confirmed_of(x, voters, s.N)), (what, "confirmed")


def _code(f, *args, **kw):
    with pytest.raises(RaftqError) as ei:
        f(*args, **kw)
    return ei.value.code, str(ei.value)


# ---- Step --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CASES, ids=RI.case_id)
def test_step_batch_against_the_reference(S, kw):
    start, voters, m, want, after = _case(_key(kw))
    sw = RI.case_switches(kw)
    with _engine(S, start[0], voters, start[1], **sw) as e:
        got, _ = e.step_batch(np.array(m))
        _same_records(got, want, m, kw)
        _same_after(e, after, voters, sw["mode"], sw["lead_transfer"], kw)


def _unpacked(S, m40):
    m = np.zeros(len(m40), S.MSG_DT)
    for k in ("group", "from", "type", "reject", "term", "index", "commit"):
        m[k] = m40[k]
    hint = m40["type"] == S.MSG_APP_RESP
    m["log_term"], m["reject_hint"] = np.where(hint, 0, m40["aux"]), np.where(hint, m40["aux"], 0)
    return m


@pytest.mark.parametrize("kw", [_pick(n=(3, 0), self_peer=(0, 0), masks=(False, False)), _pick(n=(9, 0), self_peer=(8, 0), masks=(True, False)),
                                _pick(mode=(RI.LEASE, RI.SAFE)), HOT[0], _pick(band=("b32", None), masks=(True, False))], ids=RI.case_id)
def test_step_packed_records_and_result_formats(S, kw):
    """the 40-byte inbound record takes types 15 and 16 and a heartbeat's context; the three result formats say the same: log_term
    rides the commit slot of RAFTQ_OUT_READ_INDEX and of a RAFTQ_OUT_PROGRESS with RAFTQ_OUTF_READ_READY (a packed record carries no
    RAFTQ_MSGF_*, so no MsgProp: the batch goes without them)"""
    start, voters, m, _, _ = _case(_key(kw))
    sw = RI.case_switches(kw)
    m = np.array(m)
    m40 = S.pack_msgs40(m[m["type"] != P.MsgProp])
    m = _unpacked(S, m40)
    after = RI.copy_start(start)
    want = RI.step_batch(after[0], voters, after[1], m, **sw)
    assert np.isin((S.OUT_READ_INDEX, S.OUT_READ_STATE, S.OUT_FORWARD), want["type"]).all()
    ready = (want["type"] == S.OUT_PROGRESS) & ((want["flags"] & S.OUTF_READ_READY) != 0)
    assert sw["mode"] == RI.LEASE or (ready.sum() >= 4 and (want["commit"][ready] != want["log_term"][ready]).any())
    for fmt in (0, 1, 2):
        with _engine(S, start[0], voters, start[1], **sw) as e:
            e.set_compact(fmt)
            e.step_submit_packed(m40)
            recs, _ = e.step_collect()
            exp = want
            if fmt == 0:
                got = recs
            elif fmt == 1:
                got = S.expand_compact(np.array(m), recs)
                reads = (recs["type"] == S.OUT_READ_INDEX) | ((recs["type"] == S.OUT_PROGRESS) & ((recs["flags"] & S.OUTF_READ_READY) != 0))
                assert np.array_equal(recs["commit"][reads], want["log_term"][reads])  # the slot itself
                exp = want.copy()
                exp["commit"][ready] = 0  # (not delivered by the 40-byte record: a MsgHeartbeatResp moves no commit index)
            else:
                got = S.expand_short(np.array(m), recs, start[0].last_index, start[0].committed)
            _same_records(got, exp, m, (kw, fmt))
            _same_after(e, after, voters, sw["mode"], sw["lead_transfer"], (kw, fmt))


@pytest.mark.parametrize("walk", ["lists", "sort"])
def test_step_both_walks(S, monkeypatch, walk):
    """a batch with 40 records of one group takes the sorted walk by itself; RAFTQ_STEP_WALK=sort sends every batch there"""
    if walk == "sort":
        monkeypatch.setenv("RAFTQ_STEP_WALK", "sort")
    else:
        monkeypatch.delenv("RAFTQ_STEP_WALK", raising=False)
    for kw in HOT + [_pick(n=(5, 0), self_peer=(4, 0), masks=(True, False)), _pick(band=("b63", None), masks=(False, False))]:  # (HOT: a b32 case too)
        start, voters, m, want, after = _case(_key(kw))
        sw = RI.case_switches(kw)
        assert not kw.get("hot") or np.bincount(m["group"].astype(np.int64)).max() > 32
        with _engine(S, start[0], voters, start[1], **sw) as e:
            got, _ = e.step_batch(np.array(m))
            _same_records(got, want, m, (kw, walk))
            _same_after(e, after, voters, sw["mode"], sw["lead_transfer"], (kw, walk))


def _leaders(n, me, g, term=4, tail=9):
    """g led groups at term 4 with a log of 9 entries, 7 of them committed, the gate open"""
    s = pyoracle.NodeState(g, n, me)
    s.term[:], s.vote[:], s.lead[:], s.role[:], s.last_index[:], s.last_term[:], s.first_idx[:], s.committed[:] = term, me + 1, me + 1, 2, tail, term, 1, tail - 2
    s.match[:] = tail
    return s


def test_pipelined_three_in_flight(S):
    """submit / collect, three in flight: the requests in one batch, the acknowledgements of their round in the next, a beat and a
    late acknowledgement in the third -- each walk reads the record the one before it wrote"""
    n, me, g = 5, 0, 64
    s, x = _leaders(n, me, g), RI.zero_extra(g, n)
    grp = np.arange(g, dtype=np.uint64)
    b1 = np.concatenate([S.pack_msgs(grp, S.MSG_READ_INDEX, frm=me), S.pack_msgs(grp[::2], S.MSG_READ_INDEX, term=4, frm=3)])
    b2 = np.concatenate([S.pack_msgs(grp, S.MSG_HEARTBEAT_RESP, term=4, frm=1, index=1), S.pack_msgs(grp, S.MSG_HEARTBEAT_RESP, term=4, frm=2, index=1)])
    b3 = np.concatenate([S.pack_msgs(grp, S.MSG_BEAT), S.pack_msgs(grp, S.MSG_HEARTBEAT_RESP, term=4, frm=4, index=2)])
    start = (V.copy_state(s), x.copy())
    w1, w2, w3 = (RI.step_batch(s, None, x, b) for b in (b1, b2, b3))
    assert (w1["type"] == S.OUT_READ_INDEX).all() and (w1["flags"] == 0).all() and (w1["index"] == 7).all()
    assert ((w2["flags"][g:] & S.OUTF_READ_READY) != 0).all() and (w2["log_term"][g:] == 1).all() and (w2["flags"][:g] & S.OUTF_READ_READY == 0).all()
    assert np.array_equal(w3["index"][:g], np.where(np.arange(g) % 2 == 0, 2, 0)) and (w3["flags"][g:] & S.OUTF_READ_READY == 0).all()
    with _engine(S, start[0], None, start[1]) as e:
        for b in (b1, b2, b3):
            e.step_submit(b)
        assert _code(e.set_read_index, 0)[0] == RAFTQ_ESTATE  # a batch in flight
        assert _code(e.read_reads)[0] == RAFTQ_ESTATE
        for b, w in ((b1, w1), (b2, w2), (b3, w3)):
            got, _ = e.step_collect()
            _same_records(got, w, b, "pipelined")
        _same_after(e, (s, x), None, what="pipelined")


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def _node_filter(wm, we, g, n, me):
    """ref_step_props.node_filter (raftq_step_set_props is on) with what the header says the switches change: frames of types 13 to
    18 are kinds a peer sends, checked as MsgVoteResp is and flagged as little -- a MsgReadIndex with its context entry too.  (A
    case holds the kinds of a switch only where that switch is on: step_case plants MsgPreVoteResp under pre_vote alone.)"""
    from tests import ref_pre_vote as PV

    plain = wm.copy()
    new = np.isin(wm["type"], NEW_KINDS + (T.MsgTransferLeader, T.MsgTimeoutNow, PV.MsgPreVote, PV.MsgPreVoteResp))
    plain["type"] = np.where(new, R.MsgVoteResp, wm["type"])
    out, rec = P.node_filter(plain, we, g, n, me, True, True)
    out["type"] = rec["type"] = wm["type"]
    return out, rec


def _with_contexts(m):
    """every MsgReadIndex says that it carries one entry -- its context -- so that frames_of gives its frame one"""
    m = np.array(m)
    req = m["type"] == RI.MsgReadIndex
    m["_pad"][req, 1] |= V.MSGF_ENTRIES
    m["_resv"][req] = 1
    return m


@pytest.mark.parametrize("kw", [_pick(n=(3, 0), self_peer=(2, 0), masks=(False, False)), _pick(n=(9, 0), self_peer=(0, 0), masks=(True, False)),
                                _pick(band=("top", None), masks=(True, False))], ids=RI.case_id)
def test_step_frames_and_packed(S, kw):
    """raftq_step_frames and raftq_step_frames_packed over a stream holding frames of types 15 and 16 among the usual kinds: the
    decoded records against the codec oracle (the filter's flags restated), results and state against the reference"""
    from oracle import pywire as W
    from raftsql_amd import wire
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from tests import packed_rule

    start, voters, m, _, _ = _case(_key(kw))
    sw = RI.case_switches(kw)
    s0, me = start[0], start[0].self_peer
    stream, off = P.frames_of(np.random.default_rng(78), _with_contexts(m), me, empty_props=0.0)
    wm, we, bad = W.wire_decode(stream, off)
    assert bad == 0 and np.isin(wm["type"], NEW_KINDS).sum() >= 40
    assert (wm["n_ents"][wm["type"] == RI.MsgReadIndex] == 1).all()
    if kw.get("band") == "top":  # every term on the wire and every position is a ten-byte varint
        pos = np.isin(wm["type"], (R.MsgApp, R.MsgAppResp, R.MsgVote, RI.MsgReadIndexResp))
        assert (wm["term"][wm["term"] != 0] >= 2**63).all() and (wm["index"][pos & (wm["index"] != 0)] >= 2**63).mean() > 0.9
    want_m, rec = _node_filter(wm, we, s0.G, s0.N, me)
    new = np.isin(want_m["type"], NEW_KINDS)
    assert ((want_m["flags"][new] & (V.MSGF_SKIP | V.MSGF_HOLD | V.MSGF_ENTRIES | V.MSGF_BARRIER)) == 0).all() and ((want_m["flags"] & V.MSGF_SKIP) != 0).any()
    after = RI.copy_start(start)
    want_o = RI.step_batch(after[0], voters, after[1], rec, **sw)
    assert np.isin((S.OUT_READ_INDEX, S.OUT_READ_STATE, S.OUT_FORWARD), want_o["type"]).all() and ((want_o["flags"] & S.OUTF_READ_READY) != 0).any()
    n = len(wm)
    ps, po = pinned_copy(np.ascontiguousarray(stream)), pinned_copy(np.ascontiguousarray(off, np.uint64))
    with _engine(S, s0, voters, start[1], cls=wire.WireEngine, **sw) as e:
        gm, ge, go, c = e.step_frames(ps, po, pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT))
        assert (c.n_msgs, c.n_ents, c.n_malformed, c.bytes) == (n, len(we), 0, len(stream))
        _same_records(gm, want_m, None, "records")
        _same_records(ge, we, None, "entry headers")
        _same_records(go, want_o, rec, "results")
        _same_after(e, after, voters, sw["mode"], sw["lead_transfer"], "frames")
    for form in (packed_rule.FORM_40, packed_rule.FORM_HEAD):
        ht = packed_rule.RESPONSE_KINDS if form == packed_rule.FORM_HEAD else 0
        want_narrow, want_wide = packed_rule.pack(want_m, me, form, ht)
        with _engine(S, s0, voters, start[1], cls=wire.WireEngine, **sw) as e:
            narrow, wide, ge, go, c, n_wide = e.step_frames_packed(ps, po, form, pinned_empty(n, wire._FORM_DT[form]), pinned_empty(len(want_wide) + 1, W.WIRE_MSG_DT),
                                                                   pinned_empty(len(we) + 1, W.WIRE_ENT_DT), head_types=ht)
            assert n_wide == len(want_wide) and (want_wide["type"] == RI.MsgReadIndex).sum() == (wm["type"] == RI.MsgReadIndex).sum()  # a frame with entries is wide
            _same_records(narrow, want_narrow, None, ("narrow", form))
            _same_records(wide, want_wide, None, ("wide", form))
            _same_records(go, want_o, rec, ("results", form))
            _same_after(e, after, voters, sw["mode"], sw["lead_transfer"], ("packed", form))
    # without the switch the two kinds stay frames of a kind a peer never sends
    with _engine(S, s0, voters, start[1], cls=wire.WireEngine, **dict(sw, mode=0)) as e:
        gm, _, go, _ = e.step_frames(ps, po, pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT))
        assert ((gm["flags"][new] & V.MSGF_SKIP) != 0).all() and (go["type"][new] == V.OutSkipped).all()


def _wire_records(g, me, frm, term, kinds, index):
    from oracle import pywire as W

    w = np.zeros(g, W.WIRE_MSG_DT)
    w["group"], w["to"], w["from"], w["term"], w["type"], w["index"] = np.arange(g), me, frm, term, kinds, index
    return w


def test_step_submit_wire_takes_the_two_kinds(S):
    from oracle import pywire as W
    from raftsql_amd.wire import WireEngine

    n, me, g = 3, 1, 32
    s = _leaders(n, me, g)
    fol = np.arange(g) >= g // 2
    s.role[fol], s.lead[fol], s.vote[fol], s.first_idx[fol] = 0, 1, 0, 0
    s.match[0, fol] = s.match[2, fol] = 0
    w = _wire_records(g, me, 0, 4, np.where(fol, RI.MsgReadIndexResp, RI.MsgReadIndex), np.where(fol, 6, 0))
    stream, off = W.wire_encode(w, np.zeros(0, W.WIRE_ENT_DT), np.zeros(1, np.uint8))
    rec = np.zeros(g, S.MSG_DT)
    for k in ("group", "term", "log_term", "index", "from", "type"):
        rec[k] = w[k]
    x = RI.zero_extra(g, n)
    start = (V.copy_state(s), x.copy())
    want = RI.step_batch(s, None, x, rec)
    assert (want["type"][~fol] == S.OUT_READ_INDEX).all() and (want["log_term"][~fol] == 1).all() and (want["to"][~fol] == 0).all()
    assert (want["type"][fol] == S.OUT_READ_STATE).all() and (want["index"][fol] == 6).all()
    with _engine(S, start[0], None, start[1], cls=WireEngine) as e:
        e.step_submit_wire(stream, off)
        got, _ = e.step_collect()
        _same_records(got, want, rec, "submit_wire")
        _same_after(e, (s, x), None, what="submit_wire")
    with _engine(S, start[0], None, start[1], mode=0, cls=WireEngine) as e:
        e.step_submit_wire(stream, off)
        assert _code(e.step_collect)[0] == RAFTQ_EINVAL  # an unknown kind fails its batch


def test_frames_respond_echoes_the_context_and_leaves_reads_to_the_host(S):
    """raftq_step_frames_respond: a device-built MsgHeartbeatResp carries Index = the heartbeat's -- byte for byte raftq_wire_encode of
    host-built records, in both modes, a zero context among them --; RAFTQ_OUT_READ_INDEX, RAFTQ_OUT_READ_STATE and a forwarded read
    carry no RAFTQ_OUTF_ANSWERED and end their group's device-answered prefix; RAFTQ_OUTF_READ_READY ends none"""
    _frames_respond(S, 4, 9, None)


def test_frames_respond_echoes_the_context_at_b63(S):
    """the same at a term of 2^63 + 1 over a log that ends at 2^63 + 2: every echoed frame holds the context 2^32 + 7 (or the
    next one) in a five-byte varint beside a ten-byte term"""
    _frames_respond(S, 2**63 + 1, 2**63 + 2, 2**32 + 7)


def _frames_respond(S, term, tail, context):
    from oracle import pywire as W
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from raftsql_amd.wire import WIRE_ENT_DT, WIRE_MSG_DT, WireEngine

    n, me, g = 3, 1, 48
    kind = np.arange(g) % 6  # 0, 1: following, heartbeats only | 2: following, a read state first | 3: following, a forwarded read first
    led = kind >= 4          # 4: led, a request first | 5: led with a request pending, the completing acknowledgement first
    s = _leaders(n, me, g, term, tail)
    s.role[~led], s.lead[~led], s.vote[~led], s.first_idx[~led] = 0, 3, 0, 0
    s.match[0, ~led] = s.match[2, ~led] = 0
    x = RI.zero_extra(g, n)
    x.seq[kind == 5], x.acked[me, kind == 5] = 1, 1
    ctx = (np.arange(g, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x10000001)  # zero, small and beyond 2^32
    if context is not None:
        ctx[:] = context
    ctx[kind == 0] = 0
    first_index = ctx.copy()
    first_index[kind == 2], first_index[kind == 3], first_index[kind == 4], first_index[kind == 5] = tail - 2, 0, 0, 1
    first = _wire_records(g, me, 2, term, np.choose(kind, [R.MsgHeartbeat, R.MsgHeartbeat, RI.MsgReadIndexResp, RI.MsgReadIndex, RI.MsgReadIndex, R.MsgHeartbeatResp]),
                          first_index)
    second_index = ctx + np.uint64(1)
    second_index[led] = 0
    second = _wire_records(g, me, 2, term, np.where(led, R.MsgHeartbeatResp, R.MsgHeartbeat), second_index)
    w = np.concatenate([first, second])
    stream, off = W.wire_encode(w, np.zeros(0, W.WIRE_ENT_DT), np.zeros(1, np.uint8))
    at_tail = pinned_copy(np.full((g + 63) // 64, ~np.uint64(0), np.uint64))
    for mode in (RI.SAFE, RI.LEASE):
        with _engine(S, s, None, x, mode=mode, cls=WireEngine) as e:
            out, peer_off = pinned_empty(e.respond_cap(2 * g), np.uint8), pinned_empty(n + 1, np.uint64)
            resp_off = pinned_empty(2 * g * (n - 1) + 1, np.uint64)
            _, _, outs, got, _, po, _, rc = e.step_frames_respond(pinned_copy(stream), pinned_copy(off), pinned_empty(2 * g, WIRE_MSG_DT), pinned_empty(4, WIRE_ENT_DT),
                                                                  at_tail, out, resp_off, peer_off)
            a, b = outs[:g], outs[g:]
            if mode == RI.SAFE:
                assert np.array_equal(a["type"], np.choose(kind, [S.OUT_HEARTBEAT_RESP, S.OUT_HEARTBEAT_RESP, S.OUT_READ_STATE, S.OUT_FORWARD, S.OUT_READ_INDEX, S.OUT_PROGRESS]))
                assert ((a["flags"][kind == 5] & S.OUTF_READ_READY) != 0).all() and (a["log_term"][kind == 5] == 1).all()
            assert np.array_equal((a["flags"] & ANSWERED) != 0, kind < 2)
            # behind a read result the group's heartbeat is the host's to answer; behind READ_READY nothing ended (a leader's
            # MsgHeartbeatResp asks for nothing either way)
            assert np.array_equal((b["flags"] & ANSWERED) != 0, kind < 2)
            assert np.array_equal(a["index"][kind < 2], ctx[kind < 2]) and np.array_equal(b["index"][kind < 2], ctx[kind < 2] + np.uint64(1))
            # the frames: one slice, peer 2's, in result order
            answered = np.concatenate([np.flatnonzero(kind < 2), g + np.flatnonzero(kind < 2)])
            host = np.zeros(len(answered), W.WIRE_MSG_DT)
            host["group"], host["to"], host["from"], host["term"], host["type"] = w["group"][answered], 2, me, term, R.MsgHeartbeatResp
            host["index"] = w["index"][answered]
            want_bytes, _ = W.wire_encode(host, np.zeros(0, W.WIRE_ENT_DT), np.zeros(1, np.uint8))
            assert int(rc.n_msgs) == len(answered) and bytes(got) == want_bytes.tobytes(), mode
            assert po.tolist() == [0, 0, 0, len(answered)]  # frame indices: peer 2's slice holds them all


# ---- three nodes -------------------------------------------------------------------------------------------------------------------
def _mirror(S, c):
    """three handles on one device behind a ref_read_index.Cluster: every Tick and every Step batch of the reference is made on the
    node's handle too, and all of the handle is held to the reference after each"""
    es = [_engine(S, c.s[k], None, c.x[k], c.mode, c.pre_vote, c.lead_transfer, election_tick=c.et, heartbeat_tick=c.ht, seed=c.seed + k) for k in range(c.N)]

    def on_tick(k, act):
        n_hup, n_beat = es[k].tick()
        assert (n_hup, n_beat) == (int((act == 1).sum()), int((act == 2).sum())), (c.rounds, k)
        g_act, g_el, g_role = es[k].read_tick()
        assert np.array_equal(g_act, act) and np.array_equal(g_el, c.s[k].elapsed) and np.array_equal(g_role, c.s[k].role), (c.rounds, k)

    def on_step(k, batch, outs):
        got, _ = es[k].step_batch(batch)
        _same_records(got, outs, batch, (c.rounds, k))
        _same_after(es[k], (c.s[k], c.x[k]), None, c.mode, c.lead_transfer, (c.rounds, k))

    c.on_tick, c.on_step = on_tick, on_step
    return es


@pytest.mark.parametrize("mode", [RI.SAFE, RI.LEASE], ids=["safe", "lease"])
def test_three_nodes(S, mode):
    from tests import test_read_index_ref as TR

    for scenario, modes in TR.SCENARIOS.items():
        if mode not in modes:
            continue
        c = RI.Cluster(TR.G_SCENARIO, True, mode=mode, **TR.CLUSTER_KW)
        es = _mirror(S, c)
        try:
            scenario(c)
        finally:
            for e in es:
                e.close()


# ---- the switch off, and what the switch closes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [_pick(n=(3, 0), self_peer=(0, 0), masks=(False, False)), _pick(n=(9, 0), self_peer=(8, 0), masks=(True, False))], ids=RI.case_id)
def test_step_switch_off_twin(S, kw):
    """with the switch off a batch holding type 15 or 16 fails and applies nothing, and the case stripped of the two kinds is
    byte-identical between a handle that had the switch on and off again and one that never heard of it -- a heartbeat's context is
    then not looked at and not echoed"""
    start, voters, m, _, _ = _case(_key(kw))
    sw = dict(RI.case_switches(kw), mode=0)
    m = np.array(m)
    plain = m[~np.isin(m["type"], NEW_KINDS)]
    assert len(plain) < len(m)
    ref = RI.copy_start(start)
    ref[1].seq[:], ref[1].acked[:] = 0, 0
    want = RI.step_batch(ref[0], voters, ref[1], plain, **sw)
    assert (want["index"][want["type"] == S.OUT_HEARTBEAT_RESP] == 0).all() and ((want["flags"] & S.OUTF_READ_READY) == 0).all()
    got = []
    for touched in (True, False):
        with _engine(S, start[0], voters, start[1], **sw) as e:
            if touched:
                e.set_read_index(READ_SAFE)
                e.set_read_index(0)
                assert _code(e.step_batch, m)[0] == RAFTQ_EINVAL
                _same_after(e, (start[0], start[1]), voters, 0, sw["lead_transfer"], "a failed batch applies nothing")
            out, _ = e.step_batch(plain)
            _same_records(out, want, plain, (kw, "switch off", touched))
            _same_after(e, ref, voters, 0, sw["lead_transfer"], (kw, "switch off", touched))
            got.append(out.tobytes())
    assert got[0] == got[1]


def test_refusals_and_argument_checks(S):
    from oracle import pywire as W
    from raftsql_amd import _lib
    from raftsql_amd.engine import pinned_empty
    from raftsql_amd.wire import WireEngine

    g, n = 100, 3
    with WireEngine(g, n, 1) as e:
        for mode in (READ_SAFE, READ_LEASE):
            code, text = _code(e.set_read_index, mode)  # without CheckQuorum
            assert code == RAFTQ_ESTATE and "check quorum" in text
        e.set_read_index(0)  # (off is off)
        seq, acked = np.zeros(g, np.uint32), np.zeros((n, g), np.uint32)
        for f in (lambda: e.load_reads(seq, acked), e.read_reads):
            code, text = _code(f)
            assert code == RAFTQ_ESTATE and "read index" in text
        e.set_timers(10, 1, 1)
        e.set_check_quorum(True)
        assert _code(e.read_reads)[0] == RAFTQ_ESTATE  # CheckQuorum alone does not open them
        for bad in (3, -1):
            assert _code(e.set_read_index, bad)[0] == RAFTQ_EINVAL
        e.set_read_index(READ_LEASE)
        assert _code(e.read_reads)[0] == RAFTQ_ESTATE and _code(e.load_reads, seq, acked)[0] == RAFTQ_ESTATE  # the lease mode holds none
        code, text = _code(e.set_check_quorum, False)  # CheckQuorum turned off under it
        assert code == RAFTQ_ESTATE and "read index" in text
        # the lease mode closes nothing
        out, po = pinned_empty(e.respond_cap(g), np.uint8), pinned_empty(n + 1, np.uint64)
        e.set_tick_checks(g)
        e.tick_frames(out, None, po, g)
        e.set_read_index(READ_SAFE)
        e.set_read_index(READ_SAFE)
        for sw in (e.set_pre_vote, e.set_lead_transfer):  # independent of both: on and off beside it
            sw(True)
            sw(False)
        # the closed Tick calls
        before = e.read_tick()
        code, text = _code(e.tick_frames, out, None, po, g)
        assert code == RAFTQ_ESTATE and "read index" in text and "raftq_tick_frames" in text
        counts, nh, nb = _lib.WireCounts(), C.c_uint64(0), C.c_uint64(0)
        assert e._lib.raftq_tick_elect_frames(e._h, 0, g, g, C.byref(nh), C.byref(nb), None, out.ctypes.data, len(out), None, po.ctypes.data,
                                              C.byref(counts)) == RAFTQ_ESTATE
        text = e._lib.raftq_last_error(e._h).decode()
        assert "read index" in text and "raftq_tick_elect_frames" in text
        after = e.read_tick()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))  # a refused call has not ticked
        # the bulk calls
        seq[:] = np.arange(g) + 3
        acked[:] = (np.arange(g)[None, :] + np.arange(n)[:, None]) % 4
        e.load_reads(seq, acked)
        s2, a2, c2 = e.read_reads()
        assert np.array_equal(s2, seq) and np.array_equal(a2, acked) and np.array_equal(c2, np.sort(acked, axis=0)[n - 2])  # q = 2 of 3
        bad = acked.copy()
        bad[2, g - 1] = seq[g - 1] + 1
        assert _code(e.load_reads, None, bad)[0] == RAFTQ_EINVAL  # above the seq that stands
        low = seq.copy()
        low[0] = 0
        assert _code(e.load_reads, low, None)[0] == RAFTQ_EINVAL  # ... and a seq below the words that stand
        s2, a2, _ = e.read_reads()
        assert np.array_equal(s2, seq) and np.array_equal(a2, acked)  # nothing loaded
        e.load_reads(None, acked[::-1].copy() % 3)
        assert np.array_equal(e.read_reads()[1], acked[::-1] % 3) and np.array_equal(e.read_reads()[0], seq)
        # the clone copies the records where both handles hold them -- never the switch
        with WireEngine(g, n, 1) as d:
            d.set_timers(10, 1, 1)
            d.set_check_quorum(True)
            d.clone_state_from(e)
            assert _code(d.read_reads)[0] == RAFTQ_ESTATE
            d.set_read_index(READ_SAFE)
            assert (d.read_reads()[0] == 0).all()
            d.clone_state_from(e)
            assert np.array_equal(d.read_reads()[0], seq) and np.array_equal(d.read_reads()[1], acked[::-1] % 3)
        # a batch in flight
        e.step_submit(S.pack_msgs(np.arange(4, dtype=np.uint64), S.MSG_HUP))
        assert _code(e.set_read_index, 0)[0] == RAFTQ_ESTATE and _code(e.load_reads, seq, None)[0] == RAFTQ_ESTATE
        e.step_collect()
        # every change of mode zeroes the records
        e.set_read_index(READ_LEASE)
        e.set_read_index(READ_SAFE)
        assert all((a == 0).all() for a in e.read_reads())
        e.set_read_index(0)
        e.set_check_quorum(False)
    for name, args in (("raftq_set_read_index", (None, 1)), ("raftq_load_reads", (None, None, None)), ("raftq_read_reads", (None, None, None, None))):
        assert getattr(_lib.load(), name)(*args) == RAFTQ_EINVAL  # NULL handle
