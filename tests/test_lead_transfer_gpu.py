"""GPU: leadership transfer (raftq_set_lead_transfer; the rules in NodeT::step of every *_cq_* walk, the two kinds in classify() and in
the frames calls' filter, the transferee nibble of the activity word) against tests/ref_lead_transfer.py: every result byte, every
word of state, the activity arrays and the transferees.

Step shapes (the issue's): G = 194 groups -- a partial wave --, batches of 512 records, N in {3, 5, 9}, self in the first and in the
last slot, over every slot and over voter masks, PreVote on and off.  N = 9 with self 0 transfers to slot 8 (nibble 9 beside activity
bit 8, 32-bit vote words); lead_elapsed = 65535 stands beside a pending transferee; a batch with 40 records of one group (more than
kMaxRun = 32: the sorted walk) holds a MsgTransferLeader, the completing ack and a MsgProp; a one-voter masked group becomes leader
on MsgTimeoutNow.  What each Step input shows of the feature is asserted on the reference alone by tests/test_lead_transfer_ref.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle
from raftsql_amd._lib import RAFTQ_EINVAL, RAFTQ_ESTATE
from raftsql_amd.engine import RaftqError
from tests import _stepgen
from tests import ref_check_quorum as Q
from tests import ref_lead_transfer as T
from tests import ref_pre_vote as PV
from tests import ref_raft_py as R
from tests import ref_step_props as P
from tests import ref_step_voters as V

pytestmark = pytest.mark.gpu

CASES = T.case_list()
HOT = [c for c in CASES if c.get("hot")]
SEED = 0x5EED
ANSWERED = 0x10
NEW_KINDS = (T.MsgTransferLeader, T.MsgTimeoutNow)


def _pick(**kw):
    """the first case of the list with these arguments"""
    return next(c for c in CASES if all(c.get(k, d) == v for k, (v, d) in kw.items()))


@pytest.fixture(scope="module")
def S(gpu_engine_cls):
    from raftsql_amd import step

    return step


@functools.lru_cache(maxsize=None)
def _case(key):
    return T.step_case(**dict(key))


def _key(kw):
    return tuple(sorted(kw.items()))


def _pv(kw):
    return kw.get("pre_vote", True)


def _engine(S, s, voters, active, lead_elapsed, transferee=None, pre_vote=True, lead_transfer=True, cls=None, election_tick=Q.ELECTION_TICK,
            heartbeat_tick=1, seed=SEED):
    e = (cls or S.NodeEngine)(s.G, s.N, s.self_peer)
    e.set_timers(election_tick, heartbeat_tick, seed)
    e.set_check_quorum(True)
    e.set_step_props(True)
    if pre_vote:
        e.set_pre_vote(True)
    if lead_transfer:
        e.set_lead_transfer(True)
    _stepgen.load_engine(e, s)
    if voters is not None:
        e.load_voters(voters)
        e.set_step_voters(True)
    e.load_activity(active, lead_elapsed)
    if transferee is not None:
        e.load_transfer(transferee)
    return e


def _same_records(got, want, msgs, what=""):
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        k = got.dtype.itemsize
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, k) != want.view(np.uint8).reshape(-1, k)).any(axis=1))
        assert False, (what, len(bad), int(bad[0]), None if msgs is None else msgs[bad[0]], got[bad[0]], want[bad[0]])


def _same_after(e, after, what="", transfer=True):
    s, active, lead_elapsed, transferee = after
    _stepgen.assert_same_state(e, s)
    a, le = e.read_activity()
    assert np.array_equal(a, active), (what, "active")
    assert np.array_equal(le, lead_elapsed), (what, "lead_elapsed")
    if transfer:
        assert np.array_equal(e.read_transfer(), transferee), (what, "transferee")


def _code(f, *args, **kw):
    with pytest.raises(RaftqError) as ei:
        f(*args, **kw)
    return ei.value.code, str(ei.value)


# ---- Step --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CASES, ids=T.case_id)
def test_step_batch_against_the_reference(S, kw):
    start, voters, m, want, after = _case(_key(kw))
    with _engine(S, start[0], voters, start[1], start[2], start[3], _pv(kw)) as e:
        got, _ = e.step_batch(np.array(m))
        _same_records(got, want, m, kw)
        _same_after(e, after, kw)


def test_the_shapes_at_which_the_kernel_can_go_wrong():
    """what the issue names, read off the cases' own inputs and the reference's results"""
    kw = _pick(n=(9, 0), self_peer=(0, 0), masks=(False, False))
    start, _, m, want, after = _case(_key(kw))
    top = (after[3] == 9) & ((after[1] >> 8) & 1 == 1)
    assert top.sum() >= 4  # nibble 9 beside activity bit 8
    assert ((start[2] == 65535) & (start[3] != 0)).sum() >= 4 and ((after[2] == 65535) & (after[3] != 0)).sum() >= 4
    for kw in HOT:
        start, _, m, want, _ = _case(_key(kw))
        grp = np.bincount(m["group"].astype(np.int64)).argmax()
        mine = m["group"] == grp
        assert mine.sum() > 32 and np.isin((T.MsgTransferLeader, R.MsgAppResp, P.MsgProp), m["type"][mine]).all()
        assert ((want["flags"][mine] & T.FlagTimeoutNow) != 0).any() and (want["type"][mine] == T.OutTransfer).any()
    kw = _pick(n=(3, 0), masks=(True, False))
    start, voters, m, want, _ = _case(_key(kw))
    one = (voters[m["group"].astype(np.int64)] == 1 << start[0].self_peer) & (m["type"] == T.MsgTimeoutNow)
    assert (want["type"][one] == R.OutBecameLeader).sum() >= 4


@pytest.mark.parametrize("kw", [_pick(n=(3, 0), masks=(False, False), pre_vote=(True, True)), _pick(n=(9, 0), self_peer=(0, 0), masks=(True, False), pre_vote=(False, True)),
                                HOT[0], _pick(band=("top", None), masks=(True, False))], ids=T.case_id)
def test_step_packed_records_and_result_formats(S, kw):
    """the 40-byte inbound record takes types 13 and 14 and a MsgVote's mark; the three result formats say the same (a packed record
    carries no RAFTQ_MSGF_*, so no MsgProp: the batch goes without them)"""
    start, voters, m, _, _ = _case(_key(kw))
    m = np.array(m)
    m40 = S.pack_msgs40(m[m["type"] != P.MsgProp])
    m = np.zeros(len(m40), S.MSG_DT)
    for k in ("group", "from", "type", "reject", "term", "index", "commit"):
        m[k] = m40[k]
    hint = m40["type"] == S.MSG_APP_RESP
    m["log_term"], m["reject_hint"] = np.where(hint, 0, m40["aux"]), np.where(hint, m40["aux"], 0)
    after = T.copy_start(start)
    want, _ = T.step_batch(after[0], voters, after[1], after[2], after[3], m, _pv(kw))
    assert np.isin((S.OUT_TRANSFER, S.OUT_CAMPAIGN, S.OUT_FORWARD), want["type"]).all()
    assert ((want["flags"] & S.OUTF_TIMEOUT_NOW) != 0).any() and ((want["type"] == S.OUT_CAMPAIGN) & (want["reject"] == 1)).any()
    for fmt in (0, 1, 2):
        with _engine(S, start[0], voters, start[1], start[2], start[3], _pv(kw)) as e:
            e.set_compact(fmt)
            e.step_submit_packed(m40)
            recs, _ = e.step_collect()
            if fmt == 0:
                got = recs
            elif fmt == 1:
                got = S.expand_compact(np.array(m), recs)
            else:
                got = S.expand_short(np.array(m), recs, start[0].last_index, start[0].committed)
            _same_records(got, want, m, (kw, fmt))
            _same_after(e, after, (kw, fmt))


@pytest.mark.parametrize("walk", ["lists", "sort"])
def test_step_both_walks(S, monkeypatch, walk):
    """a batch with 40 records of one group takes the sorted walk by itself; RAFTQ_STEP_WALK=sort sends every batch there"""
    if walk == "sort":
        monkeypatch.setenv("RAFTQ_STEP_WALK", "sort")
    else:
        monkeypatch.delenv("RAFTQ_STEP_WALK", raising=False)
    for kw in HOT + [_pick(band=("b32", None), masks=(True, False))]:
        start, voters, m, want, after = _case(_key(kw))
        assert not kw.get("hot") or np.bincount(m["group"].astype(np.int64)).max() > 32
        with _engine(S, start[0], voters, start[1], start[2], start[3], _pv(kw)) as e:
            got, _ = e.step_batch(np.array(m))
            _same_records(got, want, m, (kw, walk))
            _same_after(e, after, (kw, walk))


def _leaders(S, n, me, g, behind=3):
    """g led groups at term 4 with a log of 9 entries; every peer at the tail but the last one, `behind` entries back"""
    s = pyoracle.NodeState(g, n, me)
    s.term[:], s.vote[:], s.lead[:], s.role[:], s.last_index[:], s.last_term[:], s.first_idx[:] = 4, me + 1, me + 1, 2, 9, 4, 1
    s.match[:] = 9
    t = max(p for p in range(n) if p != me)
    s.match[t] = 9 - behind
    return s, t


def test_pipelined_transfer_across_two_batches(S):
    """submit / collect: the MsgTransferLeader in one batch, the completing ack in the batch in flight behind it -- the second walk
    sees the nibble the first one wrote"""
    n, me, g = 5, 0, 64
    s, t = _leaders(S, n, me, g)
    ac, le, tr = np.zeros(g, np.uint16), np.full(g, 7, np.uint32), np.zeros(g, np.uint8)
    grp = np.arange(g, dtype=np.uint64)
    b1 = S.pack_msgs(grp, S.MSG_TRANSFER_LEADER, frm=t)
    b2 = np.concatenate([S.pack_msgs(grp[::2], S.MSG_APP_RESP, term=4, frm=t, index=9), S.pack_msgs(grp[1::2], S.MSG_APP_RESP, term=4, frm=t, index=8)])
    start = (V.copy_state(s), ac.copy(), le.copy(), tr.copy())
    w1, _ = T.step_batch(s, None, ac, le, tr, b1)
    w2, _ = T.step_batch(s, None, ac, le, tr, b2)
    assert (w1["type"] == S.OUT_TRANSFER).all() and (w1["flags"] == 0).all() and (w1["index"] == 6).all() and (le == 0).all() and (tr == t + 1).all()
    assert np.array_equal((w2["flags"] & S.OUTF_TIMEOUT_NOW) != 0, np.arange(g) < g // 2) and ((w2["flags"] & S.OUTF_UPDATED) != 0).all()
    with _engine(S, start[0], None, start[1], start[2], start[3]) as e:
        e.step_submit(b1)
        e.step_submit(b2)
        assert _code(e.set_lead_transfer, False)[0] == RAFTQ_ESTATE  # a batch in flight
        g1, _ = e.step_collect()
        g2, _ = e.step_collect()
        _same_records(g1, w1, b1, "first batch")
        _same_records(g2, w2, b2, "second batch")
        _same_after(e, (s, ac, le, tr), "pipelined")


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def _node_filter(wm, we, g, n, me):
    """ref_step_props.node_filter (raftq_step_set_props is on) with what the header says the switch changes: frames of types 13 and
    14 are kinds a peer sends, checked as MsgVoteResp is and flagged as little"""
    plain = wm.copy()
    plain["type"] = np.where(np.isin(wm["type"], NEW_KINDS), R.MsgVoteResp, wm["type"])
    out, rec = P.node_filter(plain, we, g, n, me, True, True)
    out["type"] = rec["type"] = wm["type"]
    return out, rec


@pytest.mark.parametrize("kw", [_pick(n=(3, 0), self_peer=(2, 0), masks=(False, False), pre_vote=(True, True)),
                                _pick(n=(9, 0), self_peer=(0, 0), masks=(True, False), pre_vote=(False, True)), _pick(band=("b63", None), masks=(False, False))],
                         ids=T.case_id)
def test_step_frames_and_packed(S, kw):
    """raftq_step_frames and raftq_step_frames_packed over a stream holding frames of types 13 and 14 among the usual kinds: the
    decoded records against the codec oracle (the filter's flags restated), results and state against the reference"""
    from oracle import pywire as W
    from raftsql_amd import wire
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from tests import packed_rule

    start, voters, m, _, _ = _case(_key(kw))
    s0, me = start[0], start[0].self_peer
    stream, off = P.frames_of(np.random.default_rng(77), np.array(m), me, empty_props=0.0)
    wm, we, bad = W.wire_decode(stream, off)
    assert bad == 0 and np.isin(wm["type"], NEW_KINDS).sum() >= 40
    want_m, rec = _node_filter(wm, we, s0.G, s0.N, me)
    new = np.isin(want_m["type"], NEW_KINDS)
    assert ((want_m["flags"][new] & V.MSGF_SKIP) == 0).all() and ((want_m["flags"] & V.MSGF_SKIP) != 0).any()  # (the local kinds are nobody's)
    after = T.copy_start(start)
    want_o, _ = T.step_batch(after[0], voters, after[1], after[2], after[3], rec, _pv(kw))
    assert np.isin((S.OUT_TRANSFER, S.OUT_CAMPAIGN, S.OUT_FORWARD), want_o["type"]).all() and ((want_o["flags"] & S.OUTF_TIMEOUT_NOW) != 0).any()
    n = len(wm)
    ps, po = pinned_copy(np.ascontiguousarray(stream)), pinned_copy(np.ascontiguousarray(off, np.uint64))
    with _engine(S, s0, voters, start[1], start[2], start[3], _pv(kw), cls=wire.WireEngine) as e:
        gm, ge, go, c = e.step_frames(ps, po, pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT))
        assert (c.n_msgs, c.n_ents, c.n_malformed, c.bytes) == (n, len(we), 0, len(stream))
        _same_records(gm, want_m, None, "records")
        _same_records(ge, we, None, "entry headers")
        _same_records(go, want_o, rec, "results")
        _same_after(e, after, "frames")
    for form in (packed_rule.FORM_40, packed_rule.FORM_HEAD):
        ht = packed_rule.RESPONSE_KINDS if form == packed_rule.FORM_HEAD else 0
        want_narrow, want_wide = packed_rule.pack(want_m, me, form, ht)
        with _engine(S, s0, voters, start[1], start[2], start[3], _pv(kw), cls=wire.WireEngine) as e:
            narrow, wide, ge, go, c, n_wide = e.step_frames_packed(ps, po, form, pinned_empty(n, wire._FORM_DT[form]), pinned_empty(len(want_wide) + 1, W.WIRE_MSG_DT),
                                                                   pinned_empty(len(we) + 1, W.WIRE_ENT_DT), head_types=ht)
            assert n_wide == len(want_wide)
            _same_records(narrow, want_narrow, None, ("narrow", form))
            _same_records(wide, want_wide, None, ("wide", form))
            _same_records(go, want_o, rec, ("results", form))
            _same_after(e, after, ("packed", form))
    # without the switch the two kinds stay frames of a kind a peer never sends
    with _engine(S, s0, voters, start[1], start[2], None, _pv(kw), lead_transfer=False, cls=wire.WireEngine) as e:
        gm, _, go, _ = e.step_frames(ps, po, pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT))
        assert ((gm["flags"][new] & V.MSGF_SKIP) != 0).all() and (go["type"][new] == V.OutSkipped).all()


def test_step_submit_wire_takes_the_two_kinds(S):
    from oracle import pywire as W
    from raftsql_amd.wire import WireEngine

    n, me, g = 3, 1, 32
    s = pyoracle.NodeState(g, n, me)
    s.term[:], s.last_index[:], s.last_term[:] = 4, 6, 4
    s.match[me] = 6
    s.role[:g // 2], s.lead[:g // 2], s.vote[:g // 2], s.first_idx[:g // 2] = 2, me + 1, me + 1, 1
    s.match[:, :g // 2] = 6
    s.lead[g // 2:] = 1
    w = np.zeros(g, W.WIRE_MSG_DT)
    w["group"], w["to"], w["from"], w["term"] = np.arange(g), me, 0, 4
    w["type"] = np.where(np.arange(g) < g // 2, T.MsgTransferLeader, T.MsgTimeoutNow)
    stream, off = W.wire_encode(w, np.zeros(0, W.WIRE_ENT_DT), np.zeros(1, np.uint8))
    rec = np.zeros(g, S.MSG_DT)
    for k in ("group", "term", "log_term", "index", "from", "type"):
        rec[k] = w[k]
    ac, le, tr = np.zeros(g, np.uint16), np.zeros(g, np.uint32), np.zeros(g, np.uint8)
    want, _ = T.step_batch(s_after := V.copy_state(s), None, ac, le, tr, rec)
    assert (want["type"][:g // 2] == S.OUT_TRANSFER).all() and ((want["flags"][:g // 2] & S.OUTF_TIMEOUT_NOW) != 0).all()
    assert (want["type"][g // 2:] == S.OUT_CAMPAIGN).all() and (want["reject"][g // 2:] == 1).all() and (want["term"][g // 2:] == 5).all()
    zeros = (np.zeros(g, np.uint16), np.zeros(g, np.uint32))
    with _engine(S, s, None, *zeros, cls=WireEngine) as e:
        e.step_submit_wire(stream, off)
        got, _ = e.step_collect()
        _same_records(got, want, rec, "submit_wire")
        _same_after(e, (s_after, ac, le, tr), "submit_wire")
    with _engine(S, s, None, *zeros, lead_transfer=False, cls=WireEngine) as e:
        e.step_submit_wire(stream, off)
        assert _code(e.step_collect)[0] == RAFTQ_EINVAL  # an unknown kind fails its batch


def test_frames_respond_leaves_the_new_results_to_the_host(S):
    """RAFTQ_OUT_TRANSFER, a forwarded MsgTransferLeader and a campaign from MsgTimeoutNow carry no RAFTQ_OUTF_ANSWERED and end their
    group's device-answered prefix; a committing ack from the pending transferee is answered -- its commit broadcast built -- AND
    carries RAFTQ_OUTF_TIMEOUT_NOW"""
    from oracle import pywire as W
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from raftsql_amd.wire import WIRE_ENT_DT, WIRE_MSG_DT, WireEngine

    n, me, g = 3, 1, 32
    s = pyoracle.NodeState(g, n, me)
    s.term[:], s.last_index[:], s.last_term[:] = 4, 6, 4
    s.match[me] = 6
    kind = np.arange(g) % 4  # 0: led, a MsgTransferLeader; 1: led with the transfer pending, the committing ack; 2, 3: following, 13 / 14
    led = kind < 2
    s.role[led], s.lead[led], s.vote[led], s.first_idx[led] = 2, me + 1, me + 1, 1
    s.lead[~led] = 3
    s.match[0, led], s.match[2, led], s.committed[:] = 3, 3, 3
    tr = np.where(kind == 1, 1, 0).astype(np.uint8)
    first = np.zeros(g, W.WIRE_MSG_DT)
    first["group"], first["to"], first["from"], first["term"] = np.arange(g), me, 0, 4
    first["type"] = np.choose(kind, [T.MsgTransferLeader, R.MsgAppResp, T.MsgTransferLeader, T.MsgTimeoutNow])
    first["index"] = np.where(kind == 1, 6, 0)
    second = np.zeros(g, W.WIRE_MSG_DT)  # a heartbeat response (leaders) / the leader's heartbeat (followers): answered while the prefix lasts
    second["group"], second["to"], second["from"], second["term"] = np.arange(g), me, 2, 4
    second["type"] = np.where(led, R.MsgHeartbeatResp, R.MsgHeartbeat)
    w = np.concatenate([first, second])
    stream, off = W.wire_encode(w, np.zeros(0, W.WIRE_ENT_DT), np.zeros(1, np.uint8))
    at_tail = pinned_copy(np.full((g + 63) // 64, ~np.uint64(0), np.uint64))
    with _engine(S, s, None, np.zeros(g, np.uint16), np.zeros(g, np.uint32), tr, cls=WireEngine) as e:
        out, peer_off = pinned_empty(e.respond_cap(2 * g), np.uint8), pinned_empty(n + 1, np.uint64)
        resp_off = pinned_empty(2 * g * (n - 1) + 1, np.uint64)
        _, _, outs, _, _, _, _, rc = e.step_frames_respond(pinned_copy(stream), pinned_copy(off), pinned_empty(2 * g, WIRE_MSG_DT), pinned_empty(4, WIRE_ENT_DT),
                                                           at_tail, out, resp_off, peer_off)
        a, b = outs[:g], outs[g:]
        assert np.array_equal(a["type"], np.choose(kind, [S.OUT_TRANSFER, S.OUT_PROGRESS, S.OUT_FORWARD, S.OUT_CAMPAIGN]))
        assert np.array_equal((a["flags"] & ANSWERED) != 0, kind == 1)
        ack = a[kind == 1]
        want_flags = S.OUTF_TIMEOUT_NOW | S.OUTF_UPDATED | S.OUTF_COMMITTED | S.OUTF_HARDSTATE | ANSWERED
        assert (ack["flags"] == want_flags).all() and (ack["commit"] == 6).all() and (ack["index"] == 6).all()
        assert (a["reject"][kind == 3] == 1).all() and (a["to"][kind == 2] == 2).all() and (a["index"][kind == 0] == 3).all()
        # behind the host's results nothing is the device's; behind the answered ack the heartbeat response asks for nothing
        assert ((b["flags"] & ANSWERED) == 0).all()
        assert int(rc.n_msgs) == int((kind == 1).sum()) * (n - 1)  # the commit broadcasts: one empty MsgApp to every peer but self
        assert np.array_equal(e.read_transfer(), np.where(led, 1, 0))


# ---- the Tick ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,me,masks", [(3, 0, False), (9, 8, True)])
def test_tick_aborts_a_transfer_at_the_election_timeout(S, oracle, n, me, masks):
    """raftq_tick x election_tick, and the same through raftq_tick_collect_lists under raftq_tick_set_checks, from leaders with pending
    transferees and staggered lead_elapsed: transferee, activity and action bytes against the reference after every Tick -- no Tick
    kernel knows the nibble, the word's layout does the work"""
    g, et, ht = 1500, 7, 2
    role, elapsed, active, lead_elapsed, transferee, voters = T.tick_input(g, n, me, et, 10600 + n, masks)
    assert ((transferee != 0) & (role == 2)).sum() > g // 4
    s = pyoracle.NodeState(g, n, me)
    s.role[:], s.elapsed[:] = role, elapsed
    s.lead[:] = np.where(role == 2, me + 1, 0)
    aborted = 0
    engines = []
    try:
        for fused in (False, True):
            e = _engine(S, s, None, active, lead_elapsed, transferee, election_tick=et, heartbeat_tick=ht)
            engines.append(e)
            if masks:
                e.load_voters(voters)
                e.set_tick_voters(True)
            if fused:
                e.set_tick_checks(g)
        el, ac, le, tr = elapsed.copy(), active.copy(), lead_elapsed.copy(), transferee.copy()
        for t in range(et):
            el, act, ac, le, tr2, n_hup, n_beat = T.tick(oracle, role, el, ac, le, tr, voters, me, n, et, ht, SEED, t)
            aborted += int(((tr != 0) & (tr2 == 0)).sum())
            tr = tr2
            assert engines[0].tick() == (n_hup, n_beat), t
            hups, nh, _, nb = engines[1].tick_collect_lists()
            chk, n_chk = engines[1].last_tick_checks()
            assert (nh, nb, n_chk) == (n_hup, n_beat, int((act == 3).sum())) and np.array_equal(chk, np.flatnonzero(act == 3)), t
            for e in engines:
                g_act, g_el, _ = e.read_tick()
                assert np.array_equal(g_act, act) and np.array_equal(g_el, el), t
                a, l = e.read_activity()
                assert np.array_equal(a, ac) and np.array_equal(l, le) and np.array_equal(e.read_transfer(), tr), t
        assert aborted > g // 16 and (tr != 0).any()  # (a failing check keeps the transferee until its MsgCheckQuorum is stepped)
    finally:
        for e in engines:
            e.close()


# ---- three nodes -------------------------------------------------------------------------------------------------------------------
def _mirror(S, c):
    """three handles on one device behind a ref_lead_transfer.Cluster: every Tick and every Step batch of the reference is made on
    the node's handle too, the host carrying results across as records, and all of the handle is held to the reference after each"""
    es = [_engine(S, c.s[k], None, c.active[k], c.lead_elapsed[k], c.transferee[k], c.pre_vote, election_tick=c.et, heartbeat_tick=c.ht, seed=c.seed + k)
          for k in range(c.N)]

    def on_tick(k, act):
        n_hup, n_beat = es[k].tick()
        assert (n_hup, n_beat) == (int((act == 1).sum()), int((act == 2).sum())), (c.rounds, k)
        g_act, g_el, g_role = es[k].read_tick()
        assert np.array_equal(g_act, act) and np.array_equal(g_el, c.s[k].elapsed) and np.array_equal(g_role, c.s[k].role), (c.rounds, k)
        assert np.array_equal(es[k].read_transfer(), c.transferee[k]), (c.rounds, k)

    def on_step(k, batch, outs):
        got, _ = es[k].step_batch(batch)
        _same_records(got, outs, batch, (c.rounds, k))
        _same_after(es[k], (c.s[k], c.active[k], c.lead_elapsed[k], c.transferee[k]), (c.rounds, k))

    c.on_tick, c.on_step = on_tick, on_step
    return es


@pytest.mark.parametrize("pre_vote", [False, True])
def test_three_nodes_transfer_completes_and_is_aborted(S, pre_vote):
    from tests import test_lead_transfer_ref as TR

    for scenario in (TR.completing, TR.aborted):
        c = T.Cluster(TR.G_SCENARIO, pre_vote, **TR.CLUSTER_KW[scenario.__name__])
        es = _mirror(S, c)
        try:
            scenario(c)
        finally:
            for e in es:
                e.close()


# ---- the switch off, and what the switch closes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CASES, ids=T.case_id)
def test_step_switch_off_twin(S, kw):
    """with the switch off a batch holding type 13 or 14 fails and applies nothing, a marked MsgVote is lease-ignored exactly as an
    unmarked one, and every case stripped of the two kinds is byte-identical between a handle whose switch is on and one that never
    heard of it (and what the references without the feature say)"""
    start, voters, m, _, _ = _case(_key(kw))
    m = np.array(m)
    plain = m[~np.isin(m["type"], NEW_KINDS)]
    unmarked = plain.copy()
    unmarked["reject"][unmarked["type"] == R.MsgVote] = 0
    assert len(plain) < len(m) and ((plain["type"] == R.MsgVote) & (plain["reject"] == 1)).any()
    no_tr = np.zeros(start[0].G, np.uint8)  # (without the two kinds nothing sets a transferee, so none is loaded)
    ref = T.copy_start(start)
    ref[3][:] = 0
    want, _ = T.step_batch(ref[0], voters, ref[1], ref[2], ref[3], unmarked, _pv(kw))
    assert (ref[3] == 0).all()
    got = []
    for touched in (True, False):
        with _engine(S, start[0], voters, start[1], start[2], None, _pv(kw), lead_transfer=False) as e:
            if touched:
                e.set_lead_transfer(True)
                e.set_lead_transfer(False)
                assert _code(e.step_batch, m)[0] == RAFTQ_EINVAL
                _same_after(e, (start[0], start[1], start[2], no_tr), "a failed batch applies nothing", transfer=False)
            out, _ = e.step_batch(plain)
            _same_records(out, want, plain, (kw, "switch off", touched))  # the marks change nothing
            _same_after(e, ref, (kw, "switch off", touched), transfer=False)
            got.append(out.tobytes())
    assert got[0] == got[1]
    # ... and with the switch on and no transfer anywhere, the unmarked traffic gives the same bytes
    with _engine(S, start[0], voters, start[1], start[2], no_tr, _pv(kw)) as e:
        out, _ = e.step_batch(unmarked)
        assert out.tobytes() == got[0], kw
        _same_after(e, ref, (kw, "switch on"))
    on = T.copy_start(start)
    on[3][:] = 0
    assert want.tobytes() != T.step_batch(on[0], voters, on[1], on[2], on[3], plain, _pv(kw))[0].tobytes()  # (the marks matter under the switch)


def test_refusals_and_argument_checks(S):
    from raftsql_amd import _lib
    from raftsql_amd.wire import WireEngine

    g, n = 100, 3
    with WireEngine(g, n, 1) as e:
        lib, h = e._lib, e._h
        code, text = _code(e.set_lead_transfer, True)  # without CheckQuorum
        assert code == RAFTQ_ESTATE and "check quorum" in text
        e.set_lead_transfer(False)  # (off is off)
        tr = np.zeros(g, np.uint8)
        for f in (lambda: e.load_transfer(tr), e.read_transfer):
            code, text = _code(f)
            assert code == RAFTQ_ESTATE and "lead transfer" in text
        e.set_timers(10, 1, 1)
        e.set_check_quorum(True)
        assert _code(e.read_transfer)[0] == RAFTQ_ESTATE  # CheckQuorum alone does not open them
        for bad in (2, -1):
            assert _code(e.set_lead_transfer, bad)[0] == RAFTQ_EINVAL
        e.set_lead_transfer(True)
        e.set_lead_transfer(True)
        code, text = _code(e.set_check_quorum, False)  # CheckQuorum turned off under it
        assert code == RAFTQ_ESTATE and "lead transfer" in text
        e.set_pre_vote(True)  # independent of PreVote: on and off beside it
        e.set_pre_vote(False)
        # the bulk calls
        tr[:] = np.arange(g) % (n + 1)
        active, le = (np.arange(g) % 8).astype(np.uint16), (65535 - np.arange(g)).astype(np.uint32)
        e.load_activity(active, le)
        e.load_transfer(tr)
        assert np.array_equal(e.read_transfer(), tr)
        a, l = e.read_activity()
        assert np.array_equal(a, active) and np.array_equal(l, le)  # read_activity never shows a transferee
        bad = tr.copy()
        bad[g - 1] = n + 1
        code, text = _code(e.load_transfer, bad)
        assert code == RAFTQ_EINVAL and np.array_equal(e.read_transfer(), tr)  # nothing loaded
        e.load_activity(active[::-1].copy(), None)  # load_activity preserves a transferee
        assert np.array_equal(e.read_transfer(), tr) and np.array_equal(e.read_activity()[0], active[::-1]) and np.array_equal(e.read_activity()[1], le)
        word = active.copy()
        word[3] |= 1 << 12
        assert _code(e.load_activity, word, None)[0] == RAFTQ_EINVAL  # its "slot >= n_peers" check stays as it is
        assert np.array_equal(e.read_transfer(), tr) and np.array_equal(e.read_activity()[0], active[::-1])
        # raftq_propose_frames is closed, and a refused call applies nothing
        before = e.read_node()
        counts = _lib.WireCounts()
        assert lib.raftq_propose_frames(h, None, 1, None, 0, None, 0, None, 0, None, 0, None, 0, None, C.byref(counts)) == RAFTQ_ESTATE
        text = lib.raftq_last_error(h).decode()
        assert "lead transfer" in text and "raftq_propose_frames" in text
        after = e.read_node()
        assert all(np.array_equal(before[k], after[k]) for k in before)
        assert np.array_equal(e.read_transfer(), tr)
        # the clone copies the word -- the transferee travels with it -- never the switch
        with WireEngine(g, n, 1) as d:
            d.set_timers(10, 1, 1)
            d.set_check_quorum(True)
            d.clone_state_from(e)
            assert _code(d.read_transfer)[0] == RAFTQ_ESTATE
            a, l = d.read_activity()
            assert np.array_equal(a, active[::-1]) and np.array_equal(l, le)
            d.set_lead_transfer(True)
            assert np.array_equal(d.read_transfer(), tr)
        # a batch in flight
        e.step_submit(S.pack_msgs(np.arange(4, dtype=np.uint64), S.MSG_HUP))
        assert _code(e.set_lead_transfer, False)[0] == RAFTQ_ESTATE
        e.step_collect()
        # turning it off clears every transferee and nothing else
        a0, l0 = e.read_activity()
        e.set_lead_transfer(False)
        e.set_lead_transfer(True)
        assert (e.read_transfer() == 0).all()
        a1, l1 = e.read_activity()
        assert np.array_equal(a0, a1) and np.array_equal(l0, l1)
        e.set_lead_transfer(False)
        e.set_check_quorum(False)
    for name, args in (("raftq_set_lead_transfer", (None, 1)), ("raftq_load_transfer", (None, None)), ("raftq_read_transfer", (None, None))):
        assert getattr(_lib.load(), name)(*args) == RAFTQ_EINVAL  # NULL handle
