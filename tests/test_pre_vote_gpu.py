"""GPU: PreVote (raftq_set_pre_vote; the five rules in NodeT::step of every *_cq_* walk, the two kinds in classify() and in the
frames calls' filter) against tests/ref_pre_vote.py: every result byte, every word of state, the activity arrays.

Step shapes (the issue's): G = 194 groups -- a partial wave --, batches of 512 records, N in {1, 3, 5, 9}, self in {0, N - 1}, over
every slot and over voter masks; a batch with 40 records of one group (more than kMaxRun = 32: the sorted walk).  What each Step
input shows of the feature -- each of the five rules -- is asserted on the reference alone by tests/test_pre_vote_ref.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle
from raftsql_amd._lib import RAFTQ_EINVAL, RAFTQ_ESTATE
from raftsql_amd.engine import RaftqError
from tests import _stepgen
from tests import ref_check_quorum as Q
from tests import ref_pre_vote as PV
from tests import ref_raft_py as R
from tests import ref_step_props as P
from tests import ref_step_voters as V

pytestmark = pytest.mark.gpu

CASES = PV.case_list()
SEED = 0x5EED
ANSWERED = 0x10
_ids = lambda kw: "-".join(str(v) for v in kw.values())  # noqa: E731


def _band(band, masks=False):
    """the band case (64-bit terms and indices, tests/_widegen.py) of the list with this band"""
    return next(c for c in CASES if c.get("band") == band and bool(c.get("masks")) == masks)


@pytest.fixture(scope="module")
def S(gpu_engine_cls):
    from raftsql_amd import step

    return step


@functools.lru_cache(maxsize=None)
def _case(key):
    return PV.step_case(**dict(key))


def _key(kw):
    return tuple(sorted(kw.items()))


def _engine(S, s, voters, active, lead_elapsed, pre_vote=True, cls=None, election_tick=Q.ELECTION_TICK, heartbeat_tick=1, seed=SEED):
    """both switches go on in front of the load: raftq_load_roles takes role 3 only under raftq_set_pre_vote"""
    e = (cls or S.NodeEngine)(s.G, s.N, s.self_peer)
    e.set_timers(election_tick, heartbeat_tick, seed)
    e.set_check_quorum(True)
    if pre_vote:
        e.set_pre_vote(True)
    _stepgen.load_engine(e, s)
    if voters is not None:
        e.load_voters(voters)
        e.set_step_voters(True)
    e.load_activity(active, lead_elapsed)
    return e


def _same_records(got, want, msgs, what=""):
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        k = got.dtype.itemsize
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, k) != want.view(np.uint8).reshape(-1, k)).any(axis=1))
        assert False, (what, len(bad), int(bad[0]), None if msgs is None else msgs[bad[0]], got[bad[0]], want[bad[0]])


def _same_after(e, after, what=""):
    s, active, lead_elapsed = after
    _stepgen.assert_same_state(e, s)
    a, le = e.read_activity()
    assert np.array_equal(a, active), (what, "active")
    assert np.array_equal(le, lead_elapsed), (what, "lead_elapsed")


def _code(f, *args, **kw):
    with pytest.raises(RaftqError) as ei:
        f(*args, **kw)
    return ei.value.code, str(ei.value)


# ---- Step --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", CASES, ids=_ids)
def test_step_batch_against_the_reference(S, kw):
    start, voters, m, want, after = _case(_key(kw))
    with _engine(S, start[0], voters, start[1], start[2]) as e:
        got, _ = e.step_batch(np.array(m))
        _same_records(got, want, m, kw)
        _same_after(e, after, kw)


@pytest.mark.parametrize("kw", [CASES[2], CASES[7], CASES[8], _band("b63", masks=True)], ids=_ids)
def test_step_packed_records_and_result_formats(S, kw):
    """the 40-byte inbound record takes types 17 and 18 with MsgVote's fields; the three result formats say the same"""
    start, voters, m, _, _ = _case(_key(kw))
    m40 = S.pack_msgs40(np.array(m))
    # what the device widens them to (include/raftq_step.h: a packed record carries no RAFTQ_MSGF_*, no count, one of log_term / reject_hint)
    m = np.zeros(len(m40), S.MSG_DT)
    for k in ("group", "from", "type", "reject", "term", "index", "commit"):
        m[k] = m40[k]
    hint = m40["type"] == S.MSG_APP_RESP
    m["log_term"], m["reject_hint"] = np.where(hint, 0, m40["aux"]), np.where(hint, m40["aux"], 0)
    after = (V.copy_state(start[0]), start[1].copy(), start[2].copy())
    want = PV.step_batch(after[0], voters, after[1], after[2], m)
    assert np.isin((S.OUT_PRE_CAMPAIGN, S.OUT_PRE_VOTE_RESP, S.OUT_TERM_RESP, S.OUT_CAMPAIGN), want["type"]).all()
    assert (want["log_term"][want["type"] == S.OUT_PRE_CAMPAIGN] != 0).any()  # (what the compact records have to carry)
    for fmt in (0, 1, 2):
        with _engine(S, start[0], voters, start[1], start[2]) as e:
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
    for kw in (CASES[8], CASES[9], _band("top", masks=True)):
        start, voters, m, want, after = _case(_key(kw))
        assert not kw.get("hot") or np.bincount(m["group"].astype(np.int64)).max() > 32
        with _engine(S, start[0], voters, start[1], start[2]) as e:
            got, _ = e.step_batch(np.array(m))
            _same_records(got, want, m, (kw, walk))
            _same_after(e, after, (kw, walk))


def test_pipelined_pre_election_across_two_batches(S):
    """submit / collect: MsgHup in one batch, the grants in the batch in flight behind it -- the second walk sees role 3 and the
    vote word the first one wrote"""
    n, me, g = 3, 0, 64
    s = pyoracle.NodeState(g, n, me)
    s.term[:], s.last_index[:], s.last_term[:] = 4, 9, 4
    s.match[me] = 9
    ac, le = np.zeros(g, np.uint16), np.zeros(g, np.uint32)
    grp = np.arange(g, dtype=np.uint64)
    b1 = S.pack_msgs(grp, S.MSG_HUP)
    b2 = np.concatenate([S.pack_msgs(grp[::2], S.MSG_PRE_VOTE_RESP, term=5, frm=1), S.pack_msgs(grp[1::2], S.MSG_PRE_VOTE_RESP, term=4, frm=2, reject=1)])
    start = (V.copy_state(s), ac.copy(), le.copy())
    w1 = PV.step_batch(s, None, ac, le, b1)
    w2 = PV.step_batch(s, None, ac, le, b2)
    assert (w1["type"] == S.OUT_PRE_CAMPAIGN).all() and (w1["term"] == 4).all() and (w1["flags"] == 0).all()
    assert (w2["type"][:g // 2] == S.OUT_CAMPAIGN).all() and (w2["term"][:g // 2] == 5).all() and (w2["role"][g // 2:] == S.ROLE_PRE_CANDIDATE).all()
    with _engine(S, start[0], None, start[1], start[2]) as e:
        e.step_submit(b1)
        e.step_submit(b2)
        assert _code(e.set_pre_vote, False)[0] == RAFTQ_ESTATE  # a batch in flight
        g1, _ = e.step_collect()
        g2, _ = e.step_collect()
        _same_records(g1, w1, b1, "first batch")
        _same_records(g2, w2, b2, "second batch")
        _same_after(e, (s, ac, le), "pipelined")


# ---- frames ------------------------------------------------------------------------------------------------------------------------
def _node_filter(wm, we, g, n, me):
    """tests/test_wire_gpu._node_filter with what the header says the switch changes: frames of types 17 and 18 are kinds a peer
    sends, checked as MsgVote / MsgVoteResp are and flagged as little"""
    from tests.test_wire_gpu import _node_filter as plain

    as_votes = wm.copy()
    as_votes["type"] = np.where(wm["type"] == PV.MsgPreVote, R.MsgVote, np.where(wm["type"] == PV.MsgPreVoteResp, R.MsgVoteResp, wm["type"]))
    out, rec = plain(as_votes, we, g, n, me, True)
    out["type"] = rec["type"] = wm["type"]
    return out, rec


@pytest.mark.parametrize("kw", [CASES[2], CASES[5], CASES[8], _band("b32")], ids=_ids)
def test_step_frames_and_packed(S, kw):
    """raftq_step_frames and raftq_step_frames_packed over a stream holding frames of types 17 and 18 among the usual kinds: the
    decoded records against the codec oracle (the filter's flags restated), results and state against the reference"""
    from oracle import pywire as W
    from raftsql_amd import wire
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from tests import packed_rule

    start, voters, m, _, _ = _case(_key(kw))
    s0, me = start[0], start[0].self_peer
    stream, off = P.frames_of(np.random.default_rng(77), np.array(m), me)
    wm, we, bad = W.wire_decode(stream, off)
    assert bad == 0 and np.isin(wm["type"], (PV.MsgPreVote, PV.MsgPreVoteResp)).sum() >= 40
    want_m, rec = _node_filter(wm, we, s0.G, s0.N, me)
    new = np.isin(want_m["type"], (PV.MsgPreVote, PV.MsgPreVoteResp))
    assert ((want_m["flags"][new] & V.MSGF_SKIP) == 0).all() and ((want_m["flags"] & V.MSGF_SKIP) != 0).any()  # (the local kinds are nobody's)
    after = (V.copy_state(s0), start[1].copy(), start[2].copy())
    want_o = PV.step_batch(after[0], voters, after[1], after[2], rec)
    assert np.isin((S.OUT_PRE_VOTE_RESP, S.OUT_TERM_RESP), want_o["type"]).all()  # (a MsgHup is no frame: pre-elections start in the caller's own records)
    n = len(wm)
    ps, po = pinned_copy(np.ascontiguousarray(stream)), pinned_copy(np.ascontiguousarray(off, np.uint64))
    with _engine(S, s0, voters, start[1], start[2], cls=wire.WireEngine) as e:
        gm, ge, go, c = e.step_frames(ps, po, pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT))
        assert (c.n_msgs, c.n_ents, c.n_malformed, c.bytes) == (n, len(we), 0, len(stream))
        _same_records(gm, want_m, None, "records")
        _same_records(ge, we, None, "entry headers")
        _same_records(go, want_o, rec, "results")
        _same_after(e, after, "frames")
    for form in (packed_rule.FORM_40, packed_rule.FORM_HEAD):
        ht = packed_rule.RESPONSE_KINDS if form == packed_rule.FORM_HEAD else 0
        want_narrow, want_wide = packed_rule.pack(want_m, me, form, ht)
        with _engine(S, s0, voters, start[1], start[2], cls=wire.WireEngine) as e:
            narrow, wide, ge, go, c, n_wide = e.step_frames_packed(ps, po, form, pinned_empty(n, wire._FORM_DT[form]), pinned_empty(len(want_wide) + 1, W.WIRE_MSG_DT),
                                                                   pinned_empty(len(we) + 1, W.WIRE_ENT_DT), head_types=ht)
            assert n_wide == len(want_wide)
            _same_records(narrow, want_narrow, None, ("narrow", form))
            _same_records(wide, want_wide, None, ("wide", form))
            _same_records(go, want_o, rec, ("results", form))
            _same_after(e, after, ("packed", form))
    # without the switch the two kinds stay frames of a kind a peer never sends
    with _engine(S, _no_role3(s0), voters, start[1], start[2], pre_vote=False, cls=wire.WireEngine) as e:
        gm, _, go, _ = e.step_frames(ps, po, pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT))
        assert ((gm["flags"][new] & V.MSGF_SKIP) != 0).all() and (go["type"][new] == V.OutSkipped).all()


def test_step_submit_wire_takes_the_two_kinds(S):
    from oracle import pywire as W
    from raftsql_amd.wire import WireEngine

    n, me, g = 3, 1, 32
    s = pyoracle.NodeState(g, n, me)
    s.term[:], s.last_index[:], s.last_term[:] = 4, 6, 4
    s.match[me] = 6
    s.role[g // 2:] = PV.PRE
    s.votes[me, g // 2:] = 1
    w = np.zeros(g, W.WIRE_MSG_DT)
    w["group"], w["to"], w["from"], w["term"], w["index"], w["log_term"] = np.arange(g), me, 0, 5, 9, 5
    w["type"] = np.where(np.arange(g) < g // 2, PV.MsgPreVote, PV.MsgPreVoteResp)
    stream, off = W.wire_encode(w, np.zeros(0, W.WIRE_ENT_DT), np.zeros(1, np.uint8))
    rec = np.zeros(g, S.MSG_DT)
    for k in ("group", "term", "log_term", "index", "from", "type"):
        rec[k] = w[k]
    ac, le = np.zeros(g, np.uint16), np.zeros(g, np.uint32)
    want = PV.step_batch(s_after := V.copy_state(s), None, ac, le, rec)
    assert (want["type"][:g // 2] == S.OUT_PRE_VOTE_RESP).all() and (want["type"][g // 2:] == S.OUT_CAMPAIGN).all()
    with _engine(S, s, None, np.zeros(g, np.uint16), np.zeros(g, np.uint32), cls=WireEngine) as e:
        e.step_submit_wire(stream, off)
        got, _ = e.step_collect()
        _same_records(got, want, rec, "submit_wire")
        _same_after(e, (s_after, ac, le), "submit_wire")
    with _engine(S, _no_role3(s), None, np.zeros(g, np.uint16), np.zeros(g, np.uint32), pre_vote=False, cls=WireEngine) as e:
        e.step_submit_wire(stream, off)
        assert _code(e.step_collect)[0] == RAFTQ_EINVAL  # an unknown kind fails its batch


def test_frames_respond_leaves_the_new_results_to_the_host(S):
    """RAFTQ_OUT_PRE_VOTE_RESP and RAFTQ_OUT_TERM_RESP carry no RAFTQ_OUTF_ANSWERED and end their group's device-answered prefix; a
    lease-ignored MsgPreVote builds no frame and does not end it"""
    from oracle import pywire as W
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from raftsql_amd.wire import WIRE_ENT_DT, WIRE_MSG_DT, WireEngine

    n, me, g = 3, 1, 24
    s = pyoracle.NodeState(g, n, me)
    s.term[:], s.lead[:], s.last_index[:], s.last_term[:] = 4, 3, 6, 4
    s.match[me] = 6
    kind = np.arange(g) % 3  # 0: in lease, a MsgPreVote; 1: out of lease, a MsgPreVote; 2: a stale MsgHeartbeat
    s.elapsed[:] = np.where(kind == 1, Q.ELECTION_TICK + 1, 0)
    first = np.zeros(g, W.WIRE_MSG_DT)
    first["group"], first["to"], first["from"] = np.arange(g), me, 0
    first["type"] = np.where(kind == 2, R.MsgHeartbeat, PV.MsgPreVote)
    first["term"] = np.where(kind == 2, 3, 5)
    first["index"], first["log_term"] = np.where(kind == 2, 0, 9), np.where(kind == 2, 0, 5)
    second = np.zeros(g, W.WIRE_MSG_DT)  # the leader's heartbeat: answered on the device while the prefix lasts
    second["group"], second["to"], second["from"], second["type"], second["term"] = np.arange(g), me, 2, R.MsgHeartbeat, 4
    w = np.concatenate([first, second])
    stream, off = W.wire_encode(w, np.zeros(0, W.WIRE_ENT_DT), np.zeros(1, np.uint8))
    with _engine(S, s, None, np.zeros(g, np.uint16), np.zeros(g, np.uint32), cls=WireEngine) as e:
        out, peer_off = pinned_empty(e.respond_cap(2 * g), np.uint8), pinned_empty(n + 1, np.uint64)
        resp_off = pinned_empty(2 * g * (n - 1) + 1, np.uint64)
        _, _, outs, _, _, _, _, rc = e.step_frames_respond(pinned_copy(stream), pinned_copy(off), pinned_empty(2 * g, WIRE_MSG_DT), pinned_empty(4, WIRE_ENT_DT),
                                                           None, out, resp_off, peer_off)
        a, b = outs[:g], outs[g:]
        assert np.array_equal(a["type"], np.choose(kind, [S.OUT_NONE, S.OUT_PRE_VOTE_RESP, S.OUT_TERM_RESP]))
        assert np.array_equal(a["index"], np.choose(kind, [0, 5, 0])) and (a["reject"] == 0).all() and (a["term"] == 4).all()
        assert ((a["flags"] & ANSWERED) == 0).all()
        assert (b["type"] == S.OUT_HEARTBEAT_RESP).all()
        assert np.array_equal((b["flags"] & ANSWERED) != 0, kind == 0)  # only behind the ignored MsgPreVote is the group still the device's
        assert int(rc.n_msgs) == int((kind == 0).sum())


# ---- three nodes -------------------------------------------------------------------------------------------------------------------
def _mirror(S, c):
    """three handles on one device behind a ref_pre_vote.Cluster: every Tick and every Step batch of the reference is made on the
    node's handle too, the host carrying results across as records, and all of the handle is held to the reference after each"""
    es = [_engine(S, c.s[k], None, c.active[k], c.lead_elapsed[k], election_tick=c.et, heartbeat_tick=c.ht, seed=c.seed + k) for k in range(c.N)]

    def on_tick(k, act):
        n_hup, n_beat = es[k].tick()
        assert (n_hup, n_beat) == (int((act == 1).sum()), int((act == 2).sum())), (c.rounds, k)
        g_act, g_el, g_role = es[k].read_tick()
        assert np.array_equal(g_act, act) and np.array_equal(g_el, c.s[k].elapsed) and np.array_equal(g_role, c.s[k].role), (c.rounds, k)

    def on_step(k, batch, outs):
        got, _ = es[k].step_batch(batch)
        _same_records(got, outs, batch, (c.rounds, k))
        _same_after(es[k], (c.s[k], c.active[k], c.lead_elapsed[k]), (c.rounds, k))

    c.on_tick, c.on_step = on_tick, on_step
    return es


def _close(es):
    for e in es:
        e.close()


def test_three_nodes_cut_off_and_healed(S):
    from tests.test_pre_vote_ref import G_SCENARIO, HEAL_ROUNDS

    c = PV.Cluster(G_SCENARIO, True)
    es = _mirror(S, c)
    try:
        c.run(2)
        c.cut = {2}
        c.run(3 * 2 * c.et)
        assert (c.s[2].term == 1).all() and (c.s[2].role == PV.PRE).all()
        c.cut = set()
        c.run(HEAL_ROUNDS)
        assert c.converged() and (c.s[0].role == 2).all() and (c.s[0].term == 1).all() and (c.s[2].lead == 1).all()
        assert np.array_equal(es[2].read_node()["lead"], np.ones(G_SCENARIO, np.uint32))  # (on the handle, too)
    finally:
        _close(es)


def test_three_nodes_inflated_term(S):
    from tests.test_pre_vote_ref import G_SCENARIO, INFLATED_ROUNDS

    c = PV.Cluster(G_SCENARIO, True)
    c.s[2].term[:], c.s[2].lead[:], c.s[2].vote[:] = 7, 0, 0
    es = _mirror(S, c)
    try:
        c.run(INFLATED_ROUNDS)
        assert c.converged() and (np.stack([s.term for s in c.s]).min(axis=0) >= 8).all()
    finally:
        _close(es)


# ---- the switch off, and what the switch closes ------------------------------------------------------------------------------------
def _no_role3(s):
    s = V.copy_state(s)
    s.role[s.role == PV.PRE] = 1
    return s


def test_step_switch_off_twin(S):
    """the same traffic minus the two kinds on a handle whose switch was turned on and off again, and on one that never heard of
    it: byte-identical, and what tests/ref_check_quorum.py says; a record of type 17 fails its batch and applies nothing"""
    start, voters, m, want, after = _case(_key(CASES[2]))
    m = np.array(m)
    plain = m[~np.isin(m["type"], (PV.MsgPreVote, PV.MsgPreVoteResp))]
    s0 = _no_role3(start[0])
    ref = (V.copy_state(s0), start[1].copy(), start[2].copy())
    want_plain = Q.step_batch(ref[0], None, ref[1], ref[2], plain)
    got = []
    for touched in (True, False):
        with _engine(S, s0, None, start[1], start[2], pre_vote=False) as e:
            if touched:
                e.set_pre_vote(True)
                e.set_pre_vote(False)
                code, _ = _code(e.step_batch, m)
                assert code == RAFTQ_EINVAL
                _same_after(e, (s0, start[1], start[2]), "a failed batch applies nothing")
            out, _ = e.step_batch(plain)
            _same_records(out, want_plain, plain, ("switch off", touched))
            _same_after(e, ref, ("switch off", touched))
            got.append(out.tobytes())
    assert got[0] == got[1]
    on = (V.copy_state(s0), start[1].copy(), start[2].copy())
    assert want_plain.tobytes() != PV.step_batch(on[0], None, on[1], on[2], plain).tobytes()  # (the switch matters here)


def test_refusals_and_argument_checks(S):
    from raftsql_amd import _lib

    g, n = 100, 3
    with S.NodeEngine(g, n, 1) as e:
        lib, h = e._lib, e._h
        code, text = _code(e.set_pre_vote, True)  # without CheckQuorum
        assert code == RAFTQ_ESTATE and "check quorum" in text
        e.set_pre_vote(False)  # (off is off)
        roles = np.zeros(g, np.uint8)
        roles[7] = 3
        code, text = _code(e.load_roles, roles)  # role 3, switch off: the error it always was
        assert code == RAFTQ_EINVAL and "role must be 0, 1 or 2" in text
        e.set_timers(10, 1, 1)
        e.set_check_quorum(True)
        assert _code(e.load_roles, roles)[0] == RAFTQ_EINVAL  # CheckQuorum alone does not open it
        for bad in (2, -1):
            assert _code(e.set_pre_vote, bad)[0] == RAFTQ_EINVAL
        e.set_pre_vote(True)
        e.set_pre_vote(True)
        e.load_roles(roles)
        assert e.read_tick()[2][7] == 3
        roles[8] = 4
        assert _code(e.load_roles, roles)[0] == RAFTQ_EINVAL
        code, text = _code(e.set_check_quorum, False)  # CheckQuorum turned off under it
        assert code == RAFTQ_ESTATE and "pre vote" in text
        e.read_activity()  # (the state is still there)
        nh, nb = C.c_uint64(0), C.c_uint64(0)
        po = (C.c_uint64 * 16)()
        before = e.read_tick()
        assert lib.raftq_tick_elect_frames(h, 0, 0, 0, C.byref(nh), C.byref(nb), None, None, 0, None, po, None) == RAFTQ_ESTATE
        text = lib.raftq_last_error(h).decode()
        assert "pre vote" in text and "raftq_tick_elect_frames" in text
        for x, y in zip(before, e.read_tick()):
            assert np.array_equal(x, y)  # it did not tick
        # role 3 ticks as a follower does: its election timer runs
        e.load_roles(np.full(g, 3, np.uint8), np.full(g, 25, np.uint32))
        assert e.tick() == (g, 0)
        # the clone copies state, never the switch
        with S.NodeEngine(g, n, 1) as d:
            d.clone_state_from(e)
            assert _code(d.load_roles, roles[:g] * 0 + 3)[0] == RAFTQ_EINVAL
        # a batch in flight
        e.step_submit(S.pack_msgs(np.arange(4, dtype=np.uint64), S.MSG_HUP))
        assert _code(e.set_pre_vote, False)[0] == RAFTQ_ESTATE
        e.step_collect()
        # turning it off leaves a role-3 group as it is, and a Step without the switch takes it for a follower without a leader
        e.set_pre_vote(False)
        assert (e.read_tick()[2] == 3).all()
        got, _ = e.step_batch(S.pack_msgs(np.arange(2, dtype=np.uint64), S.MSG_VOTE, term=9, frm=0, index=99, log_term=9))
        assert (got["type"] == S.OUT_VOTE_RESP).all() and (got["reject"] == 0).all() and (got["role"] == 0).all()
        e.set_check_quorum(False)
    assert _lib.load().raftq_set_pre_vote(None, 1) == RAFTQ_EINVAL  # NULL handle
