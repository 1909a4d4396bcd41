"""GPU: Step takes forwarded proposals (raftq_step_set_props; the MsgProp arm of NodeT::step in every walk kernel, the frames
filter's flag, respond()'s two host-owned results) against tests/ref_step_props.py: every result byte and every word of state.

Shapes (the issue's): G = 97 groups, batches of 512 records, N in {1, 3, 5, 9}; a batch with 40 records of one group (more than
kMaxRun = 32: the list walk stalls and the sorted walk replays); one frames call with G = 32,768 and 65,536 frames (every tile
path).  What each batch shows of the feature is asserted on the reference alone by tests/test_step_props_ref.py."""
import functools

import numpy as np
import pytest

from oracle import pywire as W
from raftsql_amd._lib import RAFTQ_EINVAL, RAFTQ_ESTATE
from raftsql_amd.engine import RaftqError
from tests import _stepgen
from tests import packed_rule
from tests import ref_raft_py as R
from tests import ref_step_props as P
from tests import ref_step_voters as V

pytestmark = pytest.mark.gpu

CASES, FRAMES = P.case_list()
ANSWERED = 0x10
_ids = lambda kw: "-".join(str(v) for v in kw.values())  # noqa: E731


@pytest.fixture(scope="module")
def S(gpu_engine_cls):
    from raftsql_amd import step

    return step


@functools.lru_cache(maxsize=None)
def _case(key):
    return P.case(**dict(key))


@functools.lru_cache(maxsize=None)
def _frames_case(key):
    return P.frames_case(**dict(key))


def _key(kw):
    return tuple(sorted(kw.items()))


def _engine(S, s, voters=None, props=True, cls=None, **kw):
    e = (cls or S.NodeEngine)(s.G, s.N, s.self_peer, **kw)
    _stepgen.load_engine(e, s)
    if voters is not None:
        e.load_voters(voters)
        e.set_step_voters(True)
    if props:
        e.set_step_props(True)
    return e


def _same_records(got, want, msgs, what=""):
    assert got.dtype.itemsize == want.dtype.itemsize and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        k = got.dtype.itemsize
        bad = np.flatnonzero((got.view(np.uint8).reshape(-1, k) != want.view(np.uint8).reshape(-1, k)).any(axis=1))
        assert False, (what, len(bad), int(bad[0]), msgs[bad[0]] if msgs is not None else None, got[bad[0]], want[bad[0]])


def _code(f, *args, **kw):
    with pytest.raises(RaftqError) as ei:
        f(*args, **kw)
    return ei.value.code


def _walk(monkeypatch, walk):
    if walk == "sort":
        monkeypatch.setenv("RAFTQ_STEP_WALK", "sort")
    else:
        monkeypatch.delenv("RAFTQ_STEP_WALK", raising=False)


# ---- parity: both walks, the three result formats, plain / hot / masked / wide ---------------------------------------------------
@pytest.mark.parametrize("compact", [0, 1, 2], ids=["64-byte-results", "40-byte-results", "32-byte-results"])
@pytest.mark.parametrize("walk", ["lists", "sort"])
@pytest.mark.parametrize("kw", CASES, ids=_ids)
def test_parity(S, kw, walk, compact, monkeypatch):
    _walk(monkeypatch, walk)
    start, voters, m, want, after = _case(_key(kw))
    with _engine(S, start, voters) as e:
        e.set_compact(compact)
        if compact:
            e.step_submit(m)
            recs, touched = e.step_collect()
            got = S.expand_compact(m, recs) if compact == 1 else S.expand_short(m, recs, start.last_index, start.committed)
        else:
            got, touched = e.step_batch(m)
        assert touched == len(np.unique(m["group"]))
        _same_records(got, want, m, (kw, walk, compact))
        _stepgen.assert_same_state(e, after)


def test_three_batches_in_flight_the_second_one_stalls(S):
    """nothing of the stalled batch nor of the one behind it is applied by the list walk; the collect replays both, in order,
    through the sorted walk -- proposals moving the tail in all three"""
    kw = dict(n=5, self_peer=4, seed=9310 + 5, hot=True)
    start, _, hot, _, _ = _case(_key(kw))
    s = V.copy_state(start)
    rng = np.random.default_rng(9400)
    batches = [P.props_batch(rng, s), hot, P.props_batch(rng, s)]
    want = [P.step_batch(s, None, m) for m in batches]
    with _engine(S, start) as e:
        for m in batches:
            e.step_submit(m)
        assert _code(e.set_step_props, False) == RAFTQ_ESTATE  # a batch in flight
        for m, w in zip(batches, want):
            got, _ = e.step_collect()
            _same_records(got, w, m)
        _stepgen.assert_same_state(e, s)


@pytest.mark.parametrize("walk", ["lists", "sort"])
def test_hand_table(S, walk, monkeypatch):
    from tests.test_step_props_ref import check_table, table_batch

    _walk(monkeypatch, walk)
    s, m, want = table_batch()
    with _engine(S, s) as e:
        got, _ = e.step_batch(m)
        check_table(got, want)
        _same_records(got, P.step_batch(s, None, m), m)
        _stepgen.assert_same_state(e, s)


# ---- masked groups ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,self_peer", [(3, 0), (5, 4), (9, 8)])
def test_masked_one_voter_leader_commits_and_a_leader_that_does_not_vote(S, n, self_peer):
    rng = np.random.default_rng(9450 + n)
    s = P.props_state(rng, n, self_peer)
    led = np.flatnonzero(s.role == 2)
    s.first_idx[led] = 1  # (the gate is open at every index: what commits is the quorum's to say)
    me = 1 << self_peer
    voters = V.random_masks(rng, n, P.G)
    alone, outside = led[:10], led[10:20]
    voters[alone] = me
    voters[outside] = ((1 << n) - 1) & ~me
    m = np.zeros(len(led), S.MSG_DT)
    for i, g in enumerate(led):
        P._prop(m, i, g, 1 + i % P.MAX_ENTS, frm=(self_peer + 1) % n)
    start = V.copy_state(s)
    want = P.step_batch(s, voters, m)
    assert (want["type"] == P.OutProposed).all()
    committed = (want["flags"] & R.FlagCommitted) != 0
    assert committed[:10].all() and np.array_equal(want["commit"][:10], want["last_index"][:10])  # its own quorum
    assert (want["commit"][10:20] < want["index"][10:20]).all()  # a non-voting leader's new entries wait for the voters
    with _engine(S, start, voters) as e:
        got, _ = e.step_batch(m)
        _same_records(got, want, m, n)
        _stepgen.assert_same_state(e, s)


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def _pinned_frames(stream, off):
    from raftsql_amd.engine import pinned_copy

    return pinned_copy(np.ascontiguousarray(stream)), pinned_copy(np.ascontiguousarray(off, np.uint64))


def _wire_engine(S, s, props=True):
    from raftsql_amd.wire import WireEngine

    return _engine(S, s, None, props, cls=WireEngine)


@pytest.mark.parametrize("walk", ["lists", "sort"])
@pytest.mark.parametrize("kw", FRAMES, ids=_ids)
def test_step_frames(S, kw, walk, monkeypatch):
    """raftq_step_frames and raftq_step_frames_packed: decoded records and entry headers against the codec oracle (with the
    filter's flags restated), results and state against the reference"""
    from raftsql_amd import wire
    from raftsql_amd.engine import pinned_empty

    _walk(monkeypatch, walk)
    s, stream, off, wm, we, by_switch = _frames_case(_key(kw))
    want_m, rec, want_o, after = by_switch[True]
    n, me = len(wm), s.self_peer
    ps, po = _pinned_frames(stream, off)
    with _wire_engine(S, s) as e:
        gm, ge, go, c = e.step_frames(ps, po, pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT))
        assert (c.n_msgs, c.n_ents, c.n_malformed, c.bytes) == (n, len(we), 0, len(stream))
        _same_records(gm, want_m, None, "records")
        _same_records(ge, we, None, "entry headers")
        _same_records(go, want_o, rec, "results")
        _stepgen.assert_same_state(e, after)
    if walk == "sort":
        return
    for form in (packed_rule.FORM_40, packed_rule.FORM_HEAD):
        ht = packed_rule.RESPONSE_KINDS if form == packed_rule.FORM_HEAD else 0
        want_narrow, want_wide = packed_rule.pack(want_m, me, form, ht)
        props_wide = (want_m["type"] == P.MsgProp) & (want_m["n_ents"] > 0)
        assert props_wide.sum() >= 8 and ((want_narrow["flags"][props_wide] & packed_rule.F_WIDE) != 0).all()  # the log's owner needs the entries
        with _wire_engine(S, s) as e:
            narrow, wide, ge, go, c, n_wide = e.step_frames_packed(ps, po, form, pinned_empty(n, wire._FORM_DT[form]), pinned_empty(len(want_wide) + 1, W.WIRE_MSG_DT),
                                                                   pinned_empty(len(we) + 1, W.WIRE_ENT_DT), head_types=ht)
            assert n_wide == len(want_wide)
            _same_records(narrow, want_narrow, None, ("narrow", form))
            _same_records(wide, want_wide, None, ("wide", form))
            _same_records(ge, we, None, ("entry headers", form))
            _same_records(go, want_o, rec, ("results", form))
            _stepgen.assert_same_state(e, after)


@pytest.mark.parametrize("kw", [kw for kw in FRAMES if kw["n"] > 1], ids=_ids)
def test_step_frames_respond(S, kw):
    """both new results are the host's (no RAFTQ_OUTF_ANSWERED) and nothing is built on the device behind a RAFTQ_OUT_PROPOSED in
    its group; everything else is the restated table of tests/test_respond_gpu.py, which leaves any result type it does not
    know to the host"""
    from raftsql_amd.engine import pinned_copy, pinned_empty
    from tests.test_respond_gpu import _bitmap, expected

    s, stream, off, wm, we, by_switch = _frames_case(_key(kw))
    want_m, rec, want_o, after = by_switch[True]
    n, n_peers, me = len(wm), s.N, s.self_peer
    at_tail = _bitmap(s.G, np.flatnonzero(s.role == 2))
    want_w, want_po, want_ans = expected(rec, want_o, s.last_term.copy(), at_tail, n_peers, me)
    want_s, want_off = W.wire_encode(want_w) if len(want_w) else (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    # the restatement's answers around the new results: none on them, none behind a PROPOSED in its group
    new = np.isin(want_o["type"], (P.OutProposed, P.OutForward))
    assert new.sum() >= 16 and not want_ans[new].any() and want_ans.sum() >= 8
    closed = set()
    behind = np.zeros(n, bool)
    for i in range(n):
        g = int(rec["group"][i])
        behind[i] = g in closed and want_o["type"][i] != V.OutSkipped
        if want_o["type"][i] == P.OutProposed:
            closed.add(g)
    assert behind.sum() >= 8 and not want_ans[behind].any()
    ps, po = _pinned_frames(stream, off)
    with _wire_engine(S, s) as e:
        out = pinned_empty(e.respond_cap(n), np.uint8)
        gm, ge, go, got_s, got_off, got_po, c, rc = e.step_frames_respond(
            ps, po, pinned_empty(n, W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT), pinned_copy(at_tail), out,
            pinned_empty(n * (n_peers - 1) + 1, np.uint64), pinned_empty(n_peers + 1, np.uint64))
        ans = (go["flags"] & ANSWERED) != 0
        assert not ans[new].any() and not ans[behind].any()
        assert np.array_equal(ans, want_ans), np.flatnonzero(ans != want_ans)[:10]
        go = go.copy()
        go["flags"] &= np.uint8(~ANSWERED & 0xFF)
        _same_records(go, want_o, rec, "results")
        _same_records(gm, want_m, None, "records")
        assert np.array_equal(got_po, want_po) and rc.n_msgs == len(want_w)
        assert bytes(got_s) == bytes(want_s) and np.array_equal(got_off, want_off)
        _stepgen.assert_same_state(e, after)


def test_step_frames_at_32768_groups(S):
    """65,536 frames over 32,768 groups: every tile of the decoder and every block of the walks; the whole result array"""
    from raftsql_amd.engine import pinned_empty

    s, stream, off, wm, we, by_switch = _frames_case(_key(P.BIG))
    want_o = by_switch[True][2]
    assert (want_o["type"] == P.OutProposed).sum() > 1000 and (want_o["type"] == P.OutForward).sum() > 1000
    ps, po = _pinned_frames(stream, off)
    with _wire_engine(S, s) as e:
        _, _, go, c = e.step_frames(ps, po, pinned_empty(len(wm), W.WIRE_MSG_DT), None)
        assert c.n_msgs == len(wm)
        _same_records(go, want_o, None, "results")


# ---- atomicity --------------------------------------------------------------------------------------------------------------------
def _spoil(m, what, n_peers):
    bad = m.copy()
    at = int(np.flatnonzero((m["type"] == P.MsgProp) & (m["term"] == 0))[200])  # a well-formed proposal far from the front
    if what == "no RAFTQ_MSGF_ENTRIES":
        bad["_pad"][at][1] = 0
    elif what == "no entries":
        bad["_resv"][at] = np.uint64(5) << np.uint64(32)  # (the high half is not the count in a caller's record)
    else:
        bad["from"][at] = n_peers
    return bad


@pytest.mark.parametrize("walk", ["lists", "sort"])
@pytest.mark.parametrize("what", ["no RAFTQ_MSGF_ENTRIES", "no entries", "from >= N"])
def test_one_malformed_msgprop_fails_the_batch_and_applies_nothing(S, what, walk, monkeypatch):
    _walk(monkeypatch, walk)
    kw = CASES[3]
    start, voters, m, want, after = _case(_key(kw))
    rng = np.random.default_rng(9500)
    m = np.concatenate([m, P.props_batch(rng, start)])  # (so that a proposal number 200 exists)
    bad = _spoil(m, what, start.N)
    assert P.malformed(bad, start.G, start.N).sum() == 1
    with _engine(S, start, voters) as e:
        assert _code(e.step_batch, bad) == RAFTQ_EINVAL
        _stepgen.assert_same_state(e, start)
        e.step_submit(bad)
        assert _code(e.step_collect) == RAFTQ_EINVAL
        _stepgen.assert_same_state(e, start)
        ref = V.copy_state(start)  # ... and the handle steps the good batch afterwards
        _same_records(e.step_batch(m)[0], P.step_batch(ref, voters, m), m)
        _stepgen.assert_same_state(e, ref)


# ---- the switch ---------------------------------------------------------------------------------------------------------------------
def test_switch_off_type_2_is_an_unknown_kind_and_frames_hold_it(S):
    from raftsql_amd.engine import pinned_empty

    kw = CASES[3]
    start, voters, m, want, after = _case(_key(kw))
    only_props = m[m["type"] == P.MsgProp][:1]
    with _engine(S, start, props=False) as e:
        assert _code(e.set_step_props, 2) == RAFTQ_EINVAL and _code(e.set_step_props, -1) == RAFTQ_EINVAL
        for batch in (m, only_props):
            assert _code(e.step_batch, batch) == RAFTQ_EINVAL
            e.step_submit(batch)
            assert _code(e.step_collect) == RAFTQ_EINVAL
        _stepgen.assert_same_state(e, start)
        # on, then off again: as before
        e.set_step_props(True)
        _same_records(e.step_batch(m)[0], want, m)
        _stepgen.assert_same_state(e, after)
        e.set_step_props(False)
        assert _code(e.step_batch, only_props) == RAFTQ_EINVAL
        _stepgen.assert_same_state(e, after)
    # where no flag byte is read the switch changes nothing: a handle without raftq_step_set_msg_flags, the 40-byte inbound
    # record (it carries no count), and a clone's destination (the switch is the handle's, not the state's)
    with _engine(S, start, msg_flags=False) as e, _engine(S, start) as on, _engine(S, start, props=False) as dst:
        assert _code(e.step_batch, only_props) == RAFTQ_EINVAL
        packed = S.pack_msgs40(only_props)
        on.step_submit_packed(packed)
        assert _code(on.step_collect) == RAFTQ_EINVAL
        dst.clone_state_from(on)
        assert _code(dst.step_batch, only_props) == RAFTQ_EINVAL
        for x in (e, on, dst):
            _stepgen.assert_same_state(x, start)
    # the frames calls, switch off: HELD / DEFERRED as ever -- against the reference over the filter the existing suites restate
    for fkw in FRAMES[1:3]:
        s, stream, off, wm, we, by_switch = _frames_case(_key(fkw))
        want_m, rec, want_o, f_after = by_switch[False]
        ps, po = _pinned_frames(stream, off)
        with _wire_engine(S, s, props=False) as e:
            gm, ge, go, c = e.step_frames(ps, po, pinned_empty(len(wm), W.WIRE_MSG_DT), pinned_empty(len(we) + 1, W.WIRE_ENT_DT))
            _same_records(gm, want_m, None, "records, switch off")
            _same_records(go, want_o, rec, "results, switch off")
            assert (go["type"][wm["type"] == P.MsgProp] == V.OutHeld).all()
            _stepgen.assert_same_state(e, f_after)


def test_submit_wire_keeps_type_2_malformed(S):
    """raftq_step_submit_wire's records carry the decoder's flags in their pad bytes, not RAFTQ_MSGF_*: out of the switch's reach"""
    fkw = FRAMES[1]
    s, stream, off, wm, we, _ = _frames_case(_key(fkw))
    i = int(np.flatnonzero((wm["type"] == P.MsgProp) & (wm["n_ents"] > 0))[0])
    one = np.ascontiguousarray(stream[int(off[i]):int(off[i + 1])])
    with _wire_engine(S, s) as e:
        e.step_submit_wire(one, np.array([0, len(one)], np.uint64))
        assert _code(e.step_collect) == RAFTQ_EINVAL
        _stepgen.assert_same_state(e, s)
